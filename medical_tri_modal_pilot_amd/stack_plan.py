"""What a fusion stack node runs, decided in one place: the typed plan of ops.FusionStackFn / ops.MultiTokenStackFn, the per-layer
schedule that their forward walks and their backward walks reversed, and the host pieces the three encoders of mbt_encoder.py
share (block collector, key lengths, gradient placement).  Pure Python over torch and tuning: importable without the HIP library."""
import math
from dataclasses import dataclass
from typing import Any, List, NamedTuple, Optional

import torch

from medical_tri_modal_pilot_amd import tuning

NB = 4                  # bottleneck tokens: the prefix rows of every stream buffer of ops.FusionStackFn
N_PREFIX = 12           # prefix rows of the multi-token stack: three of the four sets of four
PARAMS_PER_LAYER = 14


class LayerStep(NamedTuple):
    """One layer of a stack node's schedule."""
    streams: tuple               # the streams this layer runs
    cls_tok: Optional[int]       # the row a CLS-only last layer computes (ops.layer_forward cls_tok), or None
    ffn_rows: Optional[int]      # the streams other than 0 run their FFN on these first rows only (ops.layer_forward ffn_rows)
    solo: bool                   # one launch group per stream: the inputs are still being made on the side streams
    exchange: bool               # a bottleneck exchange follows this layer


@dataclass(eq=False)
class StackPlan:
    """The last argument of FusionStackFn.apply / MultiTokenStackFn.apply."""
    n_layers: int                # layers of this node
    kv: list                     # per stream int32[B] valid keys (prefix rows included) | None
    missing: Any                 # int64[B]: the samples' rows of the exchange table
    drop_p: float                # dropout probability of every block
    seeds: list                  # seeds[l][m]: the (FFN1, FFN2) dropout seeds of a block
    fused: list                  # fused[l][m]: a block's ops.FusedWeights; None for a block that is not run
    dtype: Any                   # compute dtype of the stream buffers
    vsltonly: int = 0            # 1: the last layer runs stream 0 alone (--mbt-only-vslt)
    resbottle: bool = False      # the exchange adds the previous exchange's result (--residual-bottlenecks)
    n_streams: int = 3           # 2 = the two-stream encoder: xt is None, two blocks per layer, ``missing`` holds table rows 1 / 3
    # this node holds the LAST fusion layers.  The stack may be cut into chained nodes (mbt_encoder.py ``graph_segments``): a
    # non-final node ends with an exchange like every inner layer, returns no CLS vector, and its three output buffers are the
    # next node's prebuilt inputs -- the trainer captures each node's backward in its own hipGraph so that the gradient
    # all-reduce of the later layers overlaps the backward of the earlier ones (ddp.GradReducer, staged mode)
    final: bool = True
    prebuilt: bool = False       # the inputs ARE the [B, 4+N, 256] buffers (ops.StreamInputFn); read, never written
    # the caller reads stream 0's output only (mbt_encoder.py ``first_stream_output_only``): the last layer runs stream 0 alone,
    # exactly like vsltonly == 1 does; the other outputs are zeros without a gradient
    first_only: bool = False
    # the caller never reads rows 0..3 of the outputs (mbt_encoder.py slices them off), so with vsltonly == 0 and no gradient for
    # the image / text outputs the last layer's image / text blocks get no backward at all (the reference: None, not zero)
    bott_rows_unused: bool = False
    cls_only: bool = False       # the reader takes stream 0's CLS row only: a last layer of stream 0 alone computes that one row
    # the layer (index in this node) in front of such a last layer: its image / text outputs feed the exchange (rows 0..3) and
    # nothing else, so their FFN runs on those rows (bf16 and tuning.FFN_ROWS_BEFORE_LAST; the fp32 parity build stays dense)
    exchange_only_layer: int = -1
    inputs_on_side: bool = False  # the image / text inputs are still being made on the side streams when layer 0 starts
    # row_starts(kv[0], N_0) of a PACKED vital-sign stream, made by the encoder together with a packed stream input: bf16 grouped
    # kernels only, and only for a caller that reads nothing of stream 0 but its CLS row
    pack_v: Any = None
    side_streams: Optional[list] = None     # the two extra HIP streams of ops.launch_groups, or None
    sinks: Optional[list] = None            # sinks[l][m]: a block's ops.GradSink | None; None: no gradient goes through a sink
    masks: Optional[list] = None            # multi-token stack: per stream the words of its prefix mask | None
    exchange_last: bool = True   # an exchange follows a last layer that ran every stream (the multi-token node: nothing reads it)
    # the forward is one that nobody differentiates (ops.infer_active() at the call site): the node walks the same schedule with
    # ops.layer_infer, keeps no saved record and no buffer beyond what the next exchange needs, marks its outputs
    # non-differentiable, and its backward raises.  Off by default; never together with dropout
    infer: bool = False

    def __post_init__(self):
        if self.infer and self.drop_p > 0:
            raise ValueError("infer: an inference forward runs without dropout (drop_p must be 0)")
        if not self.final and (not self.prebuilt or self.resbottle):
            raise ValueError("a non-final FusionStackFn segment needs prebuilt inputs and resbottle off")
        if self.pack_v is not None and not (self.prebuilt and self.dtype == torch.bfloat16 and self.kv[0] is not None):
            raise ValueError("a packed vital-sign stream needs prebuilt bf16 inputs with key lengths (ops.StreamInputFn)")
        if not self.final and (self.cls_only or self.first_only):
            raise ValueError("cls_only / first_only apply to a final FusionStackFn segment only")

    def block(self, li: int, m: int) -> slice:
        """where the 14 parameters of layer li, stream m lie in the node's flat argument list (and their gradients in its result)"""
        k = (li * self.n_streams + m) * PARAMS_PER_LAYER
        return slice(k, k + PARAMS_PER_LAYER)

    def sink(self, li: int, m: int):
        return self.sinks[li][m] if self.sinks else None

    def schedule(self) -> List[LayerStep]:
        """What every layer of the node runs; the forward walks it.  (Reads tuning.FFN_ROWS_BEFORE_LAST now, not at import.)"""
        L, steps = self.n_layers, []
        for li in range(L):
            alone = self.final and (self.vsltonly == 1 or self.first_only) and li == L - 1
            rows = li == self.exchange_only_layer and tuning.FFN_ROWS_BEFORE_LAST and self.dtype == torch.bfloat16
            steps.append(LayerStep(streams=(0,) if alone else tuple(range(self.n_streams)),
                                   cls_tok=NB if (alone and self.cls_only) else None, ffn_rows=NB if rows else None,
                                   solo=li == 0 and bool(self.inputs_on_side),
                                   exchange=not alone and (li < L - 1 or self.exchange_last)))
        return steps

    def backward_schedule(self, no_grad_12: bool) -> List[LayerStep]:
        """The schedule the backward walks reversed.  no_grad_12: no gradient arrived for outputs 1 and 2.  vsltonly == 0: the last
        layer ran every stream, but when nothing downstream read the image / text outputs (and nobody reads the exchanged
        bottleneck rows) their blocks have no gradient: its backward runs like the vslt-only one's (the reference's autograd never
        reaches those blocks either)."""
        steps = self.schedule()
        if (self.final and self.vsltonly != 1 and no_grad_12 and self.bott_rows_unused and not self.resbottle
                and len(steps[-1].streams) == self.n_streams):
            steps[-1] = steps[-1]._replace(streams=(0,), exchange=False)
        return steps


def keep_grads(pgrads, pshapes, where: slice, g):
    """a layer's returned gradients (None: they went through its sink) into their places `where` of the node's flat result"""
    if g is not None:
        for k, gk in zip(range(where.start, where.stop), g):
            pgrads[k] = gk.view(pshapes[k])


def zero_streams(shapes, dtype, device):
    """Zero gradient buffers with which the streams a last layer skipped re-enter: ONE fill (views of one allocation)."""
    sizes = [math.prod(s) for s in shapes]
    return [t.view(s) for t, s in zip(torch.zeros(sum(sizes), dtype=dtype, device=device).split(sizes), shapes)]


def collect_blocks(layers, dead, dtype, want_sinks=True):
    """The blocks of the fusion layers ``layers[l][m]`` as a stack node takes them -> (params, fused, seeds, drop_p, sinks): the flat
    parameter list (14 per block) and fused[l][m] / seeds[l][m] / sinks[l][m] (sinks: None without grad mode or want_sinks), all
    layer-major, stream-minor.  A block with dead(l, m) is not run: it still contributes its parameters and still draws its
    dropout seeds (every later block's seeds depend on that), but its derived weights are not prepared (None).  The live blocks'
    derived weights are made by ONE fused_weights_of call."""
    live = iter(type(layers[0][0]).fused_weights_of(
        [layer for li, row in enumerate(layers) for m, layer in enumerate(row) if not dead(li, m)], dtype))
    params, fused, seeds, p = [], [], [], 0.0
    for li, row in enumerate(layers):
        frow, srow = [], []
        for m, layer in enumerate(row):
            params += layer.param_list()
            frow.append(None if dead(li, m) else next(live))
            p, sd = layer.dropout_args()
            srow.append(sd)
        fused.append(frow)
        seeds.append(srow)
    sinks = [[layer.grad_sink() for layer in row] for row in layers] if (want_sinks and torch.is_grad_enabled()) else None
    return params, fused, seeds, p, sinks


def key_lengths(varying_lengths, mask, txt_idx, device, add, batch=None):
    """Valid tokens per stream, int64 (None for an unmasked stream): the caller's length + add[m] (the stream's CLS rows), then on
    the text stream 3 -> 0 (a missing report).  batch: a 0-d length stands for that many samples.  The caller's tensors are not
    mutated."""
    out = []
    for m, a in enumerate(add):
        if not mask[m]:
            out.append(None)
            continue
        v = torch.as_tensor(varying_lengths[m], device=device).to(torch.int64)
        if batch is not None and v.dim() == 0:
            v = v.repeat(batch)
        v = v + a
        if m == txt_idx:
            v = torch.where(v == 3, torch.zeros_like(v), v)
        out.append(v)
    return out
