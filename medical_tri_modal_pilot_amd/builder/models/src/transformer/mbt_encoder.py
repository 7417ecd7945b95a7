"""TrimodalTransformerEncoder_MBT (and the two-stream BimodalTransformerEncoder_MBT) -- host orchestration of the
modality-aware bottleneck fusion (reference: builder/models/src/transformer/mbt_encoder.py:636-784 and :519-634).

Same constructor, parameter names and forward contract as the reference.  What differs is
how the work reaches the GPU:
  * raggedness is an int32 valid-key count per sample and stream ("kv_len"), computed on the
    device with no host loop (the reference builds [B,N,N] bool masks in a Python loop over
    the batch, utils.py:87-88, and tiles them x heads);
  * each (layer, modality) block is one ops.EncoderLayerFn (fused HIP kernels);
  * the caller's length tensors are NOT mutated (the reference does ``varying_lengths[n] += 1``
    in place, :704 -- nothing downstream reads them again).
"""
import contextlib
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from medical_tri_modal_pilot_amd import ops, tuning
from medical_tri_modal_pilot_amd.stack_plan import StackPlan, collect_blocks, key_lengths
from .encoder import TransformerEncoderLayer, next_dropout_seed
from .module import PositionalEncoding


def _declare_switches(enc):
    """What models, the trainer and tests set on an encoder from outside, and what its forward() leaves for them to read (every
    encoder's __init__ declares all of them; an encoder ignores those its forward() does not name)."""
    enc.first_stream_output_only = False     # model: it reads nothing but stream 0's output (e.g. its CLS row)
    enc.pack_rows = False                    # model: such a reader takes the vital-sign stream PACKED where forward() can
    enc.inputs_on_side_streams = False       # model, per call: it made the image / text embeddings on the two side streams
    enc.time_adds = None                     # model, for ONE call: (it, tt) time embeddings still to be added to their tokens
    enc.qie_adds = None                      # model, for ONE call: (add_v, add_i, add_t, handoff) of ops.QieAddsFn (--vslt-type QIE)
    enc.cls_only_last_layer = True           # a CLS-row reader's last layer computes that one row only
    enc.graph_segments = None                # trainer: layer counts at which to cut the fusion stack into chained nodes
    enc.overlap_streams = True               # tests: off = no side streams
    enc.segment_boundaries = []              # out: the three stream buffers between consecutive nodes
    enc.last_cls, enc.last_pack = None, None  # out: stream 0's CLS row as its own autograd output; the packed stream's row starts
    enc._streams_key = None


class TrimodalTransformerEncoder_MBT(nn.Module):
    supports_segments = True      # forward() can cut the fusion stack at ``graph_segments`` (staged hipGraph steps)

    def __init__(self, batch_size: int, n_modality: int, bottlenecks_n: int, fusion_startidx: int, d_input: int,
                 n_layers: int, n_head: int, d_model: int, d_ff: int, dropout: float = 0.1, pe_maxlen: int = 10000,
                 resbottle: bool = False, txt_idx: int = 2, vsltonly: int = 0, mbt_bottlenecks_type: str = "skip",
                 use_pe: list = [True, True, True], mask: list = [True, False, True],
                 compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        if n_modality != 3:
            # the reference module builds n_modality CLS tokens but always consumes 3 streams
            # (IndexError at mbt_encoder.py:699 for --input-types vslt); see DESIGN.md, config 1.
            raise ValueError("TrimodalTransformerEncoder_MBT needs --input-types vslt_img_txt (3 streams)")
        self.vsltonly = vsltonly
        self.mbt_bottlenecks_type = mbt_bottlenecks_type
        self.use_pe = use_pe
        self.n_modality = n_modality
        self.fusion_idx = fusion_startidx
        self.txt_idx = txt_idx
        self.n_layers = n_layers
        self.d_model = d_model
        self.bottlenecks_n = bottlenecks_n
        self.mask = mask
        self.resbottle = resbottle
        self.compute_dtype = compute_dtype
        self.idx_order = torch.arange(0, batch_size).type(torch.LongTensor)
        self.layer_norms_after_concat = nn.LayerNorm(self.d_model)       # unused by forward, kept for state_dict parity
        self.cls_token_per_modality = nn.ParameterList(
            [nn.Parameter(torch.randn(1, 1, d_model)) for _ in range(n_modality)])
        self.bottlenecks = nn.Parameter(torch.randn(1, bottlenecks_n, d_model))
        self.layer_norms_in = nn.ModuleList([nn.LayerNorm(d_model) for _ in range(n_modality)])
        self.positional_encoding = PositionalEncoding(d_model, max_len=pe_maxlen)
        self.dropout = nn.Dropout(dropout)
        self.layer_stacks = nn.ModuleList(nn.ModuleList([
            TransformerEncoderLayer(d_model=d_model, num_heads=n_head, d_ff=d_ff, dropout_p=dropout)
            for _ in range(n_modality)]) for _ in range(n_layers))
        _declare_switches(self)

    def _side_streams(self, dev):
        """Two extra HIP streams: the image (54-token) and text (133-token) streams of a layer cannot fill
        256 CUs on their own, so they run beside the 1005-token vital-sign stream."""
        if not self.overlap_streams or dev.type != "cuda":
            return None
        key = (dev.type, dev.index)
        if self._streams_key != key:
            # (default priority: high-priority side streams were measured -- 13.4 -> 18.8 ms/step under graph replay,
            #  13.6 -> 14.4 ms eager)
            self._streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
            self._streams_key = key
        return self._streams

    # ---- integer artefacts (bit-exact with the reference) ---------------------------------
    def key_lengths(self, varying_lengths, device) -> List[Optional[torch.Tensor]]:
        """Valid tokens per stream INCLUDING the CLS token, before the bottleneck prefix
        (mbt_encoder.py:703-714): +1 for CLS; text length == 3 (i.e. txt_lengths == 0) -> 0;
        None for an unmasked stream."""
        return key_lengths(varying_lengths, self.mask, self.txt_idx, device, [1] * self.n_modality)

    def forward(self, enc_outputs, fixed_lengths=None, varying_lengths=None, return_attns=False, fusion_idx=None,
                missing=None):
        dev = enc_outputs[0].device
        B = enc_outputs[0].size(0)
        dt = self.compute_dtype
        # valid-key counts: one HIP launch when the lengths are int64 device tensors (ops.stream_lengths), else key_lengths()
        raw = [varying_lengths[m] if self.mask[m] else None for m in range(self.n_modality)]
        one_launch = (dev.type == "cuda" and self.n_modality == 3 and any(v is not None for v in raw) and
                      all(v is None or (torch.is_tensor(v) and v.is_cuda and v.dtype == torch.int64 and v.dim() == 1) for v in raw))
        lens = None if one_launch else self.key_lengths(varying_lengths, dev)
        if fusion_idx is not None:
            self.fusion_idx = fusion_idx
        # stream input: [CLS | tokens] -> nn.LayerNorm (+ sinusoid PE) -> dropout  (:697-729)
        n_pre = min(max(self.fusion_idx if fusion_idx is None else fusion_idx, 0), self.n_layers)
        fused_in = (n_pre == 0 and self.n_layers > 0 and enc_outputs[0].is_cuda and len(enc_outputs) == 3
                    and all(x.dtype == dt for x in enc_outputs))
        # what a reader of stream 0 alone (``first_stream_output_only``, or vsltonly) lets this call leave out, each decided once here:
        #   first_only_  the packed vital-sign stream may be used (below)
        #   first_only   the LAST fusion layer's other blocks feed nothing: they are not run (their outputs read as zeros) ...
        #   skip_last    ... and their derived weights are not prepared (vsltonly: ops.FusionStackFn skips them too)
        #   cls_only     the reader takes nothing but stream 0's CLS row and the last layer runs that stream alone: it computes that
        #                one query row only (ops.layer_forward cls_tok: K / V of all rows, attention, FFN and residuals of the CLS row)
        fso = bool(self.first_stream_output_only)
        first_only_ = fso or self.vsltonly == 1
        first_only = fso and not self.resbottle and fused_in and self.vsltonly != 1
        skip_last = first_only or (self.vsltonly == 1 and fused_in and not self.resbottle)
        cls_only = fso and fused_in and (first_only or self.vsltonly == 1) and bool(self.cls_only_last_layer) and not return_attns
        streams = []
        if one_launch:
            kv_plain, kv_fused = ops.stream_lengths([None if v is None else v.contiguous() for v in raw], self.bottlenecks_n,
                                                    self.txt_idx)
        else:
            kv_plain = [None if l is None else l.to(torch.int32).contiguous() for l in lens]
            kv_fused = [None if l is None else (l + self.bottlenecks_n).to(torch.int32).contiguous() for l in lens]
        # PACKED vital-sign stream (``pack_rows``, set by a model that reads nothing of stream 0 but its CLS row): the samples'
        # valid rows -- bottleneck prefix, CLS, real events -- are stored back to back, so every kernel of the fusion stack
        # works on sum(kv_len) rows instead of B * (4 + 1 + T) (the reference pads to the batch maximum, trainer.py:41-42, and
        # masks keys, utils.py:79-125; a pad row's output is never read and its gradient is zero).  Buffer sizes and launch
        # grids stay those of the padded batch, so hipGraph replays are unaffected (ops.row_starts).
        pack_v = None
        if (self.pack_rows and fused_in and n_pre == 0 and first_only_ and kv_fused[0] is not None
                and dt == torch.bfloat16 and not return_attns):
            pack_v = ops.row_starts(kv_fused[0], self.bottlenecks_n + 1 + enc_outputs[0].size(1))
        self.last_pack = pack_v
        # the model may have produced the image / text embeddings on the two side streams (inputs_on_side_streams):
        # their stream-input kernels stay there, and the main stream joins before the fusion stack
        side_in = self._side_streams(dev) if (fused_in and self.inputs_on_side_streams) else None
        if side_in is None and self.inputs_on_side_streams and dev.type == "cuda":
            # the image / text embeddings were produced on the side streams but this call takes a torch path on the caller's
            # stream (uni-modal layers in front of the fusion layers, mixed dtypes): join them here
            for s_ in self._side_streams(dev) or ():
                torch.cuda.current_stream(dev).wait_stream(s_)
        # ``time_adds`` (set by the model for ONE call): the image / report time embeddings (it [n_i, 256], tt [n_t, 256]) still to be
        # added to every token of their group -- inside ops.StreamInputsFn when that node runs, here through torch otherwise
        time_adds, self.time_adds = self.time_adds, None
        # ``qie_adds`` (set by the model for ONE call): ops.QieAddsFn's rows for the three streams and the hand-off dict its backward
        # reads; they exist only for ops.StreamInputsQieFn, so a call that cannot run that node is refused
        qie_adds, self.qie_adds = getattr(self, "qie_adds", None), None
        if qie_adds is not None and (time_adds is not None or not (fused_in and tuning.FUSED_INPUT_TAIL and self.bottlenecks is not None)):
            raise RuntimeError("qie_adds need the fused stream-input node (fusion from layer 0, GPU tensors in the compute dtype) "
                               "and carry the time embeddings themselves")
        if time_adds is not None and not (fused_in and tuning.FUSED_INPUT_TAIL and self.bottlenecks is not None):
            enc_outputs = list(enc_outputs)
            for m, t in ((1, time_adds[0]), (2, time_adds[1])):
                x = enc_outputs[m]
                with (torch.cuda.stream(side_in[m - 1]) if side_in is not None else contextlib.nullcontext()):
                    g = t.shape[0] // x.shape[0]
                    enc_outputs[m] = (x.reshape(t.shape[0], x.shape[1] // g, x.shape[2]) + t.to(x.dtype).unsqueeze(1)).view(x.shape)
            time_adds = None
        if fused_in:          # LN + PE + dropout written behind the bottleneck rows: one HIP launch per stream (ops.StreamInput(s)Fn)
            pdrop = self.dropout.p if self.training else 0.0
            seeds_in = [next_dropout_seed() if pdrop > 0 else 0 for _ in enc_outputs]          # (drawn in stream order)
            pes = [self.positional_encoding(x.size(1) + 1) if self.use_pe[m] else None for m, x in enumerate(enc_outputs)]
            if tuning.FUSED_INPUT_TAIL and self.bottlenecks is not None:
                # ONE autograd node for the three streams: its backward -- the tail of the step -- is one launch + one reduction
                meta = dict(pe=pes, seeds=seeds_in, pack=None if pack_v is None else (pack_v, kv_fused[0]),
                            streams=None if side_in is None else [None, side_in[0], side_in[1]])
                lns = self.layer_norms_in
                prm = [t for m in range(3) for t in (self.cls_token_per_modality[m], lns[m].weight, lns[m].bias)]
                add_i, add_t = time_adds if time_adds is not None else (None, None)
                time_adds = None                       # (added inside the node)
                if qie_adds is not None:
                    meta["qie"] = qie_adds[3]
                    streams = list(ops.StreamInputsQieFn.apply(enc_outputs[0], enc_outputs[1], enc_outputs[2], self.bottlenecks,
                                                               qie_adds[0], qie_adds[1], qie_adds[2], lns[0].eps, lns[1].eps,
                                                               lns[2].eps, pdrop, meta, *prm))
                else:
                    streams = list(ops.StreamInputsFn.apply(enc_outputs[0], enc_outputs[1], enc_outputs[2], self.bottlenecks, add_i,
                                                            add_t, lns[0].eps, lns[1].eps, lns[2].eps, pdrop, meta, *prm))
            else:
                made = {}
                # one node per stream, the vital-sign stream's created LAST: autograd runs the three (ready together, behind the
                # fusion stack's backward) latest-created first, and that stream's chain is the critical path of the step's tail
                for m in [1, 2, 0] if tuning.INPUT_NODE_ORDER == "long_last" else [0, 1, 2]:
                    x, ln = enc_outputs[m], self.layer_norms_in[m]
                    with (torch.cuda.stream(side_in[m - 1]) if (side_in is not None and m > 0) else contextlib.nullcontext()):
                        pk = (pack_v, kv_fused[0]) if (m == 0 and pack_v is not None) else (None, None)
                        made[m] = ops.StreamInputFn.apply(x, self.cls_token_per_modality[m], ln.weight, ln.bias, pes[m],
                                                          self.bottlenecks, ln.eps, pdrop, seeds_in[m], *pk)
                streams = [made[m] for m in range(len(enc_outputs))]
        for m, x in enumerate(enc_outputs if not fused_in else []):
            ln = self.layer_norms_in[m]
            x = torch.cat([self.cls_token_per_modality[m].expand(B, -1, -1).to(x.dtype), x], dim=1)
            y = F.layer_norm(x.float(), (self.d_model,), ln.weight, ln.bias, ln.eps)
            if self.use_pe[m]:
                y = y + self.positional_encoding(x.size(1))
            streams.append(self.dropout(y).to(dt))
        # (no join here when the inputs live on the side streams: ops.FusionStackFn issues each modality's first layer
        #  on that same stream and joins at the first bottleneck exchange)
        missing = missing.to(dev).long()
        n_pre = min(max(self.fusion_idx, 0), self.n_layers)
        for li in range(n_pre):                                               # uni-modal layers (:734-737)
            streams = [layer(streams[m], kv_plain[m])[0] for m, layer in enumerate(self.layer_stacks[li])]
        self.last_cls = None
        if n_pre == self.n_layers:
            return streams, 0
        # fusion layers: one explicit-buffer autograd node (ops.FusionStackFn); the streams carry the
        # bottleneck tokens in rows 0..3 of their own buffer: [bottleneck | CLS | tokens] (:745)
        fl = list(self.layer_stacks)[n_pre:]
        params, fused, seeds, p, sinks = collect_blocks(fl, lambda li, m: skip_last and li == len(fl) - 1 and m > 0, dt)
        # graph_segments (set by the trainer for staged hipGraph + DDP steps): cut the fusion layers into chained
        # ops.FusionStackFn nodes at these layer counts; segment_boundaries then holds the three stream buffers
        # between consecutive nodes (the tensors the staged backward is cut at).
        cuts = [c for c in (self.graph_segments or []) if 0 < c < len(fl)]
        if cuts and (not fused_in or self.resbottle or not torch.is_grad_enabled()):
            cuts = []
        bounds = [0] + sorted(set(cuts)) + [len(fl)]
        self.segment_boundaries = []
        zs = (streams[0], streams[1], streams[2])
        cls_v = None
        # the layer in front of a CLS-only last layer: its image / text outputs feed the bottleneck exchange and nothing else
        # (ops.layer_forward ffn_rows) -- by GLOBAL layer index, whatever segment it falls into
        g_ex = len(fl) - 2 if (cls_only and not self.resbottle) else -1
        per = 3 * ops.PARAMS_PER_LAYER      # parameters of one layer
        for b0, b1 in zip(bounds, bounds[1:]):
            final = b1 == len(fl)
            plan = StackPlan(n_layers=b1 - b0, vsltonly=self.vsltonly, resbottle=bool(self.resbottle), kv=kv_fused,
                             sinks=sinks and sinks[b0:b1], prebuilt=fused_in or b0 > 0, final=final, bott_rows_unused=True,
                             first_only=first_only and final, missing=missing, drop_p=p, seeds=seeds[b0:b1], fused=fused[b0:b1],
                             dtype=dt, side_streams=self._side_streams(dev), inputs_on_side=side_in is not None and b0 == 0,
                             pack_v=pack_v, cls_only=cls_only and final, exchange_only_layer=g_ex - b0 if b0 <= g_ex < b1 else -1,
                             infer=ops.infer_active(p))
            out_v, out_i, out_t, cls_v = ops.FusionStackFn.apply(zs[0], zs[1], zs[2], self.bottlenecks, *params[b0 * per:b1 * per], plan)
            zs = (out_v, out_i, out_t)
            if not final:
                self.segment_boundaries.append(zs)
        nb = self.bottlenecks_n
        self.last_cls = cls_v               # = outs[0][:, 0, :] as its own autograd output (cheap backward)
        # (a packed stream 0 has no [B, N] view, and with cls_only only the CLS row of the last layer exists: the reader takes ``last_cls``)
        out_v = None if (pack_v is not None or cls_only) else out_v[:, nb:]
        if self.vsltonly == 1:
            return [out_v], 0
        return [out_v, out_i[:, nb:], out_t[:, nb:]], 0


class BimodalTransformerEncoder_MBT(nn.Module):
    """Two-stream bottleneck fusion (reference: builder/models/src/transformer/mbt_encoder.py:519-634).

    Same constructor, parameter names and forward contract as the reference.  EVERY layer is a fusion layer (the
    reference's uni-modal branch is commented out, :610-615, so ``fusion_startidx`` is stored and ignored like there);
    after each layer the bottleneck tokens become the mean of both streams' (``missing == 0``) or stream 0's alone
    (``missing == 1``), :629-632.  Runs on the same explicit-buffer engine as the three-stream encoder
    (ops.FusionStackFn with ``n_streams=2``; the exchange kernel reads its weight-table rows 1 and 3)."""

    def __init__(self, batch_size: int, n_modality: int, bottlenecks_n: int, fusion_startidx: int, d_input: int,
                 n_layers: int, n_head: int, d_model: int, d_ff: int, dropout: float = 0.1, pe_maxlen: int = 10000,
                 txt_idx: int = 2, mbt_bottlenecks_type: str = "skip", use_pe: list = [True, True],
                 mask: list = [True, True], compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        if n_modality != 2:
            raise ValueError("BimodalTransformerEncoder_MBT consumes exactly two streams (the reference builds n_modality "
                             "CLS tokens and layer blocks but sets self.n_modality = 2, mbt_encoder.py:547)")
        self.mbt_bottlenecks_type = mbt_bottlenecks_type
        self.use_pe, self.mask = use_pe, mask
        self.n_modality = 2
        self.fusion_idx, self.txt_idx = fusion_startidx, txt_idx
        self.n_layers, self.d_model, self.bottlenecks_n = n_layers, d_model, bottlenecks_n
        self.compute_dtype = compute_dtype
        self.idx_order = torch.arange(0, batch_size).type(torch.LongTensor)
        self.layer_norms_after_concat = nn.LayerNorm(self.d_model)       # unused by forward, kept for state_dict parity
        self.cls_token_per_modality = nn.ParameterList(
            [nn.Parameter(torch.randn(1, 1, d_model)) for _ in range(n_modality)])
        self.bottlenecks = nn.Parameter(torch.randn(1, bottlenecks_n, d_model))
        self.layer_norms_in = nn.ModuleList([nn.LayerNorm(d_model) for _ in range(n_modality)])
        self.positional_encoding = PositionalEncoding(d_model, max_len=pe_maxlen)
        self.dropout = nn.Dropout(dropout)
        self.layer_stacks = nn.ModuleList(nn.ModuleList([
            TransformerEncoderLayer(d_model=d_model, num_heads=n_head, d_ff=d_ff, dropout_p=dropout)
            for _ in range(n_modality)]) for _ in range(n_layers))
        _declare_switches(self)

    supports_segments = False
    resbottle = False
    _side_streams = TrimodalTransformerEncoder_MBT._side_streams

    def key_lengths(self, varying_lengths, device) -> List[Optional[torch.Tensor]]:
        """Valid tokens per stream including CLS (:583-591): +1; stream ``txt_idx``: 3 -> 0; None when unmasked."""
        return key_lengths(varying_lengths, self.mask, self.txt_idx, device, [1, 1])

    def forward(self, enc_outputs, fixed_lengths=None, varying_lengths=None, return_attns=False, fusion_idx=None,
                missing=None):
        if len(enc_outputs) != 2:
            raise ValueError("BimodalTransformerEncoder_MBT takes two streams")
        dev, dt = enc_outputs[0].device, self.compute_dtype
        if fusion_idx is not None:
            self.fusion_idx = fusion_idx
        lens = self.key_lengths(varying_lengths, dev)
        pdrop = self.dropout.p if self.training else 0.0
        streams = []
        for m, x in enumerate(enc_outputs):                                   # (:575-607) CLS, LayerNorm (+PE), dropout
            ln = self.layer_norms_in[m]
            pe = self.positional_encoding(x.size(1) + 1) if self.use_pe[m] else None
            seed = next_dropout_seed() if pdrop > 0 else 0
            streams.append(ops.StreamInputFn.apply(x.to(dt), self.cls_token_per_modality[m], ln.weight, ln.bias, pe,
                                                   self.bottlenecks, ln.eps, pdrop, seed))
        kv = [None if l is None else (l + self.bottlenecks_n).to(torch.int32).contiguous() for l in lens]
        # missing 0 -> table row 1 (0.5, 0.5, 0), missing 1 -> row 3 (1, 0, 0); anything else is out of bounds for the
        # reference's two candidates (:631) and stays out of bounds for the kernel's host check
        # (checked on the host only when ``missing`` lives there: a device-side check would be a sync, and a captured
        #  step cannot have one; the kernel clamps its table index)
        if not missing.is_cuda and missing.numel() and (int(missing.max()) > 1 or int(missing.min()) < 0):
            raise IndexError("BimodalTransformerEncoder_MBT: missing must be 0 (both streams) or 1 (stream 0 only)")
        missing = missing.to(dev).long()
        if missing.is_cuda and not torch.cuda.is_current_stream_capturing():
            # device-resident flags outside a capture: an asynchronous device-side assert instead of the host check (the
            # reference's gather all_bottleneck_stack[missing, idx_order] raises; the exchange kernel alone would clamp)
            torch._assert_async(((missing >= 0) & (missing <= 1)).all(),
                                "BimodalTransformerEncoder_MBT: missing must be 0 (both streams) or 1 (stream 0 only)")
        pattern = 1 + 2 * missing
        fl = list(self.layer_stacks)
        params, fused, seeds, p, sinks = collect_blocks(fl, lambda li, m: False, dt)
        plan = StackPlan(n_layers=len(fl), n_streams=2, kv=kv + [None], sinks=sinks, prebuilt=True, bott_rows_unused=True,
                         missing=pattern, drop_p=p, seeds=seeds, fused=fused, dtype=dt, side_streams=self._side_streams(dev),
                         infer=ops.infer_active(p))
        out0, out1, _, _ = ops.FusionStackFn.apply(streams[0], streams[1], None, self.bottlenecks, *params, plan)
        nb = self.bottlenecks_n
        return [out0[:, nb:], out1[:, nb:]], 0


class TrimodalTransformerEncoder_Multitokens_MBTVSLTMAIN(nn.Module):
    """Multi-token bottleneck fusion (reference: builder/models/src/transformer/mbt_encoder.py:9-193).

    Same constructor, parameter names and forward contract as the reference.  What differs from TrimodalTransformerEncoder_MBT:
      * four CLS rows on the vital-sign stream (``cls_token`` [1, 4, 256]), none on the image and text streams;
      * four SETS of four bottleneck rows -- vit, vi, vt, it -- of which every stream carries three as a 12-row prefix
        (``bottlenecks_map``); in the first layer all of them are the one parameter ``bottlenecks`` [1, 4, 256], so its gradient is
        the sum over the nine slots (autograd sums it: the prefix is a torch expression);
      * a fixed boolean mask over the first 16 x 16 (vital signs) / 12 x 12 (image, text) block of the score matrix decides which
        CLS row and which bottleneck set see which (``prefix_masks``, :64-94), on top of the key-pad mask -- the attention kernels
        take it as ``qk_mask`` words; an unmasked stream (``mask[m]`` false) gets neither, as in the reference (:164-174);
      * after a fusion layer every set becomes the mean over the holders that ``b_out_mean_map`` selects for the sample's pattern
        (ops.bottleneck_exchange_multi).
    The layers run on the layer engine through ops.MultiTokenStackFn; the stream input (prefix | CLS | tokens, LayerNorm, PE on the
    text stream, dropout) is torch ops.  Every layer is a fusion layer (``fusion_startidx`` 0); ``resbottle`` is commented out in
    the reference class and refused here.  ``first_stream_output_only`` (set by a model that reads stream 0's output only): the
    last layer's image / text blocks are not run and their outputs read as zeros."""
    supports_segments = False
    n_cls = 4
    n_prefix = ops.N_PREFIX

    def __init__(self, batch_size: int, n_modality: int, bottlenecks_n: int, fusion_startidx: int, d_input: int, n_layers: int,
                 n_head: int, d_model: int, d_ff: int, dropout: float = 0.1, pe_maxlen: int = 5000, txt_idx: int = 2,
                 resbottle: bool = False, use_pe: list = [False, False, True], mask: list = [True, True, True],
                 compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        if n_modality != 3 or bottlenecks_n != 4:
            raise ValueError("TrimodalTransformerEncoder_Multitokens_MBTVSLTMAIN needs three streams and four bottleneck rows per set")
        if resbottle:
            raise NotImplementedError("--residual-bottlenecks 1: the reference has it commented out in this class (mbt_encoder.py:154-190)")
        if fusion_startidx != 0:
            raise NotImplementedError("the multi-token encoder is built for --mbt-fusion-startIdx 0 (every layer a fusion layer)")
        self.use_pe, self.mask = use_pe, mask
        self.n_modality, self.fusion_idx, self.txt_idx = n_modality, fusion_startidx, txt_idx
        self.n_layers, self.d_model, self.bottlenecks_n = n_layers, d_model, bottlenecks_n
        self.resbottle = resbottle
        self.compute_dtype = compute_dtype
        self.idx_order = torch.arange(0, batch_size).type(torch.LongTensor)
        self.layer_norms_after_concat = nn.LayerNorm(self.d_model)       # unused by forward, kept for state_dict parity
        self.layer_norms_in = nn.ModuleList([nn.LayerNorm(d_model) for _ in range(n_modality)])
        self.positional_encoding = PositionalEncoding(d_model, max_len=pe_maxlen)
        self.dropout = nn.Dropout(dropout)
        self.final_cls_tokens_num = self.n_cls
        self.cls_token = nn.Parameter(torch.randn(1, self.n_cls, d_model))
        self.bottlenecks = nn.Parameter(torch.randn(1, bottlenecks_n, d_model))
        self.bottlenecks_map = [list(r) for r in ops.MULTI_BOTTLENECKS_MAP]
        self.layer_stacks = nn.ModuleList(nn.ModuleList([
            TransformerEncoderLayer(d_model=d_model, num_heads=n_head, d_ff=d_ff, dropout_p=dropout)
            for _ in range(n_modality)]) for _ in range(n_layers))
        _declare_switches(self)

    def _side_streams(self, dev):
        """no side streams: the three streams of a layer go out as one grouped launch on the caller's stream"""
        return None

    # ---- integer artefacts (bit-exact with the reference) ---------------------------------
    @staticmethod
    def prefix_masks() -> List[torch.Tensor]:
        """The three boolean masks of :64-94 (True = the query row does not attend the key): [16,16], [12,12], [12,12].  Rows / keys
        0..11 are the stream's three bottleneck sets; 12..15 of the first are the CLS rows: CLS i sees set i and itself (CLS 3 only
        itself), a set sees itself and, on the vital-sign stream, its CLS row.  The image mask has ONE masked row (``[::12, :12]``)."""
        v = torch.ones(16, 16)
        v[:4, :4] = 0
        v[4:8, 4:8] = 0
        v[8:12, 8:12] = 0
        for c in range(12, 16):
            v[c, c] = 0
        for c, a in ((12, 0), (13, 4), (14, 8)):
            v[c, a:a + 4] = 0
            v[a:a + 4, c] = 0
        i = torch.zeros(12, 12)
        i[::12, :12] = 1
        t = torch.ones(12, 12)
        for m_ in (i, t):
            m_[:4, :4] = 0
            m_[4:8, 4:8] = 0
            m_[8:12, 8:12] = 0
        return [v.ge(0.5), i.ge(0.5), t.ge(0.5)]

    def mask_words(self) -> List[Optional[List[int]]]:
        """per stream the prefix mask as the attention kernels take it (bit j of word i), None for an unmasked stream"""
        return [[sum(int(mk[r, c]) << c for c in range(mk.shape[1])) for r in range(mk.shape[0])] if self.mask[m] else None
                for m, mk in enumerate(self.prefix_masks())]

    def key_lengths(self, varying_lengths, n_tokens, device) -> List[Optional[torch.Tensor]]:
        """Valid keys per stream INCLUDING the 12 prefix rows (:120-122, 166): vital signs + 4 CLS rows; text length == 3 (that is
        txt_lengths == 1) -> 0; None for an unmasked stream.  The caller's tensors are not mutated."""
        lens = key_lengths(varying_lengths, self.mask, self.txt_idx, device, [self.n_cls, 0, 0], batch=n_tokens[0][0])
        return [None if v is None else (v + self.n_prefix).to(torch.int32).contiguous() for v in lens]

    def forward(self, enc_outputs, fixed_lengths=None, varying_lengths=None, return_attns=False, fusion_idx=None, missing=None):
        if len(enc_outputs) != 3:
            raise ValueError("TrimodalTransformerEncoder_Multitokens_MBTVSLTMAIN takes three streams")
        if fusion_idx not in (None, 0):
            raise NotImplementedError("the multi-token encoder is built for fusion_idx 0")
        dev, dt = enc_outputs[0].device, self.compute_dtype
        B = enc_outputs[0].size(0)
        kv = self.key_lengths(varying_lengths, [(B, x.size(1)) for x in enc_outputs], dev)
        # pattern ids outside 0..3: the reference's gather (:187) raises; checked on the host when the ids live there, as an
        # asynchronous device-side assert otherwise (never inside a capture); the exchange kernel clamps its table index
        if not missing.is_cuda and missing.numel() and (int(missing.max()) > 3 or int(missing.min()) < 0):
            raise IndexError("TrimodalTransformerEncoder_Multitokens_MBTVSLTMAIN: missing must be in 0..3")
        missing = missing.to(dev).long().contiguous()
        if missing.is_cuda and not torch.cuda.is_current_stream_capturing():
            torch._assert_async(((missing >= 0) & (missing <= 3)).all())
        # stream input (:113-142): [4 CLS | events] on the vital-sign stream, LayerNorm (+ PE), dropout; then the 12 prefix rows
        prefix = self.bottlenecks.repeat(1, 3, 1).expand(B, -1, -1)
        zs = []
        for m, x in enumerate(enc_outputs):
            ln = self.layer_norms_in[m]
            if m == 0:
                x = torch.cat([self.cls_token.expand(B, -1, -1).to(x.dtype), x], dim=1)
            y = F.layer_norm(x.float(), (self.d_model,), ln.weight, ln.bias, ln.eps)
            if self.use_pe[m]:
                y = y + self.positional_encoding(x.size(1))
            zs.append(torch.cat([prefix.to(dt), self.dropout(y).to(dt)], dim=1).contiguous())
        fl = list(self.layer_stacks)
        first_only = bool(self.first_stream_output_only)
        params, fused, seeds, p, _ = collect_blocks(fl, lambda li, m: first_only and li == len(fl) - 1 and m > 0, dt, want_sinks=False)
        plan = StackPlan(n_layers=len(fl), kv=kv, masks=self.mask_words(), missing=missing, drop_p=p, seeds=seeds, fused=fused,
                         dtype=dt, first_only=first_only, exchange_last=False, infer=ops.infer_active(p))
        outs = ops.MultiTokenStackFn.apply(zs[0], zs[1], zs[2], *params, plan)
        return [o[:, self.n_prefix:] for o in outs], 0
