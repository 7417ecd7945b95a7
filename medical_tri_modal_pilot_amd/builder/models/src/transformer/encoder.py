"""TransformerEncoderLayer / MultiHeadAttention of the reference
(builder/models/src/transformer/encoder.py:8-34, attention.py:52-84) as thin hosts of the
fused HIP path: the modules own the parameters under the reference's names; forward()
hands them to ops.EncoderLayerFn (LN+QKV GEMM, key-masked attention, LN+FFN).
"""
from typing import Optional

import torch
import torch.nn as nn

from medical_tri_modal_pilot_amd import ops
from .module import FeedForwardUseConv, LayerNorm, Linear

_seed_counter = [0]


def next_dropout_seed() -> int:
    """Stateless-mask seeds: murmur-mixed (torch.initial_seed(), call counter)."""
    _seed_counter[0] += 1
    x = (torch.initial_seed() * 0x9E3779B1 + _seed_counter[0] * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    return x


def pad_mask_to_kv_len(mask: torch.Tensor) -> torch.Tensor:
    """[B,N,N] (or [B,1,N]) key-pad mask of utils.py:116-125 (True = padded key) -> int32 valid-key counts.
    Such masks are always a prefix of valid keys, identical for every query row."""
    return (~mask[:, 0, :]).sum(-1).to(torch.int32)


class MultiHeadAttention(nn.Module):
    def __init__(self, dim: int = 512, num_heads: int = 8) -> None:
        super().__init__()
        assert dim % num_heads == 0, "hidden_dim % num_heads should be zero."
        self.d_head = dim // num_heads
        self.num_heads = num_heads
        self.query_proj = Linear(dim, dim)
        self.key_proj = Linear(dim, dim)
        self.value_proj = Linear(dim, dim)


class TransformerEncoderLayer(nn.Module):
    def __init__(self, d_model: int = 512, num_heads: int = 8, d_ff: int = 2048, dropout_p: float = 0.3) -> None:
        super().__init__()
        if d_model != ops.D_MODEL or num_heads != ops.N_HEAD or d_ff != 4 * d_model:
            raise NotImplementedError("the MI355X kernels are built for d_model 256 / 4 heads / d_ff 1024 "
                                      "(tri_mbt_vsltcls.py:117,227-228 hard-code d_model 256)")
        self.attention_prenorm = LayerNorm(d_model)
        self.feed_forward_prenorm = LayerNorm(d_model)
        self.self_attention = MultiHeadAttention(d_model, num_heads)
        self.feed_forward = FeedForwardUseConv(d_model, d_ff, dropout_p)
        self.dropout_p = dropout_p
        self._fused_key = None
        self._fused = None

    def _fused_parts(self, dtype):
        """(key, parts): parts = ([Wq;Wk;Wv] [768,256], its bias, W1 [1024,256], W2 [256,1024]) in the compute dtype,
        or None when the cached tuple is still current (no parameter changed since it was built)."""
        a, f = self.self_attention, self.feed_forward
        ps = [a.query_proj.linear.weight, a.key_proj.linear.weight, a.value_proj.linear.weight,
              a.query_proj.linear.bias, a.key_proj.linear.bias, a.value_proj.linear.bias, f.w_1.weight, f.w_2.weight]
        key = (dtype, ops._fused_epoch[0]) + tuple((p._version, p.data_ptr()) for p in ps)
        if key == self._fused_key:
            return key, None
        # parameters living in an optim.FlatParams buffer: views of the fp32 master / the bf16 shadow that the
        # AdamW kernel keeps current -- no cast kernels in the step (only W2^T is materialised)
        flat = getattr(ps[0], "_mtmp_flat", None)
        if flat is not None and all(getattr(q, "_mtmp_flat", None) is flat for q in ps):
            ix = [flat.index_of[id(q)] for q in ps]
            wqkv, bqkv = flat.span(ix[0:3], dtype), flat.span(ix[3:6], torch.float32)
            w1, w2 = flat.span(ix[6:7], dtype), flat.span(ix[7:8], dtype)
            if all(t is not None for t in (wqkv, bqkv, w1, w2)):
                return key, (wqkv.view(3 * ps[0].shape[0], -1), bqkv, w1.view(ps[6].shape[0], -1),
                             w2.view(ps[7].shape[0], -1))
        with torch.no_grad():
            return key, (torch.cat([ps[0], ps[1], ps[2]], 0).to(dtype).contiguous(),
                         torch.cat([ps[3], ps[4], ps[5]], 0).float().contiguous(),
                         ps[6].reshape(ps[6].shape[0], -1).to(dtype).contiguous(),
                         ps[7].reshape(ps[7].shape[0], -1).to(dtype).contiguous())

    def _fused_weights(self, dtype):
        """ops.FusedWeights: parts + (W2^T, Wqkv^T, W1^T) -- the K-contiguous operands of the backward's dH / dX products; rebuilt only
        when a parameter changed (optimizer step / load_state_dict)."""
        key, parts = self._fused_parts(dtype)
        if parts is not None:
            with torch.no_grad():
                self._fused = ops.FusedWeights(*parts, parts[3].t().contiguous(), parts[0].t().contiguous(), parts[2].t().contiguous())
            self._fused_key = key
        return self._fused

    @staticmethod
    def fused_weights_of(blocks, dtype):
        """``_fused_weights`` of many blocks with ONE batched transpose per weight kind for all stale blocks (a stack
        and a strided copy instead of ~5 us launches per block on the critical path of every step)."""
        stale = []
        for blk in blocks:
            key, parts = blk._fused_parts(dtype)
            if parts is not None:
                stale.append((blk, key, parts))
        if stale:
            with torch.no_grad():
                if stale[0][2][0].is_cuda:         # one launch for the three transposes of every stale block
                    ts = ops.transpose_batch([p[j].contiguous() for _, _, p in stale for j in (3, 0, 2)])
                    w2t, wqkvt, w1t = ts[0::3], ts[1::3], ts[2::3]
                else:
                    w2t, wqkvt, w1t = (torch.stack([p[j] for _, _, p in stale]).transpose(1, 2).contiguous() for j in (3, 0, 2))
            for i, (blk, key, parts) in enumerate(stale):
                blk._fused, blk._fused_key = ops.FusedWeights(*parts, w2t[i], wqkvt[i], w1t[i]), key
        return [blk._fused for blk in blocks]

    def param_list(self):
        """The 14 parameters in ops.PARAMS order."""
        a, f = self.self_attention, self.feed_forward
        return [self.attention_prenorm.gamma, self.attention_prenorm.beta,
                a.query_proj.linear.weight, a.query_proj.linear.bias, a.key_proj.linear.weight, a.key_proj.linear.bias,
                a.value_proj.linear.weight, a.value_proj.linear.bias,
                self.feed_forward_prenorm.gamma, self.feed_forward_prenorm.beta,
                f.w_1.weight, f.w_1.bias, f.w_2.weight, f.w_2.bias]

    def forward(self, inputs: torch.Tensor, self_attn_mask: Optional[torch.Tensor] = None):
        """inputs [B,N,256] (fp32 or bf16 on the GPU); self_attn_mask: int [B] valid-key counts, or the
        reference's bool pad mask, or None.  Returns (outputs, None) like the reference (the attention
        matrix is never materialised)."""
        kv_len = self_attn_mask
        if kv_len is not None and kv_len.dtype == torch.bool:
            kv_len = pad_mask_to_kv_len(kv_len)
        if kv_len is not None:
            kv_len = kv_len.to(device=inputs.device, dtype=torch.int32).contiguous()
        p, seeds = self.dropout_args()
        if ops.infer_active(p):            # (read here, at call time: inside the node grad mode is always off)
            return ops.EncoderLayerFn.apply(inputs, kv_len, *self.param_list(), self._fused_weights(inputs.dtype), p, seeds, None, True), None
        out = ops.EncoderLayerFn.apply(inputs, kv_len, *self.param_list(), self._fused_weights(inputs.dtype), p, seeds)
        return out, None

    def grad_sink(self):
        """ops.GradSink when these parameters live in an optim.FlatParams buffer (FusedAdamW), else None."""
        P = self.param_list()
        flat = getattr(P[0], "_mtmp_flat", None)
        if flat is None or any(getattr(p, "_mtmp_flat", None) is not flat for p in P):
            return None
        key = (id(flat), flat.grad.data_ptr())
        if getattr(self, "_sink_key", None) != key:
            self._sink = ops.GradSink(flat, [flat.index_of[id(p)] for p in P])
            self._sink_key = key
        return self._sink

    def dropout_args(self):
        p = self.dropout_p if self.training else 0.0
        return p, ((next_dropout_seed(), next_dropout_seed()) if p > 0 else (0, 0))
