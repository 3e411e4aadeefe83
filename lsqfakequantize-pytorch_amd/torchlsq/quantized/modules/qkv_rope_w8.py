"""`QKVRotaryW8Q`: the first half of an attention block on 8-bit LEVELS -- the qkv projection, the rotary embedding of q and k and the
append of k and v to a `KVCacheW8` or a `PagedKVCacheW8` -- as one module over its children `qkv` (`LinearW8A8Q`) and `rotary`
(`RotaryW8Q`).  A decode step (at most 16 rows) can run as ONE launch (`torch.ops.torchlsq.lsq_linear_w8_q8_dec_rope_q`,
liblsq_hip_linrope_w8.so: the rotation and the cache writes in the linear's epilogue) with the bytes of the children run one by
one; nothing is read back to the host and no host tensor is made per call, so a step can be captured in a graph.
"""
import torch
from torch import nn

from torchlsq.functional import LevelsTensor, _levels_out, _takes_rope_epilogue
from .rope_w8 import RotaryW8Q
from .w8a8_q import LinearW8A8Q, _as_levels


class QKVRotaryW8Q(nn.Module):
    """`forward(x, cache)`: x a `LevelsTensor` [B, T, K], `cache` a `KVCacheW8` or a `PagedKVCacheW8` of `kv_heads` heads.  Returns
    `(rq, k_levels, v_levels, lengths)`: the rotated q [B, T, heads, D] and what `cache.append(k, v, rotary)` returns -- exactly
    `rotary(q, positions=cache.lengths)` and that append on the three views of `qkv(x)`, the cache's bookkeeping and
    `lengths.add_(T)` included.
    `rope_epilogue` (extra state; True / False / None: `torchlsq.functional.W8A8_ROPE_EPILOGUE_DEFAULT`): where it resolves to True, x
    has at most 16 rows, `qkv` is a plain `LinearW8A8Q` without ReLU and `rotary` has an output quantizer, the half style and qkv's
    `mid_dtype`, the projection, the rotation and the append are ONE op; calls it does not serve run the children one by one inside
    it.  Inference only."""

    def __init__(self, qkv, rotary, heads, kv_heads, rope_epilogue=None):
        super().__init__()
        assert isinstance(qkv, LinearW8A8Q) and isinstance(rotary, RotaryW8Q), "QKVRotaryW8Q takes a LinearW8A8Q and a RotaryW8Q"
        self.heads, self.kv_heads = int(heads), int(kv_heads)
        assert qkv.out_features == (self.heads + 2 * self.kv_heads) * rotary.dim, \
            "QKVRotaryW8Q: qkv has %d output features, (heads + 2 kv_heads) dim = %d are needed" % (
                qkv.out_features, (self.heads + 2 * self.kv_heads) * rotary.dim)
        self.qkv, self.rotary = qkv, rotary
        self.rope_epilogue = rope_epilogue

    def _in_epilogue(self, x, cache):
        """the one op on the cache's own buffers, then the cache's bookkeeping as `append` does it"""
        m, r = self.qkv, self.rotary
        paged = hasattr(cache, "block_table")
        kc, vc = (cache.k_pool, cache.v_pool) if paged else (cache.k, cache.v)
        v = m._wrap(vc)                             # the constants of the qkv levels, formed on the device once per call
        lv = torch.ops.torchlsq.lsq_linear_w8_q8_dec_rope_q(
            x.levels, x.scale, x.zero_point, m.weight_levels, m.weight_scale, m.weight_zero_point, m.bias, m.output_scale, m.output_shift,
            *m.output_range, v.scale, v.zero_point, r.cos, r.sin, *r._out("output"), r.mid_dtype, self.heads, self.kv_heads, kc, vc, cache.lengths,
            cache.block_table if paged else None)
        rq = _levels_out(lv, r.output_scale.detach().reshape(-1)[:1], r.output_shift.detach().reshape(-1)[:1], r.output_range)
        cache._keep("_k_side", LevelsTensor(kc, rq.scale, rq.zero_point, *r.output_range))
        cache._keep("_v_side", v)
        cache.lengths.add_(int(x.shape[1]))
        return rq, LevelsTensor(kc, *cache._k_side), LevelsTensor(vc, *cache._v_side), cache.lengths

    def forward(self, x, cache):
        x = _as_levels(x)
        m, r = self.qkv, self.rotary
        if isinstance(x, LevelsTensor) and x.levels.dim() == 3 and _takes_rope_epilogue(self.rope_epilogue, x.levels) and \
                type(m) is LinearW8A8Q and not m.relu and r.output_range is not None and not r.interleaved and m.mid_dtype == r.mid_dtype:
            return self._in_epilogue(x, cache)
        qkv = m(x)
        B, T = int(qkv.shape[0]), int(qkv.shape[1])
        lv = qkv.levels.view(B, T, self.heads + 2 * self.kv_heads, r.dim)
        q, k, v = (LevelsTensor(lv[:, :, a:b], qkv.scale, qkv.zero_point, qkv.quant_min, qkv.quant_max, qkv.type_min, qkv.type_max)
                   for a, b in ((0, self.heads), (self.heads, self.heads + self.kv_heads), (self.heads + self.kv_heads, lv.shape[2])))
        rq = r(q, positions=cache.lengths)
        return (rq,) + tuple(cache.append(k, v, rotary=r))

    def get_extra_state(self):
        return dict(rope_epilogue=self.rope_epilogue)

    def set_extra_state(self, state):
        self.rope_epilogue = state.get("rope_epilogue")

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        if self.rope_epilogue is None:      # the default is not written: the keys are the children's
            destination.pop(prefix + "_extra_state", None)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        state_dict.setdefault(prefix + "_extra_state", {})      # no key: None
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def extra_repr(self):
        return "heads=%d, kv_heads=%d" % (self.heads, self.kv_heads) + ("" if self.rope_epilogue is None else ", rope_epilogue=%s" % self.rope_epilogue)
