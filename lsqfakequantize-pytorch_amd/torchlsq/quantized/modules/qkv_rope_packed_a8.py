"""`QKVRotaryPackedA8Q`: the first half of an attention block on 8-bit LEVELS with a PACKED 4- / 2-bit group-wise qkv weight -- the qkv
projection, the rotary embedding of q and k and the append of k and v to a `KVCacheW8` or a `PagedKVCacheW8` -- as one module over its
children `qkv` (`PackedLinearA8Q`) and `rotary` (`RotaryW8Q`): what `QKVRotaryW8Q` is for 8-bit weight levels.  A decode step (at most
16 rows) can run as ONE launch (`torch.ops.torchlsq.lsq_linear_packed_q8_rope_q`, liblsq_hip_linrope_w4.so: the rotation and the cache
writes in the linear's epilogue) with the bytes of the children run one by one; nothing is read back to the host and no host tensor
is made per call, so a step can be captured in a graph.
"""
import torch

from torchlsq import functional as F
from torchlsq.functional import LevelsTensor, _levels_out, _takes_decode
from .packed_a8_q import PackedLinearA8Q
from .qkv_rope_w8 import QKVRotaryW8Q
from .rope_w8 import RotaryW8Q
from .w8a8_q import _as_levels


class QKVRotaryPackedA8Q(QKVRotaryW8Q):
    """`forward(x, cache)` returns `(rq, k_levels, v_levels, lengths)` exactly as `QKVRotaryW8Q` does, the cache's bookkeeping and
    `lengths.add_(T)` included.  `rope_epilogue` (extra state, kept only when it is not None; True / False / None:
    `torchlsq.functional.W4A8_ROPE_EPILOGUE_DEFAULT`): where it resolves to True, x has at most 16 rows, `qkv` is a plain
    `PackedLinearA8Q` without ReLU and `rotary` has an output quantizer, the half style and qkv's `mid_dtype`, the projection, the
    rotation and the append are ONE op; calls it does not serve run the children one by one inside it.  Inference only."""

    def __init__(self, qkv, rotary, heads, kv_heads, rope_epilogue=None):
        torch.nn.Module.__init__(self)
        assert isinstance(qkv, PackedLinearA8Q) and isinstance(rotary, RotaryW8Q), "QKVRotaryPackedA8Q takes a PackedLinearA8Q and a RotaryW8Q"
        self.heads, self.kv_heads = int(heads), int(kv_heads)
        assert qkv.out_features == (self.heads + 2 * self.kv_heads) * rotary.dim, \
            "QKVRotaryPackedA8Q: qkv has %d output features, (heads + 2 kv_heads) dim = %d are needed" % (
                qkv.out_features, (self.heads + 2 * self.kv_heads) * rotary.dim)
        self.qkv, self.rotary = qkv, rotary
        self.rope_epilogue = rope_epilogue

    def _in_epilogue(self, x, cache):
        """the one op on the cache's own buffers, then the cache's bookkeeping as `append` does it"""
        m, r = self.qkv, self.rotary
        paged = hasattr(cache, "block_table")
        kc, vc = (cache.k_pool, cache.v_pool) if paged else (cache.k, cache.v)
        v = m._wrap(vc)                             # the constants of the qkv levels, formed on the device once per call
        lv = torch.ops.torchlsq.lsq_linear_packed_q8_rope_q(
            x.levels, x.scale, x.zero_point, m.codes, m.scale.reshape(-1), m.zero_point.reshape(-1), m.bias, m.group_size, m.bits,
            m.output_scale, m.output_shift, *m.output_range, v.scale, v.zero_point, r.cos, r.sin, *r._out("output"), r.mid_dtype, self.heads,
            self.kv_heads, kc, vc, cache.lengths, cache.block_table if paged else None)
        rq = _levels_out(lv, r.output_scale.detach().reshape(-1)[:1], r.output_shift.detach().reshape(-1)[:1], r.output_range)
        cache._keep("_k_side", LevelsTensor(kc, rq.scale, rq.zero_point, *r.output_range))
        cache._keep("_v_side", v)
        cache.lengths.add_(int(x.shape[1]))
        return rq, LevelsTensor(kc, *cache._k_side), LevelsTensor(vc, *cache._v_side), cache.lengths

    def forward(self, x, cache):
        x = _as_levels(x)
        m, r = self.qkv, self.rotary
        takes = F.W4A8_ROPE_EPILOGUE_DEFAULT if self.rope_epilogue is None else self.rope_epilogue
        if isinstance(x, LevelsTensor) and x.levels.dim() == 3 and _takes_decode(takes, x.levels) and \
                type(m) is PackedLinearA8Q and not m.relu and r.output_range is not None and not r.interleaved and m.mid_dtype == r.mid_dtype:
            return self._in_epilogue(x, cache)
        qkv = m(x)
        B, T = int(qkv.shape[0]), int(qkv.shape[1])
        lv = qkv.levels.view(B, T, self.heads + 2 * self.kv_heads, r.dim)
        q, k, v = (LevelsTensor(lv[:, :, a:b], qkv.scale, qkv.zero_point, qkv.quant_min, qkv.quant_max, qkv.type_min, qkv.type_max)
                   for a, b in ((0, self.heads), (self.heads, self.heads + self.kv_heads), (self.heads + self.kv_heads, lv.shape[2])))
        rq = r(q, positions=cache.lengths)
        return (rq,) + tuple(cache.append(k, v, rotary=r))
