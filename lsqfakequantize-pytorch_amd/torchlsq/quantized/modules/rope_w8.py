"""Modules that keep a decoder block in 8-bit LEVELS between the qkv projection and the attention core: `RotaryW8Q` (rotary position
embedding, `torchlsq.functional.lsq_rope_w8_q`) and `KVCacheW8` (a [B, Hkv, Tmax, D] cache of k and v levels whose lengths live on
the device) -- liblsq_hip_rope_w8.so on the GPU.  The forwards take `LevelsTensor`s of [B, T, H, D]; positions and lengths are int32
tensors on the device that the kernels read, nothing is read back to the host, and a decode step can be captured in a graph
(DESIGN.md 9.19).
"""
import torch
from torch import nn

from torchlsq.functional import LevelsTensor, lsq_kv_append_w8, lsq_rope_tables, lsq_rope_w8, lsq_rope_w8_q
from .attn_w8 import _levels, _mid, _OutQ


class RotaryW8Q(_OutQ):
    """Rotary position embedding on a `LevelsTensor` [B, T, H, `dim`]: builds `lsq_rope_tables(rotary_dim or dim, max_positions, base,
    mid_dtype)` once and holds them as the NON-PERSISTENT buffers `cos` and `sin` (float32 [P, R / 2]; they are rebuilt, not loaded),
    and the constants of `output_quantizer` (a trained per-tensor `LSQFakeQuantizer`; None: floats of `mid_dtype`) as buffers.
    `forward(x, positions=None, out=None, scatter=False)` as `lsq_rope_w8_q`: token (b, t) is rotated at positions[b] + t.
    Inference only."""

    def __init__(self, output_quantizer, dim, max_positions, base=10000.0, rotary_dim=None, interleaved=False, mid_dtype=torch.float32):
        super().__init__()
        self.dim, self.max_positions, self.base = int(dim), int(max_positions), float(base)
        self.rotary_dim = self.dim if rotary_dim is None else int(rotary_dim)
        assert 2 <= self.rotary_dim <= self.dim and self.rotary_dim % 2 == 0, "RotaryW8Q: rotary_dim must be even, at least 2 and at most dim"
        self.interleaved, self.mid_dtype = bool(interleaved), _mid(mid_dtype)
        cos, sin = lsq_rope_tables(self.rotary_dim, self.max_positions, self.base, self.mid_dtype)
        self.register_buffer("cos", cos, persistent=False)
        self.register_buffer("sin", sin, persistent=False)
        self._set_out("output", output_quantizer, "RotaryW8Q")

    def forward(self, x, positions=None, out=None, scatter=False):
        x, = _levels("RotaryW8Q", x)
        assert x.levels.dim() == 4 and int(x.shape[-1]) == self.dim, "RotaryW8Q needs levels of [B, T, H, %d], got %s" % (self.dim, tuple(x.shape))
        if self.output_range is None:
            assert out is None and not scatter, "RotaryW8Q without an output quantizer returns floats: `out` and `scatter` are not served"
            return lsq_rope_w8(x, self.cos, self.sin, self.mid_dtype, positions, self.interleaved)
        return lsq_rope_w8_q(x, self.cos, self.sin, *self._out("output"), self.mid_dtype, positions, self.interleaved, out=out, scatter=scatter)

    def extra_repr(self):
        return "dim=%d, rotary_dim=%d, max_positions=%d, base=%g, %s, %s, mid_dtype=%s" % (
            self.dim, self.rotary_dim, self.max_positions, self.base, "interleaved" if self.interleaved else "half",
            "output levels %d..%d" % self.output_range[:2] if self.output_range else "floats out", str(self.mid_dtype).replace("torch.", ""))


class KVCacheW8(nn.Module):
    """A KV cache in 8-bit levels: the buffers `k` and `v` [batch, kv_heads, max_len, dim] (`k_dtype`, `v_dtype`: torch.uint8 or
    torch.int8) and `lengths` (int32 [batch], the tokens written so far), all on `device`.

    `append(k, v, rotary=None)` takes a step's `LevelsTensor`s [B, T, Hkv, D] and
      1. writes k at `lengths`: with `rotary` (a `RotaryW8Q` with an output quantizer) the rotation and the scatter are ONE launch,
         straight into the cache; without it k is copied as it is;
      2. writes v by `lsq_kv_append_w8`;
      3. `lengths.add_(T)`,
    and returns `(k_levels, v_levels, lengths)`: the whole caches as `LevelsTensor`s [B, Hkv, Tmax, D] and the new lengths, ready for
    `AttentionCoreW8Q(causal=True).forward(q, k_levels, v_levels, key_lengths=lengths)` -- slots beyond a batch's length are never
    looked at.  The caches take their constants (scale and zero point tensors, ranges) from the FIRST append and assert the ranges
    afterwards; the constants' tensors are held, not copied, as plain attributes and not as buffers: `reset()` does not clear them,
    `.to(device)` of the module does not move them, and a later append whose scale or zero point differs is NOT noticed -- its
    levels are labelled with the first append's constants.  One cache serves one pair of quantizers; build a new cache for another.
    Tokens beyond `max_len` are not written (the kernels skip them).
    `reset()` zeroes `lengths`.  Nothing is read back to the host: a decode step can be captured in a graph.  Inference only."""

    def __init__(self, batch, kv_heads, max_len, dim, k_dtype=torch.uint8, v_dtype=torch.uint8, device=None):
        super().__init__()
        assert k_dtype in (torch.uint8, torch.int8) and v_dtype in (torch.uint8, torch.int8), "KVCacheW8 holds uint8 or int8 levels"
        shape = (int(batch), int(kv_heads), int(max_len), int(dim))
        self.register_buffer("k", torch.zeros(shape, dtype=k_dtype, device=device))
        self.register_buffer("v", torch.zeros(shape, dtype=v_dtype, device=device))
        self.register_buffer("lengths", torch.zeros(shape[0], dtype=torch.int32, device=device))
        self._k_side = self._v_side = None

    @staticmethod
    def _side(x):
        return (x.scale, x.zero_point, x.quant_min, x.quant_max, x.type_min, x.type_max)

    def _keep(self, name, x):
        side = getattr(self, name)
        if side is None:
            setattr(self, name, self._side(x))
        else:
            assert side[2:] == self._side(x)[2:], "KVCacheW8: the level range %s differs from the cache's %s" % (self._side(x)[2:], side[2:])

    def append(self, k, v, rotary=None):
        k, v = _levels("KVCacheW8", k, v)
        B, H, Tmax, D = (int(n) for n in self.k.shape)
        for name, x in (("k", k), ("v", v)):
            assert x.levels.dim() == 4 and (int(x.shape[0]), int(x.shape[2]), int(x.shape[3])) == (B, H, D), \
                "KVCacheW8: %s must be [%d, T, %d, %d], got %s" % (name, B, H, D, tuple(x.shape))
        assert k.shape[1] == v.shape[1], "KVCacheW8: k and v must hold the same tokens"
        kc, vc = self.k.permute(0, 2, 1, 3), self.v.permute(0, 2, 1, 3)          # [B, Tmax, H, D] views of the caches
        if rotary is not None:
            assert rotary.output_range is not None, "KVCacheW8: `rotary` needs an output quantizer"
            kr = rotary(k, positions=self.lengths, out=kc, scatter=True)
        else:
            kr = lsq_kv_append_w8(k, kc, positions=self.lengths, scatter=True)
        vr = lsq_kv_append_w8(v, vc, positions=self.lengths, scatter=True)
        self._keep("_k_side", kr)
        self._keep("_v_side", vr)
        self.lengths.add_(int(k.shape[1]))
        return (LevelsTensor(self.k, *self._k_side), LevelsTensor(self.v, *self._v_side), self.lengths)

    def reset(self):
        self.lengths.zero_()

    def extra_repr(self):
        return "batch=%d, kv_heads=%d, max_len=%d, dim=%d, k %s, v %s" % (tuple(self.k.shape) + (str(self.k.dtype).replace("torch.", ""),
                                                                                              str(self.v.dtype).replace("torch.", "")))
