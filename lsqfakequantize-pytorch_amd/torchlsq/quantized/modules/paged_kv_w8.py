"""`PagedKVCacheW8`: a KV cache in 8-bit LEVELS held as fixed-size pages of one pool with a block table per sequence -- what a serving
loop hands out --, written by `torchlsq.functional.lsq_kv_append_paged_w8` and read in place by
`AttentionCoreW8Q.forward(..., block_table=...)` (`lsq_attention_decode_paged_w8_q`), liblsq_hip_attn_paged_w8.so on the GPU.  The
block table, the lengths and the pools live on the device, nothing is read back to the host, and a decode step can be captured in a
graph.  Which page a sequence gets is the owner's policy: the module only holds the table.
"""
import torch
from torch import nn

from torchlsq.functional import LevelsTensor, lsq_kv_append_paged_w8
from .attn_w8 import _levels


class PagedKVCacheW8(nn.Module):
    """A paged KV cache in 8-bit levels.  Buffers, all on `device`: `k_pool` and `v_pool`, logically [num_pages, kv_heads, page_size,
    dim] (`k_dtype`, `v_dtype`: torch.uint8 or torch.int8; with `page_major=False` they are the `.permute(0, 2, 1, 3)` views of
    storage in the order [num_pages, page_size, kv_heads, dim]), `block_table` (int32 [batch, max_pages]) and `lengths` (int32 [batch],
    the tokens written so far).  By default page i of sequence b is `i * batch + b` where that is below `num_pages`, else -1; the
    owner overwrites `block_table` in place with torch ops (sequences may share pages).

    `append(k, v, rotary=None)` mirrors `KVCacheW8.append`: a step's `LevelsTensor`s [B, T, Hkv, D]; with `rotary` (a `RotaryW8Q` with
    an output quantizer) k is first rotated at `lengths` into a [B, T, Hkv, D] buffer (one launch; the rotation fused into the paged
    write is not served; `rotary`'s tables must cover the positions written, since a position beyond them is not rotated and leaves
    its row of that buffer as allocated), then k and v are written by `lsq_kv_append_paged_w8` (one launch) and `lengths.add_(T)`.  A token beyond
    `max_pages * page_size` or whose entry lies outside 0 .. num_pages - 1 is not written.  Returns `(k_pool, v_pool, lengths)`: the
    pools as `LevelsTensor`s [Np, Hkv, ps, D] and the new lengths, ready for `AttentionCoreW8Q(decode=True, causal=True).forward(q,
    k_pool, v_pool, key_lengths=lengths, block_table=cache.block_table)`.  The constants are kept as in `KVCacheW8`: taken from the
    first append, plain attributes.  `reset()` zeroes `lengths`.  Nothing is read back to the host.  Inference only."""

    def __init__(self, num_pages, kv_heads, page_size, dim, batch, max_pages, k_dtype=torch.uint8, v_dtype=torch.uint8, page_major=True,
                 device=None):
        super().__init__()
        assert k_dtype in (torch.uint8, torch.int8) and v_dtype in (torch.uint8, torch.int8), "PagedKVCacheW8 holds uint8 or int8 levels"
        Np, Hkv, ps, D, B, Mp = (int(n) for n in (num_pages, kv_heads, page_size, dim, batch, max_pages))
        assert min(Np, Hkv, ps, D, B, Mp) >= 1, "PagedKVCacheW8: every extent must be at least 1"
        self.page_major = bool(page_major)
        shape = (Np, Hkv, ps, D) if self.page_major else (Np, ps, Hkv, D)
        for name, dt in (("k_pool", k_dtype), ("v_pool", v_dtype)):
            store = torch.zeros(shape, dtype=dt, device=device)
            self.register_buffer(name, store if self.page_major else store.permute(0, 2, 1, 3))
        table = torch.arange(Mp, dtype=torch.int64).reshape(1, Mp) * B + torch.arange(B, dtype=torch.int64).reshape(B, 1)
        table = torch.where(table < Np, table, torch.full_like(table, -1)).to(torch.int32)
        self.register_buffer("block_table", table.to(device) if device is not None else table)
        self.register_buffer("lengths", torch.zeros(B, dtype=torch.int32, device=device))
        self._k_side = self._v_side = None

    @staticmethod
    def _side(x):
        return (x.scale, x.zero_point, x.quant_min, x.quant_max, x.type_min, x.type_max)

    def _keep(self, name, x):
        side = getattr(self, name)
        if side is None:
            setattr(self, name, self._side(x))
        else:
            assert side[2:] == self._side(x)[2:], "PagedKVCacheW8: the level range %s differs from the cache's %s" % (self._side(x)[2:], side[2:])

    def append(self, k, v, rotary=None):
        k, v = _levels("PagedKVCacheW8", k, v)
        Np, Hkv, ps, D = (int(n) for n in self.k_pool.shape)
        B = int(self.lengths.shape[0])
        for name, x in (("k", k), ("v", v)):
            assert x.levels.dim() == 4 and (int(x.shape[0]), int(x.shape[2]), int(x.shape[3])) == (B, Hkv, D), \
                "PagedKVCacheW8: %s must be [%d, T, %d, %d], got %s" % (name, B, Hkv, D, tuple(x.shape))
        assert k.shape[1] == v.shape[1], "PagedKVCacheW8: k and v must hold the same tokens"
        if rotary is not None:
            assert rotary.output_range is not None, "PagedKVCacheW8: `rotary` needs an output quantizer"
            k = rotary(k, positions=self.lengths)
        kp, vp = lsq_kv_append_paged_w8(k, v, self.k_pool, self.v_pool, self.block_table, positions=self.lengths)
        self._keep("_k_side", kp)
        self._keep("_v_side", vp)
        self.lengths.add_(int(k.shape[1]))
        return (LevelsTensor(self.k_pool, *self._k_side), LevelsTensor(self.v_pool, *self._v_side), self.lengths)

    def reset(self):
        self.lengths.zero_()

    def extra_repr(self):
        Np, Hkv, ps, D = (int(n) for n in self.k_pool.shape)
        return "num_pages=%d, kv_heads=%d, page_size=%d, dim=%d, batch=%d, max_pages=%d, k %s, v %s, %s" % (
            Np, Hkv, ps, D, int(self.lengths.shape[0]), int(self.block_table.shape[1]), str(self.k_pool.dtype).replace("torch.", ""),
            str(self.v_pool.dtype).replace("torch.", ""), "[Np, Hkv, ps, D]" if self.page_major else "[Np, ps, Hkv, D]")
