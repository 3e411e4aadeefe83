"""Modules that keep the attention core of a converted token block in 8-bit LEVELS: `MatmulW8Q` (where a block calls a
`FloatFunctional.matmul`), `SoftmaxW8Q` (which builds and owns the integer table) and `AttentionCoreW8Q` (softmax(q k^T) v in three
launches, or with `fused=True` in one: `lsq_attention_w8_q`, liblsq_hip_attn_fused_w8.so) -- `torchlsq.functional.lsq_bmm_w8_q` /
`lsq_softmax_w8_q`, liblsq_hip_attn_w8.so on the GPU.  The forwards take
`LevelsTensor`s; nothing is read back to the host, and the chain can be captured in a graph.  There is no converter: attention
blocks differ too much in how they spell the core, so a block is rewritten by hand around these modules.

The softmax is the package's own definition (include/lsq_hip_attn_w8.h), not ATen's: against the unfused
`dequantize -> F.softmax -> levels` at most one level differs.

MASKS: `SoftmaxW8Q` and `AttentionCoreW8Q` take `causal=` at construction and `key_lengths=` in the forward; a masked
call goes through `torchlsq.functional.lsq_masked_softmax_w8_q` (liblsq_hip_attn_mask_w8.so), an unmasked one through exactly the ops
it went through before.

DECODE: `AttentionCoreW8Q(decode=True)` sends every forward through `torchlsq.functional.lsq_attention_decode_w8_q`
(liblsq_hip_attn_decode_w8.so): k and v may have fewer heads than q (grouped-query attention, read from the cache in place), one
launch, and nothing at or beyond a row's key count is read.

PREFILL: `AttentionCoreW8Q(prefill=True)` sends every forward through `torchlsq.functional.lsq_attention_prefill_w8_q`
(liblsq_hip_attn_prefill_w8.so): the same definition for any number of query rows -- the prompt in one launch of the prefill kernel,
the steps in one launch of the decode kernel, through one module instance.
"""
import torch
from torch import nn

from torchlsq.functional import (LevelsTensor, _act_constants, lsq_attention_chunk_w8_q, lsq_attention_decode_paged_w8_q, lsq_attention_decode_w8_q, lsq_attention_prefill_w8_q, lsq_attention_w8_q, lsq_bmm_w8, lsq_bmm_w8_q,
                                 lsq_masked_softmax_w8, lsq_masked_softmax_w8_q, lsq_softmax_table, lsq_softmax_w8, lsq_softmax_w8_q)
from .packed_linear_a8 import _per_tensor_constants
from .w8a8_q import _MID_DTYPES, _as_levels


def _mid(mid_dtype):
    assert mid_dtype in _MID_DTYPES.values(), "mid_dtype must be torch.float32, torch.bfloat16 or torch.float16"
    return mid_dtype


class _OutQ(nn.Module):
    """buffers `<name>_scale` and `<name>_shift` (float32 [1]) and the range of one trained per-tensor output quantizer, or none"""

    def _set_out(self, name, quantizer, what):
        if quantizer is None:
            setattr(self, name + "_range", None)
            self.register_buffer(name + "_scale", torch.ones(1, dtype=torch.float32))
            self.register_buffer(name + "_shift", torch.zeros(1, dtype=torch.float32))
            return
        scale, shift, *rng = _per_tensor_constants(quantizer, "%s (%s quantizer)" % (what, name))
        self.register_buffer(name + "_scale", scale)
        self.register_buffer(name + "_shift", shift)
        setattr(self, name + "_range", tuple(rng))

    def _out(self, name):
        return (getattr(self, name + "_scale"), getattr(self, name + "_shift")) + getattr(self, name + "_range")


def _levels(what, *xs):
    xs = tuple(_as_levels(x) for x in xs)
    assert all(isinstance(x, LevelsTensor) for x in xs), "%s reads levels: LevelsTensors or per-tensor quantized tensors" % what
    return xs


class MatmulW8Q(_OutQ):
    """`torch.matmul(a, b)` (`transpose_b`: of a and b^T) on two `LevelsTensor`s: one launch, a `LevelsTensor` of
    `output_quantizer` (a trained per-tensor `LSQFakeQuantizer`; None: floats of `mid_dtype`).  Inference only."""

    def __init__(self, output_quantizer=None, transpose_b=False, mid_dtype=torch.float32):
        super().__init__()
        self.transpose_b, self.mid_dtype = bool(transpose_b), _mid(mid_dtype)
        self._set_out("output", output_quantizer, "MatmulW8Q")

    def forward(self, a, b, out=None):
        a, b = _levels("MatmulW8Q", a, b)
        if self.output_range is None:
            return lsq_bmm_w8(a, b, self.transpose_b, self.mid_dtype)
        return lsq_bmm_w8_q(a, b, self.transpose_b, *self._out("output"), self.mid_dtype, out=out)

    matmul = forward

    def extra_repr(self):
        return "transpose_b=%s, %s, mid_dtype=%s" % (self.transpose_b, "output levels %d..%d" % self.output_range[:2]
                                                     if self.output_range else "floats out", str(self.mid_dtype).replace("torch.", ""))


class SoftmaxW8Q(_OutQ):
    """Softmax over the last axis of a `LevelsTensor` of `input_quantizer` (a trained per-tensor `LSQFakeQuantizer`, or the float32
    [1] scale of the incoming `LevelsTensor`): builds `lsq_softmax_table(s_x, alpha)` once, on the quantizer's device, and owns it
    as the buffer `table` (int32 [256]).  `alpha` carries attention's 1 / sqrt(D).  Returns a `LevelsTensor` of `output_quantizer`
    (None: floats of `mid_dtype`); `row_pad` as in `lsq_softmax_w8_q`.  `causal` (an attribute, not a buffer: False / None, True or
    an offset, as in `lsq_masked_softmax_w8_q`) and the forward's `key_lengths` (int32 [x.shape[0]] on x's device) mask a row to a
    prefix of its keys; with neither, the unmasked op runs as before.  Inference only."""

    causal = False          # (the default of a module pickled before the attribute existed)

    def __init__(self, input_quantizer, output_quantizer=None, alpha=1.0, mid_dtype=torch.float32, row_pad=16, causal=False):
        super().__init__()
        self.alpha, self.mid_dtype, self.row_pad = float(alpha), _mid(mid_dtype), int(row_pad)
        self.causal = causal
        if isinstance(input_quantizer, torch.Tensor):
            s_x = input_quantizer.detach().reshape(-1)[:1].to(torch.float32)
        else:
            scale, shift, _, _, tmin, tmax = _per_tensor_constants(input_quantizer, "SoftmaxW8Q (input quantizer)")
            s_x = _act_constants(scale, shift, tmin, tmax)[0]
        self.register_buffer("table", lsq_softmax_table(s_x, self.alpha))
        self._set_out("output", output_quantizer, "SoftmaxW8Q")

    def forward(self, x, out=None, key_lengths=None):
        x, = _levels("SoftmaxW8Q", x)
        if key_lengths is not None or (self.causal is not None and self.causal is not False):
            if self.output_range is None:
                return lsq_masked_softmax_w8(x, self.table, self.mid_dtype, causal=self.causal, key_lengths=key_lengths)
            return lsq_masked_softmax_w8_q(x, self.table, *self._out("output"), self.mid_dtype, causal=self.causal, key_lengths=key_lengths,
                                           out=out, row_pad=self.row_pad)
        if self.output_range is None:
            return lsq_softmax_w8(x, self.table, self.mid_dtype)
        return lsq_softmax_w8_q(x, self.table, *self._out("output"), self.mid_dtype, out=out, row_pad=self.row_pad)

    def extra_repr(self):
        return "alpha=%g, %s, mid_dtype=%s%s" % (self.alpha, "output levels %d..%d" % self.output_range[:2] if self.output_range
                                                 else "floats out", str(self.mid_dtype).replace("torch.", ""),
                                                 "" if self.causal is None or self.causal is False else ", causal=%r" % (self.causal,))


class AttentionCoreW8Q(nn.Module):
    """softmax(alpha q k^T) v on levels: q, k, v `LevelsTensor`s [B, H, T, D] (views of one qkv buffer are read in place) -> a
    `LevelsTensor` [B, T, H D] of `out_quantizer`, in three launches: the scores q k^T as levels of `scores_quantizer`, their
    softmax through the table of (`scores_quantizer`'s scale, `alpha`) as levels of `probs_quantizer` in rows padded to 16
    bytes, and p v written through the [B, H, T, D] view of the result.  The three quantizers are trained per-tensor
    `LSQFakeQuantizer`s.  The two matmuls write into buffers this module allocates (`out=`), so they call the host functions
    directly and not `torch.ops.torchlsq.lsq_bmm_w8_q8_q`: the same checks and kernels run, graph capture works, but the ops' fake
    kernels and their Autograd kernels that refuse grad do not cover the core; the softmax goes through its op.

    `fused=True` (opt-in; an attribute, not a buffer: the `state_dict` is the same) sends the same constants and the same table
    through `torchlsq.functional.lsq_attention_w8_q` instead: ONE launch where liblsq_hip_attn_fused_w8.so serves the shape (the scores
    and probabilities stay in LDS), the three launches elsewhere -- the same bytes either way, and q and k, v may differ in T.

    MASKS.  `causal` (an attribute, not a buffer; as in `lsq_masked_softmax_w8_q`: True lets the last query see every key) and the
    forward's `key_lengths` (int32 [B] on q's device, read in the kernel) mask the softmax.  A masked call ALWAYS runs three
    launches, also with `fused=True`, and accepts k and v of [B, H, Tk, D] with Tk != Tq (decode: Tq = 1): the scores matmul still
    computes all Tk columns, the masked softmax writes the probability quantizer's level of 0 beyond a row's prefix, and p v is
    the existing matmul on those bytes.  With neither, nothing changes in bytes or in the ops called.

    DECODE.  `decode=True` (opt-in; an attribute, not a buffer: the `state_dict` is the same) sends EVERY forward, masked or not,
    through `torchlsq.functional.lsq_attention_decode_w8_q` with the same constants, the same table, `causal` and `key_lengths`:
    k and v are [B, Hkv, Tk, D] with Hkv dividing H (query head h reads kv head h // (H / Hkv); the buffers of `KVCacheW8` as they
    are), one launch where liblsq_hip_attn_decode_w8.so serves the shape, and keys at or beyond a row's count are never read.  The
    bytes are those of `decode=False` on `repeat_interleave`d k and v whenever the probabilities quantizer's level of 0.0 equals its
    zero point (shift 0).  With `decode=False` nothing changes, including the assertion that refuses Hkv != H.

    PREFILL.  `prefill=True` (opt-in; an attribute, not a buffer: the `state_dict` is the same) sends EVERY forward through
    `torchlsq.functional.lsq_attention_prefill_w8_q` instead, with the same constants, table, `causal` and `key_lengths`: the
    definition, the operands and the bytes of `decode=True` for any number of query rows.  On the GPU a prompt takes ONE launch of
    liblsq_hip_attn_prefill_w8.so (no `repeat_interleave`, no score tensor in memory, nothing above the diagonal computed) and a
    step with (H / Hkv) Tq <= 16 one launch of the decode kernel, so one module instance serves both (set `causal` per call: an
    offset for the prompt, True for the steps).  With `prefill=False` nothing changes, for any combination of `fused` and `decode`.

    SPLIT.  `split` (opt-in; an attribute, not a buffer: the `state_dict` is the same; None, "auto" or an int >= 1 as
    in `lsq_attention_decode_w8_q`) sends a forward with (H / Hkv) Tq <= 16 through `lsq_attention_decode_w8_q(..., split=split)`,
    whichever of `decode` / `prefill` is on: one kv head's keys dealt to several workgroups (liblsq_hip_attn_decode_split_w8.so), the
    same bytes.  A forward with more rows, and every forward with `split=None`, goes where it went before.

    PAGED.  `forward(q, k, v, key_lengths=None, block_table=None)`: with a `block_table` (int32 [B, Mp] on q's device)
    and `decode` or `prefill` on, k and v are the POOLS of a paged cache, `LevelsTensor`s [Np, Hkv, ps, D] (`PagedKVCacheW8`'s), and
    the forward goes through `lsq_attention_decode_paged_w8_q` (liblsq_hip_attn_paged_w8.so) with the same constants, table, `causal`
    and `key_lengths`; `split`, where it is an int, gives `splits`, otherwise `splits` is 0 (the library's chunk).  Without a block
    table nothing changes.

    CHUNK.  `chunk=True` (opt-in; an attribute, not a buffer: the `state_dict` is the same) sends EVERY forward, dense
    or with a `block_table`, through `torchlsq.functional.lsq_attention_chunk_w8_q` (liblsq_hip_attn_chunk_w8.so) with the same
    constants, table, `causal` and `key_lengths`: the same definition for any number of query rows against up to 65536 keys, `split`,
    where it is an int, giving `splits` as in the paged route.  Only then may `causal` be "lengths": every row's keys are counted
    back from `key_lengths` in the kernels, so a prompt is fed in pieces into a growing cache (the lengths the caches' `append`
    returns) by one module instance, with no host read-back.  With `chunk=False` nothing changes.
    Inference only."""

    decode = False          # (the default of a module pickled before the attribute existed)
    prefill = False         # (likewise)
    split = None            # (likewise)
    chunk = False           # (likewise)

    def __init__(self, scores_quantizer, probs_quantizer, out_quantizer, alpha=1.0, mid_dtype=torch.float32, fused=False, causal=False,
                 decode=False, prefill=False, split=None, chunk=False):
        super().__init__()
        assert split is None or split == "auto" or (isinstance(split, int) and not isinstance(split, bool) and split >= 1), \
            "AttentionCoreW8Q: split must be None, \"auto\" or an int >= 1, got %r" % (split,)
        self.fused = bool(fused)
        self.decode = bool(decode)
        self.prefill = bool(prefill)
        self.split = split
        self.chunk = bool(chunk)
        self.scores = MatmulW8Q(scores_quantizer, True, mid_dtype)
        self.softmax = SoftmaxW8Q(scores_quantizer, probs_quantizer, alpha, mid_dtype, row_pad=16, causal=causal)
        self.context = MatmulW8Q(out_quantizer, False, mid_dtype)
        assert None not in (self.scores.output_range, self.softmax.output_range, self.context.output_range), \
            "AttentionCoreW8Q needs the three trained quantizers"

    @property
    def causal(self):
        return self.softmax.causal

    @causal.setter
    def causal(self, value):
        self.softmax.causal = value

    def forward(self, q, k, v, key_lengths=None, block_table=None):
        q, k, v = _levels("AttentionCoreW8Q", q, k, v)
        assert self.chunk or not isinstance(self.causal, str), \
            "AttentionCoreW8Q: causal=%r (key counts taken from key_lengths in the kernels) needs chunk=True" % (self.causal,)
        if self.chunk:
            splits = self.split if isinstance(self.split, int) and not isinstance(self.split, bool) else 0
            return lsq_attention_chunk_w8_q(q, k, v, self.softmax.table, self.scores._out("output"), self.softmax._out("output"),
                                            self.context._out("output"), self.scores.mid_dtype, causal=self.causal, key_lengths=key_lengths,
                                            block_table=block_table, splits=splits)
        if block_table is not None:
            assert self.decode or self.prefill, "AttentionCoreW8Q: a block_table (paged k and v) needs decode=True or prefill=True"
            splits = self.split if isinstance(self.split, int) and not isinstance(self.split, bool) else 0
            return lsq_attention_decode_paged_w8_q(q, k, v, block_table, self.softmax.table, self.scores._out("output"),
                                                   self.softmax._out("output"), self.context._out("output"), self.scores.mid_dtype,
                                                   causal=self.causal, key_lengths=key_lengths, splits=splits)
        if self.split is not None and (self.decode or self.prefill) and q.levels.dim() == 4 and k.levels.dim() == 4 and k.shape[1] > 0 \
                and q.shape[1] % k.shape[1] == 0 and q.shape[1] // k.shape[1] * q.shape[2] <= 16:
            return lsq_attention_decode_w8_q(q, k, v, self.softmax.table, self.scores._out("output"), self.softmax._out("output"),
                                             self.context._out("output"), self.scores.mid_dtype, causal=self.causal, key_lengths=key_lengths,
                                             split=self.split)
        if self.prefill:
            return lsq_attention_prefill_w8_q(q, k, v, self.softmax.table, self.scores._out("output"), self.softmax._out("output"),
                                              self.context._out("output"), self.scores.mid_dtype, causal=self.causal, key_lengths=key_lengths)
        if self.decode:
            return lsq_attention_decode_w8_q(q, k, v, self.softmax.table, self.scores._out("output"), self.softmax._out("output"),
                                             self.context._out("output"), self.scores.mid_dtype, causal=self.causal, key_lengths=key_lengths)
        masked = key_lengths is not None or (self.causal is not None and self.causal is not False)
        if self.fused and not masked:
            return lsq_attention_w8_q(q, k, v, self.softmax.table, self.scores._out("output"), self.softmax._out("output"),
                                      self.context._out("output"), self.scores.mid_dtype)
        if masked:
            assert q.levels.dim() == 4 and k.levels.dim() == 4 and k.shape == v.shape and q.shape[:2] == k.shape[:2] and q.shape[3] == k.shape[3], \
                "AttentionCoreW8Q (masked) needs q [B, H, Tq, D] and k, v [B, H, Tk, D], got %s, %s and %s" % (tuple(q.shape), tuple(k.shape), tuple(v.shape))
        else:
            assert q.levels.dim() == 4 and q.shape == k.shape == v.shape, \
                "AttentionCoreW8Q needs q, k and v of one shape [B, H, T, D], got %s, %s and %s" % (tuple(q.shape), tuple(k.shape), tuple(v.shape))
        B, H, T, D = (int(n) for n in q.shape)
        Tk = int(k.shape[2])
        # the scores' rows are padded to 16 bytes like the probabilities': both are then stored and read as packets for any T
        rng = self.scores.output_range
        scores = torch.empty((B, H, T, (Tk + 15) // 16 * 16), dtype=torch.uint8 if max(rng[1], rng[3]) > 127 else torch.int8, device=q.device)
        s = self.scores(q, k, out=scores[..., :Tk])
        p = self.softmax(s, key_lengths=key_lengths) if masked else self.softmax(s)
        rng = self.context.output_range
        buf = torch.empty((B, T, H * D), dtype=torch.uint8 if max(rng[1], rng[3]) > 127 else torch.int8, device=q.device)
        y = self.context(p, v, out=buf.view(B, T, H, D).permute(0, 2, 1, 3))
        return LevelsTensor(buf, y.scale, y.zero_point, y.quant_min, y.quant_max, y.type_min, y.type_max)

    def extra_repr(self):
        if self.chunk:
            return "chunk=True (lsq_attention_chunk_w8_q: three launches over row tiles of 16, dense or paged k and v)%s%s" % (
                "" if self.causal is None or self.causal is False else ", causal=%r" % (self.causal,),
                ", splits=%d" % self.split if isinstance(self.split, int) and not isinstance(self.split, bool) else "")
        split = "" if self.split is None else ", split=%r (lsq_attention_decode_w8_q(split=...) where (H / Hkv) Tq <= 16)" % (self.split,)
        return self._repr_route() + (split if self.decode or self.prefill else "")

    def _repr_route(self):
        if self.prefill:
            return "prefill=True (lsq_attention_prefill_w8_q: one launch of the prefill or the decode kernel where they serve the shape, " \
                "grouped-query k and v)%s" % ("" if self.causal is None or self.causal is False else ", causal=%r" % (self.causal,))
        if self.decode:
            return "decode=True (lsq_attention_decode_w8_q: one launch where the decode kernel serves the shape, grouped-query k and v)%s" \
                % ("" if self.causal is None or self.causal is False else ", causal=%r" % (self.causal,))
        return "fused=%s (%s)%s" % (self.fused, "lsq_attention_w8_q: one launch where the fused kernel serves the shape" if self.fused
                                    else "three launches", "" if self.causal is None or self.causal is False
                                    else ", causal=%r: masked calls run three launches" % (self.causal,))
