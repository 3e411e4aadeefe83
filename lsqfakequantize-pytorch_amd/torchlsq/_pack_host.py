"""Host layer of the packed export of group-wise weights: 4- / 2-bit codes plus one (qscale, qzero) per group, and back.

The format is the contract of include/lsq_hip_pack.h: code = level - quant_min, little-endian inside the byte (for 4 bits,
element 0 is the low nibble), qscale = max(|scale|, eps), qzero = zero point - quant_min, y = (code - qzero) * qscale.
GPU tensors go to liblsq_hip_pack.so with one ctypes call per op.  CPU tensors: the levels come from `cpu_levels` on the
[n / G, G] view (the formula of the kernels, operation by operation) and are packed / unpacked with torch integer ops into
the same bytes -- export is a conversion-time step, not a hot path on the CPU.
Checks and layout rules as in _group_host.py: the last dim is a multiple of G, one scale / shift per group in any shape, a
non-contiguous x is made contiguous, element-aligned views (x[1:]) run in place.
"""
import ctypes

import torch

from . import _abi
from ._abi import _DTYPE_CODE, _assert_has_ops, pack_library
from ._cpu_host import _require_cpu, cpu_levels
from ._group_host import check_group_args
from ._hip_host import _check, _on_device, _param_dtype, _params, _require_gpu, _stream_of, check_forward_dtypes


def check_pack_format(what, bits, group_size, qmin=None, qmax=None):
    _check(bits in (2, 4), "%s: bits must be 4 or 2, got %r" % (what, bits))
    _check(isinstance(group_size, int) and group_size >= 1, "%s: group_size must be a positive integer" % what)
    _check(group_size % (8 // bits) == 0,
           "%s: group_size %d is not a multiple of %d, the elements of one byte of %d-bit codes (a group must start on a "
           "byte boundary)" % (what, group_size, 8 // bits, bits))
    if qmin is not None:
        _check(0 <= qmax - qmin <= 2 ** bits - 1,
               "%s: the range [%d, %d] has more than the %d levels of %d-bit codes" % (what, qmin, qmax, 2 ** bits, bits))


def _pack_status(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, _abi._PACK_LIB.lsq_pack_last_error().decode("utf-8", "replace")))


def _pack_bytes(codes, bits):
    """[..., K] codes (uint8 values below 2^bits) -> [..., K * bits / 8] bytes, element 0 in the low bits"""
    per = 8 // bits
    c = codes.reshape(codes.shape[:-1] + (codes.shape[-1] // per, per)).to(torch.int32)
    out = c[..., 0]
    for j in range(1, per):
        out = out | (c[..., j] << (j * bits))
    return out.to(torch.uint8)


def _unpack_bytes(packed, bits):
    """[..., B] bytes -> [..., B * 8 / bits] codes as int32"""
    per = 8 // bits
    p = packed.to(torch.int32)
    parts = [(p >> (j * bits)) & (2 ** bits - 1) for j in range(per)]
    return torch.stack(parts, dim=-1).reshape(packed.shape[:-1] + (packed.shape[-1] * per,))


def pack_quantize(x, scale, shift, group_size, bits, qmin, qmax, tmin, tmax):
    """(codes, qscale, qzero): uint8 codes of shape x.shape[:-1] + (x.shape[-1] * bits / 8,), qscale (float32; float64 for a
    float64 x) and qzero (int32) in scale's shape"""
    what = "lsq_pack_per_group"
    _assert_has_ops()
    check_forward_dtypes(x, scale, shift)
    check_pack_format(what, bits, group_size, qmin, qmax)
    _check(all(abs(int(v)) <= 2 ** 23 for v in (qmin, qmax, tmin, tmax)),
           "%s: quant_min, quant_max, type_min and type_max must lie within +-2^23" % what)      # exact integers in fp32
    check_group_args(x, scale, shift, group_size)
    shape = x.shape[:-1] + (x.size(-1) * bits // 8,)
    pd = _param_dtype(x)
    if not x.is_cuda:
        _require_cpu(what, x, scale, shift)
        rows = x.numel() // group_size
        s, b = scale.detach().reshape(-1), shift.detach().reshape(-1)
        levels = cpu_levels(x.detach().reshape(rows, group_size), s, b, 0, True, qmin, qmax, tmin, tmax, qmin)
        codes = _pack_bytes(levels.view(torch.uint8).reshape(-1), bits)      # level - quant_min: the code, 0 .. 2^bits - 1
        qscale = torch.fmax(torch.full_like(s, torch.finfo(pd).eps), s.abs())
        zp = torch.fmin(torch.full_like(s, tmax), torch.fmax(torch.full_like(s, tmin), -b * (1.0 / qscale))).round()
        return codes.reshape(shape), qscale.reshape(scale.shape), (zp.to(torch.int64) - qmin).to(torch.int32).reshape(scale.shape)
    lib = pack_library()
    _require_gpu(what, x, scale, shift)
    xd, sc, sh = x.contiguous(), scale.contiguous(), shift.contiguous()
    codes = torch.empty(shape, dtype=torch.uint8, device=x.device)
    qscale = torch.empty(scale.shape, dtype=pd, device=x.device)
    qzero = torch.empty(scale.shape, dtype=torch.int32, device=x.device)
    if xd.numel() == 0:
        return codes, qscale, qzero
    _, pref = _params(qmin, qmax, tmin, tmax, True, 1.0, False, False, False)
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_pack_quantize, _DTYPE_CODE[x.dtype], xd.data_ptr(), xd.numel(), group_size, sc.data_ptr(),
                    sh.data_ptr(), pref, bits, codes.data_ptr(), qscale.data_ptr(), qzero.data_ptr(), _stream_of(idx))
    if rc:
        _pack_status(rc, "lsq_pack_quantize")
    return codes, qscale, qzero


def _check_packed(what, codes, qscale, qzero, group_size, bits):
    """the element count of [..., B] codes, after the checks the three readers share"""
    check_pack_format(what, bits, group_size)
    _check(codes.dtype == torch.uint8 and codes.dim() >= 1, "%s: codes must be a uint8 tensor with at least one dimension" % what)
    n = codes.numel() * (8 // bits)
    _check((codes.size(-1) * (8 // bits)) % group_size == 0,
           "%s: the last dimension (%d elements) is not a multiple of group_size %d" % (what, codes.size(-1) * (8 // bits), group_size))
    if qscale is not None:
        _check(qscale.dtype in (torch.float32, torch.float64) and qzero.dtype == torch.int32,
               "%s: scale must be float32 or float64 and zero_point int32" % what)
        _check(qscale.numel() == n // group_size and qzero.numel() == n // group_size,
               "%s: scale and zero_point need %d elements, got %d and %d" % (what, n // group_size, qscale.numel(), qzero.numel()))
    return n


def pack_dequantize(codes, qscale, qzero, group_size, bits, dtype):
    """the fake-quantized values of `dtype`, shape codes.shape[:-1] + (codes.shape[-1] * 8 / bits,)"""
    what = "lsq_dequantize_per_group"
    _assert_has_ops()
    n = _check_packed(what, codes, qscale, qzero, group_size, bits)
    _check(dtype in _DTYPE_CODE, "%s: not implemented for '%s'" % (what, str(dtype).replace("torch.", "")))
    _check((torch.float64 if dtype == torch.float64 else torch.float32) == qscale.dtype,
           "%s: a float64 scale dequantizes to float64, a float32 scale to float32, bfloat16 or float16" % what)
    shape = codes.shape[:-1] + (codes.size(-1) * (8 // bits),)
    if not codes.is_cuda:
        _require_cpu(what, codes, qscale, qzero)
        c = _unpack_bytes(codes.reshape(-1), bits).reshape(-1, group_size).to(qscale.dtype)
        y = (c - qzero.reshape(-1, 1).to(qscale.dtype)) * qscale.reshape(-1, 1)
        return y.to(dtype).reshape(shape)
    lib = pack_library()
    _require_gpu(what, codes, qscale, qzero)
    cd, qs, qz = codes.contiguous(), qscale.contiguous(), qzero.contiguous()
    y = torch.empty(shape, dtype=dtype, device=codes.device)
    if n == 0:
        return y
    idx = codes.device.index
    rc = _on_device(idx, lib.lsq_pack_dequantize, _DTYPE_CODE[dtype], cd.data_ptr(), n, group_size, bits, qs.data_ptr(),
                    qz.data_ptr(), y.data_ptr(), _stream_of(idx))
    if rc:
        _pack_status(rc, "lsq_pack_dequantize")
    return y


def pack_unpack(codes, bits, quant_min, level_bias):
    """one int8 byte per element, (code + quant_min - level_bias) mod 256: what lsq_levels_per_group returns"""
    what = "lsq_unpack_per_group"
    _assert_has_ops()
    _check(bits in (2, 4), "%s: bits must be 4 or 2, got %r" % (what, bits))
    n = _check_packed(what, codes, None, None, 8 // bits, bits)       # no group structure: any whole number of bytes
    lo = quant_min - level_bias
    hi = lo + 2 ** bits - 1
    _check((lo >= -128 and hi <= 127) or (lo >= 0 and hi <= 255),
           "%s: levels: [quant_min, quant_min + %d] - level_bias = [%d, %d] fits neither int8 nor uint8" % (what, 2 ** bits - 1, lo, hi))
    shape = codes.shape[:-1] + (codes.size(-1) * (8 // bits),)
    if not codes.is_cuda:
        return ((_unpack_bytes(codes.reshape(-1), bits) + lo) & 0xff).to(torch.uint8).view(torch.int8).reshape(shape)
    lib = pack_library()
    cd = codes.contiguous()
    levels = torch.empty(shape, dtype=torch.int8, device=codes.device)
    if n == 0:
        return levels
    idx = codes.device.index
    rc = _on_device(idx, lib.lsq_pack_unpack, cd.data_ptr(), n, bits, quant_min, level_bias, levels.data_ptr(), _stream_of(idx))
    if rc:
        _pack_status(rc, "lsq_pack_unpack")
    return levels


def pack_plan(dtype, n, group_size, bits):
    """The launches liblsq_hip_pack.so makes for (dtype, n, G, bits) -- host only, nothing is launched (lsq_pack_plan)."""
    lib = pack_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_pack_plan(_DTYPE_CODE[dtype], int(n), int(group_size), int(bits), ctypes.byref(out))
    if rc:
        _pack_status(rc, "lsq_pack_plan")
    return dict(quantize_grid=out[0], dequantize_grid=out[1], unpack_grid=out[2], block=out[3],
                quantize_form="packet" if out[4] else "byte", dequantize_form="packet" if out[5] else "element",
                quantize_elems=out[6], dequantize_elems=out[7])
