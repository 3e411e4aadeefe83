"""Host layer of the DECODE SHAPE of the W8A8 linears with an 8-bit output (include/lsq_hip_lindec_w8.h): the ops
`lsq_linear_w8_q8_dec_q` and `lsq_linear_w8_q8_dec_add_q` have the schemas of `lsq_linear_w8_q8_q` / `lsq_linear_w8_q8_add_q` and,
bit for bit, their results -- nothing new is defined.  What differs is the kernel a GPU call runs: when the flattened x has at most
16 rows, K % 16 == 0, K <= 65536 and the levels and the weight are 16-byte aligned, ONE ctypes call into liblsq_hip_lindec_w8.so
(16 waves per workgroup streaming the weight, a levels epilogue); every other legal call goes to `requant_w8_linear_levels` /
`resadd_w8_linear_levels` as before.  The CPU path is theirs: `_cpu_levels_linear`, then `_cpu_requant` or `_cpu_resadd`.
"""
import ctypes

import torch

from ._abi import LINDEC_W8_MAX_ROWS, _assert_has_ops, lindec_w8_library
from ._cpu_host import _require_cpu
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._qlinear_w8_host import _LEVEL_CODE, _check_w8_args, _cpu_levels_linear
from ._qlinear_w8_host import _weight_args as _linear_weight_args
from ._requant_w8_host import _STORES, _check_out, _cpu_requant, _out_struct, requant_w8_linear_levels
from ._resadd_w8_host import _check_pre, _check_res, _cpu_resadd, _pre_ref, _res_struct, resadd_w8_linear_levels
from ._w8_host_common import _name, _status, _take_out

_ERR = "lsq_lindec_w8_last_error"
_MAX_K = 65536


def _served(M, K, *operands):
    """what liblsq_hip_lindec_w8.so serves: the preconditions of its one kernel"""
    return 1 <= M <= LINDEC_W8_MAX_ROWS and 0 < K <= _MAX_K and K % 16 == 0 and all(t.data_ptr() % 16 == 0 for t in operands)


def _lindec(what, x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_scale, out_shift, rng, relu, mid_dtype, res, pre, out):
    """`res`: None or (res_levels, res_scale, res_zero); `pre`: (pre_scale, pre_shift, pre_rng), used with a residual only"""
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'" % (what, _name(x_levels.dtype)))
    ldt = _check_out(what, out_scale, out_shift, *rng, mid_dtype)
    N, K = _check_w8_args(what, x_levels, w_levels, w_scale, w_zero, bias, mid_dtype)
    _check(s_x.dtype == torch.float32 and s_x.numel() == 1 and zx.dtype == torch.int32 and zx.numel() == 1,
           "%s: s_x must be one float32 value and zx one int32 value (tensors on x's device)" % what)
    out_shape = x_levels.shape[:-1] + (N,)
    tensors = (x_levels, s_x, zx, w_levels, w_scale, w_zero, out_scale, out_shift) + ((bias,) if bias is not None else ())
    pre_scale, pre_shift, pre_rng = pre
    if res is not None:
        _check_res(what, *res, out_shape)
        has_pre = _check_pre(what, pre_scale, pre_shift, pre_rng)
        tensors += tuple(res) + ((pre_scale, pre_shift) if has_pre else ())
    lx = x_levels.reshape(-1, K)
    M = lx.size(0)
    if not any(t.is_cuda for t in tensors):
        _require_cpu(what, *tensors)
        if M == 0 or N == 0:
            return torch.empty(out_shape, dtype=ldt)
        y = _cpu_levels_linear(lx, s_x, zx, w_levels, w_scale, w_zero, bias, mid_dtype)
        if res is None:
            return _cpu_requant(y, out_scale, out_shift, rng, relu, ldt).reshape(out_shape)
        return _cpu_resadd(y, res[0].reshape(M, N), res[1], res[2], pre_scale, pre_shift, pre_rng, out_scale, out_shift, rng, relu,
                           ldt).reshape(out_shape)
    _require_gpu(what, *tensors)
    if M == 0 or N == 0:
        return torch.empty(out_shape, dtype=ldt, device=x_levels.device)
    lx, wl = lx.contiguous(), w_levels.contiguous()
    if not _served(M, K, lx, wl):       # every other legal call: the libraries that served it before this one
        if res is None:
            return requant_w8_linear_levels(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_scale, out_shift, *rng, relu, mid_dtype,
                                            out=out)
        return resadd_w8_linear_levels(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_scale, out_shift, *rng, relu, mid_dtype,
                                       *res, pre_scale, pre_shift, *pre_rng, out=out)
    lib = lindec_w8_library()
    ws, wz = w_scale.contiguous(), w_zero.contiguous()
    bd = None if bias is None else bias.contiguous()
    y = _take_out(what, out, (M, N), ldt, lx.device)
    oq = _out_struct(out_scale, out_shift, rng, relu, mid_dtype)
    rs, res_arg, pre_struct, pre_arg = None, None, None, None
    if res is not None:
        rs = _res_struct(res[0].reshape(M, N).contiguous(), res[1], res[2])
        res_arg = ctypes.byref(rs)
        pre_struct, pre_arg = _pre_ref(pre_scale, pre_shift, pre_rng)
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_lindec_w8_linear_levels, _LEVEL_CODE[lx.dtype], lx.data_ptr(), M, s_x.data_ptr(), zx.data_ptr(),
                    *_linear_weight_args(wl, ws, wz, bd, N, K), ctypes.byref(oq), res_arg, pre_arg, y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_lindec_w8_linear_levels", lib, _ERR)
    return y.reshape(out_shape)


def lindec_w8_linear_levels(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_scale, out_shift, quant_min, quant_max, type_min,
                            type_max, relu, mid_dtype, out=None):
    """`requant_w8_linear_levels` with the decode kernel for at most 16 rows.  `out` (not an argument of the op): a dense [M, N]
    level tensor to write into, at any byte offset.  Inference only."""
    rng = (int(quant_min), int(quant_max), int(type_min), int(type_max))
    return _lindec("lsq_linear_w8_q8_dec_q", x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_scale, out_shift, rng, relu,
                   mid_dtype, None, (None, None, (0, 255, 0, 255)), out)


def lindec_w8_linear_levels_add(x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_scale, out_shift, quant_min, quant_max, type_min,
                                type_max, relu, mid_dtype, res_levels, res_scale, res_zero, pre_scale=None, pre_shift=None,
                                pre_quant_min=0, pre_quant_max=255, pre_type_min=0, pre_type_max=255, out=None):
    """`resadd_w8_linear_levels` with the decode kernel for at most 16 rows.  Inference only."""
    rng = (int(quant_min), int(quant_max), int(type_min), int(type_max))
    pre_rng = (int(pre_quant_min), int(pre_quant_max), int(pre_type_min), int(pre_type_max))
    return _lindec("lsq_linear_w8_q8_dec_add_q", x_levels, s_x, zx, w_levels, w_scale, w_zero, bias, out_scale, out_shift, rng, relu,
                   mid_dtype, (res_levels, res_scale, res_zero), (pre_scale, pre_shift, pre_rng), out)


def lindec_w8_plan(M, N, K, aligned=True, y_aligned=True, res_aligned=True):
    """The launch liblsq_hip_lindec_w8.so makes for (M, N, K), host only: `served` (False: the call goes to the requant / resadd
    libraries, every other field is 0), grid, block, lds_bytes, chunks (of at most 4096 k), x_resident (one chunk holds all of K:
    x stays in LDS across a workgroup's tiles), store and res_load ("packets": N % 16 == 0 and a 16-byte aligned y / residual, or
    "bytes")."""
    lib = lindec_w8_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_lindec_w8_plan(int(M), int(N), int(K), 1 if aligned else 0, 1 if y_aligned else 0, 1 if res_aligned else 0,
                                ctypes.byref(out))
    _status(rc, "lsq_lindec_w8_plan", lib, _ERR)
    return dict(served=bool(out[0]), grid=out[1], block=out[2], lds_bytes=out[3], chunks=out[4], x_resident=bool(out[5]),
                store=_STORES[out[6]], res_load=_STORES[out[7]])
