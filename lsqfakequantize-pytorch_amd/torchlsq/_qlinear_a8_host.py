"""Host layer of the 8-bit-activation linear op on packed group-wise weights (include/lsq_hip_qlinear_a8.h states the
arithmetic; include/lsq_hip_pack.h the weight format):

    I[m, n, g] = sum_{k in g} (lx[m, k] - zx) * (code[n, k] - zero_point[n, g])      an exact integer
    y[m, n]    = s_x * sum_g scale[n, g] * float(I[m, n, g])  (+ bias[n])

Two ops over it.  `lsq_linear_packed_q8` takes the levels lx as bytes (uint8: 0..255, int8: -128..127) with s_x (float32) and
zx (int32) as one-element tensors on x's device.  `lsq_linear_packed_a8` takes a floating x and a per-tensor quantizer's
scale, shift and range and forms the levels itself -- in the kernel on the GPU, with `cpu_levels` on the CPU -- so its result
is the levels op on `lsq_levels_per_tensor`'s bytes, bit for bit.

GPU tensors: up to QLINEAR_A8_MAX_ROWS rows (the product of the leading dims) go to liblsq_hip_qlinear_a8.so with one ctypes
call; nothing is read back.  From `qgemm_a8_min_rows()` rows on, a call on a format that liblsq_hip_qgemm_a8.so serves (the decode
kernel's matrix-core form: `qgemm_a8_serves`) is ONE call of its int8 matrix-core GEMM (_qgemm_a8_host.py), which streams the
codes once per 128-row tile and keeps the decode kernel's order of the fp32 sum; the fused op allocates the M * K bytes of
levels the GEMM's pre-pass writes.  Every other call with more rows goes to the decode kernel QLINEAR_A8_MAX_ROWS at a time,
one launch per block of rows (`_launch_row_blocks`), the weight streamed once per block.  On both routes every row is the
1-row call bit for bit, whatever M is: the threshold is a matter of speed alone.  (Dequantizing the
levels to float32, (lx - zx) * s_x, for `lsq_linear_packed`'s prefill route -- a float32 weight temporary and F.linear in
float32 -- does K fp32 multiply-adds per output: its error scales with sum |a| |code - qzero|, before the cancellation inside
a group, and the bound of this op, which scales with sum |I|, does not cover that.  DESIGN.md 9.4 has the figures.)  CPU
tensors: torch int64 matrix products per group, then the same fp32 steps -- exact in I as well; not a hot path.
"""
import ctypes

import torch

from ._abi import _DTYPE_CODE, LSQ_A8_I8, LSQ_A8_U8, QLINEAR_A8_MAX_ROWS, _assert_has_ops, qlinear_a8_library
from ._cpu_host import _require_cpu, cpu_levels
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._pack_host import _unpack_bytes
from ._qgemm_a8_host import qgemm_a8_forward, qgemm_a8_forward_levels, qgemm_a8_min_rows, qgemm_a8_serves
from ._qlinear_host import _plan_dict, check_packed_linear_args
from ._w8_host_common import _act_constants, _check_range, _status

_Y_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_LEVEL_CODE = {torch.uint8: LSQ_A8_U8, torch.int8: LSQ_A8_I8}


def _check_a8_args(what, x, codes, qscale, qzero, bias, group_size, bits, y_dtype):
    """(N, K) of the packed weight, after the checks both ops and both devices share"""
    N, K = check_packed_linear_args(what, x, codes, qscale, qzero, bias, group_size, bits, y_dtype)
    _check(y_dtype in _Y_DTYPES, "%s: the output must be float32, bfloat16 or float16, got '%s'" % (what, str(y_dtype).replace("torch.", "")))
    _check(qscale.dtype == torch.float32,
           "%s: a packed weight with a float64 scale has no 8-bit-activation linear (the op computes in integers and float32)" % what)
    return N, K


def _cpu_levels_linear(lx, s_x, zx, codes, qscale, qzero, bias, group_size, bits, y_dtype, N, K):
    M = lx.size(0)
    groups = K // group_size
    a = lx.to(torch.int64) - zx.to(torch.int64).reshape(())
    cz = _unpack_bytes(codes, bits).to(torch.int64).reshape(N, groups, group_size) - qzero.reshape(N, groups, 1).to(torch.int64)
    # [groups, M, G] @ [groups, G, N]: exact in int64
    I = torch.bmm(a.reshape(M, groups, group_size).permute(1, 0, 2).contiguous(), cz.permute(1, 2, 0).contiguous())
    t = qscale.reshape(N, groups).t().reshape(groups, 1, N) * I.to(torch.float32)      # one rounding each
    y = torch.zeros(M, N, dtype=torch.float32)
    for g in range(groups):                                                             # the sum over the groups in fp32
        y = y + t[g]
    y = y * s_x.reshape(())
    if bias is not None:
        y = y + bias.to(torch.float32)
    return y.to(y_dtype)


def _row_blocks(M):
    """(first row, rows) of the launches that serve M rows: the native kernel takes QLINEAR_A8_MAX_ROWS at a time"""
    return [(m0, min(QLINEAR_A8_MAX_ROWS, M - m0)) for m0 in range(0, M, QLINEAR_A8_MAX_ROWS)]


def _gemm_operands(M, codes, qscale, qzero, bias, group_size, bits):
    """(codes, qscale, qzero, bias), contiguous, when an M-row GPU call takes the GEMM of liblsq_hip_qgemm_a8.so; else None"""
    if M < qgemm_a8_min_rows():
        return None
    cd = codes.contiguous()
    if not qgemm_a8_serves(cd, group_size, bits):
        return None
    return cd, qscale.contiguous(), qzero.contiguous(), None if bias is None else bias.contiguous()


def _launch_row_blocks(entry, x_code, xd, act_args, codes, qscale, qzero, bias, group_size, bits, y_dtype, y_args=()):
    """The GPU side of both ops: y [M, N] of y_dtype for the rows xd [M, K], QLINEAR_A8_MAX_ROWS rows per launch of the C
    entry point `entry`.  The two entry points differ in `x_code` (the dtype code of x), in `act_args` (what follows the rows
    of x: the activation's constants) and in `y_args` (what follows y)."""
    lib = qlinear_a8_library()
    fn = getattr(lib, entry)
    if not xd.is_contiguous():
        xd = xd.contiguous()
    cd, qs, qz = codes.contiguous(), qscale.contiguous(), qzero.contiguous()
    bd = None if bias is None else bias.contiguous()
    M, K, N = xd.size(0), xd.size(1), cd.size(0)
    y = torch.empty((M, N), dtype=y_dtype, device=xd.device)
    idx = xd.device.index
    x_row, y_row = K * xd.element_size(), N * y.element_size()
    for m0, rows in _row_blocks(M):
        rc = _on_device(idx, fn, x_code, xd.data_ptr() + m0 * x_row, rows, *act_args, cd.data_ptr(), N, K, group_size, bits,
                        qs.data_ptr(), qz.data_ptr(), None if bd is None else bd.data_ptr(), 0 if bd is None else _DTYPE_CODE[bd.dtype],
                        y.data_ptr() + m0 * y_row, *y_args, _stream_of(idx))
        _status(rc, entry, lib, "lsq_qlinear_a8_last_error")
    return y


def qlinear_a8_forward_levels(x_levels, s_x, zx, codes, qscale, qzero, bias, group_size, bits, out_dtype):
    """x_levels [..., K] bytes -> y [..., N] of out_dtype.  Inference only."""
    what = "lsq_linear_packed_q8"
    _assert_has_ops()
    _check(x_levels.dtype in _LEVEL_CODE, "%s: the levels must be uint8 (0..255) or int8 (-128..127), got '%s'"
           % (what, str(x_levels.dtype).replace("torch.", "")))
    N, K = _check_a8_args(what, x_levels, codes, qscale, qzero, bias, group_size, bits, out_dtype)
    _check(s_x.dtype == torch.float32 and s_x.numel() == 1 and zx.dtype == torch.int32 and zx.numel() == 1,
           "%s: s_x must be one float32 value and zx one int32 value (tensors on x's device)" % what)
    out_shape = x_levels.shape[:-1] + (N,)
    tensors = (x_levels, s_x, zx, codes, qscale, qzero) + ((bias,) if bias is not None else ())
    lx = x_levels.reshape(-1, K)
    M = lx.size(0)
    if not any(t.is_cuda for t in tensors):
        _require_cpu(what, *tensors)
        if M == 0 or N == 0:
            return torch.empty(out_shape, dtype=out_dtype)
        return _cpu_levels_linear(lx, s_x, zx, codes, qscale, qzero, bias, group_size, bits, out_dtype, N, K).reshape(out_shape)
    _require_gpu(what, *tensors)
    if M == 0 or N == 0:
        return torch.empty(out_shape, dtype=out_dtype, device=x_levels.device)
    ops = _gemm_operands(M, codes, qscale, qzero, bias, group_size, bits)
    if ops is not None:
        y = qgemm_a8_forward_levels(lx.contiguous(), s_x, zx, *ops, group_size, bits, out_dtype)
    else:
        y = _launch_row_blocks("lsq_qlinear_a8_forward_levels", _LEVEL_CODE[x_levels.dtype], lx, (s_x.data_ptr(), zx.data_ptr()), codes,
                               qscale, qzero, bias, group_size, bits, out_dtype, (_DTYPE_CODE[out_dtype],))
    return y.reshape(out_shape)


def qlinear_a8_forward(x, act_scale, act_shift, qmin, qmax, tmin, tmax, codes, qscale, qzero, bias, group_size, bits):
    """floating x [..., K] -> y [..., N] of x's dtype: the levels of the per-tensor quantizer (act_scale, act_shift, range)
    are formed on the way.  Inference only."""
    what = "lsq_linear_packed_a8"
    _assert_has_ops()
    _check(x.is_floating_point(), "%s: x must be a floating-point tensor" % what)
    _check(x.dtype in _Y_DTYPES, "%s: x must be float32, bfloat16 or float16, got '%s'" % (what, str(x.dtype).replace("torch.", "")))
    N, K = _check_a8_args(what, x, codes, qscale, qzero, bias, group_size, bits, x.dtype)
    unsigned = _check_range(what, qmin, qmax, tmin, tmax)
    _check(act_scale.dtype == torch.float32 and act_shift.dtype == torch.float32 and act_scale.numel() >= 1 and act_shift.numel() >= 1,
           "%s: the activation quantizer's scale and shift must be float32 tensors of one value (a per-tensor quantizer)" % what)
    out_shape = x.shape[:-1] + (N,)
    tensors = (x, act_scale, act_shift, codes, qscale, qzero) + ((bias,) if bias is not None else ())
    xd = x.reshape(-1, K)
    M = xd.size(0)
    on_gpu = any(t.is_cuda for t in tensors)
    if on_gpu:
        _require_gpu(what, *tensors)
    else:
        _require_cpu(what, *tensors)
    if M == 0 or N == 0:
        return torch.empty(out_shape, dtype=x.dtype, device=x.device)
    if not on_gpu:
        sc, sh = act_scale.detach().reshape(-1)[:1], act_shift.detach().reshape(-1)[:1]
        lv = cpu_levels(xd, sc, sh, 0, False, qmin, qmax, tmin, tmax, 0)
        lv = lv.view(torch.uint8) if unsigned else lv
        s_x, zx = _act_constants(sc, sh, tmin, tmax)
        return _cpu_levels_linear(lv, s_x, zx, codes, qscale, qzero, bias, group_size, bits, x.dtype, N, K).reshape(out_shape)
    sc, sh = act_scale.detach().contiguous(), act_shift.detach().contiguous()
    ops = _gemm_operands(M, codes, qscale, qzero, bias, group_size, bits)
    if ops is not None:
        y = qgemm_a8_forward(xd.contiguous(), sc, sh, qmin, qmax, tmin, tmax, *ops, group_size, bits)
    else:
        y = _launch_row_blocks("lsq_qlinear_a8_forward", _DTYPE_CODE[x.dtype], xd, (sc.data_ptr(), sh.data_ptr(), qmin, qmax, tmin, tmax),
                               codes, qscale, qzero, bias, group_size, bits, x.dtype)
    return y.reshape(out_shape)


def qlinear_a8_plan(M, N, K, group_size, bits):
    """The launch liblsq_hip_qlinear_a8.so makes for (M, N, K, G, bits) -- host only, nothing is launched."""
    lib = qlinear_a8_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_qlinear_a8_plan(int(M), int(N), int(K), int(group_size), int(bits), ctypes.byref(out))
    _status(rc, "lsq_qlinear_a8_plan", lib, "lsq_qlinear_a8_last_error")
    return _plan_dict(out)
