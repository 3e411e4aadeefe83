"""Host layer of the linear op on packed group-wise weights: y = x @ w^T (+ bias) with w = (code - zero_point) * scale read
straight from the 4- / 2-bit codes (include/lsq_hip_qlinear.h states the arithmetic; include/lsq_hip_pack.h the format).

GPU tensors: up to QLINEAR_MAX_ROWS rows of x (the product of its leading dims) go to liblsq_hip_qlinear.so with one ctypes
call -- the weight is streamed once and no dequantized copy exists.  More rows (prefill, batches of sequences) of
bfloat16 / float16 x go to the matrix-core GEMM of liblsq_hip_qgemm.so (_qgemm_host.py), which reads the codes in place
too and is invariant to the batch among its own calls -- its bits are not the decode kernel's, whose sum has another order.
What that library does not serve -- float32 x, a group that is no whole number of 16-byte code packets, codes that are not
16-byte aligned -- takes the DEQUANTIZE route: the weight is dequantized into a float32 temporary (liblsq_hip_pack.so) and
handed to torch.nn.functional.linear in float32; that route meets the accuracy contract, not the batch invariance of the
native kernels.  CPU tensors: x @ dequantize().T in float32 (float64
for a float64 scale) with torch -- as in _pack_host.py, not a hot path.
"""
import ctypes

import torch

from ._abi import _DTYPE_CODE, QLINEAR_MAX_ROWS, _assert_has_ops, qlinear_library
from ._cpu_host import _require_cpu
from ._hip_host import _check, _on_device, _require_gpu, _stream_of
from ._pack_host import _check_packed, pack_dequantize
from ._qgemm_host import qgemm_forward, qgemm_serves
from ._w8_host_common import _status

_X_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def check_packed_linear_args(what, x, codes, qscale, qzero, bias, group_size, bits, y_dtype=None):
    """(N, K) of the packed weight, after the checks every linear op on it shares, on both devices.  y_dtype: the output's
    dtype; None when it is x's, which must then be a floating-point one.  The bias is float32 or of that dtype."""
    _check_packed(what, codes, qscale, qzero, group_size, bits)
    _check(codes.dim() == 2, "%s: codes must be the [N, K * bits / 8] bytes of a 2-D weight, got %d dims" % (what, codes.dim()))
    N, K = codes.size(0), codes.size(1) * (8 // bits)
    _check(x.dim() >= 1 and x.size(-1) == K,
           "%s: the last dimension of x is %s, the packed weight has K = %d" % (what, x.size(-1) if x.dim() else "missing", K))
    if y_dtype is None:
        _check(x.is_floating_point(), "%s: x must be a floating-point tensor" % what)
    if bias is not None:
        _check(bias.dim() == 1 and bias.numel() == N, "%s: the bias needs %d values, got shape %s" % (what, N, tuple(bias.shape)))
        _check(bias.dtype in (torch.float32, x.dtype if y_dtype is None else y_dtype),
               "%s: the bias must be float32 or of %s dtype" % (what, "x's" if y_dtype is None else "the output's"))
    return N, K


def _plan_dict(out8):
    """out8[] of lsq_qlinear_plan / lsq_qlinear_a8_plan"""
    return dict(form="mfma" if out8[0] else "generic", grid=out8[1], block=out8[2], native_rows=out8[3], lds_bytes=out8[4],
                chunk=out8[5], waves_per_tile=out8[6], cols_per_tile=out8[7])


def qlinear_forward(x, codes, qscale, qzero, bias, group_size, bits):
    """x [..., K] -> y [..., N] of x's dtype.  Inference only: the caller (the op's autograd key) has refused an x that
    wants a gradient."""
    what = "lsq_linear_packed"
    _assert_has_ops()
    N, K = check_packed_linear_args(what, x, codes, qscale, qzero, bias, group_size, bits)
    out_shape = x.shape[:-1] + (N,)
    tensors = (x, codes, qscale, qzero) + ((bias,) if bias is not None else ())
    if not any(t.is_cuda for t in tensors):
        _require_cpu(what, *tensors)
        wide = torch.float64 if qscale.dtype == torch.float64 else torch.float32
        _check(x.dtype in _X_DTYPES or x.dtype == torch.float64, "%s: not implemented for '%s'" % (what, str(x.dtype).replace("torch.", "")))
        w = pack_dequantize(codes, qscale, qzero, group_size, bits, wide)
        y = x.reshape(-1, K).to(wide) @ w.t()
        if bias is not None:
            y = y + bias.to(wide)
        return y.to(x.dtype).reshape(out_shape)
    _require_gpu(what, *tensors)
    _check(qscale.dtype == torch.float32,
           "%s: a packed weight with a float64 scale has no GPU linear (the kernel computes in float32); dequantize() it, or "
           "export the weight from float32, bfloat16 or float16" % what)
    _check(x.dtype in _X_DTYPES, "%s: x must be float32, bfloat16 or float16 on the GPU, got '%s'" % (what, str(x.dtype).replace("torch.", "")))
    xd = x.reshape(-1, K)
    if not xd.is_contiguous():
        xd = xd.contiguous()
    M = xd.size(0)
    cd, qs, qz = codes.contiguous(), qscale.contiguous(), qzero.contiguous()
    if M == 0 or N == 0:
        return torch.empty(out_shape, dtype=x.dtype, device=x.device)
    if M > QLINEAR_MAX_ROWS:
        if qgemm_serves(xd, cd, group_size, bits):
            return qgemm_forward(xd, cd, qs, qz, None if bias is None else bias.contiguous(), group_size, bits).reshape(out_shape)
        # the dequantize route, for what the GEMM does not serve.  The temporary is float32 whatever x is: a weight rounded to bfloat16 / float16 carries a
        # relative error of 2^-9 / 2^-12 per term, far outside the fp32-accumulation bound of the op, so the product runs in
        # float32 and is rounded once
        w = pack_dequantize(cd, qs, qz, group_size, bits, torch.float32)
        y = torch.nn.functional.linear(xd.float(), w, None if bias is None else bias.float())
        return y.to(x.dtype).reshape(out_shape)
    lib = qlinear_library()
    bd = None if bias is None else bias.contiguous()
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_qlinear_forward, _DTYPE_CODE[x.dtype], xd.data_ptr(), M, cd.data_ptr(), N, K, group_size, bits,
                    qs.data_ptr(), qz.data_ptr(), None if bd is None else bd.data_ptr(),
                    0 if bd is None else _DTYPE_CODE[bd.dtype], y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_qlinear_forward", lib, "lsq_qlinear_last_error")
    return y.reshape(out_shape)


def qlinear_plan(dtype, M, N, K, group_size, bits):
    """The launch liblsq_hip_qlinear.so makes for (dtype, M, N, K, G, bits) -- host only, nothing is launched (lsq_qlinear_plan)."""
    lib = qlinear_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_qlinear_plan(_DTYPE_CODE[dtype], int(M), int(N), int(K), int(group_size), int(bits), ctypes.byref(out))
    _status(rc, "lsq_qlinear_plan", lib, "lsq_qlinear_last_error")
    return _plan_dict(out)
