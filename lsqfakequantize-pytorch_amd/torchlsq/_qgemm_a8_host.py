"""Host layer of the int8 matrix-core GEMM on packed group-wise weights (include/lsq_hip_qgemm_a8.h, liblsq_hip_qgemm_a8.so):
the 8-bit-activation linear ops of _qlinear_a8_host.py for more rows of x than the decode kernel serves.  One call for all
rows, the codes streamed once per 128-row tile instead of once per 16 rows -- and every row has the bits of the decode
kernel's 1-row call, so which route a call takes is a matter of speed alone.  It serves the formats of the decode kernel's
matrix-core form; `qgemm_a8_serves` says whether a format is one, from the library's plan.

`_qlinear_a8_host` validates the tensors and calls `qgemm_a8_forward_levels` / `qgemm_a8_forward` on them; nothing here is
a second op.
"""
import ctypes
import functools

import torch

from ._abi import _DTYPE_CODE, LSQ_A8_I8, LSQ_A8_U8, qgemm_a8_library
from ._hip_host import _on_device, _stream_of

# Rows from which the GPU calls of the served formats take the GEMM rather than the decode kernel 16 rows at a time: the
# smallest measured M from which the GEMM is no slower, within the measurement's spread, in every served format and for both
# entry forms (profiles/r14_qgemm_a8_ab.txt, DESIGN.md 9.6: 0.14-0.53 x the block route at 512 and 2048 rows, 0.99-3.9 x at
# 17 to 128; nothing was measured between 128 and 512).  The bits are the same on both routes: this is a speed decision.
QGEMM_A8_MIN_ROWS = 512

_LEVEL_CODE = {torch.uint8: LSQ_A8_U8, torch.int8: LSQ_A8_I8}


def _status(rc, what, lib):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, lib.lsq_qgemm_a8_last_error().decode("utf-8", "replace")))


def qgemm_a8_min_rows():
    """Rows of x from which `lsq_linear_packed_q8` / `lsq_linear_packed_a8` take the GEMM on the formats it serves."""
    return QGEMM_A8_MIN_ROWS


def qgemm_a8_plan(M, N, K, group_size, bits):
    """The launch liblsq_hip_qgemm_a8.so makes for (M, N, K, G, bits) -- host only, nothing is launched (lsq_qgemm_a8_plan).
    form "mfma": served on the matrix cores; form "unserved": the forwards refuse the format, the other fields are 0."""
    lib = qgemm_a8_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_qgemm_a8_plan(int(M), int(N), int(K), int(group_size), int(bits), ctypes.byref(out))
    _status(rc, "lsq_qgemm_a8_plan", lib)
    return dict(form="mfma" if out[0] else "unserved", grid=out[1], block=out[2], rows_per_tile=out[3], cols_per_tile=out[4],
                lds_bytes=out[5], k_per_step=out[6], subs=out[7])


@functools.lru_cache(maxsize=None)
def _format_served(group_size, bits):
    # whether a format is served depends on (G, bits) alone: asked once per format, of the library
    return qgemm_a8_plan(17, 16, group_size, group_size, bits)["form"] == "mfma"


def qgemm_a8_serves(codes, group_size, bits):
    """True when the library takes this call: the plan says form 1 for the format, and `codes` is 16-byte aligned."""
    return codes.data_ptr() % 16 == 0 and _format_served(group_size, bits)


def _weight_args(codes, qscale, qzero, bias, N, K, group_size, bits):
    return (codes.data_ptr(), N, K, group_size, bits, qscale.data_ptr(), qzero.data_ptr(), None if bias is None else bias.data_ptr(),
            0 if bias is None else _DTYPE_CODE[bias.dtype])


def qgemm_a8_forward_levels(lx, s_x, zx, codes, qscale, qzero, bias, group_size, bits, y_dtype):
    """levels lx [M, K] (uint8 / int8) -> y [M, N] of y_dtype with one launch of lsq_qgemm_a8_forward_levels.  The tensors
    are contiguous GPU tensors that `qlinear_a8_forward_levels` has checked; a format that is not served raises."""
    lib = qgemm_a8_library()
    M, K = lx.shape
    N = codes.size(0)
    y = torch.empty((M, N), dtype=y_dtype, device=lx.device)
    idx = lx.device.index
    rc = _on_device(idx, lib.lsq_qgemm_a8_forward_levels, _LEVEL_CODE[lx.dtype], lx.data_ptr(), M, s_x.data_ptr(), zx.data_ptr(),
                    *_weight_args(codes, qscale, qzero, bias, N, K, group_size, bits), y.data_ptr(), _DTYPE_CODE[y_dtype],
                    _stream_of(idx))
    _status(rc, "lsq_qgemm_a8_forward_levels", lib)
    return y


def qgemm_a8_forward(x, scale, shift, qmin, qmax, tmin, tmax, codes, qscale, qzero, bias, group_size, bits):
    """floating x [M, K] -> y [M, N] of x's dtype with one call of lsq_qgemm_a8_forward: a pre-pass writes the byte operand
    into a workspace of M * K bytes allocated here, the GEMM reads it.  Contiguous GPU tensors, checked by the caller."""
    lib = qgemm_a8_library()
    M, K = x.shape
    N = codes.size(0)
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    ws = torch.empty((M, K), dtype=torch.int8, device=x.device)
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_qgemm_a8_forward, _DTYPE_CODE[x.dtype], x.data_ptr(), M, scale.data_ptr(), shift.data_ptr(),
                    qmin, qmax, tmin, tmax, *_weight_args(codes, qscale, qzero, bias, N, K, group_size, bits), y.data_ptr(),
                    ws.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_qgemm_a8_forward", lib)
    return y
