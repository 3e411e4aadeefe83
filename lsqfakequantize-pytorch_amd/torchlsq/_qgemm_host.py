"""Host layer of the matrix-core GEMM on packed group-wise weights (include/lsq_hip_qgemm.h, liblsq_hip_qgemm.so): the linear
op of _qlinear_host.py for more rows of x than the decode kernel serves.  It reads the 4- / 2-bit codes in place -- no
dequantized copy of the weight exists -- and serves bfloat16 / float16 x on formats whose group is a whole number of
16-byte code packets; `qgemm_serves` says whether a format is one, from the library's plan.

`_qlinear_host.qlinear_forward` validates the tensors and calls `qgemm_forward` on them; nothing here is a second op.
"""
import ctypes
import functools

import torch

from ._abi import _DTYPE_CODE, qgemm_library
from ._hip_host import _on_device, _stream_of


def _status(rc, what, lib):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, lib.lsq_qgemm_last_error().decode("utf-8", "replace")))


def qgemm_plan(dtype, M, N, K, group_size, bits):
    """The launch liblsq_hip_qgemm.so makes for (dtype, M, N, K, G, bits) -- host only, nothing is launched (lsq_qgemm_plan).
    form "mfma": served on the matrix cores; form "unserved": lsq_qgemm_forward refuses the format, the other fields are 0."""
    lib = qgemm_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_qgemm_plan(_DTYPE_CODE[dtype], int(M), int(N), int(K), int(group_size), int(bits), ctypes.byref(out))
    _status(rc, "lsq_qgemm_plan", lib)
    return dict(form="mfma" if out[0] else "unserved", grid=out[1], block=out[2], rows_per_tile=out[3], cols_per_tile=out[4],
                lds_bytes=out[5], k_per_step=out[6])


@functools.lru_cache(maxsize=None)
def _format_served(dtype, group_size, bits):
    # whether a format is served depends on (dtype, G, bits) alone: asked once per format, of the library
    return qgemm_plan(dtype, 17, 16, group_size, group_size, bits)["form"] == "mfma"


def qgemm_serves(x, codes, group_size, bits):
    """True when lsq_qgemm_forward takes this call: the plan says form 1 for x's dtype and the format, and `codes` is 16-byte
    aligned."""
    return x.dtype in (torch.bfloat16, torch.float16) and codes.data_ptr() % 16 == 0 and _format_served(x.dtype, group_size, bits)


def qgemm_forward(x, codes, qscale, qzero, bias, group_size, bits):
    """x [M, K] -> y [M, N] of x's dtype with one launch of lsq_qgemm_forward.  The tensors are contiguous GPU tensors that
    `qlinear_forward` has checked; a format that is not served raises (the library's message says why)."""
    lib = qgemm_library()
    M, K = x.shape
    N = codes.size(0)
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    idx = x.device.index
    rc = _on_device(idx, lib.lsq_qgemm_forward, _DTYPE_CODE[x.dtype], x.data_ptr(), M, codes.data_ptr(), N, K, group_size, bits,
                    qscale.data_ptr(), qzero.data_ptr(), None if bias is None else bias.data_ptr(),
                    0 if bias is None else _DTYPE_CODE[bias.dtype], y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_qgemm_forward", lib)
    return y
