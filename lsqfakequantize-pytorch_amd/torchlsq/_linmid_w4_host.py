"""Host layer of liblsq_hip_linmid_w4.so (include/lsq_hip_linmid_w4.h): the levels-out linears on packed 4- / 2-bit codes for 17 to
64 rows of activation levels in ONE launch that streams the weight once.  It defines no op: `_lindec_w4_host._lindec` routes the
ops `lsq_linear_packed_q8_q` / `lsq_linear_packed_q8_add_q` here by the number of rows, and the bytes are those of the composition
stated there.  This module makes the ctypes call through its own `_on_device` binding and answers for the plan."""
import ctypes

from ._abi import _DTYPE_CODE, LINMID_W4_MAX_ROWS, LINMID_W4_MIN_ROWS, linmid_w4_library
from ._hip_host import _on_device, _stream_of
from ._qlinear_a8_host import _LEVEL_CODE
from ._requant_w8_host import _STORES
from ._w8_host_common import _status

_ERR = "lsq_linmid_w4_last_error"


def _served(M, N, K, group_size, bits, *operands):
    """what liblsq_hip_linmid_w4.so serves: its own plan's answer (host only, no launch)"""
    return LINMID_W4_MIN_ROWS <= M <= LINMID_W4_MAX_ROWS and \
        linmid_w4_plan(M, N, K, group_size, bits, all(t.data_ptr() % 16 == 0 for t in operands))["served"]


def _launch(lx, s_x, zx, cd, qs, qz, bd, group_size, bits, oq, res_arg, pre_arg, y):
    """one launch on dense operands: lx [M, K] levels, cd [N, K * bits / 8] codes, y [M, N] levels; oq / res_arg / pre_arg: the structs
    of lsq_hip_requant_w8.h / lsq_hip_resadd_w8.h by reference (or None)"""
    lib = linmid_w4_library()
    (M, K), N, idx = lx.shape, cd.size(0), lx.device.index
    rc = _on_device(idx, lib.lsq_linmid_w4_linear_levels, _LEVEL_CODE[lx.dtype], lx.data_ptr(), M, s_x.data_ptr(), zx.data_ptr(),
                    cd.data_ptr(), N, K, group_size, bits, qs.data_ptr(), qz.data_ptr(), None if bd is None else bd.data_ptr(),
                    0 if bd is None else _DTYPE_CODE[bd.dtype], oq, res_arg, pre_arg, y.data_ptr(), _stream_of(idx))
    _status(rc, "lsq_linmid_w4_linear_levels", lib, _ERR)


def linmid_w4_plan(M, N, K, group_size, bits, aligned=True, y_aligned=True, res_aligned=True):
    """The launch liblsq_hip_linmid_w4.so makes for (M, N, K, G, bits), host only: `served` (False: every other field is 0), grid,
    block, lds_bytes (at most 160 KB), subs (sub-tiles of 16 rows a wave keeps), stages (windows of x a full chunk of 4096 k is
    staged in), store and res_load ("packets": N % 16 == 0 and a 16-byte aligned y / residual, or "bytes")."""
    lib = linmid_w4_library()
    out = (ctypes.c_int32 * 8)()
    rc = lib.lsq_linmid_w4_plan(int(M), int(N), int(K), int(group_size), int(bits), 1 if aligned else 0, 1 if y_aligned else 0,
                                1 if res_aligned else 0, ctypes.byref(out))
    _status(rc, "lsq_linmid_w4_plan", lib, _ERR)
    return dict(served=bool(out[0]), grid=out[1], block=out[2], lds_bytes=out[3], subs=out[4], stages=out[5], store=_STORES[out[6]],
                res_load=_STORES[out[7]])
