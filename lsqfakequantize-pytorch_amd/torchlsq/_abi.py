"""The native libraries of the package and how they are opened: liblsq_hip.so (include/lsq_hip.h, ctypes), liblsq_cpu.so
(include/lsq_cpu.h, ctypes), liblsq_hip_group.so (include/lsq_hip_group.h, ctypes), liblsq_hip_pack.so (include/lsq_hip_pack.h,
ctypes), the linear layers on packed weights liblsq_hip_qlinear.so, liblsq_hip_qlinear_a8.so, liblsq_hip_qgemm.so and liblsq_hip_qgemm_a8.so (ctypes),
the W8A8 layers on 8-bit levels liblsq_hip_qlinear_w8.so and liblsq_hip_qconv_w8.so, their form with an 8-bit output
liblsq_hip_requant_w8.so and that form with a levels residual liblsq_hip_resadd_w8.so, pooling on levels liblsq_hip_pool_w8.so, the depthwise conv2d liblsq_hip_dwconv_w8.so, the byte table op and the gate multiply liblsq_hip_eltwise_w8.so (ctypes)
and _lsq_torch.so (the C++ torch binding of the same C ABI, torch.ops.load_library).

This is the replacement of reference torchlsq/extension.py:12-56, which located `_C.so` and `torch.ops.load_library`-ed it.
The module holds the loader STATE (`_LIB`, `_HAS_OPS`, `_CPU_LIB`, `_NATIVE_LSQ`); the host layers (_hip_host.py,
_cpu_host.py) read it through the module at call time, so tools/lsq_tools.py can swap the tools build of the library in with
`set_library`.
"""
import ctypes
import os
import threading

import torch

_HAS_OPS = False
error_str = ""
_LIB = None
_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "liblsq_hip.so")

# dtype codes of include/lsq_hip.h
LSQ_F32, LSQ_F64, LSQ_BF16, LSQ_F16 = 0, 1, 2, 3
_DTYPE_CODE = {torch.float32: LSQ_F32, torch.float64: LSQ_F64, torch.bfloat16: LSQ_BF16, torch.float16: LSQ_F16}


class LsqParams(ctypes.Structure):
    """struct lsq_params (include/lsq_hip.h)."""
    _fields_ = [("quant_min", ctypes.c_int32), ("quant_max", ctypes.c_int32),
                ("type_min", ctypes.c_int32), ("type_max", ctypes.c_int32),
                ("use_grad_scaling", ctypes.c_int32), ("sym", ctypes.c_int32),
                ("eval_mode", ctypes.c_int32), ("init_mode", ctypes.c_int32),
                ("grad_scaler", ctypes.c_double), ("numel_for_scaler", ctypes.c_int64)]


class LsqFwdExtras(ctypes.Structure):
    """struct lsq_fwd_extras (include/lsq_hip.h)."""
    _fields_ = [("levels", ctypes.c_void_p), ("level_bias", ctypes.c_int32), ("aux_kind", ctypes.c_int32)]


class LsqBwdExtras(ctypes.Structure):
    """struct lsq_bwd_extras (include/lsq_hip.h)."""
    _fields_ = [("ticket", ctypes.c_void_p)]


class LsqObserverUpdate(ctypes.Structure):
    """struct lsq_observer_update (include/lsq_hip.h)."""
    _fields_ = [("mode", ctypes.c_int32), ("first", ctypes.c_int32), ("averaging_constant", ctypes.c_float),
                ("quant_min", ctypes.c_int32), ("quant_max", ctypes.c_int32), ("symmetric", ctypes.c_int32),
                ("zero_point_symmetric", ctypes.c_int32), ("eps", ctypes.c_float)]


class LsqPcItem(ctypes.Structure):
    """struct lsq_pc_item (include/lsq_hip.h): one tensor of a multi-tensor launch."""
    _fields_ = [("x", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("y", ctypes.c_void_p), ("dx", ctypes.c_void_p),
                ("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p), ("ds", ctypes.c_void_p), ("db", ctypes.c_void_p),
                ("outer", ctypes.c_int64), ("channels", ctypes.c_int64), ("inner", ctypes.c_int64)]


class LsqCommOptions(ctypes.Structure):
    """struct lsq_comm_options (include/lsq_hip.h)."""
    _fields_ = [("size", ctypes.c_int32), ("event_system_fence", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


LSQ_TICKET_BYTES = 4096
ABI_VERSION = 6

_vp, _i64, _int, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
_PP = ctypes.POINTER(LsqParams)
_EP = ctypes.POINTER(LsqFwdExtras)
_BP = ctypes.POINTER(LsqBwdExtras)

# every symbol include/lsq_hip.h declares: (restype, argtypes)
C_ABI = {
    "lsq_hip_abi_version": (_int, []),
    "lsq_hip_runtime_version": (_i64, []),
    "lsq_hip_last_error": (ctypes.c_char_p, []),
    "lsq_hip_grad_scaler": (ctypes.c_double, [_int, _int, _i64, ctypes.c_int32, _i64, ctypes.c_int32, ctypes.c_double]),
    "lsq_hip_policy_ticket": (_int, [ctypes.c_int32, ctypes.c_int32, _i64]),
    "lsq_hip_policy_saves_mask": (_int, [ctypes.c_int32] * 4),
    "lsq_hip_backward_per_tensor_workspace": (_sz, [_int, _i64]),
    "lsq_hip_forward_per_tensor": (_int, [_int, _vp, _vp, _i64, _vp, _vp, _PP, _EP, _vp]),
    "lsq_hip_backward_per_tensor": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _PP, _BP, _vp, _sz, _vp]),
    "lsq_hip_backward_per_channel_workspace": (_sz, [_int, _i64, _i64, _i64]),
    "lsq_hip_forward_per_channel": (_int, [_int, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _PP, _EP, _vp]),
    "lsq_hip_backward_per_channel": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _PP, _BP,
                                            _vp, _sz, _vp]),
    "lsq_hip_sharded_finish": (_int, [_int, _vp, _i64, ctypes.c_int32, _PP, _vp, _vp, _vp]),
    "lsq_hip_per_channel_multi_ok": (_int, [_int, _i64, _i64, _i64, _int]),
    "lsq_hip_plan_backward_per_channel": (_int, [_int, _i64, _i64, _i64, _int, _PP, ctypes.POINTER(ctypes.c_int32 * 8)]),
    "lsq_hip_comm_unique_id": (_int, [_vp]),
    "lsq_hip_comm_create": (_int, [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(LsqCommOptions), ctypes.POINTER(_vp)]),
    "lsq_hip_comm_configure": (_int, [_vp, ctypes.POINTER(LsqCommOptions)]),
    "lsq_hip_comm_tune": (_int, [_vp, _vp]),
    "lsq_hip_comm_destroy": (_int, [_vp]),
    "lsq_hip_comm_info": (_int, [_vp, ctypes.POINTER(ctypes.c_int32 * 8)]),
    "lsq_hip_comm_side_stream": (_vp, [_vp]),
    "lsq_hip_comm_join": (_int, [_vp, _vp]),
    "lsq_hip_comm_all_reduce": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp]),
    "lsq_hip_comm_all_reduce_begin": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp, ctypes.POINTER(ctypes.c_int32)]),
    "lsq_hip_comm_all_reduce_end": (_int, [_vp, ctypes.c_int32, _vp]),
    "lsq_hip_forward_per_channel_multi": (_int, [_int, ctypes.POINTER(LsqPcItem), ctypes.c_int32, _PP, _vp]),
    "lsq_hip_backward_per_channel_multi": (_int, [_int, ctypes.POINTER(LsqPcItem), ctypes.c_int32, _PP, _vp]),
    "lsq_hip_relayout": (_int, [_int, _vp, _vp, _i64, _i64, _i64, _vp]),
    "lsq_hip_backward_from_mask": (_int, [_int, _vp, _vp, _vp, _i64, _vp]),
    "lsq_hip_minmax_workspace": (_sz, [_int, _i64, _i64, _i64]),
    "lsq_hip_minmax_per_tensor": (_int, [_int, _vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "lsq_hip_minmax_per_channel": (_int, [_int, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _sz, _vp]),
    "lsq_hip_meanstd_workspace": (_sz, [_int, _i64, _i64, _i64]),
    "lsq_hip_meanstd_per_tensor": (_int, [_int, _vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "lsq_hip_meanstd_per_channel": (_int, [_int, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _sz, _vp]),
    "lsq_hip_observer_update": (_int, [_i64, _vp, _vp, _vp, _vp, ctypes.POINTER(LsqObserverUpdate), _vp, _vp, _vp]),
}
# NOT bound here: the `_ex` twins (a trailing launch-variant code) and the lsq_hip_debug_* knobs of csrc/lsq_internal.h.
# They exist only in the tools build of the library (tools/_tune/liblsq_hip_tools.so), which tools/lsq_tools.py loads and
# swaps in for this module's handle; the `variant` arguments below are for that build and raise on the production library.


def _load_library():
    """dlopen liblsq_hip.so and type its entry points (the replacement of reference extension.py:39-45)."""
    global _LIB
    if not os.path.isfile(_LIB_PATH):
        raise ImportError("%s not found -- build it with `python __graft_entry__.py` or "
                          "`make -C lsqfakequantize-pytorch_amd/csrc`" % _LIB_PATH)
    lib = ctypes.CDLL(_LIB_PATH)
    for name, (res, args) in C_ABI.items():
        fn = getattr(lib, name)  # AttributeError -> OSError-like failure below
        fn.restype = res
        fn.argtypes = args
    abi = lib.lsq_hip_abi_version()
    if abi != ABI_VERSION:
        raise ImportError("liblsq_hip.so has ABI version %d, this package needs %d" % (abi, ABI_VERSION))
    _LIB = lib


try:
    _load_library()
    _HAS_OPS = True
except (ImportError, OSError, AttributeError) as e:  # surfaced by _assert_has_ops(), like the reference
    error_str = str(e)


def _load_companion(name, table, version_fn, abi_version):
    """dlopen the companion library `name` next to liblsq_hip.so, type the entry points of `table` and check its ABI
    version (`version_fn`): (handle, "") or, when it cannot be used, (None, why).  The package works without it; its ops then raise."""
    try:
        lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), name))
        for fname, (res, args) in table.items():
            fn = getattr(lib, fname)
            fn.restype = res
            fn.argtypes = args
        abi = getattr(lib, version_fn)()
        if abi != abi_version:
            raise OSError("%s has ABI version %d, this package needs %d" % (name, abi, abi_version))
        return lib, ""
    except (OSError, AttributeError) as e:
        return None, str(e)


def _require_companion(lib, name, what, err):
    """`lib`, the ctypes handle of the companion library `name`; raises when it is missing (`err`: why)"""
    _assert_has_ops()
    if lib is None:
        raise RuntimeError("torchlsq: %s liblsq_hip_%s.so, which could not be loaded (build it with "
                           "`python __graft_entry__.py`): %s" % (what, name, err))
    return lib


# The kernels for tensors in host memory (include/lsq_cpu.h): the counterpart of the reference's CPU dispatch.
C_ABI_CPU = {
    "lsq_cpu_abi_version": (_int, []),
    "lsq_cpu_last_error": (ctypes.c_char_p, []),
    "lsq_cpu_set_num_threads": (None, [_int]),
    "lsq_cpu_forward_per_tensor": (_int, [_int, _vp, _vp, _i64, _vp, _vp, _PP]),
    "lsq_cpu_backward_per_tensor": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _PP]),
    "lsq_cpu_forward_per_channel": (_int, [_int, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _PP]),
    "lsq_cpu_backward_per_channel": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _PP]),
    "lsq_cpu_sharded_finish": (_int, [_int, _vp, _i64, ctypes.c_int32, _PP, _vp, _vp]),
}
_CPU_LIB, cpu_error_str = _load_companion("liblsq_cpu.so", C_ABI_CPU, "lsq_cpu_abi_version", ABI_VERSION)


# The group-wise ops, one tensor per call or many in one launch each way (include/lsq_hip_group.h): a companion library
# next to liblsq_hip.so, whose ABI (C_ABI above, pinned against include/lsq_hip.h) it leaves as it is.
class LsqGroupItem(ctypes.Structure):
    """lsq_group_item (include/lsq_hip_group.h): one tensor of a fused group-wise call."""
    _fields_ = [("x", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("y", ctypes.c_void_p), ("dx", ctypes.c_void_p),
                ("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p), ("ds", ctypes.c_void_p), ("db", ctypes.c_void_p),
                ("n", ctypes.c_int64), ("group_size", ctypes.c_int64)]


GROUP_ABI_VERSION = 2
GROUP_MULTI_ITEMS = 28          # LSQ_GROUP_MULTI_ITEMS: items per fused launch
_GIP = ctypes.POINTER(LsqGroupItem)
C_ABI_GROUP = {
    "lsq_group_abi_version": (_int, []),
    "lsq_group_last_error": (ctypes.c_char_p, []),
    "lsq_group_forward": (_int, [_int, _vp, _vp, _i64, _i64, _vp, _vp, _PP, _EP, _vp]),
    "lsq_group_backward": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _PP, _vp]),
    "lsq_group_plan": (_int, [_int, _i64, _i64, ctypes.POINTER(ctypes.c_int32 * 8)]),
    "lsq_group_multi_forward": (_int, [_int, _GIP, ctypes.c_int32, _PP, _vp]),
    "lsq_group_multi_backward": (_int, [_int, _GIP, ctypes.c_int32, _PP, _vp]),
    "lsq_group_multi_plan": (_int, [_int, _GIP, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
}
_GROUP_LIB, group_error_str = _load_companion("liblsq_hip_group.so", C_ABI_GROUP, "lsq_group_abi_version",
                                                GROUP_ABI_VERSION)


def group_library():
    """The ctypes handle of liblsq_hip_group.so (raises if it is missing)."""
    return _require_companion(_GROUP_LIB, "group", "the group-wise ops need", group_error_str)


# Packed 4- / 2-bit export of group-wise weights, and the way back (include/lsq_hip_pack.h): a third companion library; the
# ABIs above stay as they are.
PACK_ABI_VERSION = 1
C_ABI_PACK = {
    "lsq_pack_abi_version": (_int, []),
    "lsq_pack_last_error": (ctypes.c_char_p, []),
    "lsq_pack_quantize": (_int, [_int, _vp, _i64, _i64, _vp, _vp, _PP, _int, _vp, _vp, _vp, _vp]),
    "lsq_pack_dequantize": (_int, [_int, _vp, _i64, _i64, _int, _vp, _vp, _vp, _vp]),
    "lsq_pack_unpack": (_int, [_vp, _i64, _int, _int, _int, _vp, _vp]),
    "lsq_pack_plan": (_int, [_int, _i64, _i64, _int, ctypes.POINTER(ctypes.c_int32 * 8)]),
}
_PACK_LIB, pack_error_str = _load_companion("liblsq_hip_pack.so", C_ABI_PACK, "lsq_pack_abi_version", PACK_ABI_VERSION)


def pack_library():
    """The ctypes handle of liblsq_hip_pack.so (raises if it is missing)."""
    return _require_companion(_PACK_LIB, "pack", "the packed export ops need", pack_error_str)


# The linear layer that reads packed weights in place (include/lsq_hip_qlinear.h): a fourth companion library; the ABIs above
# stay as they are.
QLINEAR_ABI_VERSION = 1
QLINEAR_MAX_ROWS = 16           # LSQ_QLINEAR_MAX_ROWS: rows of x one launch serves
C_ABI_QLINEAR = {
    "lsq_qlinear_abi_version": (_int, []),
    "lsq_qlinear_last_error": (ctypes.c_char_p, []),
    "lsq_qlinear_forward": (_int, [_int, _vp, _i64, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _int, _vp, _vp]),
    "lsq_qlinear_plan": (_int, [_int, _i64, _i64, _i64, _i64, _int, ctypes.POINTER(ctypes.c_int32 * 8)]),
}
_QLINEAR_LIB, qlinear_error_str = _load_companion("liblsq_hip_qlinear.so", C_ABI_QLINEAR, "lsq_qlinear_abi_version",
                                                    QLINEAR_ABI_VERSION)


def qlinear_library():
    """The ctypes handle of liblsq_hip_qlinear.so (raises if it is missing)."""
    return _require_companion(_QLINEAR_LIB, "qlinear", "the packed linear op needs", qlinear_error_str)


# 8-bit activation levels on the packed codes (include/lsq_hip_qlinear_a8.h): a fifth companion library; the ABIs above stay as
# they are.
QLINEAR_A8_ABI_VERSION = 1
QLINEAR_A8_MAX_ROWS = 16        # LSQ_QLINEAR_A8_MAX_ROWS: rows of x one launch serves
LSQ_A8_U8, LSQ_A8_I8 = 0, 1     # level_dtype of lsq_qlinear_a8_forward_levels
C_ABI_QLINEAR_A8 = {
    "lsq_qlinear_a8_abi_version": (_int, []),
    "lsq_qlinear_a8_last_error": (ctypes.c_char_p, []),
    "lsq_qlinear_a8_forward_levels": (_int, [_int, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _int, _vp, _int,
                                             _vp]),
    "lsq_qlinear_a8_forward": (_int, [_int, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp,
                                      _int, _vp, _vp]),
    "lsq_qlinear_a8_plan": (_int, [_i64, _i64, _i64, _i64, _int, ctypes.POINTER(ctypes.c_int32 * 8)]),
}
_QLINEAR_A8_LIB, qlinear_a8_error_str = _load_companion("liblsq_hip_qlinear_a8.so", C_ABI_QLINEAR_A8, "lsq_qlinear_a8_abi_version",
                                                          QLINEAR_A8_ABI_VERSION)


def qlinear_a8_library():
    """The ctypes handle of liblsq_hip_qlinear_a8.so (raises if it is missing)."""
    return _require_companion(_QLINEAR_A8_LIB, "qlinear_a8", "the 8-bit-activation packed linear op needs", qlinear_a8_error_str)


# The same linear layer for more rows of x than the decode kernel serves: a matrix-core GEMM on the codes
# (include/lsq_hip_qgemm.h): a sixth companion library; the ABIs above stay as they are.
QGEMM_ABI_VERSION = 1
C_ABI_QGEMM = {
    "lsq_qgemm_abi_version": (_int, []),
    "lsq_qgemm_last_error": (ctypes.c_char_p, []),
    "lsq_qgemm_forward": (_int, [_int, _vp, _i64, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _int, _vp, _vp]),
    "lsq_qgemm_plan": (_int, [_int, _i64, _i64, _i64, _i64, _int, ctypes.POINTER(ctypes.c_int32 * 8)]),
}
_QGEMM_LIB, qgemm_error_str = _load_companion("liblsq_hip_qgemm.so", C_ABI_QGEMM, "lsq_qgemm_abi_version", QGEMM_ABI_VERSION)


def qgemm_library():
    """The ctypes handle of liblsq_hip_qgemm.so (raises if it is missing)."""
    return _require_companion(_QGEMM_LIB, "qgemm", "the packed linear op on more than %d rows needs" % QLINEAR_MAX_ROWS, qgemm_error_str)


# qlinear_a8 for more rows than its decode kernel serves: an int8 matrix-core GEMM on the codes with the decode kernel's
# bits (include/lsq_hip_qgemm_a8.h): a seventh companion library; the ABIs above stay as they are.
QGEMM_A8_ABI_VERSION = 1
C_ABI_QGEMM_A8 = {
    "lsq_qgemm_a8_abi_version": (_int, []),
    "lsq_qgemm_a8_last_error": (ctypes.c_char_p, []),
    "lsq_qgemm_a8_forward_levels": (_int, [_int, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _int, _vp, _int,
                                           _vp]),
    "lsq_qgemm_a8_forward": (_int, [_int, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp,
                                    _int, _vp, _vp, _vp]),
    "lsq_qgemm_a8_plan": (_int, [_i64, _i64, _i64, _i64, _int, ctypes.POINTER(ctypes.c_int32 * 8)]),
}
_QGEMM_A8_LIB, qgemm_a8_error_str = _load_companion("liblsq_hip_qgemm_a8.so", C_ABI_QGEMM_A8, "lsq_qgemm_a8_abi_version",
                                                      QGEMM_A8_ABI_VERSION)


def qgemm_a8_library():
    """The ctypes handle of liblsq_hip_qgemm_a8.so (raises if it is missing)."""
    return _require_companion(_QGEMM_A8_LIB, "qgemm_a8", "the 8-bit-activation packed linear op on more than %d rows needs"
                              % QLINEAR_A8_MAX_ROWS, qgemm_a8_error_str)


# W8A8: 8-bit activation levels times 8-bit weight levels with one (scale, zero point) per output row, any number of rows
# (include/lsq_hip_qlinear_w8.h): an eighth companion library; the ABIs above stay as they are.
QLINEAR_W8_ABI_VERSION = 1
LSQ_W8_U8, LSQ_W8_I8 = 0, 1     # level_dtype and w_level_dtype
C_ABI_QLINEAR_W8 = {
    "lsq_qlinear_w8_abi_version": (_int, []),
    "lsq_qlinear_w8_last_error": (ctypes.c_char_p, []),
    "lsq_qlinear_w8_forward_levels": (_int, [_int, _vp, _i64, _vp, _vp, _int, _vp, _i64, _i64, _vp, _vp, _vp, _int, _vp, _int, _vp]),
    "lsq_qlinear_w8_forward": (_int, [_int, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _i64, _i64, _vp, _vp, _vp, _int,
                                      _vp, _vp, _vp]),
    "lsq_qlinear_w8_plan": (_int, [_i64, _i64, _i64, _int, ctypes.POINTER(ctypes.c_int32 * 8)]),
}
_QLINEAR_W8_LIB, qlinear_w8_error_str = _load_companion("liblsq_hip_qlinear_w8.so", C_ABI_QLINEAR_W8, "lsq_qlinear_w8_abi_version",
                                                          QLINEAR_W8_ABI_VERSION)


def qlinear_w8_library():
    """The ctypes handle of liblsq_hip_qlinear_w8.so (raises if it is missing)."""
    return _require_companion(_QLINEAR_W8_LIB, "qlinear_w8", "the W8A8 linear op needs", qlinear_w8_error_str)


# W8A8 conv2d: the same arithmetic as an implicit GEMM on channels-last levels (include/lsq_hip_qconv_w8.h): a ninth companion
# library; the ABIs above stay as they are.
class LsqQconvW8Geom(ctypes.Structure):
    """lsq_qconv_w8_geom (include/lsq_hip_qconv_w8.h): x [B, H, W, Cin], weight [Cout, kh, kw, Cin], stride, padding, dilation."""
    _fields_ = [(name, ctypes.c_int64) for name in ("B", "Cin", "H", "W", "Cout", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw")]


QCONV_W8_ABI_VERSION = 1
_CGP = ctypes.POINTER(LsqQconvW8Geom)
C_ABI_QCONV_W8 = {
    "lsq_qconv_w8_abi_version": (_int, []),
    "lsq_qconv_w8_last_error": (ctypes.c_char_p, []),
    "lsq_qconv_w8_forward_levels": (_int, [_int, _vp, _vp, _vp, _CGP, _int, _vp, _vp, _vp, _vp, _int, _vp, _int, _vp]),
    "lsq_qconv_w8_forward": (_int, [_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _CGP, _int, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp]),
    "lsq_qconv_w8_plan": (_int, [_CGP, _int, ctypes.POINTER(ctypes.c_int32 * 8)]),
}
_QCONV_W8_LIB, qconv_w8_error_str = _load_companion("liblsq_hip_qconv_w8.so", C_ABI_QCONV_W8, "lsq_qconv_w8_abi_version",
                                                      QCONV_W8_ABI_VERSION)


def qconv_w8_library():
    """The ctypes handle of liblsq_hip_qconv_w8.so (raises if it is missing)."""
    return _require_companion(_QCONV_W8_LIB, "qconv_w8", "the W8A8 conv2d op needs", qconv_w8_error_str)


# W8A8 linear and conv2d with an 8-bit output: the next layer's per-tensor quantizer (and a ReLU) in the epilogue
# (include/lsq_hip_requant_w8.h): a tenth companion library; the ABIs above stay as they are.
class LsqRequantW8Out(ctypes.Structure):
    """lsq_requant_w8_out (include/lsq_hip_requant_w8.h): the output quantizer of one call"""
    _fields_ = [("out_scale", ctypes.c_void_p), ("out_shift", ctypes.c_void_p)] + \
               [(name, ctypes.c_int64) for name in ("quant_min", "quant_max", "type_min", "type_max", "relu", "mid_dtype")]


REQUANT_W8_ABI_VERSION = 1
_ROP = ctypes.POINTER(LsqRequantW8Out)
_PLAN9 = ctypes.POINTER(ctypes.c_int32 * 9)
C_ABI_REQUANT_W8 = {
    "lsq_requant_w8_abi_version": (_int, []),
    "lsq_requant_w8_last_error": (ctypes.c_char_p, []),
    "lsq_requant_w8_linear_levels": (_int, [_int, _vp, _i64, _vp, _vp, _int, _vp, _i64, _i64, _vp, _vp, _vp, _int, _ROP, _vp, _vp]),
    "lsq_requant_w8_linear": (_int, [_int, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _i64, _i64, _vp, _vp, _vp, _int,
                                     _ROP, _vp, _vp, _vp]),
    "lsq_requant_w8_conv_levels": (_int, [_int, _vp, _vp, _vp, _CGP, _int, _vp, _vp, _vp, _vp, _int, _ROP, _vp, _vp]),
    "lsq_requant_w8_conv": (_int, [_int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _CGP, _int, _vp, _vp, _vp, _vp, _int, _ROP, _vp, _vp,
                                   _vp]),
    "lsq_requant_w8_plan_linear": (_int, [_i64, _i64, _i64, _int, _int, _PLAN9]),
    "lsq_requant_w8_plan_conv": (_int, [_CGP, _int, _int, _PLAN9]),
}
_REQUANT_W8_LIB, requant_w8_error_str = _load_companion("liblsq_hip_requant_w8.so", C_ABI_REQUANT_W8, "lsq_requant_w8_abi_version",
                                                        REQUANT_W8_ABI_VERSION)


def requant_w8_library():
    """The ctypes handle of liblsq_hip_requant_w8.so (raises if it is missing)."""
    return _require_companion(_REQUANT_W8_LIB, "requant_w8", "the W8A8 ops with an 8-bit output need", requant_w8_error_str)


# W8A8 linear and conv2d that close a residual block: a residual given as levels added in the 8-bit epilogue
# (include/lsq_hip_resadd_w8.h): an eleventh companion library; the ABIs above stay as they are.
class LsqResaddW8Res(ctypes.Structure):
    """lsq_resadd_w8_res (include/lsq_hip_resadd_w8.h): the residual levels of one call and their device constants"""
    _fields_ = [("levels", ctypes.c_void_p), ("level_dtype", ctypes.c_int64), ("scale", ctypes.c_void_p), ("zero_point", ctypes.c_void_p)]


class LsqResaddW8Pre(ctypes.Structure):
    """lsq_resadd_w8_pre (include/lsq_hip_resadd_w8.h): the layer's own output fake-quantizer"""
    _fields_ = [("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p)] + \
               [(name, ctypes.c_int64) for name in ("quant_min", "quant_max", "type_min", "type_max")]


RESADD_W8_ABI_VERSION = 1
_RRP = ctypes.POINTER(LsqResaddW8Res)
_RPP = ctypes.POINTER(LsqResaddW8Pre)
_PLAN10 = ctypes.POINTER(ctypes.c_int32 * 10)
C_ABI_RESADD_W8 = {
    "lsq_resadd_w8_abi_version": (_int, []),
    "lsq_resadd_w8_last_error": (ctypes.c_char_p, []),
    "lsq_resadd_w8_linear_levels": (_int, [_int, _vp, _i64, _vp, _vp, _int, _vp, _i64, _i64, _vp, _vp, _vp, _int, _ROP, _RRP, _RPP, _vp,
                                           _vp]),
    "lsq_resadd_w8_conv_levels": (_int, [_int, _vp, _vp, _vp, _CGP, _int, _vp, _vp, _vp, _vp, _int, _ROP, _RRP, _RPP, _vp, _vp]),
    "lsq_resadd_w8_plan_linear": (_int, [_i64, _i64, _i64, _int, _int, _int, _PLAN10]),
    "lsq_resadd_w8_plan_conv": (_int, [_CGP, _int, _int, _int, _PLAN10]),
}
_RESADD_W8_LIB, resadd_w8_error_str = _load_companion("liblsq_hip_resadd_w8.so", C_ABI_RESADD_W8, "lsq_resadd_w8_abi_version",
                                                      RESADD_W8_ABI_VERSION)


def resadd_w8_library():
    """The ctypes handle of liblsq_hip_resadd_w8.so (raises if it is missing)."""
    return _require_companion(_RESADD_W8_LIB, "resadd_w8", "the W8A8 ops that add a levels residual need", resadd_w8_error_str)


# 2-D max and average pooling on channels-last 8-bit levels (include/lsq_hip_pool_w8.h): a twelfth companion library; the ABIs
# above stay as they are.
class LsqPoolW8Geom(ctypes.Structure):
    """lsq_pool_w8_geom (include/lsq_hip_pool_w8.h): x [B, H, W, C], kernel, stride, padding, dilation, ceil_mode"""
    _fields_ = [(name, ctypes.c_int64) for name in ("B", "C", "H", "W", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw", "ceil_mode")]


class LsqPoolW8Avg(ctypes.Structure):
    """lsq_pool_w8_avg (include/lsq_hip_pool_w8.h): the average pool's device constants, output quantizer (or none) and divisor"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("s_x", "zx", "out_scale", "out_shift")] + \
               [(name, ctypes.c_int64) for name in ("quant_min", "quant_max", "type_min", "type_max", "mid_dtype", "count_include_pad",
                                                    "has_divisor", "divisor_override")]


POOL_W8_ABI_VERSION = 1
_PGP = ctypes.POINTER(LsqPoolW8Geom)
_PLAN8 = ctypes.POINTER(ctypes.c_int32 * 8)
C_ABI_POOL_W8 = {
    "lsq_pool_w8_abi_version": (_int, []),
    "lsq_pool_w8_last_error": (ctypes.c_char_p, []),
    "lsq_pool_w8_max": (_int, [_int, _vp, _PGP, _vp, _vp]),
    "lsq_pool_w8_avg_forward": (_int, [_int, _vp, _PGP, ctypes.POINTER(LsqPoolW8Avg), _vp, _vp]),
    "lsq_pool_w8_adaptive": (_int, [_i64, _i64, _PGP]),
    "lsq_pool_w8_plan_max": (_int, [_PGP, _int, _PLAN8]),
    "lsq_pool_w8_plan_avg": (_int, [_PGP, _int, _PLAN8]),
}
_POOL_W8_LIB, pool_w8_error_str = _load_companion("liblsq_hip_pool_w8.so", C_ABI_POOL_W8, "lsq_pool_w8_abi_version", POOL_W8_ABI_VERSION)


def pool_w8_library():
    """The ctypes handle of liblsq_hip_pool_w8.so (raises if it is missing)."""
    return _require_companion(_POOL_W8_LIB, "pool_w8", "the pooling ops on 8-bit levels need", pool_w8_error_str)


# W8A8 depthwise conv2d (groups == C) on channels-last 8-bit levels, levels or floats out (include/lsq_hip_dwconv_w8.h): a
# thirteenth companion library; the ABIs above stay as they are.
class LsqDwconvW8Out(ctypes.Structure):
    """lsq_dwconv_w8_out (include/lsq_hip_dwconv_w8.h): the output quantizer (or none: floats), the activation and mid_dtype"""
    _fields_ = [("out_scale", ctypes.c_void_p), ("out_shift", ctypes.c_void_p)] + \
               [(name, ctypes.c_int64) for name in ("quant_min", "quant_max", "type_min", "type_max", "act", "mid_dtype")]


DWCONV_W8_ABI_VERSION = 1
_DOP = ctypes.POINTER(LsqDwconvW8Out)
C_ABI_DWCONV_W8 = {
    "lsq_dwconv_w8_abi_version": (_int, []),
    "lsq_dwconv_w8_last_error": (ctypes.c_char_p, []),
    "lsq_dwconv_w8_forward_levels": (_int, [_int, _vp, _vp, _vp, _CGP, _int, _vp, _vp, _vp, _vp, _int, _DOP, _vp, _vp]),
    "lsq_dwconv_w8_plan": (_int, [_CGP, _int, _int, _PLAN8]),
}
_DWCONV_W8_LIB, dwconv_w8_error_str = _load_companion("liblsq_hip_dwconv_w8.so", C_ABI_DWCONV_W8, "lsq_dwconv_w8_abi_version",
                                                        DWCONV_W8_ABI_VERSION)


def dwconv_w8_library():
    """The ctypes handle of liblsq_hip_dwconv_w8.so (raises if it is missing)."""
    return _require_companion(_DWCONV_W8_LIB, "dwconv_w8", "the W8A8 depthwise conv2d ops need", dwconv_w8_error_str)


# Elementwise ops on 8-bit levels: a 256-entry byte table and the SE gate multiply (include/lsq_hip_eltwise_w8.h): a fourteenth
# companion library; the ABIs above stay as they are.
class LsqEltwiseW8Shape(ctypes.Structure):
    """lsq_eltwise_w8_shape (include/lsq_hip_eltwise_w8.h): x and y [B, H, W, C], the gate [B, C]"""
    _fields_ = [(name, ctypes.c_int64) for name in ("B", "C", "H", "W")]


class LsqEltwiseW8Mul(ctypes.Structure):
    """lsq_eltwise_w8_mul (include/lsq_hip_eltwise_w8.h): the gate multiply's device constants, output quantizer (or none) and mid_dtype"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("s_x", "zx", "s_g", "zg", "out_scale", "out_shift")] + \
               [(name, ctypes.c_int64) for name in ("quant_min", "quant_max", "type_min", "type_max", "mid_dtype")]


ELTWISE_W8_ABI_VERSION = 1
_ESP = ctypes.POINTER(LsqEltwiseW8Shape)
C_ABI_ELTWISE_W8 = {
    "lsq_eltwise_w8_abi_version": (_int, []),
    "lsq_eltwise_w8_last_error": (ctypes.c_char_p, []),
    "lsq_eltwise_w8_lut": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "lsq_eltwise_w8_mul_gate": (_int, [_int, _vp, _int, _vp, _ESP, ctypes.POINTER(LsqEltwiseW8Mul), _vp, _vp]),
    "lsq_eltwise_w8_plan_lut": (_int, [_i64, _int, _PLAN8]),
    "lsq_eltwise_w8_plan_mul": (_int, [_ESP, _int, _PLAN8]),
}
_ELTWISE_W8_LIB, eltwise_w8_error_str = _load_companion("liblsq_hip_eltwise_w8.so", C_ABI_ELTWISE_W8, "lsq_eltwise_w8_abi_version",
                                                          ELTWISE_W8_ABI_VERSION)


def eltwise_w8_library():
    """The ctypes handle of liblsq_hip_eltwise_w8.so (raises if it is missing)."""
    return _require_companion(_ELTWISE_W8_LIB, "eltwise_w8", "the table op and the gate multiply on 8-bit levels need", eltwise_w8_error_str)


# LayerNorm and RMSNorm on 8-bit levels with exact integer row statistics (include/lsq_hip_norm_w8.h): a fifteenth companion
# library; the ABIs above stay as they are.
class LsqNormW8Geom(ctypes.Structure):
    """lsq_norm_w8_geom (include/lsq_hip_norm_w8.h): x and y [R, C], the kind of norm and the level dtype"""
    _fields_ = [(name, ctypes.c_int64) for name in ("R", "C", "kind", "x_dtype")]


class LsqNormW8Consts(ctypes.Structure):
    """lsq_norm_w8_consts (include/lsq_hip_norm_w8.h): the device constants, weight and bias (or none), output quantizer (or none),
    the dtypes and eps"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("s_x", "zx", "weight", "bias", "out_scale", "out_shift")] + \
               [(name, ctypes.c_int64) for name in ("param_dtype", "quant_min", "quant_max", "type_min", "type_max", "mid_dtype")] + \
               [("eps", ctypes.c_float)]


NORM_W8_ABI_VERSION = 1
_NGP = ctypes.POINTER(LsqNormW8Geom)
C_ABI_NORM_W8 = {
    "lsq_norm_w8_abi_version": (_int, []),
    "lsq_norm_w8_last_error": (ctypes.c_char_p, []),
    "lsq_norm_w8": (_int, [_NGP, ctypes.POINTER(LsqNormW8Consts), _vp, _vp, _vp]),
    "lsq_norm_w8_plan": (_int, [_NGP, _int, _int, _int, _PLAN8]),
}
_NORM_W8_LIB, norm_w8_error_str = _load_companion("liblsq_hip_norm_w8.so", C_ABI_NORM_W8, "lsq_norm_w8_abi_version", NORM_W8_ABI_VERSION)


def norm_w8_library():
    """The ctypes handle of liblsq_hip_norm_w8.so (raises if it is missing)."""
    return _require_companion(_NORM_W8_LIB, "norm_w8", "LayerNorm and RMSNorm on 8-bit levels need", norm_w8_error_str)


# The attention core on 8-bit levels: a strided batched matmul and a softmax on an integer table (include/lsq_hip_attn_w8.h): a
# sixteenth companion library; the ABIs above stay as they are.
class LsqAttnW8Strides(ctypes.Structure):
    """lsq_attn_w8_strides (include/lsq_hip_attn_w8.h): the two batch strides and the row stride of one tensor, in elements"""
    _fields_ = [(name, ctypes.c_int64) for name in ("s0", "s1", "ld")]


class LsqBmmW8Geom(ctypes.Structure):
    """lsq_bmm_w8_geom (include/lsq_hip_attn_w8.h): the extents, the form, the level dtypes and the strides of A, B and y"""
    _fields_ = [(name, ctypes.c_int64) for name in ("B0", "B1", "M", "N", "K", "form", "a_dtype", "b_dtype")] + \
               [(name, LsqAttnW8Strides) for name in ("a", "b", "y")]


class LsqAttnW8Out(ctypes.Structure):
    """lsq_attn_w8_out (include/lsq_hip_attn_w8.h): the output quantizer (or none: floats) and mid_dtype"""
    _fields_ = [("out_scale", ctypes.c_void_p), ("out_shift", ctypes.c_void_p)] + \
               [(name, ctypes.c_int64) for name in ("quant_min", "quant_max", "type_min", "type_max", "mid_dtype")]


class LsqBmmW8Consts(ctypes.Structure):
    """lsq_bmm_w8_consts (include/lsq_hip_attn_w8.h): each operand's scale and zero point on the device"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("s_a", "z_a", "s_b", "z_b")]


class LsqSoftmaxW8Geom(ctypes.Structure):
    """lsq_softmax_w8_geom (include/lsq_hip_attn_w8.h): x and y [R, C] with their row strides, and the level dtype"""
    _fields_ = [(name, ctypes.c_int64) for name in ("R", "C", "ldx", "ldy", "x_dtype")]


ATTN_W8_ABI_VERSION = 1
_BGP = ctypes.POINTER(LsqBmmW8Geom)
_AOP = ctypes.POINTER(LsqAttnW8Out)
_SGP = ctypes.POINTER(LsqSoftmaxW8Geom)
C_ABI_ATTN_W8 = {
    "lsq_attn_w8_abi_version": (_int, []),
    "lsq_attn_w8_last_error": (ctypes.c_char_p, []),
    "lsq_bmm_w8": (_int, [_BGP, ctypes.POINTER(LsqBmmW8Consts), _AOP, _vp, _vp, _vp, _vp]),
    "lsq_bmm_w8_plan": (_int, [_BGP, _int, _int, _int, _PLAN8]),
    "lsq_softmax_w8": (_int, [_SGP, _AOP, _vp, _vp, _vp, _vp]),
    "lsq_softmax_w8_plan": (_int, [_SGP, _int, _PLAN8]),
}
_ATTN_W8_LIB, attn_w8_error_str = _load_companion("liblsq_hip_attn_w8.so", C_ABI_ATTN_W8, "lsq_attn_w8_abi_version", ATTN_W8_ABI_VERSION)


def attn_w8_library():
    """The ctypes handle of liblsq_hip_attn_w8.so (raises if it is missing)."""
    return _require_companion(_ATTN_W8_LIB, "attn_w8", "batched matmul and softmax on 8-bit levels need", attn_w8_error_str)


# The attention core on 8-bit levels in one launch, scores and probabilities in LDS (include/lsq_hip_attn_fused_w8.h): a seventeenth
# companion library; the ABIs above stay as they are.
class LsqAttnFusedW8Geom(ctypes.Structure):
    """lsq_attn_fused_w8_geom (include/lsq_hip_attn_fused_w8.h): the extents, the level dtypes and the strides of q, k, v and y"""
    _fields_ = [(name, ctypes.c_int64) for name in ("B", "H", "Tq", "Tk", "D", "q_dtype", "k_dtype", "v_dtype")] + \
               [(name, LsqAttnW8Strides) for name in ("q", "k", "v", "y")]


class LsqAttnFusedW8Consts(ctypes.Structure):
    """lsq_attn_fused_w8_consts (include/lsq_hip_attn_fused_w8.h): the scale and zero point of q, k, v and of the probabilities as an
    operand, on the device"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("s_q", "z_q", "s_k", "z_k", "s_v", "z_v", "s_p", "z_p")]


ATTN_FUSED_W8_ABI_VERSION = 1
_AFGP = ctypes.POINTER(LsqAttnFusedW8Geom)
C_ABI_ATTN_FUSED_W8 = {
    "lsq_attn_fused_w8_abi_version": (_int, []),
    "lsq_attn_fused_w8_last_error": (ctypes.c_char_p, []),
    "lsq_attn_fused_w8": (_int, [_AFGP, ctypes.POINTER(LsqAttnFusedW8Consts), _AOP, _AOP, _AOP, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsq_attn_fused_w8_plan": (_int, [_AFGP, _int, _int, _PLAN8]),
}
_ATTN_FUSED_W8_LIB, attn_fused_w8_error_str = _load_companion("liblsq_hip_attn_fused_w8.so", C_ABI_ATTN_FUSED_W8,
                                                              "lsq_attn_fused_w8_abi_version", ATTN_FUSED_W8_ABI_VERSION)


def attn_fused_w8_library():
    """The ctypes handle of liblsq_hip_attn_fused_w8.so (raises if it is missing)."""
    return _require_companion(_ATTN_FUSED_W8_LIB, "attn_fused_w8", "the fused attention core on 8-bit levels needs", attn_fused_w8_error_str)


# The masked softmax on 8-bit levels: the integer-table softmax over a prefix of every row, causal and key-length masks
# (include/lsq_hip_attn_mask_w8.h): an eighteenth companion library; the ABIs above stay as they are.
class LsqSoftmaxMaskW8Geom(ctypes.Structure):
    """lsq_softmax_mask_w8_geom (include/lsq_hip_attn_mask_w8.h): x and y [R, C] with their row strides, the level dtype, and what
    makes a row's prefix length: Tq, the rows that share one entry of key_lengths, causal and its offset"""
    _fields_ = [(name, ctypes.c_int64) for name in ("R", "C", "ldx", "ldy", "x_dtype", "Tq", "rows_per_length", "causal", "causal_offset")]


ATTN_MASK_W8_ABI_VERSION = 1
_SMGP = ctypes.POINTER(LsqSoftmaxMaskW8Geom)
C_ABI_ATTN_MASK_W8 = {
    "lsq_attn_mask_w8_abi_version": (_int, []),
    "lsq_attn_mask_w8_last_error": (ctypes.c_char_p, []),
    "lsq_softmax_mask_w8": (_int, [_SMGP, _AOP, _vp, _vp, _vp, _vp, _vp]),
    "lsq_softmax_mask_w8_plan": (_int, [_SMGP, _int, _int, _PLAN8]),
}
_ATTN_MASK_W8_LIB, attn_mask_w8_error_str = _load_companion("liblsq_hip_attn_mask_w8.so", C_ABI_ATTN_MASK_W8,
                                                            "lsq_attn_mask_w8_abi_version", ATTN_MASK_W8_ABI_VERSION)


def attn_mask_w8_library():
    """The ctypes handle of liblsq_hip_attn_mask_w8.so (raises if it is missing)."""
    return _require_companion(_ATTN_MASK_W8_LIB, "attn_mask_w8", "the masked softmax on 8-bit levels needs", attn_mask_w8_error_str)


# Rotary position embedding and the KV-cache append on 8-bit levels, positions on the device (include/lsq_hip_rope_w8.h): a
# nineteenth companion library; the ABIs above stay as they are.
class LsqRopeW8Geom(ctypes.Structure):
    """lsq_rope_w8_geom (include/lsq_hip_rope_w8.h): x [B, T, H, D] and y [B, Tout, H, D] with their three strides each, the rotary
    dimension, the tables' positions, the level dtype, the pairing style, scatter and the mode"""
    _fields_ = [(name, ctypes.c_int64) for name in ("B", "T", "H", "D", "R", "P", "Tout", "x_sb", "x_st", "x_sh", "y_sb", "y_st", "y_sh",
                                                    "x_dtype", "style", "scatter", "mode")]


class LsqRopeW8In(ctypes.Structure):
    """lsq_rope_w8_in (include/lsq_hip_rope_w8.h): x's scale and zero point on the device"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("s_x", "zx")]


class LsqRopeW8Out(ctypes.Structure):
    """lsq_rope_w8_out (include/lsq_hip_rope_w8.h): the output quantizer (or none: floats) and mid_dtype"""
    _fields_ = [("out_scale", ctypes.c_void_p), ("out_shift", ctypes.c_void_p)] + \
               [(name, ctypes.c_int64) for name in ("quant_min", "quant_max", "type_min", "type_max", "mid_dtype")]


ROPE_W8_ABI_VERSION = 1
_RGP = ctypes.POINTER(LsqRopeW8Geom)
C_ABI_ROPE_W8 = {
    "lsq_rope_w8_abi_version": (_int, []),
    "lsq_rope_w8_last_error": (ctypes.c_char_p, []),
    "lsq_rope_w8": (_int, [_RGP, ctypes.POINTER(LsqRopeW8In), ctypes.POINTER(LsqRopeW8Out), _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsq_rope_w8_plan": (_int, [_RGP, _int, _PLAN8]),
}
_ROPE_W8_LIB, rope_w8_error_str = _load_companion("liblsq_hip_rope_w8.so", C_ABI_ROPE_W8, "lsq_rope_w8_abi_version", ROPE_W8_ABI_VERSION)


def rope_w8_library():
    """The ctypes handle of liblsq_hip_rope_w8.so (raises if it is missing)."""
    return _require_companion(_ROPE_W8_LIB, "rope_w8", "rotary embedding and the KV-cache append on 8-bit levels need", rope_w8_error_str)


# Decode attention on 8-bit levels against a grouped-query KV cache in one launch (include/lsq_hip_attn_decode_w8.h): a twentieth
# companion library; the ABIs above stay as they are.
class LsqAttnDecodeW8Geom(ctypes.Structure):
    """lsq_attn_decode_w8_geom (include/lsq_hip_attn_decode_w8.h): the extents, the level dtypes, the mask and the strides of q, k, v
    and y"""
    _fields_ = [(name, ctypes.c_int64) for name in ("B", "H", "Hkv", "Tq", "Tk", "D", "q_dtype", "k_dtype", "v_dtype", "causal",
                                                    "causal_offset", "has_lengths")] + \
               [(name, LsqAttnW8Strides) for name in ("q", "k", "v", "y")]


class LsqAttnDecodeW8Consts(ctypes.Structure):
    """lsq_attn_decode_w8_consts (include/lsq_hip_attn_decode_w8.h): the scale and zero point of q, k, v and of the probabilities as an
    operand, on the device"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("s_q", "z_q", "s_k", "z_k", "s_v", "z_v", "s_p", "z_p")]


ATTN_DECODE_W8_ABI_VERSION = 1
_ADGP = ctypes.POINTER(LsqAttnDecodeW8Geom)
C_ABI_ATTN_DECODE_W8 = {
    "lsq_attn_decode_w8_abi_version": (_int, []),
    "lsq_attn_decode_w8_last_error": (ctypes.c_char_p, []),
    "lsq_attn_decode_w8": (_int, [_ADGP, ctypes.POINTER(LsqAttnDecodeW8Consts), _AOP, _AOP, _AOP, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsq_attn_decode_w8_plan": (_int, [_ADGP, _int, _int, _PLAN8]),
}
_ATTN_DECODE_W8_LIB, attn_decode_w8_error_str = _load_companion("liblsq_hip_attn_decode_w8.so", C_ABI_ATTN_DECODE_W8,
                                                                "lsq_attn_decode_w8_abi_version", ATTN_DECODE_W8_ABI_VERSION)


def attn_decode_w8_library():
    """The ctypes handle of liblsq_hip_attn_decode_w8.so (raises if it is missing)."""
    return _require_companion(_ATTN_DECODE_W8_LIB, "attn_decode_w8", "decode attention on 8-bit levels needs", attn_decode_w8_error_str)


# Prefill attention on 8-bit levels in one launch: causal and key-length masked, grouped-query, any number of query rows
# (include/lsq_hip_attn_prefill_w8.h): a twenty-first companion library; the ABIs above stay as they are.  Its geometry and constants
# are lsq_attn_decode_w8's structs.
ATTN_PREFILL_W8_ABI_VERSION = 1
C_ABI_ATTN_PREFILL_W8 = {
    "lsq_attn_prefill_w8_abi_version": (_int, []),
    "lsq_attn_prefill_w8_last_error": (ctypes.c_char_p, []),
    "lsq_attn_prefill_w8": (_int, [_ADGP, ctypes.POINTER(LsqAttnDecodeW8Consts), _AOP, _AOP, _AOP, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsq_attn_prefill_w8_plan": (_int, [_ADGP, _int, _int, _PLAN8]),
}
_ATTN_PREFILL_W8_LIB, attn_prefill_w8_error_str = _load_companion("liblsq_hip_attn_prefill_w8.so", C_ABI_ATTN_PREFILL_W8,
                                                                  "lsq_attn_prefill_w8_abi_version", ATTN_PREFILL_W8_ABI_VERSION)


def attn_prefill_w8_library():
    """The ctypes handle of liblsq_hip_attn_prefill_w8.so (raises if it is missing)."""
    return _require_companion(_ATTN_PREFILL_W8_LIB, "attn_prefill_w8", "prefill attention on 8-bit levels needs", attn_prefill_w8_error_str)


# Split-key decode attention on 8-bit levels: one kv head's keys dealt to several workgroups, three launches and a caller-owned
# workspace (include/lsq_hip_attn_decode_split_w8.h): a twenty-second companion library; the ABIs above stay as they are.  Its geometry
# and constants are lsq_attn_decode_w8's structs.
ATTN_DECODE_SPLIT_W8_ABI_VERSION = 1
C_ABI_ATTN_DECODE_SPLIT_W8 = {
    "lsq_attn_decode_split_w8_abi_version": (_int, []),
    "lsq_attn_decode_split_w8_last_error": (ctypes.c_char_p, []),
    "lsq_attn_decode_split_w8_workspace": (_int, [_ADGP, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "lsq_attn_decode_split_w8": (_int, [_ADGP, ctypes.POINTER(LsqAttnDecodeW8Consts), _AOP, _AOP, _AOP, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        ctypes.c_int64, ctypes.c_int64, _vp]),
    "lsq_attn_decode_split_w8_plan": (_int, [_ADGP, _int, _int, ctypes.c_int64, _PLAN8]),
}
_ATTN_DECODE_SPLIT_W8_LIB, attn_decode_split_w8_error_str = _load_companion("liblsq_hip_attn_decode_split_w8.so", C_ABI_ATTN_DECODE_SPLIT_W8,
                                                                            "lsq_attn_decode_split_w8_abi_version",
                                                                            ATTN_DECODE_SPLIT_W8_ABI_VERSION)


def attn_decode_split_w8_library():
    """The ctypes handle of liblsq_hip_attn_decode_split_w8.so (raises if it is missing)."""
    return _require_companion(_ATTN_DECODE_SPLIT_W8_LIB, "attn_decode_split_w8", "split-key decode attention on 8-bit levels needs",
                              attn_decode_split_w8_error_str)


# A paged KV cache on 8-bit levels: the append into pages of a pool and the split-key decode attention reading the pool through a
# block table (include/lsq_hip_attn_paged_w8.h): a twenty-third companion library; the ABIs above stay as they are.  The decode's
# geometry and constants are lsq_attn_decode_w8's structs, the geometry's k and v strides being the pools' (page, head, slot).
class LsqAttnPagedW8Pages(ctypes.Structure):
    """lsq_attn_paged_w8_pages (include/lsq_hip_attn_paged_w8.h): the pages of a pool, the slots of a page, the entries of a block
    table row and the row stride of the block table"""
    _fields_ = [(name, ctypes.c_int64) for name in ("Np", "ps", "Mp", "bt_ld")]


class LsqKvAppendPagedW8Geom(ctypes.Structure):
    """lsq_kv_append_paged_w8_geom (include/lsq_hip_attn_paged_w8.h): the sources' extents and strides, the pages and the pools' strides"""
    _fields_ = [(name, ctypes.c_int64) for name in ("B", "T", "Hkv", "D")] + [("pages", LsqAttnPagedW8Pages)] + \
               [(name, ctypes.c_int64) for name in ("k_sb", "k_st", "k_sh", "v_sb", "v_st", "v_sh", "kp_sp", "kp_sh", "kp_ss", "vp_sp",
                                                    "vp_sh", "vp_ss")]


ATTN_PAGED_W8_ABI_VERSION = 1
_APPP = ctypes.POINTER(LsqAttnPagedW8Pages)
_KAGP = ctypes.POINTER(LsqKvAppendPagedW8Geom)
C_ABI_ATTN_PAGED_W8 = {
    "lsq_attn_paged_w8_abi_version": (_int, []),
    "lsq_attn_paged_w8_last_error": (ctypes.c_char_p, []),
    "lsq_attn_paged_w8_workspace": (_int, [_ADGP, _APPP, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "lsq_attn_paged_w8_decode": (_int, [_ADGP, _APPP, ctypes.POINTER(LsqAttnDecodeW8Consts), _AOP, _AOP, _AOP, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _vp, ctypes.c_int64, ctypes.c_int64, _vp]),
    "lsq_attn_paged_w8_plan": (_int, [_ADGP, _APPP, _int, _int, ctypes.c_int64, _PLAN8]),
    "lsq_kv_append_paged_w8": (_int, [_KAGP, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lsq_kv_append_paged_w8_plan": (_int, [_KAGP, _int, _PLAN8]),
}
_ATTN_PAGED_W8_LIB, attn_paged_w8_error_str = _load_companion("liblsq_hip_attn_paged_w8.so", C_ABI_ATTN_PAGED_W8,
                                                              "lsq_attn_paged_w8_abi_version", ATTN_PAGED_W8_ABI_VERSION)


def attn_paged_w8_library():
    """The ctypes handle of liblsq_hip_attn_paged_w8.so (raises if it is missing)."""
    return _require_companion(_ATTN_PAGED_W8_LIB, "attn_paged_w8", "the paged KV cache on 8-bit levels needs", attn_paged_w8_error_str)


# Chunked prefill attention on 8-bit levels: the split launches with the query rows of a kv head dealt to row tiles of 16, on a dense
# cache or on pools through a block table, and the mask mode that counts every row's keys back from key_lengths
# (include/lsq_hip_attn_chunk_w8.h): a twenty-fourth companion library; the ABIs above stay as they are.  Its geometry, constants and
# pages are lsq_attn_decode_w8's and lsq_attn_paged_w8's structs; its plans report nine values.
ATTN_CHUNK_W8_ABI_VERSION = 1
_PLAN9 = ctypes.POINTER(ctypes.c_int32 * 9)
C_ABI_ATTN_CHUNK_W8 = {
    "lsq_attn_chunk_w8_abi_version": (_int, []),
    "lsq_attn_chunk_w8_last_error": (ctypes.c_char_p, []),
    "lsq_attn_chunk_w8_workspace": (_int, [_ADGP, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "lsq_attn_chunk_paged_w8_workspace": (_int, [_ADGP, _APPP, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "lsq_attn_chunk_w8": (_int, [_ADGP, ctypes.POINTER(LsqAttnDecodeW8Consts), _AOP, _AOP, _AOP, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                 ctypes.c_int64, ctypes.c_int64, _vp]),
    "lsq_attn_chunk_paged_w8": (_int, [_ADGP, _APPP, ctypes.POINTER(LsqAttnDecodeW8Consts), _AOP, _AOP, _AOP, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp, ctypes.c_int64, ctypes.c_int64, _vp]),
    "lsq_attn_chunk_w8_plan": (_int, [_ADGP, _int, _int, ctypes.c_int64, _PLAN9]),
    "lsq_attn_chunk_paged_w8_plan": (_int, [_ADGP, _APPP, _int, _int, ctypes.c_int64, _PLAN9]),
}
_ATTN_CHUNK_W8_LIB, attn_chunk_w8_error_str = _load_companion("liblsq_hip_attn_chunk_w8.so", C_ABI_ATTN_CHUNK_W8,
                                                              "lsq_attn_chunk_w8_abi_version", ATTN_CHUNK_W8_ABI_VERSION)


def attn_chunk_w8_library():
    """The ctypes handle of liblsq_hip_attn_chunk_w8.so (raises if it is missing)."""
    return _require_companion(_ATTN_CHUNK_W8_LIB, "attn_chunk_w8", "chunked prefill attention on 8-bit levels needs", attn_chunk_w8_error_str)


# The gated product act(gate) * up of a gated MLP on 8-bit levels: a 256-entry float table on the gate byte, both operands read in
# place through a row stride (include/lsq_hip_glu_w8.h): a twenty-fifth companion library; the ABIs above stay as they are.
class LsqGluW8Shape(ctypes.Structure):
    """lsq_glu_w8_shape (include/lsq_hip_glu_w8.h): gate, up and y [rows, C], the row strides of gate and up in bytes"""
    _fields_ = [(name, ctypes.c_int64) for name in ("rows", "C", "gate_row_stride", "up_row_stride")]


class LsqGluW8Consts(ctypes.Structure):
    """lsq_glu_w8_consts (include/lsq_hip_glu_w8.h): up's device constants, the output quantizer (or none) and mid_dtype"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("s_u", "z_u", "out_scale", "out_shift")] + \
               [(name, ctypes.c_int64) for name in ("quant_min", "quant_max", "type_min", "type_max", "mid_dtype")]


GLU_W8_ABI_VERSION = 1
_GSP = ctypes.POINTER(LsqGluW8Shape)
C_ABI_GLU_W8 = {
    "lsq_glu_w8_abi_version": (_int, []),
    "lsq_glu_w8_last_error": (ctypes.c_char_p, []),
    "lsq_glu_w8": (_int, [_int, _vp, _int, _vp, _vp, _GSP, ctypes.POINTER(LsqGluW8Consts), _vp, _vp]),
    "lsq_glu_w8_plan": (_int, [_GSP, _int, _PLAN8]),
}
_GLU_W8_LIB, glu_w8_error_str = _load_companion("liblsq_hip_glu_w8.so", C_ABI_GLU_W8, "lsq_glu_w8_abi_version", GLU_W8_ABI_VERSION)


def glu_w8_library():
    """The ctypes handle of liblsq_hip_glu_w8.so (raises if it is missing)."""
    return _require_companion(_GLU_W8_LIB, "glu_w8", "the gated product on 8-bit levels needs", glu_w8_error_str)


# The optional second host layer: torchlsq/_lsq_torch.so, the C++ torch binding of the same C ABI
# (csrc/torch_binding/lsq_torch_binding.cpp, namespace `torchlsq_native`).  It adds no device code; it only
# moves the per-call tensor bookkeeping and the autograd node from Python to C++.  `functional.lsq` prefers it
# for GPU tensors; everything in this module keeps working without it.  TORCHLSQ_HOST_BINDING=ctypes skips it.
_NATIVE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lsq_torch.so")
_NATIVE_LSQ = None
native_error_str = ""


def _load_native_binding():
    global _NATIVE_LSQ, native_error_str
    if os.environ.get("TORCHLSQ_HOST_BINDING", "").lower() == "ctypes":
        native_error_str = "disabled by TORCHLSQ_HOST_BINDING=ctypes"
        return
    if not os.path.isfile(_NATIVE_PATH):
        native_error_str = "%s not found (make -C lsqfakequantize-pytorch_amd/csrc binding)" % _NATIVE_PATH
        return
    try:
        torch.ops.load_library(_NATIVE_PATH)
        if int(torch.ops.torchlsq_native._abi_version()) != ABI_VERSION:
            raise OSError("_lsq_torch.so was built against another ABI version of liblsq_hip.so")
        _NATIVE_LSQ = torch.ops.torchlsq_native.lsq.default
    except (OSError, RuntimeError, AttributeError) as e:
        native_error_str = str(e)


if _HAS_OPS:
    _load_native_binding()


def native_lsq():
    """`torch.ops.torchlsq_native.lsq` (the C++ front op + autograd node) or None when _lsq_torch.so is absent."""
    return _NATIVE_LSQ


def host_binding():
    """'native' (C++ torch binding loaded) or 'ctypes'."""
    return "native" if _NATIVE_LSQ is not None else "ctypes"


def set_host_binding(kind):
    """Switch `functional.lsq` between the two host layers at run time (tests, A/B measurements)."""
    global _NATIVE_LSQ
    if kind == "ctypes":
        _NATIVE_LSQ = None
    elif kind == "native":
        if not hasattr(torch.ops, "torchlsq_native") or not os.path.isfile(_NATIVE_PATH):
            raise RuntimeError("the C++ torch binding is not available: %s" % native_error_str)
        try:
            _NATIVE_LSQ = torch.ops.torchlsq_native.lsq.default
        except (AttributeError, RuntimeError):
            torch.ops.load_library(_NATIVE_PATH)
            _NATIVE_LSQ = torch.ops.torchlsq_native.lsq.default
    else:
        raise ValueError("host binding must be 'native' or 'ctypes'")


def _has_ops():
    return _HAS_OPS


def _assert_has_ops():
    if not _HAS_OPS:
        raise RuntimeError(
            "torchlsq (MI355X build): the native HIP library could not be loaded, so the LSQ ops are "
            "unavailable.  There is no CPU or eager fallback.  Build it with `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950).\n\nImport error details:\n\t%s" % error_str)


def library():
    """The ctypes handle of liblsq_hip.so (raises if it is missing)."""
    _assert_has_ops()
    return _LIB


def _check_hip_version():
    """Counterpart of the reference's _check_cuda_version (extension.py:71-96): the HIP runtime the
    library was compiled against must have the same major version as the one PyTorch uses."""
    if not _HAS_OPS:
        return -1
    v = int(_LIB.lsq_hip_runtime_version())
    hip = getattr(torch.version, "hip", None)
    if v > 0 and hip is not None:
        lib_major = v // 10000000
        t_major = int(hip.split(".")[0])
        if lib_major != t_major:
            raise RuntimeError("Detected that PyTorch and torchlsq were compiled with different HIP versions. "
                               "PyTorch has HIP Version=%s and torchlsq has HIP_VERSION=%d. "
                               "Please rebuild torchlsq against your PyTorch's ROCm." % (hip, v))
    return v

def set_library(lib):
    """Make `lib` (a typed ctypes handle exporting include/lsq_hip.h) the library the Python host layer calls; returns the
    previous handle.  For tools/lsq_tools.py (the tools build) -- the C++ binding keeps the library it was linked against."""
    global _LIB
    prev, _LIB = _LIB, lib
    return prev
