"""CPU: the C-ABI library loads without a GPU and exports exactly what include/lsq_hip.h declares.

No compute entry point is executed here (there is no GPU); only host-side helpers and the argument
validation that happens before any HIP call.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsq_hip.h")
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip.so")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lsq_hip_\w+)\s*\(", text)))


def test_header_symbols_are_exported():
    names = _declared()
    assert len(names) == 37, names
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("lsq_")))
    # exported == declared, not a superset: no `_ex` twin, no lsq_hip_debug_* knob, nothing else with C linkage
    assert exported == names, "C symbols exported %s != declared in include/lsq_hip.h %s" % (exported, names)
    assert "debug" not in nm
    lib = ctypes.CDLL(LIB)
    for n in names:
        getattr(lib, n)


def test_tools_build_carries_the_internal_entry_points():
    """tools/_tune/liblsq_hip_tools.so (-DLSQ_TOOLS): include/lsq_hip.h plus csrc/lsq_internal.h, typed by tools/lsq_tools.py"""
    import lsq_tools
    lib = lsq_tools.load()
    assert lib.lsq_hip_abi_version() == 6
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "csrc", "lsq_internal.h")).read(), flags=re.S)
    internal = sorted(set(re.findall(r"\b(lsq_hip_\w+)\s*\(", text)))
    assert internal == sorted(lsq_tools.internal_abi()), (internal, sorted(lsq_tools.internal_abi()))
    for n in internal:
        getattr(lib, n)


def test_python_binding_table_matches_header():
    from torchlsq import extension as E
    assert sorted(E.C_ABI) == _declared()
    assert E._HAS_OPS and E.library().lsq_hip_abi_version() == E.ABI_VERSION == 6
    assert E.library().lsq_hip_runtime_version() > 0
    import torch
    assert torch.ops.torchlsq._cuda_version() == E.library().lsq_hip_runtime_version()


def test_struct_layouts():
    from torchlsq import extension as E
    assert ctypes.sizeof(E.LsqParams) == 48        # 8 x int32 + double + int64
    assert E.LsqParams.grad_scaler.offset == 32 and E.LsqParams.numel_for_scaler.offset == 40
    assert ctypes.sizeof(E.LsqFwdExtras) == 16


def test_host_grad_scaler_matches_reference_chain(small_cases):
    """lsq_hip_grad_scaler is pure host code: same bits as the reference-derived golden records."""
    from torchlsq import extension as E
    lib = E.library()
    for r in small_cases[0]["scaler_chain"]:
        dt = np.dtype(r["dtype"])
        n = int(np.prod(r["shape"]))
        code = E.LSQ_F32 if dt == np.float32 else E.LSQ_F64
        C = r["shape"][r["axis"]] if r["kind"] == "pc" else 1
        s = lib.lsq_hip_grad_scaler(code, int(r["kind"] == "pc"), n, r["qmax"], C, 1, r["grad_scaler"])
        got = np.array([r["qmax"]], dtype=dt) * np.array([s], dtype=dt)
        assert got.tobytes() == bytes.fromhex(r["ds_hex"]), r
    assert lib.lsq_hip_grad_scaler(E.LSQ_F32, 0, 1000, 127, 1, 0, 0.25) == 0.25


def test_argument_validation_never_reaches_the_gpu():
    from torchlsq import extension as E
    lib = E.library()
    p = E.LsqParams(0, 127, 0, 255, 1, 0, 0, 0, 1.0, 0)
    bad = E.LsqParams(5, 1, 0, 255, 1, 0, 0, 0, 1.0, 0)
    assert lib.lsq_hip_forward_per_tensor(99, None, None, 16, None, None, ctypes.byref(p), None, None) == -1
    assert b"dtype" in lib.lsq_hip_last_error()
    assert lib.lsq_hip_forward_per_tensor(0, None, None, 16, None, None, None, None, None) == -1
    assert lib.lsq_hip_forward_per_tensor(0, None, None, 16, None, None, ctypes.byref(bad), None, None) == -1
    assert lib.lsq_hip_forward_per_tensor(0, None, None, -4, None, None, ctypes.byref(p), None, None) == -1
    assert lib.lsq_hip_forward_per_tensor(0, None, None, 16, None, None, ctypes.byref(p), None, None) == -1   # NULL buffers
    assert b"NULL" in lib.lsq_hip_last_error()
    assert lib.lsq_hip_forward_per_tensor(0, None, None, 0, None, None, ctypes.byref(p), None, None) == 0     # empty: no-op
    assert lib.lsq_hip_backward_per_tensor(0, None, None, None, None, None, None, 0, None, None, ctypes.byref(p), None, None, 0, None) == -1
    assert lib.lsq_hip_backward_per_channel(0, None, None, None, None, None, None, 4, 0, 4, None, None, ctypes.byref(p), None, None, 0, None) == -1
    assert lib.lsq_hip_forward_per_channel(0, None, None, 0, 8, 4, None, None, ctypes.byref(p), None, None) == 0
    assert lib.lsq_hip_backward_per_tensor_workspace(0, 1 << 20) >= 256 * 8 * 16
    # ABI v4: the sharded epilogue and the levels-only forward validate before they launch, too
    assert lib.lsq_hip_sharded_finish(0, None, 4, 1, ctypes.byref(p), None, None, None) == -1 and b"NULL" in lib.lsq_hip_last_error()
    assert lib.lsq_hip_sharded_finish(0, 8, 0, 1, ctypes.byref(p), 8, 8, None) == -1                   # no channels
    assert lib.lsq_hip_sharded_finish(0, 8, 3, 0, ctypes.byref(p), 8, 8, None) == -1                   # per-tensor has one channel
    assert lib.lsq_hip_sharded_finish(0, 12, 1, 0, ctypes.byref(p), 8, 8, None) == -1 and b"aligned" in lib.lsq_hip_last_error()
    wide = E.LsqParams(-200, 127, -200, 255, 1, 0, 0, 0, 1.0, 0)          # 328 levels: fit neither int8 nor uint8
    ex = E.LsqFwdExtras(64, 0, 0)
    assert lib.lsq_hip_forward_per_tensor(0, 64, None, 16, 64, 64, ctypes.byref(wide), ctypes.byref(ex), None) == -1
    assert b"neither int8 nor uint8" in lib.lsq_hip_last_error()
    assert lib.lsq_hip_forward_per_tensor(0, 64, None, 16, 64, 64, ctypes.byref(p), None, None) == -1    # y == NULL needs levels


def test_cpu_library_exports_its_header_and_devices_never_substitute():
    """include/lsq_cpu.h <-> liblsq_cpu.so <-> the ctypes table; CPU tensors are served by the CPU kernels, and neither
    device's kernels ever stand in for the other's: without the HIP library the package refuses CPU tensors too."""
    import pytest
    import torch
    import torchlsq  # noqa: F401
    from torchlsq import extension as E
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsq_cpu.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(lsq_cpu_\w+)\s*\(", text)))
    assert declared == sorted(E.C_ABI_CPU) and len(declared) == 8
    cpu_lib = os.path.join(os.path.dirname(LIB), "liblsq_cpu.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", cpu_lib], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if " T " in l)
    assert set(declared) <= exported
    undefined = subprocess.run(["nm", "-D", "--undefined-only", cpu_lib], capture_output=True, text=True, check=True).stdout
    assert "hip" not in undefined.lower() and "lsq_oracle" not in undefined     # host code only, and not the oracle
    x, s, b = torch.linspace(-1, 3, 64), torch.tensor([0.03]), torch.tensor([0.1])
    y = torch.ops.torchlsq.lsq_forward_per_tensor(x, s, b, 0, 127, 0, 255, True, 1.0, False, False, False)
    assert y.device.type == "cpu" and y.shape == x.shape and not torch.equal(y, x)
    # the package is the MI355X build: no HIP library -> nothing works, CPU tensors included
    from torchlsq import _abi
    saved = _abi._HAS_OPS
    _abi._HAS_OPS = False
    try:
        with pytest.raises(RuntimeError, match="native HIP library could not be loaded"):
            torch.ops.torchlsq.lsq_forward_per_tensor(x, s, b, 0, 127, 0, 255, True, 1.0, False, False, False)
    finally:
        _abi._HAS_OPS = saved
    # a CPU parameter next to a GPU tensor (or the reverse) is an error, not a silent copy
    with pytest.raises(RuntimeError, match="expected all tensors on the CPU"):
        E.cpu_forward(x, s.to("meta"), b, 0, False, 0, 127, 0, 255, True, 1.0, False, False, False)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "lsqfakequantize-pytorch_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "lsq_oracle" not in text and "from oracle" not in text and "import oracle" not in text, f


def test_cpp_torch_binding_uses_only_the_public_abi():
    """torchlsq/_lsq_torch.so (csrc/torch_binding) is host code over the SAME header:
    every lsq_hip_* symbol it imports is declared in include/lsq_hip.h (none of the internal `_ex` twins), it
    contains no device code, and it registers the reference's operator set under `torchlsq_native`."""
    import torch
    from torchlsq import extension as E
    binding = os.path.join(os.path.dirname(LIB), "_lsq_torch.so")
    assert os.path.isfile(binding), "build it: make -C lsqfakequantize-pytorch_amd/csrc binding"
    nm = subprocess.run(["nm", "-D", "--undefined-only", binding], capture_output=True, text=True, check=True).stdout
    imported = sorted(set(l.split()[-1] for l in nm.splitlines() if "lsq_hip_" in l))
    assert imported and set(imported) <= set(_declared()), imported
    for needed in ("lsq_hip_forward_per_tensor", "lsq_hip_backward_per_tensor", "lsq_hip_forward_per_channel",
                   "lsq_hip_backward_per_channel", "lsq_hip_backward_from_mask"):
        assert needed in imported
    sections = subprocess.run(["readelf", "-S", "-W", binding], capture_output=True, text=True, check=True).stdout
    assert ".hip_fatbin" not in sections and ".hipFatBinSegment" not in sections
    assert E.host_binding() == "native", E.native_error_str
    ns = torch.ops.torchlsq_native
    assert int(ns._abi_version()) == E.ABI_VERSION
    ref = torch.ops.torchlsq
    for op in ("lsq", "lsq_forward_per_tensor", "lsq_backward_per_tensor", "lsq_forward_per_channel", "lsq_backward_per_channel"):
        a = str(getattr(ns, op).default._schema).split("(", 1)[1]
        b = str(getattr(ref, op).default._schema).split("(", 1)[1]
        assert a == b, (op, a, b)                       # argument lists identical to the reference schemas
    # CPU tensors: this binding is the GPU host layer only -- no kernel registered for them, never a fallback
    x, s, b = torch.zeros(4), torch.ones(1), torch.zeros(1)
    import pytest
    with pytest.raises(NotImplementedError):
        ns.lsq_forward_per_tensor(x, s, b, 0, 255, 0, 255, True, 1.0, False, False, False)
    with pytest.raises(RuntimeError, match="expected a tensor on the GPU"):
        ns.lsq(x, s, b, 0, 255, 0, 255, 1, True, 1.0, True, False, False, False)
    # switching host layers at run time
    E.set_host_binding("ctypes")
    assert E.host_binding() == "ctypes" and E.native_lsq() is None
    E.set_host_binding("native")
    assert E.host_binding() == "native"


def test_comm_entry_points_validate_before_anything_else():
    """lsq_hip_comm_*: RCCL is resolved lazily with dlopen (no link dependency: the library loaded above), a unique id can be
    made without a GPU, and bad arguments come back as LSQ_EINVAL with a message -- nothing is launched here."""
    from torchlsq import extension as E
    lib = E.library()
    needed = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "rccl" not in needed.lower() and "nccl" not in needed.lower()
    uid = E.HipComm.unique_id()
    assert len(uid) == E.LSQ_COMM_ID_BYTES and any(uid)
    assert lib.lsq_hip_comm_unique_id(None) == -1 and b"NULL" in lib.lsq_hip_last_error()
    out = ctypes.c_void_p()
    buf = (ctypes.c_ubyte * E.LSQ_COMM_ID_BYTES).from_buffer_copy(uid)
    assert lib.lsq_hip_comm_create(ctypes.cast(buf, ctypes.c_void_p), 3, 2, None, ctypes.byref(out)) == -1      # rank 3 of 2
    assert b"rank 3 of 2" in lib.lsq_hip_last_error() and not out.value
    # options are arguments, validated like any other (lsq_comm_options: a sized struct, NULL = defaults)
    from torchlsq import _abi
    assert ctypes.sizeof(_abi.LsqCommOptions) == 16
    bad = _abi.LsqCommOptions(size=16, event_system_fence=7)
    assert lib.lsq_hip_comm_create(ctypes.cast(buf, ctypes.c_void_p), 0, 1, ctypes.byref(bad), ctypes.byref(out)) == -1
    assert b"event_system_fence" in lib.lsq_hip_last_error() and not out.value
    short = _abi.LsqCommOptions(size=2)
    assert lib.lsq_hip_comm_create(ctypes.cast(buf, ctypes.c_void_p), 0, 1, ctypes.byref(short), ctypes.byref(out)) == -1
    assert lib.lsq_hip_comm_tune(None, None) == -1 and lib.lsq_hip_comm_configure(None, None) == -1
    assert lib.lsq_hip_comm_all_reduce(None, None, None, 1, E.LSQ_F64, E.LSQ_COMM_SUM, None) == -1
    assert lib.lsq_hip_comm_all_reduce_end(None, 0, None) == -1 and lib.lsq_hip_comm_join(None, None) == -1
    assert lib.lsq_hip_comm_destroy(None) == 0 and not lib.lsq_hip_comm_side_stream(None)


def test_the_shipped_library_reads_no_environment_variable():
    """include/lsq_hip.h: "no behaviour depends on the process environment" -- the product binary does not even import getenv
    (RCCL, resolved with dlopen, reads its own NCCL_* / RCCL_* variables: that is RCCL's contract, not this library's); the
    experiment switches of earlier rounds (LSQ_COMM_PICK_STREAM, LSQ_COMM_EVENT_FENCE) are lsq_comm_options / lsq_hip_comm_tune now"""
    und = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    imported = sorted(set(l.split()[-1].split("@")[0] for l in und.splitlines() if l.strip()))
    assert not [n for n in imported if "getenv" in n], [n for n in imported if "getenv" in n]
    src = open(os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "csrc", "lsq_comm.hip")).read()
    assert "getenv" not in src


def test_plan_query_answers_without_launching_anything():
    """lsq_hip_plan_backward_per_channel on a box without a GPU: the CU count falls back to MI355X's 256, the kernel families
    come out as on the GPU (tests/test_shipped_binary_gpu.py asserts them there together with the results)"""
    from torchlsq import extension as E
    lib = E.library()
    p = E.LsqParams(0, 127, 0, 255, 1, 0, 0, 0, 1.0, 0)

    def kind(code, outer, C, inner, aligned=1):
        out = (ctypes.c_int32 * 8)()
        assert lib.lsq_hip_plan_backward_per_channel(code, outer, C, inner, aligned, ctypes.byref(p), ctypes.byref(out)) == 0
        return out[4], out[6]
    assert kind(E.LSQ_BF16, 64, 2048, 49)[0] == 4 and kind(E.LSQ_F32, 33, 2048, 49)[0] == 4          # owner windows
    assert kind(E.LSQ_F32, 320, 256, 196)[0] == 1                                                       # 256-lane windows
    assert kind(E.LSQ_BF16, 12608, 768, 1) == (2, 768) and kind(E.LSQ_F32, 12608, 768, 1) == (2, 256)   # row groups, fat / usual
    assert kind(E.LSQ_F32, 1, 512, 4608)[0] == 3                                                        # segment walk (config 3)
    assert kind(E.LSQ_BF16, 64, 2048, 49, aligned=0)[0] == 1                                            # unaligned: element-wise windows
    out = (ctypes.c_int32 * 8)()
    assert lib.lsq_hip_plan_backward_per_channel(E.LSQ_F32, 0, 8, 8, 1, ctypes.byref(p), ctypes.byref(out)) == -1


def test_per_channel_ops_reject_buffers_that_are_not_element_aligned():
    """include/lsq_hip.h: the per-channel forward and backward take element-aligned x / y / grad / dx only (the launch policy
    plans for nothing else): a misaligned one is LSQ_EINVAL before anything is planned or launched.  Fake addresses, as in the
    plan test above -- a library without the check would launch kernels on them, so this runs only where no GPU is visible."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("fake buffer addresses: checked on machines without a GPU only")
    from torchlsq import extension as E
    lib = E.library()
    p = E.LsqParams(0, 127, 0, 255, 1, 0, 0, 0, 1.0, 0)
    ok = 1 << 20
    for code, esz in ((E.LSQ_F32, 4), (E.LSQ_F64, 8), (E.LSQ_BF16, 2), (E.LSQ_F16, 2)):
        bad = ok + esz // 2
        for x, y in ((bad, ok), (ok, bad)):
            assert lib.lsq_hip_forward_per_channel(code, x, y, 64, 32, 49, ok, ok, ctypes.byref(p), None, None) == -1     # LSQ_EINVAL
            assert b"element-aligned" in lib.lsq_hip_last_error()
        for grad, x, dx in ((bad, ok, ok), (ok, bad, ok), (ok, ok, bad)):
            assert lib.lsq_hip_backward_per_channel(code, grad, x, dx, ok, ok, None, 64, 32, 49, ok, ok, ctypes.byref(p), None,
                                                    ok, 1 << 30, None) == -1
            assert b"element-aligned" in lib.lsq_hip_last_error()
