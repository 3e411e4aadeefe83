"""tests/w8_routes.py without a GPU: the CPU paths of the three decode-step hosts enter no library, the recorder names what goes
through a module's `_on_device` and calls through, and the module's binding is put back when the block raises."""
import pytest
import torch

import test_lindec_w8_cpu as D
import test_linglu_w8_cpu as G
import test_linrope_w8_cpu as P
from torchlsq import _hip_host, _lindec_w8_host, _linglu_w8_host, _linrope_w8_host, extension
from w8_routes import entered

HOSTS = (_lindec_w8_host, _linglu_w8_host, _linrope_w8_host)


def test_cpu_tensors_enter_no_library():
    with entered(_lindec_w8_host) as dec, entered(_linglu_w8_host) as glu, entered(_linrope_w8_host) as rope:
        c = D.case(*D.CPU_CASES[3])
        assert torch.equal(D.run(c), c["want"])
        c = G.case(*G.CPU_CASES[0])
        assert torch.equal(extension.linglu_w8_q(*G.args_of(c)), c["want"])
        c = P.case(*P.CPU_CASES[0])
        assert torch.equal(P.call(c)[0], c["want"][0])
    assert dec == [] and glu == [] and rope == []
    assert all(m._on_device is _hip_host._on_device for m in HOSTS)


@pytest.mark.parametrize("host", HOSTS, ids=lambda m: m.__name__.rsplit(".", 1)[-1])
def test_recorder_names_the_symbol_calls_through_and_is_undone(host, monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)    # `_on_device` asks for it; there is no device here

    def lsq_some_launch(a, b):
        return a - b

    with entered(host) as names:
        assert host._on_device is not _hip_host._on_device
        assert host._on_device(0, lsq_some_launch, 7, 4) == 3 and host._on_device(0, lsq_some_launch, 1, 1) == 0
        assert all(m._on_device is _hip_host._on_device for m in HOSTS if m is not host)    # the other modules' bindings are theirs
    assert names == ["lsq_some_launch"] * 2 and host._on_device is _hip_host._on_device
    with pytest.raises(KeyError):
        with entered(host) as names:
            host._on_device(0, lsq_some_launch, 2, 1)
            raise KeyError("inside the block")
    assert names == ["lsq_some_launch"] and host._on_device is _hip_host._on_device


def test_ctypes_gives_a_function_pointer_the_name_of_its_symbol():
    """what the GPU tests compare the recorded names with"""
    assert extension.lindec_w8_library().lsq_lindec_w8_linear_levels.__name__ == "lsq_lindec_w8_linear_levels"
    assert extension.linglu_w8_library().lsq_linglu_w8.__name__ == "lsq_linglu_w8"
    assert extension.linrope_w8_library().lsq_linrope_w8.__name__ == "lsq_linrope_w8"
