"""CPU: the fused group-wise calls (lsq_group_multi_* of include/lsq_hip_group.h, liblsq_hip_group.so,
torchlsq.functional.lsq_foreach_per_group, LSQWeightGroup(group_wise=True)) without a GPU.

  * their gfx950 code objects follow the device-code rules of tests/test_group_cpu.py;
  * argument validation fails the whole call for a bad item anywhere in the list, before anything is launched;
  * the host-only plan gives every item its single call's grids;
  * CPU tensors go through lsq_per_group one by one: same values and gradients.
"""
import ctypes
import os
import re

import pytest
import torch

from helpers import gfx950_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lsqfakequantize-pytorch_amd", "torchlsq", "liblsq_hip_group.so")


@pytest.fixture(scope="module")
def multi_kernels(tmp_path_factory):
    every = gfx950_kernels(LIB, str(tmp_path_factory.mktemp("grpmulticode")))
    out = {n: v for n, v in every.items() if "_grp_multi_kernel" in n}
    # 4 storage types x (forward: init x form = 4; backward: 6 mode combinations x 3 reductions = 18)
    assert len([n for n in out if "fwd_grp_multi_kernel" in n]) == 16, sorted(out)
    assert len([n for n in out if "bwd_grp_multi_kernel" in n]) == 72, sorted(out)
    return out


def test_fused_kernels_follow_the_device_code_rules(multi_kernels):
    """no scratch, no v_fma_mix, contraction off (FMAs only inside the correctly rounded division), 16-byte packets"""
    packets = 0
    for name, (body, scratch) in multi_kernels.items():
        ops = re.findall(r"^\s+([a-z_0-9]+)\s", body, re.M)
        assert scratch == 0 and not [o for o in ops if o.startswith("scratch_")], "%s uses %d bytes of scratch" % (name, scratch)
        assert not [o for o in ops if o.startswith("v_fma_mix") or o.startswith("v_mad_mix")], name
        n_fma = sum(1 for o in ops if re.fullmatch(r"v_(fma|fmac|mad|mac)_f(32|64)(_e32|_e64)?", o))
        n_div = sum(1 for o in ops if o.startswith("v_div_fmas_f"))
        assert n_fma <= 5 * n_div, "%s: %d FMAs for %d divisions" % (name, n_fma, n_div)
        # packet form (forward PACKET = true: last template argument Lb1E; backward modes 0 and 1): dwordx4 in and out
        if re.search(r"fwd_grp_multi_kernelI.*Lb1EEEv", name) or re.search(r"bwd_grp_multi_kernelI.*Li[01]EEEv", name):
            assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops, name
            packets += 1
    assert packets == 8 + 48


def _items(E, specs, ok=1 << 20):
    """lsq_group_item array from (n, G) pairs with fake, aligned addresses (validation only: nothing may launch)"""
    arr = (E.LsqGroupItem * max(1, len(specs)))()
    for k, (n, G) in enumerate(specs):
        it = arr[k]
        it.x = it.grad = it.y = it.dx = it.scale = it.shift = it.ds = it.db = ok + k * (1 << 16)
        it.n, it.group_size = n, G
    return arr


def test_fused_argument_validation_fails_the_whole_call():
    from torchlsq import extension as E
    lib = E.group_library()
    p = E.LsqParams(-8, 7, -128, 127, 1, 1, 0, 0, 1.0, 0)
    pp = ctypes.byref(p)
    good = [(256, 32), (768 * 4, 128), (96 * 3, 96), (24, 3), (0, 7)]

    def err():
        return lib.lsq_group_last_error()

    calls = (lib.lsq_group_multi_forward, lib.lsq_group_multi_backward)
    for call in calls:
        for bad_at in (0, 2, len(good)):          # first, middle and last item
            for (n, G), msg in (((250, 32), b"multiple of group_size"), ((256, 0), b"group_size must be positive"),
                                ((-32, 32), b"negative element count")):
                specs = list(good)
                specs.insert(bad_at, (n, G))
                arr = _items(E, specs)
                assert call(E.LSQ_F32, arr, len(specs), pp, None) == -1
                assert msg in err() and (b"item %d:" % bad_at) in err(), err()
            for field, off, msg in (("x", 0, b"NULL"), ("scale", 0, b"NULL"), ("x", 2, b"element-aligned"),
                                    ("shift", 2, b"element-aligned")):
                arr = _items(E, good)
                setattr(arr[bad_at % len(good)], field, None if off == 0 else getattr(arr[bad_at % len(good)], field) + off)
                assert call(E.LSQ_F32, arr, len(good), pp, None) == -1
                assert msg in err() and (b"item %d:" % (bad_at % len(good))) in err(), err()
        arr = _items(E, good)
        assert call(E.LSQ_F32, arr, -1, pp, None) == -1 and b"negative item count" in err()
        assert call(E.LSQ_F32, None, 3, pp, None) == -1 and b"items is NULL" in err()
        assert call(9, arr, len(good), pp, None) == -1 and b"dtype" in err()
        assert call(E.LSQ_F32, arr, len(good), None, None) == -1 and b"NULL" in err()
        shard = E.LsqParams(-8, 7, -128, 127, 1, 1, 0, 0, 1.0, 4096)
        assert call(E.LSQ_F32, arr, len(good), ctypes.byref(shard), None) == -1 and b"numel_for_scaler" in err()
        bad = E.LsqParams(7, -8, -128, 127, 1, 1, 0, 0, 1.0, 0)
        assert call(E.LSQ_F32, arr, len(good), ctypes.byref(bad), None) == -1 and b"quant_min" in err()
        # f64 elements need 8-byte alignment; the parameters of 16-bit storage are fp32 (4 bytes)
        arr = _items(E, good)
        arr[1].x += 4
        assert call(E.LSQ_F64, arr, len(good), pp, None) == -1 and b"item 1:" in err()
        # an empty item's buffers are not read; nothing to do is not an error
        arr = _items(E, [(0, 8)])
        arr[0].x = arr[0].y = arr[0].grad = arr[0].dx = None
        assert call(E.LSQ_BF16, arr, 1, pp, None) == 0 and call(E.LSQ_BF16, arr, 0, pp, None) == 0
    # direction-specific buffers
    arr = _items(E, good)
    arr[3].dx = None
    assert lib.lsq_group_multi_backward(E.LSQ_F32, arr, len(good), pp, None) == -1 and b"item 3: NULL" in err()
    arr = _items(E, good)
    arr[1].db = arr[1].db + 2
    assert lib.lsq_group_multi_backward(E.LSQ_F32, arr, len(good), pp, None) == -1 and b"item 1:" in err()
    arr = _items(E, good)
    arr[4].y = None                 # (n == 0: not read)
    arr[2].y = arr[2].y + 1
    assert lib.lsq_group_multi_forward(E.LSQ_BF16, arr, len(good), pp, None) == -1 and b"item 2:" in err()


def test_plan_gives_every_item_its_single_grids_host_only():
    from torchlsq import extension as E
    for dtype, V in ((torch.float32, 4), (torch.bfloat16, 8), (torch.float64, 2), (torch.float16, 8)):
        sizes = [768 * 768, 768 * 3072, 0, 3072 * 768, 64 * 96 * 5, 48 * 72, 4096 * 4096, 96 * 2]
        Gs = [128, 128, 7, 128, 96, 3, 128, 96]
        per, launches = E.group_multi_plan(dtype, sizes, Gs)
        classes = set()
        for (launch, fwd, bwd), m, G in zip(per, sizes, Gs):
            if m == 0:
                assert (launch, fwd, bwd) == (-1, 0, 0)
                continue
            p = E.group_plan(dtype, m, G)
            assert (fwd, bwd) == (p["fwd_grid"], p["bwd_grid"]), (dtype, m, G)
            classes.add((p["form"], p["reduction"], launch))
        # one launch per reduction class here (fewer than 28 items each): the launch index follows the class
        assert launches == len({c[:2] for c in classes}) == len({c[2] for c in classes}), (dtype, classes)
        # more than LSQ_GROUP_MULTI_ITEMS items of one class split
        k = E.GROUP_MULTI_ITEMS
        per, launches = E.group_multi_plan(dtype, [4096] * (2 * k + 1), [128] * (2 * k + 1))
        assert launches == 3 and [p[0] for p in per] == [i // k for i in range(2 * k + 1)]
    with pytest.raises(RuntimeError, match="item 1: element count 100 is not a multiple"):
        E.group_multi_plan(torch.float32, [256, 100], [32, 32])


def test_cpu_tensors_equal_per_tensor_lsq_per_group():
    from torchlsq.functional import lsq_foreach_per_group, lsq_per_group
    torch.manual_seed(0)
    specs = [((8, 256), 128), ((6, 96), 96), ((5, 9), 3), ((4, 64), 32)]
    xs = [torch.randn(sh) * 0.3 for sh, _ in specs]
    ss = [torch.rand(sh[0], sh[1] // G) * 0.05 + 0.01 for sh, G in specs]
    ss[3] = torch.tensor([0.02])                        # one-element parameters are repeated once per group
    bs = [torch.randn(sh[0], sh[1] // G) * 0.02 for sh, G in specs]
    gs = [torch.randn(sh) for sh, _ in specs]
    Gs = [G for _, G in specs]
    for kw in (dict(quant_min=-8, quant_max=7, is_affine=False), dict(quant_min=0, quant_max=15, grad_scaler=0.5),
               dict(quant_min=0, quant_max=15, init_mode=True)):
        got = []
        for fused in (True, False):
            x = [t.clone().requires_grad_() for t in xs]
            s = [t.clone().requires_grad_() for t in ss]
            b = [t.clone().requires_grad_() for t in bs]
            if fused:
                ys = lsq_foreach_per_group(x, s, b, Gs, **kw)
            else:
                ys = [lsq_per_group(*a, **kw) for a in zip(x, s, b, Gs)]
            torch.autograd.backward(ys, gs)
            got.append([t.detach() for t in ys] + [t.grad for t in x + s + b])
        for a, c in zip(*got):
            assert a.shape == c.shape and torch.equal(a, c), kw
    with pytest.raises(AssertionError, match="one int or one per tensor"):
        lsq_foreach_per_group(xs, ss, bs, [128, 96])


def test_weight_group_option_without_a_gpu():
    import torch.nn as nn
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver, MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer, LSQWeightGroup
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(256, 128), nn.ReLU(), nn.Linear(128, 64))
    model.qconfig = QConfig(
        activation=LSQFakeQuantizer.with_args(observer=MovingAverageMinMaxObserver, otype="activation", init_batches=1),
        weight=LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                          qscheme=torch.per_channel_symmetric, quant_min=-8, quant_max=7, group_size=64))
    prepare_qat(model.train(), inplace=True)
    ref = LSQWeightGroup(model)
    assert ref.group_wise is False and ref.last_fused_groups == 0
    ref.remove()
    group = LSQWeightGroup(model, group_wise=True)
    x = torch.randn(4, 256)
    for _ in range(3):
        model(x).sum().backward()
    # CPU weights are never fused: the quantizers' own calls
    assert group.group_wise is True and group.last_fused == 0 and group.last_fused_groups == 0
    group.remove()
