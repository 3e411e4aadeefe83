"""GPU: the fused group-wise calls (lsq_group_multi_* -> torchlsq.functional.lsq_foreach_per_group,
LSQWeightGroup(group_wise=True)).

The contract: lsq_foreach_per_group(xs, ss, bs, Gs, ...) == [lsq_per_group(x, s, b, G, ...) for ...] bit for bit -- y, dx,
d_scale and d_shift in every mode -- because every tensor is walked by the workgroups of its own single call.
"""
import copy

import pytest
import torch
import torchlsq  # noqa: F401  (registers torch.ops.torchlsq.*)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64]
MODES = {"affine": dict(quant_min=0, quant_max=15, type_min=0, type_max=255),
         "sym": dict(quant_min=-8, quant_max=7, type_min=-128, type_max=127, is_affine=False),
         "eval": dict(quant_min=0, quant_max=15, eval_mode=True, grad_scaler=0.5),
         "init": dict(quant_min=-8, quant_max=7, is_affine=False, init_mode=True, use_grad_scaling=False)}


def _specs(dtype):
    """(shape, G) pairs reaching every class: P2 with <= 64 and > 64 packets per group, a scan over packets, the element
    form -- mixed sizes, and one item big enough for a persistent grid"""
    V = {torch.float32: 4, torch.float64: 2}.get(dtype, 8)
    big = (1024 * V, 4096)            # 2^22 packets: more tiles than one round of the chip
    return [((64, 768), 128), ((48, 1024), 64 * V * 2), ((32, 512), 512), ((40, 384), 96), ((96, 18), 3), ((50, 36), 6),
            (big, 128), ((3, 1536), 1536), ((768, 768), 128)]


def _inputs(specs, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    pd = torch.float64 if dtype == torch.float64 else torch.float32
    out = []
    for shape, G in specs:
        x = torch.randn(shape, generator=g, dtype=torch.float64) * 0.3
        x.view(-1)[::97] = 0.0
        pshape = shape[:-1] + (shape[-1] // G,)
        s = torch.rand(pshape, generator=g, dtype=torch.float64) * 0.05 + 0.01
        s.view(-1)[::5] *= -1
        b = torch.randn(pshape, generator=g, dtype=torch.float64) * 0.02
        gr = torch.randn(shape, generator=g, dtype=torch.float64)
        out.append((x.to(dtype).to(DEV), s.to(pd).to(DEV), b.to(pd).to(DEV), gr.to(dtype).to(DEV)))
    return out


def _run(inputs, Gs, fused, kw, live=None):
    """outputs and gradients of the fused call or of one lsq_per_group per tensor; `live`: the outputs that get a gradient"""
    from torchlsq.functional import lsq_foreach_per_group, lsq_per_group
    xs = [t[0].clone().requires_grad_(True) for t in inputs]
    ss = [t[1].clone().requires_grad_(True) for t in inputs]
    bs = [t[2].clone().requires_grad_(True) for t in inputs]
    if fused:
        ys = lsq_foreach_per_group(xs, ss, bs, Gs, **kw)
    else:
        ys = [lsq_per_group(x, s, b, G, **kw) for x, s, b, G in zip(xs, ss, bs, Gs)]
    live = range(len(ys)) if live is None else live
    torch.autograd.backward([ys[i] for i in live], [inputs[i][3] for i in live])
    torch.cuda.synchronize()
    return [y.detach() for y in ys], [x.grad for x in xs], [s.grad for s in ss], [b.grad for b in bs]


def _assert_same(a, b, what):
    for name, la, lb in zip(("y", "dx", "d_scale", "d_shift"), a, b):
        for i, (u, v) in enumerate(zip(la, lb)):
            if u is None or v is None:
                assert u is None and v is None, (what, name, i)
                continue
            assert u.shape == v.shape and u.dtype == v.dtype, (what, name, i)
            assert torch.equal(u, v), "%s: %s of tensor %d differs" % (what, name, i)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("mode", list(MODES))
def test_fused_equals_single_calls(dtype, mode):
    specs = _specs(dtype)
    inputs = _inputs(specs, dtype, seed=len(mode) + 7)
    Gs = [G for _, G in specs]
    E = torchlsq.extension
    per, launches = E.group_multi_plan(dtype, [t[0].numel() for t in inputs], Gs)
    assert launches == 3 and len({p[0] for p in per}) == 3          # P2, scan over packets, element form
    assert max(p[1] for p in per) == torch.cuda.get_device_properties(0).multi_processor_count * 16   # a persistent grid
    kw = MODES[mode]
    _assert_same(_run(inputs, Gs, True, kw), _run(inputs, Gs, False, kw), "%s %s" % (dtype, mode))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_views_non_contiguous_inputs_and_one_element_parameters(dtype):
    specs = [((45, 256), 32), ((12, 96), 96), ((20, 30), 6), ((16, 512), 128)]
    inputs = _inputs(specs, dtype, seed=5)
    Gs = [G for _, G in specs]
    views = []
    for k, (x, s, b, g) in enumerate(inputs):
        if k == 0:      # an element-aligned x[1:] view, not 16-byte aligned
            buf = torch.empty(x.numel() + 8, dtype=dtype, device=DEV)
            xv = buf[1:1 + x.numel()].view(x.shape)
            xv.copy_(x)
            assert xv.data_ptr() % 16
            x = xv
        elif k == 1:    # non-contiguous
            x = x.t().contiguous().t()
            assert not x.is_contiguous()
        elif k == 2:    # one-element parameters: repeated once per group
            s, b = s.reshape(-1)[:1].clone(), b.reshape(-1)[:1].clone()
        views.append((x, s, b, g))
    kw = MODES["sym"]
    got, want = _run(views, Gs, True, kw), _run(views, Gs, False, kw)
    _assert_same(got, want, str(dtype))
    assert got[2][2].shape == (1,)


def test_more_items_than_one_launch_takes_and_mixed_g():
    E = torchlsq.extension
    k = E.GROUP_MULTI_ITEMS
    specs = [((16 + 8 * (i % 5), 256 * (1 + i % 3)), (128, 64, 256)[i % 3]) for i in range(2 * k + 5)]
    inputs = _inputs(specs, torch.float32, seed=11)
    Gs = [G for _, G in specs]
    per, launches = E.group_multi_plan(torch.float32, [t[0].numel() for t in inputs], Gs)
    assert launches == 3
    _assert_same(_run(inputs, Gs, True, MODES["affine"]), _run(inputs, Gs, False, MODES["affine"]), "split")


def test_two_launches_are_bit_identical_and_plan_matches_single_plans():
    E = torchlsq.extension
    for dtype in (torch.float32, torch.bfloat16):
        specs = _specs(dtype)
        inputs = _inputs(specs, dtype, seed=3)
        Gs = [G for _, G in specs]
        first = _run(inputs, Gs, True, MODES["affine"])
        _assert_same(_run(inputs, Gs, True, MODES["affine"]), first, "again")
        per, _ = E.group_multi_plan(dtype, [t[0].numel() for t in inputs], Gs)
        for (launch, fwd, bwd), t, G in zip(per, inputs, Gs):
            p = E.group_plan(dtype, t[0].numel(), G)
            assert (fwd, bwd) == (p["fwd_grid"], p["bwd_grid"])


def test_unused_outputs_get_no_gradients():
    specs = [((32, 256), 128), ((16, 384), 96), ((24, 12), 3), ((8, 512), 256)]
    inputs = _inputs(specs, torch.float32, seed=9)
    Gs = [G for _, G in specs]
    for kw in (MODES["affine"], MODES["init"]):
        got = _run(inputs, Gs, True, kw, live=[1, 3])
        want = _run(inputs, Gs, False, kw, live=[1, 3])
        _assert_same(got, want, "live subset")
        assert got[1][0] is None and got[2][0] is None and got[3][2] is None and got[1][1] is not None


def test_steady_state_never_synchronises():
    from torchlsq.functional import lsq_foreach_per_group
    specs = [((64, 768), 128), ((48, 384), 96), ((40, 18), 3)]
    inputs = _inputs(specs, torch.bfloat16, seed=2)
    Gs = [G for _, G in specs]
    xs = [t[0].clone().requires_grad_(True) for t in inputs]
    ss = [t[1].clone().requires_grad_(True) for t in inputs]
    bs = [t[2].clone().requires_grad_(True) for t in inputs]
    lsq_foreach_per_group(xs, ss, bs, Gs, -8, 7)         # warm-up (first launches, caches)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            ys = lsq_foreach_per_group(xs, ss, bs, Gs, -8, 7, -128, 127)
            torch.autograd.backward(ys, [t[3] for t in inputs])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_one_item_beyond_2_31_elements_with_small_ones():
    free, _ = torch.cuda.mem_get_info()
    if free < 64 * 2 ** 30:
        pytest.skip("needs ~64 GB of free device memory")
    from torchlsq.functional import lsq_foreach_per_group, lsq_per_group
    dtype, K, G = torch.bfloat16, 4096, 128
    rows = (2 ** 31 + 2 ** 20) // K
    gen = torch.Generator(device=DEV).manual_seed(7)
    big = (torch.randn((rows, K), generator=gen, device=DEV, dtype=torch.float32) * 0.3).to(dtype)
    gbig = torch.randn((rows, K), generator=gen, device=DEV, dtype=torch.float32).to(dtype)
    assert big.numel() > 2 ** 31
    sb = torch.rand((rows, K // G), generator=gen, device=DEV) * 0.05 + 0.01
    bb = torch.randn((rows, K // G), generator=gen, device=DEV) * 0.02
    small = _inputs([((64, 768), 128), ((48, 96), 96)], dtype, seed=4)
    xs = [big] + [t[0] for t in small]
    ss = [sb.requires_grad_(True)] + [t[1].requires_grad_(True) for t in small]
    bs = [bb.requires_grad_(True)] + [t[2].requires_grad_(True) for t in small]
    grads = [gbig] + [t[3] for t in small]
    Gs = [G, 128, 96]
    ys = lsq_foreach_per_group(xs, ss, bs, Gs, 0, 15)
    fused = [y.detach() for y in ys]
    torch.autograd.backward(ys, grads)
    fds = [s.grad.clone() for s in ss]
    fdb = [b.grad.clone() for b in bs]
    del ys
    for s, b in zip(ss, bs):
        s.grad = b.grad = None
    for i in range(3):
        y = lsq_per_group(xs[i], ss[i], bs[i], Gs[i], 0, 15)
        assert torch.equal(y.detach().view(torch.int16), fused[i].view(torch.int16)), i
        y.backward(grads[i])
        del y
        assert torch.equal(ss[i].grad, fds[i]) and torch.equal(bs[i].grad, fdb[i]), i
    del fused, xs, big, gbig
    torch.cuda.empty_cache()


def test_qat_model_with_group_wise_fusion():
    import torch.nn as nn
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver, MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer, LSQWeightGroup

    torch.manual_seed(0)
    # weight rows: conv 32 * 2 * 2 = 128, linear 1024 and 256 -- all multiples of the group size
    model = nn.Sequential(nn.Conv2d(32, 16, 2), nn.ReLU(), nn.Flatten(), nn.Linear(16 * 8 * 8, 256), nn.ReLU(),
                          nn.Linear(256, 10))
    model.qconfig = QConfig(
        activation=LSQFakeQuantizer.with_args(observer=MovingAverageMinMaxObserver, otype="activation", init_batches=1),
        weight=LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                          qscheme=torch.per_channel_symmetric, quant_min=-8, quant_max=7, group_size=128))
    model = model.to(DEV).train()
    prepare_qat(model, inplace=True)
    twin = copy.deepcopy(model)
    group = LSQWeightGroup(twin, group_wise=True)
    x = torch.randn(8, 32, 9, 9, device=DEV)
    target = torch.randint(0, 10, (8,), device=DEV)
    model(x)
    twin(x)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    opt2 = torch.optim.SGD(twin.parameters(), lr=0.01)
    for step in range(4):
        outs = []
        for net, o in ((model, opt), (twin, opt2)):
            o.zero_grad()
            out = net(x)
            loss = torch.nn.functional.cross_entropy(out, target)
            loss.backward()
            o.step()
            outs.append(out.detach())
        assert torch.isfinite(outs[0]).all()
        assert torch.equal(outs[0], outs[1]), step
        if step > 0:
            assert group.last_fused_groups == 3 and group.last_fused == 0, step
    qs = [m.weight_fake_quant for m in model.modules() if hasattr(m, "weight_fake_quant")]
    qs2 = [m.weight_fake_quant for m in twin.modules() if hasattr(m, "weight_fake_quant")]
    for q, q2 in zip(qs, qs2):
        assert q.scale.grad is not None and torch.allclose(q.scale.grad, q2.scale.grad, rtol=1e-4, atol=1e-9)
        assert torch.allclose(q.scale, q2.scale, rtol=1e-6, atol=0)
    group.remove()
