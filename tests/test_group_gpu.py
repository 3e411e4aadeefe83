"""GPU: group-wise LSQ (liblsq_hip_group.so -> torchlsq.functional.lsq_per_group / LSQFakeQuantizer(group_size=...)).

The contract: lsq_per_group(x, s, b, G, ...) == lsq(x.reshape(-1, G), s.reshape(-1), b.reshape(-1), ..., axis=0,
is_perchannel=True).reshape(x.shape) for y, dx, d_scale, d_shift in every mode.
  * fp32 / fp64: y, dx and the integer levels bit-identical to the CPU oracle's per-channel op on [1, N / G, G];
    d_scale / d_shift within 1e-6 * sum|terms| of its fp64 sums;
  * bf16 / fp16: y, dx and levels bit-identical to the per-channel HIP path on the reshape; d_scale / d_shift against the
    oracle run on the fp32 values of the same inputs (the terms are the same fp32 numbers).
"""
import copy
import itertools

import numpy as np
import pytest
import torch
import torchlsq  # noqa: F401  (registers torch.ops.torchlsq.*)

from helpers import assert_bits_equal, assert_reduction_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GROUPS = [1, 2, 3, 4, 7, 8, 32, 64, 128, 256, 4096, "K"]
DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
NP = {torch.float32: np.float32, torch.float64: np.float64}


def _shape(G):
    if G == "K":
        return (5, 1536), 1536
    rows = 37 if G < 32 else (9 if G < 4096 else 3)
    return (rows, G * (12 if G < 4096 else 2)), G


def _inputs(shape, G, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    pd = torch.float64 if dtype == torch.float64 else torch.float32
    x = (torch.randn(shape, generator=g, dtype=torch.float64) * 0.3)
    x.view(-1)[::97] = 0.0
    ng = x.numel() // G
    s = torch.rand(ng, generator=g, dtype=torch.float64) * 0.05 + 0.01
    s[::5] *= -1
    b = torch.randn(ng, generator=g, dtype=torch.float64) * 0.02
    gr = torch.randn(shape, generator=g, dtype=torch.float64)
    pshape = shape[:-1] + (shape[-1] // G,)
    return (x.to(dtype).to(DEV), s.to(pd).reshape(pshape).to(DEV), b.to(pd).reshape(pshape).to(DEV), gr.to(dtype).to(DEV))


def _oracle(x, s, b, gr, G, qmin, qmax, tmin, tmax, ugs, gsc, sym, ev, init):
    from oracle import lsq_oracle as O
    wide = x.dtype in (torch.bfloat16, torch.float16)
    npd = np.float32 if wide else NP[x.dtype]
    xn = x.float().cpu().numpy() if wide else x.cpu().numpy()
    gn = gr.float().cpu().numpy() if wide else gr.cpu().numpy()
    sn, bn = s.cpu().numpy().astype(npd).reshape(-1), b.cpu().numpy().astype(npd).reshape(-1)
    ng = sn.size
    y = O.fwd_pc(xn, sn, bn, 1, ng, G, qmin, qmax, tmin, tmax, init_mode=init)
    r = O.bwd_pc(gn, xn, sn, bn, 1, ng, G, qmin, qmax, tmin, tmax, ugs, gsc, sym, ev, init)
    lv = O.levels_pc(xn, sn, bn, 1, ng, G, qmin, qmax, tmin, tmax)
    return y, r, lv


def _group_ops(x, s, b, gr, G, args):
    y = torch.ops.torchlsq.lsq_forward_per_group(x, s, b, G, *args)
    dx, ds, db = torch.ops.torchlsq.lsq_backward_per_group(gr, x, s, b, G, *args)
    return y, dx, ds, db


def _channel_ops(x, s, b, gr, G, args):
    x2, g2 = x.reshape(-1, G), gr.reshape(-1, G)
    y = torch.ops.torchlsq.lsq_forward_per_channel(x2, s.reshape(-1), b.reshape(-1), 0, *args)
    dx, ds, db = torch.ops.torchlsq.lsq_backward_per_channel(g2, x2, s.reshape(-1), b.reshape(-1), 0, *args)
    return y.reshape(x.shape), dx.reshape(x.shape), ds, db


MODES = list(itertools.product([False, True], [False, True], [False, True], [False, True]))   # sym, eval, init, use_gs


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("G", GROUPS, ids=str)
def test_parity_with_the_per_channel_op_on_the_reshape(dtype, G):
    shape, G = _shape(G)
    x, s, b, gr = _inputs(shape, G, dtype, seed=G * 13 + shape[0])
    for k, (sym, ev, init, ugs) in enumerate(MODES):
        qmin, qmax, tmin, tmax = (-8, 7, -128, 127) if sym else (0, 15, 0, 255)
        gsc = 0.5 if k % 3 else 1.0
        args = (qmin, qmax, tmin, tmax, ugs, gsc, sym, ev, init)
        what = "%s G=%d sym=%d eval=%d init=%d ugs=%d" % (dtype, G, sym, ev, init, ugs)
        y, dx, ds, db = _group_ops(x, s, b, gr, G, args)
        torch.cuda.synchronize()
        assert ds.shape == s.shape and db.shape == b.shape and y.shape == x.shape and dx.shape == x.shape
        oy, r, olv = _oracle(x, s, b, gr, G, *args)
        if dtype in NP:
            assert_bits_equal(y.cpu().numpy(), oy.reshape(shape), what + " y")
            assert_bits_equal(dx.cpu().numpy(), r.dx.reshape(shape), what + " dx")
        else:
            cy, cdx, _, _ = _channel_ops(x, s, b, gr, G, args)
            assert torch.equal(y.view(torch.int16), cy.view(torch.int16)), what + " y"
            assert torch.equal(dx.view(torch.int16), cdx.view(torch.int16)), what + " dx"
        assert_reduction_close(ds.cpu().numpy(), r.ds_wide, r.abs_ds, what + " d_scale")
        assert_reduction_close(db.cpu().numpy(), r.db_wide, r.abs_db, what + " d_shift")
        if k == 0:
            lv = torch.ops.torchlsq.lsq_levels_per_group(x, s, b, G, qmin, qmax, tmin, tmax, 0)
            if dtype in NP:
                assert np.array_equal(lv.cpu().numpy().astype(np.int32).reshape(-1), olv.reshape(-1)), what + " levels"
            else:
                clv = torch.ops.torchlsq.lsq_levels_per_channel(x.reshape(-1, G), s.reshape(-1), b.reshape(-1), 0, qmin, qmax,
                                                                tmin, tmax, 0)
                assert torch.equal(lv.reshape(-1, G), clv), what + " levels"


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_misaligned_views_and_non_contiguous_inputs(dtype):
    from torchlsq.functional import lsq_per_group
    G, rows, K = 32, 45, 256
    x, s, b, gr = _inputs((rows, K), G, dtype, seed=5)
    args = (-8, 7, -128, 127, True, 1.0, True, False, False)
    ref = _group_ops(x, s, b, gr, G, args)
    # element-aligned, not 16-byte aligned: x[1:]-style views of bigger buffers (each with its own offset)
    for off_x, off_g in ((1, 0), (0, 3), (2, 5)):
        bx = torch.empty(rows * K + 8, dtype=dtype, device=DEV)
        bg = torch.empty(rows * K + 8, dtype=dtype, device=DEV)
        xv = bx[off_x:off_x + rows * K].view(rows, K)
        gv = bg[off_g:off_g + rows * K].view(rows, K)
        xv.copy_(x)
        gv.copy_(gr)
        assert xv.data_ptr() % 16 or gv.data_ptr() % 16
        got = _group_ops(xv, s, b, gv, G, args)
        for a, c in zip(got, ref):
            assert torch.equal(a, c)
    # non-contiguous x / grad: made contiguous first
    xt = x.t().contiguous().t()
    gt = gr.t().contiguous().t()
    assert not xt.is_contiguous()
    got = _group_ops(xt, s, b, gt, G, args)
    for a, c in zip(got, ref):
        assert torch.equal(a, c)
    # functional: the same numbers through autograd, parameters of any shape with the right numel
    xs, ss, bs = x.clone().requires_grad_(), s.reshape(-1).clone().requires_grad_(), b.reshape(-1).clone().requires_grad_()
    y = lsq_per_group(xs, ss, bs, G, -8, 7, -128, 127, is_affine=False)
    y.backward(gr)
    assert torch.equal(y, ref[0]) and torch.equal(xs.grad, ref[1])
    assert ss.grad.shape == (rows * K // G,) and torch.equal(ss.grad, ref[2].reshape(-1)) and torch.equal(bs.grad, ref[3].reshape(-1))


def test_ragged_tails_and_group_counts():
    """group counts that fill no whole unit / pass / tile of the kernels, in both forms"""
    for dtype in (torch.float32, torch.bfloat16):
        for G, rows in ((8, 1), (8, 3), (64, 5), (256, 7), (24, 11), (5, 13), (1, 17)):
            K = G * 3
            x, s, b, gr = _inputs((rows, K), G, dtype, seed=G + rows)
            args = (0, 15, 0, 255, True, 1.0, False, False, False)
            y, dx, ds, db = _group_ops(x, s, b, gr, G, args)
            cy, cdx, cds, cdb = _channel_ops(x, s, b, gr, G, args)
            assert torch.equal(y, cy) and torch.equal(dx, cdx), (dtype, G, rows)
            oy, r, _ = _oracle(x, s, b, gr, G, *args)
            assert_reduction_close(ds.cpu().numpy(), r.ds_wide, r.abs_ds, "ragged d_scale")
            assert_reduction_close(db.cpu().numpy(), r.db_wide, r.abs_db, "ragged d_shift")


def test_launches_are_bit_identical():
    for dtype, G in ((torch.float32, 128), (torch.bfloat16, 32), (torch.float32, 24), (torch.float32, 4096), (torch.float16, 3)):
        x, s, b, gr = _inputs((64, G * 16), G, dtype, seed=3)
        args = (0, 15, 0, 255, True, 1.0, False, False, False)
        first = _group_ops(x, s, b, gr, G, args)
        for _ in range(19):
            again = _group_ops(x, s, b, gr, G, args)
            for a, c in zip(again, first):
                assert torch.equal(a, c), (dtype, G)


def test_plan_on_the_device():
    from torchlsq import extension as E
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for dtype, V in ((torch.float32, 4), (torch.bfloat16, 8), (torch.float64, 2), (torch.float16, 8)):
        for G in (V, 32, 128, 256, 3 * V):
            p = E.group_plan(dtype, G * 2 ** 20, G)
            assert p["form"] == "packet" and p["lanes_per_group"] == G // V, (dtype, G, p)
            assert p["fwd_grid"] <= cus * 16 and p["fwd_grid"] % cus == 0, p       # whole rounds of the chip
        p = E.group_plan(dtype, 7 * 2 ** 20, 7)
        assert p["form"] == "element" and p["reduction"] == "scan"


def test_torch_compile_fullgraph_equals_eager():
    from torchlsq.functional import lsq_per_group
    G = 64
    x, s, b, gr = _inputs((32, 512), G, torch.float32, seed=11)
    x.requires_grad_(True)
    s.requires_grad_(True)
    b.requires_grad_(True)

    def f(x, s, b):
        return lsq_per_group(x * 2.0, s, b, G, 0, 15) * 0.5

    def run(fn):
        out = fn(x, s, b)
        return out, torch.autograd.grad(out, (x, s, b), grad_outputs=gr)

    ref, g_ref = run(f)
    cf = torch.compile(f, backend="inductor", fullgraph=True)
    for _ in range(2):
        out, g = run(cf)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        for a, c in zip(g, g_ref):
            assert torch.equal(a, c)


@pytest.mark.parametrize("dtype", [torch.bfloat16])
def test_beyond_2_31_elements(dtype):
    """x of 2^31 + 2^20 elements: the whole tensor equals its two halves bit for bit (the split is on a multiple of every
    unit of the kernels), and both ends agree with the oracle"""
    free, _ = torch.cuda.mem_get_info()
    K, G = 4096, 128
    rows = (2 ** 31 + 2 ** 20) // K
    if free < 40 * 2 ** 30:
        pytest.skip("needs ~40 GB of free device memory")
    n = rows * K
    assert n > 2 ** 31
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = (torch.randn((rows, K), generator=gen, device=DEV, dtype=torch.float32) * 0.3).to(dtype)
    gr = torch.randn((rows, K), generator=gen, device=DEV, dtype=torch.float32).to(dtype)
    ng = n // G
    s = torch.rand((rows, K // G), generator=gen, device=DEV) * 0.05 + 0.01
    b = torch.randn((rows, K // G), generator=gen, device=DEV) * 0.02
    args = (0, 15, 0, 255, True, 1.0, False, False, False)
    y, dx, ds, db = _group_ops(x, s, b, gr, G, args)
    half = rows // 2
    for lo, hi in ((0, half), (half, rows)):
        hy, hdx, hds, hdb = _group_ops(x[lo:hi], s[lo:hi], b[lo:hi], gr[lo:hi], G, args)
        assert torch.equal(hy.view(torch.int16), y[lo:hi].view(torch.int16))
        assert torch.equal(hdx.view(torch.int16), dx[lo:hi].view(torch.int16))
        assert torch.equal(hds, ds[lo:hi]) and torch.equal(hdb, db[lo:hi])
        del hy, hdx, hds, hdb
    for sl in (slice(0, 64), slice(rows - 64, rows)):
        oy, r, _ = _oracle(x[sl], s[sl], b[sl], gr[sl], G, *args)     # (the per-group scaler depends on G only)
        assert torch.equal(y[sl].cpu(), torch.from_numpy(oy).to(dtype))
        assert torch.equal(dx[sl].cpu(), torch.from_numpy(r.dx).to(dtype))
        assert_reduction_close(ds[sl].cpu().numpy(), r.ds_wide, r.abs_ds, "2^31 d_scale")
        assert_reduction_close(db[sl].cpu().numpy(), r.db_wide, r.abs_db, "2^31 d_shift")
    assert ng > 2 ** 24
    del x, gr, y, dx
    torch.cuda.empty_cache()


def _qat_model(group_size, dev, seed=0):
    import torch.nn as nn
    from torch.ao.quantization import QConfig, prepare_qat
    from torch.ao.quantization.observer import MovingAverageMinMaxObserver, MovingAveragePerChannelMinMaxObserver
    from torchlsq.quantized import LSQFakeQuantizer

    torch.manual_seed(seed)
    # weight rows: conv 32 * 2 * 2 = 128, linear 1024 and 256 -- all multiples of the group size
    model = nn.Sequential(nn.Conv2d(32, 16, 2), nn.ReLU(), nn.Flatten(), nn.Linear(16 * 8 * 8, 256), nn.ReLU(),
                          nn.Linear(256, 10))
    model.qconfig = QConfig(
        activation=LSQFakeQuantizer.with_args(observer=MovingAverageMinMaxObserver, otype="activation", init_batches=1),
        weight=LSQFakeQuantizer.with_args(observer=MovingAveragePerChannelMinMaxObserver, otype="weight", dtype=torch.qint8,
                                          qscheme=torch.per_channel_symmetric, quant_min=-8, quant_max=7,
                                          group_size=group_size))
    model = model.to(dev).train()
    prepare_qat(model, inplace=True)
    return model


def test_qat_linear_and_conv_with_group_size_128():
    from torchlsq.quantized import LSQWeightGroup
    dev = DEV
    model = _qat_model(128, dev)
    twin = copy.deepcopy(model)
    group = LSQWeightGroup(twin)
    qs = [(m, m.weight_fake_quant) for m in model.modules() if hasattr(m, "weight_fake_quant")]
    assert len(qs) == 3 and all(q.group_size == 128 for _, q in qs)
    x = torch.randn(8, 32, 9, 9, device=dev)
    target = torch.randint(0, 10, (8,), device=dev)
    model(x)
    twin(x)
    for m, q in qs:
        row = m.weight.numel() // m.weight.shape[0]
        assert q.scale.shape == (m.weight.shape[0], row // 128) and q.scale.is_cuda
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
        assert torch.equal(outs[0], outs[1]), step       # LSQWeightGroup leaves grouped quantizers to their own calls
    assert group.last_fused == 0
    for (m, q), (m2, q2) in zip(qs, [(m, m.weight_fake_quant) for m in twin.modules() if hasattr(m, "weight_fake_quant")]):
        # (the last step's weight gradients come from the convolution / GEMM backward, which need not be bit-reproducible;
        # every output above was, so the quantizers did the same with and without the group)
        assert q.scale.grad is not None and torch.allclose(q.scale.grad, q2.scale.grad, rtol=1e-4, atol=1e-9)
        assert torch.allclose(q.scale, q2.scale, rtol=1e-6, atol=0)
        y = q(m.weight)
        levels, sc, zp = q.quantize(m.weight)
        out_c = m.weight.shape[0]
        deq = (levels.reshape(out_c, -1, 128).float() - zp.unsqueeze(-1).float()) * sc.unsqueeze(-1)
        assert torch.equal(deq.reshape(m.weight.shape), y.detach())
        scale, zero_point = q.calculate_qparams()
        assert scale.shape == q.scale.shape and zero_point.shape == q.scale.shape
    sd = model.state_dict()
    fresh = _qat_model(128, dev, seed=1)
    fresh(x)
    fresh.load_state_dict(sd)
    fresh.train()
    for (m, q), (m2, q2) in zip(qs, [(m, m.weight_fake_quant) for m in fresh.modules() if hasattr(m, "weight_fake_quant")]):
        assert torch.equal(q.scale, q2.scale) and torch.equal(q(m.weight), q2(m2.weight))
    group.remove()
