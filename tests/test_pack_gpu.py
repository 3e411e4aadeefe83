"""GPU: the packed export of group-wise weights (liblsq_hip_pack.so -> torchlsq.functional.lsq_pack_per_group /
LSQFakeQuantizer.export_packed).  Every comparison is bit-exact.

  * fp32 / fp64: the codes are the numpy packing of the CPU oracle's levels (the per-channel op on [1, N / G, G]);
  * bf16 / fp16: the codes are the torch packing of the existing lsq_levels_per_group output;
  * lsq_dequantize_per_group carries the bits of lsq_forward_per_group (compared as integer views), the unpacked bytes are
    lsq_levels_per_group's, and the GPU codes are the CPU path's codes.

Inputs as in tests/test_pack_cpu.py (its docstring has the reason): codes cannot carry the sign of a zero, so the bit-exact
comparisons run where dequantize is bit-identical by the format's own rule (quant_min >= 0, or no zero point of +0.0):
affine ranges with random shifts, symmetric ranges with shift +0.0 and with shifts whose zero point is a non-zero integer.
"""
import numpy as np
import pytest
import torch
import torchlsq  # noqa: F401  (registers torch.ops.torchlsq.*)

from test_group_gpu import _qat_model, _shape

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
NP = {torch.float32: np.float32, torch.float64: np.float64}
INT = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16, torch.float16: torch.int16}
RANGES = {(4, "sym"): (-8, 7, -128, 127), (2, "sym"): (-2, 1, -128, 127), (4, "affine"): (0, 15, 0, 255), (2, "affine"): (0, 3, 0, 255)}
RANGES.update({(4, "sym_shift"): RANGES[(4, "sym")], (2, "sym_shift"): RANGES[(2, "sym")]})
SCHEMES = ("sym", "sym_shift", "affine")
GROUPS = ["byte", 8, 24, 32, 96, 128, 256, 4096, "K"]


def _inputs(shape, G, dtype, seed, scheme, edge=True):
    g = torch.Generator(device="cpu").manual_seed(seed)
    pd = torch.float64 if dtype == torch.float64 else torch.float32
    x = torch.randn(shape, generator=g, dtype=torch.float64) * 0.3
    x.view(-1)[::97] = 0.0
    if edge:
        x.view(-1)[5], x.view(-1)[11], x.view(-1)[shape[-1] + 3], x.view(-1)[7] = float("nan"), float("inf"), float("-inf"), -0.0
    ng = x.numel() // G
    s = torch.rand(ng, generator=g, dtype=torch.float64) * 0.05 + 0.01
    s[::5] *= -1
    if scheme == "sym":
        b = torch.zeros(ng, dtype=torch.float64)
    elif scheme == "sym_shift":                             # a zero point of 1 .. 5 with quant_min < 0
        b = -torch.randint(1, 6, (ng,), generator=g).to(torch.float64) * s.abs()
    else:
        b = -(torch.rand(ng, generator=g, dtype=torch.float64) * 6 + 1) * s.abs()
    pshape = shape[:-1] + (shape[-1] // G,)
    return x.to(dtype).to(DEV), s.to(pd).reshape(pshape).to(DEV), b.to(pd).reshape(pshape).to(DEV)


def torch_pack(codes, bits):
    """the format of include/lsq_hip_pack.h in torch integer ops: [..., K] codes -> [..., K * bits / 8] bytes"""
    per = 8 // bits
    c = codes.reshape(codes.shape[:-1] + (codes.shape[-1] // per, per)).to(torch.int32)
    out = torch.zeros_like(c[..., 0])
    for j in range(per):
        out |= c[..., j] << (j * bits)
    return out.to(torch.uint8)


def np_pack(codes, bits):
    per = 8 // bits
    c = np.asarray(codes, dtype=np.uint8).reshape(-1, per)
    out = np.zeros(c.shape[0], dtype=np.uint8)
    for j in range(per):
        out |= (c[:, j] << (j * bits)).astype(np.uint8)
    return out


def _check_all(x, s, b, G, bits, rng, what, oracle=True):
    """pack x and hold codes, constants, dequantize, unpack and the CPU path to their references"""
    from torchlsq.functional import lsq_pack_per_group
    qmin, qmax, tmin, tmax = rng
    dtype = x.dtype
    p = lsq_pack_per_group(x, s, b, G, bits, qmin, qmax, tmin, tmax)
    torch.cuda.synchronize()
    assert p.codes.shape == x.shape[:-1] + (x.shape[-1] * bits // 8,) and p.codes.dtype == torch.uint8 and p.codes.is_cuda, what
    assert p.scale.shape == s.shape and p.zero_point.shape == s.shape and p.zero_point.dtype == torch.int32, what
    lv = torch.ops.torchlsq.lsq_levels_per_group(x, s, b, G, qmin, qmax, tmin, tmax, 0)
    if dtype in NP and oracle:
        from oracle import lsq_oracle as O
        ng = s.numel()
        olv = O.levels_pc(x.cpu().numpy(), s.cpu().numpy().reshape(-1), b.cpu().numpy().reshape(-1), 1, ng, G, qmin, qmax, tmin,
                          tmax).reshape(-1).astype(np.int64)
        assert np.array_equal(p.codes.cpu().numpy().reshape(-1), np_pack(olv - qmin, bits)), what + " codes vs the oracle"
    assert torch.equal(p.codes, torch_pack(lv.to(torch.int32) - qmin, bits)), what + " codes vs lsq_levels_per_group"
    y = torch.ops.torchlsq.lsq_forward_per_group(x, s, b, G, qmin, qmax, tmin, tmax, True, 1.0, False, False, False)
    d = torch.ops.torchlsq.lsq_dequantize_per_group(p.codes, p.scale, p.zero_point, G, bits, dtype)
    assert d.shape == x.shape and d.dtype == dtype
    assert torch.equal(d.view(INT[dtype]), y.view(INT[dtype])), what + " dequantize vs the forward"
    assert torch.equal(torch.ops.torchlsq.lsq_unpack_per_group(p.codes, bits, qmin, 0), lv), what + " unpack vs levels"
    sq = s.abs().clamp_min(torch.finfo(s.dtype).eps)
    zp = torch.fmin(torch.full_like(sq, tmax), torch.fmax(torch.full_like(sq, tmin), -b * (1.0 / sq))).round()
    assert torch.equal(p.scale, sq) and torch.equal(p.zero_point.to(torch.int64), zp.to(torch.int64) - qmin), what + " constants"
    if dtype != torch.float16:                              # (the CPU kernels have no fp16)
        c = lsq_pack_per_group(x.cpu(), s.cpu(), b.cpu(), G, bits, qmin, qmax, tmin, tmax)
        assert torch.equal(c.codes, p.codes.cpu()) and torch.equal(c.scale, p.scale.cpu()), what + " CPU path"
        assert torch.equal(c.zero_point, p.zero_point.cpu()), what + " CPU path"
    return p, y


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("bits", [4, 2])
@pytest.mark.parametrize("G", GROUPS, ids=str)
def test_codes_dequantize_and_unpack(dtype, bits, G):
    shape, G = _shape(8 // bits if G == "byte" else G)
    for scheme in SCHEMES:
        x, s, b = _inputs(shape, G, dtype, seed=G * 13 + bits, scheme=scheme)
        _check_all(x, s, b, G, bits, RANGES[(bits, scheme)], "%s %d-bit G=%d %s" % (dtype, bits, G, scheme))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("bits", [4, 2])
def test_misaligned_views_non_contiguous_inputs_and_offset_codes(dtype, bits):
    from torchlsq.functional import lsq_dequantize_per_group, lsq_pack_per_group, lsq_unpack_per_group
    G, rows, K = 32, 45, 256
    rng = RANGES[(bits, "sym")]
    x, s, b = _inputs((rows, K), G, dtype, seed=5, scheme="sym")
    ref, y = _check_all(x, s, b, G, bits, rng, "reference")
    for off in (1, 3, 5, 7):                                # element-aligned, not 16-byte aligned
        buf = torch.empty(rows * K + 8, dtype=dtype, device=DEV)
        xv = buf[off:off + rows * K].view(rows, K)
        xv.copy_(x)
        assert xv.data_ptr() % 16
        assert torch.equal(lsq_pack_per_group(xv, s, b, G, bits, *rng).codes, ref.codes), off
    xt = x.t().contiguous().t()
    assert not xt.is_contiguous() and torch.equal(lsq_pack_per_group(xt, s, b, G, bits, *rng).codes, ref.codes)
    nbytes = ref.codes.numel()
    for off in (1, 2, 3, 4, 7, 8):                          # codes at any byte offset: the slower forms
        buf = torch.zeros(nbytes + 16, dtype=torch.uint8, device=DEV)
        cv = buf[off:off + nbytes].view(ref.codes.shape)
        cv.copy_(ref.codes)
        d = lsq_dequantize_per_group(cv, ref.scale, ref.zero_point, G, bits, dtype)
        assert torch.equal(d.view(INT[dtype]), y.view(INT[dtype])), off
        assert torch.equal(lsq_unpack_per_group(cv, bits, rng[0]), ref.levels()), off
    nc = ref.codes.t().contiguous().t()                     # non-contiguous codes are made contiguous
    assert torch.equal(lsq_dequantize_per_group(nc, ref.scale, ref.zero_point, G, bits, dtype).view(INT[dtype]), y.view(INT[dtype]))
    # a packed weight survives the trip through the host
    moved = type(ref).from_state({k: (v.cpu().to(DEV) if torch.is_tensor(v) else v) for k, v in ref.state().items()})
    assert torch.equal(moved.dequantize(dtype).view(INT[dtype]), y.view(INT[dtype]))


def test_ragged_tails_and_empty():
    """sizes whose last tile holds 1 .. V - 1 packets more than whole tiles, whose unpack tail is not a multiple of 16
    elements, and n == 0"""
    from torchlsq.functional import lsq_pack_per_group
    for dtype in (torch.float32, torch.bfloat16, torch.float64):
        for bits in (4, 2):
            small = ((2, 1), (6, 1), (6, 3)) if bits == 4 else ()          # n % 4 == 2: no whole fp32 packet at the end
            for G, rows in ((8, 1), (8, 3), (64, 5), (256, 7), (24, 11), (40, 13), (4, 17), (4, 1)) + small:
                for scheme in SCHEMES:
                    x, s, b = _inputs((rows, G * 3), G, dtype, seed=G + rows, scheme=scheme, edge=False)
                    _check_all(x, s, b, G, bits, RANGES[(bits, scheme)], "ragged %s %d-bit G=%d rows=%d" % (dtype, bits, G, rows))
            # whole tiles (256 lanes x 4 packets) plus 1 .. 3 packets
            V = {torch.float32: 4, torch.bfloat16: 8, torch.float64: 2}[dtype]
            lane = max(V, 8 // bits)
            for extra in (1, 2, 3):
                n = (1024 + extra) * lane
                x, s, b = _inputs((1, n), lane, dtype, seed=extra, scheme="affine", edge=False)
                _check_all(x, s, b, lane, bits, RANGES[(bits, "affine")], "tile + %d" % extra, oracle=False)
    e = lsq_pack_per_group(torch.empty(0, 64, device=DEV), torch.empty(0, 2, device=DEV), torch.empty(0, 2, device=DEV), 32, 4, -8, 7)
    assert e.codes.shape == (0, 32) and e.dequantize().shape == (0, 64) and e.levels().shape == (0, 64) and e.codes.is_cuda


def test_plan_on_the_device():
    from torchlsq import extension as E
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for dtype in DTYPES:
        for bits in (4, 2):
            p = E.pack_plan(dtype, 128 * 2 ** 20, 128, bits)
            assert p["quantize_form"] == "packet" and p["dequantize_form"] == "packet"
            for k in ("quantize_grid", "dequantize_grid", "unpack_grid"):
                assert p[k] == cus * 16, (k, p)             # whole rounds of the chip


def test_torch_compile_fullgraph_equals_eager():
    G, bits = 64, 4
    x, s, b = _inputs((32, 512), G, torch.float32, seed=11, scheme="sym", edge=False)

    def f(x, s, b):
        codes, qs, qz = torch.ops.torchlsq.lsq_pack_per_group(x * 2.0, s, b, G, bits, -8, 7, -128, 127)
        return torch.ops.torchlsq.lsq_dequantize_per_group(codes, qs, qz, G, bits, torch.float32) * 0.5, codes

    ref, ref_codes = f(x, s, b)
    cf = torch.compile(f, backend="inductor", fullgraph=True)
    for _ in range(2):
        out, codes = cf(x, s, b)
        torch.cuda.synchronize()
        assert torch.equal(out, ref) and torch.equal(codes, ref_codes)


@pytest.mark.slow
def test_beyond_2_31_elements():
    """bf16 x of 2^31 + 2^20 elements, on the GPU against the torch packing of the existing levels op (in slabs) and the
    existing forward"""
    from torchlsq.functional import lsq_pack_per_group
    free, _ = torch.cuda.mem_get_info()
    if free < 40 * 2 ** 30:
        pytest.skip("needs ~40 GB of free device memory")
    K, G, bits = 4096, 128, 4
    rows = (2 ** 31 + 2 ** 20) // K
    assert rows * K > 2 ** 31
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = (torch.randn((rows, K), generator=gen, device=DEV, dtype=torch.float32) * 0.3).to(torch.bfloat16)
    s = torch.rand((rows, K // G), generator=gen, device=DEV) * 0.05 + 0.01
    b = torch.zeros((rows, K // G), device=DEV)
    p = lsq_pack_per_group(x, s, b, G, bits, -8, 7, -128, 127)
    lv = torch.ops.torchlsq.lsq_levels_per_group(x, s, b, G, -8, 7, -128, 127, 0)
    step = 2 ** 14
    for lo in range(0, rows, step):
        assert torch.equal(p.codes[lo:lo + step], torch_pack(lv[lo:lo + step].to(torch.int32) + 8, bits)), lo
    assert torch.equal(p.levels(), lv)
    del lv
    y = torch.ops.torchlsq.lsq_forward_per_group(x, s, b, G, -8, 7, -128, 127, True, 1.0, True, False, False)
    del x
    d = p.dequantize(torch.bfloat16)
    assert torch.equal(d.view(torch.int16), y.view(torch.int16))
    del d, y, p
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_qat_linear_w4_g128_export_equals_the_module(dtype):
    from torchlsq.quantized import LSQWeightGroup
    model = _qat_model(128, DEV)
    x = torch.randn(8, 32, 9, 9, device=DEV)
    target = torch.randint(0, 10, (8,), device=DEV)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    for _ in range(4):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(x), target).backward()
        opt.step()
    group = LSQWeightGroup(model, register_hook=False)
    layers = {n: m for n, m in model.named_modules() if hasattr(m, "weight_fake_quant")}
    assert len(layers) == 3
    if dtype == torch.float32:
        out = group.export_packed()
        assert sorted(out) == sorted(layers)
    for name, m in layers.items():
        q = m.weight_fake_quant
        w = m.weight.detach().to(dtype)
        p = q.export_packed(w)
        assert p.bits == 4 and p.group_size == 128 and tuple(p.shape) == tuple(w.shape) and p.codes.is_cuda
        assert p.codes.numel() * 2 == w.numel()
        y = q(w).detach()
        assert y.dtype == dtype
        assert torch.equal(p.dequantize(dtype).view(INT[dtype]), y.view(INT[dtype])), name
        if dtype == torch.float32:
            assert torch.equal(out[name].codes, p.codes) and torch.equal(out[name].scale, p.scale)
        levels, sc, zp = q.quantize(w)
        assert torch.equal(p.levels(torch.qint8), levels) and torch.equal(p.scale, sc)
