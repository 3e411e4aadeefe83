"""Rotary embedding and the KV-cache append on 8-bit levels on the GPU (liblsq_hip_rope_w8.so): bit for bit against the CPU path -- the
definition, which tests/test_rope_w8_cpu.py holds to a numpy restatement and to the existing ops composed --: every packets
instantiation with the plan asserted, the generic family, the placement with positions on the device, both sides of the
heads-per-lane threshold, repeats, batch independence, a decode step captured in a graph, and smoke().
"""
import pytest
import torch

import rope_w8_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8, I8, F32, BF16, F16 = C.U8, C.I8, C.F32, C.BF16, C.F16
SIDES = ((C.OUT_U8, BF16), (C.OUT_I8, F16), (None, F32), (None, BF16))


def _plan_of(x, view, R, P, mid, q, interleaved=False, scatter=False, copy=False, aligned=True):
    from torchlsq import extension as E
    from torchlsq._rope_w8_host import _strides3
    B, T, H, D = x.shape
    elem = 1 if (q is not None or copy) else torch.empty((), dtype=mid).element_size()
    return E.rope_w8_plan(B, T, H, D, R, P, view.shape[1], _strides3(x), _strides3(view), aligned, elem, x.dtype, interleaved, scatter, copy)


def _check(x, R, kernel, note, positions=None, interleaved=False, scatter=False, Tmax=None, sides=SIDES, P=16, hpl=None):
    """GPU against the CPU path on every side, x read in place, out the [B, Tmax, H, D] view of a guarded cache; the plan for exactly
    these strides must name `kernel`"""
    B, T, H, D = x.shape
    Tmax = T if Tmax is None else Tmax
    consts = C.constants(x.dtype)
    xin = _regrid(x)               # the same offset and strides on the GPU
    for q, mid in sides:
        cos, sin = C.tables(R, P, mid)
        ydt = (U8 if max(q[3], q[5]) > 127 else I8) if q is not None else mid
        cbuf, cview = C.cache_view(B, H, Tmax, D, ydt)
        want = C.run_rope("cpu", x, consts, cos, sin, q, mid, positions, interleaved, out=cview, scatter=scatter)
        gbuf, gview = C.cache_view(B, H, Tmax, D, ydt, DEV)
        aligned = xin.data_ptr() % 16 == 0 and gview.data_ptr() % 16 == 0
        pl = _plan_of(xin, gview, R, P, mid, q, interleaved, scatter, aligned=aligned)
        assert pl["kernel"] == kernel and (hpl is None or pl["heads_per_lane"] == hpl), (note, pl)
        got = C.run_rope(DEV, xin, consts, cos, sin, q, mid, positions, interleaved, out=gview, scatter=scatter)
        torch.cuda.synchronize()
        C.same(got, want, (note, q is None, mid))
        C.same(gbuf, cbuf, (note, "guard bytes", q is None, mid))          # the whole buffer: nothing outside the logical y changed


def _regrid(x):
    """the same strided view on the GPU: the storage is moved whole"""
    base = torch.empty(0, dtype=x.dtype).set_(x.untyped_storage()).to(DEV)
    return base.as_strided(x.shape, x.stride(), x.storage_offset())


# ---------------------------------------------------------------------------------------------------
# 1: every packets instantiation
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [U8, I8], ids=str)
@pytest.mark.parametrize("H", [1, 3, 8])
@pytest.mark.parametrize("D,R,interleaved,kernel", [(32, 32, False, "packets_half"), (128, 128, False, "packets_half"), (64, 32, False, "packets_half"),
                                                    (16, 16, True, "packets_interleaved"), (64, 64, True, "packets_interleaved"),
                                                    (64, 16, True, "packets_interleaved")], ids=str)
def test_packets_kernels(D, R, interleaved, kernel, H, dtype):
    for i, v in enumerate(C.qkv_views(2, 5, H, D, D + H, dtype)):       # the q and the k view of one buffer, read in place
        assert not v.is_contiguous() or H * D == 0
        _check(v, R, kernel, (D, R, H, "qk"[i]), positions=[3, 0], interleaved=interleaved, Tmax=7)


# ---------------------------------------------------------------------------------------------------
# 2: the generic family
# ---------------------------------------------------------------------------------------------------
def test_generic_kernel():
    for interleaved in (False, True):
        _check(C.levels((2, 5, 3, 6), 1), 4, "generic", "D 6 R 4", positions=[1, 2], interleaved=interleaved)
        _check(C.levels((2, 5, 3, 32), 2, I8), 8, "generic", "D 32 R 8", positions=[1, 2], interleaved=interleaved)
    # a base one byte off
    buf = C.levels((2 * 5 * 3 * 32 + 16,), 3)
    _check(buf[1:1 + 960].view(2, 5, 3, 32), 32, "generic", "base + 1")
    # a head stride of 24: D = 16 rows 24 bytes apart
    buf = C.levels((2, 5, 3, 24), 4)
    _check(buf[..., :16], 16, "generic", "stride 24", interleaved=True)
    _check(buf[..., :16], 16, "generic", "stride 24 half")


# ---------------------------------------------------------------------------------------------------
# 3: placement on the device
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("positions,scatter", [([0, 9], True), ([0, 9], False), ([-3, 2], True), ([-3, 13], False), ([14, 7], True), (None, True)], ids=str)
def test_placement(positions, scatter):
    """Tmax = 12, T = 5, the tables hold 16 positions: with [0, 9] the second batch's last two tokens fall outside the cache; negative
    positions and positions beyond the tables are skipped as well"""
    x = C.qkv_views(2, 5, 3, 32, 21)[1]
    _check(x, 32, "packets_half", "packets", positions=positions, scatter=scatter, Tmax=12)
    _check(C.levels((2, 5, 3, 6), 22), 4, "generic", "generic", positions=positions, scatter=scatter, Tmax=12, sides=SIDES[:1] + SIDES[2:3])
    # COPY on the same cases, both kernels
    for xs, kernel in ((x, "copy_packets"), (C.levels((2, 5, 3, 6), 23, I8), "copy_generic")):
        B, T, H, D = xs.shape
        cbuf, cview = C.cache_view(B, H, 12, D, xs.dtype)
        torch.ops.torchlsq.lsq_kv_copy_w8(xs, cview, C.pos_tensor(positions), scatter)
        gbuf, gview = C.cache_view(B, H, 12, D, xs.dtype, DEV)
        gx = _regrid(xs)
        assert _plan_of(gx, gview, None, 1, None, None, scatter=scatter, copy=True)["kernel"] == kernel
        torch.ops.torchlsq.lsq_kv_copy_w8(gx, gview, C.pos_tensor(positions, DEV), scatter)
        torch.cuda.synchronize()
        C.same(gbuf, cbuf, (kernel, positions, scatter))
        assert bool((cbuf.view(U8) != C.GUARD).any())


# ---------------------------------------------------------------------------------------------------
# 4: both sides of the heads-per-lane threshold
# ---------------------------------------------------------------------------------------------------
HPL = [  # D, R, interleaved, kernel, H, tokens, heads per lane: 2 x 256 workgroups of 256 lanes need 131072 (token, head group, unit) items
    (16, 16, True, "packets_interleaved", 6, 65536, 4), (16, 16, True, "packets_interleaved", 6, 65536 - 128, 2),
    (16, 16, True, "packets_interleaved", 3, 131072, 3), (16, 16, True, "packets_interleaved", 8, 40, 1),
    # half style, one pair of packets per head: H = 6 walks 4 + 2 heads
    (32, 32, False, "packets_half", 6, 65536, 4), (32, 32, False, "packets_half", 6, 65536 - 128, 2), (32, 32, False, "packets_half", 3, 131072, 3),
    # half style with packets beyond R: three units per head, a pair and two that pass through
    (64, 32, False, "packets_half", 6, 22016, 4), (64, 32, False, "packets_half", 6, 16000, 2), (64, 32, False, "packets_half", 3, 44032, 3),
    # the interleaved style with a packet beyond R
    (32, 16, True, "packets_interleaved", 6, 32768, 4)]


@pytest.mark.parametrize("D,R,interleaved,kernel,H,tokens,hpl", HPL, ids=str)
def test_heads_per_lane(D, R, interleaved, kernel, H, tokens, hpl):
    """both kernels on both sides of the grid bound, the plan's heads per lane asserted: the head walk with 4 (a partial last walk), 3,
    2 and 1 heads, with and without units beyond R"""
    x = C.levels((8, tokens // 8, H, D), H + D, U8)
    _check(x, R, kernel, (D, R, H, tokens), positions=[0, 1, 2, 3, 4, 5, 6, 7], interleaved=interleaved, sides=SIDES[:1], P=tokens // 8 + 8, hpl=hpl)


# ---------------------------------------------------------------------------------------------------
# 5, 6: repeats and batch independence
# ---------------------------------------------------------------------------------------------------
def test_repeats_and_batch_independence():
    consts = C.constants(U8)
    cos, sin = C.tables(32, 16, BF16)
    x = C.levels((2, 5, 3, 64), 31)
    runs = []
    for _ in range(2):
        buf, view = C.cache_view(2, 3, 12, 64, U8, DEV)
        C.run_rope(DEV, x, consts, cos, sin, C.OUT_U8, BF16, [0, 4], out=view, scatter=True)
        runs.append(buf)
    x2 = x.clone()
    x2[1] = C.levels((5, 3, 64), 32)
    buf2, view2 = C.cache_view(2, 3, 12, 64, U8, DEV)
    C.run_rope(DEV, x2, consts, cos, sin, C.OUT_U8, BF16, [0, 6], out=view2, scatter=True)
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1])
    first = runs[0][64:-64].view(2, 3, 12, 64)
    other = buf2[64:-64].view(2, 3, 12, 64)
    assert torch.equal(first[0], other[0]) and not torch.equal(first[1], other[1])


# ---------------------------------------------------------------------------------------------------
# 7: a decode step captured in a graph
# ---------------------------------------------------------------------------------------------------
def test_decode_step_in_a_graph():
    import copy
    from torchlsq.quantized import KVCacheW8
    case = C.decode_case()
    B, H, T, D = case["B"], case["H"], case["T"], case["D"]
    rot, core = copy.deepcopy(case["rot"]).to(DEV), copy.deepcopy(case["core"]).to(DEV)
    cache = KVCacheW8(B, H, case["Tmax"], D, device=DEV)
    # the step's static input: token 0 of this buffer; the constants are on the device before the capture
    gcase = dict(case, qkv=torch.zeros((B, 1, 3, H, D), dtype=U8, device=DEV), consts=C.to(DEV, case["consts"]))
    out = torch.zeros((B, 1, H * D), dtype=U8, device=DEV)

    def step():
        out.copy_(C.decode_step(gcase, rot, core, cache, 0, DEV))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        step()
    cache.reset()                          # only device buffers are rewritten from here on
    cache.k.zero_()
    cache.v.zero_()
    cpu_cache = KVCacheW8(B, H, case["Tmax"], D)
    for t in range(T):
        gcase["qkv"].copy_(case["qkv"][:, t:t + 1])
        g.replay()
        torch.cuda.synchronize()
        want = C.decode_step(case, case["rot"], case["core"], cpu_cache, t)
        assert torch.equal(out.cpu(), want), "replay %d is not the CPU decode" % t
        assert torch.equal(want[:, 0], case["prefill"][:, t]), "replay %d is not the prefill's row" % t
        assert cache.lengths.tolist() == [t + 1] * B
    assert torch.equal(cache.k.cpu(), cpu_cache.k) and torch.equal(cache.v.cpu(), cpu_cache.v)


# ---------------------------------------------------------------------------------------------------
# 8: smoke() with its new step
# ---------------------------------------------------------------------------------------------------
def test_smoke(capsys):
    import __graft_entry__ as ge
    ge.smoke()
    assert "rotary + KV-cache append" in capsys.readouterr().out
