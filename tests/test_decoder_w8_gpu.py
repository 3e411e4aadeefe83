"""A whole decoder layer on 8-bit levels on the GPU (tests/decoder_w8_cases.py): every stage of the layer and the cache against the CPU
path's, bit for bit, for the whole sequence as one prompt, as a prompt and steps and token by token, on the dense, the split and the
paged cache routes, for one batch entry alone and for a whole-layer decode step replayed from a graph -- and the `mid_dtype=float32` run
against a plain float64 model of the layer, a reference that is not the package.  Before a comparison the plan functions are asked, on
the operands' real strides and alignment, which kernels the calls took: a silent fall to the composition cannot pass for the kernels.
Every comparison with the CPU path is torch.equal.
"""
import copy
import functools

import pytest
import torch

import attn_fused_w8_cases as F
import attn_paged_w8_cases as P
import decoder_w8_cases as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = tuple(L.CASES)


def _mid_id(mid):
    return str(mid).replace("torch.", "")


@functools.lru_cache(maxsize=None)
def gpu_layer(name, mid):
    """the CPU-built layer moved: its constants, tables and weights are those of the CPU run"""
    return copy.deepcopy(L.chain(name, mid)).to(DEV)


def gpu_input(name, rows=slice(None)):
    from torchlsq.functional import LevelsTensor
    xl = L.input_levels(name)
    return LevelsTensor(xl.levels[rows].contiguous().to(DEV), xl.scale.to(DEV), xl.zero_point.to(DEV), xl.quant_min, xl.quant_max)


def _aligned(*tensors):
    return all(t.data_ptr() % 16 == 0 for t in tensors)


def _strides_are(t, want):
    """on every axis of more than one element (the stride of an axis of one is never used and torch reports what it likes)"""
    return all(n == 1 or s == w for n, s, w in zip(t.shape, t.stride(), want))


def plan_check(name, layer, cache, route, seen):
    """the `each` of `L.sequence`: asserts the kernels a call took from the plan functions, on the operands as they lie"""
    from torchlsq import extension as E
    c = L.CASES[name]
    H, Hkv, D, d, hidden, Tmax = (c[k] for k in ("H", "Hkv", "D", "d", "hidden", "Tmax"))
    W = (H + 2 * Hkv) * D

    def each(T, start, mids):
        B = int(mids["n1"].shape[0])
        M = B * T
        # the four linears: matrix cores and a tiled shape; the libraries with an 8-bit output have no decode shape, a step (M <= 16)
        # takes their 32-row tile
        for mod, x, y, res, N, K in ((layer.qkv, "n1", "qkv", None, W, d), (layer.proj, "ctx", "add1", "x", d, H * D),
                                     (layer.fc1, "n2", "fc1", None, hidden, d), (layer.fc2, "gelu", "out", "add1", d, hidden)):
            ok = _aligned(mids[x].levels, mod.weight_levels)
            if res is None:
                pl = E.requant_w8_plan_linear(M, N, K, aligned=ok, y_aligned=_aligned(mids[y].levels))
            else:
                pl = E.resadd_w8_plan_linear(M, N, K, aligned=ok, y_aligned=_aligned(mids[y].levels), res_aligned=_aligned(mids[res].levels))
                assert pl["res_load"] == "packets", pl
            assert pl["form"] == "mfma" and pl["shape"] in ("tiles", "tiles_split_k") and pl["store"] == "packets", (y, M, pl)
            assert M > 16 or pl["rows_per_tile"] == 32, (y, M, pl)
            seen.add(("linear", "step" if M <= 16 else "prompt", pl["shape"], pl["rows_per_tile"]))
        assert E.norm_w8_plan(M, d, aligned=_aligned(mids["x"].levels, mids["n1"].levels, mids["add1"].levels, mids["n2"].levels),
                              has_bias=False, kind="rms")["family"] == "packets"
        # rope reads the q view of the qkv buffer in place and writes the q columns of a second one
        q4 = mids["rq"].levels
        assert tuple(q4.shape) == (B, T, H, D) and _strides_are(q4, (T * W, W, D, 1))
        qv = L.heads(mids["qkv"], H, Hkv, D)[0].levels
        rp = E.rope_w8_plan(B, T, H, D, P=Tmax, x_strides=tuple(qv.stride()[:3]), y_strides=tuple(q4.stride()[:3]),
                            aligned=_aligned(qv, q4, layer.rot.cos, layer.rot.sin))
        assert rp["kernel"] == "packets_half", rp
        q = q4.permute(0, 2, 1, 3)
        k, v = mids["k_cache"].levels, mids["v_cache"].levels
        kw = dict(q_strides=F.strides(q), qkv_aligned=_aligned(q, k, v), causal=True, has_lengths=True)
        assert _strides_are(q, (T * W, D, W, 1))              # the qkv view's strides
        if L.is_paged(cache):
            Np, ps, Mp = int(k.shape[0]), int(k.shape[2]), int(cache.block_table.shape[1])
            pl = E.attn_paged_w8_plan(B, H, Hkv, T, D, Np, ps, Mp, 2, bt_ld=int(cache.block_table.stride(0)) if B > 1 else Mp,
                                      k_strides=P.pool_strides(k), v_strides=P.pool_strides(v),
                                      causal_offset=Tmax - 1 if T == 1 else start, **kw)
            # (more than 16 query rows per kv head: the pages are gathered and the existing ops composed)
            assert pl["family"] == ("paged" if T == 1 else "composition"), pl
            assert T > 1 or (pl["splits"] == 2 and pl["chunk"] == 64), pl
        else:
            kw.update(k_strides=F.strides(k), v_strides=F.strides(v))
            if T == 1 and route == "split":
                pl = E.attn_decode_split_w8_plan(B, H, Hkv, 1, Tmax, D, 2, causal_offset=Tmax - 1, **kw)
                assert pl["family"] == "split" and pl["splits"] == 2 and pl["chunk"] == 64, pl
            elif T == 1:
                pl = E.attn_decode_w8_plan(B, H, Hkv, 1, Tmax, D, causal_offset=Tmax - 1, **kw)
                assert pl["family"] == "decode", pl
            else:
                assert E.attn_decode_w8_plan(B, H, Hkv, T, Tmax, D, causal_offset=start, **kw)["family"] != "decode"
                pl = E.attn_prefill_w8_plan(B, H, Hkv, T, Tmax, D, causal_offset=start, **kw)
                assert pl["family"] == "prefill", pl
        seen.add(("attention", pl["family"]))
    return each


def gpu_sequence(name, mid, how, route, rows=slice(None)):
    """(the GPU's levels of the sequence by stage, what the plans said)"""
    layer, xl = gpu_layer(name, mid), gpu_input(name, rows)
    cache, seen = L.make_cache(name, route, DEV, B=int(xl.shape[0])), set()
    with torch.no_grad():
        got = L.sequence(layer, xl, cache, L.chunks_of(name, how), route, each=plan_check(name, layer, cache, route, seen))
    return got, seen


@functools.lru_cache(maxsize=None)
def gpu_whole(name, mid):
    """the whole prompt on the dense cache, once per case and mid_dtype: leave it unchanged"""
    return gpu_sequence(name, mid, "whole", "dense")


# ---------------------------------------------------------------------------------------------------
# 1, 2: the whole prompt, stage by stage against the CPU run and against float64
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mid", L.MIDS, ids=_mid_id)
@pytest.mark.parametrize("name", NAMES)
def test_the_whole_prompt_stage_by_stage_against_the_cpu_run(name, mid):
    got, seen = gpu_whole(name, mid)
    assert ("attention", "prefill") in seen and {s[:2] for s in seen if s[0] == "linear"} == {("linear", "prompt")}, seen
    assert L.differing(got, L.cpu_run(name, mid)) == [], (name, _mid_id(mid))


@pytest.mark.parametrize("name", NAMES)
def test_float32_against_the_float64_reference(name):
    """the same run against a reference that is not the package: no level further than 1, at most 0.1 % of a stage's levels different"""
    L.assert_close_to_reference(gpu_whole(name, L.F32)[0], name, "float32, GPU")


# ---------------------------------------------------------------------------------------------------
# 3: prompt then steps, and token by token
# ---------------------------------------------------------------------------------------------------
STEP_FAMILY = {"dense": "decode", "split": "split", "paged": "paged"}


def _steps_equal_the_whole_prompt(name, mid, how, route):
    c = L.CASES[name]
    got, seen = gpu_sequence(name, mid, how, route)
    assert ("attention", STEP_FAMILY[route]) in seen, seen
    assert ("linear", "step", "tiles_split_k", 32) in seen and c["B"] <= 16, seen
    if how == "steps":
        assert ("attention", "composition" if route == "paged" else "prefill") in seen, seen
    assert L.differing(got, gpu_whole(name, mid)[0]) == [], (name, how, route, "against the GPU's whole prompt")
    assert L.differing(got, L.cpu_run(name, mid)) == [], (name, how, route, "against the CPU's whole prompt")


@pytest.mark.parametrize("route", L.ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_prompt_then_steps(name, route):
    c = L.CASES[name]
    if name == "long":
        assert c["prompt"] < 64 < L.total(c) and c["prompt"] // L.PAGE < (L.total(c) - 1) // L.PAGE        # a chunk and a page border
    _steps_equal_the_whole_prompt(name, L.BF16, "steps", route)


@pytest.mark.parametrize("route", L.ROUTES)
def test_token_by_token(route):
    _steps_equal_the_whole_prompt("short", L.F16, "tokens", route)


# ---------------------------------------------------------------------------------------------------
# 4: a batch entry alone
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_a_batch_entry_alone(name):
    """B = 1: the linears at T rows and at one row; the result is its rows of the B = 2 run"""
    got, seen = gpu_sequence(name, L.BF16, "steps", "dense", rows=slice(1, 2))
    assert ("attention", "prefill") in seen and ("attention", "decode") in seen, seen
    want, cpu = gpu_whole(name, L.BF16)[0], L.cpu_run(name, L.BF16)
    for s in L.STAGES + L.CACHED:
        assert torch.equal(got[s], want[s][1:2]) and torch.equal(got[s], cpu[s][1:2]), (name, s)


# ---------------------------------------------------------------------------------------------------
# 5: one whole-layer decode step in a graph
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ("split", "paged"))
def test_a_whole_layer_decode_step_replays_in_a_graph(route):
    """the prompt of `long` eagerly, then ONE step of the whole layer -- norm, qkv, rope, append, attention, proj + x, norm, fc1, GELU,
    fc2 + residual -- captured once, the constants on the device before the capture and the workspaces allocated inside it; a replay
    per step with only the token buffer rewritten: every stage equals the eager GPU step and the CPU run's row, `lengths` follows
    across the 64-key chunk border and a page border"""
    name, mid = "long", L.BF16
    c = L.CASES[name]
    Pn, B = c["prompt"], c["B"]
    layer, xl, cpu = gpu_layer(name, mid), gpu_input(name), L.cpu_run(name, mid)
    caches = [L.make_cache(name, route, DEV) for _ in range(2)]            # the graph's and the eager run's
    seen = set()
    with torch.no_grad():
        for cache in caches:
            L.run(layer, L.with_levels(xl, xl.levels[:, :Pn].contiguous()), cache, 0, route)
    graph_cache, eager_cache = caches
    token = L.with_levels(xl, xl.levels[:, Pn:Pn + 1].contiguous())        # the buffer the replays read
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        L.run(layer, token, graph_cache, True, route)
    torch.cuda.current_stream().wait_stream(side)
    graph_cache.lengths.fill_(Pn)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        _, held = L.run(layer, token, graph_cache, True, route)
    graph_cache.lengths.fill_(Pn)
    check = plan_check(name, layer, eager_cache, route, seen)
    for t in range(c["steps"]):
        token.levels.copy_(xl.levels[:, Pn + t:Pn + t + 1])
        graph.replay()
        with torch.no_grad():
            _, eager = L.run(layer, L.with_levels(xl, xl.levels[:, Pn + t:Pn + t + 1].contiguous()), eager_cache, True, route)
        check(1, Pn + t, eager)
        assert graph_cache.lengths.tolist() == [Pn + t + 1] * B == eager_cache.lengths.tolist()
        for s in L.STAGES:
            got = held[s].levels.reshape(B, 1, -1)
            assert torch.equal(got, eager[s].levels.reshape(B, 1, -1)), (route, t, s, "against the eager step")
            assert torch.equal(got.cpu(), cpu[s][:, Pn + t:Pn + t + 1]), (route, t, s, "against the CPU run")
    assert ("attention", STEP_FAMILY[route]) in seen and graph_cache.lengths.tolist() == [L.total(c)] * B and L.total(c) > 64
    for got, want in zip(L.cached(graph_cache, held["k_cache"], held["v_cache"], L.total(c)), (cpu["k"], cpu["v"])):
        assert torch.equal(got.cpu(), want)
