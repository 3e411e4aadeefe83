"""What tests/test_decoder_w8_cpu.py and tests/test_decoder_w8_gpu.py share: ONE WHOLE pre-norm decoder layer on 8-bit levels, built from
the ops the other suites test one at a time,

    x -> RMSNorm n1 -> qkv Linear(d, (H + 2 Hkv) D) -> split -> rotary on q and k -> cache append -> causal grouped-query attention
      (alpha D^-1/2) -> proj Linear + x -> RMSNorm n2 -> fc1 -> GELU -> fc2 + residual

as a float `nn.Module` (`DecoderLayer`, `nn.Linear` children: the weight quantizers come from `prepare_qat` as in
`norm_w8_cases._prepared`, per-channel symmetric qint8), its per-tensor quint8 activation quantizers fitted stage by stage on the whole
sequence (`requant_w8_cases.trained_quantizer`, each on the float op applied to the fake-quantized values of the stage before; the
probabilities take `attn_w8_cases.trained(0, 1)`), the conversion through the modules' `from_float` (`Chain`), `heads` (the qkv
`LevelsTensor` cut into its q, k and v views, nothing copied), `run` (one call of the layer on a cache: the output and every
intermediate `LevelsTensor`), `sequence` (a sequence fed in chunks: one prompt, a prompt and steps, token by token) and `reference`
(the same layer in plain torch float64).  Everything is seeded and computed once per case.

The quantizer SITES, fourteen: the input, n1, qkv; the rotary output (one quantizer for q and k; v stays on qkv's); scores,
probabilities, context; proj's own output and the first add; n2, fc1, GELU, fc2's own output and the second add.  The STAGES a run hands
out are the nine `LevelsTensor`s that exist in memory -- n1, qkv, rq (rotated q), ctx, add1, n2, fc1, gelu, out -- and the cache's k
(rotated) and v; scores and probabilities never leave the attention kernels, and the two linears' own outputs never leave their
epilogues.

The two CASES are the smallest shapes at which each mechanism is live: `short` has the heads of `attn_decode_w8_cases.gqa_decode_case`;
in `long` four query heads share a kv head and the lengths run 61 .. 67, across the 64-key chunk border of the split and paged kernels
and a page border (page size 16, 8 pages per entry, a pool of 2 * 8 + 1 pages under a seeded permutation).  Tmax is 128: the split plan
refuses two splits below 65 keys.  q is rotated into the q columns of a second [B, T, (H + 2 Hkv) D] buffer, so attention reads q at
the qkv view's strides (T W, D, W); k is rotated into the cache and v appended from its view in place.

THE FLOAT64 REFERENCE knows nothing of the ops: the dequantized weight levels, the textbook RMSNorm, matmul and bias, half-rotation
rope from float64 angles, a masked `softmax`, the erf GELU and the residual adds, and at each site clamp(rint(v / s) + z, quant_min,
quant_max) with that site's scale and zero point.  No integer table, no `mid_dtype` rounding, no fp32 step.  It runs FREE: each stage
reads the reference's own levels of the stage before.  The condition a `mid_dtype=float32` run is held to, on the CPU and on the GPU
(`assert_close_to_reference`): no level further than 1 from the reference's, and at most 0.1 % of a stage's levels different.

MEASURED on the CPU path (the GPU's bytes are the same), whole prompt, per cent of a stage's levels that differ from the float64
reference's / worst distance in levels; a stage of `short` holds 2 816 to 11 264 levels, one of `long` 17 152 to 137 216:

    case   mid       n1        qkv        rq         k          v          ctx        add1       n2         fc1        gelu       out
    short  float32   0/0       0/0        0/0        0/0        0/0        0/0        0/0        0/0        0/0        0/0        0/0
    long   float32   0/0       0/0        0/0        0/0        0/0        0/0        0/0        0/0        0/0        0/0        0/0
    short  bfloat16  1.85/1    12.23/1    15.27/2    14.99/2    12.68/1    44.27/7    30.31/2    27.47/3    42.09/3    29.96/6    34.62/3
    long   bfloat16  1.28/1    10.75/1    14.84/2    14.96/2    10.54/1    48.39/8    33.78/3    27.76/3    46.05/3    33.31/6    38.35/4
    short  float16   0.14/1    1.61/1     1.92/2     2.34/2     1.74/1     13.16/5    12.50/2    12.27/2    26.11/3    18.47/5    15.84/3
    long   float16   0.14/1    2.82/1     3.75/2     3.70/2     2.78/1     28.42/8    22.43/2    18.40/3    38.04/3    27.15/5    26.91/3

At bfloat16 and float16 the model between the quantizers is by definition not real arithmetic: those shares are printed by the CPU test
and nothing is asserted about them.

WHAT THE FLOAT32 ZEROS ARE WORTH.  The float32 steps of the definition put a value within about 2e-5 of a level off real arithmetic,
so roughly one output in 10^5 lies so near a tie that the two round apart: a legitimate difference of one level.  Free running, such
a level does not stay alone.  One level in n2 moves a few per cent of its row of fc1 by a level, and the GELU's output quantizer is about
twice as fine as its input's (it covers half the range), so one level of fc1 becomes two or three of gelu; one level in n1 reaches k and
v and from there every later row's context.  Over the seeds 0 .. 7 `short` had no differing level at any seed; `long` (about 820 000
levels in all) had none at one seed, three levels off by one at a second, near-ties whose wake broke the 1-level cap at gelu at four, and a
near-tie in n1 whose wake broke both conditions at two.  `long` therefore takes the seed without a near-tie (6) -- the seed moves, the cap
stays --: with it any level that moves anywhere in the layer shows, which is what the test is for, and a change of the inputs (seed,
shapes, calibration) may meet a near-tie again and needs the seed looked at, not the cap.  The quantizers
are fitted on float64 intermediates for the same reason: fitted on float32 matmuls they, and the place of the near-ties, depended on the
machine's BLAS; as they are, the constants, the CPU path's levels and the reference's were the same bytes on two different machines.
"""
import functools

import torch

import attn_w8_cases as A
import norm_w8_cases as N
import requant_w8_cases as R

F32, BF16, F16 = A.F32, A.BF16, A.F16
MIDS = R.MIDS
PAGE, PAGES = 16, 8
ROUTES = ("dense", "split", "paged")
STAGES = ("n1", "qkv", "rq", "ctx", "add1", "n2", "fc1", "gelu", "out")
CACHED = ("k", "v")
CASES = {"short": dict(B=2, H=4, Hkv=2, D=32, d=128, hidden=256, prompt=19, steps=3, Tmax=128, seed=0),
         "long": dict(B=2, H=8, Hkv=2, D=64, d=512, hidden=1024, prompt=61, steps=6, Tmax=128, seed=6)}
BASE = 10000.0
EPS = 1e-6
MAX_SHARE, MAX_DISTANCE = 1e-3, 1


def total(c):
    return c["prompt"] + c["steps"]


# ---------------------------------------------------------------------------------------------------
# plain torch, any floating dtype: what the float layer and the float64 reference compute between two quantizers
# ---------------------------------------------------------------------------------------------------
def rope(t, start=0):
    """half-rotation rotary embedding of t [B, T, heads, D] at the positions start .. start + T - 1, the angles in float64"""
    T, D = int(t.shape[1]), int(t.shape[3])
    inv = torch.pow(torch.tensor(BASE, dtype=torch.float64), -torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = (start + torch.arange(T, dtype=torch.float64)).reshape(T, 1) * inv.reshape(1, -1)
    c, s = (f(ang).to(t.dtype).reshape(1, T, 1, D // 2) for f in (torch.cos, torch.sin))
    a, b = t[..., :D // 2], t[..., D // 2:]
    return torch.cat((a * c - b * s, b * c + a * s), -1)


def scores_of(q, k):
    """q [B, T, H, D] on k [B, T, Hkv, D] -> q k^T [B, H, T, T]: query head h reads kv head h // (H / Hkv)"""
    return torch.einsum("bthd,bshd->bhts", q, k.repeat_interleave(q.shape[2] // k.shape[2], dim=2))


def causal(T):
    return torch.ones(T, T, dtype=torch.bool).tril()


def causal_softmax(s, alpha):
    return torch.softmax((alpha * s).masked_fill(~causal(int(s.shape[-1])), float("-inf")), -1)


def context_of(p, v):
    """p [B, H, T, T] on v [B, T, Hkv, D] -> [B, T, H D]"""
    y = torch.einsum("bhts,bshd->bthd", p, v.repeat_interleave(p.shape[1] // v.shape[2], dim=2))
    return y.reshape(y.shape[0], y.shape[1], -1)


def rms_norm(v, w, eps=EPS):
    return v / torch.sqrt((v * v).mean(-1, keepdim=True) + eps) * w


def gelu(v):
    return 0.5 * v * (1 + torch.erf(v / 2.0 ** 0.5))


# ---------------------------------------------------------------------------------------------------
# the float layer and its quantizers
# ---------------------------------------------------------------------------------------------------
class DecoderLayer(torch.nn.Module):
    def __init__(self, H, Hkv, D, d, hidden):
        super().__init__()
        self.H, self.Hkv, self.D = H, Hkv, D
        self.n1 = torch.nn.RMSNorm(d, eps=EPS)
        self.qkv = torch.nn.Linear(d, (H + 2 * Hkv) * D)
        self.proj = torch.nn.Linear(H * D, d)
        self.n2 = torch.nn.RMSNorm(d, eps=EPS)
        self.fc1 = torch.nn.Linear(d, hidden)
        self.act = torch.nn.GELU()
        self.fc2 = torch.nn.Linear(hidden, d)

    def split(self, h):
        """a float qkv [B, T, (H + 2 Hkv) D] as q [B, T, H, D], k and v [B, T, Hkv, D]"""
        H, Hkv, D = self.H, self.Hkv, self.D
        h = h.reshape(h.shape[0], h.shape[1], H + 2 * Hkv, D)
        return h[:, :, :H], h[:, :, H:H + Hkv], h[:, :, H + Hkv:]

    def forward(self, x):
        q, k, v = self.split(self.qkv(self.n1(x)))
        p = causal_softmax(scores_of(rope(q), rope(k)), self.D ** -0.5)
        a = self.proj(context_of(p, v)) + x
        return self.fc2(self.act(self.fc1(self.n2(a)))) + a


@functools.lru_cache(maxsize=None)
def fitted(name):
    """(the QAT layer in eval mode, its fourteen activation quantizers by site, the float32 sequence [B, prompt + steps, d])"""
    c = CASES[name]
    torch.manual_seed(6100 + c["seed"])
    net = DecoderLayer(c["H"], c["Hkv"], c["D"], c["d"], c["hidden"])
    g = torch.Generator().manual_seed(6200 + c["seed"])
    with torch.no_grad():
        net.qkv.weight.mul_(3.0)                 # scores of a few units: a softmax that is neither flat nor one-hot
        for norm in (net.n1, net.n2):
            norm.weight.copy_(1 + 0.2 * torch.randn(norm.weight.shape, generator=g))
    x = torch.randn(c["B"], total(c), c["d"], generator=g) * 2
    net = N._prepared(net, x)
    qs = {}

    # The float ops between two quantizers run in float64 and a quantizer sees their float32 rounding: a float32 matmul's last bits
    # depend on the machine's BLAS, a quantizer fitted to its minimum and maximum would too, and with it every level near a tie.
    def fit(site, sample):
        qs[site] = R.trained_quantizer(sample.float())
        return qs[site](sample.float()).double()

    def linear(mod, v):
        return v @ mod.weight_fake_quant(mod.weight).double().t() + mod.bias.double()

    with torch.no_grad():
        xq = fit("in", x)
        h = fit("qkv", linear(net.qkv, fit("n1", rms_norm(xq, net.n1.weight.double()))))
        q, k, v = net.split(h)
        rq, rk = rope(q), rope(k)
        qs["rot"] = R.trained_quantizer(torch.cat((rq.flatten(), rk.flatten())).float())
        rq, rk = (qs["rot"](t.float()).double() for t in (rq, rk))
        s = scores_of(rq, rk)
        qs["scores"] = R.trained_quantizer(s[..., causal(total(c))].float())       # what a row sees: nothing above the diagonal is read
        qs["probs"] = A.trained(0.0, 1.0)
        p = causal_softmax(qs["scores"](s.float()).double(), c["D"] ** -0.5)
        y = fit("ctx", context_of(qs["probs"](p.float()).double(), v))
        a1 = fit("add1", fit("proj", linear(net.proj, y)) + xq)
        f1 = fit("fc1", linear(net.fc1, fit("n2", rms_norm(a1, net.n2.weight.double()))))
        f2 = fit("fc2", linear(net.fc2, fit("gelu", gelu(f1))))
        fit("add2", f2 + a1)
    return net, qs, x


def input_levels(name):
    """the sequence as the LevelsTensor [B, prompt + steps, d] of the input quantizer, on the CPU"""
    from torchlsq.functional import LevelsTensor
    _, qs, x = fitted(name)
    return LevelsTensor.from_quantized(qs["in"].quantize(x))


# ---------------------------------------------------------------------------------------------------
# the layer on levels
# ---------------------------------------------------------------------------------------------------
class Chain(torch.nn.Module):
    """the converted layer: every module from its `from_float`; `.to(device)` moves the constants, the tables and the weights"""

    def __init__(self, net, qs, mid, Tmax):
        from torchlsq.quantized import ActivationW8Q, AttentionCoreW8Q, LinearW8A8AddQ, LinearW8A8Q, RMSNormW8Q, RotaryW8Q
        super().__init__()
        self.H, self.Hkv, self.D = net.H, net.Hkv, net.D
        self.n1 = RMSNormW8Q.from_float(net.n1, qs["n1"], mid_dtype=mid)
        self.qkv = LinearW8A8Q.from_float(net.qkv, qs["n1"], qs["qkv"], mid_dtype=mid)
        self.rot = RotaryW8Q(qs["rot"], net.D, Tmax, base=BASE, mid_dtype=mid)
        self.core = AttentionCoreW8Q(qs["scores"], qs["probs"], qs["ctx"], alpha=net.D ** -0.5, mid_dtype=mid, prefill=True)
        self.proj = LinearW8A8AddQ.from_float(net.proj, qs["ctx"], qs["add1"], pre_quantizer=qs["proj"], mid_dtype=mid)
        self.n2 = RMSNormW8Q.from_float(net.n2, qs["n2"], mid_dtype=mid)
        self.fc1 = LinearW8A8Q.from_float(net.fc1, qs["n2"], qs["fc1"], mid_dtype=mid)
        self.act = ActivationW8Q.from_float(net.act, qs["fc1"], qs["gelu"], mid_dtype=mid)
        self.fc2 = LinearW8A8AddQ.from_float(net.fc2, qs["gelu"], qs["add2"], pre_quantizer=qs["fc2"], mid_dtype=mid)


@functools.lru_cache(maxsize=None)
def chain(name, mid):
    """the converted layer of a case on the CPU, built once: copy.deepcopy(...).to(device) it, never change it"""
    net, qs, _ = fitted(name)
    return Chain(net, qs, mid, CASES[name]["Tmax"]).eval()


def with_levels(x, levels):
    from torchlsq.functional import LevelsTensor
    return LevelsTensor(levels, x.scale, x.zero_point, x.quant_min, x.quant_max, x.type_min, x.type_max)


def heads(qkv, H, Hkv, D):
    """the qkv LevelsTensor [B, T, (H + 2 Hkv) D] as q [B, T, H, D], k and v [B, T, Hkv, D]: views of its bytes, nothing is copied"""
    B, T, W = (int(n) for n in qkv.shape)
    assert W == (H + 2 * Hkv) * D
    lv = qkv.levels.view(B, T, H + 2 * Hkv, D)
    q, k, v = (with_levels(qkv, lv[:, :, a:b]) for a, b in ((0, H), (H, H + Hkv), (H + Hkv, H + 2 * Hkv)))
    assert q.levels.data_ptr() == qkv.levels.data_ptr() and v.levels.data_ptr() == qkv.levels.data_ptr() + (H + Hkv) * D
    return q, k, v


def is_paged(cache):
    return hasattr(cache, "block_table")


def run(layer, x, cache, causal, route="dense"):
    """one call of the layer: x a LevelsTensor [B, T, d] of the input quantizer, its tokens appended to `cache` at the cache's
    lengths; `causal`: the offset (the tokens the cache held) for a prompt, True for a step; `route`: "split" and "paged" set the core's
    split=2 (a step's keys in two chunks of 64), a paged cache is read through its block table -> (the output LevelsTensor [B, T, d], every intermediate by stage)"""
    H, Hkv, D = layer.H, layer.Hkv, layer.D
    layer.core.causal = causal
    layer.core.split = None if route == "dense" else 2
    n1 = layer.n1(x)
    qkv = layer.qkv(n1)
    q, k, v = heads(qkv, H, Hkv, D)
    B, T = int(q.shape[0]), int(q.shape[1])
    rbuf = torch.empty_like(qkv.levels)                      # the rotated q in the q columns of a second qkv buffer
    rq = layer.rot(q, positions=cache.lengths, out=rbuf[..., :H * D].view(B, T, H, D))
    kl, vl, lens = cache.append(k, v, rotary=layer.rot)
    ctx = layer.core(with_levels(rq, rq.levels.permute(0, 2, 1, 3)), kl, vl, key_lengths=lens,
                     block_table=cache.block_table if is_paged(cache) else None)
    add1 = layer.proj(ctx, x)
    n2 = layer.n2(add1)
    fc1 = layer.fc1(n2)
    gl = layer.act(fc1)
    out = layer.fc2(gl, add1)
    return out, dict(x=x, n1=n1, qkv=qkv, rq=rq, ctx=ctx, add1=add1, n2=n2, fc1=fc1, gelu=gl, out=out, k_cache=kl, v_cache=vl)


def make_cache(name, route, device=None, B=None):
    """an empty cache of a case: KVCacheW8 for "dense" and "split", PagedKVCacheW8 under a seeded permutation for "paged" """
    from torchlsq.quantized import KVCacheW8, PagedKVCacheW8
    c = CASES[name]
    B = c["B"] if B is None else B
    if route != "paged":
        return KVCacheW8(B, c["Hkv"], c["Tmax"], c["D"], device=device)
    assert PAGE * PAGES == c["Tmax"]
    Np = 2 * PAGES + 1
    cache = PagedKVCacheW8(Np, c["Hkv"], PAGE, c["D"], B, PAGES, device=device)
    table = torch.randperm(Np, generator=A.gen(400 + c["seed"]))[:c["B"] * PAGES].reshape(c["B"], PAGES).to(torch.int32)
    cache.block_table.copy_(table[:B])
    return cache


def cached(cache, kl, vl, length):
    """the first `length` slots of the cache as dense levels [B, Hkv, length, D]: (k, v); a paged pool gathered through its table"""
    if is_paged(cache):
        from torchlsq.functional import lsq_kv_gather_paged_w8
        kl, vl = lsq_kv_gather_paged_w8(kl, cache.block_table), lsq_kv_gather_paged_w8(vl, cache.block_table)
    return kl.levels[:, :, :length], vl.levels[:, :, :length]


def chunks_of(name, how):
    c = CASES[name]
    return {"whole": [total(c)], "steps": [c["prompt"]] + [1] * c["steps"], "tokens": [1] * total(c)}[how]


def sequence(layer, xl, cache, chunks, route="dense", each=None):
    """the sequence xl [B, T, d] fed to the layer in `chunks` (token counts) from the cache as it is (empty) -> {stage: the levels of
    every call joined along T, on the CPU; "k", "v": the cache's first T slots}; `each(T, start, mids)` sees every call"""
    got, start = {s: [] for s in STAGES}, 0
    for T in chunks:
        x = with_levels(xl, xl.levels[:, start:start + T].contiguous())
        _, mids = run(layer, x, cache, True if T == 1 else start, route)
        if each is not None:
            each(T, start, mids)
        for s in STAGES:
            lv = mids[s].levels
            got[s].append(lv.reshape(lv.shape[0], T, -1).cpu())
        start += T
    out = {s: torch.cat(v, 1) for s, v in got.items()}
    assert cache.lengths.tolist() == [start] * int(xl.shape[0])
    out["k"], out["v"] = (t.cpu() for t in cached(cache, mids["k_cache"], mids["v_cache"], start))
    return out


@functools.lru_cache(maxsize=None)
def cpu_run(name, mid, how="whole", route="dense"):
    """the CPU path's levels of the whole sequence, computed once and shared: leave them unchanged"""
    import copy
    return sequence(copy.deepcopy(chain(name, mid)), input_levels(name), make_cache(name, route), chunks_of(name, how), route)


def differing(a, b):
    """the stages (and cache sides) at which two results of `sequence` are not the same bytes: a failure names them"""
    return [s for s in STAGES + CACHED if not (a[s].shape == b[s].shape and torch.equal(a[s], b[s]))]


# ---------------------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------------------
def site(q):
    """(scale, zero point, quant_min, quant_max) of a site as plain numbers, from the constants the package derives for the quantizer"""
    from torchlsq.functional import _act_constants
    from torchlsq.quantized.modules.packed_linear_a8 import _per_tensor_constants
    scale, shift, qmin, qmax, tmin, tmax = _per_tensor_constants(q, "site")
    s, z = _act_constants(scale, shift, tmin, tmax)
    return float(s.double()), int(z), qmin, qmax


def to_levels(v, st):
    s, z, lo, hi = st
    return torch.clamp(torch.round(v / s) + z, lo, hi)           # torch.round: half to even, rint


def values(lv, st):
    return (lv - st[1]) * st[0]


def weight64(m):
    """(the dequantized weight levels [out, in], the bias) of a converted linear in float64"""
    w = (m.weight_levels.double() - m.weight_zero_point.double().reshape(-1, 1)) * m.weight_scale.double().reshape(-1, 1)
    return w, m.bias.detach().double()


@functools.lru_cache(maxsize=None)
def reference(name):
    """{stage: float64 levels of the whole sequence as one causal prompt, "k", "v" as `sequence` gives them}"""
    c = CASES[name]
    net, qs, x = fitted(name)
    m = chain(name, F32)
    st = {k: site(q) for k, q in qs.items()}
    H, Hkv, D = c["H"], c["Hkv"], c["D"]
    B, T = c["B"], total(c)

    def linear(lv, src, mod, dst):
        w, b = weight64(mod)
        return to_levels(values(lv, st[src]) @ w.t() + b, st[dst])

    out = {}
    x0 = to_levels(x.double(), st["in"])
    out["n1"] = to_levels(rms_norm(values(x0, st["in"]), m.n1.weight.double(), m.n1.eps), st["n1"])
    out["qkv"] = linear(out["n1"], "n1", m.qkv, "qkv")
    q, k, v = (t for t in net.split(values(out["qkv"], st["qkv"])))
    rq, rk = to_levels(rope(q), st["rot"]), to_levels(rope(k), st["rot"])
    out["rq"] = rq.reshape(B, T, H * D)
    out["k"], out["v"] = rk.permute(0, 2, 1, 3), net.split(out["qkv"])[2].permute(0, 2, 1, 3)
    s = to_levels(scores_of(values(rq, st["rot"]), values(rk, st["rot"])), st["scores"])
    p = to_levels(causal_softmax(values(s, st["scores"]), D ** -0.5), st["probs"])
    out["ctx"] = to_levels(context_of(values(p, st["probs"]), v), st["ctx"])
    o = linear(out["ctx"], "ctx", m.proj, "proj")
    out["add1"] = to_levels(values(o, st["proj"]) + values(x0, st["in"]), st["add1"])
    out["n2"] = to_levels(rms_norm(values(out["add1"], st["add1"]), m.n2.weight.double(), m.n2.eps), st["n2"])
    out["fc1"] = linear(out["n2"], "n2", m.fc1, "fc1")
    out["gelu"] = to_levels(gelu(values(out["fc1"], st["fc1"])), st["gelu"])
    o = linear(out["gelu"], "gelu", m.fc2, "fc2")
    out["out"] = to_levels(values(o, st["fc2"]) + values(out["add1"], st["add1"]), st["add2"])
    return out


def distance(got, name):
    """{stage: (the share of levels that differ from the float64 reference's, the worst distance in levels)}"""
    ref, res = reference(name), {}
    for s in STAGES + CACHED:
        d = (got[s].double().reshape(ref[s].shape) - ref[s]).abs()
        res[s] = (float((d != 0).double().mean()), int(d.max()))
    return res


def distance_line(res):
    return "  ".join("%s %.3f%%/%d" % (s, 100 * res[s][0], res[s][1]) for s in STAGES + CACHED)


def assert_close_to_reference(got, name, note=""):
    res = distance(got, name)
    print("%s %s against float64: %s" % (name, note, distance_line(res)))
    for s, (share, worst) in res.items():
        assert worst <= MAX_DISTANCE and share <= MAX_SHARE, (name, note, s, "%.4f %% of the levels differ, by at most %d" % (100 * share, worst))
    return res
