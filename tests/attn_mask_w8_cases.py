"""What tests/test_attn_mask_w8_cpu.py and tests/test_attn_mask_w8_gpu.py share: the prefix lengths of a masked softmax restated in
plain Python, the masked ops run on a device of choice, the output side's level of 0 from the existing levels op, and the
composition `y[r, :n] == the existing softmax of x[r, :n]` that holds the masked op to the unmasked one bit for bit.  Inputs,
tables and quantizers come from attn_w8_cases; everything is seeded.
"""
import torch

import attn_w8_cases as A

F32, BF16, F16, U8, I8 = A.F32, A.BF16, A.F16, A.U8, A.I8
INT8_Q = (A.one(1.0 / 255), A.one(128.0 / 255), -128, 127, -128, 127)       # zero point -128: the level of 0 is not the byte 0
SHIFTED_Q = (A.one(1.0 / 200), A.one(-0.1), 0, 255, 0, 255)                 # zero point 20
SIDES = ((A.PROB_Q, BF16), (INT8_Q, F32), (SHIFTED_Q, F16), (None, F32), (None, BF16), (None, F16))


def prefix_lengths(shape, offset=None, lengths=None):
    """n_r of the contract for x of `shape` [.., Tq, Tk], row by row in Python: `offset` the causal offset (None: not causal),
    `lengths` one int per leading index (None: none)"""
    Tq, C = int(shape[-2]), int(shape[-1])
    R = 1
    for d in shape[:-1]:
        R *= int(d)
    per = R // int(shape[0]) if lengths is not None else None
    out = []
    for r in range(R):
        n = C
        if offset is not None:
            n = min(n, r % Tq + 1 + offset)
        if lengths is not None:
            n = min(n, max(int(lengths[r // per]), 0))
        out.append(n)
    return out


def lens_tensor(lengths, dev="cpu"):
    return None if lengths is None else torch.tensor([int(v) for v in lengths], dtype=torch.int32, device=dev)


def run_masked(dev, x, tab, q, mid, offset=None, lengths=None, row_pad=1, shift=()):
    """the masked op on `dev`: `offset` None or the causal offset, `lengths` None or a list / an int32 tensor"""
    ops = torch.ops.torchlsq
    x, = A.to(dev, (x,), shift)
    lt = lengths.to(dev) if isinstance(lengths, torch.Tensor) else lens_tensor(lengths, dev)
    mask = (offset is not None, 0 if offset is None else int(offset), lt)
    if q is None:
        return ops.lsq_softmax_mask_w8_q8(x, tab.to(dev), mid, *mask)
    return ops.lsq_softmax_mask_w8_q8_q(x, tab.to(dev), *A.to(dev, q), mid, *mask, row_pad)


def zero_of(q, mid):
    """the output side's own value of p = 0: the level of 0.0 by the existing levels op, or +0.0 of `mid`"""
    z = torch.zeros(1, dtype=mid)
    if q is None:
        return z
    lv = torch.ops.torchlsq.lsq_levels_per_tensor(z, *q, 0)
    return lv.view(U8) if max(q[3], q[5]) > 127 else lv


def composed(x, tab, q, mid, n):
    """the expected result from the EXISTING unmasked CPU op alone: rows with the same n go through it together on x[rows, :n]; the
    rest of every row is `zero_of`"""
    C = int(x.shape[-1])
    rows = x.reshape(-1, C)
    z = zero_of(q, mid)
    want = z.expand(rows.shape[0], C).clone()
    n = torch.tensor(n)
    for v in sorted(set(n.tolist())):
        if v == 0:
            continue
        pick = (n == v).nonzero().reshape(-1)
        want[pick, :v] = A.run_softmax("cpu", rows[pick][:, :v].contiguous(), tab, q, mid)
    return want.view(x.shape)


def same(got, want, note=""):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (note, got.dtype, want.dtype, got.shape, want.shape)
    assert torch.equal(A.bits(got.cpu().contiguous()), A.bits(want.contiguous())), note


def poisoned(x, n, how, seed=0):
    """x with the bytes at i >= n_r replaced: "max" the type's maximum, "random" random bytes"""
    C = int(x.shape[-1])
    rows = x.reshape(-1, C).clone()
    beyond = torch.arange(C).reshape(1, -1) >= torch.tensor(n).reshape(-1, 1)
    if how == "max":
        fill = torch.full_like(rows, 255 if x.dtype == U8 else 127)
    else:
        fill = A.levels(rows.shape, 900 + seed, x.dtype)
    return torch.where(beyond, fill, rows).view(x.shape)
