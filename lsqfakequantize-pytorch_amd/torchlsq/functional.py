"""torchlsq.functional -- the functional entry point of the LSQ / LSQ+ fake quantizer.

Drop-in for reference torchlsq/functional.py:8-97: same name, same argument list, defaults and
assertions; the work is done by `torch.ops.torchlsq.lsq` (registered in torchlsq/extension.py on top
of the gfx950 kernels).
"""
import torch
from torch.autograd.function import once_differentiable

from . import extension as _E
from .extension import _assert_has_ops
from ._w8_host_common import _act_constants

Tensor = torch.Tensor


class _LSQOnDevice(torch.autograd.Function):
    """Direct autograd binding of the gfx950 kernels for GPU tensors.

    Same computation as `torch.ops.torchlsq.lsq` (the registered ops stay available and are what the
    dispatcher-level tests exercise); this class only skips the dispatcher round trips -- two Python
    re-entries per op -- which dominate the cost of small layers.  Mirrors LSQPer*Function of the
    reference (csrc/ops/autograd/lsq_autograd.cpp:16-74,111-173): saves {input, scale, shift}, backward
    returns gradients for those three only, double backward is refused.
    """

    @staticmethod
    def forward(ctx, x, scale, shift, cfg):
        (qmin, qmax, tmin, tmax, axis, use_gs, gs, sym, per_channel, eval_mode, init_mode, mask_backward) = cfg
        # eval mode (plain fake-quantizer behaviour): the backward only needs "was the element strictly inside the
        # range", so the forward emits that as one byte per element and autograd keeps the mask instead of x (1 instead
        # of 4 bytes per fp32 element, and the backward reads 9 instead of 12 bytes per element).
        # The mask is that of the FORWARD's parameter values, whereas the reference recomputes it in its backward from
        # the saved (x, scale, shift) (lsq_autograd.cpp:46-73), i.e. from the parameter values AT BACKWARD TIME.  The two
        # differ only if scale / shift are overwritten in place (param.data.copy_, which autograd's version check does
        # not see) between this forward and its backward -- which is exactly what the observer-driven phase of
        # LSQFakeQuantizer does on every call (observers.py:417-420).  `mask_backward=False` (what the module passes
        # while its observer is enabled) keeps the reference's behaviour: x is saved and the eval backward runs on the
        # current parameters.  (The C++ host binding's LsqNode has the same switch.)
        masked = _E.saves_mask(eval_mode, init_mode, x.requires_grad, mask_backward)
        if per_channel:
            y = _E.hip_forward_per_channel(x, scale, shift, axis, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode,
                                           init_mode, want_mask=masked)
        else:
            y = _E.hip_forward_per_tensor(x, scale, shift, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode,
                                          want_mask=masked)
        ctx.masked = masked
        if masked:
            y, mask = y
            ctx.save_for_backward(mask, scale, shift)
        else:
            ctx.save_for_backward(x, scale, shift)
        ctx.cfg = cfg
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, scale, shift = ctx.saved_tensors
        (qmin, qmax, tmin, tmax, axis, use_gs, gs, sym, per_channel, eval_mode, init_mode, _) = ctx.cfg
        if ctx.masked:      # x is the inside mask here; d_scale = d_shift = 0 (lsq_kernel.h:142-144)
            return _E.hip_backward_from_mask(grad_out, x), torch.zeros_like(scale), torch.zeros_like(shift), None
        if per_channel:
            dx, ds, db = _E.hip_backward_per_channel(grad_out, x, scale, shift, axis, qmin, qmax, tmin, tmax, use_gs, gs,
                                                     sym, eval_mode, init_mode)
        else:
            dx, ds, db = _E.hip_backward_per_tensor(grad_out, x, scale, shift, qmin, qmax, tmin, tmax, use_gs, gs, sym,
                                                    eval_mode, init_mode)
        return dx, ds, db, None


class _LSQOnHost(torch.autograd.Function):
    """The same for tensors in host memory (liblsq_cpu.so, the counterpart of the reference's CPU dispatch key): straight to
    the kernels' host layer instead of through the dispatcher -- torch.library's Python autograd wrapper costs ~70 us per call
    (schema defaults, two re-entries), several times the kernel on a small tensor.  Mirrors lsq_autograd.cpp:16-74,111-173:
    saves {input, scale, shift}; the eval backward recomputes the mask from them (no mask variant here)."""

    @staticmethod
    def forward(ctx, x, scale, shift, cfg):
        (qmin, qmax, tmin, tmax, axis, use_gs, gs, sym, per_channel, eval_mode, init_mode, _) = cfg
        ctx.save_for_backward(x, scale, shift)
        ctx.cfg = cfg
        return _E.cpu_forward(x, scale, shift, axis, per_channel, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, scale, shift = ctx.saved_tensors
        (qmin, qmax, tmin, tmax, axis, use_gs, gs, sym, per_channel, eval_mode, init_mode, _) = ctx.cfg
        dx, ds, db = _E.cpu_backward(grad_out, x, scale, shift, axis, per_channel, qmin, qmax, tmin, tmax, use_gs, gs, sym,
                                     eval_mode, init_mode)
        return dx, ds, db, None


def lsq(x: Tensor, scale: Tensor, shift: Tensor,
        quant_min: int = 0,
        quant_max: int = 255,
        type_min: int = None,
        type_max: int = None,
        axis: int = 1,
        use_grad_scaling: bool = True,
        grad_scaler: float = 1.,
        is_affine: bool = True,
        is_perchannel: bool = False,
        eval_mode: bool = False,
        init_mode: bool = False, *,
        mask_backward: bool = True) -> Tensor:
    """Learned Step Size Quantization (LSQ+, arXiv:2004.09576) fake quantizer: quantize -> dequantize
    with `scale` and `shift` as learnable parameters.

    Forward (per element, reference csrc/ops/kernels/lsq_kernel.h:6-14)::

        s   = max(|scale|, eps)
        zp  = round(clamp(-shift / s, type_min, type_max))          # the integer zero point
        x_q = round(clamp(x / s + zp, quant_min, quant_max))        # round half to even
        x_r = (x_q - zp) * s

    Backward (lsq_kernel.h:94-123), with xq the *unrounded* clamped value::

        d x     = grad                       if quant_min < xq < quant_max else 0
        d scale = grad * (x_r - x) / s       inside;   grad * (quant_min|quant_max - zp) at the borders
        d shift = 0 inside (or if symmetric); grad at the borders

    `d scale` and `d shift` are summed over the tensor (per channel along `axis` when
    `is_perchannel`) and, when `use_grad_scaling`, multiplied by
    grad_scaler / sqrt(numel * quant_max [/ channels]) (arXiv:1902.08153).

    Args:
        x: input tensor (float32/float64; this build also takes bfloat16/float16 with fp32 parameters).
        scale, shift: 1-D tensors -- one element for per-tensor, one per channel otherwise
            (a single-element tensor is broadcast in the per-channel case).
        quant_min, quant_max: bounds of the quantized range (default 0..255).
        type_min, type_max: numeric limits of the quantized *type* used to clamp the zero point;
            default to quant_min / quant_max.
        axis: channel dimension of the per-channel scheme.
        use_grad_scaling, grad_scaler: gradient scaling of the parameters, see above.
        is_affine: asymmetric (True) or symmetric (False: no gradient for `shift`) quantization.
        is_perchannel: per-channel (True) or per-tensor (False).
        eval_mode: behave like a plain fake-quantizer (no parameter gradients).
        init_mode: parameter-initialisation phase: the forward is the identity and the parameter
            gradients are those of ||x_r - x||^2 (the upstream gradient is ignored for them).
        mask_backward (keyword only; this build, GPU tensors): in eval mode keep the forward's one-byte "inside the
            range" mask for the backward (default) instead of x.  False = the reference's behaviour to the letter: x is
            saved and the backward recomputes the mask from the parameters as they are THEN (lsq_autograd.cpp:46-73) --
            it only matters when scale / shift are overwritten in place between a forward and its backward.
    """
    _assert_has_ops()
    if not is_affine:
        assert quant_min <= 0 <= quant_max, 'quantization range must be covered 0 in symmetric quantization'
    if type_min is None:
        type_min = quant_min
    if type_max is None:
        type_max = quant_max
    on_gpu = x.is_cuda and scale.is_cuda and shift.is_cuda
    on_host = not (x.is_cuda or scale.is_cuda or shift.is_cuda) and x.device.type == "cpu"
    if (on_gpu or on_host) and not torch.jit.is_tracing() and not torch.compiler.is_compiling():
        # front-op checks and routing of quantops::ops::lsq (lsq.cpp:104-134), then straight to the kernels
        native = _E._NATIVE_LSQ if on_gpu else None
        if native is not None:      # C++ front op + autograd node (csrc/torch_binding): same kernels, less host time
            if not mask_backward:
                native = torch.ops.torchlsq_native.lsq_keep_input.default
            return native(x, scale, shift, quant_min, quant_max, type_min, type_max, axis, bool(use_grad_scaling),
                          float(grad_scaler), bool(is_affine), bool(is_perchannel), bool(eval_mode), bool(init_mode))
        if scale.dim() != 1:
            raise RuntimeError("scale should be a 1-D tensor, even in per tensor case(please, avoid torch.Scalar too)")
        if shift.dim() != 1:
            raise RuntimeError("shift should be a 1-D tensor, even in per tensor case(please, avoid torch.Scalar too)")
        if is_perchannel:
            size = max(scale.size(0), shift.size(0))
            if scale.size(0) != size:
                scale = scale.repeat(size)      # differentiable: a size-1 leaf receives the summed gradient
            if shift.size(0) != size:
                shift = shift.repeat(size)
        cfg = (quant_min, quant_max, type_min, type_max, axis, bool(use_grad_scaling), float(grad_scaler),
               not is_affine, bool(is_perchannel), bool(eval_mode), bool(init_mode), bool(mask_backward))
        return (_LSQOnDevice if on_gpu else _LSQOnHost).apply(x, scale, shift, cfg)
    return torch.ops.torchlsq.lsq(x, scale, shift, quant_min, quant_max, type_min, type_max,
                                  axis, use_grad_scaling, grad_scaler, is_affine, is_perchannel,
                                  eval_mode, init_mode)


def lsq_quantize(x: Tensor, scale: Tensor, shift: Tensor,
                 quant_min: int = 0,
                 quant_max: int = 255,
                 type_min: int = None,
                 type_max: int = None,
                 axis: int = 1,
                 is_perchannel: bool = False,
                 dtype=torch.quint8) -> Tensor:
    """The REAL quantized tensor behind `lsq`'s fake-quantized output (an addition of this build): a `torch.quint8` /
    `torch.qint8` tensor whose integer representation holds the levels x_q of the forward (lsq_kernel.h:13) and whose
    quantizer carries s = max(|scale|, eps) and the integer zero point zp = round(clamp(-shift / s, type_min, type_max)) the
    kernels use -- so for FLOAT32 x `lsq_quantize(...).dequantize()` equals `lsq(...)` bit for bit ((x_q - zp) * s, the same
    two fp32 operations; torch's quantizer dequantizes in fp32, so a float64 x agrees only to fp32 precision and a 16-bit x
    gets fp32 where `lsq` returns the value rounded to 16 bits -- the integer levels are the forward's in every case).  The
    per-tensor form reads scale / zero point back to the host once per call (torch's per-tensor quantizer holds host numbers):
    a conversion-time function, not one for a training loop.  One pass that reads x and writes ONE byte per element (no
    fake-quantized output: 5 instead of 9 bytes per fp32 element on the GPU).  The step after the path: reference quantized/modules/observers.py:378-422 hands scale and
    zero_point to torch's converter, which quantizes again with its own rounding; here the trained quantizer emits them.
    """
    _assert_has_ops()
    assert dtype in (torch.quint8, torch.qint8), "dtype must be torch.quint8 or torch.qint8"
    type_min = quant_min if type_min is None else type_min
    type_max = quant_max if type_max is None else type_max
    lo, hi = (0, 255) if dtype == torch.quint8 else (-128, 127)
    assert lo <= quant_min <= quant_max <= hi, "the quantized range must fit the quantized type"
    if scale.dim() != 1 or shift.dim() != 1:
        raise RuntimeError("scale and shift should be 1-D tensors, even in per tensor case(please, avoid torch.Scalar too)")
    x, scale, shift = x.detach(), scale.detach(), shift.detach()
    if is_perchannel:
        size = max(scale.size(0), shift.size(0))
        scale = scale if scale.size(0) == size else scale.repeat(size)
        shift = shift if shift.size(0) == size else shift.repeat(size)
        levels = torch.ops.torchlsq.lsq_levels_per_channel(x, scale, shift, axis, quant_min, quant_max, type_min, type_max, 0)
    else:
        levels = torch.ops.torchlsq.lsq_levels_per_tensor(x, scale, shift, quant_min, quant_max, type_min, type_max, 0)
    # the quantizer's constants exactly as the kernels derive them (lsq_cpu.cpp:44-47 / lsq_kernel.h:157-158,12): |scale|
    # floored at eps, the zero point from -shift * (1 / s), clamped to the type's range, rounded half to even
    s = scale.abs().clamp_min(torch.finfo(scale.dtype).eps)
    zp = torch.fmin(torch.full_like(s, type_max), torch.fmax(torch.full_like(s, type_min), -shift * (1.0 / s))).round()
    int_repr = levels.view(torch.uint8) if dtype == torch.quint8 else levels        # the byte is q mod 256 either way
    if is_perchannel:
        return torch._make_per_channel_quantized_tensor(int_repr, s.to(torch.float64), zp.to(torch.int64), axis)
    s0, zp0 = torch.stack([s[0].double(), zp[0].double()]).tolist()          # the quantizer wants host numbers: ONE read-back
    return torch._make_per_tensor_quantized_tensor(int_repr, s0, int(zp0))


class _LSQForeach(torch.autograd.Function):
    """N per-channel quantizers as ONE autograd node over the multi-tensor kernels (lsq_hip_*_per_channel_multi): one launch
    per 32 tensors each way instead of N.  Same arithmetic and summation order as N `lsq` calls (bit-identical outputs and
    gradients); saves {x_i, scale_i, shift_i} like the reference's nodes (lsq_autograd.cpp:111-173)."""

    @staticmethod
    def forward(ctx, cfg, n, *tensors):
        xs, scales, shifts = tensors[:n], tensors[n:2 * n], tensors[2 * n:]
        (qmin, qmax, tmin, tmax, axes, use_gs, gs, sym, eval_mode, init_mode) = cfg
        ys = _E.hip_forward_per_channel_multi(xs, scales, shifts, axes, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode,
                                              init_mode)
        ctx.save_for_backward(*tensors)
        ctx.cfg, ctx.n = cfg, n
        ctx.set_materialize_grads(False)        # an unused output arrives as None in backward, not as a zero tensor
        return tuple(ys)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_outs):
        n = ctx.n
        tensors = ctx.saved_tensors
        xs, scales, shifts = tensors[:n], tensors[n:2 * n], tensors[2 * n:]
        (qmin, qmax, tmin, tmax, axes, use_gs, gs, sym, eval_mode, init_mode) = ctx.cfg
        # an output nobody used has no gradient: its tensor takes no part in the launch and gets NO gradients, exactly what N
        # separate lsq calls give it (with init_mode the parameter gradients ignore the upstream gradient, lsq_kernel.h:116: a
        # zero-filled stand-in would invent d_scale / d_shift for it)
        live = [i for i in range(n) if grad_outs[i] is not None]
        dxs, dss, dbs = [None] * n, [None] * n, [None] * n
        if live:
            outs = _E.hip_backward_per_channel_multi([grad_outs[i] for i in live], [xs[i] for i in live], [scales[i] for i in live],
                                                     [shifts[i] for i in live], [axes[i] for i in live], qmin, qmax, tmin, tmax,
                                                     use_gs, gs, sym, eval_mode, init_mode)
            for i, o in zip(live, outs):
                dxs[i], dss[i], dbs[i] = o
        return (None, None) + tuple(dxs) + tuple(dss) + tuple(dbs)


def lsq_foreach(xs, scales, shifts,
                quant_min: int = 0,
                quant_max: int = 255,
                type_min: int = None,
                type_max: int = None,
                axis=0,
                use_grad_scaling: bool = True,
                grad_scaler: float = 1.,
                is_affine: bool = True,
                eval_mode: bool = False,
                init_mode: bool = False):
    """`lsq(x_i, scale_i, shift_i, ..., is_perchannel=True)` for every i, horizontally fused (an addition of this build).

    The per-channel quantizers of many tensors -- typically all conv / linear weights of a QAT model, each a few MB and
    launch-latency-bound on its own -- run in ONE launch per 32 tensors each way.  `axis` is one int or one per tensor; all
    other arguments are shared and mean what they mean in `lsq`.  Returns the list of outputs; gradients reach every x_i,
    scale_i, shift_i exactly as through N separate `lsq` calls (bit-identical).  Tensors the multi-tensor kernels do not take
    (CPU tensors, channel rows too short or unaligned, tensors so small or so large that the single-tensor policy splits their
    channels differently: `torchlsq.extension.hip_multi_eligible`) silently go through `lsq` one by one.
    """
    _assert_has_ops()
    n = len(xs)
    assert len(scales) == n and len(shifts) == n, "xs, scales and shifts must have the same length"
    if not is_affine:
        assert quant_min <= 0 <= quant_max, 'quantization range must be covered 0 in symmetric quantization'
    type_min = quant_min if type_min is None else type_min
    type_max = quant_max if type_max is None else type_max
    axes = [int(axis)] * n if isinstance(axis, int) else [int(a) for a in axis]
    assert len(axes) == n
    fusable = not torch.jit.is_tracing() and not torch.compiler.is_compiling()
    all_gpu = all(x.is_cuda and sc.is_cuda and sh.is_cuda for x, sc, sh in zip(xs, scales, shifts))
    if fusable and n > 1 and _E._NATIVE_LSQ is not None and all_gpu:     # (a list with CPU entries: the Python partition below)
        # C++ host layer: the partition into fused / single tensors, the checks and the one autograd node all happen there
        # (a table row and an output allocation of host time per tensor instead of a Python call chain)
        return list(torch.ops.torchlsq_native.lsq_foreach(list(xs), list(scales), list(shifts), axes, quant_min, quant_max,
                                                          type_min, type_max, bool(use_grad_scaling), float(grad_scaler),
                                                          bool(is_affine), bool(eval_mode), bool(init_mode)))
    out = [None] * n
    groups = {}
    for i in range(n):
        x, sc, sh = xs[i], scales[i], shifts[i]
        if (fusable and x.is_cuda and sc.is_cuda and sh.is_cuda and sc.dim() == 1 and sh.dim() == 1
                and _E.hip_multi_eligible(x, axes[i])):
            groups.setdefault((x.device, x.dtype), []).append(i)
        else:
            out[i] = lsq(x, sc, sh, quant_min, quant_max, type_min, type_max, axes[i], use_grad_scaling, grad_scaler, is_affine,
                         True, eval_mode, init_mode)
    for idx in groups.values():
        if len(idx) == 1:       # nothing to fuse
            i = idx[0]
            out[i] = lsq(xs[i], scales[i], shifts[i], quant_min, quant_max, type_min, type_max, axes[i], use_grad_scaling,
                         grad_scaler, is_affine, True, eval_mode, init_mode)
            continue
        sc_l, sh_l = [], []
        for i in idx:       # front-op rule (lsq.cpp:124-126): a size-1 parameter is repeated up to the other's size
            sc, sh = scales[i], shifts[i]
            size = max(sc.size(0), sh.size(0))
            sc_l.append(sc if sc.size(0) == size else sc.repeat(size))
            sh_l.append(sh if sh.size(0) == size else sh.repeat(size))
        cfg = (quant_min, quant_max, type_min, type_max, tuple(axes[i] for i in idx), bool(use_grad_scaling), float(grad_scaler),
               not is_affine, bool(eval_mode), bool(init_mode))
        ys = _LSQForeach.apply(cfg, len(idx), *[xs[i] for i in idx], *sc_l, *sh_l)
        for i, y in zip(idx, ys):
            out[i] = y
    return out


class _LSQGroupOnDevice(torch.autograd.Function):
    """`lsq_per_group` for GPU tensors straight to liblsq_hip_group.so (as _LSQOnDevice does for `lsq`): saves
    {input, scale, shift}, or -- eval mode -- the forward's one-byte inside mask, whose backward is lsq_hip_backward_from_mask."""

    @staticmethod
    def forward(ctx, x, scale, shift, cfg):
        (group_size, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode) = cfg
        masked = _E.saves_mask(eval_mode, init_mode, x.requires_grad, True)
        y = _E.group_forward(x, scale, shift, group_size, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode,
                             want_mask=masked)
        ctx.masked = masked
        if masked:
            y, mask = y
            ctx.save_for_backward(mask, scale, shift)
        else:
            ctx.save_for_backward(x, scale, shift)
        ctx.cfg = cfg
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, scale, shift = ctx.saved_tensors
        if ctx.masked:      # x is the inside mask here; d_scale = d_shift = 0 (lsq_kernel.h:142-144)
            return _E.hip_backward_from_mask(grad_out, x), torch.zeros_like(scale), torch.zeros_like(shift), None
        dx, ds, db = _E.group_backward(grad_out, x, scale, shift, *ctx.cfg)
        return dx, ds, db, None


def _group_params(x, scale, shift, group_size):
    """the front-op rule (lsq.cpp:124-126) for groups: a parameter of numel 1 is repeated once per group (differentiably)"""
    groups = x.numel() // group_size if group_size > 0 else 0
    if scale.numel() == 1 and groups != 1:
        scale = scale.reshape(1).repeat(groups)
    if shift.numel() == 1 and groups != 1:
        shift = shift.reshape(1).repeat(groups)
    return scale, shift


def lsq_per_group(x: Tensor, scale: Tensor, shift: Tensor, group_size: int,
                  quant_min: int = 0,
                  quant_max: int = 255,
                  type_min: int = None,
                  type_max: int = None,
                  use_grad_scaling: bool = True,
                  grad_scaler: float = 1.,
                  is_affine: bool = True,
                  eval_mode: bool = False,
                  init_mode: bool = False) -> Tensor:
    """Group-wise LSQ (an addition of this build): one learned `scale` / `shift` per run of `group_size` (G) consecutive
    elements of the last dimension -- the scheme of low-bit transformer weights (e.g. W4 with G = 128).

    Group j is `x.reshape(-1, G)[j]`; x.shape[-1] must be a multiple of G.  `scale` / `shift` are documented with the shape
    `x.shape[:-1] + (x.shape[-1] // G,)`, but any shape with x.numel() // G elements is taken (a one-element parameter is
    repeated), and their gradients come back in their own shapes.  By definition the result -- y, dx, d_scale, d_shift, in
    every mode -- is that of

        lsq(x.reshape(-1, G), scale.reshape(-1), shift.reshape(-1), ..., axis=0, is_perchannel=True).reshape(x.shape)

    including the per-channel gradient scaler 1 / sqrt(G * quant_max); the other arguments mean what they mean in `lsq`.
    GPU tensors run the group kernels of liblsq_hip_group.so (one launch each way, no workspace), CPU tensors the
    per-channel CPU kernels on that view.
    """
    _assert_has_ops()
    if not is_affine:
        assert quant_min <= 0 <= quant_max, 'quantization range must be covered 0 in symmetric quantization'
    type_min = quant_min if type_min is None else type_min
    type_max = quant_max if type_max is None else type_max
    group_size = int(group_size)
    scale, shift = _group_params(x, scale, shift, group_size)
    on_gpu = x.is_cuda and scale.is_cuda and shift.is_cuda
    if on_gpu and not torch.jit.is_tracing() and not torch.compiler.is_compiling():
        _E.check_group_args(x, scale, shift, group_size)
        cfg = (group_size, quant_min, quant_max, type_min, type_max, bool(use_grad_scaling), float(grad_scaler),
               not is_affine, bool(eval_mode), bool(init_mode))
        return _LSQGroupOnDevice.apply(x, scale, shift, cfg)
    return torch.ops.torchlsq.lsq_forward_per_group(x, scale, shift, group_size, quant_min, quant_max, type_min, type_max,
                                                    bool(use_grad_scaling), float(grad_scaler), not is_affine,
                                                    bool(eval_mode), bool(init_mode))


def lsq_levels_per_group(x: Tensor, scale: Tensor, shift: Tensor, group_size: int,
                         quant_min: int = 0,
                         quant_max: int = 255,
                         type_min: int = None,
                         type_max: int = None,
                         dtype=torch.quint8) -> Tensor:
    """The integer levels x_q of `lsq_per_group`'s forward, one byte per element in x's shape: torch.uint8 for
    dtype=torch.quint8, torch.int8 for torch.qint8 (torch has no per-group quantized tensor; the constants that go with
    them are s = max(|scale|, eps) and zp = round(clamp(-shift * (1 / s), type_min, type_max)) per group, so that
    (x_q - zp) * s is `lsq_per_group`'s output -- bit for bit for float32 x).  One pass, one byte written per element."""
    _assert_has_ops()
    assert dtype in (torch.quint8, torch.qint8), "dtype must be torch.quint8 or torch.qint8"
    type_min = quant_min if type_min is None else type_min
    type_max = quant_max if type_max is None else type_max
    lo, hi = (0, 255) if dtype == torch.quint8 else (-128, 127)
    assert lo <= quant_min <= quant_max <= hi, "the quantized range must fit the quantized type"
    group_size = int(group_size)
    x, scale, shift = x.detach(), scale.detach(), shift.detach()
    scale, shift = _group_params(x, scale, shift, group_size)
    levels = torch.ops.torchlsq.lsq_levels_per_group(x, scale, shift, group_size, quant_min, quant_max, type_min, type_max, 0)
    return levels.view(torch.uint8) if dtype == torch.quint8 else levels


class _LSQGroupForeach(torch.autograd.Function):
    """N group-wise quantizers of one dtype as ONE autograd node over the multi-tensor group kernels (the fused calls of
    liblsq_hip_group.so): one launch per reduction class and per 28 tensors each way instead of N.  Every tensor is walked
    by the workgroups of its own single call, so outputs and gradients carry the same bits as N `lsq_per_group` calls.
    Saves {x_i, scale_i, shift_i}, as _LSQForeach does."""

    @staticmethod
    def forward(ctx, cfg, n, *tensors):
        xs, scales, shifts = tensors[:n], tensors[n:2 * n], tensors[2 * n:]
        (group_sizes, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode) = cfg
        ys = _E.group_forward_multi(xs, scales, shifts, group_sizes, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode,
                                    init_mode)
        ctx.save_for_backward(*tensors)
        ctx.cfg, ctx.n = cfg, n
        ctx.set_materialize_grads(False)        # an unused output arrives as None in backward, not as a zero tensor
        return tuple(ys)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_outs):
        n = ctx.n
        tensors = ctx.saved_tensors
        xs, scales, shifts = tensors[:n], tensors[n:2 * n], tensors[2 * n:]
        (group_sizes, qmin, qmax, tmin, tmax, use_gs, gs, sym, eval_mode, init_mode) = ctx.cfg
        # an output nobody used gets no gradients, as in _LSQForeach (with init_mode a zero-filled stand-in would invent
        # d_scale / d_shift for it)
        live = [i for i in range(n) if grad_outs[i] is not None]
        dxs, dss, dbs = [None] * n, [None] * n, [None] * n
        if live:
            outs = _E.group_backward_multi([grad_outs[i] for i in live], [xs[i] for i in live], [scales[i] for i in live],
                                           [shifts[i] for i in live], [group_sizes[i] for i in live], qmin, qmax, tmin, tmax,
                                           use_gs, gs, sym, eval_mode, init_mode)
            for i, o in zip(live, outs):
                dxs[i], dss[i], dbs[i] = o
        return (None, None) + tuple(dxs) + tuple(dss) + tuple(dbs)


def lsq_foreach_per_group(xs, scales, shifts, group_size,
                          quant_min: int = 0,
                          quant_max: int = 255,
                          type_min: int = None,
                          type_max: int = None,
                          use_grad_scaling: bool = True,
                          grad_scaler: float = 1.,
                          is_affine: bool = True,
                          eval_mode: bool = False,
                          init_mode: bool = False):
    """`lsq_per_group(x_i, scale_i, shift_i, G_i, ...)` for every i, horizontally fused (an addition of this build).

    The group-wise quantizers of many tensors -- typically all weights of a QAT model with W4 g128-style scales, most of
    them too small to fill the GPU on their own -- run in one launch each way per reduction class and per 28 tensors:
    one launch each way in the common case of one G that is a multiple of the 16-byte packet.  `group_size` is one int or
    one per tensor; all other arguments are shared and mean what they mean in `lsq_per_group` (a one-element parameter is
    repeated once per group, gradients come back in the parameters' own shapes).  Returns the list of outputs; outputs
    and gradients are bit-identical to N separate `lsq_per_group` calls.  CPU tensors, empty tensors, calls under tracing
    or torch.compile, and a dtype with a single GPU tensor go through `lsq_per_group` one by one.
    """
    _assert_has_ops()
    n = len(xs)
    assert len(scales) == n and len(shifts) == n, "xs, scales and shifts must have the same length"
    if not is_affine:
        assert quant_min <= 0 <= quant_max, 'quantization range must be covered 0 in symmetric quantization'
    type_min = quant_min if type_min is None else type_min
    type_max = quant_max if type_max is None else type_max
    sizes = [int(group_size)] * n if isinstance(group_size, int) else [int(g) for g in group_size]
    assert len(sizes) == n, "group_size must be one int or one per tensor"
    fusable = not torch.jit.is_tracing() and not torch.compiler.is_compiling()
    out = [None] * n
    classes = {}
    for i in range(n):
        x, sc, sh = xs[i], scales[i], shifts[i]
        if fusable and x.is_cuda and sc.is_cuda and sh.is_cuda and x.numel() > 0:
            classes.setdefault((x.device, x.dtype), []).append(i)
        else:
            out[i] = lsq_per_group(x, sc, sh, sizes[i], quant_min, quant_max, type_min, type_max, use_grad_scaling,
                                   grad_scaler, is_affine, eval_mode, init_mode)
    for idx in classes.values():
        if len(idx) == 1:       # nothing to fuse
            i = idx[0]
            out[i] = lsq_per_group(xs[i], scales[i], shifts[i], sizes[i], quant_min, quant_max, type_min, type_max,
                                   use_grad_scaling, grad_scaler, is_affine, eval_mode, init_mode)
            continue
        sc_l, sh_l = [], []
        for i in idx:
            sc, sh = _group_params(xs[i], scales[i], shifts[i], sizes[i])
            _E.check_group_args(xs[i], sc, sh, sizes[i])
            sc_l.append(sc)
            sh_l.append(sh)
        cfg = (tuple(sizes[i] for i in idx), quant_min, quant_max, type_min, type_max, bool(use_grad_scaling),
               float(grad_scaler), not is_affine, bool(eval_mode), bool(init_mode))
        ys = _LSQGroupForeach.apply(cfg, len(idx), *[xs[i] for i in idx], *sc_l, *sh_l)
        for i, y in zip(idx, ys):
            out[i] = y
    return out


class PackedGroupTensor:
    """A group-wise quantized weight in its deployment format (torch has no per-group quantized tensor; the layout is the
    contract of include/lsq_hip_pack.h):

        codes       uint8, shape[:-1] + (shape[-1] * bits / 8,): `bits`-bit codes (level - quant_min), little-endian inside
                    the byte -- for 4 bits, element 0 is the low nibble
        scale       max(|scale|, eps) per group (float32; float64 for a float64 weight)
        zero_point  int32 per group, in code units (the forward's zero point minus quant_min)
        bits, group_size, quant_min, shape

    `dequantize(dtype)` is `(code - zero_point) * scale`: for the storage type the weight was packed from, the output of
    `lsq_per_group` bit for bit, except that codes do not carry the sign of a zero (see `lsq_pack_per_group`).  `levels()` are the bytes of `lsq_levels_per_group`."""

    def __init__(self, codes, scale, zero_point, bits, group_size, quant_min, shape):
        self.codes, self.scale, self.zero_point = codes, scale, zero_point
        self.bits, self.group_size, self.quant_min = int(bits), int(group_size), int(quant_min)
        self.shape = torch.Size(shape)

    def dequantize(self, dtype=None) -> Tensor:
        """the fake-quantized weight in `dtype` (default: the scale's dtype), in the original shape"""
        dtype = self.scale.dtype if dtype is None else dtype
        return lsq_dequantize_per_group(self.codes, self.scale, self.zero_point, self.group_size, self.bits, dtype).reshape(self.shape)

    def levels(self, dtype=torch.qint8) -> Tensor:
        """the integer levels, one byte per element in the original shape: torch.int8 for torch.qint8, torch.uint8 for
        torch.quint8 (as `lsq_levels_per_group`)"""
        return lsq_unpack_per_group(self.codes, self.bits, self.quant_min, dtype).reshape(self.shape)

    def linear(self, x: Tensor, bias: Tensor = None) -> Tensor:
        """`x @ dequantize().T (+ bias)` computed from the codes (`lsq_linear_packed`): no dequantized weight is written"""
        return lsq_linear_packed(x, self, bias)

    def linear_a8(self, x: Tensor, bias: Tensor = None, scale: Tensor = None, shift: Tensor = None, quant_min: int = None,
                  quant_max: int = None, type_min: int = None, type_max: int = None, out_dtype=None) -> Tensor:
        """the same layer on the 8-bit levels of a per-tensor activation quantizer, summed in integers (`lsq_linear_packed_a8`)"""
        return lsq_linear_packed_a8(x, self, bias, scale, shift, quant_min, quant_max, type_min, type_max, out_dtype)

    def state(self):
        """a plain dict of tensors and ints, for torch.save / a checkpoint; `from_state` is the way back"""
        return dict(codes=self.codes, scale=self.scale, zero_point=self.zero_point, bits=self.bits, group_size=self.group_size,
                    quant_min=self.quant_min, shape=list(self.shape))

    @classmethod
    def from_state(cls, state):
        return cls(state["codes"], state["scale"], state["zero_point"], state["bits"], state["group_size"], state["quant_min"],
                   state["shape"])

    def __repr__(self):
        return "PackedGroupTensor(shape=%s, bits=%d, group_size=%d, quant_min=%d, device=%s)" % (
            tuple(self.shape), self.bits, self.group_size, self.quant_min, self.codes.device)


def lsq_pack_per_group(x: Tensor, scale: Tensor, shift: Tensor, group_size: int, bits: int,
                       quant_min: int, quant_max: int,
                       type_min: int = None,
                       type_max: int = None) -> PackedGroupTensor:
    """`x` under the group-wise quantizer (`scale`, `shift`, G = `group_size`: the arguments of `lsq_per_group`) as packed
    `bits`-bit codes (4 or 2; quant_max - quant_min must fit, and G must be a multiple of 8 / bits): one pass over x that
    writes bits / 8 bytes per element and the per-group constants.  The codes are the levels of `lsq_per_group`'s forward,
    so `lsq_pack_per_group(...).dequantize(x.dtype)` equals `lsq_per_group(...)` as numbers, and bit for bit iff quant_min >= 0
    or no group's zero point is +0.0.  Codes cannot carry the sign of a zero: with quant_min < 0 and a zero point of +0.0 --
    -shift / scale in [+0.0, 0.5], which includes shift = -0.0 -- the forward gives -0.0 for positions in [-0.5, 0) and
    dequantize gives +0.0.  A shift of +0.0 (zero point -0.0) or a non-zero integer zero point is bit-safe
    (include/lsq_hip_pack.h)."""
    _assert_has_ops()
    type_min = quant_min if type_min is None else type_min
    type_max = quant_max if type_max is None else type_max
    group_size = int(group_size)
    x, scale, shift = x.detach(), scale.detach(), shift.detach()
    scale, shift = _group_params(x, scale, shift, group_size)
    codes, qscale, qzero = torch.ops.torchlsq.lsq_pack_per_group(x, scale, shift, group_size, int(bits), quant_min, quant_max,
                                                                 type_min, type_max)
    return PackedGroupTensor(codes, qscale, qzero, bits, group_size, quant_min, x.shape)


def lsq_dequantize_per_group(codes: Tensor, scale: Tensor, zero_point: Tensor, group_size: int, bits: int,
                             dtype=torch.float32) -> Tensor:
    """The fake-quantized values behind packed codes (`PackedGroupTensor.dequantize`): (code - zero_point) * scale per
    group of `group_size` elements, as `dtype`, in the shape codes.shape[:-1] + (codes.shape[-1] * 8 / bits,)."""
    _assert_has_ops()
    return torch.ops.torchlsq.lsq_dequantize_per_group(codes, scale, zero_point, int(group_size), int(bits), dtype)


def lsq_unpack_per_group(codes: Tensor, bits: int, quant_min: int, dtype=torch.qint8) -> Tensor:
    """The integer levels behind packed codes, one byte per element (`PackedGroupTensor.levels`): torch.int8 for
    dtype=torch.qint8, torch.uint8 for torch.quint8 -- the bytes of `lsq_levels_per_group`."""
    _assert_has_ops()
    assert dtype in (torch.quint8, torch.qint8), "dtype must be torch.quint8 or torch.qint8"
    lo, hi = (0, 255) if dtype == torch.quint8 else (-128, 127)
    assert lo <= quant_min and quant_min + 2 ** int(bits) - 1 <= hi, "the quantized range must fit the quantized type"
    levels = torch.ops.torchlsq.lsq_unpack_per_group(codes, int(bits), int(quant_min), 0)
    return levels.view(torch.uint8) if dtype == torch.quint8 else levels


def lsq_linear_packed(x: Tensor, packed: PackedGroupTensor, bias: Tensor = None) -> Tensor:
    """A linear layer on a packed group-wise weight: `y[..., n] = sum_k x[..., k] * w[n, k] (+ bias[n])` with
    `w = (code - zero_point) * scale` read straight from the 4- / 2-bit codes of `packed` (a 2-D weight [N, K], or any shape
    viewed as [shape[0], numel / shape[0]] like the group-wise quantizer does).  x is bfloat16, float16 or float32; y has its
    dtype.  Accumulation in float32, the bias (float32 or x's dtype) added in float32 before the one rounding; no atomics,
    repeated calls are bit-identical.  On the GPU up to 16 rows of x (the product of its leading dims) run the native kernel
    of liblsq_hip_qlinear.so -- the weight is streamed once, and row m of the result is bit for bit the 1-row call on x[m];
    more rows (prefill) of bfloat16 / float16 x run the matrix-core GEMM of liblsq_hip_qgemm.so on the codes -- no dequantized
    copy of the weight, and a row's bits do not depend on the other rows or on its place among them, though they are not the
    16-row kernel's bits (another order of the same sum).  Float32 x beyond 16 rows, a group size that is no multiple of
    128 / bits, and codes that are not 16-byte aligned dequantize into a float32 temporary and call
    `torch.nn.functional.linear` in float32, which meets the same accuracy bound but not that invariance.  Inference only: an x that requires grad under enabled grad mode raises."""
    _assert_has_ops()
    codes = packed.codes.reshape(packed.shape[0], -1) if packed.codes.dim() != 2 else packed.codes
    groups = codes.size(0) * codes.size(1) * (8 // packed.bits) // packed.group_size
    return torch.ops.torchlsq.lsq_linear_packed(x, codes, packed.scale.reshape(groups), packed.zero_point.reshape(groups), bias,
                                                packed.group_size, packed.bits)


def lsq_linear_packed_a8(x: Tensor, packed: PackedGroupTensor, bias: Tensor = None, scale: Tensor = None, shift: Tensor = None,
                         quant_min: int = None, quant_max: int = None, type_min: int = None, type_max: int = None,
                         out_dtype=None) -> Tensor:
    """`lsq_linear_packed` on QUANTIZED activations (W4A8 / W2A8): with lx the 8-bit level of an activation, zx its zero point
    and s_x its scale, `y[..., n] = s_x * sum_g scale[n, g] * I[..., n, g] (+ bias[n])` where
    `I = sum_{k in g} (lx[k] - zx) * (code[n, k] - zero_point[n, g])` is an exact integer, converted to float32 once per group.

    * floating x (bfloat16, float16 or float32) with the per-tensor quantizer's `scale` and `shift` (float32 tensors of one
      value), `quant_min`, `quant_max` and optionally the type's range: the levels are those of
      `lsq(x, scale, shift, ...)` -- formed inside the kernel on the GPU, no quantized copy of x is written -- and y has x's
      dtype.  Equal, bit for bit, to the second form on `lsq_levels_per_tensor`'s bytes.
    * a per-tensor `torch.quint8` / `torch.qint8` tensor as x (e.g. `m.quantize(x)`) with `out_dtype` (default float32): its
      `int_repr()`, `q_scale()` and `q_zero_point()` are used; scale, shift and the range arguments are ignored.

    No atomics; repeated calls are bit-identical; on the GPU up to 16 rows run the native kernel of
    liblsq_hip_qlinear_a8.so and row m of the result is bit for bit the 1-row call.  More rows take the same kernel 16 at
    a time, one launch per block of rows: the same bits, the weight streamed once per block.  Inference only."""
    _assert_has_ops()
    codes = packed.codes.reshape(packed.shape[0], -1) if packed.codes.dim() != 2 else packed.codes
    groups = codes.size(0) * codes.size(1) * (8 // packed.bits) // packed.group_size
    w = (codes, packed.scale.reshape(groups), packed.zero_point.reshape(groups), bias, packed.group_size, packed.bits)
    if x.is_quantized:
        assert x.qscheme() in (torch.per_tensor_affine, torch.per_tensor_symmetric) and x.dtype in (torch.quint8, torch.qint8), \
            "lsq_linear_packed_a8 needs a per-tensor torch.quint8 / torch.qint8 tensor"
        s_x = torch.tensor([x.q_scale()], dtype=torch.float32, device=x.device)
        zx = torch.tensor([x.q_zero_point()], dtype=torch.int32, device=x.device)
        return torch.ops.torchlsq.lsq_linear_packed_q8(x.int_repr(), s_x, zx, *w, torch.float32 if out_dtype is None else out_dtype)
    assert scale is not None and shift is not None and quant_min is not None and quant_max is not None, \
        "lsq_linear_packed_a8 on a floating x needs the activation quantizer's scale, shift, quant_min and quant_max"
    assert out_dtype is None or out_dtype == x.dtype, "a floating x gives y of x's dtype"
    type_min = quant_min if type_min is None else type_min
    type_max = quant_max if type_max is None else type_max
    return torch.ops.torchlsq.lsq_linear_packed_a8(x, scale, shift, int(quant_min), int(quant_max), int(type_min), int(type_max), *w)


def w8_weight_operands(weight_q: Tensor):
    """(levels [N, K] int8 / uint8, scale [N] float32, zero point [N] int32) of a 2-D per-channel (axis 0) or per-tensor
    `torch.qint8` / `torch.quint8` weight, e.g. `LSQFakeQuantizer.quantize(w)`: what `lsq_linear_w8_q8` / `_a8` take.  A
    per-tensor quantizer's one pair is repeated N times.  Nothing is read back from the device.  A 4-D conv weight
    [Cout, Cin, kh, kw] gives its 4-D levels and the same two vectors: what `lsq_conv2d_w8_q8` / `_a8` take."""
    if weight_q.is_quantized and weight_q.dtype in (torch.qint8, torch.quint8) and weight_q.dim() == 4:
        what = "lsq_conv2d_w8a8"        # a conv weight [Cout, Cin, kh, kw]: the same three operands, the levels 4-D
    else:
        what = "lsq_linear_w8a8"
        assert weight_q.is_quantized and weight_q.dtype in (torch.qint8, torch.quint8) and weight_q.dim() == 2, \
            "lsq_linear_w8a8 needs a 2-D torch.qint8 / torch.quint8 weight [out_features, in_features]"
    levels = weight_q.int_repr()
    N = levels.size(0)
    if weight_q.qscheme() in (torch.per_channel_affine, torch.per_channel_symmetric):
        assert weight_q.q_per_channel_axis() == 0, "%s needs a weight quantized per output row (axis 0)" % what
        scale = weight_q.q_per_channel_scales().to(torch.float32)
        zero = weight_q.q_per_channel_zero_points().to(torch.int32)
    else:
        assert weight_q.qscheme() in (torch.per_tensor_affine, torch.per_tensor_symmetric), \
            "%s needs a per-channel or per-tensor quantized weight" % what
        scale = torch.full((N,), weight_q.q_scale(), dtype=torch.float32, device=levels.device)
        zero = torch.full((N,), weight_q.q_zero_point(), dtype=torch.int32, device=levels.device)
    return levels, scale, zero


def lsq_linear_w8a8(x: Tensor, weight_q: Tensor, bias: Tensor = None, scale: Tensor = None, shift: Tensor = None,
                    quant_min: int = None, quant_max: int = None, type_min: int = None, type_max: int = None,
                    out_dtype=None) -> Tensor:
    """A linear layer on 8-bit activations and an 8-bit weight (W8A8), summed in integers: with lx the level of an activation,
    zx its zero point and s_x its scale, lw the level of a weight and (s_w[n], zw[n]) the scale and zero point of output row n,
    `y[..., n] = ((s_w[n] * float(I)) * s_x) + bias[n]` where `I = sum_k (lx[k] - zx) * (lw[n, k] - zw[n])` is an exact integer
    over all of K, converted to float32 once.

    `weight_q` is the 2-D per-channel (axis 0) or per-tensor `torch.qint8` / `torch.quint8` tensor that
    `LSQFakeQuantizer.quantize(w)` / `lsq_quantize` return.

    * floating x (bfloat16, float16 or float32) with the per-tensor activation quantizer's `scale` and `shift` (float32 tensors
      of one value), `quant_min`, `quant_max` and optionally the type's range: the levels are those of `lsq(x, scale, shift,
      ...)` and y has x's dtype.  Equal, bit for bit, to the second form on `lsq_levels_per_tensor`'s bytes.
    * a per-tensor `torch.quint8` / `torch.qint8` tensor as x (e.g. `m.quantize(x)`) with `out_dtype` (default float32): its
      `int_repr()`, `q_scale()` and `q_zero_point()` are used; scale, shift and the range arguments are ignored.

    No atomics; repeated calls are bit-identical; a row's bits do not depend on the number of rows or on its position; the
    GPU result (liblsq_hip_qlinear_w8.so, int8 matrix cores, any number of rows in one call) equals the CPU result bit for
    bit.  Inference only."""
    _assert_has_ops()
    w = w8_weight_operands(weight_q) + (bias,)
    if x.is_quantized:
        assert x.qscheme() in (torch.per_tensor_affine, torch.per_tensor_symmetric) and x.dtype in (torch.quint8, torch.qint8), \
            "lsq_linear_w8a8 needs a per-tensor torch.quint8 / torch.qint8 tensor"
        s_x = torch.tensor([x.q_scale()], dtype=torch.float32, device=x.device)
        zx = torch.tensor([x.q_zero_point()], dtype=torch.int32, device=x.device)
        return torch.ops.torchlsq.lsq_linear_w8_q8(x.int_repr(), s_x, zx, *w, torch.float32 if out_dtype is None else out_dtype)
    assert scale is not None and shift is not None and quant_min is not None and quant_max is not None, \
        "lsq_linear_w8a8 on a floating x needs the activation quantizer's scale, shift, quant_min and quant_max"
    assert out_dtype is None or out_dtype == x.dtype, "a floating x gives y of x's dtype"
    type_min = quant_min if type_min is None else type_min
    type_max = quant_max if type_max is None else type_max
    return torch.ops.torchlsq.lsq_linear_w8_a8(x, scale, shift, int(quant_min), int(quant_max), int(type_min), int(type_max), *w)


def _conv_padding(padding, kernel, stride, dilation):
    """(ph, pw) of F.conv2d's `padding` argument: ints, a pair, 'valid', or 'same' where it is symmetric (stride 1 and an even
    dilation * (kernel - 1) per axis; torch pads the odd remainder on one side only, which this op does not do)"""
    if isinstance(padding, str):
        if padding == "valid":
            return (0, 0)
        if padding != "same":
            raise ValueError("lsq_conv2d_w8a8: padding must be ints, a pair, 'valid' or 'same', got %r" % padding)
        if tuple(stride) != (1, 1):
            raise ValueError("lsq_conv2d_w8a8: padding='same' needs stride 1, got %s" % (tuple(stride),))
        total = [d * (k - 1) for d, k in zip(dilation, kernel)]
        if any(t % 2 for t in total):
            raise ValueError("lsq_conv2d_w8a8: padding='same' is asymmetric for kernel %s with dilation %s (dilation * (kernel - 1) "
                             "is odd); only symmetric zero padding is served" % (tuple(kernel), tuple(dilation)))
        return tuple(t // 2 for t in total)
    return _two(padding, "padding")


def _two(v, name):
    v = tuple(int(e) for e in v) if isinstance(v, (tuple, list)) else (int(v),)
    if len(v) not in (1, 2):
        raise ValueError("lsq_conv2d_w8a8: %s must be one int or a pair of ints" % name)
    return v * 2 if len(v) == 1 else v


def lsq_conv2d_w8a8(x: Tensor, weight_q: Tensor, bias: Tensor = None, stride=1, padding=0, dilation=1, groups: int = 1,
                    scale: Tensor = None, shift: Tensor = None, quant_min: int = None, quant_max: int = None, type_min: int = None,
                    type_max: int = None, out_dtype=None) -> Tensor:
    """A 2-D convolution on 8-bit activations and an 8-bit weight (W8A8), summed in integers: `lsq_linear_w8a8`'s arithmetic with
    the sum running over every tap (i, j) and input channel c,
    `y[b, n, oh, ow] = ((s_w[n] * float(I)) * s_x) + bias[n]`, `I = sum (lx[b, c, oh sh - ph + i dh, ow sw - pw + j dw] - zx) *
    (lw[n, c, i, j] - zw[n])`; a tap in the zero padding contributes 0.  `F.conv2d`'s arguments with `groups == 1` and zero
    padding: `padding` is ints, a pair, 'valid', or 'same' where that is symmetric.

    `weight_q` is the 4-D per-channel (axis 0) or per-tensor `torch.qint8` / `torch.quint8` tensor that
    `LSQFakeQuantizer.quantize(conv.weight)` returns.  x [B, Cin, H, W] is floating (with the per-tensor activation quantizer's
    `scale`, `shift`, `quant_min`, `quant_max`; y has x's dtype) or a per-tensor `torch.quint8` / `torch.qint8` tensor (with
    `out_dtype`, default float32), exactly as in `lsq_linear_w8a8`; the two forms agree bit for bit.

    The result is [B, Cout, OH, OW] in channels-last memory.  The kernels read channels-last operands: an x or a weight that is
    not channels-last is copied into that format first (one extra pass over it).  No atomics; repeated calls are bit-identical;
    the GPU result (liblsq_hip_qconv_w8.so, an int8 matrix-core implicit GEMM) equals the CPU result (one int64 `F.conv2d`)
    bit for bit.  Inference only."""
    _assert_has_ops()
    if groups != 1:
        raise ValueError("lsq_conv2d_w8a8 serves groups == 1 only, got groups = %d" % groups)
    assert weight_q.is_quantized and weight_q.dtype in (torch.qint8, torch.quint8) and weight_q.dim() == 4, \
        "lsq_conv2d_w8a8 needs a 4-D torch.qint8 / torch.quint8 weight [out_channels, in_channels, kh, kw]"
    stride, dilation = _two(stride, "stride"), _two(dilation, "dilation")
    padding = _conv_padding(padding, weight_q.shape[2:], stride, dilation)
    w = w8_weight_operands(weight_q) + (bias, list(stride), list(padding), list(dilation))
    if x.is_quantized:
        assert x.qscheme() in (torch.per_tensor_affine, torch.per_tensor_symmetric) and x.dtype in (torch.quint8, torch.qint8), \
            "lsq_conv2d_w8a8 needs a per-tensor torch.quint8 / torch.qint8 tensor"
        s_x = torch.tensor([x.q_scale()], dtype=torch.float32, device=x.device)
        zx = torch.tensor([x.q_zero_point()], dtype=torch.int32, device=x.device)
        return torch.ops.torchlsq.lsq_conv2d_w8_q8(x.int_repr(), s_x, zx, *w, torch.float32 if out_dtype is None else out_dtype)
    assert scale is not None and shift is not None and quant_min is not None and quant_max is not None, \
        "lsq_conv2d_w8a8 on a floating x needs the activation quantizer's scale, shift, quant_min and quant_max"
    assert out_dtype is None or out_dtype == x.dtype, "a floating x gives y of x's dtype"
    type_min = quant_min if type_min is None else type_min
    type_max = quant_max if type_max is None else type_max
    return torch.ops.torchlsq.lsq_conv2d_w8_a8(x, scale, shift, int(quant_min), int(quant_max), int(type_min), int(type_max), *w)


class LevelsTensor:
    """The 8-bit levels of a per-tensor quantized activation with their constants ON THE DEVICE: what one W8A8 layer with an
    8-bit output hands to the next.  `levels` (uint8 or int8; a convolution's are a logical [B, C, H, W] tensor in channels-last
    memory), `scale` (float32 [1], the sanitised scale) and `zero_point` (int32 [1]) on the levels' device, and the level range
    `quant_min`, `quant_max`, `type_min`, `type_max`.  The real value of a level is (level - zero_point) * scale.  Nothing here
    reads back to the host except `to_quantized()`."""

    def __init__(self, levels, scale, zero_point, quant_min, quant_max, type_min=None, type_max=None):
        assert levels.dtype in (torch.uint8, torch.int8), "LevelsTensor holds uint8 or int8 levels"
        assert scale.dtype == torch.float32 and scale.numel() == 1 and zero_point.dtype == torch.int32 and zero_point.numel() == 1, \
            "LevelsTensor needs one float32 scale and one int32 zero point (tensors on the levels' device)"
        self.levels, self.scale, self.zero_point = levels, scale.reshape(1), zero_point.reshape(1)
        self.quant_min, self.quant_max = int(quant_min), int(quant_max)
        self.type_min = self.quant_min if type_min is None else int(type_min)
        self.type_max = self.quant_max if type_max is None else int(type_max)

    shape = property(lambda self: self.levels.shape)
    device = property(lambda self: self.levels.device)
    dtype = property(lambda self: self.levels.dtype)

    def dequantize(self, dtype=torch.float32) -> Tensor:
        """(levels - zero_point) * scale in float32, then `dtype`"""
        return ((self.levels.to(torch.float32) - self.zero_point.to(torch.float32)) * self.scale).to(dtype)

    def to_quantized(self) -> Tensor:
        """a per-tensor torch.quint8 / torch.qint8 tensor of the same levels; reads scale and zero point back to the host"""
        return torch._make_per_tensor_quantized_tensor(self.levels, float(self.scale.item()), int(self.zero_point.item()))

    def flatten(self, start_dim=1, end_dim=-1):
        """the levels flattened like `torch.flatten` (of the logical shape), same constants"""
        return LevelsTensor(self.levels.flatten(start_dim, end_dim), self.scale, self.zero_point, self.quant_min, self.quant_max,
                            self.type_min, self.type_max)

    @classmethod
    def from_quantized(cls, xq: Tensor):
        """from a per-tensor torch.quint8 / torch.qint8 tensor; its scale and zero point are uploaded once"""
        assert xq.is_quantized and xq.qscheme() in (torch.per_tensor_affine, torch.per_tensor_symmetric) and \
            xq.dtype in (torch.quint8, torch.qint8), "LevelsTensor.from_quantized needs a per-tensor torch.quint8 / torch.qint8 tensor"
        lo, hi = (0, 255) if xq.dtype == torch.quint8 else (-128, 127)
        return cls(xq.int_repr(), torch.tensor([xq.q_scale()], dtype=torch.float32, device=xq.device),
                   torch.tensor([xq.q_zero_point()], dtype=torch.int32, device=xq.device), lo, hi, lo, hi)


def _levels_out(levels, out_scale, out_shift, rng):
    s, z = _act_constants(out_scale, out_shift, rng[2], rng[3])
    return LevelsTensor(levels, s, z, *rng)


def _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, relu):
    assert out_scale is not None and out_shift is not None and out_quant_min is not None and out_quant_max is not None, \
        "%s needs the output quantizer's out_scale, out_shift, out_quant_min and out_quant_max" % what
    tmin = out_quant_min if out_type_min is None else out_type_min
    tmax = out_quant_max if out_type_max is None else out_type_max
    sc = out_scale.detach().reshape(-1)[:1].to(torch.float32)
    sh = out_shift.detach().reshape(-1)[:1].to(torch.float32)
    return (sc, sh, int(out_quant_min), int(out_quant_max), int(tmin), int(tmax), bool(relu))


def lsq_linear_w8a8_q(x, weight_q: Tensor, bias: Tensor = None, scale: Tensor = None, shift: Tensor = None, quant_min: int = None,
                      quant_max: int = None, type_min: int = None, type_max: int = None, out_scale: Tensor = None,
                      out_shift: Tensor = None, out_quant_min: int = None, out_quant_max: int = None, out_type_min: int = None,
                      out_type_max: int = None, relu: bool = False, mid_dtype=torch.float32) -> LevelsTensor:
    """`lsq_linear_w8a8` with an 8-bit output: the integer sum, its fp32 steps `v`, `u = float(round_to(mid_dtype, v))`, an
    optional ReLU (a select: a NaN stays a NaN) and the levels of the per-tensor quantizer (`out_scale`, `out_shift`,
    `out_quant_min`, `out_quant_max`, type range) of `u` -- in one launch, one byte written per output
    (liblsq_hip_requant_w8.so).  Bit for bit the composition `lsq_linear_w8a8(..., out_dtype=mid_dtype)`, the select,
    `lsq_levels_per_tensor`; `mid_dtype` is the dtype in which the unfused model hands y to the next quantizer.

    x is a `LevelsTensor` (its device constants are used, nothing is read back), a per-tensor `torch.quint8` / `torch.qint8`
    tensor, or a floating tensor with the INPUT quantizer's `scale`, `shift`, `quant_min`, `quant_max` (then `mid_dtype` is x's
    dtype).  Returns a `LevelsTensor` whose constants are formed on the device from `out_scale` and `out_shift`.
    Inference only."""
    _assert_has_ops()
    what = "lsq_linear_w8a8_q"
    w = w8_weight_operands(weight_q) + (bias,)
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, relu)
    if isinstance(x, Tensor) and x.is_quantized:
        x = LevelsTensor.from_quantized(x)
    if isinstance(x, LevelsTensor):
        lv = torch.ops.torchlsq.lsq_linear_w8_q8_q(x.levels, x.scale, x.zero_point, *w, *o, mid_dtype)
    else:
        assert scale is not None and shift is not None and quant_min is not None and quant_max is not None, \
            "%s on a floating x needs the input quantizer's scale, shift, quant_min and quant_max" % what
        assert mid_dtype in (None, torch.float32, x.dtype), "a floating x fixes mid_dtype to x's dtype"
        type_min = quant_min if type_min is None else type_min
        type_max = quant_max if type_max is None else type_max
        lv = torch.ops.torchlsq.lsq_linear_w8_a8_q(x, scale, shift, int(quant_min), int(quant_max), int(type_min), int(type_max), *w, *o)
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_conv2d_w8a8_q(x, weight_q: Tensor, bias: Tensor = None, stride=1, padding=0, dilation=1, groups: int = 1, scale: Tensor = None,
                      shift: Tensor = None, quant_min: int = None, quant_max: int = None, type_min: int = None, type_max: int = None,
                      out_scale: Tensor = None, out_shift: Tensor = None, out_quant_min: int = None, out_quant_max: int = None,
                      out_type_min: int = None, out_type_max: int = None, relu: bool = False, mid_dtype=torch.float32) -> LevelsTensor:
    """`lsq_conv2d_w8a8` with an 8-bit output, exactly as `lsq_linear_w8a8_q` is to `lsq_linear_w8a8`.  The returned levels are a
    logical [B, Cout, OH, OW] tensor in channels-last memory: the next convolution's operand as it lies.  Inference only."""
    _assert_has_ops()
    what = "lsq_conv2d_w8a8_q"
    if groups != 1:
        raise ValueError("lsq_conv2d_w8a8_q serves groups == 1 only, got groups = %d" % groups)
    assert weight_q.is_quantized and weight_q.dtype in (torch.qint8, torch.quint8) and weight_q.dim() == 4, \
        "lsq_conv2d_w8a8_q needs a 4-D torch.qint8 / torch.quint8 weight [out_channels, in_channels, kh, kw]"
    stride, dilation = _two(stride, "stride"), _two(dilation, "dilation")
    padding = _conv_padding(padding, weight_q.shape[2:], stride, dilation)
    w = w8_weight_operands(weight_q) + (bias, list(stride), list(padding), list(dilation))
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, relu)
    if isinstance(x, Tensor) and x.is_quantized:
        x = LevelsTensor.from_quantized(x)
    if isinstance(x, LevelsTensor):
        lv = torch.ops.torchlsq.lsq_conv2d_w8_q8_q(x.levels, x.scale, x.zero_point, *w, *o, mid_dtype)
    else:
        assert scale is not None and shift is not None and quant_min is not None and quant_max is not None, \
            "%s on a floating x needs the input quantizer's scale, shift, quant_min and quant_max" % what
        assert mid_dtype in (None, torch.float32, x.dtype), "a floating x fixes mid_dtype to x's dtype"
        type_min = quant_min if type_min is None else type_min
        type_max = quant_max if type_max is None else type_max
        lv = torch.ops.torchlsq.lsq_conv2d_w8_a8_q(x, scale, shift, int(quant_min), int(quant_max), int(type_min), int(type_max), *w, *o)
    return _levels_out(lv, o[0], o[1], o[2:6])


def _res_args(what, residual, pre_scale, pre_shift, pre_quant_min, pre_quant_max, pre_type_min, pre_type_max):
    assert isinstance(residual, LevelsTensor), "%s needs the residual as a LevelsTensor" % what
    if pre_scale is None:
        assert pre_shift is None, "%s: pre_scale and pre_shift come together" % what
        return (residual.levels, residual.scale, residual.zero_point, None, None, 0, 255, 0, 255)
    assert pre_shift is not None and pre_quant_min is not None and pre_quant_max is not None, \
        "%s with a pre-quantizer needs pre_scale, pre_shift, pre_quant_min and pre_quant_max" % what
    tmin = pre_quant_min if pre_type_min is None else pre_type_min
    tmax = pre_quant_max if pre_type_max is None else pre_type_max
    sc = pre_scale.detach().reshape(-1)[:1].to(torch.float32)
    sh = pre_shift.detach().reshape(-1)[:1].to(torch.float32)
    return (residual.levels, residual.scale, residual.zero_point, sc, sh, int(pre_quant_min), int(pre_quant_max), int(tmin), int(tmax))


def lsq_linear_w8a8_add_q(x, weight_q: Tensor, bias: Tensor, residual: LevelsTensor, out_scale: Tensor = None, out_shift: Tensor = None,
                          out_quant_min: int = None, out_quant_max: int = None, out_type_min: int = None, out_type_max: int = None,
                          relu: bool = False, mid_dtype=torch.float32, pre_scale: Tensor = None, pre_shift: Tensor = None,
                          pre_quant_min: int = None, pre_quant_max: int = None, pre_type_min: int = None,
                          pre_type_max: int = None) -> LevelsTensor:
    """The end of a residual block in one launch: `lsq_linear_w8a8_q` with `residual`, a `LevelsTensor` of the output's shape,
    added before the ReLU.  With u the layer's value rounded to `mid_dtype`: `p` is u, or with a pre-quantizer (`pre_scale`,
    `pre_shift`, `pre_quant_min`, `pre_quant_max`, type range: the layer's own output fake-quantizer, as a torch.ao QAT layer
    applies it before a `FloatFunctional.add`) `lsq(u, ...)`; `t = p + residual.dequantize(mid_dtype)` in `mid_dtype`; an
    optional ReLU (a select); the levels of the output quantizer (the add's) of t -- one byte read and one written per output
    (liblsq_hip_resadd_w8.so).  Bit for bit the composition `lsq_linear_w8a8(..., out_dtype=mid_dtype)`, `lsq`, the add, the
    select, `lsq_levels_per_tensor`.

    x is a `LevelsTensor` or a per-tensor `torch.quint8` / `torch.qint8` tensor.  Returns a `LevelsTensor`; nothing is read
    back from the device.  Inference only."""
    _assert_has_ops()
    what = "lsq_linear_w8a8_add_q"
    w = w8_weight_operands(weight_q) + (bias,)
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, relu)
    r = _res_args(what, residual, pre_scale, pre_shift, pre_quant_min, pre_quant_max, pre_type_min, pre_type_max)
    if isinstance(x, Tensor) and x.is_quantized:
        x = LevelsTensor.from_quantized(x)
    assert isinstance(x, LevelsTensor), "%s needs x as a LevelsTensor or a per-tensor quantized tensor" % what
    lv = torch.ops.torchlsq.lsq_linear_w8_q8_add_q(x.levels, x.scale, x.zero_point, *w, *o, mid_dtype, *r)
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_conv2d_w8a8_add_q(x, weight_q: Tensor, bias: Tensor, residual: LevelsTensor, stride=1, padding=0, dilation=1, groups: int = 1,
                          out_scale: Tensor = None, out_shift: Tensor = None, out_quant_min: int = None, out_quant_max: int = None,
                          out_type_min: int = None, out_type_max: int = None, relu: bool = False, mid_dtype=torch.float32,
                          pre_scale: Tensor = None, pre_shift: Tensor = None, pre_quant_min: int = None, pre_quant_max: int = None,
                          pre_type_min: int = None, pre_type_max: int = None) -> LevelsTensor:
    """`lsq_conv2d_w8a8_q` with a residual, exactly as `lsq_linear_w8a8_add_q` is to `lsq_linear_w8a8_q`.  `residual` holds a
    logical [B, Cout, OH, OW] level tensor; one that is not in channels-last memory is copied into that format first.  The
    returned levels are in channels-last memory.  Inference only."""
    _assert_has_ops()
    what = "lsq_conv2d_w8a8_add_q"
    if groups != 1:
        raise ValueError("lsq_conv2d_w8a8_add_q serves groups == 1 only, got groups = %d" % groups)
    assert weight_q.is_quantized and weight_q.dtype in (torch.qint8, torch.quint8) and weight_q.dim() == 4, \
        "lsq_conv2d_w8a8_add_q needs a 4-D torch.qint8 / torch.quint8 weight [out_channels, in_channels, kh, kw]"
    stride, dilation = _two(stride, "stride"), _two(dilation, "dilation")
    padding = _conv_padding(padding, weight_q.shape[2:], stride, dilation)
    w = w8_weight_operands(weight_q) + (bias, list(stride), list(padding), list(dilation))
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, relu)
    r = _res_args(what, residual, pre_scale, pre_shift, pre_quant_min, pre_quant_max, pre_type_min, pre_type_max)
    if isinstance(x, Tensor) and x.is_quantized:
        x = LevelsTensor.from_quantized(x)
    assert isinstance(x, LevelsTensor), "%s needs x as a LevelsTensor or a per-tensor quantized tensor" % what
    lv = torch.ops.torchlsq.lsq_conv2d_w8_q8_add_q(x.levels, x.scale, x.zero_point, *w, *o, mid_dtype, *r)
    return _levels_out(lv, o[0], o[1], o[2:6])


def _pool_levels(what, x):
    if isinstance(x, Tensor) and x.is_quantized:
        x = LevelsTensor.from_quantized(x)
    assert isinstance(x, LevelsTensor) and x.levels.dim() == 4, "%s needs x as a LevelsTensor (or a per-tensor quantized tensor) of [B, C, H, W]" % what
    return x


def _pool_geometry(kernel_size, stride, padding):
    kernel = _two(kernel_size, "kernel_size")
    return list(kernel), list(kernel if stride is None or stride == [] else _two(stride, "stride")), list(_two(padding, "padding"))


def lsq_max_pool2d_w8(x: LevelsTensor, kernel_size, stride=None, padding=0, dilation=1, ceil_mode: bool = False) -> LevelsTensor:
    """`F.max_pool2d` on 8-bit levels: the max over each window's taps inside the input of the levels as integers (a tap in the
    padding does not take part), one byte read and a fraction of one written per activation (liblsq_hip_pool_w8.so).  The
    result holds levels of the SAME quantizer: it carries x's `scale` and `zero_point` tensors as they are, nothing is copied or
    read back.  Because dequantize is non-decreasing this is also, bit for bit, `F.max_pool2d(x.dequantize(dtype))` taken back
    to levels.  `F.max_pool2d`'s arguments; padding is at most half the kernel.  A `LevelsTensor` in NCHW memory is copied to
    channels-last first; the returned levels are a logical [B, C, OH, OW] tensor in channels-last memory.  Inference only."""
    _assert_has_ops()
    x = _pool_levels("lsq_max_pool2d_w8", x)
    kernel, stride, padding = _pool_geometry(kernel_size, stride, padding)
    lv = torch.ops.torchlsq.lsq_max_pool2d_q8(x.levels, kernel, stride, padding, list(_two(dilation, "dilation")), bool(ceil_mode))
    return LevelsTensor(lv, x.scale, x.zero_point, x.quant_min, x.quant_max, x.type_min, x.type_max)


def lsq_avg_pool2d_w8_q(x: LevelsTensor, kernel_size, stride=None, padding=0, ceil_mode: bool = False, count_include_pad: bool = True,
                        divisor_override: int = None, out_scale: Tensor = None, out_shift: Tensor = None, out_quant_min: int = None,
                        out_quant_max: int = None, out_type_min: int = None, out_type_max: int = None,
                        mid_dtype=torch.float32) -> LevelsTensor:
    """`F.avg_pool2d` on 8-bit levels with an 8-bit output: the exact integer sum S of (level - zero_point) over each window's taps
    inside the input, `v = (float(S) * scale) / float(D)` in fp32 with `F.avg_pool2d`'s divisor D (`divisor_override`, else the
    window clipped to the padded extent with `count_include_pad`, else the taps inside the input), `u = round_to(mid_dtype, v)`
    and the levels of the per-tensor output quantizer (`out_scale`, `out_shift`, `out_quant_min`, `out_quant_max`, type range) of
    u -- one launch (liblsq_hip_pool_w8.so), nothing is read back.  v is within two roundings of the exact mean; it is not
    ATen's float `avg_pool2d`, which sums rounded floats in an order of its own.  Returns a `LevelsTensor` in channels-last
    memory whose constants are formed on the device.  Inference only."""
    _assert_has_ops()
    what = "lsq_avg_pool2d_w8_q"
    x = _pool_levels(what, x)
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, False)
    kernel, stride, padding = _pool_geometry(kernel_size, stride, padding)
    lv = torch.ops.torchlsq.lsq_avg_pool2d_q8_q(x.levels, x.scale, x.zero_point, kernel, stride, padding, bool(ceil_mode),
                                                bool(count_include_pad), divisor_override, *o[:6], mid_dtype)
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_avg_pool2d_w8(x: LevelsTensor, kernel_size, stride=None, padding=0, ceil_mode: bool = False, count_include_pad: bool = True,
                      divisor_override: int = None, out_dtype=torch.float32) -> Tensor:
    """`lsq_avg_pool2d_w8_q` without an output quantizer: the averages `round_to(out_dtype, v)` as a floating
    [B, C, OH, OW] tensor in channels-last memory.  Inference only."""
    _assert_has_ops()
    x = _pool_levels("lsq_avg_pool2d_w8", x)
    kernel, stride, padding = _pool_geometry(kernel_size, stride, padding)
    return torch.ops.torchlsq.lsq_avg_pool2d_q8(x.levels, x.scale, x.zero_point, kernel, stride, padding, bool(ceil_mode),
                                                bool(count_include_pad), divisor_override, out_dtype)


def lsq_adaptive_avg_pool2d_w8_q(x: LevelsTensor, output_size, out_scale: Tensor = None, out_shift: Tensor = None,
                                 out_quant_min: int = None, out_quant_max: int = None, out_type_min: int = None,
                                 out_type_max: int = None, mid_dtype=torch.float32) -> LevelsTensor:
    """`F.adaptive_avg_pool2d` on 8-bit levels with an 8-bit output, for an `output_size` that divides H and W evenly (1: global
    pooling): `lsq_avg_pool2d_w8_q` with kernel = stride = (H / OH, W / OW).  Any other output size is refused."""
    _assert_has_ops()
    x = _pool_levels("lsq_adaptive_avg_pool2d_w8_q", x)
    kernel = _E.pool_w8_adaptive_kernel(x.shape[2], x.shape[3], output_size)
    return lsq_avg_pool2d_w8_q(x, kernel, kernel, 0, False, True, None, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min,
                               out_type_max, mid_dtype)


def lsq_adaptive_avg_pool2d_w8(x: LevelsTensor, output_size, out_dtype=torch.float32) -> Tensor:
    """`lsq_adaptive_avg_pool2d_w8_q` without an output quantizer: floats out."""
    _assert_has_ops()
    x = _pool_levels("lsq_adaptive_avg_pool2d_w8", x)
    kernel = _E.pool_w8_adaptive_kernel(x.shape[2], x.shape[3], output_size)
    return lsq_avg_pool2d_w8(x, kernel, kernel, 0, False, True, None, out_dtype)


_DW_ACTS = {None: 0, "none": 0, "relu": 1, "relu6": 2, False: 0, True: 1, 0: 0, 1: 1, 2: 2}


def dw_weight_operands(weight_q: Tensor):
    """(levels [kh, kw, C] int8 / uint8, TAP-MAJOR, scale [C] float32, zero point [C] int32) of the 4-D [C, 1, kh, kw] per-channel
    (axis 0) or per-tensor `torch.qint8` / `torch.quint8` weight of a depthwise convolution, e.g. `LSQFakeQuantizer.quantize(w)`:
    what `lsq_dwconv2d_w8_q8` / `_q` take.  The permutation is one small copy; nothing is read back from the device."""
    assert weight_q.is_quantized and weight_q.dtype in (torch.qint8, torch.quint8) and weight_q.dim() == 4 and weight_q.shape[1] == 1, \
        "lsq_depthwise_conv2d_w8a8 needs a 4-D torch.qint8 / torch.quint8 weight [channels, 1, kh, kw] (a channel multiplier is not served)"
    levels, scale, zero = w8_weight_operands(weight_q)
    return levels[:, 0].permute(1, 2, 0).contiguous(), scale, zero


def _dw_input(what, x, scale, shift, quant_min, quant_max, type_min, type_max):
    """x as a LevelsTensor: as it is, from a per-tensor quantized tensor, or from a floating x through `lsq_levels_per_tensor`
    with the input quantizer's constants formed on the device"""
    if isinstance(x, LevelsTensor):
        return x
    if x.is_quantized:
        return LevelsTensor.from_quantized(x)
    assert scale is not None and shift is not None and quant_min is not None and quant_max is not None, \
        "%s on a floating x needs the input quantizer's scale, shift, quant_min and quant_max" % what
    type_min = quant_min if type_min is None else type_min
    type_max = quant_max if type_max is None else type_max
    rng = (int(quant_min), int(quant_max), int(type_min), int(type_max))
    sc, sh = scale.detach().reshape(-1)[:1].to(torch.float32), shift.detach().reshape(-1)[:1].to(torch.float32)
    lv = torch.ops.torchlsq.lsq_levels_per_tensor(x.detach(), sc, sh, *rng, 0)
    s_x, zx = _act_constants(sc, sh, rng[2], rng[3])
    return LevelsTensor(lv.view(torch.uint8) if max(rng[1], rng[3]) > 127 else lv, s_x, zx, *rng)


def _dw_args(what, weight_q, bias, stride, padding, dilation, act):
    assert act in _DW_ACTS, "%s: act must be 'none', 'relu' or 'relu6', got %r" % (what, act)
    wl, ws, wz = dw_weight_operands(weight_q)
    stride, dilation = _two(stride, "stride"), _two(dilation, "dilation")
    padding = _conv_padding(padding, wl.shape[:2], stride, dilation)
    return (wl, ws, wz, bias, list(stride), list(padding), list(dilation)), _DW_ACTS[act]


def lsq_depthwise_conv2d_w8a8_q(x, weight_q: Tensor, bias: Tensor = None, stride=1, padding=0, dilation=1, scale: Tensor = None,
                                shift: Tensor = None, quant_min: int = None, quant_max: int = None, type_min: int = None,
                                type_max: int = None, out_scale: Tensor = None, out_shift: Tensor = None, out_quant_min: int = None,
                                out_quant_max: int = None, out_type_min: int = None, out_type_max: int = None, act="none",
                                mid_dtype=None) -> LevelsTensor:
    """A DEPTHWISE 2-D convolution (`F.conv2d` with `groups == in_channels == out_channels`) on 8-bit activations and an 8-bit
    weight with an 8-bit output: per channel c the exact integer `I = sum over the taps inside x of (lx - zx) * (lw[c] - zw[c])`
    (a tap in the zero padding contributes 0), `v = ((s_w[c] * float(I)) * s_x) + bias[c]` in fp32, `u = round_to(mid_dtype, v)`,
    `act` ('none', 'relu' or 'relu6'; selects, a NaN stays a NaN) and the levels of the per-tensor output quantizer
    (`out_scale`, `out_shift`, `out_quant_min`, `out_quant_max`, type range) -- one launch, one byte read and one written per
    activation (liblsq_hip_dwconv_w8.so); the GPU result equals the CPU result (one int64 grouped `F.conv2d`) bit for bit.

    `weight_q` is the [C, 1, kh, kw] per-channel (axis 0) or per-tensor `torch.qint8` / `torch.quint8` weight that
    `LSQFakeQuantizer.quantize(conv.weight)` returns.  The kernel reads it tap-major, [kh, kw, C]: THIS FUNCTION PERMUTES IT ON
    EVERY CALL (one small copy); `torchlsq.quantized.DepthwiseConv2dW8A8Q` stores it that way once, at conversion.
    x is a `LevelsTensor` (its device constants are used), a per-tensor `torch.quint8` / `torch.qint8` tensor, or a floating
    [B, C, H, W] tensor with the INPUT quantizer's `scale`, `shift`, `quant_min`, `quant_max`, which goes through
    `lsq_levels_per_tensor` first (`mid_dtype` then defaults to x's dtype, else to float32).  Nothing is read back to the host.
    Returns a `LevelsTensor` in channels-last memory.  Inference only."""
    _assert_has_ops()
    what = "lsq_depthwise_conv2d_w8a8_q"
    w, a = _dw_args(what, weight_q, bias, stride, padding, dilation, act)
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, False)
    if mid_dtype is None:
        mid_dtype = x.dtype if isinstance(x, Tensor) and not x.is_quantized else torch.float32
    x = _dw_input(what, x, scale, shift, quant_min, quant_max, type_min, type_max)
    lv = torch.ops.torchlsq.lsq_dwconv2d_w8_q8_q(x.levels, x.scale, x.zero_point, *w, *o[:6], a, mid_dtype)
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_depthwise_conv2d_w8a8(x, weight_q: Tensor, bias: Tensor = None, stride=1, padding=0, dilation=1, scale: Tensor = None,
                              shift: Tensor = None, quant_min: int = None, quant_max: int = None, type_min: int = None,
                              type_max: int = None, act="none", out_dtype=None) -> Tensor:
    """`lsq_depthwise_conv2d_w8a8_q` without an output quantizer: the activated values as `out_dtype` floats (default: a floating
    x's dtype, else float32), [B, C, OH, OW] in channels-last memory.  The weight is permuted on every call, as there.
    Inference only."""
    _assert_has_ops()
    what = "lsq_depthwise_conv2d_w8a8"
    w, a = _dw_args(what, weight_q, bias, stride, padding, dilation, act)
    if out_dtype is None:
        out_dtype = x.dtype if isinstance(x, Tensor) and not x.is_quantized else torch.float32
    x = _dw_input(what, x, scale, shift, quant_min, quant_max, type_min, type_max)
    return torch.ops.torchlsq.lsq_dwconv2d_w8_q8(x.levels, x.scale, x.zero_point, *w, a, out_dtype)


# -------------------------------------------------------------------------------------------------
# elementwise ops on 8-bit levels: activation functions as a 256-entry byte table, and the squeeze-and-excitation multiply
# -------------------------------------------------------------------------------------------------
def _named_acts():
    F = torch.nn.functional
    return {"identity": None, "relu": F.relu, "relu6": F.relu6, "hardtanh": F.hardtanh, "leaky_relu": F.leaky_relu,
            "hardswish": F.hardswish, "hardsigmoid": F.hardsigmoid, "silu": F.silu, "gelu": F.gelu,
            "gelu_tanh": lambda v: F.gelu(v, approximate="tanh"), "sigmoid": torch.sigmoid, "tanh": torch.tanh}


def act_function(fn):
    """(callable or None, name) of an activation given as None (the identity), one of the names "identity", "relu", "relu6",
    "hardtanh", "leaky_relu", "hardswish", "hardsigmoid", "silu", "gelu", "gelu_tanh", "sigmoid", "tanh", the `torch.nn` module
    of one of them (its parameters -- a Hardtanh's bounds, a LeakyReLU's slope, a GELU's `approximate` -- are kept), or any
    other callable, which is taken as it is"""
    nn, F = torch.nn, torch.nn.functional
    if fn is None:
        return None, "identity"
    if isinstance(fn, str):
        named = _named_acts()
        assert fn in named, "unknown activation %r: one of %s, an nn module of one of them, or a callable" % (fn, sorted(named))
        return named[fn], fn
    if isinstance(fn, nn.Hardtanh) and not isinstance(fn, nn.ReLU6):
        lo, hi = float(fn.min_val), float(fn.max_val)
        return (lambda v: F.hardtanh(v, lo, hi)), "hardtanh(%g, %g)" % (lo, hi)
    if isinstance(fn, nn.LeakyReLU):
        slope = float(fn.negative_slope)
        return (lambda v: F.leaky_relu(v, slope)), "leaky_relu(%g)" % slope
    if isinstance(fn, nn.GELU):
        return act_function("gelu_tanh" if fn.approximate == "tanh" else "gelu")
    for cls, name in ((nn.Identity, "identity"), (nn.ReLU6, "relu6"), (nn.ReLU, "relu"), (nn.Hardswish, "hardswish"),
                      (nn.Hardsigmoid, "hardsigmoid"), (nn.SiLU, "silu"), (nn.Sigmoid, "sigmoid"), (nn.Tanh, "tanh")):
        if isinstance(fn, cls):
            return act_function(name)
    assert callable(fn), "an activation is a name, a torch.nn activation module or a callable, got %s" % type(fn).__name__
    return fn, getattr(fn, "__name__", type(fn).__name__)


def lsq_act_table(fn, in_scale: Tensor, in_zero_point: Tensor, in_dtype, out_scale: Tensor, out_shift: Tensor, out_quant_min: int,
                  out_quant_max: int, out_type_min: int = None, out_type_max: int = None, mid_dtype=torch.float32) -> Tensor:
    """The 256-entry byte table (uint8 [256], on `in_scale`'s device) of an elementwise function between two per-tensor 8-bit
    quantizers, built from existing ops alone -- no new kernel, nothing read back:

        b  = arange(256, uint8) viewed as `in_dtype` (uint8 / int8): every byte an input level can be stored as
        u  = LevelsTensor(b, in_scale, in_zero_point).dequantize(mid_dtype)
        v  = fn(u)                        a torch callable, same shape, must return `mid_dtype`; None: the identity
        table = lsq_levels_per_tensor(v, out_scale, out_shift, out range, 0) as bytes

    so `table[levels]` (`lsq_lut_w8`) equals the unfused chain dequantize -> fn -> the next quantizer on the same device, bit for
    bit, for any `fn` (`act_function` lists the names and modules).  The entries of bytes outside the input's
    quant_min..quant_max are filled the same way and never read.  With `fn=None` the table REQUANTIZES from one per-tensor
    quantizer to another, which is what the branches of a concatenation need before they can share one.  The clamp-type
    functions (identity, relu, relu6, hardtanh) give the same table on the CPU and on the GPU; for the transcendental ones ATen's
    CPU and GPU kernels may round differently, so build the table on the device whose unfused chain it has to equal."""
    _assert_has_ops()
    assert in_dtype in (torch.uint8, torch.int8), "lsq_act_table: in_dtype must be torch.uint8 or torch.int8"
    call, _ = act_function(fn)
    o = _out_args("lsq_act_table", out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, False)
    b = torch.arange(256, dtype=torch.uint8, device=in_scale.device).view(in_dtype)
    lo, hi = (0, 255) if in_dtype == torch.uint8 else (-128, 127)
    u = LevelsTensor(b, in_scale.detach(), in_zero_point, lo, hi).dequantize(mid_dtype)
    v = u if call is None else call(u)
    assert isinstance(v, Tensor) and v.shape == u.shape and v.dtype == mid_dtype, \
        "lsq_act_table: the function must return a %s tensor of its input's shape" % str(mid_dtype).replace("torch.", "")
    return torch.ops.torchlsq.lsq_levels_per_tensor(v, *o[:6], 0).view(torch.uint8)


def _levels_in(what, x):
    if isinstance(x, Tensor) and x.is_quantized:
        x = LevelsTensor.from_quantized(x)
    assert isinstance(x, LevelsTensor), "%s needs a LevelsTensor (or a per-tensor quantized tensor)" % what
    return x


def lsq_lut_w8(x: LevelsTensor, table: Tensor, out_scale: Tensor = None, out_shift: Tensor = None, out_quant_min: int = None,
               out_quant_max: int = None, out_type_min: int = None, out_type_max: int = None) -> LevelsTensor:
    """`table[x.levels]` in one launch (liblsq_hip_eltwise_w8.so): one byte read and one written per activation, in x's shape
    and memory layout.  `table` is `lsq_act_table`'s for x's quantizer and the output quantizer given here, whose constants the
    returned `LevelsTensor` carries (formed on the device).  Inference only."""
    _assert_has_ops()
    x = _levels_in("lsq_lut_w8", x)
    o = _out_args("lsq_lut_w8", out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, False)
    lv = torch.ops.torchlsq.lsq_lut_w8(x.levels, table, torch.uint8 if max(o[3], o[5]) > 127 else torch.int8)
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_act_w8_q(x: LevelsTensor, fn, out_scale: Tensor = None, out_shift: Tensor = None, out_quant_min: int = None,
                 out_quant_max: int = None, out_type_min: int = None, out_type_max: int = None, mid_dtype=torch.float32) -> LevelsTensor:
    """An activation function on 8-bit levels with an 8-bit output: bit for bit `lsq_levels_per_tensor(fn(x.dequantize(mid_dtype)),
    output quantizer)` on x's device.  THIS FUNCTION BUILDS THE TABLE ON EVERY CALL (`lsq_act_table`: a handful of launches on 256
    elements) before the one launch of `lsq_lut_w8`; `torchlsq.quantized.ActivationW8Q` builds it once, at conversion.  `fn` as in
    `act_function`.  Inference only."""
    x = _levels_in("lsq_act_w8_q", x)
    table = lsq_act_table(fn, x.scale, x.zero_point, x.levels.dtype, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min,
                          out_type_max, mid_dtype)
    return lsq_lut_w8(x, table, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max)


def _gate_operands(what, x, gate):
    x, gate = _levels_in(what, x), _levels_in(what, gate)
    assert x.levels.dim() in (2, 4) and tuple(gate.levels.shape) in (tuple(x.shape[:2]), tuple(x.shape[:2]) + (1, 1)), \
        "%s needs x of [B, C, H, W] or [B, C] and a gate of [B, C] or [B, C, 1, 1], got %s and %s" % (what, tuple(x.shape), tuple(gate.shape))
    return x.levels, x.scale, x.zero_point, gate.levels, gate.scale, gate.zero_point


def lsq_mul_gate_w8_q(x: LevelsTensor, gate: LevelsTensor, out_scale: Tensor = None, out_shift: Tensor = None, out_quant_min: int = None,
                      out_quant_max: int = None, out_type_min: int = None, out_type_max: int = None,
                      mid_dtype=torch.float32) -> LevelsTensor:
    """The squeeze-and-excitation multiply on 8-bit levels with an 8-bit output: x [B, C, H, W] (or [B, C]) times a gate of
    [B, C] or [B, C, 1, 1], both `LevelsTensor`s of quantizers and level dtypes of their own.  Bit for bit
    `lsq_levels_per_tensor(x.dequantize(mid_dtype) * gate.dequantize(mid_dtype)[:, :, None, None], output quantizer)`: each operand
    rounded to `mid_dtype`, one rounded product, the output quantizer's levels -- one launch (liblsq_hip_eltwise_w8.so), one byte
    read and one written per activation, nothing read back.  Returns a `LevelsTensor` in x's shape (4-D: channels-last memory).
    Inference only."""
    _assert_has_ops()
    what = "lsq_mul_gate_w8_q"
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, False)
    lv = torch.ops.torchlsq.lsq_mul_gate_w8_q8_q(*_gate_operands(what, x, gate), *o[:6], mid_dtype)
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_mul_gate_w8(x: LevelsTensor, gate: LevelsTensor, out_dtype=torch.float32) -> Tensor:
    """`lsq_mul_gate_w8_q` without an output quantizer: the products `round_to(out_dtype, a * g)` as a floating tensor in x's
    shape.  Inference only."""
    _assert_has_ops()
    return torch.ops.torchlsq.lsq_mul_gate_w8_q8(*_gate_operands("lsq_mul_gate_w8", x, gate), out_dtype)


# -------------------------------------------------------------------------------------------------
# the gated product of a gated MLP (SwiGLU / GeGLU / classic GLU) on 8-bit levels: act(gate) * up in one launch
# -------------------------------------------------------------------------------------------------
def lsq_glu_table(fn, gate_scale: Tensor, gate_zero_point: Tensor, gate_dtype, act_out=None, mid_dtype=torch.float32) -> Tensor:
    """The 256-entry FLOAT table (float32 [256], on `gate_scale`'s device, holding values of `mid_dtype`) of the gate side of a
    gated MLP, built from existing ops alone -- no new kernel, nothing read back:

        b = arange(256, uint8) viewed as `gate_dtype` (uint8 / int8): every byte a gate level can be stored as
        u = LevelsTensor(b, gate_scale, gate_zero_point).dequantize(mid_dtype)
        without an activation quantizer (`act_out` None):   A = fn(u).float()
        with one, `act_out` = (scale, shift, quant_min, quant_max[, type_min, type_max]) of the quantizer after the activation:
            A = LevelsTensor(lsq_act_table(fn, ..., act_out, mid_dtype), that quantizer's constants).dequantize(mid_dtype).float()

    so `lsq_glu_w8_q(gate, up, A, ...)` equals the unfused chains `lsq_levels_per_tensor(fn(gate.dequantize(mid)) *
    up.dequantize(mid), out)` and `lsq_mul_gate_w8_q(lsq_lut_w8(gate, act table), up, out)` on the same device, bit for bit.  `fn`
    as in `act_function` ("silu", "gelu", "gelu_tanh", "sigmoid" for the classic GLU, "relu", ..., a module or any callable).
    For the transcendental functions ATen's CPU and GPU kernels may round differently (`lsq_act_table`): build the table on the
    device whose unfused chain it has to equal, or build it once and move it."""
    _assert_has_ops()
    assert gate_dtype in (torch.uint8, torch.int8), "lsq_glu_table: gate_dtype must be torch.uint8 or torch.int8"
    assert mid_dtype in (torch.float32, torch.bfloat16, torch.float16), "lsq_glu_table: mid_dtype must be float32, bfloat16 or float16"
    if act_out is not None:
        assert isinstance(act_out, (tuple, list)) and len(act_out) in (4, 6), \
            "lsq_glu_table: act_out is (scale, shift, quant_min, quant_max[, type_min, type_max]) of the activation's quantizer"
        o = _out_args("lsq_glu_table", *act_out, *([None] * (6 - len(act_out))), False)
        lv = lsq_act_table(fn, gate_scale, gate_zero_point, gate_dtype, *o[:6], mid_dtype=mid_dtype)
        lv = lv if max(o[3], o[5]) > 127 else lv.view(torch.int8)
        return _levels_out(lv, o[0], o[1], o[2:6]).dequantize(mid_dtype).float()
    call, _ = act_function(fn)
    b = torch.arange(256, dtype=torch.uint8, device=gate_scale.device).view(gate_dtype)
    lo, hi = (0, 255) if gate_dtype == torch.uint8 else (-128, 127)
    u = LevelsTensor(b, gate_scale.detach().reshape(-1)[:1].to(torch.float32), gate_zero_point, lo, hi).dequantize(mid_dtype)
    v = u if call is None else call(u)
    assert isinstance(v, Tensor) and v.shape == u.shape and v.dtype == mid_dtype, \
        "lsq_glu_table: the function must return a %s tensor of its input's shape" % str(mid_dtype).replace("torch.", "")
    return v.float()


def _glu_operands(what, gate, up):
    gate, up = _levels_in(what, gate), _levels_in(what, up)
    assert gate.levels.dim() >= 1 and tuple(gate.shape) == tuple(up.shape), \
        "%s needs gate and up of one shape [.., C], got %s and %s" % (what, tuple(gate.shape), tuple(up.shape))
    return gate.levels, up.levels, up.scale, up.zero_point


def lsq_glu_w8_q(gate: LevelsTensor, up: LevelsTensor, table: Tensor, out_scale: Tensor = None, out_shift: Tensor = None,
                 out_quant_min: int = None, out_quant_max: int = None, out_type_min: int = None, out_type_max: int = None,
                 mid_dtype=torch.float32) -> LevelsTensor:
    """The gated product of a gated MLP on 8-bit levels with an 8-bit output, `act(gate) * up`: gate and up are `LevelsTensor`s
    of one shape [.., C], with quantizers and level dtypes of their own, `table` is `lsq_glu_table`'s for gate's quantizer.
    Per element a = table[gate byte], d = up.dequantize(mid_dtype), one rounded product, the output quantizer's levels -- ONE
    launch (liblsq_hip_glu_w8.so), two bytes read and one written per element, nothing read back.  Each operand is read in place
    where its innermost stride is 1 and its leading axes share one row stride: the halves `gu[..., :C]` and `gu[..., C:]` of a
    fused gate_up linear's output are not copied.  Returns a dense `LevelsTensor` of that shape.  Inference only."""
    _assert_has_ops()
    what = "lsq_glu_w8_q"
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, False)
    lv = torch.ops.torchlsq.lsq_glu_w8_q8_q(*_glu_operands(what, gate, up), table, *o[:6], mid_dtype)
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_glu_w8(gate: LevelsTensor, up: LevelsTensor, table: Tensor, out_dtype=torch.float32) -> Tensor:
    """`lsq_glu_w8_q` without an output quantizer: the products `round_to(out_dtype, table[gate byte] * up.dequantize(out_dtype))`
    as a dense floating tensor of the operands' shape.  Inference only."""
    _assert_has_ops()
    return torch.ops.torchlsq.lsq_glu_w8_q8(*_glu_operands("lsq_glu_w8", gate, up), table, out_dtype)


def lsq_glu_act_w8_q(gate: LevelsTensor, up: LevelsTensor, fn, out_scale: Tensor = None, out_shift: Tensor = None,
                     out_quant_min: int = None, out_quant_max: int = None, out_type_min: int = None, out_type_max: int = None,
                     act_out=None, mid_dtype=torch.float32) -> LevelsTensor:
    """`lsq_glu_w8_q` for an activation given as in `act_function`: bit for bit `lsq_levels_per_tensor(fn(gate.dequantize(
    mid_dtype)) * up.dequantize(mid_dtype), output quantizer)` on the operands' device.  THIS FUNCTION BUILDS THE TABLE ON EVERY
    CALL (`lsq_glu_table`: a handful of launches on 256 elements) before the one launch of `lsq_glu_w8_q`;
    `torchlsq.quantized.GLUW8Q` builds it once, at conversion.  Inference only."""
    gate = _levels_in("lsq_glu_act_w8_q", gate)
    table = lsq_glu_table(fn, gate.scale, gate.zero_point, gate.levels.dtype, act_out, mid_dtype)
    return lsq_glu_w8_q(gate, up, table, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, mid_dtype)


def _norm_rows(what, x, weight, bias, normalized_shape, dim):
    """(levels whose LAST axis is the normalised one, as a dense view where x's memory allows it; weight and bias flattened; the
    way back to x's shape and memory format)"""
    x = _levels_in(what, x)
    lv = x.levels
    if dim in (1, -3) and lv.dim() == 4:
        # channels-last memory: [B, H, W, C] is a dense view, C per pixel is the trailing axis
        assert normalized_shape is None or tuple(normalized_shape) == (lv.shape[1],), \
            "%s: dim=1 normalises over the %d channels, got normalized_shape %s" % (what, lv.shape[1], tuple(normalized_shape))
        rows, back = lv.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1), lambda y: y.permute(0, 3, 1, 2)
    else:
        assert dim in (-1, lv.dim() - 1), \
            "%s: dim must be -1 (the trailing axes) or 1 for a 4-D levels tensor in channels-last memory (C per pixel), got dim=%r for %d " \
            "dims" % (what, dim, lv.dim())
        n = 1 if normalized_shape is None else len(tuple(normalized_shape))
        assert 1 <= n <= lv.dim() and (normalized_shape is None or tuple(normalized_shape) == tuple(lv.shape[-n:])), \
            "%s: normalized_shape %s is not the trailing shape of %s" % (what, normalized_shape, tuple(lv.shape))
        shape = tuple(lv.shape)
        rows, back = lv.contiguous().reshape(shape[:len(shape) - n] + (-1,)), lambda y: y.reshape(shape)
    w = None if weight is None else weight.detach().reshape(-1)
    b = None if bias is None else bias.detach().reshape(-1)
    return x, rows, w, b, back


def _norm_w8_q(op, what, x, weight, bias, eps, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, mid_dtype,
               normalized_shape, dim):
    _assert_has_ops()
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, False)
    x, rows, w, b, back = _norm_rows(what, x, weight, bias, normalized_shape, dim)
    lv = op(rows, x.scale, x.zero_point, w, b, float(eps), *o[:6], mid_dtype)
    return _levels_out(back(lv), o[0], o[1], o[2:6])


def _norm_w8(op, what, x, weight, bias, eps, out_dtype, normalized_shape, dim):
    _assert_has_ops()
    x, rows, w, b, back = _norm_rows(what, x, weight, bias, normalized_shape, dim)
    return back(op(rows, x.scale, x.zero_point, w, b, float(eps), out_dtype))


def lsq_layer_norm_w8_q(x: LevelsTensor, weight: Tensor = None, bias: Tensor = None, eps: float = 1e-5, out_scale: Tensor = None,
                        out_shift: Tensor = None, out_quant_min: int = None, out_quant_max: int = None, out_type_min: int = None,
                        out_type_max: int = None, mid_dtype=torch.float32, normalized_shape=None, dim: int = -1) -> LevelsTensor:
    """LayerNorm on 8-bit levels with an 8-bit output, one launch (liblsq_hip_norm_w8.so): one byte read and one written per
    activation, nothing read back.  The row statistics are EXACT integers of the levels (and do not depend on the zero point):
    S1 = sum b, S2 = sum b^2, V = C S2 - S1^2, t = float(C b - S1) * ((1 / sqrt(float(V) / (C C) + eps / s_x^2)) / C), then
    `(t * weight) + bias` in float32, one rounding to `mid_dtype`, and the output quantizer's levels.  The CPU path is this
    definition in torch ops and the GPU equals it bit for bit.  IT IS NOT ATen's `layer_norm`: against
    `lsq_levels_per_tensor(F.layer_norm(x.dequantize()))` a small share of the levels differs by one.
    `dim=-1` normalises the trailing axis, or the trailing axes `normalized_shape` flattened (weight and bias of that shape);
    `dim=1` is for a 4-D levels tensor in channels-last memory and normalises over C per pixel (ConvNeXt's norm).  Returns a
    `LevelsTensor` in x's shape and memory format.  A constant row gives level(bias); with eps = 0 it gives quant_min (0 * inf).
    Inference only."""
    return _norm_w8_q(torch.ops.torchlsq.lsq_layer_norm_w8_q8_q, "lsq_layer_norm_w8_q", x, weight, bias, eps, out_scale, out_shift,
                      out_quant_min, out_quant_max, out_type_min, out_type_max, mid_dtype, normalized_shape, dim)


def lsq_layer_norm_w8(x: LevelsTensor, weight: Tensor = None, bias: Tensor = None, eps: float = 1e-5, out_dtype=torch.float32,
                      normalized_shape=None, dim: int = -1) -> Tensor:
    """`lsq_layer_norm_w8_q` without an output quantizer: the normalised values rounded once to `out_dtype`, as a floating tensor
    in x's shape and memory format.  Inference only."""
    return _norm_w8(torch.ops.torchlsq.lsq_layer_norm_w8_q8, "lsq_layer_norm_w8", x, weight, bias, eps, out_dtype, normalized_shape, dim)


def lsq_rms_norm_w8_q(x: LevelsTensor, weight: Tensor = None, bias: Tensor = None, eps: float = 1e-6, out_scale: Tensor = None,
                      out_shift: Tensor = None, out_quant_min: int = None, out_quant_max: int = None, out_type_min: int = None,
                      out_type_max: int = None, mid_dtype=torch.float32, normalized_shape=None, dim: int = -1) -> LevelsTensor:
    """RMSNorm on 8-bit levels with an 8-bit output, one launch: d = b - zero_point, Q = sum d^2 (an exact integer),
    t = float(d) * (1 / sqrt(float(Q) / C + eps / s_x^2)), then as `lsq_layer_norm_w8_q`.  Inference only."""
    return _norm_w8_q(torch.ops.torchlsq.lsq_rms_norm_w8_q8_q, "lsq_rms_norm_w8_q", x, weight, bias, eps, out_scale, out_shift,
                      out_quant_min, out_quant_max, out_type_min, out_type_max, mid_dtype, normalized_shape, dim)


def lsq_rms_norm_w8(x: LevelsTensor, weight: Tensor = None, bias: Tensor = None, eps: float = 1e-6, out_dtype=torch.float32,
                    normalized_shape=None, dim: int = -1) -> Tensor:
    """`lsq_rms_norm_w8_q` without an output quantizer: floats of `out_dtype` in x's shape and memory format.  Inference only."""
    return _norm_w8(torch.ops.torchlsq.lsq_rms_norm_w8_q8, "lsq_rms_norm_w8", x, weight, bias, eps, out_dtype, normalized_shape, dim)


def _bmm_w8_args(what, a, b, transpose_b):
    a, b = _levels_in(what, a), _levels_in(what, b)
    squeeze = []
    la, lb = a.levels, b.levels
    if la.dim() == 1:
        la, squeeze = la.contiguous().unsqueeze(0), squeeze + [-2]
    if lb.dim() == 1:
        lb = lb.contiguous().unsqueeze(0 if transpose_b else -1)
        squeeze = squeeze + [-1]
    assert la.dim() == lb.dim() or la.dim() == 2 or lb.dim() == 2, \
        "%s: a and b need the same batch axes (they are not broadcast), got %s and %s" % (what, tuple(a.shape), tuple(b.shape))
    if la.dim() < lb.dim():         # a 2-D operand beside a batched one is repeated as a view: a zero batch stride
        la = la.expand(tuple(lb.shape[:-2]) + tuple(la.shape))
    elif lb.dim() < la.dim():
        lb = lb.expand(tuple(la.shape[:-2]) + tuple(lb.shape))
    return (la, a.scale, a.zero_point, lb, b.scale, b.zero_point, bool(transpose_b)), squeeze


def _squeeze(y, dims):
    """drops the axes a 1-D operand added: -1 is N (b was 1-D), -2 is M (a was 1-D)"""
    if -1 in dims:
        y = y.squeeze(-1)
    if -2 in dims:
        y = y.squeeze(-1 if -1 in dims else -2)
    return y


def lsq_bmm_w8_q(a: LevelsTensor, b: LevelsTensor, transpose_b: bool = False, out_scale: Tensor = None, out_shift: Tensor = None,
                 out_quant_min: int = None, out_quant_max: int = None, out_type_min: int = None, out_type_max: int = None,
                 mid_dtype=torch.float32, out: Tensor = None) -> LevelsTensor:
    """A batched matmul of two `LevelsTensor`s with an 8-bit output, one launch (liblsq_hip_attn_w8.so): a [.., M, K] times
    b [.., K, N], or b [.., N, K] with `transpose_b` (q k^T), up to two batch axes, the same on both sides; each operand uint8 or
    int8 with its own per-tensor constants.  I = sum_k (la - za)(lb - zb) is exact, v = (s_b * float(I)) * s_a two rounded float32
    multiplies -- `lsq_linear_w8a8`'s steps with b in the weight's role and no bias --, one rounding to `mid_dtype`, then the
    output quantizer's levels.  There is no alpha: the 1 / sqrt(D) of attention goes into `lsq_softmax_table` or is absorbed by
    the scores' quantizer.  The CPU path is this definition in torch ops and the GPU equals it bit for bit.

    THE OPERANDS ARE READ IN PLACE where their innermost stride is 1: a `qkv.view(B, T, 3, H, D)[:, :, i].permute(0, 2, 1, 3)` view,
    probabilities with padded rows (`lsq_softmax_w8_q(row_pad=16)`).  On the GPU, bases and strides that are multiples of 16 run on
    the matrix cores (K, or N of a [.., K, N] b, need not be a multiple of 16); anything else legal takes a generic kernel.  A 1-D
    operand (taken as `torch.matmul` takes it), a view without unit innermost stride, or one whose rows overlap (an expanded or
    sliding-window view) IS MADE DENSE FIRST.  `out`: a uint8 / int8 tensor [.., M, N] with unit innermost stride and rows that do
    not overlap to write into, e.g. the [B, H, T, D] view of a [B, T, H D] buffer; bytes outside it are not written.  WITH `out` THE
    CALL GOES TO THE HOST FUNCTION DIRECTLY, not through `torch.ops.torchlsq.lsq_bmm_w8_q8_q` (an op returns a fresh tensor): the same
    checks and kernels run, but the op's fake kernel and its Autograd kernel that refuses grad do not.  Returns a `LevelsTensor` whose constants are formed on the device.  Inference only."""
    _assert_has_ops()
    what = "lsq_bmm_w8_q"
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, False)
    args, squeeze = _bmm_w8_args(what, a, b, transpose_b)
    if out is None:
        lv = torch.ops.torchlsq.lsq_bmm_w8_q8_q(*args, *o[:6], mid_dtype)
    else:
        from .extension import attn_w8_bmm_q
        assert not squeeze, "%s: `out` is not served with a 1-D operand" % what
        lv = attn_w8_bmm_q(*args, *o[:6], mid_dtype, out=out)
    return _levels_out(_squeeze(lv, squeeze), o[0], o[1], o[2:6])


def lsq_bmm_w8(a: LevelsTensor, b: LevelsTensor, transpose_b: bool = False, out_dtype=torch.float32) -> Tensor:
    """`lsq_bmm_w8_q` without an output quantizer: `round_to(out_dtype, (s_b * float(I)) * s_a)` as a floating tensor [.., M, N].
    A 1-D operand, a view without unit innermost stride, or one whose rows overlap is made dense first.  Inference only."""
    _assert_has_ops()
    args, squeeze = _bmm_w8_args("lsq_bmm_w8", a, b, transpose_b)
    return _squeeze(torch.ops.torchlsq.lsq_bmm_w8_q8(*args, out_dtype), squeeze)


def lsq_softmax_table(x_scale: Tensor, alpha: float = 1.0) -> Tensor:
    """The 256-entry table (int32 [256], on `x_scale`'s device) of `lsq_softmax_w8_q` for levels of a per-tensor quantizer with the
    scale `x_scale` (a `LevelsTensor.scale`), built from existing torch ops, nothing read back.  In float64:

        table[d] = int32(rint(exp(-(float64(s_x) * float64(float32(alpha))) * d) * 2^24)),   d = 0 .. 255

    so table[0] = 2^24 and the entries do not increase.  `alpha` carries attention's 1 / sqrt(D).  A float64 exp may differ in its
    last place between devices, hence an entry by 1: for equal results on two devices build the table once and move it."""
    a = float(torch.tensor(float(alpha), dtype=torch.float32))
    t = x_scale.detach().reshape(-1)[:1].to(torch.float64) * a
    d = torch.arange(256, dtype=torch.float64, device=x_scale.device)
    return torch.round(torch.exp(-t * d) * float(1 << 24)).to(torch.int32)


def lsq_softmax_w8_q(x: LevelsTensor, table: Tensor, out_scale: Tensor = None, out_shift: Tensor = None, out_quant_min: int = None,
                     out_quant_max: int = None, out_type_min: int = None, out_type_max: int = None, mid_dtype=torch.float32,
                     out: Tensor = None, row_pad: int = 1) -> LevelsTensor:
    """Softmax over the last axis of 8-bit levels with an 8-bit output, one launch (liblsq_hip_attn_w8.so), no exp in the kernel:
    m = max b, E_i = table[m - b_i] (`lsq_softmax_table` for x's scale), S = sum E an EXACT integer with no summation order,
    p_i = float(E_i) * (1.0f / float(S)), one rounding to `mid_dtype`, then the output quantizer's levels.  x's scale and zero
    point are not read: they live in the table.  The CPU path is this definition in torch ops and the GPU equals it bit for bit for
    the same table.  IT IS NOT ATen's `softmax`: against `lsq_levels_per_tensor(F.softmax(alpha * x.dequantize()))` at most one
    level differs.  x is read in place where its innermost stride is 1 and its rows lie one stride apart (else
    it is made dense first).  `row_pad=16` allocates the result with rows padded to a multiple of 16 bytes and returns the
    [.., :C] view, so that a following `lsq_bmm_w8_q` runs on the matrix cores for any C; `out`: a tensor of x's shape to write
    into instead -- that call goes to the host function directly, not through `torch.ops.torchlsq.lsq_softmax_w8_q8_q`: the same
    checks and kernels, without the op's fake kernel and its Autograd kernel that refuses grad.  Returns a `LevelsTensor`.  Inference only."""
    _assert_has_ops()
    what = "lsq_softmax_w8_q"
    x = _levels_in(what, x)
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, False)
    if out is None:
        lv = torch.ops.torchlsq.lsq_softmax_w8_q8_q(x.levels, table, *o[:6], mid_dtype, int(row_pad))
    else:
        from .extension import attn_w8_softmax_q
        lv = attn_w8_softmax_q(x.levels, table, *o[:6], mid_dtype, 1, out=out)
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_attention_w8_q(q: LevelsTensor, k: LevelsTensor, v: LevelsTensor, table: Tensor, scores_out, probs_out, out,
                       mid_dtype=torch.float32) -> LevelsTensor:
    """The attention core softmax(q k^T) v on 8-bit levels with an 8-bit output IN ONE LAUNCH (liblsq_hip_attn_fused_w8.so): q
    [B, H, Tq, D], k and v [B, H, Tk, D] `LevelsTensor`s (views of one qkv buffer are read in place), `table` the softmax's
    (`lsq_softmax_table` of the scores' scale and alpha), and the three output sides `scores_out`, `probs_out`, `out`, each the
    6-tuple (scale, shift, quant_min, quant_max, type_min, type_max) of a per-tensor quantizer as `MatmulW8Q._out()` yields it.
    There is no new arithmetic: the result is, byte for byte,

        s = lsq_bmm_w8_q(q, k, True, *scores_out, mid_dtype);  p = lsq_softmax_w8_q(s, table, *probs_out, mid_dtype)
        y = lsq_bmm_w8_q(p, v, False, *out, mid_dtype, out=<the [B, H, Tq, D] view of a [B, Tq, H D] buffer>)

    returned as a `LevelsTensor` [B, Tq, H D] of `out`'s quantizer.  On the GPU the scores and probabilities are bytes in LDS and
    never reach memory where q, k, v have 16-byte aligned bases and strides that are multiples of 16, D % 16 == 0, 16 <= D <= 128 and
    Tk <= 2048 (`torchlsq.extension.attn_fused_w8_plan` says which); every other input the three ops serve runs those three
    launches.  The CPU path is the composition above and the GPU equals it bit for bit.  Inference only."""
    _assert_has_ops()
    what = "lsq_attention_w8_q"
    q, k, v = _levels_in(what, q), _levels_in(what, k), _levels_in(what, v)
    sides = []
    for name, side in (("scores_out", scores_out), ("probs_out", probs_out), ("out", out)):
        assert side is not None and len(side) == 6, "%s: %s must be (scale, shift, quant_min, quant_max, type_min, type_max)" % (what, name)
        sides.append(_out_args("%s (%s)" % (what, name), *side, False))
    lv = torch.ops.torchlsq.lsq_attention_w8_q8_q(q.levels, q.scale, q.zero_point, k.levels, k.scale, k.zero_point, v.levels, v.scale,
                                                  v.zero_point, table, *sides[0][:6], *sides[1][:6], *sides[2][:6], mid_dtype)
    o = sides[2]
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_softmax_w8(x: LevelsTensor, table: Tensor, out_dtype=torch.float32) -> Tensor:
    """`lsq_softmax_w8_q` without an output quantizer: the probabilities rounded once to `out_dtype`, in x's shape.
    Inference only."""
    _assert_has_ops()
    return torch.ops.torchlsq.lsq_softmax_w8_q8(_levels_in("lsq_softmax_w8", x).levels, table, out_dtype)


def _causal_args(what, x, causal):
    """(causal, causal_offset) of the ops from `causal`: None / False off, True the offset Tk - Tq, an int that offset"""
    if causal is None or causal is False:
        return False, 0
    assert x.levels.dim() >= 2, "%s: causal needs levels of at least 2 axes [.., Tq, Tk], got %s" % (what, tuple(x.shape))
    Tq, Tk = int(x.shape[-2]), int(x.shape[-1])
    if causal is True:
        assert Tk >= Tq, "%s: causal=True lets the last query see every key and needs Tk >= Tq, got Tq = %d and Tk = %d" % (what, Tq, Tk)
        return True, Tk - Tq
    assert isinstance(causal, int) and causal >= 0, "%s: causal must be None, a bool or an offset >= 0, got %r" % (what, causal)
    return True, int(causal)


def lsq_masked_softmax_w8_q(x: LevelsTensor, table: Tensor, out_scale: Tensor = None, out_shift: Tensor = None, out_quant_min: int = None,
                            out_quant_max: int = None, out_type_min: int = None, out_type_max: int = None, mid_dtype=torch.float32,
                            causal=None, key_lengths: Tensor = None, out: Tensor = None, row_pad: int = 1) -> LevelsTensor:
    """`lsq_softmax_w8_q` under a causal and / or a key-length mask, one launch (liblsq_hip_attn_mask_w8.so): x is [.., Tq, Tk]
    levels and row t of each [Tq, Tk] matrix sees its first

        n = min(Tk,  t + 1 + offset  where causal,  max(key_lengths[leading index], 0)  where key_lengths is given)

    keys.  `causal=True`: offset = Tk - Tq, the KV-cache convention -- the last query sees every key; the diagonal for Tq == Tk; it
    needs Tk >= Tq.  `causal=<int>`: that offset (>= 0).  `causal=None` / `False`: off.  `key_lengths`: an int32 tensor [x.shape[0]]
    on x's device (x then has at least 3 axes), read in the kernel and never on the host, so a captured graph follows it; values
    below 0 or above Tk are clamped.  The first n outputs of a row equal `lsq_softmax_w8_q` of that prefix BIT FOR BIT; the rest
    are the output quantizer's level of 0.  A row with n = 0 is all level-of-0 (ATen gives NaN).  Bytes of x beyond n are never
    looked at (unwritten KV-cache slots).  `out` and `row_pad` as in `lsq_softmax_w8_q`.  Inference only."""
    _assert_has_ops()
    what = "lsq_masked_softmax_w8_q"
    x = _levels_in(what, x)
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, False)
    on, off = _causal_args(what, x, causal)
    if out is None:
        lv = torch.ops.torchlsq.lsq_softmax_mask_w8_q8_q(x.levels, table, *o[:6], mid_dtype, on, off, key_lengths, int(row_pad))
    else:
        from .extension import attn_mask_w8_softmax_q
        lv = attn_mask_w8_softmax_q(x.levels, table, *o[:6], mid_dtype, on, off, key_lengths, 1, out=out)
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_attention_decode_w8_q(q: LevelsTensor, k: LevelsTensor, v: LevelsTensor, table: Tensor, scores_out, probs_out, out,
                              mid_dtype=torch.float32, causal=None, key_lengths: Tensor = None, split=None) -> LevelsTensor:
    """DECODE attention on 8-bit levels against a grouped-query KV cache, one launch (liblsq_hip_attn_decode_w8.so): q
    [B, H, Tq, D] `LevelsTensor` (a view of a qkv buffer is read in place) against k and v [B, Hkv, Tk, D] `LevelsTensor`s -- the
    cache buffers of `KVCacheW8`, read in place -- with Hkv dividing H: query head h reads kv head h // (H / Hkv), HF's `repeat_kv`.
    `table`, `scores_out`, `probs_out`, `out` and `mid_dtype` as in `lsq_attention_w8_q`; `causal` (None / False, True: the offset
    Tk - Tq, or an int offset >= 0) and `key_lengths` (int32 [B] on q's device, read in the kernel and never on the host, so a
    captured graph follows it) as in `lsq_masked_softmax_w8_q`.  Row (b, h, t) sees its first

        n = min(Tk,  t + 1 + offset  where causal,  max(key_lengths[b], 0)  where key_lengths is given)

    keys: its scores are `lsq_bmm_w8_q`'s bytes, its probabilities `lsq_masked_softmax_w8_q`'s bytes for that prefix, and the
    context sums (p_j - z_p)(lv_j - z_v) over j < n ALONE -- keys at or beyond n take no part and their bytes are never read; a
    row with n = 0 is `out`'s level of 0.0.  The result equals `AttentionCoreW8Q(causal=...)(q, k.repeat_interleave(G, 1),
    v.repeat_interleave(G, 1), key_lengths)` BIT FOR BIT whenever the probabilities quantizer's level of 0.0 equals its zero point
    as an operand (every quantizer with shift 0); where they differ, that route reads cache slots nobody wrote and this op does
    not.  On the GPU one workgroup takes a (b, kv head) and the H / Hkv heads share its k and v reads where (H / Hkv) Tq <= 16,
    D % 16 == 0, 16 <= D <= 128, Tk <= 8192 and q, k, v have 16-byte aligned bases and strides that are multiples of 16
    (`torchlsq.extension.attn_decode_w8_plan` says which); every other input runs the existing ops composed, with the same bytes.
    The CPU path is that composition and the GPU equals it bit for bit.  Returns a `LevelsTensor` [B, Tq, H D].  Inference only.

    `split` (opt-in; None: everything above, untouched) deals one kv head's keys to several workgroups
    (liblsq_hip_attn_decode_split_w8.so: three launches and a workspace allocated per call; served up to Tk = 65536) -- for small batches
    against long caches, where one workgroup per (b, kv head) leaves most of the part idle.  The bytes are the same for every value:
    every intermediate of the definition is a byte or an exact integer without a summation order.  An int >= 1 asks for at most that
    many splits (never more than one per 64 keys; 1 is legal); "auto" takes the split form, with the library's own chunk, where the
    single-launch kernel does not serve the shape but the split kernels do (Tk > 8192), or where B Hkv is at most the device's CU
    count (the largest grid at which the split form was measured to win: DESIGN.md 9.22) and Tk is at least two chunks, and
    today's path elsewhere (`torchlsq.extension.attn_decode_split_w8_plan(..., splits="auto")` says which)."""
    what = "lsq_attention_decode_w8_q"
    if split is None:
        return _attention_gqa_w8_q(what, torch.ops.torchlsq.lsq_attention_decode_w8_q8_q, q, k, v, table, scores_out, probs_out, out,
                                   mid_dtype, causal, key_lengths)
    assert split == "auto" or (isinstance(split, int) and not isinstance(split, bool) and split >= 1), \
        "%s: split must be None, \"auto\" or an int >= 1, got %r" % (what, split)
    ql, kl = _levels_in(what, q).levels, _levels_in(what, k).levels
    assert ql.dim() == 4 and kl.dim() == 4, "%s: q and k must have 4 axes, got %s and %s" % (what, tuple(ql.shape), tuple(kl.shape))
    if split == "auto":
        from ._attn_decode_split_w8_host import auto_splits
        cus = torch.cuda.get_device_properties(ql.device).multi_processor_count if ql.is_cuda else None
        vl = _levels_in(what, v).levels
        aligned = all(t.data_ptr() % 16 == 0 for t in (ql, kl, vl))
        strides = {n + "_strides": (t.stride(0), t.stride(1), t.stride(2)) for n, t in (("q", ql), ("k", kl), ("v", vl))}
        if not (vl.dim() == 4 and kl.numel() and ql.numel() and kl.shape[1] and ql.shape[1] % kl.shape[1] == 0 and
                auto_splits(ql.shape[0], ql.shape[1], kl.shape[1], ql.shape[2], kl.shape[2], ql.shape[3], cus, aligned, **strides)):
            return _attention_gqa_w8_q(what, torch.ops.torchlsq.lsq_attention_decode_w8_q8_q, q, k, v, table, scores_out, probs_out, out,
                                       mid_dtype, causal, key_lengths)
        splits = 0
    else:
        splits = max(1, min(split, (int(kl.shape[2]) + 63) // 64))
    return _attention_gqa_w8_q(what, torch.ops.torchlsq.lsq_attention_decode_split_w8_q8_q, q, k, v, table, scores_out, probs_out, out,
                               mid_dtype, causal, key_lengths, (splits,))


def _attention_gqa_w8_q(what, op, q, k, v, table, scores_out, probs_out, out, mid_dtype, causal, key_lengths, more=()):
    """the argument handling `lsq_attention_decode_w8_q` and `lsq_attention_prefill_w8_q` share, and the call of their op"""
    _assert_has_ops()
    q, k, v = _levels_in(what, q), _levels_in(what, k), _levels_in(what, v)
    sides = []
    for name, side in (("scores_out", scores_out), ("probs_out", probs_out), ("out", out)):
        assert side is not None and len(side) == 6, "%s: %s must be (scale, shift, quant_min, quant_max, type_min, type_max)" % (what, name)
        sides.append(_out_args("%s (%s)" % (what, name), *side, False))
    on, off = False, 0
    if causal is not None and causal is not False:
        assert q.levels.dim() == 4 and k.levels.dim() == 4, "%s: q and k must have 4 axes, got %s and %s" % (what, tuple(q.shape), tuple(k.shape))
        Tq, Tk = int(q.shape[2]), int(k.shape[2])
        if causal is True:
            assert Tk >= Tq, "%s: causal=True lets the last query see every key and needs Tk >= Tq, got Tq = %d and Tk = %d" % (what, Tq, Tk)
            on, off = True, Tk - Tq
        else:
            assert isinstance(causal, int) and causal >= 0, "%s: causal must be None, a bool or an offset >= 0, got %r" % (what, causal)
            on, off = True, int(causal)
    lv = op(q.levels, q.scale, q.zero_point, k.levels, k.scale, k.zero_point, v.levels, v.scale, v.zero_point, table, *sides[0][:6],
            *sides[1][:6], *sides[2][:6], mid_dtype, on, off, key_lengths, *more)
    o = sides[2]
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_attention_prefill_w8_q(q: LevelsTensor, k: LevelsTensor, v: LevelsTensor, table: Tensor, scores_out, probs_out, out,
                               mid_dtype=torch.float32, causal=None, key_lengths: Tensor = None) -> LevelsTensor:
    """PREFILL attention on 8-bit levels, one launch (liblsq_hip_attn_prefill_w8.so): the arguments, the `causal` conventions, the
    definition and the result of `lsq_attention_decode_w8_q` -- q [B, H, Tq, D] against k and v [B, Hkv, Tk, D] with Hkv dividing H,
    row (b, h, t) sees its first n = min(Tk, t + 1 + offset where causal, max(key_lengths[b], 0) where given) keys and nothing at or
    beyond n is read -- for ANY number of query rows.  On the GPU, in this order: where (H / Hkv) Tq <= 16 and the decode kernel
    serves the shape, that kernel (`lsq_attention_decode_w8_q` unchanged); else one launch of the prefill kernel -- a workgroup per
    (b, h, 64 query rows), the scores and the probabilities in LDS, every key loop ended at the largest n of its rows, so the work
    above the diagonal is not done and k and v are not repeated -- where D % 16 == 0, 16 <= D <= 128, q, k, v have 16-byte aligned
    bases and strides that are multiples of 16 and min(Tk, Tq + offset) (causal; else Tk) <= 2048
    (`torchlsq.extension.attn_prefill_w8_plan` says which; a long cache is served in place); every other input runs the existing
    ops composed.  The bytes are the same on every route: the CPU path is `lsq_attention_decode_w8_q`'s and the GPU equals it bit
    for bit.  Returns a `LevelsTensor` [B, Tq, H D].  Inference only."""
    return _attention_gqa_w8_q("lsq_attention_prefill_w8_q", torch.ops.torchlsq.lsq_attention_prefill_w8_q8_q, q, k, v, table, scores_out,
                               probs_out, out, mid_dtype, causal, key_lengths)


def lsq_masked_softmax_w8(x: LevelsTensor, table: Tensor, out_dtype=torch.float32, causal=None, key_lengths: Tensor = None) -> Tensor:
    """`lsq_masked_softmax_w8_q` without an output quantizer: the probabilities rounded once to `out_dtype`, +0.0 beyond a row's
    prefix, in x's shape.  Inference only."""
    _assert_has_ops()
    what = "lsq_masked_softmax_w8"
    x = _levels_in(what, x)
    on, off = _causal_args(what, x, causal)
    return torch.ops.torchlsq.lsq_softmax_mask_w8_q8(x.levels, table, out_dtype, on, off, key_lengths)


def lsq_rope_tables(dim: int, max_positions: int, base: float = 10000.0, mid_dtype=torch.float32, device=None):
    """The `(cos, sin)` tables of `lsq_rope_w8_q` for the rotary dimension `dim` (even) and the positions 0 .. `max_positions` - 1:
    float32 [P, dim / 2] on `device`, built in float64 from torch ops -- angle[p, i] = p * base^(-2 i / dim) --, taken to float32,
    rounded ONCE to `mid_dtype` and widened back, so that they hold values of `mid_dtype`.  Any other scheme (scaled, NTK, YaRN) is
    a table of the caller's with the same layout and rounding."""
    dim, P = int(dim), int(max_positions)
    assert dim >= 2 and dim % 2 == 0 and P >= 1, "lsq_rope_tables: dim must be even and at least 2, max_positions at least 1"
    assert mid_dtype in (torch.float32, torch.bfloat16, torch.float16), "lsq_rope_tables: mid_dtype must be float32, bfloat16 or float16"
    inv = torch.pow(torch.tensor(float(base), dtype=torch.float64, device=device),
                    -torch.arange(0, dim, 2, dtype=torch.float64, device=device) / dim)
    ang = torch.arange(P, dtype=torch.float64, device=device).reshape(P, 1) * inv.reshape(1, -1)
    return tuple(f(ang).to(torch.float32).to(mid_dtype).to(torch.float32).contiguous() for f in (torch.cos, torch.sin))


def _rope_operand(x):
    """x [B, T, H, D] as the ops take it"""
    assert x.levels.dim() == 4, "rotary embedding needs levels of [B, T, H, D], got %s" % (tuple(x.shape),)
    return x.levels, x.scale, x.zero_point


def lsq_rope_w8_q(x: LevelsTensor, cos: Tensor, sin: Tensor, out_scale: Tensor = None, out_shift: Tensor = None, out_quant_min: int = None,
                  out_quant_max: int = None, out_type_min: int = None, out_type_max: int = None, mid_dtype=torch.float32,
                  positions: Tensor = None, interleaved: bool = False, out: Tensor = None, scatter: bool = False) -> LevelsTensor:
    """Rotary position embedding on 8-bit levels with an 8-bit output, one launch (liblsq_hip_rope_w8.so): x [B, T, H, D] (a
    `qkv.view(B, T, 3, H, D)[:, :, i]` view is read in place), `cos` and `sin` from `lsq_rope_tables` for the SAME `mid_dtype`
    (float32 [P, R / 2]; R <= D: partial rotary, the features beyond R are only requantized), `positions` an int32 tensor [B] on x's
    device (None: zeros) that is read in the kernel and never on the host, so a captured graph follows it: token (b, t) has the
    position p = positions[b] + t.  Bit for bit HF's `x * cos + rotate_half(x) * sin` (`interleaved=True`: the pairs (2 i, 2 i + 1))
    evaluated with torch ops on `x.dequantize(mid_dtype)`, every product and sum rounded to `mid_dtype`, then
    `lsq_levels_per_tensor` of the output quantizer.  `out`: a uint8 / int8 tensor [B, Tout, H, D] with unit innermost stride to
    write into -- the `.permute(0, 2, 1, 3)` view of a [B, H, Tmax, D] cache is one --, token t at output token t or, with
    `scatter=True`, at output token p.  A TOKEN WITH p < 0 OR p >= P, OR WITH `scatter` p >= Tout, IS NOT WRITTEN AT ALL.  With
    `out` the call goes to the host function directly, not through `torch.ops.torchlsq.lsq_rope_w8_q8_q`.  Returns a `LevelsTensor`
    (with `out`: on that view).  Inference only."""
    _assert_has_ops()
    what = "lsq_rope_w8_q"
    x = _levels_in(what, x)
    o = _out_args(what, out_scale, out_shift, out_quant_min, out_quant_max, out_type_min, out_type_max, False)
    if out is None:
        assert not scatter, "%s: scatter needs `out`" % what
        lv = torch.ops.torchlsq.lsq_rope_w8_q8_q(*_rope_operand(x), cos, sin, *o[:6], mid_dtype, positions, bool(interleaved))
    else:
        from .extension import rope_w8_q
        lv = rope_w8_q(*_rope_operand(x), cos, sin, *o[:6], mid_dtype, positions, bool(interleaved), out=out, scatter=scatter)
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_rope_w8(x: LevelsTensor, cos: Tensor, sin: Tensor, out_dtype=torch.float32, positions: Tensor = None,
                interleaved: bool = False) -> Tensor:
    """`lsq_rope_w8_q` without an output quantizer: the rotated values as `out_dtype` floats [B, T, H, D] (the tables hold values of
    `out_dtype`).  Inference only."""
    _assert_has_ops()
    x = _levels_in("lsq_rope_w8", x)
    return torch.ops.torchlsq.lsq_rope_w8_q8(*_rope_operand(x), cos, sin, out_dtype, positions, bool(interleaved))


def lsq_kv_append_w8(x: LevelsTensor, out: Tensor, positions: Tensor = None, scatter: bool = True) -> LevelsTensor:
    """The KV-cache append on 8-bit levels, one launch and no arithmetic (liblsq_hip_rope_w8.so, COPY): x's levels [B, T, H, D] (v,
    or a k that is rotated already) into `out` [B, Tout, H, D] of the same dtype -- the `.permute(0, 2, 1, 3)` view of a
    [B, H, Tmax, D] cache --, token t at output token `positions[b] + t` (`scatter=False`: at t).  `positions` is int32 [B] on x's
    device and read in the kernel.  A token whose position lies outside 0 .. Tout - 1 is not written.  Returns `out` as a
    `LevelsTensor` with x's constants.  Inference only."""
    _assert_has_ops()
    x = _levels_in("lsq_kv_append_w8", x)
    assert x.levels.dim() == 4, "lsq_kv_append_w8 needs levels of [B, T, H, D], got %s" % (tuple(x.shape),)
    torch.ops.torchlsq.lsq_kv_copy_w8(x.levels, out, positions, bool(scatter))
    return LevelsTensor(out, x.scale, x.zero_point, x.quant_min, x.quant_max, x.type_min, x.type_max)


def lsq_kv_gather_paged_w8(pool: LevelsTensor, block_table: Tensor) -> LevelsTensor:
    """The dense cache a block table names: `pool` a `LevelsTensor` [Np, Hkv, ps, D] (any view with unit innermost
    stride), `block_table` int32 [B, Mp] on its device -> a `LevelsTensor` [B, Hkv, Mp ps, D] with

        result[b, hkv, j, :] = pool[clamp(block_table[b, j // ps], 0, Np - 1), hkv, j % ps, :]

    in torch ops, nothing is read back.  It is the DEFINITION of the paged layout, the route a paged user had before
    `lsq_attention_decode_paged_w8_q`, and the way back to a dense cache.  Inference only."""
    _assert_has_ops()
    pool = _levels_in("lsq_kv_gather_paged_w8", pool)
    return LevelsTensor(_E.kv_gather_paged_w8(pool.levels, block_table), pool.scale, pool.zero_point, pool.quant_min, pool.quant_max,
                        pool.type_min, pool.type_max)


def lsq_attention_decode_paged_w8_q(q: LevelsTensor, k_pool: LevelsTensor, v_pool: LevelsTensor, block_table: Tensor, table: Tensor,
                                    scores_out, probs_out, out, mid_dtype=torch.float32, causal=None, key_lengths: Tensor = None,
                                    splits: int = 0) -> LevelsTensor:
    """DECODE attention on 8-bit levels against a PAGED KV cache (liblsq_hip_attn_paged_w8.so): q [B, H, Tq, D] `LevelsTensor` against
    the pools `k_pool` and `v_pool`, `LevelsTensor`s [Np, Hkv, ps, D] (Hkv dividing H; any view with unit innermost stride, so the
    storage order [Np, ps, Hkv, D] too) through `block_table`, int32 [B, Mp] on their device, read in the kernels and never on the
    host, so a captured graph follows it.  The logical capacity is Tk = Mp ps <= 65536 keys and key j of batch entry b lies in page
    clamp(block_table[b, j // ps], 0, Np - 1) at slot j % ps: READS CLAMP, a wrong entry never leaves the pool.  The result is

        lsq_attention_decode_w8_q(q, lsq_kv_gather_paged_w8(k_pool, block_table), lsq_kv_gather_paged_w8(v_pool, block_table), ...)

    BIT FOR BIT, with the same `table`, sides, `mid_dtype`, `causal` (True: the offset Tk - Tq with this Tk) and `key_lengths` -- and
    that IS the CPU path.  Entries at logical pages at or beyond ceil(n / ps) and pool bytes at keys at or beyond a batch entry's
    largest key count are never read.  On the GPU no page is copied where (H / Hkv) Tq <= 16, D % 16 == 0, 16 <= D <= 128, ps is a power
    of two >= 16 and q and the pools have 16-byte aligned bases and strides that are multiples of 16: the three launches of the
    split-key decode with a workspace allocated per call (`torchlsq.extension.attn_paged_w8_plan` says which); every other input is
    gathered and composed, with the same bytes.  `splits`: 0 the library's own chunk, s >= 1 at most s splits (clamped to one per 64
    keys); the bytes are the same for every value.  Returns a `LevelsTensor` [B, Tq, H D].  Inference only."""
    what = "lsq_attention_decode_paged_w8_q"
    _assert_has_ops()
    q, k_pool, v_pool = _levels_in(what, q), _levels_in(what, k_pool), _levels_in(what, v_pool)
    assert isinstance(splits, int) and not isinstance(splits, bool) and splits >= 0, "%s: splits must be an int >= 0, got %r" % (what, splits)
    assert q.levels.dim() == 4 and k_pool.levels.dim() == 4 and block_table.dim() == 2, \
        "%s: q must be [B, H, Tq, D], the pools [Np, Hkv, ps, D] and block_table [B, Mp], got %s, %s and %s" \
        % (what, tuple(q.shape), tuple(k_pool.shape), tuple(block_table.shape))
    sides = []
    for name, side in (("scores_out", scores_out), ("probs_out", probs_out), ("out", out)):
        assert side is not None and len(side) == 6, "%s: %s must be (scale, shift, quant_min, quant_max, type_min, type_max)" % (what, name)
        sides.append(_out_args("%s (%s)" % (what, name), *side, False))
    Tq, Tk = int(q.shape[2]), int(block_table.shape[1]) * int(k_pool.shape[2])
    on, off = False, 0
    if causal is not None and causal is not False:
        if causal is True:
            assert Tk >= Tq, "%s: causal=True lets the last query see every key and needs Mp ps >= Tq, got Tq = %d and %d" % (what, Tq, Tk)
            on, off = True, Tk - Tq
        else:
            assert isinstance(causal, int) and causal >= 0, "%s: causal must be None, a bool or an offset >= 0, got %r" % (what, causal)
            on, off = True, int(causal)
    splits = min(splits, (Tk + 63) // 64)
    lv = torch.ops.torchlsq.lsq_attention_decode_paged_w8_q8_q(q.levels, q.scale, q.zero_point, k_pool.levels, k_pool.scale, k_pool.zero_point,
                                                               v_pool.levels, v_pool.scale, v_pool.zero_point, block_table, table,
                                                               *sides[0][:6], *sides[1][:6], *sides[2][:6], mid_dtype, on, off, key_lengths,
                                                               splits)
    o = sides[2]
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_attention_chunk_w8_q(q: LevelsTensor, k: LevelsTensor, v: LevelsTensor, table: Tensor, scores_out, probs_out, out,
                             mid_dtype=torch.float32, causal=None, key_lengths: Tensor = None, block_table: Tensor = None,
                             splits: int = 0) -> LevelsTensor:
    """CHUNKED PREFILL attention on 8-bit levels (liblsq_hip_attn_chunk_w8.so): the arguments, the definition and the
    result of `lsq_attention_decode_w8_q` -- q [B, H, Tq, D] against k and v [B, Hkv, Tk, D] with Hkv dividing H, or, with a
    `block_table` (int32 [B, Mp]), against the POOLS [Np, Hkv, ps, D] of a paged cache as in `lsq_attention_decode_paged_w8_q`
    (Tk = Mp ps, READS CLAMP) -- for ANY number of query rows against up to 65536 keys.  `causal` is None / False, True (the offset
    Tk - Tq), an int offset >= 0, or "lengths":

        L_b = min(Tk, max(key_lengths[b], 0)),      n(b, t) = max(0, L_b - (Tq - 1 - t))

    -- the last query row of batch entry b sees its L_b keys, the row before it one fewer, a row whose count would be negative none
    (`out`'s level of 0.0).  It needs `key_lengths`, which is read in the kernels and never on the host: feed a prompt in pieces into
    a growing cache with the lengths `KVCacheW8.append` / `PagedKVCacheW8.append` return and one captured graph serves every piece.
    With Tq = 1 it is `causal=True` with `key_lengths`.  Keys at or beyond n take no part and are never read.  On the GPU: three
    launches -- those of the split-key decode with the (H / Hkv) Tq rows of a kv head dealt to row tiles of 16, every tile's key loops
    ended at its own largest n -- and a workspace allocated per call of

        B Hkv R ldw + 8 B Hkv S R D bytes,     R = (H / Hkv) Tq,  ldw = 16 ceil(Tk / 16)  (paged: Mp ps),  S the splits

    (large in R: 512 tokens x 4 heads a kv head x 32768 keys are 64 MB per kv head) where D % 16 == 0, 16 <= D <= 128, ps is a power
    of two >= 16 and q, k, v have 16-byte aligned bases and strides that are multiples of 16 (`torchlsq.extension.attn_chunk_w8_plan`
    / `attn_chunk_paged_w8_plan` say which); every other input is (gathered and) composed from the existing ops, with the same bytes.
    `splits`: 0 the library's own chunk, s >= 1 at most s splits of the keys (clamped to one per 64 keys); the bytes are the same for
    every value.  The CPU path is that composition.  Returns a `LevelsTensor` [B, Tq, H D].  Inference only."""
    what = "lsq_attention_chunk_w8_q"
    _assert_has_ops()
    q, k, v = _levels_in(what, q), _levels_in(what, k), _levels_in(what, v)
    assert isinstance(splits, int) and not isinstance(splits, bool) and splits >= 0, "%s: splits must be an int >= 0, got %r" % (what, splits)
    assert q.levels.dim() == 4 and k.levels.dim() == 4 and (block_table is None or block_table.dim() == 2), \
        "%s: q must be [B, H, Tq, D], k and v [B, Hkv, Tk, D] (pools [Np, Hkv, ps, D] with a block_table [B, Mp]), got %s and %s" \
        % (what, tuple(q.shape), tuple(k.shape))
    sides = []
    for name, side in (("scores_out", scores_out), ("probs_out", probs_out), ("out", out)):
        assert side is not None and len(side) == 6, "%s: %s must be (scale, shift, quant_min, quant_max, type_min, type_max)" % (what, name)
        sides.append(_out_args("%s (%s)" % (what, name), *side, False))
    Tq = int(q.shape[2])
    Tk = int(k.shape[2]) if block_table is None else int(block_table.shape[1]) * int(k.shape[2])
    mode, off = 0, 0
    if isinstance(causal, str):
        assert causal == "lengths", "%s: causal must be None, a bool, an offset >= 0 or \"lengths\", got %r" % (what, causal)
        assert key_lengths is not None, "%s: causal=\"lengths\" counts every row's keys back from key_lengths and needs them" % what
        mode = 2
    elif causal is True:
        assert Tk >= Tq, "%s: causal=True lets the last query see every key and needs Tk >= Tq, got Tq = %d and Tk = %d" % (what, Tq, Tk)
        mode, off = 1, Tk - Tq
    elif causal is not None and causal is not False:
        assert isinstance(causal, int) and causal >= 0, "%s: causal must be None, a bool, an offset >= 0 or \"lengths\", got %r" % (what, causal)
        mode, off = 1, int(causal)
    splits = min(splits, (Tk + 63) // 64)
    head = (q.levels, q.scale, q.zero_point, k.levels, k.scale, k.zero_point, v.levels, v.scale, v.zero_point)
    tail = (table, *sides[0][:6], *sides[1][:6], *sides[2][:6], mid_dtype, mode, off, key_lengths, splits)
    if block_table is None:
        lv = torch.ops.torchlsq.lsq_attention_chunk_w8_q8_q(*head, *tail)
    else:
        lv = torch.ops.torchlsq.lsq_attention_chunk_paged_w8_q8_q(*head, block_table, *tail)
    o = sides[2]
    return _levels_out(lv, o[0], o[1], o[2:6])


def lsq_kv_append_paged_w8(k: LevelsTensor, v: LevelsTensor, k_pool: Tensor, v_pool: Tensor, block_table: Tensor, positions: Tensor = None):
    """The append into a PAGED KV cache, k and v in one launch and no arithmetic (liblsq_hip_attn_paged_w8.so): the levels of k and v
    [B, T, Hkv, D] (views of a qkv buffer are read in place; v, and a k that is rotated already) into the pools `k_pool` and `v_pool`
    [Np, Hkv, ps, D] of the same dtypes through `block_table` int32 [B, Mp]: token (b, t) at p = positions[b] + t (`positions`: int32
    [B] on the device, read in the kernel; None: zeros) goes to page block_table[b, p // ps], slot p % ps.  WRITES SKIP, they do not
    clamp: a token with p < 0, p >= Mp ps or an entry outside [0, Np) is not written at all.  Two tokens of one call that name the
    same physical slot are the caller's error (which bytes win is undefined).  Returns the pools as `LevelsTensor`s with k's and v's
    constants.  Inference only."""
    _assert_has_ops()
    what = "lsq_kv_append_paged_w8"
    k, v = _levels_in(what, k), _levels_in(what, v)
    assert k.levels.dim() == 4 and v.levels.dim() == 4, "%s needs levels of [B, T, Hkv, D], got %s and %s" % (what, tuple(k.shape), tuple(v.shape))
    k_pool, v_pool = (p.levels if isinstance(p, LevelsTensor) else p for p in (k_pool, v_pool))      # (the pools a previous append returned)
    torch.ops.torchlsq.lsq_kv_append_paged_w8(k.levels, v.levels, k_pool, v_pool, block_table, positions)
    return (LevelsTensor(k_pool, k.scale, k.zero_point, k.quant_min, k.quant_max, k.type_min, k.type_max),
            LevelsTensor(v_pool, v.scale, v.zero_point, v.quant_min, v.quant_max, v.type_min, v.type_max))
