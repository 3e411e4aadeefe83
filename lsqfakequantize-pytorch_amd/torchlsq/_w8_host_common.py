"""What the host layers of the ops on 8-bit levels say the same way: the status of a ctypes call, the checks of a quantizer's range,
of the per-tensor constants and of an output side ("levels out" through an output quantizer, or "floats out" as `mid_dtype`), the
CPU path's last step, and `out`.  The W8 host modules import these from here and not from whichever of them needed one first.
"""
import torch

from ._cpu_host import _require_cpu, cpu_levels
from ._hip_host import _check, _require_gpu

_LEVEL_CODE = {torch.uint8: 0, torch.int8: 1}       # LSQ_*_W8_U8 / _I8 of every level op's header
_FLOATS = (torch.float32, torch.bfloat16, torch.float16)


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _one(t, dtype):
    return t.dtype == dtype and t.numel() == 1


def _pair(what, name, v):
    v = tuple(int(e) for e in v) if isinstance(v, (tuple, list)) else (int(v),)
    _check(len(v) in (1, 2), "%s: %s must be one int or a pair of ints" % (what, name))
    return v * 2 if len(v) == 1 else v


def _status(rc, what, lib, last_error):
    """raise for the non-zero status `rc` of the call `what` into `lib`, with the message its `last_error` entry point holds"""
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, getattr(lib, last_error)().decode("utf-8", "replace")))


def _check_range(what, qmin, qmax, tmin, tmax):
    lo, hi = min(qmin, tmin), max(qmax, tmax)
    _check(qmin <= qmax and tmin <= tmax and ((lo >= 0 and hi <= 255) or (lo >= -128 and hi <= 127)),
           "%s: [quant_min, quant_max] = [%d, %d] and [type_min, type_max] = [%d, %d] must lie within 0..255 or within -128..127"
           % (what, qmin, qmax, tmin, tmax))
    return hi > 127


def _act_constants(scale, shift, tmin, tmax):
    """(s_x float32 [1], zx int32 [1]) as the per-tensor kernels derive them: max(|scale|, eps) and
    round(clamp(-shift * (1 / s), type range)) -- tensor ops on scale's device, nothing is read back"""
    s = scale.detach().reshape(-1)[:1].to(torch.float32).abs().clamp_min(torch.finfo(torch.float32).eps)
    b = shift.detach().reshape(-1)[:1].to(torch.float32)
    zp = torch.fmin(torch.full_like(s, tmax), torch.fmax(torch.full_like(s, tmin), -b * (1.0 / s))).round()
    return s, zp.to(torch.int32)


def _check_x_constants(what, s_x, zx):
    _check(_one(s_x, torch.float32) and _one(zx, torch.int32),
           "%s: x_scale must be one float32 value and x_zero one int32 value (tensors on the levels' device)" % what)


def _check_out_q(what, out_q, mid_dtype, where="the levels' device"):
    """(y's dtype, the range, the tensors of the output quantizer) after its checks; `out_q`: (out_scale, out_shift, quant_min,
    quant_max, type_min, type_max), or None for floats out"""
    _check(mid_dtype in _FLOATS, "%s: %s must be float32, bfloat16 or float16, got '%s'"
           % (what, "mid_dtype" if out_q else "out_dtype", _name(mid_dtype)))
    if not out_q:
        return mid_dtype, (0, 0, 0, 0), ()
    out_scale, out_shift, rng = out_q[0], out_q[1], tuple(int(v) for v in out_q[2:])
    unsigned = _check_range(what + " (output quantizer)", *rng)
    _check(_one(out_scale, torch.float32) and _one(out_shift, torch.float32),
           "%s: out_scale and out_shift must be float32 tensors of one value (a per-tensor quantizer) on %s" % (what, where))
    return (torch.uint8 if unsigned else torch.int8), rng, (out_scale, out_shift)


def _on_one_device(what, tensors):
    """True: all on the GPU; False: all on the CPU; anything else is refused"""
    on_gpu = any(t.is_cuda for t in tensors)
    if on_gpu:
        _require_gpu(what, *tensors)
    else:
        _require_cpu(what, *tensors)
    return on_gpu


def _cpu_finish(u, out_q, rng, ydt):
    """the CPU path's last step: u (a `mid_dtype` tensor) as the output quantizer's levels, or as it is"""
    if out_q:
        lv = cpu_levels(u, out_q[0].detach().reshape(-1), out_q[1].detach().reshape(-1), 0, False, *rng, 0)
        u = lv.view(torch.uint8) if ydt == torch.uint8 else lv
    return u


def _take_out(what, out, shape, dtype, device, memory_format=torch.contiguous_format):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device, memory_format=memory_format)
    _check(out.dtype == dtype and tuple(out.shape) == tuple(shape) and out.device == device and out.is_contiguous(memory_format=memory_format),
           "%s: `out` must be a dense %s tensor of shape %s on x's device" % (what, _name(dtype), tuple(shape)))
    return out
