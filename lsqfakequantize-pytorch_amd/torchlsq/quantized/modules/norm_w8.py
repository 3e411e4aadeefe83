"""Normalisation modules that keep a converted block in 8-bit LEVELS at its norm: `LayerNormW8Q` (ConvNeXt's LayerNorm over C per
pixel, a token block's LayerNorm before qkv / fc1) and `RMSNormW8Q` -- `torchlsq.functional.lsq_layer_norm_w8_q` /
`lsq_rms_norm_w8_q`, liblsq_hip_norm_w8.so on the GPU: exact integer row statistics of the levels, one byte read and one written per
activation.  The forwards take `LevelsTensor`s (or per-tensor quantized tensors); nothing is read back to the host, and the chain can
be captured in a graph.  `convert_w8a8_norm(model, norms, channels_first=(), mid_dtype=...)` swaps the listed modules.

The result is the package's own definition (include/lsq_hip_norm_w8.h), not ATen's `layer_norm`: against the unfused
`dequantize -> F.layer_norm -> levels` a small share of the output levels differs by one.
"""
import copy

import torch
from torch import nn

from torchlsq.functional import LevelsTensor, lsq_layer_norm_w8, lsq_layer_norm_w8_q, lsq_rms_norm_w8, lsq_rms_norm_w8_q
from .packed_linear_a8 import _per_tensor_constants
from .w8a8_q import _MID_DTYPES, _as_levels

_PARAM_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_MAX_C = 65536
_RMS_NORM = getattr(nn, "RMSNorm", None)


class _NormW8Q(nn.Module):
    """what the two modules share.  Buffers: `weight` and `bias` (of `normalized_shape`, or empty when the norm has none),
    `output_scale` and `output_shift` (float32 [1]).  Extra state: `normalized_shape`, `eps`, the output range, `mid_dtype`,
    `dim` (-1: the trailing axes; 1: C per pixel of a 4-D channels-last tensor) and whether levels or floats come out."""
    _q = _f = None
    _default_eps = 1e-5

    def __init__(self, normalized_shape, eps=None, weight=True, bias=True, device=None, dtype=torch.float32, output_range=(0, 255, 0, 255),
                 mid_dtype=torch.float32, dim=-1, levels_out=True):
        super().__init__()
        assert mid_dtype in _MID_DTYPES.values(), "mid_dtype must be torch.float32, torch.bfloat16 or torch.float16"
        assert dtype in _PARAM_DTYPES, "weight and bias must be float32, bfloat16 or float16"
        assert dim in (-1, 1), "dim must be -1 (the trailing axes) or 1 (C per pixel of a 4-D channels-last tensor)"
        shape = (int(normalized_shape),) if isinstance(normalized_shape, int) else tuple(int(v) for v in normalized_shape)
        self.normalized_shape = shape
        self.eps = float(self._default_eps if eps is None else eps)
        self.register_buffer("weight", torch.ones(shape if weight else (0,), dtype=dtype, device=device))
        self.register_buffer("bias", torch.zeros(shape if bias else (0,), dtype=dtype, device=device))
        self.register_buffer("output_scale", torch.ones(1, dtype=torch.float32, device=device))
        self.register_buffer("output_shift", torch.zeros(1, dtype=torch.float32, device=device))
        self.output_range = tuple(int(v) for v in output_range)
        self.mid_dtype, self.dim, self.levels_out = mid_dtype, int(dim), bool(levels_out)

    def forward(self, x):
        x = _as_levels(x)
        assert isinstance(x, LevelsTensor), "%s reads levels: a LevelsTensor or a per-tensor quantized tensor" % type(self).__name__
        w = self.weight if self.weight.numel() else None
        b = self.bias if self.bias.numel() else None
        shape = None if self.dim == 1 else self.normalized_shape
        if not self.levels_out:
            return type(self)._f(x, w, b, self.eps, self.mid_dtype, shape, self.dim)
        return type(self)._q(x, w, b, self.eps, self.output_scale, self.output_shift, *self.output_range, self.mid_dtype, shape, self.dim)

    def get_extra_state(self):
        return dict(normalized_shape=list(self.normalized_shape), eps=self.eps, output_range=list(self.output_range),
                    mid_dtype=str(self.mid_dtype).replace("torch.", ""), dim=self.dim, levels_out=self.levels_out,
                    weight=bool(self.weight.numel()), bias=bool(self.bias.numel()))

    def set_extra_state(self, state):
        self.normalized_shape = tuple(int(v) for v in state["normalized_shape"])
        self.eps = float(state["eps"])
        self.output_range = tuple(int(v) for v in state["output_range"])
        self.mid_dtype = _MID_DTYPES[state["mid_dtype"]]
        self.dim, self.levels_out = int(state["dim"]), bool(state["levels_out"])

    def extra_repr(self):
        out = "output levels %d..%d" % self.output_range[:2] if self.levels_out else "floats out"
        return "%s, eps=%g, dim=%d, %s, mid_dtype=%s" % (self.normalized_shape, self.eps, self.dim, out,
                                                         str(self.mid_dtype).replace("torch.", ""))

    @classmethod
    def from_float(cls, norm, output_quantizer=None, mid_dtype=torch.float32, channels_first=False):
        """from a float norm module (`weight`, `bias`, `eps`, `normalized_shape`) and the trained per-tensor `LSQFakeQuantizer` of
        its output (None: the module returns floats of `mid_dtype`).  `channels_first`: the norm acts over C per pixel of a
        [B, C, H, W] tensor (ConvNeXt's LayerNorm2d), read from channels-last levels."""
        what = "%s.from_float" % cls.__name__
        shape = getattr(norm, "normalized_shape", None)
        assert shape is not None, "%s: the module has no normalized_shape" % what
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(v) for v in shape)
        n = 1
        for v in shape:
            n *= v
        assert 1 <= n <= _MAX_C, "%s: %d normalised elements per row, at most %d are served" % (what, n, _MAX_C)
        assert not channels_first or len(shape) == 1, "%s: a channels-first norm has a normalized_shape of one axis (C)" % what
        w, b = getattr(norm, "weight", None), getattr(norm, "bias", None)
        ref = w if w is not None else b
        assert ref is None or ref.dtype in _PARAM_DTYPES, "%s: weight and bias must be float32, bfloat16 or float16" % what
        device = ref.device if ref is not None else (output_quantizer.scale.device if output_quantizer is not None else None)
        eps = getattr(norm, "eps", None)
        m = cls(shape, eps, w is not None, b is not None, device, ref.dtype if ref is not None else torch.float32, mid_dtype=mid_dtype,
                dim=1 if channels_first else -1, levels_out=output_quantizer is not None)
        with torch.no_grad():
            if w is not None:
                m.weight.copy_(w.detach())
            if b is not None:
                m.bias.copy_(b.detach().to(m.bias.dtype))
        if output_quantizer is not None:
            scale, shift, *rng = _per_tensor_constants(output_quantizer, what + " (output quantizer)")
            dev = m.output_scale.device
            m.output_scale, m.output_shift, m.output_range = scale.to(dev), shift.to(dev), tuple(rng)
        m.train(norm.training)
        return m


class LayerNormW8Q(_NormW8Q):
    """`nn.LayerNorm` on a `LevelsTensor`: one launch, a `LevelsTensor` of the output quantizer (or floats) in x's shape and memory
    format.  Inference only."""
    _q, _f = staticmethod(lsq_layer_norm_w8_q), staticmethod(lsq_layer_norm_w8)
    _default_eps = 1e-5


class RMSNormW8Q(_NormW8Q):
    """`nn.RMSNorm` on a `LevelsTensor` (an absent eps is float32's machine epsilon, as torch takes it for float32 input).
    Inference only."""
    _q, _f = staticmethod(lsq_rms_norm_w8_q), staticmethod(lsq_rms_norm_w8)
    _default_eps = torch.finfo(torch.float32).eps


def convert_w8a8_norm(model, norms, channels_first=(), mid_dtype=torch.float32, inplace=False):
    """Replace the normalisation modules of `model`.  `norms` maps the qualified name of an `nn.LayerNorm` (or a subclass, such as a
    LayerNorm2d) or an `nn.RMSNorm` to the trained per-tensor `LSQFakeQuantizer` of its output -- it becomes a `LayerNormW8Q` /
    `RMSNormW8Q` that hands `LevelsTensor`s on -- or to None: the module then returns floats of `mid_dtype`.  Names listed in
    `channels_first` normalise over C per pixel of a [B, C, H, W] tensor (read from channels-last levels).  `mid_dtype`: the
    dtype in which the unfused model computed between the quantizers.  Anything else is refused by name.  Works beside the other
    `convert_w8a8_*` converters on disjoint names.  Returns the model (a deep copy unless inplace=True)."""
    assert mid_dtype in _MID_DTYPES.values(), "mid_dtype must be torch.float32, torch.bfloat16 or torch.float16"
    if not inplace:
        model = copy.deepcopy(model)
    modules = dict(model.named_modules())
    channels_first = set(channels_first)
    unknown = channels_first - set(norms)
    if unknown:
        raise ValueError("convert_w8a8_norm: channels_first names %s are not among the norms to convert" % sorted(unknown))
    swaps = []
    for name, quantizer in norms.items():
        child = modules.get(name)
        if isinstance(child, nn.LayerNorm):
            cls = LayerNormW8Q
        elif _RMS_NORM is not None and isinstance(child, _RMS_NORM):
            cls = RMSNormW8Q
        else:
            raise ValueError("convert_w8a8_norm: %r is not an nn.LayerNorm or nn.RMSNorm (got %s); GroupNorm and BatchNorm are not served"
                             % (name, type(child).__name__))
        try:
            swaps.append((name, cls.from_float(child, quantizer, mid_dtype, name in channels_first)))
        except AssertionError as e:
            raise ValueError("convert_w8a8_norm: %r cannot be served: %s" % (name, e)) from None
    for name, new in swaps:
        if name == "":
            return new
        parent_name, _, leaf = name.rpartition(".")
        setattr(modules[parent_name], leaf, new)
    return model
