"""Elementwise modules that keep a converted block in 8-bit LEVELS at its activation functions and at its squeeze-and-excitation
gate: `ActivationW8Q` (any elementwise function between two per-tensor quantizers as a 256-entry byte table, built once at
conversion) and `MulGateW8Q` (x * gate with the next quantizer's levels out, in the place of a `FloatFunctional`) --
`torchlsq.functional.lsq_act_table` / `lsq_lut_w8` / `lsq_mul_gate_w8_q`, liblsq_hip_eltwise_w8.so on the GPU.  The forwards take
`LevelsTensor`s (or per-tensor quantized tensors); nothing is read back to the host, and the chain can be captured in a graph.
`convert_w8a8_eltwise(model, activations, muls, mid_dtype=...)` swaps the listed modules.
"""
import copy

import torch
from torch import nn

from torchlsq.functional import LevelsTensor, _act_constants, act_function, lsq_act_table
from .packed_linear_a8 import _per_tensor_constants
from .w8a8_q import _MID_DTYPES, _as_levels

_ACT_MODULES = (nn.Identity, nn.ReLU, nn.ReLU6, nn.Hardtanh, nn.LeakyReLU, nn.Hardswish, nn.Hardsigmoid, nn.SiLU, nn.GELU, nn.Sigmoid,
                nn.Tanh)


def _level_dtype(rng):
    return torch.uint8 if max(rng[1], rng[3]) > 127 else torch.int8


class _EltwiseOutput(nn.Module):
    """what the two modules share: buffers `output_scale` and `output_shift` (float32 [1]); the output range and `mid_dtype` as
    extra state"""

    def _init_output(self, device, output_range, mid_dtype):
        assert mid_dtype in _MID_DTYPES.values(), "mid_dtype must be torch.float32, torch.bfloat16 or torch.float16"
        self.register_buffer("output_scale", torch.ones(1, dtype=torch.float32, device=device))
        self.register_buffer("output_shift", torch.zeros(1, dtype=torch.float32, device=device))
        self.output_range = tuple(int(v) for v in output_range)
        self.mid_dtype = mid_dtype

    def _set_output(self, output_quantizer, what):
        scale, shift, *rng = _per_tensor_constants(output_quantizer, what)
        device = self.output_scale.device
        self.output_scale, self.output_shift, self.output_range = scale.to(device), shift.to(device), tuple(rng)

    def _wrap(self, levels):
        s, z = _act_constants(self.output_scale, self.output_shift, self.output_range[2], self.output_range[3])   # on the device
        return LevelsTensor(levels, s, z, *self.output_range)

    def get_extra_state(self):
        return dict(output_range=list(self.output_range), mid_dtype=str(self.mid_dtype).replace("torch.", ""))

    def set_extra_state(self, state):
        self.output_range = tuple(int(v) for v in state["output_range"])
        self.mid_dtype = _MID_DTYPES[state["mid_dtype"]]

    def _output_repr(self):
        return "output levels %d..%d, mid_dtype=%s" % (self.output_range[0], self.output_range[1], str(self.mid_dtype).replace("torch.", ""))


class ActivationW8Q(_EltwiseOutput):
    """An activation function between two per-tensor 8-bit quantizers as a byte table: buffer `table` (uint8 [256], indexed by the
    input level's byte as stored), built ONCE by `from_float`; `forward(x)` is one launch, `table[x.levels]`, and returns a
    `LevelsTensor` of the output quantizer in x's shape and memory layout.  The function's name travels in the extra state for
    the record; the table is what computes.  Inference only."""

    def __init__(self, device=None, output_range=(0, 255, 0, 255), mid_dtype=torch.float32, function="identity"):
        super().__init__()
        self.register_buffer("table", torch.arange(256, dtype=torch.uint8, device=device))
        self._init_output(device, output_range, mid_dtype)
        self.function = str(function)

    def forward(self, x):
        x = _as_levels(x)
        assert isinstance(x, LevelsTensor), "ActivationW8Q reads levels: a LevelsTensor or a per-tensor quantized tensor"
        return self._wrap(torch.ops.torchlsq.lsq_lut_w8(x.levels, self.table, _level_dtype(self.output_range)))

    def get_extra_state(self):
        return dict(super().get_extra_state(), function=self.function)

    def set_extra_state(self, state):
        super().set_extra_state(state)
        self.function = str(state["function"])

    def extra_repr(self):
        return "%s, %s" % (self.function, self._output_repr())

    @classmethod
    def from_float(cls, act, input_quantizer, output_quantizer, mid_dtype=torch.float32, device=None):
        """from an activation (a name, a `torch.nn` activation module or a callable: `torchlsq.functional.act_function`) and the
        trained per-tensor `LSQFakeQuantizer`s of its input and of its output.  The table is built here, once, on `device`
        (default: the output quantizer's) from existing ops: build it on the device whose unfused chain it has to equal."""
        what = "ActivationW8Q.from_float"
        in_scale, in_shift, *in_rng = _per_tensor_constants(input_quantizer, what + " (input quantizer)")
        _per_tensor_constants(output_quantizer, what + " (output quantizer)")
        device = output_quantizer.scale.device if device is None else torch.device(device)
        _, name = act_function(act)
        m = cls(device, mid_dtype=mid_dtype, function=name)
        m._set_output(output_quantizer, what + " (output quantizer)")
        s, z = _act_constants(in_scale.to(device), in_shift.to(device), in_rng[2], in_rng[3])
        with torch.no_grad():
            m.table = lsq_act_table(act, s, z, _level_dtype(in_rng), m.output_scale, m.output_shift, *m.output_range, mid_dtype=mid_dtype)
        m.train(act.training if isinstance(act, nn.Module) else False)
        return m


def _is_gate(t, other):
    """whether `t` is the [B, C] / [B, C, 1, 1] gate of `other`"""
    ts, os_ = tuple(t.shape), tuple(other.shape)
    return len(os_) in (2, 4) and ts[:2] == os_[:2] and (len(ts) == 2 or (len(ts) == 4 and ts[2:] == (1, 1)))


class MulGateW8Q(_EltwiseOutput):
    """The squeeze-and-excitation multiply on `LevelsTensor`s, in the place of the `torch.ao.nn.quantized.FloatFunctional` of a
    quantizable SE block: `mul(a, b)` takes the activation [B, C, H, W] and its gate [B, C, 1, 1] (or [B, C]) in either order --
    torchvision writes `self.skip_mul.mul(self._scale(input), input)` -- and returns the `LevelsTensor` of its own output
    quantizer; `forward(x, gate)` is the same.  Inference only."""

    def __init__(self, device=None, output_range=(0, 255, 0, 255), mid_dtype=torch.float32):
        super().__init__()
        self._init_output(device, output_range, mid_dtype)

    def mul(self, a, b):
        a, b = _as_levels(a), _as_levels(b)
        if not (isinstance(a, LevelsTensor) and isinstance(b, LevelsTensor)):
            raise TypeError("MulGateW8Q needs two LevelsTensors (or per-tensor quantized tensors), got %s and %s"
                            % (type(a).__name__, type(b).__name__))
        if _is_gate(b, a):
            x, gate = a, b
        elif _is_gate(a, b):
            x, gate = b, a
        else:
            raise ValueError("MulGateW8Q needs an activation of [B, C, H, W] (or [B, C]) and its gate of [B, C, 1, 1] (or [B, C]), got %s "
                             "and %s" % (tuple(a.shape), tuple(b.shape)))
        lv = torch.ops.torchlsq.lsq_mul_gate_w8_q8_q(x.levels, x.scale, x.zero_point, gate.levels, gate.scale, gate.zero_point,
                                                     self.output_scale, self.output_shift, *self.output_range, self.mid_dtype)
        return self._wrap(lv)

    def forward(self, x, gate):
        return self.mul(x, gate)

    def extra_repr(self):
        return self._output_repr()

    @classmethod
    def from_float(cls, mod=None, output_quantizer=None, mid_dtype=torch.float32, device=None):
        """from the block's `FloatFunctional` (or None) and the trained per-tensor `LSQFakeQuantizer` of the product; the
        quantizer defaults to the FloatFunctional's `activation_post_process`"""
        what = "MulGateW8Q.from_float (output quantizer)"
        if output_quantizer is None:
            output_quantizer = getattr(mod, "activation_post_process", None)
        _per_tensor_constants(output_quantizer, what)
        m = cls(output_quantizer.scale.device if device is None else device, mid_dtype=mid_dtype)
        m._set_output(output_quantizer, what)
        m.train(mod.training if isinstance(mod, nn.Module) else False)
        return m


def convert_w8a8_eltwise(model, activations=None, muls=None, mid_dtype=torch.float32, inplace=False):
    """Replace the elementwise modules of `model`.  `activations` maps the qualified name of an activation module (`nn.ReLU`,
    `nn.ReLU6`, `nn.Hardtanh`, `nn.LeakyReLU`, `nn.Hardswish`, `nn.Hardsigmoid`, `nn.SiLU`, `nn.GELU`, `nn.Sigmoid`, `nn.Tanh`,
    `nn.Identity`) to the pair (input quantizer, output quantizer) of trained per-tensor `LSQFakeQuantizer`s around it: it becomes
    an `ActivationW8Q` whose table is built here, once, on the output quantizer's device.  `muls` maps the name of a
    `FloatFunctional` used as `.mul(x, gate)` to the quantizer of the product (None: its `activation_post_process`): it becomes a
    `MulGateW8Q`, so a quantizable SE block keeps its `forward`.  `mid_dtype`: the dtype in which the unfused model computed
    between the quantizers.  Anything else is refused by name.  Works beside `convert_w8a8_q` / `convert_w8a8_add_q` /
    `convert_w8a8_pool` / `convert_w8a8_depthwise` on disjoint names.  Returns the model (a deep copy unless inplace=True)."""
    assert mid_dtype in _MID_DTYPES.values(), "mid_dtype must be torch.float32, torch.bfloat16 or torch.float16"
    if not inplace:
        model = copy.deepcopy(model)
    modules = dict(model.named_modules())
    swaps = []
    for name, quantizers in (activations or {}).items():
        child = modules.get(name)
        if not isinstance(child, _ACT_MODULES):
            raise ValueError("convert_w8a8_eltwise: %r is not an activation module that a byte table serves (got %s)"
                             % (name, type(child).__name__))
        if not (isinstance(quantizers, (tuple, list)) and len(quantizers) == 2):
            raise ValueError("convert_w8a8_eltwise: %r needs the pair (input quantizer, output quantizer)" % name)
        swaps.append((name, ActivationW8Q.from_float(child, quantizers[0], quantizers[1], mid_dtype)))
    for name, quantizer in (muls or {}).items():
        child = modules.get(name)
        if child is None or not hasattr(child, "mul") or isinstance(child, MulGateW8Q):
            raise ValueError("convert_w8a8_eltwise: %r is not a FloatFunctional whose mul a gate multiply could stand in for (got %s)"
                             % (name, type(child).__name__))
        if quantizer is None and getattr(child, "activation_post_process", None) is None:
            raise ValueError("convert_w8a8_eltwise: %r has no activation_post_process and no output quantizer was given" % name)
        swaps.append((name, MulGateW8Q.from_float(child, quantizer, mid_dtype)))
    for name, new in swaps:
        if name == "":
            return new
        parent_name, _, leaf = name.rpartition(".")
        setattr(modules[parent_name], leaf, new)
    return model
