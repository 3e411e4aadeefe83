"""W8A8 layers that CLOSE A RESIDUAL BLOCK: `LinearW8A8AddQ` and `Conv2dW8A8AddQ` are `LinearW8A8Q` / `Conv2dW8A8Q` that add a
residual `LevelsTensor` in the kernel's epilogue, after the layer's own optional output fake-quantizer (`pre`) and before the
ReLU and the add's quantizer (`torchlsq.functional.lsq_linear_w8a8_add_q` / `lsq_conv2d_w8a8_add_q`, liblsq_hip_resadd_w8.so on
the GPU): `out = relu(q_add(conv_last(h) + identity))` in one launch, one byte read and one written per activation.
`AddW8A8Q` stands in for the block's `torch.ao.nn.quantized.FloatFunctional`, so that the block's `forward` needs no
rewriting; `convert_w8a8_add_q(model, adds, input_quantizers, mid_dtype=...)` swaps both.
"""
import copy

import torch
from torch import nn

from torchlsq.functional import LevelsTensor
from .linear_w8a8 import _is_w8_linear
from .packed_linear_a8 import _per_tensor_constants
from .w8a8_q import Conv2dW8A8Q, LinearW8A8Q, _as_levels, _has_batch_norm, _plain_or_relu_conv

_LAYER_S = object()     # from_float's default pre_quantizer: the layer's own activation_post_process, when it has one


class PendingAdd:
    """What `forward(x)` of the two modules returns: nothing has been launched; `.add(residual, relu)` launches the layer with
    the residual in its epilogue and returns the `LevelsTensor`."""

    def __init__(self, module, x):
        self.module, self.x = module, x

    def add(self, residual, relu=None):
        return self.module._launch(self.x, residual, self.module.relu if relu is None else bool(relu))


class _PreQuantizer:
    """what the two modules add: buffers `pre_scale` and `pre_shift` (float32 [1]) and the range `pre_range` (None: the layer
    has no output fake-quantizer of its own) as extra state"""

    def _init_pre(self, device):
        self.register_buffer("pre_scale", torch.ones(1, dtype=torch.float32, device=device))
        self.register_buffer("pre_shift", torch.zeros(1, dtype=torch.float32, device=device))
        self.pre_range = None

    def _set_pre(self, pre_quantizer, what, device):
        if pre_quantizer is None:
            self.pre_range = None
            return
        scale, shift, qmin, qmax, tmin, tmax = _per_tensor_constants(pre_quantizer, what)
        self.pre_scale, self.pre_shift = scale.to(device), shift.to(device)
        self.pre_range = (qmin, qmax, tmin, tmax)

    def _res_args(self, residual):
        residual = _as_levels(residual)
        assert isinstance(residual, LevelsTensor), "the residual must be a LevelsTensor (or a per-tensor quantized tensor)"
        pre = (None, None, 0, 255, 0, 255) if self.pre_range is None else (self.pre_scale, self.pre_shift, *self.pre_range)
        return (residual.levels, residual.scale, residual.zero_point, *pre)

    def _out_args_with(self, relu):
        return (self.output_scale, self.output_shift, *self.output_range, relu)

    def _pre_state(self):
        return dict(pre_range=None if self.pre_range is None else list(self.pre_range))

    def _load_pre_state(self, state):
        self.pre_range = None if state.get("pre_range") is None else tuple(int(v) for v in state["pre_range"])

    def _pre_repr(self):
        return ", residual add" + ("" if self.pre_range is None else ", own output levels %d..%d" % self.pre_range[:2])

    def forward(self, x, residual=None):
        if residual is None:
            return PendingAdd(self, x)
        return self._launch(x, residual, self.relu)

    def get_extra_state(self):
        return dict(super().get_extra_state(), **self._pre_state())

    def set_extra_state(self, state):
        super().set_extra_state(state)
        self._load_pre_state(state)

    def extra_repr(self):
        return super().extra_repr() + self._pre_repr()


def _layer_pre(layer, pre_quantizer):
    if pre_quantizer is not _LAYER_S:
        return pre_quantizer
    own = getattr(layer, "activation_post_process", None)
    return None if isinstance(own, nn.Identity) else own        # (a qconfig with activation=nn.Identity: no quantizer)


class LinearW8A8AddQ(_PreQuantizer, LinearW8A8Q):
    """`LinearW8A8Q` with a residual.  `forward(x, residual)` takes x as a `LevelsTensor` or a per-tensor quantized tensor and
    the residual as a `LevelsTensor` of the output's shape, and returns a `LevelsTensor`; `forward(x)` returns a `PendingAdd`.
    Inference only."""

    def __init__(self, *args, device=None, **kwargs):
        super().__init__(*args, device=device, **kwargs)
        self._init_pre(device)

    def _launch(self, x, residual, relu):
        x = _as_levels(x)
        assert isinstance(x, LevelsTensor), "LinearW8A8AddQ reads levels: a LevelsTensor or a per-tensor quantized tensor"
        lv = torch.ops.torchlsq.lsq_linear_w8_q8_add_q(x.levels, x.scale, x.zero_point, self.weight_levels, self.weight_scale,
                                                       self.weight_zero_point, self.bias, *self._out_args_with(relu), self.mid_dtype,
                                                       *self._res_args(residual))
        return self._wrap(lv)

    @classmethod
    def from_float(cls, layer, input_quantizer=None, output_quantizer=None, pre_quantizer=_LAYER_S, relu=False,
                   mid_dtype=torch.float32):
        """as `LinearW8A8Q.from_float`, with `output_quantizer` the ADD's quantizer (required) and `pre_quantizer` the layer's own
        output fake-quantizer: by default its `activation_post_process` if it has one, None for none"""
        pre = _layer_pre(layer, pre_quantizer)
        m = super().from_float(layer, input_quantizer, output_quantizer, relu, mid_dtype)
        m._set_pre(pre, "LinearW8A8AddQ.from_float (pre-quantizer)", m.weight_levels.device)
        return m


class Conv2dW8A8AddQ(_PreQuantizer, Conv2dW8A8Q):
    """`Conv2dW8A8Q` with a residual: as `LinearW8A8AddQ`.  The residual is a logical [B, Cout, OH, OW] `LevelsTensor`; one in
    NCHW memory is copied to channels-last first.  Inference only."""

    def __init__(self, *args, device=None, **kwargs):
        super().__init__(*args, device=device, **kwargs)
        self._init_pre(device)

    def _launch(self, x, residual, relu):
        x = _as_levels(x)
        assert isinstance(x, LevelsTensor), "Conv2dW8A8AddQ reads levels: a LevelsTensor or a per-tensor quantized tensor"
        lv = torch.ops.torchlsq.lsq_conv2d_w8_q8_add_q(x.levels, x.scale, x.zero_point, self.weight_levels, self.weight_scale,
                                                       self.weight_zero_point, self.bias, list(self.stride), list(self.padding),
                                                       list(self.dilation), *self._out_args_with(relu), self.mid_dtype,
                                                       *self._res_args(residual))
        return self._wrap(lv)

    @classmethod
    def from_float(cls, layer, input_quantizer=None, output_quantizer=None, pre_quantizer=_LAYER_S, relu=False,
                   mid_dtype=torch.float32):
        """as `Conv2dW8A8Q.from_float`, with `output_quantizer` the ADD's quantizer (required) and `pre_quantizer` the layer's own
        output fake-quantizer: by default its `activation_post_process` if it has one, None for none"""
        pre = _layer_pre(layer, pre_quantizer)
        m = super().from_float(layer, input_quantizer, output_quantizer, relu, mid_dtype)
        m._set_pre(pre, "Conv2dW8A8AddQ.from_float (pre-quantizer)", m.weight_levels.device)
        return m


class AddW8A8Q(nn.Module):
    """Stands in for the `torch.ao.nn.quantized.FloatFunctional` that closes a residual block: `add(a, b)` and `add_relu(a, b)`
    take exactly one `PendingAdd` (the converted last layer's `forward(x)`) and one `LevelsTensor` (the identity), in either
    order, and launch the layer with the residual in its epilogue."""

    def forward(self, x):
        raise RuntimeError("AddW8A8Q is not intended to use the 'forward'. Please use the underlying operation")

    @staticmethod
    def _close(a, b, relu):
        if isinstance(b, PendingAdd):
            a, b = b, a
        if not isinstance(a, PendingAdd) or isinstance(b, PendingAdd) or not (isinstance(b, LevelsTensor) or
                                                                            (isinstance(b, torch.Tensor) and b.is_quantized)):
            raise TypeError("AddW8A8Q needs one pending layer output (Linear/Conv2dW8A8AddQ.forward(x)) and one LevelsTensor, got %s "
                            "and %s" % (type(a).__name__, type(b).__name__))
        return a.add(b, relu=relu)

    def add(self, a, b):
        return self._close(a, b, False)

    def add_relu(self, a, b):
        return self._close(a, b, True)


def convert_w8a8_add_q(model, adds, input_quantizers, mid_dtype=torch.float32, inplace=False):
    """Replace the ends of the residual blocks of `model`.  `adds` maps the qualified name of a block's
    `torch.ao.nn.quantized.FloatFunctional` to the name of the layer whose output it adds to the identity, e.g.
    `{"layer1.0.add_relu": "layer1.0.conv2"}`; `input_quantizers` maps that layer's name to the trained per-tensor
    `LSQFakeQuantizer` of its input.  The layer becomes a `LinearW8A8AddQ` / `Conv2dW8A8AddQ` whose output quantizer is the
    FloatFunctional's `activation_post_process` and whose pre-quantizer is the layer's own `activation_post_process` if it has
    one; the FloatFunctional becomes an `AddW8A8Q`, so the block's `forward` (`self.add_relu.add_relu(out, identity)`) stays
    as it is.  A layer with a batch norm is refused by name.  `convert_w8a8_q` serves the other layers of the same model: the
    two work on disjoint names.  Returns the model (a deep copy unless inplace=True)."""
    if not inplace:
        model = copy.deepcopy(model)
    modules = dict(model.named_modules())
    for add_name, name in adds.items():
        ff, child = modules.get(add_name), modules.get(name)
        if child is None or name not in input_quantizers:
            raise ValueError("convert_w8a8_add_q: %r closes %r, which is not a module of the model that input_quantizers lists" %
                             (add_name, name))
        if _has_batch_norm(child):
            raise ValueError("convert_w8a8_add_q: %r is a %s module: its batch norm is not folded (not served)" %
                             (name, type(child).__name__))
        if ff is None or not (hasattr(ff, "add") and hasattr(ff, "add_relu")) or getattr(ff, "activation_post_process", None) is None:
            raise ValueError("convert_w8a8_add_q: %r is not a FloatFunctional with an activation_post_process" % add_name)
        args = (child, input_quantizers[name], ff.activation_post_process)
        if _plain_or_relu_conv(child):
            new = Conv2dW8A8AddQ.from_float(*args, mid_dtype=mid_dtype)
        elif _is_w8_linear(child):
            new = LinearW8A8AddQ.from_float(*args, mid_dtype=mid_dtype)
        else:
            raise ValueError("convert_w8a8_add_q: %r is not a linear layer or a 2-D convolution with groups == 1 and zero padding that "
                             "has a trained per-channel (ch_axis 0) or per-tensor LSQFakeQuantizer weight quantizer" % name)
        for qualified, mod in ((name, new), (add_name, AddW8A8Q())):
            parent_name, _, leaf = qualified.rpartition(".")
            setattr(modules[parent_name], leaf, mod)
    return model
