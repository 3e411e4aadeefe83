"""W4A8 / W2A8 deployment of group-wise QAT linear layers: `PackedLinearA8` is `PackedLinear` -- the weight as packed 4- / 2-bit
codes with one (scale, zero point) per group -- plus the trained per-tensor quantizer of the layer's INPUT: its scale and
shift as buffers, its range as extra state.  The forward multiplies the input's 8-bit levels with the codes in integers
(`torchlsq.functional.lsq_linear_packed_a8`, liblsq_hip_qlinear_a8.so on the GPU): a floating input is quantized inside the
kernel, a per-tensor quantized tensor is read as it is.  `convert_packed_a8(model, input_quantizers)` swaps the listed
group-wise linear layers for one.  `PackedLinear` and `convert_packed` are unchanged.
"""
import copy

import torch
from torch import nn

from torchlsq.functional import PackedGroupTensor, lsq_linear_packed_a8
from .observers import TYPES_RANGE_MAPPING, LSQFakeQuantizer
from .packed_linear import PackedLinear, _is_groupwise_linear


def _per_tensor_constants(q, what):
    """(scale [1], shift [1], quant_min, quant_max, type_min, type_max) of a trained per-tensor LSQFakeQuantizer"""
    if not isinstance(q, LSQFakeQuantizer):
        raise ValueError("%s needs the LSQFakeQuantizer that quantizes the layer's input, got %s" % (what, type(q).__name__))
    if q.is_perchannel or q.group_size is not None:
        raise ValueError("%s needs a per-tensor input quantizer; a per-channel or group-wise quantizer has no single (scale, zero "
                         "point) for the integer product" % what)
    if getattr(q, "scale", None) is None or not q._initialized:
        raise ValueError("%s: the input quantizer has not seen a batch yet (no trained scale)" % what)
    tmin, tmax = TYPES_RANGE_MAPPING[q.dtype]['range']
    return (q.scale.detach().reshape(-1)[:1].to(torch.float32).clone(), q.shift.detach().reshape(-1)[:1].to(torch.float32).clone(),
            int(q.quant_min), int(q.quant_max), int(tmin), int(tmax))


class PackedLinearA8(PackedLinear):
    """`PackedLinear` on quantized activations.  Buffers: those of `PackedLinear` plus `input_scale` and `input_shift`
    (float32 [1]); the input quantizer's quant_min, quant_max, type_min and type_max travel in the extra state next to bits,
    group_size and quant_min of the weight.  `forward(x)`: a floating x is quantized with the input quantizer's constants
    inside the kernel (y has x's dtype); a per-tensor torch.quint8 / qint8 tensor is used as it is (y is float32).
    Inference only."""

    def __init__(self, in_features, out_features, bits=4, group_size=32, quant_min=-8, bias=True, device=None,
                 input_range=(0, 255, 0, 255)):
        super().__init__(in_features, out_features, bits, group_size, quant_min, bias, device)
        self.register_buffer("input_scale", torch.ones(1, dtype=torch.float32, device=device))
        self.register_buffer("input_shift", torch.zeros(1, dtype=torch.float32, device=device))
        self.input_range = tuple(int(v) for v in input_range)

    def forward(self, x):
        if x.is_quantized:
            y = lsq_linear_packed_a8(x, self.packed(), self.bias)
        else:
            y = lsq_linear_packed_a8(x, self.packed(), self.bias, self.input_scale, self.input_shift, *self.input_range)
        return y if self.activation_post_process is None else self.activation_post_process(y)

    def get_extra_state(self):
        state = super().get_extra_state()
        state["input_range"] = list(self.input_range)
        return state

    def set_extra_state(self, state):
        super().set_extra_state(state)
        self.input_range = tuple(int(v) for v in state["input_range"])

    def extra_repr(self):
        return super().extra_repr() + ", input levels %d..%d" % self.input_range[:2]

    def _set_input(self, input_quantizer, what):
        scale, shift, qmin, qmax, tmin, tmax = _per_tensor_constants(input_quantizer, what)
        self.input_scale = scale.to(self.codes.device)
        self.input_shift = shift.to(self.codes.device)
        self.input_range = (qmin, qmax, tmin, tmax)
        return self

    @classmethod
    def from_packed(cls, p: PackedGroupTensor, bias=None, input_quantizer=None):
        """from a packed 2-D weight [out, in], a bias and the trained per-tensor quantizer of the layer's input"""
        scale_etc = _per_tensor_constants(input_quantizer, "PackedLinearA8.from_packed")       # refuse before anything is built
        base = PackedLinear.from_packed(p, bias)
        m = cls(base.in_features, base.out_features, base.bits, base.group_size, base.quant_min, bias=bias is not None,
                device=p.codes.device, input_range=scale_etc[2:])
        m.codes, m.scale, m.zero_point, m.bias = base.codes, base.scale, base.zero_point, base.bias
        return m._set_input(input_quantizer, "PackedLinearA8.from_packed")

    @classmethod
    def from_float(cls, layer, input_quantizer=None, bits=None):
        """from a (QAT) linear layer whose `weight_fake_quant` is a trained group-wise `LSQFakeQuantizer`, and the trained
        per-tensor `LSQFakeQuantizer` that quantizes this layer's input (usually the previous module's
        `activation_post_process` or a QuantStub's); an output `activation_post_process` of the layer is kept"""
        _per_tensor_constants(input_quantizer, "PackedLinearA8.from_float")
        q = getattr(layer, "weight_fake_quant", None)
        if not isinstance(q, LSQFakeQuantizer) or q.group_size is None:
            raise ValueError("PackedLinearA8.from_float needs a linear layer whose weight_fake_quant is a group-wise "
                             "LSQFakeQuantizer (group_size=...)")
        m = cls.from_packed(q.export_packed(layer.weight.detach(), bits), layer.bias, input_quantizer)
        post = getattr(layer, "activation_post_process", None)
        if post is not None and not isinstance(post, nn.Identity):
            m.activation_post_process = post
        m.train(layer.training)
        return m


def convert_packed_a8(model, input_quantizers, inplace=False):
    """Replace the group-wise linear layers of `model` that `input_quantizers` lists -- a dict from a module's qualified name
    (as in `model.named_modules()`) to the trained per-tensor `LSQFakeQuantizer` of its input -- by `PackedLinearA8`;
    everything else is left alone.  A listed name that is no group-wise linear layer is an error.  Returns the model (a deep
    copy unless inplace=True; the quantizers are only read)."""
    if not inplace:
        model = copy.deepcopy(model)
    modules = dict(model.named_modules())
    for name, quantizer in input_quantizers.items():
        child = modules.get(name)
        if child is None or not _is_groupwise_linear(child):
            raise ValueError("convert_packed_a8: %r is not a linear layer with a group-wise LSQFakeQuantizer weight quantizer" % name)
        new = PackedLinearA8.from_float(child, quantizer)
        if name == "":
            return new
        parent_name, _, leaf = name.rpartition(".")
        setattr(modules[parent_name], leaf, new)
    return model
