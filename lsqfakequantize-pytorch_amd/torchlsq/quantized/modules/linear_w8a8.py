"""W8A8 deployment of 8-bit QAT linear layers -- the README's qconfig: per-tensor `quint8` activations, per-channel `qint8`
weights.  `LinearW8A8` keeps the weight as its 8-bit LEVELS with one (scale, zero point) per output row, and the trained
per-tensor quantizer of the layer's INPUT: its scale and shift as buffers, its range as extra state.  The forward multiplies
the input's 8-bit levels with the weight's in integers over all of K (`torchlsq.functional.lsq_linear_w8a8`,
liblsq_hip_qlinear_w8.so on the GPU): a floating input is quantized on the way, a per-tensor quantized tensor is read as it
is.  `convert_w8a8(model, input_quantizers)` swaps the listed linear layers for one (and the listed 2-D convolutions for a
`Conv2dW8A8`, conv_w8a8.py).
"""
import copy

import torch
from torch import nn

from torchlsq.functional import w8_weight_operands
from .observers import LSQFakeQuantizer
from .conv_w8a8 import Conv2dW8A8, _fused_conv, _is_w8_conv
from .packed_linear_a8 import _per_tensor_constants

_LEVEL_DTYPES = {"int8": torch.int8, "uint8": torch.uint8}


def _is_w8_linear(mod):
    """an nn.Linear whose weight quantizer is a trained per-channel (axis 0) or per-tensor LSQFakeQuantizer without groups"""
    q = getattr(mod, "weight_fake_quant", None)
    return (isinstance(mod, nn.Linear) and isinstance(q, LSQFakeQuantizer) and q.group_size is None
            and (not q.is_perchannel or q.ch_axis == 0) and getattr(q, "scale", None) is not None and q._initialized)


class LinearW8A8(nn.Module):
    """`nn.Linear` on 8-bit levels.  Buffers: `weight_levels` (int8 or uint8 [out, in]), `weight_scale` (float32 [out]),
    `weight_zero_point` (int32 [out]), `input_scale` and `input_shift` (float32 [1]); `bias` is a parameter (or None).  The
    input quantizer's quant_min, quant_max, type_min and type_max and the weight's level type travel in the state dict as
    extra state.  `forward(x)`: a floating x is quantized with the input quantizer's constants (y has x's dtype); a per-tensor
    torch.quint8 / qint8 tensor is used as it is (y is float32).  Inference only."""

    def __init__(self, in_features, out_features, bias=True, device=None, weight_dtype=torch.int8, input_range=(0, 255, 0, 255)):
        super().__init__()
        assert weight_dtype in (torch.int8, torch.uint8)
        self.in_features, self.out_features = int(in_features), int(out_features)
        self.register_buffer("weight_levels", torch.zeros(out_features, in_features, dtype=weight_dtype, device=device))
        self.register_buffer("weight_scale", torch.ones(out_features, dtype=torch.float32, device=device))
        self.register_buffer("weight_zero_point", torch.zeros(out_features, dtype=torch.int32, device=device))
        self.register_buffer("input_scale", torch.ones(1, dtype=torch.float32, device=device))
        self.register_buffer("input_shift", torch.zeros(1, dtype=torch.float32, device=device))
        self.bias = nn.Parameter(torch.zeros(out_features, device=device), requires_grad=False) if bias else None
        self.input_range = tuple(int(v) for v in input_range)
        self.activation_post_process = None

    def forward(self, x):
        w = (self.weight_levels, self.weight_scale, self.weight_zero_point, self.bias)
        if x.is_quantized:
            assert x.qscheme() in (torch.per_tensor_affine, torch.per_tensor_symmetric) and x.dtype in (torch.quint8, torch.qint8), \
                "LinearW8A8 needs a floating or a per-tensor torch.quint8 / torch.qint8 input"
            s_x = torch.tensor([x.q_scale()], dtype=torch.float32, device=x.device)
            zx = torch.tensor([x.q_zero_point()], dtype=torch.int32, device=x.device)
            y = torch.ops.torchlsq.lsq_linear_w8_q8(x.int_repr(), s_x, zx, *w, torch.float32)
        else:
            y = torch.ops.torchlsq.lsq_linear_w8_a8(x, self.input_scale, self.input_shift, *self.input_range, *w)
        return y if self.activation_post_process is None else self.activation_post_process(y)

    def get_extra_state(self):
        return dict(input_range=list(self.input_range), weight_dtype=str(self.weight_levels.dtype).replace("torch.", ""))

    def set_extra_state(self, state):
        self.input_range = tuple(int(v) for v in state["input_range"])
        self.weight_levels = self.weight_levels.view(_LEVEL_DTYPES[state["weight_dtype"]])

    def extra_repr(self):
        return "in_features=%d, out_features=%d, bias=%s, weight levels %s, input levels %d..%d" % (
            self.in_features, self.out_features, self.bias is not None, str(self.weight_levels.dtype).replace("torch.", ""),
            self.input_range[0], self.input_range[1])

    @classmethod
    def from_quantized(cls, weight_q, bias=None, input_quantizer=None):
        """from the 2-D per-channel (axis 0) or per-tensor torch.qint8 / quint8 weight that `LSQFakeQuantizer.quantize(w)`
        returns, a bias and the trained per-tensor quantizer of the layer's input"""
        scale, shift, qmin, qmax, tmin, tmax = _per_tensor_constants(input_quantizer, "LinearW8A8.from_quantized")
        levels, w_scale, w_zero = w8_weight_operands(weight_q)
        out_f, in_f = levels.shape
        m = cls(in_f, out_f, bias=bias is not None, device=levels.device, weight_dtype=levels.dtype, input_range=(qmin, qmax, tmin, tmax))
        m.weight_levels = levels.detach().clone()
        m.weight_scale = w_scale.detach().clone()
        m.weight_zero_point = w_zero.detach().clone()
        m.input_scale = scale.to(levels.device)
        m.input_shift = shift.to(levels.device)
        if bias is not None:
            m.bias = nn.Parameter(bias.detach().clone(), requires_grad=False)
        return m

    @classmethod
    def from_float(cls, layer, input_quantizer=None):
        """from a (QAT) linear layer whose `weight_fake_quant` is a trained per-channel (axis 0) or per-tensor
        `LSQFakeQuantizer`, and the trained per-tensor `LSQFakeQuantizer` that quantizes this layer's input (usually the
        previous module's `activation_post_process` or a QuantStub's); an output `activation_post_process` of the layer is
        kept"""
        _per_tensor_constants(input_quantizer, "LinearW8A8.from_float")        # refuse before anything is built
        q = getattr(layer, "weight_fake_quant", None)
        if not isinstance(q, LSQFakeQuantizer) or q.group_size is not None:
            raise ValueError("LinearW8A8.from_float needs a linear layer whose weight_fake_quant is a per-channel or per-tensor "
                             "LSQFakeQuantizer (a group-wise one deploys as PackedLinearA8)")
        if q.is_perchannel and q.ch_axis != 0:
            raise ValueError("LinearW8A8.from_float needs a weight quantized per output row (ch_axis 0), got ch_axis %d" % q.ch_axis)
        if getattr(q, "scale", None) is None or not q._initialized:
            raise ValueError("LinearW8A8.from_float: the weight quantizer has not seen a batch yet (no trained scale)")
        with torch.no_grad():
            m = cls.from_quantized(q.quantize(layer.weight.detach()), layer.bias, input_quantizer)
        post = getattr(layer, "activation_post_process", None)
        if post is not None and not isinstance(post, nn.Identity):
            m.activation_post_process = post
        m.train(layer.training)
        return m


def convert_w8a8(model, input_quantizers, inplace=False):
    """Replace the layers of `model` that `input_quantizers` lists -- a dict from a module's qualified name (as in
    `model.named_modules()`) to the trained per-tensor `LSQFakeQuantizer` of its input -- by `LinearW8A8` (an `nn.Linear`) or
    `Conv2dW8A8` (a plain `nn.Conv2d` / `torch.ao.nn.qat.Conv2d` with groups == 1 and padding_mode 'zeros'); everything else
    is left alone.  A listed name that is neither, or whose weight quantizer is not a trained per-channel (ch_axis 0) or
    per-tensor `LSQFakeQuantizer` without group_size, is an error; so is a fused Conv-BN / Conv-ReLU QAT module.  Returns the
    model (a deep copy unless inplace=True; the quantizers are only read)."""
    if not inplace:
        model = copy.deepcopy(model)
    modules = dict(model.named_modules())
    for name, quantizer in input_quantizers.items():
        child = modules.get(name)
        if child is not None and _fused_conv(child):
            raise ValueError("convert_w8a8: %r is a fused %s module, not a linear layer or a plain 2-D convolution: its batch norm "
                             "is not folded and its ReLU not applied by Conv2dW8A8 (not served)" % (name, type(child).__name__))
        if child is not None and _is_w8_conv(child):
            new = Conv2dW8A8.from_float(child, quantizer)
        elif child is not None and _is_w8_linear(child):
            new = LinearW8A8.from_float(child, quantizer)
        else:
            raise ValueError("convert_w8a8: %r is not a linear layer or a 2-D convolution with groups == 1 and zero padding that has "
                             "a trained per-channel (ch_axis 0) or per-tensor LSQFakeQuantizer weight quantizer" % name)
        if name == "":
            return new
        parent_name, _, leaf = name.rpartition(".")
        setattr(modules[parent_name], leaf, new)
    return model
