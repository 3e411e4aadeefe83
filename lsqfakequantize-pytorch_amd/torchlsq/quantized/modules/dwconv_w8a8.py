"""W8A8 deployment of 8-bit QAT DEPTHWISE 2-D convolutions (`groups == in_channels == out_channels`), the layer every block of
MobileNet, EfficientNet, MNASNet and ConvNeXt holds: `DepthwiseConv2dW8A8Q` keeps the weight as its 8-bit LEVELS tap-major,
[kh, kw, C] -- the layout the kernel reads, stored once at conversion -- with one (scale, zero point) per channel, the trained
per-tensor quantizer of the layer's INPUT, and the per-tensor quantizer of its OUTPUT (or none: floats out) with 'none', 'relu'
or 'relu6' in the kernel's epilogue (`torch.ops.torchlsq.lsq_dwconv2d_w8_q8_q` / `lsq_dwconv2d_w8_q8`, liblsq_hip_dwconv_w8.so on
the GPU).  The forward takes a `LevelsTensor`, a per-tensor quantized tensor or a floating tensor and returns a `LevelsTensor` (or
floats): between two W8A8 layers one byte per activation is written, nothing is read back to the host, and the chain can be
captured in a graph.  `convert_w8a8_depthwise(model, input_quantizers, output_quantizers, relu=(), relu6=(), mid_dtype=...)`
swaps the listed layers.
"""
import copy

import torch
from torch import nn

from torchlsq.functional import LevelsTensor, _act_constants, _conv_padding, _two, dw_weight_operands
from .observers import LSQFakeQuantizer
from .packed_linear_a8 import _per_tensor_constants
from .w8a8_q import _MID_DTYPES, _as_levels, _fused_relu, _has_batch_norm

_LEVEL_DTYPES = {"int8": torch.int8, "uint8": torch.uint8}
_ACTS = {"none": 0, "relu": 1, "relu6": 2}


def _is_w8_depthwise(mod):
    """an nn.Conv2d / torch.ao.nn.qat.Conv2d / ConvReLU2d with groups == in_channels == out_channels and zero padding, no batch
    norm, whose weight quantizer is a trained per-channel (axis 0) or per-tensor LSQFakeQuantizer without groups"""
    q = getattr(mod, "weight_fake_quant", None)
    return (isinstance(mod, nn.Conv2d) and not _has_batch_norm(mod) and mod.groups == mod.in_channels == mod.out_channels
            and mod.padding_mode == "zeros" and isinstance(q, LSQFakeQuantizer) and q.group_size is None
            and (not q.is_perchannel or q.ch_axis == 0) and getattr(q, "scale", None) is not None and q._initialized)


class DepthwiseConv2dW8A8Q(nn.Module):
    """`nn.Conv2d(C, C, k, groups=C)` (zero padding) on 8-bit levels with an 8-bit (or floating) output.  Buffers: `weight_levels`
    (int8 or uint8 [kh, kw, C], tap-major), `weight_scale` (float32 [C]), `weight_zero_point` (int32 [C]), `input_scale`,
    `input_shift`, `output_scale`, `output_shift` (float32 [1]); `bias` is a parameter (or None).  Stride, padding, dilation, the
    input and output ranges, `act`, `mid_dtype`, whether the output is quantized and the weight's level type travel in the state
    dict as extra state.  `forward(x)`: a `LevelsTensor` is used as it is (its constants stay on the device), a per-tensor
    torch.quint8 / qint8 tensor likewise, a floating x goes through `lsq_levels_per_tensor` with the input quantizer's constants
    first.  Returns a `LevelsTensor` in channels-last memory, or `mid_dtype` floats without an output quantizer.
    Inference only."""

    def __init__(self, channels, kernel_size, stride=1, padding=0, dilation=1, bias=True, device=None, weight_dtype=torch.int8,
                 input_range=(0, 255, 0, 255), output_range=(0, 255, 0, 255), act="none", mid_dtype=torch.float32, quantized=True):
        super().__init__()
        assert weight_dtype in (torch.int8, torch.uint8)
        assert act in _ACTS, "act must be 'none', 'relu' or 'relu6'"
        assert mid_dtype in _MID_DTYPES.values(), "mid_dtype must be torch.float32, torch.bfloat16 or torch.float16"
        self.channels = self.in_channels = self.out_channels = self.groups = int(channels)
        self.kernel_size = _two(kernel_size, "kernel_size")
        self.stride, self.dilation = _two(stride, "stride"), _two(dilation, "dilation")
        self.padding = _conv_padding(padding, self.kernel_size, self.stride, self.dilation)
        self.register_buffer("weight_levels", torch.zeros(self.kernel_size + (self.channels,), dtype=weight_dtype, device=device))
        self.register_buffer("weight_scale", torch.ones(channels, dtype=torch.float32, device=device))
        self.register_buffer("weight_zero_point", torch.zeros(channels, dtype=torch.int32, device=device))
        self.register_buffer("input_scale", torch.ones(1, dtype=torch.float32, device=device))
        self.register_buffer("input_shift", torch.zeros(1, dtype=torch.float32, device=device))
        self.register_buffer("output_scale", torch.ones(1, dtype=torch.float32, device=device))
        self.register_buffer("output_shift", torch.zeros(1, dtype=torch.float32, device=device))
        self.bias = nn.Parameter(torch.zeros(channels, device=device), requires_grad=False) if bias else None
        self.input_range = tuple(int(v) for v in input_range)
        self.output_range = tuple(int(v) for v in output_range)
        self.act, self.mid_dtype, self.quantized = act, mid_dtype, bool(quantized)
        self.activation_post_process = None

    def _input_levels(self, x):
        x = _as_levels(x)
        if isinstance(x, LevelsTensor):
            return x
        lv = torch.ops.torchlsq.lsq_levels_per_tensor(x, self.input_scale, self.input_shift, *self.input_range, 0)
        s_x, zx = _act_constants(self.input_scale, self.input_shift, self.input_range[2], self.input_range[3])
        return LevelsTensor(lv.view(torch.uint8) if max(self.input_range[1], self.input_range[3]) > 127 else lv, s_x, zx, *self.input_range)

    def forward(self, x):
        x = self._input_levels(x)
        w = (self.weight_levels, self.weight_scale, self.weight_zero_point, self.bias, list(self.stride), list(self.padding),
             list(self.dilation))
        if not self.quantized:
            return torch.ops.torchlsq.lsq_dwconv2d_w8_q8(x.levels, x.scale, x.zero_point, *w, _ACTS[self.act], self.mid_dtype)
        lv = torch.ops.torchlsq.lsq_dwconv2d_w8_q8_q(x.levels, x.scale, x.zero_point, *w, self.output_scale, self.output_shift,
                                                     *self.output_range, _ACTS[self.act], self.mid_dtype)
        s, z = _act_constants(self.output_scale, self.output_shift, self.output_range[2], self.output_range[3])   # on the device
        return LevelsTensor(lv, s, z, *self.output_range)

    def get_extra_state(self):
        return dict(input_range=list(self.input_range), weight_dtype=str(self.weight_levels.dtype).replace("torch.", ""),
                    stride=list(self.stride), padding=list(self.padding), dilation=list(self.dilation),
                    output_range=list(self.output_range), act=self.act, mid_dtype=str(self.mid_dtype).replace("torch.", ""),
                    quantized=self.quantized)

    def set_extra_state(self, state):
        self.input_range = tuple(int(v) for v in state["input_range"])
        self.output_range = tuple(int(v) for v in state["output_range"])
        self.stride, self.padding, self.dilation = (tuple(int(v) for v in state[k]) for k in ("stride", "padding", "dilation"))
        self.weight_levels = self.weight_levels.view(_LEVEL_DTYPES[state["weight_dtype"]])
        self.act, self.mid_dtype, self.quantized = state["act"], _MID_DTYPES[state["mid_dtype"]], bool(state["quantized"])

    def extra_repr(self):
        out = "output levels %d..%d" % self.output_range[:2] if self.quantized else "floating output"
        return "%d, kernel_size=%s, stride=%s, padding=%s, dilation=%s, bias=%s, weight levels %s, input levels %d..%d, %s, act=%s, mid_dtype=%s" % (
            self.channels, self.kernel_size, self.stride, self.padding, self.dilation, self.bias is not None,
            str(self.weight_levels.dtype).replace("torch.", ""), self.input_range[0], self.input_range[1], out, self.act,
            str(self.mid_dtype).replace("torch.", ""))

    @classmethod
    def from_quantized(cls, weight_q, bias=None, input_quantizer=None, stride=1, padding=0, dilation=1, output_quantizer=None,
                       act="none", mid_dtype=torch.float32):
        """from the [C, 1, kh, kw] per-channel (axis 0) or per-tensor torch.qint8 / quint8 weight that
        `LSQFakeQuantizer.quantize(w)` returns (permuted to tap-major here, once), a bias, the trained per-tensor quantizers of the
        layer's input and output (output: None gives floats) and the convolution's geometry"""
        scale, shift, qmin, qmax, tmin, tmax = _per_tensor_constants(input_quantizer, "DepthwiseConv2dW8A8Q.from_quantized")
        out = None if output_quantizer is None else _per_tensor_constants(output_quantizer, "DepthwiseConv2dW8A8Q.from_quantized (output quantizer)")
        levels, w_scale, w_zero = dw_weight_operands(weight_q)
        dev = levels.device
        m = cls(levels.shape[2], tuple(levels.shape[:2]), stride, padding, dilation, bias=bias is not None, device=dev,
                weight_dtype=levels.dtype, input_range=(qmin, qmax, tmin, tmax), act=act, mid_dtype=mid_dtype, quantized=out is not None)
        m.weight_levels = levels.detach().clone()
        m.weight_scale, m.weight_zero_point = w_scale.detach().clone(), w_zero.detach().clone()
        m.input_scale, m.input_shift = scale.to(dev), shift.to(dev)
        if out is not None:
            m.output_scale, m.output_shift, m.output_range = out[0].to(dev), out[1].to(dev), tuple(out[2:])
        if bias is not None:
            m.bias = nn.Parameter(bias.detach().clone(), requires_grad=False)
        return m

    @classmethod
    def from_float(cls, layer, input_quantizer=None, output_quantizer=None, act="none", mid_dtype=torch.float32):
        """from a (QAT) `nn.Conv2d` / `torch.ao.nn.qat.Conv2d` / `ConvReLU2d` (which sets act to 'relu' where it is 'none') with
        groups == in_channels == out_channels and zero padding whose `weight_fake_quant` is a trained per-channel (axis 0) or
        per-tensor `LSQFakeQuantizer`; a module with a batch norm is refused.  `output_quantizer`: None gives the floating output."""
        if _has_batch_norm(layer):
            raise ValueError("DepthwiseConv2dW8A8Q.from_float: %s carries a batch norm, which is not folded (not served)" % type(layer).__name__)
        _per_tensor_constants(input_quantizer, "DepthwiseConv2dW8A8Q.from_float")
        if act not in _ACTS:
            raise ValueError("DepthwiseConv2dW8A8Q.from_float: act must be 'none', 'relu' or 'relu6', got %r" % (act,))
        if not isinstance(layer, nn.Conv2d) or layer.padding_mode != "zeros" or not (layer.groups == layer.in_channels == layer.out_channels):
            raise ValueError("DepthwiseConv2dW8A8Q.from_float needs a 2-D convolution with groups == in_channels == out_channels (no "
                             "channel multiplier) and padding_mode 'zeros'")
        if not _is_w8_depthwise(layer):
            raise ValueError("DepthwiseConv2dW8A8Q.from_float needs a convolution whose weight_fake_quant is a trained per-channel "
                             "(ch_axis 0) or per-tensor LSQFakeQuantizer")
        if _fused_relu(layer) and act == "none":
            act = "relu"
        with torch.no_grad():
            m = cls.from_quantized(layer.weight_fake_quant.quantize(layer.weight.detach()), layer.bias, input_quantizer, layer.stride,
                                   layer.padding, layer.dilation, output_quantizer, act, mid_dtype)
        m.train(layer.training)
        return m


def convert_w8a8_depthwise(model, input_quantizers, output_quantizers, relu=(), relu6=(), mid_dtype=torch.float32, inplace=False):
    """Replace the depthwise convolutions of `model` that `input_quantizers` lists -- a dict from a module's qualified name to the
    trained per-tensor `LSQFakeQuantizer` of its input -- by `DepthwiseConv2dW8A8Q`.  `output_quantizers` maps the same names to
    the quantizer of the layer's output (the next layer's input quantizer); a name it leaves out takes the layer's
    `activation_post_process`, and where there is none (or the name maps to None) the layer gives floats.  `relu` / `relu6`: names
    whose layer is followed by a ReLU / ReLU6, which moves into the kernel -- when the layer sits in an `nn.Sequential` directly
    before an `nn.ReLU` / `nn.ReLU6`, that module becomes an `nn.Identity`; otherwise remove it from the model's forward
    yourself.  Accepted: `nn.Conv2d` / `torch.ao.nn.qat.Conv2d` / `ConvReLU2d` with groups == in_channels == out_channels and
    padding_mode 'zeros'; a module with a batch norm is refused by name.  Works beside `convert_w8a8_q`, `convert_w8a8_add_q` and
    `convert_w8a8_pool` on disjoint names.  Returns the model (a deep copy unless inplace=True)."""
    if not inplace:
        model = copy.deepcopy(model)
    modules = dict(model.named_modules())
    unknown = [n for n in list(output_quantizers) + list(relu) + list(relu6) if n not in input_quantizers]
    if unknown:
        raise ValueError("convert_w8a8_depthwise: %r is listed in output_quantizers, relu or relu6 but not in input_quantizers" % unknown[0])
    both = [n for n in relu if n in relu6]
    if both:
        raise ValueError("convert_w8a8_depthwise: %r is listed in relu and in relu6" % both[0])
    for name, quantizer in input_quantizers.items():
        child = modules.get(name)
        if child is not None and _has_batch_norm(child):
            raise ValueError("convert_w8a8_depthwise: %r is a %s module: its batch norm is not folded (not served)" % (name, type(child).__name__))
        if child is None or not _is_w8_depthwise(child):
            raise ValueError("convert_w8a8_depthwise: %r is not a 2-D convolution with groups == in_channels == out_channels and zero "
                             "padding that has a trained per-channel (ch_axis 0) or per-tensor LSQFakeQuantizer weight quantizer" % name)
        if name in output_quantizers:
            out_q = output_quantizers[name]
        else:
            out_q = getattr(child, "activation_post_process", None)
            out_q = out_q if isinstance(out_q, LSQFakeQuantizer) else None
        act = "relu6" if name in relu6 else "relu" if name in relu else "none"
        new = DepthwiseConv2dW8A8Q.from_float(child, quantizer, out_q, act, mid_dtype)
        if name == "":
            return new
        parent_name, _, leaf = name.rpartition(".")
        parent = modules[parent_name]
        setattr(parent, leaf, new)
        follower = nn.ReLU6 if act == "relu6" else nn.ReLU
        if act != "none" and isinstance(parent, nn.Sequential) and leaf.isdigit() and int(leaf) + 1 < len(parent) \
                and type(parent[int(leaf) + 1]) is follower:
            parent[int(leaf) + 1] = nn.Identity()
    return model
