"""W8A8 deployment of 8-bit QAT 2-D convolutions -- the README's qconfig on the layers it was made for: per-tensor `quint8`
activations, per-channel `qint8` weights.  `Conv2dW8A8` keeps the weight as its 8-bit LEVELS [out, in, kh, kw] in channels-last
memory with one (scale, zero point) per output channel, and the trained per-tensor quantizer of the layer's INPUT: its scale and
shift as buffers, its range and the convolution's geometry as extra state.  The forward multiplies the input's 8-bit levels
with the weight's in integers over every tap and input channel (`torchlsq.functional.lsq_conv2d_w8a8`, liblsq_hip_qconv_w8.so
on the GPU): a floating input is quantized on the way, a per-tensor quantized tensor is read as it is.  The output is
channels-last.  `convert_w8a8(model, input_quantizers)` (linear_w8a8.py) swaps the listed convolutions for one.
"""
import torch
from torch import nn

from torchlsq.functional import _conv_padding, _two, w8_weight_operands
from .observers import LSQFakeQuantizer
from .packed_linear_a8 import _per_tensor_constants

_LEVEL_DTYPES = {"int8": torch.int8, "uint8": torch.uint8}


def _fused_conv(mod):
    """a fused Conv-BN / Conv-ReLU (QAT) module of torch.ao.nn.intrinsic: its batch norm is not folded and its ReLU not applied here"""
    import torch.ao.nn.intrinsic as nni
    return isinstance(mod, nni._FusedModule)


def _is_w8_conv(mod):
    """a plain nn.Conv2d / torch.ao.nn.qat.Conv2d with groups == 1 and zero padding whose weight quantizer is a trained
    per-channel (axis 0) or per-tensor LSQFakeQuantizer without groups"""
    q = getattr(mod, "weight_fake_quant", None)
    return (isinstance(mod, nn.Conv2d) and not _fused_conv(mod) and mod.groups == 1 and mod.padding_mode == "zeros"
            and isinstance(q, LSQFakeQuantizer) and q.group_size is None and (not q.is_perchannel or q.ch_axis == 0)
            and getattr(q, "scale", None) is not None and q._initialized)


class Conv2dW8A8(nn.Module):
    """`nn.Conv2d` (groups == 1, zero padding) on 8-bit levels.  Buffers: `weight_levels` (int8 or uint8 [out, in, kh, kw], held
    channels-last), `weight_scale` (float32 [out]), `weight_zero_point` (int32 [out]), `input_scale` and `input_shift`
    (float32 [1]); `bias` is a parameter (or None).  Stride, padding and dilation, the input quantizer's quant_min, quant_max,
    type_min and type_max and the weight's level type travel in the state dict as extra state.  `forward(x)`: a floating x is
    quantized with the input quantizer's constants (y has x's dtype); a per-tensor torch.quint8 / qint8 tensor is used as it
    is (y is float32).  y is channels-last; an x that is not is copied into that format first.  Inference only."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=True, device=None,
                 weight_dtype=torch.int8, input_range=(0, 255, 0, 255)):
        super().__init__()
        assert weight_dtype in (torch.int8, torch.uint8)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size = _two(kernel_size, "kernel_size")
        self.stride, self.dilation = _two(stride, "stride"), _two(dilation, "dilation")
        self.padding = _conv_padding(padding, self.kernel_size, self.stride, self.dilation)
        levels = torch.zeros((self.out_channels, self.in_channels) + self.kernel_size, dtype=weight_dtype, device=device)
        self.register_buffer("weight_levels", levels.contiguous(memory_format=torch.channels_last))
        self.register_buffer("weight_scale", torch.ones(out_channels, dtype=torch.float32, device=device))
        self.register_buffer("weight_zero_point", torch.zeros(out_channels, dtype=torch.int32, device=device))
        self.register_buffer("input_scale", torch.ones(1, dtype=torch.float32, device=device))
        self.register_buffer("input_shift", torch.zeros(1, dtype=torch.float32, device=device))
        self.bias = nn.Parameter(torch.zeros(out_channels, device=device), requires_grad=False) if bias else None
        self.input_range = tuple(int(v) for v in input_range)
        self.activation_post_process = None

    def forward(self, x):
        w = (self.weight_levels, self.weight_scale, self.weight_zero_point, self.bias, list(self.stride), list(self.padding),
             list(self.dilation))
        if x.is_quantized:
            assert x.qscheme() in (torch.per_tensor_affine, torch.per_tensor_symmetric) and x.dtype in (torch.quint8, torch.qint8), \
                "Conv2dW8A8 needs a floating or a per-tensor torch.quint8 / torch.qint8 input"
            s_x = torch.tensor([x.q_scale()], dtype=torch.float32, device=x.device)
            zx = torch.tensor([x.q_zero_point()], dtype=torch.int32, device=x.device)
            y = torch.ops.torchlsq.lsq_conv2d_w8_q8(x.int_repr(), s_x, zx, *w, torch.float32)
        else:
            y = torch.ops.torchlsq.lsq_conv2d_w8_a8(x, self.input_scale, self.input_shift, *self.input_range, *w)
        return y if self.activation_post_process is None else self.activation_post_process(y)

    def get_extra_state(self):
        return dict(input_range=list(self.input_range), weight_dtype=str(self.weight_levels.dtype).replace("torch.", ""),
                    stride=list(self.stride), padding=list(self.padding), dilation=list(self.dilation))

    def set_extra_state(self, state):
        self.input_range = tuple(int(v) for v in state["input_range"])
        self.stride, self.padding, self.dilation = (tuple(int(v) for v in state[k]) for k in ("stride", "padding", "dilation"))
        self.weight_levels = self.weight_levels.view(_LEVEL_DTYPES[state["weight_dtype"]])

    def extra_repr(self):
        return "%d, %d, kernel_size=%s, stride=%s, padding=%s, dilation=%s, bias=%s, weight levels %s, input levels %d..%d" % (
            self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding, self.dilation, self.bias is not None,
            str(self.weight_levels.dtype).replace("torch.", ""), self.input_range[0], self.input_range[1])

    @classmethod
    def from_quantized(cls, weight_q, bias=None, input_quantizer=None, stride=1, padding=0, dilation=1):
        """from the 4-D per-channel (axis 0) or per-tensor torch.qint8 / quint8 weight that `LSQFakeQuantizer.quantize(w)`
        returns, a bias, the trained per-tensor quantizer of the layer's input and the convolution's geometry"""
        scale, shift, qmin, qmax, tmin, tmax = _per_tensor_constants(input_quantizer, "Conv2dW8A8.from_quantized")
        assert weight_q.dim() == 4, "Conv2dW8A8.from_quantized needs a 4-D weight [out_channels, in_channels, kh, kw]"
        levels, w_scale, w_zero = w8_weight_operands(weight_q)
        m = cls(levels.shape[1], levels.shape[0], tuple(levels.shape[2:]), stride, padding, dilation, bias=bias is not None,
                device=levels.device, weight_dtype=levels.dtype, input_range=(qmin, qmax, tmin, tmax))
        m.weight_levels = levels.detach().clone(memory_format=torch.channels_last)
        m.weight_scale = w_scale.detach().clone()
        m.weight_zero_point = w_zero.detach().clone()
        m.input_scale = scale.to(levels.device)
        m.input_shift = shift.to(levels.device)
        if bias is not None:
            m.bias = nn.Parameter(bias.detach().clone(), requires_grad=False)
        return m

    @classmethod
    def from_float(cls, layer, input_quantizer=None):
        """from a plain (QAT) `nn.Conv2d` / `torch.ao.nn.qat.Conv2d` with groups == 1 and zero padding whose `weight_fake_quant`
        is a trained per-channel (axis 0) or per-tensor `LSQFakeQuantizer`, and the trained per-tensor `LSQFakeQuantizer` that
        quantizes this layer's input; an output `activation_post_process` of the layer is kept"""
        _per_tensor_constants(input_quantizer, "Conv2dW8A8.from_float")        # refuse before anything is built
        if _fused_conv(layer):
            raise ValueError("Conv2dW8A8.from_float: %s is a fused Conv-BN / Conv-ReLU module; its batch norm is not folded and its "
                             "ReLU not applied by this layer (not served)" % type(layer).__name__)
        if not isinstance(layer, nn.Conv2d) or layer.groups != 1 or layer.padding_mode != "zeros":
            raise ValueError("Conv2dW8A8.from_float needs a 2-D convolution with groups == 1 and padding_mode 'zeros'")
        q = getattr(layer, "weight_fake_quant", None)
        if not isinstance(q, LSQFakeQuantizer) or q.group_size is not None:
            raise ValueError("Conv2dW8A8.from_float needs a convolution whose weight_fake_quant is a per-channel or per-tensor "
                             "LSQFakeQuantizer")
        if q.is_perchannel and q.ch_axis != 0:
            raise ValueError("Conv2dW8A8.from_float needs a weight quantized per output channel (ch_axis 0), got ch_axis %d" % q.ch_axis)
        if getattr(q, "scale", None) is None or not q._initialized:
            raise ValueError("Conv2dW8A8.from_float: the weight quantizer has not seen a batch yet (no trained scale)")
        with torch.no_grad():
            m = cls.from_quantized(q.quantize(layer.weight.detach()), layer.bias, input_quantizer, layer.stride, layer.padding,
                                   layer.dilation)
        post = getattr(layer, "activation_post_process", None)
        if post is not None and not isinstance(post, nn.Identity):
            m.activation_post_process = post
        m.train(layer.training)
        return m
