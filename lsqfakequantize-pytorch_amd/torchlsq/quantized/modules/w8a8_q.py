"""W8A8 layers that hand 8-bit LEVELS to the next layer: `LinearW8A8Q` and `Conv2dW8A8Q` are `LinearW8A8` / `Conv2dW8A8` with the
trained per-tensor quantizer of their OUTPUT (the next layer's input quantizer) and an optional ReLU in the kernel's epilogue
(`torchlsq.functional.lsq_linear_w8a8_q` / `lsq_conv2d_w8a8_q`, liblsq_hip_requant_w8.so on the GPU).  The forward takes a
floating tensor, a per-tensor quantized tensor or a `LevelsTensor` and returns a `LevelsTensor`: between two such layers one
byte per activation is written, nothing is read back to the host, and the chain can be captured in a graph.
`convert_w8a8_q(model, input_quantizers, output_quantizers, relu=(), mid_dtype=...)` swaps the listed layers.
"""
import copy

import torch
from torch import nn

from torchlsq.functional import LevelsTensor, _act_constants
from .conv_w8a8 import Conv2dW8A8, _is_w8_conv
from .linear_w8a8 import LinearW8A8, _is_w8_linear
from .observers import LSQFakeQuantizer
from .packed_linear_a8 import _per_tensor_constants

_MID_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def _has_batch_norm(mod):
    """a fused QAT module that carries a batch norm (ConvBn2d, ConvBnReLU2d, LinearBn1d, ...): not folded here"""
    return hasattr(mod, "bn") or "Bn" in type(mod).__name__


def _fused_relu(mod):
    """torch.ao.nn.intrinsic.qat.ConvReLU2d / LinearReLU: a QAT layer whose forward applies a ReLU"""
    import torch.ao.nn.intrinsic as nni
    return isinstance(mod, nni._FusedModule) and "ReLU" in type(mod).__name__


class _OutputQuantizer:
    """what the two modules add: buffers `output_scale` and `output_shift` (float32 [1]); the output range, `relu` and
    `mid_dtype` as extra state"""

    def _init_output(self, device, output_range, relu, mid_dtype):
        assert mid_dtype in _MID_DTYPES.values(), "mid_dtype must be torch.float32, torch.bfloat16 or torch.float16"
        self.register_buffer("output_scale", torch.ones(1, dtype=torch.float32, device=device))
        self.register_buffer("output_shift", torch.zeros(1, dtype=torch.float32, device=device))
        self.output_range = tuple(int(v) for v in output_range)
        self.relu, self.mid_dtype = bool(relu), mid_dtype
        self.activation_post_process = None

    def _set_output(self, output_quantizer, what, device):
        scale, shift, qmin, qmax, tmin, tmax = _per_tensor_constants(output_quantizer, what)
        self.output_scale, self.output_shift = scale.to(device), shift.to(device)
        self.output_range = (qmin, qmax, tmin, tmax)

    def _out_args(self):
        return (self.output_scale, self.output_shift, *self.output_range, self.relu)

    def _wrap(self, levels):
        s, z = _act_constants(self.output_scale, self.output_shift, self.output_range[2], self.output_range[3])   # on the device
        return LevelsTensor(levels, s, z, *self.output_range)

    def _output_state(self):
        return dict(output_range=list(self.output_range), relu=self.relu, mid_dtype=str(self.mid_dtype).replace("torch.", ""))

    def _load_output_state(self, state):
        self.output_range = tuple(int(v) for v in state["output_range"])
        self.relu, self.mid_dtype = bool(state["relu"]), _MID_DTYPES[state["mid_dtype"]]

    def _output_repr(self):
        return ", output levels %d..%d, relu=%s, mid_dtype=%s" % (self.output_range[0], self.output_range[1], self.relu,
                                                                  str(self.mid_dtype).replace("torch.", ""))


def _as_levels(x):
    if isinstance(x, torch.Tensor) and x.is_quantized:
        return LevelsTensor.from_quantized(x)       # uploads the tensor's host constants: not for a captured graph
    return x


class LinearW8A8Q(LinearW8A8, _OutputQuantizer):
    """`LinearW8A8` with an 8-bit output.  `forward(x)` takes a `LevelsTensor` (its constants stay on the device), a per-tensor
    torch.quint8 / qint8 tensor or a floating x (quantized with the input quantizer's constants; `mid_dtype` is then x's
    dtype) and returns a `LevelsTensor`.  Inference only."""

    def __init__(self, in_features, out_features, bias=True, device=None, weight_dtype=torch.int8, input_range=(0, 255, 0, 255),
                 output_range=(0, 255, 0, 255), relu=False, mid_dtype=torch.float32):
        super().__init__(in_features, out_features, bias, device, weight_dtype, input_range)
        self._init_output(device, output_range, relu, mid_dtype)

    def forward(self, x):
        w = (self.weight_levels, self.weight_scale, self.weight_zero_point, self.bias)
        x = _as_levels(x)
        if isinstance(x, LevelsTensor):
            lv = torch.ops.torchlsq.lsq_linear_w8_q8_q(x.levels, x.scale, x.zero_point, *w, *self._out_args(), self.mid_dtype)
        else:
            lv = torch.ops.torchlsq.lsq_linear_w8_a8_q(x, self.input_scale, self.input_shift, *self.input_range, *w, *self._out_args())
        return self._wrap(lv)

    def get_extra_state(self):
        return dict(super().get_extra_state(), **self._output_state())

    def set_extra_state(self, state):
        super().set_extra_state(state)
        self._load_output_state(state)

    def extra_repr(self):
        return super().extra_repr() + self._output_repr()

    @classmethod
    def from_quantized(cls, weight_q, bias=None, input_quantizer=None, output_quantizer=None, relu=False, mid_dtype=torch.float32):
        _per_tensor_constants(output_quantizer, "LinearW8A8Q.from_quantized (output quantizer)")
        base = LinearW8A8.from_quantized(weight_q, bias, input_quantizer)
        m = cls(base.in_features, base.out_features, bias=base.bias is not None, device=base.weight_levels.device,
                weight_dtype=base.weight_levels.dtype, input_range=base.input_range, relu=relu, mid_dtype=mid_dtype)
        for name in ("weight_levels", "weight_scale", "weight_zero_point", "input_scale", "input_shift", "bias"):
            setattr(m, name, getattr(base, name))
        m._set_output(output_quantizer, "LinearW8A8Q.from_quantized (output quantizer)", base.weight_levels.device)
        return m

    @classmethod
    def from_float(cls, layer, input_quantizer=None, output_quantizer=None, relu=False, mid_dtype=torch.float32):
        """from a (QAT) linear layer -- `torch.ao.nn.intrinsic.qat.LinearReLU` included, which sets relu -- as
        `LinearW8A8.from_float`; `output_quantizer` defaults to the layer's `activation_post_process`"""
        if _has_batch_norm(layer):
            raise ValueError("LinearW8A8Q.from_float: %s carries a batch norm, which is not folded (not served)" % type(layer).__name__)
        if output_quantizer is None:
            output_quantizer = getattr(layer, "activation_post_process", None)
        _per_tensor_constants(output_quantizer, "LinearW8A8Q.from_float (output quantizer)")
        base = LinearW8A8.from_float(layer, input_quantizer)
        with torch.no_grad():
            m = cls.from_quantized(layer.weight_fake_quant.quantize(layer.weight.detach()), layer.bias, input_quantizer,
                                   output_quantizer, relu or _fused_relu(layer), mid_dtype)
        m.train(base.training)
        return m


class Conv2dW8A8Q(Conv2dW8A8, _OutputQuantizer):
    """`Conv2dW8A8` with an 8-bit output: as `LinearW8A8Q`.  The returned levels are a logical [B, Cout, OH, OW] tensor in
    channels-last memory, the next convolution's operand as it lies.  Inference only."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, bias=True, device=None,
                 weight_dtype=torch.int8, input_range=(0, 255, 0, 255), output_range=(0, 255, 0, 255), relu=False,
                 mid_dtype=torch.float32):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, bias, device, weight_dtype, input_range)
        self._init_output(device, output_range, relu, mid_dtype)

    def forward(self, x):
        w = (self.weight_levels, self.weight_scale, self.weight_zero_point, self.bias, list(self.stride), list(self.padding),
             list(self.dilation))
        x = _as_levels(x)
        if isinstance(x, LevelsTensor):
            lv = torch.ops.torchlsq.lsq_conv2d_w8_q8_q(x.levels, x.scale, x.zero_point, *w, *self._out_args(), self.mid_dtype)
        else:
            lv = torch.ops.torchlsq.lsq_conv2d_w8_a8_q(x, self.input_scale, self.input_shift, *self.input_range, *w, *self._out_args())
        return self._wrap(lv)

    def get_extra_state(self):
        return dict(super().get_extra_state(), **self._output_state())

    def set_extra_state(self, state):
        super().set_extra_state(state)
        self._load_output_state(state)

    def extra_repr(self):
        return super().extra_repr() + self._output_repr()

    @classmethod
    def from_quantized(cls, weight_q, bias=None, input_quantizer=None, stride=1, padding=0, dilation=1, output_quantizer=None,
                       relu=False, mid_dtype=torch.float32):
        _per_tensor_constants(output_quantizer, "Conv2dW8A8Q.from_quantized (output quantizer)")
        base = Conv2dW8A8.from_quantized(weight_q, bias, input_quantizer, stride, padding, dilation)
        m = cls(base.in_channels, base.out_channels, base.kernel_size, base.stride, base.padding, base.dilation,
                bias=base.bias is not None, device=base.weight_levels.device, weight_dtype=base.weight_levels.dtype,
                input_range=base.input_range, relu=relu, mid_dtype=mid_dtype)
        for name in ("weight_levels", "weight_scale", "weight_zero_point", "input_scale", "input_shift", "bias"):
            setattr(m, name, getattr(base, name))
        m._set_output(output_quantizer, "Conv2dW8A8Q.from_quantized (output quantizer)", base.weight_levels.device)
        return m

    @classmethod
    def from_float(cls, layer, input_quantizer=None, output_quantizer=None, relu=False, mid_dtype=torch.float32):
        """from a (QAT) 2-D convolution with groups == 1 and zero padding -- `torch.ao.nn.intrinsic.qat.ConvReLU2d` included,
        which sets relu; a module with a batch norm is refused -- as `Conv2dW8A8.from_float`; `output_quantizer` defaults to the
        layer's `activation_post_process`"""
        if _has_batch_norm(layer):
            raise ValueError("Conv2dW8A8Q.from_float: %s carries a batch norm, which is not folded (not served)" % type(layer).__name__)
        if output_quantizer is None:
            output_quantizer = getattr(layer, "activation_post_process", None)
        _per_tensor_constants(input_quantizer, "Conv2dW8A8Q.from_float")
        _per_tensor_constants(output_quantizer, "Conv2dW8A8Q.from_float (output quantizer)")
        if not isinstance(layer, nn.Conv2d) or layer.groups != 1 or layer.padding_mode != "zeros":
            raise ValueError("Conv2dW8A8Q.from_float needs a 2-D convolution with groups == 1 and padding_mode 'zeros'")
        q = getattr(layer, "weight_fake_quant", None)
        if not (isinstance(q, LSQFakeQuantizer) and q.group_size is None and (not q.is_perchannel or q.ch_axis == 0)
                and getattr(q, "scale", None) is not None and q._initialized):
            raise ValueError("Conv2dW8A8Q.from_float needs a convolution whose weight_fake_quant is a trained per-channel (ch_axis 0) "
                             "or per-tensor LSQFakeQuantizer")
        with torch.no_grad():
            m = cls.from_quantized(q.quantize(layer.weight.detach()), layer.bias, input_quantizer, layer.stride, layer.padding,
                                   layer.dilation, output_quantizer, relu or _fused_relu(layer), mid_dtype)
        m.train(layer.training)
        return m


def _plain_or_relu_conv(mod):
    """_is_w8_conv, which refuses every fused module, with ConvReLU2d let through"""
    if _fused_relu(mod) and not _has_batch_norm(mod) and isinstance(mod, nn.Conv2d):
        q = getattr(mod, "weight_fake_quant", None)
        return (mod.groups == 1 and mod.padding_mode == "zeros" and isinstance(q, LSQFakeQuantizer) and q.group_size is None
                and (not q.is_perchannel or q.ch_axis == 0) and getattr(q, "scale", None) is not None and q._initialized)
    return _is_w8_conv(mod)


def convert_w8a8_q(model, input_quantizers, output_quantizers, relu=(), mid_dtype=torch.float32, inplace=False):
    """Replace the layers of `model` that `input_quantizers` lists -- a dict from a module's qualified name to the trained
    per-tensor `LSQFakeQuantizer` of its input -- by `LinearW8A8Q` / `Conv2dW8A8Q`.  `output_quantizers` maps the same names to
    the quantizer of the layer's output (the next layer's input quantizer); a name it leaves out takes the layer's
    `activation_post_process`.  `relu`: names whose layer is followed by a ReLU, which moves into the kernel -- when the layer
    sits in an `nn.Sequential` directly before an `nn.ReLU`, that module becomes an `nn.Identity`; otherwise remove the ReLU
    from the model's forward yourself.  `torch.ao.nn.intrinsic.qat.ConvReLU2d` and `LinearReLU` convert with relu on; a module
    with a batch norm is refused by name.  `mid_dtype`: the dtype in which the unfused model handed y to the next quantizer.
    Modules between two converted layers must pass a `LevelsTensor` on (`nn.Flatten` and `nn.Identity` do).  Returns the model
    (a deep copy unless inplace=True)."""
    if not inplace:
        model = copy.deepcopy(model)
    modules = dict(model.named_modules())
    unknown = [n for n in list(output_quantizers) + list(relu) if n not in input_quantizers]
    if unknown:
        raise ValueError("convert_w8a8_q: %r is listed in output_quantizers or relu but not in input_quantizers" % unknown[0])
    for name, quantizer in input_quantizers.items():
        child = modules.get(name)
        if child is not None and _has_batch_norm(child):
            raise ValueError("convert_w8a8_q: %r is a %s module: its batch norm is not folded (not served)" % (name, type(child).__name__))
        args = (child, quantizer, output_quantizers.get(name), name in relu, mid_dtype)
        if child is not None and _plain_or_relu_conv(child):
            new = Conv2dW8A8Q.from_float(*args)
        elif child is not None and _is_w8_linear(child):
            new = LinearW8A8Q.from_float(*args)
        else:
            raise ValueError("convert_w8a8_q: %r is not a linear layer or a 2-D convolution with groups == 1 and zero padding that "
                             "has a trained per-channel (ch_axis 0) or per-tensor LSQFakeQuantizer weight quantizer" % name)
        if name == "":
            return new
        parent_name, _, leaf = name.rpartition(".")
        parent = modules[parent_name]
        setattr(parent, leaf, new)
        if name in relu and isinstance(parent, nn.Sequential) and leaf.isdigit() and int(leaf) + 1 < len(parent) \
                and isinstance(parent[int(leaf) + 1], nn.ReLU):
            parent[int(leaf) + 1] = nn.Identity()
    return model
