"""W4A8 / W2A8 layers that hand 8-bit LEVELS to the next layer: `PackedLinearA8Q` is `PackedLinearA8` with the trained per-tensor
quantizer of its OUTPUT and an optional ReLU, `PackedLinearA8AddQ` adds a residual `LevelsTensor` before them, after the layer's own
optional output fake-quantizer (`torchlsq.functional.lsq_linear_packed_a8_q` / `lsq_linear_packed_a8_add_q`; on the GPU one launch of
liblsq_hip_lindec_w4.so for at most 16 rows with `decode`, the existing ops composed otherwise, the same bytes either way).  The
forward takes a `LevelsTensor` or a per-tensor quantized tensor and returns a `LevelsTensor`: a floating x is not served.
`convert_packed_a8_q(model, input_quantizers, output_quantizers, relu=(), mid_dtype=...)` swaps the listed group-wise layers.
"""
import copy

import torch
from torch import nn

from torchlsq.functional import lsq_linear_packed_a8_add_q, lsq_linear_packed_a8_q
from .packed_linear import _is_groupwise_linear
from .packed_linear_a8 import PackedLinearA8, _per_tensor_constants
from .w8a8_add_q import _LAYER_S, _PreQuantizer, _layer_pre
from .w8a8_q import _OutputQuantizer, _as_levels


class PackedLinearA8Q(PackedLinearA8, _OutputQuantizer):
    """`PackedLinearA8` with an 8-bit output.  Extra state: `PackedLinearA8`'s, the output range, `relu`, `mid_dtype`, and `decode`
    when it is not None (True: liblsq_hip_lindec_w4.so for at most 16 rows, liblsq_hip_linmid_w4.so for 17 to 64 and blocks of 64 rows
    below `qgemm_a8_min_rows()`; False: never; None: `W4A8_DECODE_DEFAULT` up to 16 rows, `W4A8_MID_DEFAULT` beyond: the faster of the two
    libraries per block of rows).  Inference only."""

    def __init__(self, in_features, out_features, bits=4, group_size=32, quant_min=-8, bias=True, device=None,
                 input_range=(0, 255, 0, 255), output_range=(0, 255, 0, 255), relu=False, mid_dtype=torch.float32):
        super().__init__(in_features, out_features, bits, group_size, quant_min, bias, device, input_range)
        self._init_output(device, output_range, relu, mid_dtype)
        self.decode = None

    def forward(self, x):
        return lsq_linear_packed_a8_q(_as_levels(x), self.packed(), self.bias, *self._out_args(), self.mid_dtype, self.decode)

    def get_extra_state(self):
        state = dict(super().get_extra_state(), **self._output_state())
        if self.decode is not None:
            state["decode"] = bool(self.decode)
        return state

    def set_extra_state(self, state):
        super().set_extra_state(state)
        self._load_output_state(state)
        self.decode = state.get("decode")

    def extra_repr(self):
        return super().extra_repr() + self._output_repr() + ("" if self.decode is None else ", decode=%s" % self.decode)

    @classmethod
    def from_float(cls, layer, input_quantizer=None, output_quantizer=None, relu=False, mid_dtype=torch.float32, bits=None):
        """from a (QAT) linear layer with a trained group-wise weight quantizer, as `PackedLinearA8.from_float`; `output_quantizer`
        defaults to the layer's `activation_post_process`"""
        what = "%s.from_float (output quantizer)" % cls.__name__
        if output_quantizer is None:
            output_quantizer = getattr(layer, "activation_post_process", None)
        _per_tensor_constants(output_quantizer, what)
        base = PackedLinearA8.from_float(layer, input_quantizer, bits)
        m = cls(base.in_features, base.out_features, base.bits, base.group_size, base.quant_min, bias=base.bias is not None,
                device=base.codes.device, input_range=base.input_range, relu=relu, mid_dtype=mid_dtype)
        for name in ("codes", "scale", "zero_point", "bias", "input_scale", "input_shift"):
            setattr(m, name, getattr(base, name))
        m._set_output(output_quantizer, what, base.codes.device)
        m.train(base.training)
        return m


class PackedLinearA8AddQ(_PreQuantizer, PackedLinearA8Q):
    """`PackedLinearA8Q` with a residual.  `forward(x, residual)` takes the residual as a `LevelsTensor` of the output's shape and
    returns a `LevelsTensor`; `forward(x)` returns a `PendingAdd` for an `AddW8A8Q`.  Inference only."""

    def __init__(self, *args, device=None, **kwargs):
        super().__init__(*args, device=device, **kwargs)
        self._init_pre(device)

    def _launch(self, x, residual, relu):
        pre = (None,) * 6 if self.pre_range is None else (self.pre_scale, self.pre_shift, *self.pre_range)
        return lsq_linear_packed_a8_add_q(_as_levels(x), self.packed(), self.bias, _as_levels(residual), *self._out_args_with(relu),
                                          self.mid_dtype, *pre, self.decode)

    @classmethod
    def from_float(cls, layer, input_quantizer=None, output_quantizer=None, pre_quantizer=_LAYER_S, relu=False,
                   mid_dtype=torch.float32, bits=None):
        """as `PackedLinearA8Q.from_float`, with `output_quantizer` the ADD's quantizer (required) and `pre_quantizer` the layer's
        own output fake-quantizer: by default its `activation_post_process` if it has one, None for none"""
        pre = _layer_pre(layer, pre_quantizer)
        m = super().from_float(layer, input_quantizer, output_quantizer, relu, mid_dtype, bits)
        m._set_pre(pre, "PackedLinearA8AddQ.from_float (pre-quantizer)", m.codes.device)
        return m


def convert_packed_a8_q(model, input_quantizers, output_quantizers, relu=(), mid_dtype=torch.float32, inplace=False, decode=None):
    """Replace the group-wise linear layers of `model` that `input_quantizers` lists -- a dict from a module's qualified name to the
    trained per-tensor `LSQFakeQuantizer` of its input -- by `PackedLinearA8Q`.  `output_quantizers` maps the same names to the
    quantizer of the layer's output (the next layer's input quantizer); a name it leaves out takes the layer's
    `activation_post_process`.  `relu`: names whose layer is followed by a ReLU, which moves into the op -- an `nn.ReLU` directly
    behind the layer in an `nn.Sequential` becomes an `nn.Identity`.  `decode` becomes the `decode` attribute of every converted
    layer.  Returns the model (a deep copy unless inplace=True)."""
    if not inplace:
        model = copy.deepcopy(model)
    modules = dict(model.named_modules())
    unknown = [n for n in list(output_quantizers) + list(relu) if n not in input_quantizers]
    if unknown:
        raise ValueError("convert_packed_a8_q: %r is listed in output_quantizers or relu but not in input_quantizers" % unknown[0])
    for name, quantizer in input_quantizers.items():
        child = modules.get(name)
        if child is None or not _is_groupwise_linear(child):
            raise ValueError("convert_packed_a8_q: %r is not a linear layer with a group-wise LSQFakeQuantizer weight quantizer" % name)
        new = PackedLinearA8Q.from_float(child, quantizer, output_quantizers.get(name), name in relu, mid_dtype)
        new.decode = decode
        if name == "":
            return new
        parent_name, _, leaf = name.rpartition(".")
        parent = modules[parent_name]
        setattr(parent, leaf, new)
        if name in relu and isinstance(parent, nn.Sequential) and leaf.isdigit() and int(leaf) + 1 < len(parent) \
                and isinstance(parent[int(leaf) + 1], nn.ReLU):
            parent[int(leaf) + 1] = nn.Identity()
    return model
