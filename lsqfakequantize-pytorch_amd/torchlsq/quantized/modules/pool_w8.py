"""Pooling modules that keep a converted network in 8-bit LEVELS between its W8A8 layers: `MaxPool2dW8` (levels of the same
quantizer out), `AvgPool2dW8Q` and `AdaptiveAvgPool2dW8Q` (the levels of a trained per-tensor output quantizer out, or floats
when none is given) -- `torchlsq.functional.lsq_max_pool2d_w8` / `lsq_avg_pool2d_w8_q` / `lsq_avg_pool2d_w8`,
liblsq_hip_pool_w8.so on the GPU.  The forward takes a `LevelsTensor` (or a per-tensor quantized tensor); nothing is read back
to the host, and the chain can be captured in a graph.  `convert_w8a8_pool(model, pools, mid_dtype=...)` swaps the listed
pooling modules.
"""
import copy

import torch
from torch import nn

from torchlsq.functional import (LevelsTensor, _act_constants, lsq_adaptive_avg_pool2d_w8, lsq_avg_pool2d_w8, lsq_max_pool2d_w8)
from .packed_linear_a8 import _per_tensor_constants
from .w8a8_q import _MID_DTYPES, _as_levels


def _pair(v):
    return tuple(int(e) for e in v) if isinstance(v, (tuple, list)) else (int(v), int(v))


class MaxPool2dW8(nn.Module):
    """`nn.MaxPool2d` on a `LevelsTensor`: the byte max of each window, levels of the same quantizer out (the input's `scale`
    and `zero_point` tensors are handed on as they are).  Inference only."""

    def __init__(self, kernel_size, stride=None, padding=0, dilation=1, ceil_mode=False):
        super().__init__()
        self.kernel_size = _pair(kernel_size)
        self.stride = self.kernel_size if stride is None else _pair(stride)
        self.padding, self.dilation, self.ceil_mode = _pair(padding), _pair(dilation), bool(ceil_mode)

    def forward(self, x):
        return lsq_max_pool2d_w8(_as_levels(x), self.kernel_size, self.stride, self.padding, self.dilation, self.ceil_mode)

    def extra_repr(self):
        return "kernel_size=%s, stride=%s, padding=%s, dilation=%s, ceil_mode=%s" % (self.kernel_size, self.stride, self.padding,
                                                                                     self.dilation, self.ceil_mode)

    @classmethod
    def from_float(cls, pool, output_quantizer=None, mid_dtype=torch.float32):
        """from an `nn.MaxPool2d`; a max pool has no quantizer of its own (its output holds the input's levels)"""
        if not isinstance(pool, nn.MaxPool2d) or pool.return_indices:
            raise ValueError("MaxPool2dW8.from_float needs an nn.MaxPool2d without return_indices, got %s" % type(pool).__name__)
        if output_quantizer is not None:
            raise ValueError("MaxPool2dW8.from_float: a max pool hands on the levels of its input's quantizer; an output quantizer "
                             "is not served")
        m = cls(pool.kernel_size, pool.stride, pool.padding, pool.dilation, pool.ceil_mode)
        m.train(pool.training)
        return m


class _AvgPoolW8(nn.Module):
    """what the two average pools share: the output state of the `...Q` modules -- buffers `output_scale` and `output_shift`
    (float32 [1]); the output range, `mid_dtype` and `quantized` (False: the floating output) as extra state"""

    def _init_avg(self, device, output_range, mid_dtype, quantized):
        assert mid_dtype in _MID_DTYPES.values(), "mid_dtype must be torch.float32, torch.bfloat16 or torch.float16"
        self.register_buffer("output_scale", torch.ones(1, dtype=torch.float32, device=device))
        self.register_buffer("output_shift", torch.zeros(1, dtype=torch.float32, device=device))
        self.output_range = tuple(int(v) for v in output_range)
        self.mid_dtype, self.quantized = mid_dtype, bool(quantized)

    def get_extra_state(self):
        return dict(output_range=list(self.output_range), mid_dtype=str(self.mid_dtype).replace("torch.", ""), quantized=self.quantized)

    def set_extra_state(self, state):
        self.output_range = tuple(int(v) for v in state["output_range"])
        self.mid_dtype, self.quantized = _MID_DTYPES[state["mid_dtype"]], bool(state["quantized"])

    def _finish(self, pool, output_quantizer, what):
        if output_quantizer is not None:
            scale, shift, *rng = _per_tensor_constants(output_quantizer, what)
            device = self.output_scale.device
            self.output_scale, self.output_shift, self.output_range = scale.to(device), shift.to(device), tuple(rng)
        self.train(pool.training)
        return self

    def _wrap(self, levels):
        s, z = _act_constants(self.output_scale, self.output_shift, self.output_range[2], self.output_range[3])   # on the device
        return LevelsTensor(levels, s, z, *self.output_range)

    def _avg_repr(self):
        name = str(self.mid_dtype).replace("torch.", "")
        return (", output levels %d..%d, mid_dtype=%s" % (self.output_range[0], self.output_range[1], name) if self.quantized
                else ", floating output, dtype=%s" % name)


class AvgPool2dW8Q(_AvgPoolW8):
    """`nn.AvgPool2d` on a `LevelsTensor`: an exact integer window sum, two fp32 steps, a rounding to `mid_dtype` and the output
    quantizer's levels (a `LevelsTensor`), or -- built without an output quantizer -- the `mid_dtype` floats.  Inference only."""

    def __init__(self, kernel_size, stride=None, padding=0, ceil_mode=False, count_include_pad=True, divisor_override=None, device=None,
                 output_range=(0, 255, 0, 255), mid_dtype=torch.float32, quantized=True):
        super().__init__()
        self.kernel_size = _pair(kernel_size)
        self.stride = self.kernel_size if stride is None else _pair(stride)
        self.padding, self.ceil_mode, self.count_include_pad = _pair(padding), bool(ceil_mode), bool(count_include_pad)
        self.divisor_override = None if divisor_override is None else int(divisor_override)
        self._init_avg(device, output_range, mid_dtype, quantized)

    def forward(self, x):
        x = _as_levels(x)
        args = (x, self.kernel_size, self.stride, self.padding, self.ceil_mode, self.count_include_pad, self.divisor_override)
        if not self.quantized:
            return lsq_avg_pool2d_w8(*args, out_dtype=self.mid_dtype)
        lv = torch.ops.torchlsq.lsq_avg_pool2d_q8_q(x.levels, x.scale, x.zero_point, list(self.kernel_size), list(self.stride),
                                                    list(self.padding), self.ceil_mode, self.count_include_pad, self.divisor_override,
                                                    self.output_scale, self.output_shift, *self.output_range, self.mid_dtype)
        return self._wrap(lv)

    def extra_repr(self):
        return "kernel_size=%s, stride=%s, padding=%s%s" % (self.kernel_size, self.stride, self.padding, self._avg_repr())

    @classmethod
    def from_float(cls, pool, output_quantizer=None, mid_dtype=torch.float32, device=None):
        """from an `nn.AvgPool2d` and the trained per-tensor `LSQFakeQuantizer` of its output (None: floats out)"""
        what = "AvgPool2dW8Q.from_float (output quantizer)"
        if not isinstance(pool, nn.AvgPool2d):
            raise ValueError("AvgPool2dW8Q.from_float needs an nn.AvgPool2d, got %s" % type(pool).__name__)
        if output_quantizer is not None:
            _per_tensor_constants(output_quantizer, what)
            device = output_quantizer.scale.device if device is None else device
        m = cls(pool.kernel_size, pool.stride, pool.padding, pool.ceil_mode, pool.count_include_pad, pool.divisor_override, device,
                mid_dtype=mid_dtype, quantized=output_quantizer is not None)
        return m._finish(pool, output_quantizer, what)


class AdaptiveAvgPool2dW8Q(_AvgPoolW8):
    """`nn.AdaptiveAvgPool2d` on a `LevelsTensor`, for an output size that divides H and W evenly (1: global pooling), as
    `AvgPool2dW8Q`.  Inference only."""

    def __init__(self, output_size, device=None, output_range=(0, 255, 0, 255), mid_dtype=torch.float32, quantized=True):
        super().__init__()
        self.output_size = output_size
        self._init_avg(device, output_range, mid_dtype, quantized)

    def forward(self, x):
        x = _as_levels(x)
        if not self.quantized:
            return lsq_adaptive_avg_pool2d_w8(x, self.output_size, self.mid_dtype)
        kernel = list(_adaptive_kernel(x, self.output_size))
        lv = torch.ops.torchlsq.lsq_avg_pool2d_q8_q(x.levels, x.scale, x.zero_point, kernel, kernel, [0, 0], False, True, None,
                                                    self.output_scale, self.output_shift, *self.output_range, self.mid_dtype)
        return self._wrap(lv)

    def extra_repr(self):
        return "output_size=%s%s" % (self.output_size, self._avg_repr())

    @classmethod
    def from_float(cls, pool, output_quantizer=None, mid_dtype=torch.float32, device=None):
        """from an `nn.AdaptiveAvgPool2d` and the trained per-tensor `LSQFakeQuantizer` of its output (None: floats out)"""
        what = "AdaptiveAvgPool2dW8Q.from_float (output quantizer)"
        if not isinstance(pool, nn.AdaptiveAvgPool2d):
            raise ValueError("AdaptiveAvgPool2dW8Q.from_float needs an nn.AdaptiveAvgPool2d, got %s" % type(pool).__name__)
        if output_quantizer is not None:
            _per_tensor_constants(output_quantizer, what)
            device = output_quantizer.scale.device if device is None else device
        m = cls(pool.output_size, device, mid_dtype=mid_dtype, quantized=output_quantizer is not None)
        return m._finish(pool, output_quantizer, what)


def _adaptive_kernel(x, output_size):
    from torchlsq import extension
    return extension.pool_w8_adaptive_kernel(x.shape[2], x.shape[3], output_size)


def convert_w8a8_pool(model, pools, mid_dtype=torch.float32, inplace=False):
    """Replace the pooling modules of `model` that `pools` lists -- a dict from a module's qualified name to the trained per-tensor
    `LSQFakeQuantizer` of its OUTPUT, or to None -- by `MaxPool2dW8` (`nn.MaxPool2d`: its output holds the input's levels, a
    quantizer given for one is refused), `AvgPool2dW8Q` (`nn.AvgPool2d`) or `AdaptiveAvgPool2dW8Q` (`nn.AdaptiveAvgPool2d`); None
    on an average pool gives the floating output.  (torch.ao's prepare_qat gives pooling modules no `activation_post_process`,
    so there is no default to take the quantizer from.)  `mid_dtype`: the dtype in which the unfused model handed the pool's
    result to that quantizer.  Works beside `convert_w8a8_q` / `convert_w8a8_add_q` on disjoint names.  Returns the model (a deep
    copy unless inplace=True)."""
    assert mid_dtype in _MID_DTYPES.values(), "mid_dtype must be torch.float32, torch.bfloat16 or torch.float16"
    if not inplace:
        model = copy.deepcopy(model)
    modules = dict(model.named_modules())
    for name, quantizer in pools.items():
        child = modules.get(name)
        if isinstance(child, nn.MaxPool2d):
            if quantizer is not None:
                raise ValueError("convert_w8a8_pool: %r is a max pool, which hands on the levels of its input's quantizer; give None, "
                                 "not an output quantizer" % name)
            new = MaxPool2dW8.from_float(child)
        elif isinstance(child, nn.AvgPool2d):
            new = AvgPool2dW8Q.from_float(child, quantizer, mid_dtype)
        elif isinstance(child, nn.AdaptiveAvgPool2d):
            new = AdaptiveAvgPool2dW8Q.from_float(child, quantizer, mid_dtype)
        else:
            raise ValueError("convert_w8a8_pool: %r is not an nn.MaxPool2d, nn.AvgPool2d or nn.AdaptiveAvgPool2d (got %s)"
                             % (name, type(child).__name__))
        if name == "":
            return new
        parent_name, _, leaf = name.rpartition(".")
        setattr(modules[parent_name], leaf, new)
    return model
