"""Deployment of group-wise QAT linear layers: `PackedLinear` keeps a weight as packed 4- / 2-bit codes with one (scale, zero
point) per group -- the format of include/lsq_hip_pack.h -- and computes `y = x @ w^T + bias` straight from the codes
(`torchlsq.functional.lsq_linear_packed`, liblsq_hip_qlinear.so on the GPU).  `convert_packed(model)` swaps every linear layer
whose `weight_fake_quant` is a group-wise `LSQFakeQuantizer` for one; afterwards no module holds a full-precision copy of a
converted weight.
"""
import copy

import torch
from torch import nn

from torchlsq.functional import PackedGroupTensor, lsq_linear_packed
from .observers import LSQFakeQuantizer


class PackedLinear(nn.Module):
    """`nn.Linear` on a packed weight.  Buffers: `codes` (uint8 [out, in * bits / 8]), `scale` (float32 [out, in / G]),
    `zero_point` (int32 [out, in / G]); `bias` is a parameter as before (or None).  bits, group_size and quant_min travel in
    the state dict as extra state, so `load_state_dict` restores a layer built with other settings of the same shapes.
    Inference only (the op refuses an input that requires grad)."""

    def __init__(self, in_features, out_features, bits=4, group_size=32, quant_min=-8, bias=True, device=None):
        super().__init__()
        assert bits in (2, 4) and in_features % group_size == 0 and group_size % (8 // bits) == 0
        self.in_features, self.out_features = int(in_features), int(out_features)
        self.bits, self.group_size, self.quant_min = int(bits), int(group_size), int(quant_min)
        groups = in_features // group_size
        self.register_buffer("codes", torch.zeros(out_features, in_features * bits // 8, dtype=torch.uint8, device=device))
        self.register_buffer("scale", torch.ones(out_features, groups, dtype=torch.float32, device=device))
        self.register_buffer("zero_point", torch.zeros(out_features, groups, dtype=torch.int32, device=device))
        self.bias = nn.Parameter(torch.zeros(out_features, device=device), requires_grad=False) if bias else None
        self.activation_post_process = None

    def packed(self) -> PackedGroupTensor:
        """the weight as a `PackedGroupTensor` (views of the buffers)"""
        return PackedGroupTensor(self.codes, self.scale, self.zero_point, self.bits, self.group_size, self.quant_min,
                                 (self.out_features, self.in_features))

    def forward(self, x):
        y = lsq_linear_packed(x, self.packed(), self.bias)
        return y if self.activation_post_process is None else self.activation_post_process(y)

    def get_extra_state(self):
        return dict(bits=self.bits, group_size=self.group_size, quant_min=self.quant_min)

    def set_extra_state(self, state):
        self.bits, self.group_size, self.quant_min = int(state["bits"]), int(state["group_size"]), int(state["quant_min"])

    def extra_repr(self):
        return "in_features=%d, out_features=%d, bits=%d, group_size=%d, bias=%s" % (
            self.in_features, self.out_features, self.bits, self.group_size, self.bias is not None)

    @classmethod
    def from_packed(cls, p: PackedGroupTensor, bias=None):
        """from a packed 2-D weight [out, in] (a float64 scale is kept as float32: the kernel computes in float32)"""
        assert len(p.shape) == 2, "PackedLinear needs a 2-D weight, got shape %s" % (tuple(p.shape),)
        out_f, in_f = p.shape
        m = cls(in_f, out_f, p.bits, p.group_size, p.quant_min, bias=bias is not None, device=p.codes.device)
        groups = in_f // p.group_size
        m.codes = p.codes.detach().reshape(out_f, -1).clone()
        m.scale = p.scale.detach().reshape(out_f, groups).to(torch.float32).clone()
        m.zero_point = p.zero_point.detach().reshape(out_f, groups).clone()
        if bias is not None:
            m.bias = nn.Parameter(bias.detach().clone(), requires_grad=False)
        return m

    @classmethod
    def from_float(cls, layer, bits=None):
        """from a (QAT) linear layer whose `weight_fake_quant` is a trained group-wise `LSQFakeQuantizer`; an output
        `activation_post_process` of the layer is kept"""
        q = getattr(layer, "weight_fake_quant", None)
        if not isinstance(q, LSQFakeQuantizer) or q.group_size is None:
            raise ValueError("PackedLinear.from_float needs a linear layer whose weight_fake_quant is a group-wise "
                             "LSQFakeQuantizer (group_size=...)")
        m = cls.from_packed(q.export_packed(layer.weight.detach(), bits), layer.bias)
        post = getattr(layer, "activation_post_process", None)
        if post is not None and not isinstance(post, nn.Identity):
            m.activation_post_process = post
        m.train(layer.training)
        return m


def _is_groupwise_linear(mod):
    q = getattr(mod, "weight_fake_quant", None)
    return isinstance(mod, nn.Linear) and isinstance(q, LSQFakeQuantizer) and q.group_size is not None


def convert_packed(model, inplace=False):
    """Replace every linear layer of `model` whose `weight_fake_quant` is a group-wise `LSQFakeQuantizer` by a `PackedLinear`
    built from it; everything else is left alone.  Returns the model (a deep copy unless inplace=True)."""
    if not inplace:
        model = copy.deepcopy(model)
    if _is_groupwise_linear(model):
        return PackedLinear.from_float(model)
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if _is_groupwise_linear(child):
                setattr(parent, name, PackedLinear.from_float(child))
    return model
