"""The gated MLP of a Llama / Mistral / Qwen / Gemma block on 8-bit LEVELS with PACKED 4- / 2-bit group-wise weights:
`GatedMLPPackedA8Q` is `down(act(gate(x)) * up(x))` as `GatedMLPW8Q` is it for 8-bit weight levels -- ONE fused gate_up
`PackedLinearA8Q` whose halves the product reads in place where gate and up share an output quantizer, `GLUW8Q` for the product, a
`PackedLinearA8Q` / `PackedLinearA8AddQ` down projection -- and, where `glu_epilogue` resolves to True and x has at most 16 rows, the
projections and the product in ONE launch (`lsq_linear_packed_q8_glu_q`, liblsq_hip_linglu_w4.so) with the same bytes.
`convert_packed_a8_glu(model, {mlp_name: dict(...)})` swaps the listed MLP modules.
"""
import copy

import torch
from torch import nn

from torchlsq import functional as F
from torchlsq.functional import LevelsTensor, _act_constants, _takes_decode
from .glu_w8 import _GLU_KEYS, _GLU_NEEDED, GLUW8Q
from .packed_a8_q import PackedLinearA8AddQ, PackedLinearA8Q
from .packed_linear import _is_groupwise_linear
from .w8a8_q import _MID_DTYPES, _as_levels


def _fuse_packed(a, b):
    """ONE `PackedLinearA8Q` whose output rows are a's, then b's: the codes, their per-group constants and the biases concatenated
    along N; a and b share their format and their input and output quantizers"""
    assert (a.bias is None) == (b.bias is None) and (a.bits, a.group_size, a.quant_min) == (b.bits, b.group_size, b.quant_min), \
        "a fused gate_up linear needs both projections with or both without a bias, and one packed format"
    m = PackedLinearA8Q(a.in_features, a.out_features + b.out_features, a.bits, a.group_size, a.quant_min, bias=a.bias is not None,
                        device=a.codes.device, input_range=a.input_range, output_range=a.output_range, relu=False, mid_dtype=a.mid_dtype)
    for name in ("codes", "scale", "zero_point"):
        setattr(m, name, torch.cat([getattr(a, name), getattr(b, name)], 0).contiguous())
    for name in ("input_scale", "input_shift", "output_scale", "output_shift"):
        setattr(m, name, getattr(a, name).clone())
    if a.bias is not None:
        m.bias = nn.Parameter(torch.cat([a.bias.detach(), b.bias.detach()], 0), requires_grad=False)
    m.decode = a.decode
    return m


class GatedMLPPackedA8Q(nn.Module):
    """`down(act(gate_proj(x)) * up_proj(x))` on levels with packed weights.  Children: `gate_up` (ONE `PackedLinearA8Q` of 2 C output
    rows, gate's then up's) or `gate_proj` and `up_proj` (two of one format), `glu` (`GLUW8Q`) and `down` (`PackedLinearA8Q` /
    `PackedLinearA8AddQ`).  `forward(x, residual=None)`: x a `LevelsTensor`; the residual, a `LevelsTensor`, is handed to a
    `PackedLinearA8AddQ` down.  `glu_epilogue` (extra state, kept only when it is not None; True / False / None:
    `torchlsq.functional.W4A8_GLU_EPILOGUE_DEFAULT`): where it resolves to True and x has at most 16 rows, the projections and the
    product are ONE op (`lsq_linear_packed_q8_glu_q`) with the same bytes.  Inference only."""

    def __init__(self, glu, down, gate_up=None, gate_proj=None, up_proj=None, glu_epilogue=None):
        super().__init__()
        assert (gate_up is None) != (gate_proj is None) and (gate_proj is None) == (up_proj is None), \
            "GatedMLPPackedA8Q takes one fused gate_up linear or the pair gate_proj, up_proj"
        self.fused = gate_up is not None
        if self.fused:
            self.gate_up = gate_up
        else:
            self.gate_proj, self.up_proj = gate_proj, up_proj
        self.glu, self.down = glu, down
        self.glu_epilogue = glu_epilogue

    def _projections(self):
        """(codes, scale, zero_point, bias) of gate and of up -- the row halves of the fused linear as views -- and their two linears"""
        if not self.fused:
            g, u = self.gate_proj, self.up_proj
            return (g.codes, g.scale, g.zero_point, g.bias), (u.codes, u.scale, u.zero_point, u.bias), g, u
        m, C = self.gate_up, self.gate_up.out_features // 2
        w = (m.codes, m.scale, m.zero_point, m.bias)
        return tuple(None if t is None else t[:C] for t in w), tuple(None if t is None else t[C:] for t in w), m, m

    def _product_in_epilogue(self, x):
        gw, uw, g, u = self._projections()
        glu = self.glu
        s_u, z_u = _act_constants(u.output_scale, u.output_shift, u.output_range[2], u.output_range[3])      # u._wrap's, on the device
        flat = lambda w: (w[0], w[1].reshape(-1), w[2].reshape(-1), w[3])
        lv = torch.ops.torchlsq.lsq_linear_packed_q8_glu_q(x.levels, x.scale, x.zero_point, *flat(gw), g.output_scale, g.output_shift,
                                                           *g.output_range, *flat(uw), u.output_scale, u.output_shift, *u.output_range,
                                                           g.group_size, g.bits, s_u, z_u, glu.table, glu.output_scale, glu.output_shift,
                                                           *glu.output_range, glu.mid_dtype)
        return glu._wrap(lv)

    def forward(self, x, residual=None):
        x = _as_levels(x)
        lins = (self.gate_up,) if self.fused else (self.gate_proj, self.up_proj)
        takes = F.W4A8_GLU_EPILOGUE_DEFAULT if self.glu_epilogue is None else self.glu_epilogue
        if isinstance(x, LevelsTensor) and _takes_decode(takes, x.levels) and \
                all(type(m) is PackedLinearA8Q and not m.relu and m.mid_dtype == self.glu.mid_dtype for m in lins) and \
                (lins[0].bits, lins[0].group_size) == (lins[-1].bits, lins[-1].group_size):
            h = self._product_in_epilogue(x)
        else:
            h = self.glu(self.gate_up(x)) if self.fused else self.glu(self.gate_proj(x), self.up_proj(x))
        if residual is not None:
            if not isinstance(self.down, PackedLinearA8AddQ):
                raise TypeError("GatedMLPPackedA8Q: a residual needs a PackedLinearA8AddQ as the down projection, got %s"
                                % type(self.down).__name__)
            return self.down(h, residual)
        return self.down(h)

    def get_extra_state(self):
        return dict(glu_epilogue=self.glu_epilogue)

    def set_extra_state(self, state):
        self.glu_epilogue = state.get("glu_epilogue")

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        if self.glu_epilogue is None:       # the default is not written: a default module's state dict has no extra key
            destination.pop(prefix + "_extra_state", None)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        state_dict.setdefault(prefix + "_extra_state", {})      # no key: None
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def extra_repr(self):
        return "" if self.glu_epilogue is None else "glu_epilogue=%s" % self.glu_epilogue

    @classmethod
    def from_float(cls, gate_proj, up_proj, down, act, input_quantizer, gate_quantizer, up_quantizer, hidden_quantizer,
                   act_quantizer=None, mid_dtype=torch.float32, decode=None, glu_epilogue=None):
        """from the (QAT) linear layers `gate_proj` and `up_proj` with trained group-wise weight quantizers of one format, the
        ALREADY CONVERTED down projection (`PackedLinearA8Q` / `PackedLinearA8AddQ`), the activation, and the trained per-tensor
        `LSQFakeQuantizer`s of the MLP's input, of the two projections' outputs, of the product (the down projection's input) and,
        where the model has one, of the activation's output.  When `gate_quantizer is up_quantizer` the two projections become ONE
        linear and the product reads its halves in place; otherwise two.  `decode` becomes the `decode` attribute of the
        projections made here (the down projection keeps its own), `glu_epilogue` the module's."""
        if not isinstance(down, PackedLinearA8Q):
            raise ValueError("GatedMLPPackedA8Q.from_float: the down projection must be a converted PackedLinearA8Q or PackedLinearA8AddQ, "
                             "got %s" % type(down).__name__)
        if gate_proj.out_features != up_proj.out_features or gate_proj.in_features != up_proj.in_features or \
                down.in_features != gate_proj.out_features:
            raise ValueError("GatedMLPPackedA8Q.from_float: gate_proj and up_proj must have one shape [C, K] and down must read C features")
        g = PackedLinearA8Q.from_float(gate_proj, input_quantizer, gate_quantizer, False, mid_dtype)
        u = PackedLinearA8Q.from_float(up_proj, input_quantizer, up_quantizer, False, mid_dtype)
        if (g.bits, g.group_size) != (u.bits, u.group_size):
            raise ValueError("GatedMLPPackedA8Q.from_float: gate_proj and up_proj must have one bits and one group_size, got %d / %d and "
                             "%d / %d" % (g.bits, g.group_size, u.bits, u.group_size))
        g.decode = u.decode = decode
        glu = GLUW8Q.from_float(act, gate_quantizer, hidden_quantizer, act_quantizer, mid_dtype, device=g.codes.device)
        if gate_quantizer is up_quantizer and g.quant_min == u.quant_min:
            m = cls(glu, down, gate_up=_fuse_packed(g, u), glu_epilogue=glu_epilogue)
        else:
            m = cls(glu, down, gate_proj=g, up_proj=u, glu_epilogue=glu_epilogue)
        m.train(gate_proj.training)
        return m


def convert_packed_a8_glu(model, mlps, mid_dtype=torch.float32, inplace=False, decode=None, glu_epilogue=None):
    """`convert_w8a8_glu` for gated MLPs whose `gate_proj`, `up_proj` and `down_proj` carry trained GROUP-WISE weight quantizers:
    `mlps` maps the qualified name of such a module (with an `act_fn` or `act` child) to the same dict of trained per-tensor
    `LSQFakeQuantizer`s -- `input_quantizer`, `gate_quantizer`, `up_quantizer` (the same object as `gate_quantizer`: ONE fused
    gate_up linear), `hidden_quantizer`, `down_output_quantizer` and optionally `act_quantizer` and `add_quantizer` (the down
    projection becomes a `PackedLinearA8AddQ`).  The module becomes a `GatedMLPPackedA8Q`.  Anything else is refused by name.
    `decode` becomes the `decode` attribute of every linear layer made here, `glu_epilogue` that of every `GatedMLPPackedA8Q`.
    Returns the model (a deep copy unless inplace=True)."""
    assert mid_dtype in _MID_DTYPES.values(), "mid_dtype must be torch.float32, torch.bfloat16 or torch.float16"
    if not inplace:
        model = copy.deepcopy(model)
    modules = dict(model.named_modules())
    swaps = []
    for name, q in mlps.items():
        child = modules.get(name)
        act = None if child is None else getattr(child, "act_fn", getattr(child, "act", None))
        if child is None or act is None or not all(_is_groupwise_linear(getattr(child, n, None)) for n in ("gate_proj", "up_proj", "down_proj")):
            raise ValueError("convert_packed_a8_glu: %r is not a gated MLP with gate_proj, up_proj and down_proj linear children that have "
                             "group-wise weight quantizers and an act_fn (or act) (got %s)" % (name, type(child).__name__))
        if not isinstance(q, dict) or any(k not in _GLU_KEYS for k in q) or any(k not in q for k in _GLU_NEEDED):
            raise ValueError("convert_packed_a8_glu: %r needs a dict with input_quantizer, gate_quantizer, up_quantizer, hidden_quantizer "
                             "and down_output_quantizer (optionally act_quantizer, add_quantizer)" % name)
        if q.get("add_quantizer") is not None:
            down = PackedLinearA8AddQ.from_float(child.down_proj, q["hidden_quantizer"], q["add_quantizer"], q["down_output_quantizer"],
                                                 mid_dtype=mid_dtype)
        else:
            down = PackedLinearA8Q.from_float(child.down_proj, q["hidden_quantizer"], q["down_output_quantizer"], False, mid_dtype)
        down.decode = decode
        swaps.append((name, GatedMLPPackedA8Q.from_float(child.gate_proj, child.up_proj, down, act, q["input_quantizer"],
                                                         q["gate_quantizer"], q["up_quantizer"], q["hidden_quantizer"],
                                                         q.get("act_quantizer"), mid_dtype, decode, glu_epilogue)))
    for name, new in swaps:
        if name == "":
            return new
        parent_name, _, leaf = name.rpartition(".")
        setattr(modules[parent_name], leaf, new)
    return model
