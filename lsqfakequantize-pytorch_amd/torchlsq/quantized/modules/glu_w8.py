"""The gated MLP of a Llama / Mistral / Qwen / Gemma block on 8-bit LEVELS: `GLUW8Q` is the gated product `act(gate) * up`
between the gate_up linear and the down linear (the activation as a 256-entry float table on the gate byte, built once at
conversion; `torchlsq.functional.lsq_glu_table` / `lsq_glu_w8_q`, liblsq_hip_glu_w8.so on the GPU), and `GatedMLPW8Q` is the
whole `down(act(gate(x)) * up(x))` -- with ONE fused gate_up linear whose halves the product reads in place where gate and up
share an output quantizer.  The forwards take and return `LevelsTensor`s; nothing is read back to the host, and the chain can be
captured in a graph.  `convert_w8a8_glu(model, {mlp_name: dict(...)})` swaps the listed MLP modules.
"""
import copy

import torch
from torch import nn

from torchlsq.functional import LevelsTensor, _act_constants, act_function, lsq_glu_table
from .eltwise_w8 import _EltwiseOutput, _level_dtype
from .packed_linear_a8 import _per_tensor_constants
from .w8a8_add_q import LinearW8A8AddQ
from .w8a8_q import _MID_DTYPES, LinearW8A8Q, _as_levels


class GLUW8Q(_EltwiseOutput):
    """The gated product on `LevelsTensor`s: buffers `table` (float32 [256], indexed by the gate level's byte as stored, holding
    values of `mid_dtype`), `output_scale` and `output_shift`; the output range, `mid_dtype` and the function's name travel in
    the extra state (the table is what computes).  `forward(gate, up)` takes two `LevelsTensor`s of one shape [.., C];
    `forward(gate_up)` takes ONE of [.., 2 C] and cuts its last axis into halves as views, which the kernel reads in place.  One
    launch; returns the dense `LevelsTensor` of the output quantizer.  Inference only."""

    def __init__(self, device=None, output_range=(0, 255, 0, 255), mid_dtype=torch.float32, function="identity"):
        super().__init__()
        self.register_buffer("table", torch.zeros(256, dtype=torch.float32, device=device))
        self._init_output(device, output_range, mid_dtype)
        self.function = str(function)

    def forward(self, gate, up=None):
        gate = _as_levels(gate)
        if up is None:
            assert isinstance(gate, LevelsTensor) and gate.shape[-1] % 2 == 0, \
                "GLUW8Q(gate_up) needs one LevelsTensor whose last axis holds gate and up, an even number of columns"
            C = gate.shape[-1] // 2
            rng = (gate.scale, gate.zero_point, gate.quant_min, gate.quant_max, gate.type_min, gate.type_max)
            gate, up = LevelsTensor(gate.levels[..., :C], *rng), LevelsTensor(gate.levels[..., C:], *rng)
        up = _as_levels(up)
        if not (isinstance(gate, LevelsTensor) and isinstance(up, LevelsTensor)):
            raise TypeError("GLUW8Q needs two LevelsTensors (or per-tensor quantized tensors), got %s and %s"
                            % (type(gate).__name__, type(up).__name__))
        lv = torch.ops.torchlsq.lsq_glu_w8_q8_q(gate.levels, up.levels, up.scale, up.zero_point, self.table, self.output_scale,
                                                self.output_shift, *self.output_range, self.mid_dtype)
        return self._wrap(lv)

    def get_extra_state(self):
        return dict(super().get_extra_state(), function=self.function)

    def set_extra_state(self, state):
        super().set_extra_state(state)
        self.function = str(state["function"])

    def extra_repr(self):
        return "%s(gate) * up, %s" % (self.function, self._output_repr())

    @classmethod
    def from_float(cls, act, gate_quantizer, output_quantizer, act_quantizer=None, mid_dtype=torch.float32, device=None):
        """from the activation (a name, a `torch.nn` activation module or a callable: `torchlsq.functional.act_function`), the
        trained per-tensor `LSQFakeQuantizer` of the gate projection's output, that of the product and, where the model
        quantizes between the activation and the product, that one.  The table is built here, once, on `device` (default: the
        output quantizer's) from existing ops: build it on the device whose unfused chain it has to equal."""
        what = "GLUW8Q.from_float"
        g_scale, g_shift, *g_rng = _per_tensor_constants(gate_quantizer, what + " (gate quantizer)")
        _per_tensor_constants(output_quantizer, what + " (output quantizer)")
        device = output_quantizer.scale.device if device is None else torch.device(device)
        act_out = None
        if act_quantizer is not None:
            a_scale, a_shift, *a_rng = _per_tensor_constants(act_quantizer, what + " (activation quantizer)")
            act_out = (a_scale.to(device), a_shift.to(device), *a_rng)
        _, name = act_function(act)
        m = cls(device, mid_dtype=mid_dtype, function=name)
        m._set_output(output_quantizer, what + " (output quantizer)")
        s, z = _act_constants(g_scale.to(device), g_shift.to(device), g_rng[2], g_rng[3])
        with torch.no_grad():
            m.table = lsq_glu_table(act, s, z, _level_dtype(g_rng), act_out, mid_dtype)
        m.train(act.training if isinstance(act, nn.Module) else False)
        return m


def _fuse_linears(a, b):
    """ONE `LinearW8A8Q` whose output rows are a's, then b's: the weights, their per-row constants and the biases concatenated
    along N; a and b share their input and output quantizers"""
    assert (a.bias is None) == (b.bias is None) and a.weight_levels.dtype == b.weight_levels.dtype, \
        "a fused gate_up linear needs both projections with or both without a bias, and one weight level type"
    m = LinearW8A8Q(a.in_features, a.out_features + b.out_features, bias=a.bias is not None, device=a.weight_levels.device,
                    weight_dtype=a.weight_levels.dtype, input_range=a.input_range, output_range=a.output_range, relu=False,
                    mid_dtype=a.mid_dtype)
    for name in ("weight_levels", "weight_scale", "weight_zero_point"):
        setattr(m, name, torch.cat([getattr(a, name), getattr(b, name)], 0).contiguous())
    for name in ("input_scale", "input_shift", "output_scale", "output_shift"):
        setattr(m, name, getattr(a, name).clone())
    if a.bias is not None:
        m.bias = nn.Parameter(torch.cat([a.bias.detach(), b.bias.detach()], 0), requires_grad=False)
    return m


class GatedMLPW8Q(nn.Module):
    """`down(act(gate_proj(x)) * up_proj(x))` on levels.  Children: `gate_up` (ONE `LinearW8A8Q` of 2 C output rows, gate's then
    up's) or `gate_proj` and `up_proj` (two), `glu` (`GLUW8Q`) and `down` (`LinearW8A8Q` / `LinearW8A8AddQ`).
    `forward(x, residual=None)`: x a `LevelsTensor`; the residual, a `LevelsTensor`, is handed to a `LinearW8A8AddQ` down.
    Inference only."""

    def __init__(self, glu, down, gate_up=None, gate_proj=None, up_proj=None):
        super().__init__()
        assert (gate_up is None) != (gate_proj is None) and (gate_proj is None) == (up_proj is None), \
            "GatedMLPW8Q takes one fused gate_up linear or the pair gate_proj, up_proj"
        self.fused = gate_up is not None
        if self.fused:
            self.gate_up = gate_up
        else:
            self.gate_proj, self.up_proj = gate_proj, up_proj
        self.glu, self.down = glu, down

    def forward(self, x, residual=None):
        h = self.glu(self.gate_up(x)) if self.fused else self.glu(self.gate_proj(x), self.up_proj(x))
        if residual is not None:
            if not isinstance(self.down, LinearW8A8AddQ):
                raise TypeError("GatedMLPW8Q: a residual needs a LinearW8A8AddQ as the down projection, got %s" % type(self.down).__name__)
            return self.down(h, residual)
        return self.down(h)

    @classmethod
    def from_float(cls, gate_proj, up_proj, down, act, input_quantizer, gate_quantizer, up_quantizer, hidden_quantizer,
                   act_quantizer=None, mid_dtype=torch.float32):
        """from the (QAT) linear layers `gate_proj` and `up_proj`, the ALREADY CONVERTED down projection (`LinearW8A8Q` /
        `LinearW8A8AddQ`), the activation, and the trained per-tensor `LSQFakeQuantizer`s of the MLP's input, of the two
        projections' outputs, of the product (the down projection's input) and, where the model has one, of the activation's
        output.  When `gate_quantizer is up_quantizer` the two projections become ONE linear and the product reads its halves
        in place; otherwise two."""
        if not isinstance(down, (LinearW8A8Q, LinearW8A8AddQ)):
            raise ValueError("GatedMLPW8Q.from_float: the down projection must be a converted LinearW8A8Q or LinearW8A8AddQ, got %s"
                             % type(down).__name__)
        if gate_proj.out_features != up_proj.out_features or gate_proj.in_features != up_proj.in_features or \
                down.in_features != gate_proj.out_features:
            raise ValueError("GatedMLPW8Q.from_float: gate_proj and up_proj must have one shape [C, K] and down must read C features")
        g = LinearW8A8Q.from_float(gate_proj, input_quantizer, gate_quantizer, False, mid_dtype)
        u = LinearW8A8Q.from_float(up_proj, input_quantizer, up_quantizer, False, mid_dtype)
        glu = GLUW8Q.from_float(act, gate_quantizer, hidden_quantizer, act_quantizer, mid_dtype, device=g.weight_levels.device)
        if gate_quantizer is up_quantizer:
            m = cls(glu, down, gate_up=_fuse_linears(g, u))
        else:
            m = cls(glu, down, gate_proj=g, up_proj=u)
        m.train(gate_proj.training)
        return m


_GLU_NEEDED = ("input_quantizer", "gate_quantizer", "up_quantizer", "hidden_quantizer", "down_output_quantizer")
_GLU_KEYS = _GLU_NEEDED + ("act_quantizer", "add_quantizer")


def convert_w8a8_glu(model, mlps, mid_dtype=torch.float32, inplace=False):
    """Replace the gated MLP modules of `model`.  `mlps` maps the qualified name of a module that has `gate_proj`, `up_proj` and
    `down_proj` linear children and an `act_fn` (or `act`) child to a dict of trained per-tensor `LSQFakeQuantizer`s:
    `input_quantizer`, `gate_quantizer`, `up_quantizer` (the same object as `gate_quantizer`: ONE fused gate_up linear),
    `hidden_quantizer` (the product's, the down projection's input), `down_output_quantizer` (the down projection's own output)
    and optionally `act_quantizer` (between the activation and the product) and `add_quantizer` (the quantizer of the block's
    residual add: the down projection becomes a `LinearW8A8AddQ`, and `forward(x, residual)` hands the residual to it).  The
    module becomes a `GatedMLPW8Q`.  Anything else is refused by name.  Returns the model (a deep copy unless inplace=True)."""
    assert mid_dtype in _MID_DTYPES.values(), "mid_dtype must be torch.float32, torch.bfloat16 or torch.float16"
    if not inplace:
        model = copy.deepcopy(model)
    modules = dict(model.named_modules())
    swaps = []
    for name, q in mlps.items():
        child = modules.get(name)
        act = None if child is None else getattr(child, "act_fn", getattr(child, "act", None))
        if child is None or act is None or not all(isinstance(getattr(child, n, None), nn.Linear) for n in ("gate_proj", "up_proj", "down_proj")):
            raise ValueError("convert_w8a8_glu: %r is not a gated MLP with gate_proj, up_proj and down_proj linear children and an "
                             "act_fn (or act) (got %s)" % (name, type(child).__name__))
        if not isinstance(q, dict) or any(k not in _GLU_KEYS for k in q) or any(k not in q for k in _GLU_NEEDED):
            raise ValueError("convert_w8a8_glu: %r needs a dict with input_quantizer, gate_quantizer, up_quantizer, hidden_quantizer and "
                             "down_output_quantizer (optionally act_quantizer, add_quantizer)" % name)
        if q.get("add_quantizer") is not None:
            down = LinearW8A8AddQ.from_float(child.down_proj, q["hidden_quantizer"], q["add_quantizer"], q["down_output_quantizer"],
                                             mid_dtype=mid_dtype)
        else:
            down = LinearW8A8Q.from_float(child.down_proj, q["hidden_quantizer"], q["down_output_quantizer"], False, mid_dtype)
        swaps.append((name, GatedMLPW8Q.from_float(child.gate_proj, child.up_proj, down, act, q["input_quantizer"], q["gate_quantizer"],
                                                   q["up_quantizer"], q["hidden_quantizer"], q.get("act_quantizer"), mid_dtype)))
    for name, new in swaps:
        if name == "":
            return new
        parent_name, _, leaf = name.rpartition(".")
        setattr(modules[parent_name], leaf, new)
    return model
