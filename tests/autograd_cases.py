"""The case table of the autograd-boundary contract suite (tests/test_gpu_autograd_contract.py, tests/test_autograd_cases_host.py): one
entry per public wrapper of dp_gsat_amd/ops.py and per dispatch branch the wrapper itself chooses.  An entry holds small seeded inputs
(CPU, fp32), the restatement of the operation in plain torch (oracle/ops.py, oracle/modules.py; evaluated in fp32 and fp64 under
autograd), the list of differentiable inputs, how to call the wrapper on the device, and -- in one phrase each -- the calling patterns
that do not apply to it.  Nothing here touches a GPU at import; ``Case.device`` imports the package when it is called.

References are computed once per (case, set that requires grad, outputs used, number of backward runs) and left unchanged."""
import functools
import itertools
import zlib
from collections import OrderedDict

import numpy as np
import torch

from oracle import bookkeeping as obk
from oracle import modules as om
from oracle import ops as oops
from tests import extractor_cases as xc
from tests import philox_ref
from tests import pna_oracle as po
from tests.graphs import random_batch, shuffle_edges
from tests.util import TOL

PATTERNS = ("baseline", "frozen", "unused", "layouts", "rerun", "partial_full", "stale", "grad_mode")
AGG4 = ["mean", "min", "max", "std"]
BN_EPS, BN_MOMENTUM = 1e-5, 0.1

# case name -> the draw that meets the slack condition of tests/test_autograd_cases_host.py (4 |ref32 - ref64| <= TOL * scale on every tensor
# of every reference of the case), found on the CPU references alone: the first of 0, 1, 2, ... that passes.  Absent: draw 0.
REDRAW = {"pna_none_twopass": 2, "pna_stack3_lifted": 1}


class Case:
    """``inputs``: OrderedDict name -> fp32 CPU tensor, the differentiable inputs (everything else lives in the closures).
    ``oracle(t)`` / ``device(dev, t)``: dict of tensors -> tuple of outputs.  ``groups``: the units the frozen-subset pattern takes its
    subsets over (default: every input on its own).  ``layouts``: input name -> the views it is fed as.  ``na``: pattern -> why not.
    ``env`` / ``own_gemm_flops``: environment and ``ops._OWN_GEMM_FLOPS`` for the device call.  ``other_launch``: inputs whose gradient under
    a frozen subset need NOT be bitwise the baseline's, with the reason (a different launch).  ``weights``: input name -> per-entry
    conditioning weights (>= 1) of its gradient, for the PNA entries: tests/test_gpu_pna.py's std_conditioning, the family's existing cap."""

    def __init__(self, name, inputs, oracle, device, groups=None, layouts=None, na=None, env=None, own_gemm_flops=None, other_launch=None,
                 weights=None):
        self.name, self.inputs, self.oracle, self.device = name, OrderedDict(inputs), oracle, device
        self.weights = dict(weights or {})
        self.diff = list(self.inputs)
        self.groups = [tuple(g) for g in groups] if groups is not None else [(k,) for k in self.diff]
        assert sorted(k for g in self.groups for k in g) == sorted(self.diff)
        self.layouts = dict(layouts or {})
        self.env, self.own_gemm_flops = dict(env or {}), own_gemm_flops
        self.other_launch = dict(other_launch or {})
        self.na = dict(na or {})
        if len(self.groups) < 2:
            self.na.setdefault("frozen", "one differentiable input: no proper subset")
            self.na.setdefault("partial_full", "one differentiable input: a partial backward is the full one")
        if self.n_out < 2:
            self.na.setdefault("unused", "one output")

    @functools.cached_property
    def out_shapes(self):
        with torch.no_grad():
            return [tuple(o.shape) for o in self.oracle({k: v.clone() for k, v in self.inputs.items()})]

    @property
    def n_out(self):
        return len(self.out_shapes)

    def gouts(self, dtype=torch.float32):
        """One dense upstream gradient per output, seeded by the case's name."""
        g = torch.Generator().manual_seed(zlib.crc32(self.name.encode()) & 0x7FFFFFFF)
        return [torch.randn(s, generator=g).to(dtype) for s in self.out_shapes]

    def subsets(self):
        """Every non-empty proper subset of the groups, as frozensets of input names (the set that requires grad)."""
        out = []
        for r in range(1, len(self.groups)):
            for comb in itertools.combinations(self.groups, r):
                out.append(frozenset(k for g in comb for k in g))
        return out

    def used_masks(self):
        """The unused-output pattern: every output alone."""
        n = self.n_out
        return [tuple(i == j for j in range(n)) for i in range(n)] if n > 1 else []


_REFS = {}


def reference(case, dtype, need=None, used=None, times=1):
    """(outputs, {input: gradient or None}) of the oracle in ``dtype``: ``need`` requires grad (default: all), the backward runs through the
    ``used`` outputs (default: all) ``times`` times into the same .grad."""
    need = frozenset(case.diff) if need is None else frozenset(need)
    key = (case.name, dtype, need, used, times)
    if key not in _REFS:
        t = {k: v.to(dtype).clone().requires_grad_(k in need) for k, v in case.inputs.items()}
        outs = case.oracle(t)
        gouts = case.gouts(dtype)
        pick = [i for i in range(len(outs)) if (used is None or used[i]) and outs[i].requires_grad]
        for n in range(times):
            torch.autograd.backward([outs[i] for i in pick], [gouts[i] for i in pick], retain_graph=n + 1 < times)
        _REFS[key] = (tuple(o.detach() for o in outs), {k: t[k].grad for k in case.diff})
    return _REFS[key]


def reference_partial_then_full(case, dtype):
    """torch.autograd.grad on the first group alone (graph retained), then the full backward: the gradients of the full backward."""
    t = {k: v.to(dtype).clone().requires_grad_(True) for k, v in case.inputs.items()}
    outs, gouts = case.oracle(t), case.gouts(dtype)
    torch.autograd.grad(outs, [t[k] for k in case.groups[0]], gouts, retain_graph=True)
    torch.autograd.backward(outs, gouts)
    return {k: t[k].grad for k in case.diff}


def slack_report(case):
    """[(what, 4 |r32 - r64|max, TOL * scale)] over every tensor of every reference the GPU tests compare against."""
    rows = []
    variants = [("baseline", None, None)] + [("frozen " + "+".join(sorted(s)), s, None) for s in case.subsets()] \
        + [("used " + "".join("1" if u else "0" for u in m), None, m) for m in case.used_masks()]
    for label, need, used in variants:
        (o32, g32), (o64, g64) = reference(case, torch.float32, need, used), reference(case, torch.float64, need, used)
        pairs = [(f"out{i}", a, b) for i, (a, b) in enumerate(zip(o32, o64))] + [("d" + k, g32[k], g64[k]) for k in case.diff]
        for what, a, b in pairs:
            assert (a is None) == (b is None)
            if a is None or a.numel() == 0:
                continue
            scale = max(1.0, a.double().abs().max().item())
            w = case.weights.get(what[1:]) if what.startswith("d") else None
            gap = (a.double() - b).abs() if w is None else (a.double() - b).abs() / w.view(a.shape)
            rows.append((f"{case.name} [{label}] {what}", 4.0 * gap.max().item(), TOL * scale))
    return rows


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _draw(name):
    return REDRAW.get(name, 0)


def _gen(name, salt=0):
    return torch.Generator().manual_seed((zlib.crc32(name.encode()) + 7919 * salt + 100003 * _draw(name)) & 0x7FFFFFFF)


@functools.lru_cache(maxsize=None)
def small_batch():
    """12 molecule-like graphs, ~200 nodes, undirected, edges shuffled: (edge_index, batch, N)."""
    ei, batch, N = random_batch(41, 12, 5, 30)
    return shuffle_edges(ei, 3), batch, N


@functools.lru_cache(maxsize=None)
def hub_batch():
    """pna_oracle.hub_graph(): rows of 257, 512, 513 and 1025 in-edges (the chunked branches); one graph."""
    ei, N, _ = po.hub_graph()
    return ei, torch.zeros(N, dtype=torch.int64), N


def _avg_deg(ei, N):
    return oops.pna_avg_deg(torch.from_numpy(obk.deg_histogram(ei, N)))


def _index(dev, ei, batch, N):
    """A fresh BatchIndex whose hub status is known on the host (so that the branch a case names is the branch taken)."""
    from dp_gsat_amd.graph_index import BatchIndex
    ix = BatchIndex(ei.to(dev), N)
    seg = ix.graphs(batch.to(dev))
    ix.long_rows
    return ix, seg


def _pna_weights(xs, ei, N, att=None, na=None):
    """std_conditioning of tests/test_gpu_pna.py per layer input ``xs`` = {name: x}; a node's attention receives the gradient of every
    edge it touches, so its weight is the largest of theirs."""
    from tests.test_gpu_pna import std_conditioning
    w_att = None if na is None else oops.lift_node_att_to_edge_att(na.view(-1, 1), ei)
    if att is not None:
        w_att = att.view(-1, 1)
    out, w_edge = {}, torch.ones(ei.shape[1], dtype=torch.float64)
    for k, x in xs.items():
        out[k], w_e = std_conditioning(x, ei, w_att, N)
        w_edge = torch.maximum(w_edge, w_e)
    if att is not None:
        out["att"] = w_edge.view(-1, 1)
    if na is not None:
        w_n = torch.ones(N, dtype=torch.float64)
        for side in (ei[0], ei[1]):
            w_n.scatter_reduce_(0, side, w_edge, "amax")
        out["na"] = w_n.view(-1, 1)
    return out


X_LAYOUTS = ("colslice", "transposed")
ATT_LAYOUTS = ("flat", "column", "expanded")


# ---- masked sum (GIN / GINE) -----------------------------------------------------------------------------------------------------------
def _sum_case(name, hub, with_att, with_emb, H=16):
    ei, batch, N = hub_batch() if hub else small_batch()
    f = po.float_inputs(ei, N, H, 11 + _draw(name), edge_emb=with_emb)
    inputs = [("x", f.x)]
    if with_att:
        inputs.append(("att", f.att.view(-1, 1)))
    if with_emb:
        inputs.append(("edge_emb", f.emb))

    def oracle(t):
        if with_emb:
            return (oops.gine_aggregate(t["x"], ei, t["edge_emb"], t.get("att"), eps=0.25),)
        return (oops.gin_aggregate(t["x"], ei, t.get("att"), eps=0.25),)

    def device(dev, t):
        from dp_gsat_amd.ops import masked_sum_aggregate
        ix, _ = _index(dev, ei, batch, N)
        assert (ix.long_rows[0] is not None) == hub
        return (masked_sum_aggregate(t["x"], ix, t.get("att"), t.get("edge_emb"), eps=0.25),)

    layouts = {"x": X_LAYOUTS}
    if with_att:
        layouts["att"] = ATT_LAYOUTS
    return Case(name, inputs, oracle, device, layouts=layouts)


# ---- PNA aggregation ---------------------------------------------------------------------------------------------------------------------
def _pna_case(name, H, hub=False, mode="edge", with_emb=False, passthrough=False):
    """mode: "edge" ([E, 1] attention), "none", "node" (LiftedAttention formed inside the kernels: needs H >= 64 and no hub).  With an edge
    embedding the aggregators are mean, min, max, var: std_conditioning knows no embedding part, and the wrapper takes the same branch."""
    aggr = ["mean", "min", "max", "var"] if with_emb else AGG4
    ei, batch, N = hub_batch() if hub else small_batch()
    f = po.float_inputs(ei, N, H, 23 + _draw(name), edge_emb=with_emb)
    avg = _avg_deg(ei, N)
    inputs = [("x", f.x)]
    if mode == "edge":
        inputs.append(("att", f.att.view(-1, 1)))
    if mode == "node":
        inputs.append(("na", f.na.view(-1, 1)))
    if with_emb:
        inputs.append(("edge_emb", f.emb))

    def oracle(t):
        w = t.get("att")
        if mode == "node":
            w = oops.lift_node_att_to_edge_att(t["na"], ei)
        out = oops.pna_aggregate(t["x"], ei, w, aggr, ["identity"], avg, t.get("edge_emb"))
        return (out, t["x"] * 1.0) if passthrough else (out,)

    def device(dev, t):
        from dp_gsat_amd.ops import LiftedAttention, PnaAggregate, pna_aggregate
        ix, _ = _index(dev, ei, batch, N)
        assert (ix.long_rows_nowait[0] is not None) == hub
        tiled = bool(H >= 64 and not hub and not with_emb and ix.pna_tiles(H))
        assert tiled == (H >= 64 and not hub and not with_emb), "the tiled backward does not cover this case"
        w = t.get("att")
        if mode == "node":
            w = LiftedAttention(t["na"], ix)
        out = pna_aggregate(t["x"], ix, w, t.get("edge_emb"), aggr, ["identity"], avg, passthrough=passthrough)
        if mode == "node":
            assert w._edge is None, "the lifted attention was written out: not the in-kernel path"
        return tuple(out) if passthrough else (out,)

    layouts = {"x": X_LAYOUTS}
    if mode == "edge":
        layouts["att"] = ATT_LAYOUTS
    if mode == "node":
        layouts["na"] = ("flat", "column")
    weights = {} if with_emb else _pna_weights({"x": f.x}, ei, N, att=f.att if mode == "edge" else None, na=f.na if mode == "node" else None)
    return Case(name, inputs, oracle, device, layouts=layouts, weights=weights)


def _pna_stack_case(name, conv):
    """Three layers on ONE LiftedAttention + another consumer of node_att (as the info loss is): the shared d node_att buffer."""
    ei, batch, N = small_batch()
    H, Ho, L = (64, 64, 3) if conv else (128, None, 3)
    g = _gen(name)
    avg = {"lin": 1.0, "log": 1.0}
    inputs = [(f"x{i}", torch.randn(N, H, generator=g)) for i in range(L)] + [("na", torch.rand(N, 1, generator=g))]
    if conv:
        inputs += [("W", torch.randn(Ho, 8 * H, generator=g) / (8 * H) ** 0.5), ("b", torch.randn(Ho, generator=g) * 0.1)]

    def oracle(t):
        node_att = t["na"] * 1.0
        w = oops.lift_node_att_to_edge_att(node_att, ei)
        outs = [oops.pna_aggregate(t[f"x{i}"], ei, w, AGG4, ["identity"], avg) for i in range(L)]
        if conv:
            outs = [o @ t["W"].t() + t["b"] for o in outs]
        return tuple(outs) + ((node_att * node_att).sum(),)

    def device(dev, t):
        from dp_gsat_amd.ops import LiftedAttention, pna_aggregate, pna_conv
        ix, _ = _index(dev, ei, batch, N)
        node_att = t["na"] * 1.0                                # a non-leaf, as the sampler's output is
        att = LiftedAttention(node_att, ix)
        if conv:
            outs = [pna_conv(t[f"x{i}"], ix, att, None, AGG4, ["identity"], avg, t["W"], t["b"]) for i in range(L)]
            assert all(o is not None for o in outs), "pna_conv declined the compact path"
        else:
            outs = [pna_aggregate(t[f"x{i}"], ix, att, None, AGG4, ["identity"], avg) for i in range(L)]
        assert att._edge is None and att._shared is not None
        return tuple(outs) + ((node_att * node_att).sum(),)

    groups = [tuple(f"x{i}" for i in range(L)), ("na",)] + ([("W", "b")] if conv else [])
    d = dict(inputs)
    weights = _pna_weights({f"x{i}": d[f"x{i}"] for i in range(L)}, ei, N, na=d["na"])
    return Case(name, inputs, oracle, device, groups=groups, env={"GSAT_PNA_COMPACT": "1"} if conv else None, weights=weights,
                na={"unused": "four outputs of four nodes: no multi-output node to leave half used (the single layers cover it)",
                    "layouts": "covered by the single-layer entries"})


def _pna_conv_case(name, mode, passthrough=False, H=64, Ho=64):
    ei, batch, N = small_batch()
    f = po.float_inputs(ei, N, H, 37 + _draw(name))
    g = _gen(name)
    avg = {"lin": 1.0, "log": 1.0}
    inputs = [("x", f.x)]
    if mode == "edge":
        inputs.append(("att", f.att.view(-1, 1)))
    if mode == "node":
        inputs.append(("na", f.na.view(-1, 1)))
    inputs += [("W", torch.randn(Ho, 8 * H, generator=g) / (8 * H) ** 0.5), ("b", torch.randn(Ho, generator=g) * 0.1)]

    def oracle(t):
        w = t.get("att")
        if mode == "node":
            w = oops.lift_node_att_to_edge_att(t["na"], ei)
        out = oops.pna_aggregate(t["x"], ei, w, AGG4, ["identity"], avg) @ t["W"].t() + t["b"]
        return (out, t["x"] * 1.0) if passthrough else (out,)

    def device(dev, t):
        from dp_gsat_amd.ops import LiftedAttention, pna_conv
        ix, _ = _index(dev, ei, batch, N)
        w = t.get("att")
        if mode == "node":
            w = LiftedAttention(t["na"], ix)
        out = pna_conv(t["x"], ix, w, None, AGG4, ["identity"], avg, t["W"], t["b"], passthrough=passthrough)
        assert out is not None, "pna_conv declined the compact path"
        return tuple(out) if passthrough else (out,)

    layouts = {"x": X_LAYOUTS}
    if mode == "edge":
        layouts["att"] = ATT_LAYOUTS
    weights = _pna_weights({"x": f.x}, ei, N, att=f.att if mode == "edge" else None, na=f.na if mode == "node" else None)
    return Case(name, inputs, oracle, device, layouts=layouts, env={"GSAT_PNA_COMPACT": "1"}, weights=weights)


# ---- extractor ---------------------------------------------------------------------------------------------------------------------------
_EXT_KEYS = ["feature_extractor.%d.%s" % (i, p) for i in (0, 4, 8) for p in ("weight", "bias")]
_PNAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
PHILOX_SEED = 0x5EED1234ABCD


def _extractor_case(name, edge_mode, stream_rows=None, philox=False, H=16):
    c = xc.make_case("regular", "boundaries", edge_mode, H, True, sorted_edges=stream_rows is not None)
    ei, batch, G_, M = c["ei"], c["batch"], c["G"], c["M"]
    _, C1, C2 = xc.widths(edge_mode, H)
    if philox:
        masks = [torch.from_numpy(philox_ref.keep_mask(PHILOX_SEED, k + 1, M, C, xc.P_DROP)) for k, C in enumerate((C1, C2))]
        u = torch.from_numpy(philox_ref.concrete_uniform(PHILOX_SEED, M))
    else:
        masks, u = list(c["masks"]), c["u"]
    inputs = [("emb", c["emb"])] + list(zip(_PNAMES, c["params"]))

    def oracle(t):
        W = [(t["W1"], t["b1"]), (t["W2"], t["b2"]), (t["W3"], t["b3"])]
        dt = t["emb"].dtype
        z = oops.extractor_forward(t["emb"], ei, batch, G_, W, edge_mode, xc.P_DROP, [m.to(dt) for m in masks], True)
        return z, oops.concrete_sample(z, u.to(dt).view(-1, 1), True)

    def device(dev, t):
        import dp_gsat_amd as G
        ext = G.ExtractorMLP(H, edge_mode, stream_rows=stream_rows).to(dev).train()

        class Attend(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.ext = ext

            def forward(self, emb):
                if philox:
                    return self.ext.attend(emb, ei_d, batch_d, noise="philox", seed=PHILOX_SEED)
                return self.ext.attend(emb, ei_d, batch_d, noise=u.to(dev), dropout_masks=[m.to(dev) for m in masks])

        ei_d, batch_d = ei.to(dev), batch.to(dev)
        params = {"ext." + k: t[n] for k, n in zip(_EXT_KEYS, _PNAMES)}
        return tuple(torch.func.functional_call(Attend(), params, (t["emb"],)))

    return Case(name, inputs, oracle, device, groups=[("emb",), _PNAMES], layouts={"emb": X_LAYOUTS, "W2": ("transposed",)})


# ---- samplers, lift, symmetrise, losses --------------------------------------------------------------------------------------------------
def _sampler_case(name, kind):
    M = 301
    g = _gen(name)
    z = torch.randn(M, 1, generator=g) * 2
    u = torch.rand(M, 1, generator=g).clamp_(1e-4, 1 - 1e-4)
    seed = 0x1234F00D
    if kind == "gumbel_seed":
        u = torch.from_numpy(philox_ref.gumbel_uniform(seed, M)).view(M, 1)

    def oracle(t):
        dt = t["logits"].dtype
        if kind == "concrete_train":
            return (oops.concrete_sample(t["logits"], u.to(dt), True, temp=0.7),)
        if kind == "concrete_eval":
            return (oops.concrete_sample(t["logits"], None, False),)
        return (oops.gumbel_sigmoid(t["logits"], u.to(dt), tau=0.6),)

    def device(dev, t):
        from dp_gsat_amd.gsat import concrete_sample, gumbel_sigmoid
        if kind == "concrete_train":
            return (concrete_sample(t["logits"], temp=0.7, training=True, noise=u.to(dev)),)
        if kind == "concrete_eval":
            return (concrete_sample(t["logits"], training=False),)
        if kind == "gumbel_noise":
            return (gumbel_sigmoid(t["logits"], tau=0.6, noise=u.to(dev)),)
        return (gumbel_sigmoid(t["logits"], tau=0.6, seed=seed),)

    return Case(name, [("logits", z)], oracle, device, layouts={"logits": ("flat", "column", "expanded")})


def _lift_case(name):
    ei, batch, N = small_batch()
    na = torch.rand(N, 1, generator=_gen(name))

    def oracle(t):
        return (oops.lift_node_att_to_edge_att(t["na"], ei),)

    def device(dev, t):
        from dp_gsat_amd.ops import LiftedAttention
        ix, _ = _index(dev, ei, batch, N)
        return (LiftedAttention(t["na"], ix).edge(),)

    return Case(name, [("na", na)], oracle, device, layouts={"na": ("flat", "column")})


def _symmetrise_case(name, device_flag):
    ei, batch, N = small_batch()
    assert obk.is_undirected(ei, N)
    rev = torch.from_numpy(np.asarray(obk.reverse_edge_perm(ei, N))).long()
    att = torch.rand(ei.shape[1], 1, generator=_gen(name))

    def oracle(t):
        return (oops.symmetrise(t["att"], rev),)

    def device(dev, t):
        from dp_gsat_amd.gsat import symmetrise_edge_att
        from dp_gsat_amd.graph_index import get_index
        from dp_gsat_amd.ops import Symmetrise
        ei_d = ei.to(dev)
        if device_flag:                                         # what symmetrise_edge_att does in sync-free mode
            return (Symmetrise.apply(t["att"], *get_index(ei_d, N).rev_and_flag),)
        return (symmetrise_edge_att(t["att"], ei_d, N),)

    return Case(name, [("att", att)], oracle, device, layouts={"att": ("expanded",)})


def _info_case(name, tensor_prior):
    M = 777
    g = _gen(name)
    att = torch.rand(M, 1, generator=g) * 0.9 + 0.05
    r = (torch.rand(M, 1, generator=g) * 0.5 + 0.3) if tensor_prior else 0.7

    def oracle(t):
        return (oops.info_loss(t["att"], r.to(t["att"].dtype) if tensor_prior else r),)

    def device(dev, t):
        from dp_gsat_amd.gsat import info_loss
        return (info_loss(t["att"], r.to(dev) if tensor_prior else r),)

    return Case(name, [("att", att)], oracle, device, layouts={"att": ("flat", "column", "expanded")})


def _f1_case(name, count):
    M = 777
    g = _gen(name)
    p = torch.rand(M, generator=g)
    y = (torch.rand(M, generator=g) > 0.6).float()
    m = M if count is None else count

    def oracle(t):
        pp = t["p"]
        loss = om.f1_sparsity_loss(pp[:m], y.to(pp.dtype)[:m])
        return (loss + 0.0 * pp.sum(),)                            # entries beyond the count: a zero gradient, not None

    def device(dev, t):
        from dp_gsat_amd.dual_gsat import f1_sparsity_loss_valid
        mv = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
        return (f1_sparsity_loss_valid(t["p"], y.to(dev), mv),)

    return Case(name, [("p", p)], oracle, device, layouts={"p": ("expanded",)})


def _criterion_case(name, mode):
    G_ = 37
    g = _gen(name)
    if mode == "bce":
        z, y, nc, ml = torch.randn(G_, 1, generator=g), (torch.rand(G_, 1, generator=g) > 0.5).float(), 2, False
    elif mode == "ce":
        z, y, nc, ml = torch.randn(G_, 5, generator=g), torch.randint(0, 5, (G_,), generator=g).float(), 5, False
    else:
        z, y, nc, ml = torch.randn(G_, 6, generator=g), (torch.rand(G_, 6, generator=g) > 0.5).float(), 6, True
        y[torch.rand(G_, 6, generator=g) < 0.2] = float("nan")

    def oracle(t):
        # oracle.modules.Criterion.forward, minus its targets.float() (which would pin the fp64 evaluation to fp32 targets)
        zz = t["logits"]
        F = torch.nn.functional
        if mode == "bce":
            loss = F.binary_cross_entropy_with_logits(zz, y.to(zz.dtype))
        elif mode == "ce":
            loss = F.cross_entropy(zz, y.long())
        else:
            is_labeled = y == y
            loss = F.binary_cross_entropy_with_logits(zz[is_labeled], y[is_labeled].to(zz.dtype))
        return (loss + 0.0 * zz.sum(),)                            # unlabelled entries: a zero gradient, not None

    def device(dev, t):
        from dp_gsat_amd.get_model import Criterion
        return (Criterion(nc, ml, capturable=True)(t["logits"], y.to(dev)),)

    return Case(name, [("logits", z)], oracle, device, layouts={"logits": ("transposed",) if z.shape[1] > 1 else ()})


# ---- normalisation, encoders, tails, linear, pooling ------------------------------------------------------------------------------------
def _instance_norm_case(name, C=16):
    sizes = [4, 5, 32, 33, 64, 12, 40, 7]
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    x = torch.randn(batch.numel(), C, generator=_gen(name))

    def oracle(t):
        return (oops.instance_norm(t["x"], batch, len(sizes)),)

    def device(dev, t):
        from dp_gsat_amd.get_model import InstanceNorm
        return (InstanceNorm(C)(t["x"], batch.to(dev)),)

    return Case(name, [("x", x)], oracle, device, layouts={"x": X_LAYOUTS})


EMB_DIMS = (7, 5, 3, 11)                                            # 26 rows: the padded one-hot width (28) differs from the table's


def embedding_idx(N=300):
    g = torch.Generator().manual_seed(77)
    return torch.stack([torch.randint(0, d, (N,), generator=g) for d in EMB_DIMS], dim=1)


def _embedding_case(name, H=16):
    x_idx = embedding_idx()
    W = torch.randn(sum(EMB_DIMS), H, generator=_gen(name))
    offs = torch.tensor([0] + list(np.cumsum(EMB_DIMS)[:-1]))

    def oracle(t):
        return (t["W"][x_idx + offs].sum(dim=1),)

    def device(dev, t):
        from dp_gsat_amd.ops import EmbeddingSum
        return (EmbeddingSum.apply(x_idx.to(dev), t["W"], list(EMB_DIMS), {}),)

    return Case(name, [("W", W)], oracle, device, layouts={"W": X_LAYOUTS})


BN_SEED = 0xB47C4
BN_P = 0.25


def _bn_case(name, training, relu, residual=False, dropout=False, N=300, C=16):
    g = _gen(name)
    x = torch.randn(N, C, generator=g) * 1.5 + 0.3
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    inputs = [("x", x), ("weight", w), ("bias", b)]
    if residual:
        inputs.append(("residual", torch.randn(N, C, generator=g)))
    p = BN_P if dropout else 0.0
    keep = torch.from_numpy(philox_ref.keep_mask(BN_SEED, 3, N, C, p)) if dropout else None

    def oracle(t):
        xx = t["x"]
        dt = xx.dtype
        if training:
            mean, var = xx.mean(dim=0), xx.var(dim=0, unbiased=False)
        else:
            mean, var = rm.to(dt), rv.to(dt)
        y = (xx - mean) / torch.sqrt(var + BN_EPS) * t["weight"] + t["bias"]
        if relu:
            y = torch.relu(y)
        if residual:
            y = y + t["residual"]
        if dropout:
            y = y * keep.to(dt) / (1.0 - p)
        return (y,)

    def device(dev, t):
        from dp_gsat_amd.ops import BatchNormFn
        return (BatchNormFn.apply(t["x"], t["weight"], t["bias"], rm.to(dev), rv.to(dev), training, BN_MOMENTUM, BN_EPS, relu,
                                  t.get("residual"), p, BN_SEED, None, None),)

    layouts = {"x": X_LAYOUTS}
    if residual:
        layouts["residual"] = X_LAYOUTS
    return Case(name, inputs, oracle, device, layouts=layouts)


RD_SEED = 0xD20F


def _relu_dropout_case(name, p, N=300, C=16):
    x = torch.randn(N, C, generator=_gen(name))
    keep = torch.from_numpy(philox_ref.keep_mask(RD_SEED, 5, N, C, p)) if p > 0 else None

    def oracle(t):
        y = torch.relu(t["x"])
        return (y * keep.to(y.dtype) / (1.0 - p) if p > 0 else y,)

    def device(dev, t):
        from dp_gsat_amd.ops import ReluDropout, relu_dropout
        if p > 0:
            return (ReluDropout.apply(t["x"], p, RD_SEED, None),)      # what relu_dropout calls, under a seed the reference can restate
        return (relu_dropout(t["x"], 0.5, False),)

    return Case(name, [("x", x)], oracle, device, layouts={"x": X_LAYOUTS})


def _linear_case(name, K, own, bias=True, M=300, N_out=32):
    g = _gen(name)
    inputs = [("x", torch.randn(M, K, generator=g)), ("weight", torch.randn(N_out, K, generator=g) / K ** 0.5)]
    if bias:
        inputs.append(("bias", torch.randn(N_out, generator=g) * 0.1))

    def oracle(t):
        return (torch.nn.functional.linear(t["x"], t["weight"], t.get("bias")),)

    def device(dev, t):
        from dp_gsat_amd.ops import linear
        return (linear(t["x"], t["weight"], t.get("bias")),)

    return Case(name, inputs, oracle, device, layouts={"x": X_LAYOUTS, "weight": ("transposed",)}, own_gemm_flops=0.0 if own else None)


def _pool_case(name, mean, H=16):
    ei, batch, N = small_batch()
    x = torch.randn(N, H, generator=_gen(name))
    G_ = int(batch.max()) + 1

    def oracle(t):
        return ((oops.global_mean_pool if mean else oops.global_add_pool)(t["x"], batch, G_),)

    def device(dev, t):
        from dp_gsat_amd.ops import segment_pool
        _, seg = _index(dev, ei, batch, N)
        return (segment_pool(t["x"], seg, mean),)

    return Case(name, [("x", x)], oracle, device, layouts={"x": X_LAYOUTS})


BUILDERS = OrderedDict([
    ("sum_plain", lambda n: _sum_case(n, False, False, False)),
    ("sum_att", lambda n: _sum_case(n, False, True, False)),
    ("sum_emb", lambda n: _sum_case(n, False, False, True)),
    ("sum_att_emb", lambda n: _sum_case(n, False, True, True)),
    ("sum_att_hub", lambda n: _sum_case(n, True, True, False)),
    ("sum_att_emb_hub", lambda n: _sum_case(n, True, True, True)),
    ("pna_none_twopass", lambda n: _pna_case(n, 16, mode="none")),
    ("pna_edge_twopass", lambda n: _pna_case(n, 16)),
    ("pna_edge_emb_twopass", lambda n: _pna_case(n, 16, with_emb=True)),
    ("pna_edge_tiled", lambda n: _pna_case(n, 128)),
    ("pna_edge_hub", lambda n: _pna_case(n, 16, hub=True)),
    ("pna_node_lifted", lambda n: _pna_case(n, 128, mode="node")),
    ("pna_edge_twopass_passthrough", lambda n: _pna_case(n, 16, passthrough=True)),
    ("pna_edge_tiled_passthrough", lambda n: _pna_case(n, 128, passthrough=True)),
    ("pna_node_lifted_passthrough", lambda n: _pna_case(n, 128, mode="node", passthrough=True)),
    ("pna_stack3_lifted", lambda n: _pna_stack_case(n, conv=False)),
    ("pna_conv_none", lambda n: _pna_conv_case(n, "none")),
    ("pna_conv_edge", lambda n: _pna_conv_case(n, "edge")),
    ("pna_conv_node", lambda n: _pna_conv_case(n, "node")),
    ("pna_conv_edge_passthrough", lambda n: _pna_conv_case(n, "edge", passthrough=True)),
    ("pna_conv_node_passthrough", lambda n: _pna_conv_case(n, "node", passthrough=True)),
    ("pna_conv_stack3_lifted", lambda n: _pna_stack_case(n, conv=True)),
    ("extractor_node", lambda n: _extractor_case(n, False)),
    ("extractor_edge", lambda n: _extractor_case(n, True)),
    ("extractor_edge_streamed", lambda n: _extractor_case(n, True, stream_rows=96)),
    ("extractor_node_philox", lambda n: _extractor_case(n, False, philox=True)),
    ("extractor_edge_philox", lambda n: _extractor_case(n, True, philox=True)),
    ("concrete_sample_train", lambda n: _sampler_case(n, "concrete_train")),
    ("concrete_sample_eval", lambda n: _sampler_case(n, "concrete_eval")),
    ("gumbel_sigmoid_noise", lambda n: _sampler_case(n, "gumbel_noise")),
    ("gumbel_sigmoid_seed", lambda n: _sampler_case(n, "gumbel_seed")),
    ("lift", _lift_case),
    ("symmetrise_host_flag", lambda n: _symmetrise_case(n, False)),
    ("symmetrise_device_flag", lambda n: _symmetrise_case(n, True)),
    ("info_loss_scalar_prior", lambda n: _info_case(n, False)),
    ("info_loss_tensor_prior", lambda n: _info_case(n, True)),
    ("f1_sparsity_all", lambda n: _f1_case(n, None)),
    ("f1_sparsity_count", lambda n: _f1_case(n, 700)),
    ("criterion_bce", lambda n: _criterion_case(n, "bce")),
    ("criterion_ce", lambda n: _criterion_case(n, "ce")),
    ("criterion_multilabel", lambda n: _criterion_case(n, "ml")),
    ("instance_norm", _instance_norm_case),
    ("embedding_sum", _embedding_case),
    ("bn_train", lambda n: _bn_case(n, True, False)),
    ("bn_train_relu", lambda n: _bn_case(n, True, True)),
    ("bn_eval", lambda n: _bn_case(n, False, False)),
    ("bn_eval_relu", lambda n: _bn_case(n, False, True)),
    ("bn_train_relu_residual", lambda n: _bn_case(n, True, True, residual=True)),
    ("bn_train_relu_residual_dropout", lambda n: _bn_case(n, True, True, residual=True, dropout=True)),
    ("bn_eval_relu_residual", lambda n: _bn_case(n, False, True, residual=True)),
    ("relu_dropout_eval", lambda n: _relu_dropout_case(n, 0.0)),
    ("relu_dropout_seeded", lambda n: _relu_dropout_case(n, 0.3)),
    ("linear_library", lambda n: _linear_case(n, 64, own=False)),
    ("linear_own_gemm", lambda n: _linear_case(n, 64, own=True)),
    ("linear_own_gemm_nobias", lambda n: _linear_case(n, 64, own=True, bias=False)),
    ("linear_padded_columns", lambda n: _linear_case(n, 10, own=False)),
    ("segment_pool_sum", lambda n: _pool_case(n, False)),
    ("segment_pool_mean", lambda n: _pool_case(n, True)),
])
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def get(name):
    return BUILDERS[name](name)


def pattern_cases():
    """[(pattern, case name, detail)] -- every pattern case the GPU suite runs; ``detail`` names the subset / the outputs used."""
    out = []
    for name in NAMES:
        c = get(name)
        for p in PATTERNS:
            if p in c.na:
                continue
            if p == "frozen":
                out += [(p, name, "+".join(sorted(s))) for s in c.subsets()]
            elif p == "unused":
                out += [(p, name, "".join("1" if u else "0" for u in m)) for m in c.used_masks()]
            else:
                out.append((p, name, ""))
    return out


def not_applicable():
    return [(name, p, get(name).na[p]) for name in NAMES for p in PATTERNS if p in get(name).na]
