"""Records tests/golden/ref_* : inputs, weights, random draws and outputs of the REFERENCE'S OWN classes (TEST INFRASTRUCTURE ONLY).

    python -m oracle.record_reference [--out DIR] [--reference DIR]

Run on a CPU machine that holds a checkout of the reference ($GSAT_REFERENCE_DIR, default: ../reference beside this repository).  The reference's modules
(src/models, src/utils, example/gsat.py) are imported UNMODIFIED; the third-party names they need and that are not
installed (torch-geometric, torch-scatter, torch-sparse, ogb) come from the stand-in under oracle/standin/, which is put
on sys.path in this process only and is refused when a real install of one of them exists.  Nothing of the reference is
written out except data its classes read or produce while they run: tensors and case settings.

Every case runs single-threaded, in fp64 and in fp32, from the same fp32 weights and inputs.  The concrete noise and the
extractor's dropout keep-masks are drawn here and handed to the reference by substituting ``Tensor.uniform_``,
``torch.rand_like`` and ``F.dropout`` for the duration of a run; the fixture holds them.  The fp64 run asserts the input rules of the suite:
no min/max ties that a backward could resolve in two ways, 1/sigma of the extractor's InstanceNorm and the margin of its
ReLU (tests/test_gpu_autograd_models.py), and the std aggregator's conditioning weight.  A case whose first seed misses
them takes the next one; the seed used is written to ref_cases.json.

Files per model case: ref_<case>.npz (inputs, ``state.*``, draws, ``f32.*`` / ``f64.*`` outputs) and the parameter
gradients of the two runs, ref_<case>.grad32.npz / ref_<case>.grad64.npz.  ref_operators.npz holds the operator cases and
ref_dual.npz one dual/primal step of src/run_gsat.py (recorded where that module imports over the placeholders).
"""
import argparse
import contextlib
import importlib
import importlib.util
import io
import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STANDIN = os.path.join(HERE, "standin")
DEFAULT_REFERENCE = os.environ.get("GSAT_REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))     # default: a sibling checkout
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden")
THIRD_PARTY = ("torch_geometric", "torch_scatter", "torch_sparse", "ogb")
DRAGGED_IN = ("rdkit", "seaborn", "tensorboard", "torch.utils.tensorboard", "torch.utils.tensorboard.summary")
MAX_FILE_BYTES = 1 << 20

# the conditioning rules of tests/test_gpu_autograd_models.py
MAX_INV_SIGMA = 50.0
RELU_MARGIN_PER_INV_SIGMA = 4e-7
MAX_STD_WEIGHT = 250.0         # its MOLHIV_STD_WEIGHT: molecule-like rows of two near-equal messages cannot do better

ALL_AGGREGATORS = ["sum", "mean", "min", "max", "var", "std"]
ALL_SCALERS = ["identity", "amplification", "attenuation", "linear", "inverse_linear"]


class InputRule(AssertionError):
    """The drawn inputs of a case miss a rule of the suite: the recorder moves on to the next seed."""


# ---------------------------------------------------------------------------------------------------------------------------------
# importing the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def load_reference(reference_dir=DEFAULT_REFERENCE):
    """Namespace of the reference's classes.  Changes sys.path and sys.modules of THIS process: call it in a recording process only."""
    for name in THIRD_PARTY:
        spec = importlib.util.find_spec(name) if name not in sys.modules else sys.modules[name].__spec__
        if spec is not None and not (spec.origin or "").startswith(STANDIN):
            raise RuntimeError(f"{name} is installed ({spec.origin}): record with the real packages, not the stand-in")
    if STANDIN not in sys.path:
        sys.path.insert(0, STANDIN)
    os.environ.setdefault("MPLBACKEND", "Agg")
    placeholder = importlib.import_module("_placeholder")
    for name in DRAGGED_IN:
        placeholder.install(name)
    src = os.path.join(reference_dir, "src")
    if src not in sys.path:
        sys.path.insert(0, src)           # the reference runs from src/: its `datasets`, `models`, `utils` come first
    with contextlib.redirect_stdout(io.StringIO()):
        models = importlib.import_module("models")
        utils = importlib.import_module("utils")
        conv_layers = importlib.import_module("models.conv_layers")
        spec = importlib.util.spec_from_file_location("reference_example_gsat", os.path.join(reference_dir, "example", "gsat.py"))
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
        try:                                  # the dual/primal step: importable only where its plotting and metric imports resolve
            run_gsat = importlib.import_module("run_gsat")
        except ImportError:
            run_gsat = None
    for mod in (models, utils, example):
        assert os.path.abspath(mod.__file__).startswith(os.path.abspath(reference_dir)), mod.__file__
    return NS(GIN=models.GIN, PNA=models.PNA, SPMotifNet=models.SPMotifNet, PNAConvSimple=conv_layers.PNAConvSimple,
              Criterion=utils.Criterion, MLP=utils.MLP, reorder_like=utils.reorder_like, GSAT=example.GSAT,
              ExtractorMLP=example.ExtractorMLP, conv_layers=conv_layers, run_gsat=run_gsat)


# ---------------------------------------------------------------------------------------------------------------------------------
# pre-drawn randomness
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def draws(u=None, masks=(), rand=()):
    """While active, ``Tensor.uniform_`` fills its tensor with ``u`` (a tensor, or a list used in order), every ``F.dropout`` that
    drops (training, p > 0) applies the next keep-mask of ``masks`` scaled by 1 / (1 - p), and ``torch.rand_like`` returns the next
    tensor of ``rand``.  Every draw handed in must be used, and none may be missing."""
    import torch.nn.functional as F
    left = {"u": [] if u is None else (list(u) if isinstance(u, (list, tuple)) else [u]), "masks": list(masks), "rand": list(rand)}
    real_uniform, real_dropout, real_rand_like = torch.Tensor.uniform_, F.dropout, torch.rand_like

    def rand_like(input, **kwargs):
        assert left["rand"], "an undrawn rand_like call"
        return left["rand"].pop(0).to(input.dtype).view(input.shape)

    def uniform_(self, *args, **kwargs):
        assert left["u"], "an undrawn uniform_ call"
        return self.copy_(left["u"].pop(0).to(self.dtype).view(self.shape))

    def dropout(input, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return input
        assert left["masks"], "an undrawn dropout call"
        keep = left["masks"].pop(0).to(input.dtype)
        assert keep.shape == input.shape, (keep.shape, input.shape)
        return input * keep / (1.0 - p)

    torch.Tensor.uniform_, F.dropout, torch.rand_like = uniform_, dropout, rand_like
    try:
        yield
    finally:
        torch.Tensor.uniform_, F.dropout, torch.rand_like = real_uniform, real_dropout, real_rand_like
    assert not left["u"] and not left["masks"] and not left["rand"], "draws left unused"


# ---------------------------------------------------------------------------------------------------------------------------------
# the input rules, observed on the running reference through hooks (nothing of its text is edited)
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def watch_inputs(ref, ext, seen):
    """Records into ``seen``: (1 / sigma, closest non-zero normalised pre-activation) of every InstanceNorm call of ``ext``;
    the std conditioning weight of every PNA layer call; the number of min/max ties of every PNAConvSimple.aggregate."""
    from tests.test_gpu_pna import std_conditioning
    handles = []

    def norm_hook(module, inputs, out):
        x, seg = inputs[0].detach().double(), inputs[1]
        inv = 0.0
        for g in range(int(seg.max()) + 1):
            rows = x[seg == g]
            if rows.shape[0] > 0:
                inv = max(inv, float((rows.var(0, unbiased=False) + module.eps).rsqrt().max()))
        o = out.detach()
        seen["norm"].append((inv, float(o[o != 0].abs().min())))

    if ext is not None:
        for m in ext.modules():
            if type(m).__name__ == "InstanceNorm":
                handles.append(m.register_forward_hook(norm_hook))
    Conv = ref.PNAConvSimple
    real_forward, real_aggregate = Conv.forward, Conv.aggregate

    def forward(self, x, edge_index, edge_attr=None, edge_atten=None):
        w_dx, w_e = std_conditioning(x.detach(), edge_index, None if edge_atten is None else edge_atten.detach(), x.shape[0])
        seen["std"].append(max(float(w_dx.max()), float(w_e.max())))
        self._masked_call, self._width = edge_atten is not None, x.shape[1]
        return real_forward(self, x, edge_index, edge_attr, edge_atten=edge_atten)

    def aggregate(self, inputs, index, dim_size=None):
        # the x_i part of an UNMASKED message is one element of x repeated along its row: every tie rule sends the same sum back to it
        first = 0 if getattr(self, "_masked_call", True) else getattr(self, "_width", 0)
        seen["ties"].append(count_ties(inputs.detach()[:, first:], index, dim_size))
        return real_aggregate(self, inputs, index, dim_size)

    Conv.forward, Conv.aggregate = forward, aggregate
    try:
        yield
    finally:
        Conv.forward, Conv.aggregate = real_forward, real_aggregate
        for h in handles:
            h.remove()


def count_ties(m, index, dim_size):
    """Entries of rows with more than one message that attain their row's minimum or maximum more than once."""
    ties = 0
    for i in range(dim_size):
        rows = m[index == i]
        if rows.shape[0] > 1:
            ties += int(((rows == rows.min(0).values).sum(0) > 1).sum()) + int(((rows == rows.max(0).values).sum(0) > 1).sum())
    return ties


def check_rules(seen, std_used):
    if seen["norm"]:
        inv, margin = max(a for a, _ in seen["norm"]), min(b for _, b in seen["norm"])
        if not (inv <= MAX_INV_SIGMA and margin >= RELU_MARGIN_PER_INV_SIGMA * inv):
            raise InputRule(f"1/sigma {inv:.1f}, closest pre-activation {margin:.2e}")
    if sum(seen["ties"]) != 0:
        raise InputRule(f"{sum(seen['ties'])} min/max ties")
    if std_used and max(seen["std"], default=1.0) > MAX_STD_WEIGHT:
        raise InputRule(f"std weight {max(seen['std']):.1f}")
    return dict(inv_sigma=max((a for a, _ in seen["norm"]), default=0.0), std_weight=max(seen["std"], default=1.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def graphs(rng, num_graphs, n_lo, n_hi, both_directions, isolated=0, extra=0.3):
    """Random trees plus ring-closing edges; ``isolated`` nodes without any edge are appended to the first graphs."""
    src, dst, batch, off = [], [], [], 0
    for g in range(num_graphs):
        n = int(rng.randint(n_lo, n_hi + 1))
        es = {(int(rng.randint(0, v)), v) for v in range(1, n)}
        for _ in range(int(extra * n)):
            a, b = (int(t) for t in rng.randint(0, n, size=2))
            if a != b:
                es.add((min(a, b), max(a, b)))
        for a, b in sorted(es):
            src.append(a + off), dst.append(b + off)
            if both_directions:
                src.append(b + off), dst.append(a + off)
        n += 1 if g < isolated else 0
        batch += [g] * n
        off += n
    ei = torch.tensor([src, dst], dtype=torch.int64)
    ei = ei[:, torch.from_numpy(rng.permutation(ei.shape[1]))].contiguous()          # edge order carries no meaning
    return ei, torch.tensor(batch, dtype=torch.int64), off


def distinct_categorical(rng, dims, groups):
    """One row of categorical features per member; the rows of one group (a list of member ids) are pairwise different."""
    total = sum(len(g) for g in groups)
    out = np.zeros((total, len(dims)), dtype=np.int64)
    for members in groups:
        used = set()
        for m in members:
            while True:
                row = tuple(int(rng.randint(0, d)) for d in dims)
                if row not in used:
                    used.add(row)
                    out[m] = row
                    break
    return torch.from_numpy(out)


CASES = {
    # name: settings.  H and the layer counts are chosen for the dispatch paths of the HIP side, not for a workload
    "gin_edge": dict(backbone="GIN", H=64, n_layers=2, x_dim=5, edge_attr_dim=0, num_class=2, multi_label=False, learn_edge_att=True,
                     both_directions=True, with_eval=True, seed=100),
    "gin_node": dict(backbone="GIN", H=64, n_layers=2, x_dim=5, edge_attr_dim=0, num_class=2, multi_label=False, learn_edge_att=False,
                     both_directions=True, seed=200),
    "gine_directed": dict(backbone="GIN", H=32, n_layers=2, x_dim=4, edge_attr_dim=2, num_class=3, multi_label=False,
                          learn_edge_att=True, both_directions=False, seed=300),
    "pna_node": dict(backbone="PNA", H=64, n_layers=3, x_dim=9, edge_attr_dim=0, num_class=2, multi_label=False, learn_edge_att=False,
                     both_directions=True, atom_encoder=True, aggregators=["mean", "min", "max", "std"], scalers=False, seed=400),
    "pna_scalers_edgeattr": dict(backbone="PNA", H=16, n_layers=2, x_dim=9, edge_attr_dim=3, num_class=2, multi_label=False,
                                 learn_edge_att=True, both_directions=True, atom_encoder=True, isolated=3,
                                 aggregators=["mean", "min", "max", "std"], scalers=True, seed=500),
    "spmotif_leconv": dict(backbone="SPMotifNet", H=32, n_layers=2, x_dim=4, edge_attr_dim=1, num_class=3, multi_label=False,
                           learn_edge_att=True, both_directions=False, seed=600),
    "multilabel": dict(backbone="GIN", H=16, n_layers=2, x_dim=9, edge_attr_dim=3, num_class=12, multi_label=True, learn_edge_att=False,
                       both_directions=True, atom_encoder=True, seed=700),
}
EPOCH = 12
NUM_GRAPHS = 12


def model_config(s, deg):
    cfg = dict(model_name=s["backbone"], n_layers=s["n_layers"], hidden_size=s["H"], dropout_p=0.0, use_edge_attr=True,
               atom_encoder=s.get("atom_encoder", False))
    if s["backbone"] == "PNA":
        cfg.update(aggregators=s["aggregators"], scalers=s["scalers"], deg=deg)
    return cfg


def make_inputs(s, seed):
    from ogb.utils.features import get_atom_feature_dims, get_bond_feature_dims
    rng = np.random.RandomState(seed)
    ei, batch, N = graphs(rng, NUM_GRAPHS, 9, 16, s["both_directions"], isolated=s.get("isolated", 0))
    E = ei.shape[1]
    g = torch.Generator().manual_seed(seed)
    d = dict(edge_index=ei, batch=batch)
    if s.get("atom_encoder"):
        d["x"] = distinct_categorical(rng, get_atom_feature_dims(), [list(range(N))])
    else:
        d["x"] = torch.randn(N, s["x_dim"], generator=g)
    if s["edge_attr_dim"] == 0:
        d["edge_attr"] = None
    elif s.get("atom_encoder"):       # bond features: the in-edges of one node differ, so their embedded messages do
        d["edge_attr"] = distinct_categorical(rng, get_bond_feature_dims(), [(ei[1] == i).nonzero().view(-1).tolist() for i in range(N)])
    elif s["backbone"] == "SPMotifNet":
        d["edge_attr"] = torch.rand(E, 1, generator=g) + 0.5              # LEConv's edge_weight
    else:
        d["edge_attr"] = torch.randn(E, s["edge_attr_dim"], generator=g)
    if s["multi_label"]:
        y = torch.randint(0, 2, (NUM_GRAPHS, s["num_class"]), generator=g).float()
        y[torch.rand(y.shape, generator=g) < 0.25] = float("nan")
    elif s["num_class"] == 2:
        y = torch.randint(0, 2, (NUM_GRAPHS, 1), generator=g).float()
    else:
        y = torch.randint(0, s["num_class"], (NUM_GRAPHS,), generator=g)
    d["y"] = y
    d["deg"] = torch.bincount(torch.bincount(ei[1], minlength=N), minlength=10)
    M = E if s["learn_edge_att"] else N
    C1 = (4 if s["learn_edge_att"] else 2) * s["H"]
    d["u"] = torch.rand(M, 1, generator=g).clamp_(1e-10, 1 - 1e-10)
    d["mask1"] = torch.rand(M, C1, generator=g) > 0.5
    d["mask2"] = torch.rand(M, s["H"], generator=g) > 0.5
    return d


def cast(t, dtype):
    return t.to(dtype) if t is not None and t.is_floating_point() else t


def build_models(ref, s, d, seed):
    """The reference's classifier and extractor with their own initialisation; BatchNorm running statistics as a few training passes
    leave them (fp64, then rounded: one fp32 state for both runs), so that eval mode reads something other than (0, 1)."""
    torch.manual_seed(seed)
    backbone = {"GIN": ref.GIN, "PNA": ref.PNA, "SPMotifNet": ref.SPMotifNet}[s["backbone"]]
    with contextlib.redirect_stdout(io.StringIO()):
        clf = backbone(s["x_dim"], s["edge_attr_dim"], s["num_class"], s["multi_label"], model_config(s, d["deg"]))
        ext = ref.ExtractorMLP(s["H"], s["learn_edge_att"])
        warm = backbone(s["x_dim"], s["edge_attr_dim"], s["num_class"], s["multi_label"], model_config(s, d["deg"]))
        warm.load_state_dict(clf.state_dict())
        warm.double().train()
        with torch.no_grad():
            for _ in range(5):
                warm.get_emb(cast(d["x"], torch.float64), d["edge_index"], batch=d["batch"], edge_attr=cast(d["edge_attr"], torch.float64))
    clf.load_state_dict({k: v.to(clf.state_dict()[k].dtype) for k, v in warm.state_dict().items()})
    return clf, ext


def run_step(ref, s, d, state, dtype, training, check):
    """One forward_pass (and backward) of the reference's GSAT in ``dtype``: (outputs, gradients, what the input rules saw)."""
    torch.manual_seed(0)
    backbone = {"GIN": ref.GIN, "PNA": ref.PNA, "SPMotifNet": ref.SPMotifNet}[s["backbone"]]
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        clf = backbone(s["x_dim"], s["edge_attr_dim"], s["num_class"], s["multi_label"], model_config(s, d["deg"]))
        ext = ref.ExtractorMLP(s["H"], s["learn_edge_att"])
        clf.load_state_dict(state["clf"])
        ext.load_state_dict(state["ext"])
        clf, ext = clf.to(dtype), ext.to(dtype)
        gsat = ref.GSAT(clf, ext, ref.Criterion(s["num_class"], s["multi_label"]), None, learn_edge_att=s["learn_edge_att"])
        gsat.train(training)
        got = {}
        ext.register_forward_pre_hook(lambda m, inputs: got.__setitem__("emb", inputs[0]))
        ext.register_forward_hook(lambda m, inputs, out: got.__setitem__("att_log_logits", out))
        sample = gsat.sampling
        gsat.sampling = lambda logits, train: got.setdefault("att", sample(logits, train))
        data = NS(x=cast(d["x"], dtype), edge_index=d["edge_index"], batch=d["batch"], edge_attr=cast(d["edge_attr"], dtype),
                  y=cast(d["y"], dtype))
        seen = dict(norm=[], std=[], ties=[])
        with watch_inputs(ref, ext, seen) if check else contextlib.nullcontext():
            with draws(d["u"] if training else None, [d["mask1"], d["mask2"]] if training else []):
                edge_att, loss, loss_dict, clf_logits = gsat.forward_pass(data, EPOCH, training)
        grads = {}
        if training:
            loss.backward()
            for prefix, m in (("clf.", clf), ("ext.", ext)):
                grads.update({prefix + k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
    outs = dict(emb=got["emb"], att_log_logits=got["att_log_logits"], att=got["att"], edge_att=edge_att, clf_logits=clf_logits,
                loss=loss.view(1), pred=torch.tensor([loss_dict["pred"]], dtype=torch.float64),
                info=torch.tensor([loss_dict["info"]], dtype=torch.float64))
    return {k: v.detach().clone() for k, v in outs.items()}, grads, seen


def record_case(ref, name, out_dir):
    s = CASES[name]
    for seed in range(s["seed"], s["seed"] + 40):
        d = make_inputs(s, seed)
        clf, ext = build_models(ref, s, d, seed)
        state = dict(clf={k: v.clone() for k, v in clf.state_dict().items()}, ext={k: v.clone() for k, v in ext.state_dict().items()})
        try:
            o64, g64, seen = run_step(ref, s, d, state, torch.float64, True, check=True)
            facts = check_rules(seen, std_used=s["backbone"] == "PNA")
        except InputRule as why:
            print(f"  {name}: seed {seed} misses an input rule ({why})")
            continue
        break
    else:
        raise RuntimeError(f"{name}: no seed meets the input rules")
    o32, g32, _ = run_step(ref, s, d, state, torch.float32, True, check=False)
    arrays = {k: v for k, v in d.items() if v is not None}
    arrays["edge_index"], arrays["batch"] = d["edge_index"].to(torch.int32), d["batch"].to(torch.int32)
    for part in ("clf", "ext"):
        arrays.update({f"state.{part}.{k}": v for k, v in state[part].items()})
    arrays.update({"f32." + k: v for k, v in o32.items()})
    arrays.update({"f64." + k: v for k, v in o64.items()})
    if s.get("with_eval"):
        arrays.update({"f32.eval." + k: v for k, v in run_step(ref, s, d, state, torch.float32, False, check=False)[0].items()})
        arrays.update({"f64.eval." + k: v for k, v in run_step(ref, s, d, state, torch.float64, False, check=False)[0].items()})
    assert set(g32) == set(g64)
    save(os.path.join(out_dir, f"ref_{name}.npz"), arrays)
    save(os.path.join(out_dir, f"ref_{name}.grad32.npz"), g32)
    save(os.path.join(out_dir, f"ref_{name}.grad64.npz"), g64)
    settings = {k: v for k, v in s.items() if k != "seed"}
    settings.update(seed=seed, epoch=EPOCH, num_graphs=NUM_GRAPHS, num_nodes=int(d["x"].shape[0]), num_edges=int(d["edge_index"].shape[1]),
                    undirected=bool(s["both_directions"]), in_degree_0=int((torch.bincount(d["edge_index"][1], minlength=d["x"].shape[0]) == 0).sum()),
                    in_degree_1=int((torch.bincount(d["edge_index"][1], minlength=d["x"].shape[0]) == 1).sum()),
                    state_keys=dict(clf=list(state["clf"]), ext=list(state["ext"])), **facts)
    print(f"  {name}: seed {seed}, N {settings['num_nodes']}, E {settings['num_edges']}, loss {float(o64['loss']):.6f}, {facts}")
    return settings


def save(path, arrays):
    np.savez_compressed(path, **{k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()})
    size = os.path.getsize(path)
    assert size < MAX_FILE_BYTES, f"{path}: {size} bytes"


# ---------------------------------------------------------------------------------------------------------------------------------
# operator cases
# ---------------------------------------------------------------------------------------------------------------------------------
R_EPOCHS = [0, 1, 9, 10, 11, 19, 20, 35, 40, 41, 99, 1000]
R_SETTINGS = [dict(decay_interval=10, decay_r=0.1, final_r=0.7), dict(decay_interval=10, decay_r=0.1, final_r=0.5),
              dict(decay_interval=20, decay_r=0.1, final_r=0.5), dict(decay_interval=3, decay_r=0.25, final_r=0.1, init_r=0.8)]


def record_operators(ref, out_dir):
    out = {}
    rng = np.random.RandomState(11)
    g = torch.Generator().manual_seed(11)
    # PNAConvSimple.aggregate: every aggregator x every scaler, rows of 0, 1 and more messages
    ei, _, N = graphs(rng, 3, 6, 9, both_directions=False, isolated=2)
    index = ei[1]
    deg_hist = torch.bincount(torch.bincount(index, minlength=N), minlength=10)
    F_in = 6
    m32 = torch.randn(index.shape[0], F_in, generator=g)
    cot = torch.randn(N, len(ALL_AGGREGATORS) * len(ALL_SCALERS) * F_in, generator=g)
    assert count_ties(m32, index, N) == 0 and int((torch.bincount(index, minlength=N) == 0).sum()) >= 2
    out.update({"agg.index": index.to(torch.int32), "agg.deg_hist": deg_hist, "agg.messages": m32, "agg.cotangent": cot})
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        with contextlib.redirect_stdout(io.StringIO()):
            conv = ref.PNAConvSimple(F_in, 4, ALL_AGGREGATORS, ALL_SCALERS, deg_hist)
        m = m32.detach().to(dtype, copy=True).requires_grad_(True)
        y = conv.aggregate(m, index, N)
        y.backward(cot.to(dtype))
        out.update({f"agg.{tag}.out": y.detach(), f"agg.{tag}.grad": m.grad})
    out["agg.avg_deg"] = torch.tensor([conv.avg_deg["lin"], conv.avg_deg["log"]], dtype=torch.float64)
    # ExtractorMLP alone, both modes, train and eval
    H = 16
    ei, batch, N = graphs(rng, 6, 8, 12, both_directions=True)
    emb32 = torch.randn(N, H, generator=g)
    out.update({"ext.edge_index": ei.to(torch.int32), "ext.batch": batch.to(torch.int32), "ext.emb": emb32})
    for mode, edge in (("edge", True), ("node", False)):
        torch.manual_seed(5 + edge)
        ext = ref.ExtractorMLP(H, edge)
        state = {k: v.clone() for k, v in ext.state_dict().items()}
        M = ei.shape[1] if edge else N
        masks = [torch.rand(M, (4 if edge else 2) * H, generator=g) > 0.5, torch.rand(M, H, generator=g) > 0.5]
        cot = torch.randn(M, 1, generator=g)
        out.update({f"ext.{mode}.state.{k}": v for k, v in state.items()})
        out.update({f"ext.{mode}.mask1": masks[0], f"ext.{mode}.mask2": masks[1], f"ext.{mode}.cotangent": cot})
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            for training in (True, False):
                ext = ref.ExtractorMLP(H, edge)
                ext.load_state_dict(state)
                ext.to(dtype).train(training)
                emb = emb32.detach().to(dtype, copy=True).requires_grad_(True)
                seen = dict(norm=[], std=[], ties=[])
                with watch_inputs(ref, ext, seen), draws(None, masks if training else []):
                    z = ext(emb, ei, batch)
                if dtype == torch.float64:
                    check_rules(seen, False)
                z.backward(cot.to(dtype))
                t = "train" if training else "eval"
                out[f"ext.{mode}.{tag}.{t}.logits"] = z.detach()
                out[f"ext.{mode}.{tag}.{t}.grad.emb"] = emb.grad
                out.update({f"ext.{mode}.{tag}.{t}.grad.{k}": p.grad for k, p in ext.named_parameters()})
    # Criterion, three modes
    G = 9
    crit_in = {
        "binary": (2, False, torch.randn(G, 1, generator=g) * 2, torch.randint(0, 2, (G, 1), generator=g).float()),
        "multiclass": (3, False, torch.randn(G, 3, generator=g) * 2, torch.randint(0, 3, (G,), generator=g)),
        "multilabel": (12, True, torch.randn(G, 12, generator=g) * 2, torch.randint(0, 2, (G, 12), generator=g).float()),
    }
    crit_in["multilabel"][3][torch.rand(G, 12, generator=g) < 0.3] = float("nan")
    for mode, (num_class, multi_label, logits32, targets) in crit_in.items():
        out.update({f"crit.{mode}.logits": logits32, f"crit.{mode}.targets": targets})
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            with contextlib.redirect_stdout(io.StringIO()):
                crit = ref.Criterion(num_class, multi_label)
            logits = logits32.detach().to(dtype, copy=True).requires_grad_(True)
            loss = crit(logits, cast(targets, dtype))
            loss.backward()
            out.update({f"crit.{mode}.{tag}.loss": loss.detach().view(1), f"crit.{mode}.{tag}.grad": logits.grad})
    # get_r, sampling, lift
    out["r.epochs"] = torch.tensor(R_EPOCHS)
    for i, kw in enumerate(R_SETTINGS):
        out[f"r.{i}"] = torch.tensor([ref.GSAT.get_r(current_epoch=e, **kw) for e in R_EPOCHS], dtype=torch.float64)
    z32 = torch.randn(40, 1, generator=g) * 3
    u = torch.rand(40, 1, generator=g).clamp_(1e-10, 1 - 1e-10)
    u[0], u[1] = 1e-10, 1 - 1e-10            # the ends of the reference's uniform_ range
    out.update({"sample.logits": z32, "sample.u": u.double()})
    lift_ei = torch.from_numpy(rng.randint(0, 40, size=(2, 70)))
    out["lift.edge_index"] = lift_ei.to(torch.int32)
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        with draws(u):
            out[f"sample.{tag}.train"] = ref.GSAT.sampling(z32.to(dtype), True)
        out[f"sample.{tag}.eval"] = ref.GSAT.sampling(z32.to(dtype), False)
        out[f"lift.{tag}"] = ref.GSAT.lift_node_att_to_edge_att(out[f"sample.{tag}.train"], lift_ei)
    save(os.path.join(out_dir, "ref_operators.npz"), out)
    print(f"  operators: {len(out)} arrays")
    return dict(r_settings=R_SETTINGS, aggregators=ALL_AGGREGATORS, scalers=ALL_SCALERS, extractor_hidden=H)


# ---------------------------------------------------------------------------------------------------------------------------------
# the dual/primal step of src/run_gsat.py (node attention on both graphs: the only mode its dual_forward_pass can run)
# ---------------------------------------------------------------------------------------------------------------------------------
DUAL = dict(H=16, n_layers=2, primal_x_dim=5, dual_x_dim=7, num_graphs=6, epoch=52, seed=800,        # epoch > 50: the attention mixing runs
            primal_method=dict(method_name="GSAT", epochs=100, pred_loss_coef=1.0, info_loss_coef=0.5, decay_interval=10, decay_r=0.1,
                               final_r=0.7, init_r=0.9),
            dual_method=dict(method_name="GSAT", epochs=100, pred_loss_coef=0.75, info_loss_coef=1.25, decay_interval=20, decay_r=0.1,
                             final_r=0.5, init_r=0.9),
            shared=dict(learn_edge_att=False, precision_k=5, num_viz_samples=0, viz_interval=1000, viz_norm_att=False, extractor_dropout_p=0.5))


def record_dual(ref, out_dir):
    from tests.graphs import line_graph
    R, s = ref.run_gsat, DUAL
    H = s["H"]
    cfg = dict(model_name="GIN", n_layers=s["n_layers"], hidden_size=H, dropout_p=0.0, use_edge_attr=True)
    for seed in range(s["seed"], s["seed"] + 40):
        rng = np.random.RandomState(seed)
        g = torch.Generator().manual_seed(seed)
        ei, batch, N = graphs(rng, s["num_graphs"], 14, 20, both_directions=True)
        ei = ei[:, torch.argsort(batch[ei[0]], stable=True)].contiguous()          # edges grouped by graph: the dual's batch vector is sorted
        dei, dbatch = line_graph(ei, batch)
        E = ei.shape[1]
        y = torch.randint(0, 2, (s["num_graphs"], 1), generator=g).float()
        d = {"p.x": torch.randn(N, s["primal_x_dim"], generator=g), "p.edge_index": ei, "p.batch": batch, "p.y": y,
             "p.edge_label": (torch.rand(E, generator=g) < 0.3).float(), "d.x": torch.randn(E, s["dual_x_dim"], generator=g),
             "d.edge_index": dei, "d.batch": dbatch, "d.y": y.clone(),
             "p.u": torch.rand(N, 1, generator=g).clamp_(1e-10, 1 - 1e-10), "d.U": torch.rand(E, 1, generator=g),
             "d.u_unused": torch.rand(E, 1, generator=g).clamp_(1e-10, 1 - 1e-10),
             "p.mask1": torch.rand(N, 2 * H, generator=g) > 0.5, "p.mask2": torch.rand(N, H, generator=g) > 0.5,
             "d.mask1": torch.rand(E, 2 * H, generator=g) > 0.5, "d.mask2": torch.rand(E, H, generator=g) > 0.5}
        torch.manual_seed(seed)

        def build():
            with contextlib.redirect_stdout(io.StringIO()):
                return dict(pclf=ref.GIN(s["primal_x_dim"], 0, 2, False, cfg), pext=R.ExtractorMLP(H, s["shared"], "primal"),
                            dclf=ref.GIN(s["dual_x_dim"], 0, 2, False, cfg), dext=R.ExtractorMLP(H, s["shared"], "dual"))
        state = {k: {n: v.clone() for n, v in m.state_dict().items()} for k, m in build().items()}

        def run(dtype, check):
            m = build()
            for k in m:
                m[k].load_state_dict(state[k])
                m[k].to(dtype)
            with contextlib.redirect_stdout(io.StringIO()):
                gsat = R.GSAT(m["pclf"], m["pext"], None, None, None, "cpu", None, "recording", 2, False, 0, s["primal_method"], s["shared"], cfg,
                              m["dclf"], m["dext"], None, None, None, "cpu", None, "recording", 2, False, 0, s["dual_method"], s["shared"], cfg)
                gsat.to(dtype)                   # (its train() is the reference's training loop: the parts are set to training mode one by one)
                for part in m.values():
                    part.train()
                pd = NS(x=d["p.x"].to(dtype), edge_index=ei, batch=batch, edge_attr=None, y=y.to(dtype), edge_label=d["p.edge_label"])
                dd = NS(x=d["d.x"].to(dtype), edge_index=dei, batch=dbatch, edge_attr=None, y=y.to(dtype))
                seen = dict(norm=[], std=[], ties=[])
                with watch_inputs(ref, torch.nn.ModuleList([m["pext"], m["dext"]]), seen) if check else contextlib.nullcontext():
                    with draws([d["p.u"], d["d.u_unused"]], [d["p.mask1"], d["p.mask2"], d["d.mask1"], d["d.mask2"]], [d["d.U"]]):
                        att, loss, ld, logits = gsat.dual_forward_pass(pd, dd, s["epoch"], True)
                loss.backward()
            if check:
                check_rules(seen, False)
            outs = dict(primal_edge_att=att, loss=loss.view(1), clf_logits=logits,
                        **{"dict." + k: torch.tensor([v], dtype=torch.float64) for k, v in ld.items()})
            outs.update({f"grad.{k}.{n}": p.grad for k in m for n, p in m[k].named_parameters() if p.grad is not None})
            return {k: v.detach().clone() for k, v in outs.items()}
        try:
            o64 = run(torch.float64, True)
        except InputRule as why:
            print(f"  dual: seed {seed} misses an input rule ({why})")
            continue
        break
    else:
        raise RuntimeError("dual: no seed meets the input rules")
    o32 = run(torch.float32, False)
    arrays = dict(d)
    for k in ("p.edge_index", "p.batch", "d.edge_index", "d.batch"):
        arrays[k] = d[k].to(torch.int32)
    arrays.update({f"state.{k}.{n}": v for k in state for n, v in state[k].items()})
    arrays.update({"f32." + k: v for k, v in o32.items()})
    arrays.update({"f64." + k: v for k, v in o64.items()})
    save(os.path.join(out_dir, "ref_dual.npz"), arrays)
    print(f"  dual: seed {seed}, N {N}, E {E}, dual edges {dei.shape[1]}, loss {float(o64['loss']):.6f}")
    return dict({k: v for k, v in s.items() if k != "seed"}, seed=seed, num_nodes=N, num_edges=E)


def record_all(out_dir=DEFAULT_OUT, reference_dir=DEFAULT_REFERENCE, cases=None):
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    ref = load_reference(reference_dir)
    os.makedirs(out_dir, exist_ok=True)
    settings = {"cases": {name: record_case(ref, name, out_dir) for name in (cases or CASES)}}
    settings["operators"] = record_operators(ref, out_dir)
    if ref.run_gsat is not None and not cases:
        settings["dual"] = record_dual(ref, out_dir)
    settings["versions"] = dict(standin_for=dict(zip(THIRD_PARTY, ("2.0.3", "2.0.9", "0.6.12", "1.3.2"))))
    with open(os.path.join(out_dir, "ref_cases.json"), "w") as f:
        json.dump(settings, f, indent=1, sort_keys=True)
        f.write("\n")
    return settings


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--reference", default=DEFAULT_REFERENCE)
    ap.add_argument("--case", action="append", help="record only these model cases (default: all)")
    a = ap.parse_args()
    if not os.path.isdir(a.reference):
        sys.exit(f"no reference checkout at {a.reference}")
    record_all(a.out, a.reference, a.case)
