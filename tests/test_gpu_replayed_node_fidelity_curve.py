"""gpu: ReplayedFidelityCurve(unit="node") -- the node-fidelity curve of a node-attention model as replays of one captured graph -- against
the log oracle on the logits it publishes, against the eager ``explanation_node_fidelity_curve`` on the same batches, its host-side
``kept_node_fraction`` against the stacks' valid words, that a node-curve epoch between training steps changes nothing, its refusals,
that ``unit="edge"`` is the class as it was, and the training example with ``--fidelity-unit node``."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import fidelity_curve_oracle as fco
from tests import node_stack_oracle as nso
from tests import padded_oracle as po
from tests import train_log as tl
from tests.replay import pin_seed_stream
from tests.test_gpu_fidelity_curve_log import P_RTOL
from tests.test_gpu_replayed_fidelity import H, IDS, SLOTS, _dump, _graphs, _gsat, _training_state
from tests.util import TOL, assert_no_memset_nodes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("GIN", dict(ks=[2, 5]), False), ("GIN", dict(ratios=[0.3, 0.7]), True), ("PNA", dict(ratios=[0.3, 0.7]), False),
         ("PNA", dict(ks=[2, 5]), True)]


def _ragged_capacity(graphs):
    nodes, edges = po.sizes(graphs)
    return int(nodes.mean() * 10) + 2, int(edges.mean() * 10)          # room for about ten mean graphs: batches of differing graph counts


@pytest.mark.parametrize("backbone,levels,ragged", CASES, ids=["GIN-ks-fixed", "GIN-ratios-ragged", "PNA-ratios-fixed", "PNA-ks-ragged"])
def test_run_equals_the_log_oracle_and_the_eager_node_curve(dev, backbone, levels, ragged):
    import dp_gsat_amd as G
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat, _ = _gsat(dev, backbone, False, graphs)
    capacity = _ragged_capacity(graphs) if ragged else None
    values = next(iter(levels.values()))
    S, V = len(values), 2 * len(values) + 1
    graph = tl.kept_debug_graph()
    assert graph is not None, "this torch cannot keep a captured hipGraph for debug_dump"
    modes = [m.training for m in gsat.modules()]
    before = {n: t.detach().clone() for n, t in list(gsat.named_parameters()) + list(gsat.named_buffers())}
    rc = G.ReplayedFidelityCurve(gsat, ds, SLOTS, capacity=capacity, ragged=ragged, graph=graph, unit="node", **levels)
    assert [m.training for m in gsat.modules()] == modes and not G.graph_index.sync_free() and gsat.sync_loss_dict
    assert rc.unit == "node" and rc.log.state.tolist() == [0] * 20 and not rc.overflowed()
    assert all(torch.equal(t, before[n]) for n, t in list(gsat.named_parameters()) + list(gsat.named_buffers()))
    text = _dump(graph)
    assert text is not None, "no dump of a kept graph"
    assert assert_no_memset_nodes(text, "ReplayedFidelityCurve(unit='node')")
    names = tl.library_kernels(tl.kernel_nodes(text))
    mine = [n for n in names if "k_stkn_" in n or "k_stk_" in n]
    assert len(mine) == 6 and "k_stk_levels" in mine[0] and "k_stkn_hist" in mine[1] and "k_stkn_fill" in mine[-1], mine          # whatever S is
    assert not any("k_subp_" in n for n in names) and "k_fidc_commit" in names[-1], names[-6:]       # no per-level extraction; the append last

    got = rc.run(np.asarray(IDS))
    again = rc.run(np.asarray(IDS))
    assert got == again                                                                # bitwise repeatable
    if ragged:
        rows = [[int(i) for i in row.tolist() if i >= 0] for row in rc.batches(IDS)]
        replayed = [True] * len(rows)
        assert len({len(r) for r in rows}) > 1 and all(1 <= len(r) <= SLOTS for r in rows), [len(r) for r in rows]
    else:
        rows = [IDS[s:s + SLOTS] for s in range(0, len(IDS), SLOTS)]
        replayed = [len(r) == SLOTS for r in rows]
    assert got["n"] == len(IDS) and rc.log.state.tolist()[:3] == [len(IDS), len(rows), 0] and got["levels"] == values

    cls, p, kept_e, kept_n, edges, nodes, top = [], [], np.zeros(S, np.int64), np.zeros(S, np.int64), 0, 0, 1.0
    eager = {k: np.zeros(S) for k in ("p_keep", "p_drop")}
    for row, is_replay in zip(rows, replayed):
        ub = ds.collate(torch.tensor(row, device=dev))
        if is_replay:
            rc.step(row, 0)
            assert rc.batch.valid.tolist() == [ub.num_nodes, ub.num_edges, len(row), 0]
            logits, stack, node_att = rc.logits.clone(), rc.stack, rc.node_att
            assert stack.graphs_per_variant == SLOTS + 1 and stack.node_capacity == rc.capacity[0]
            assert torch.equal(rc.node_level, stack.node_level) and node_att.shape[0] == rc.capacity[0]
        else:
            gsat.eval()                                                                # the eager tail, through the code run() takes
            node_att, stack, logits = rc._forward(ub, 0)
            gsat.train()
            assert stack.graphs_per_variant == len(row) + 1 and stack.node_capacity == ub.num_nodes + 2
        sv = stack.valid.cpu().numpy()
        N, B = ub.num_nodes, len(row)
        # the published levels are the oracle's levels of the published scores, and the stack's counts follow from them
        level = nso.node_levels_oracle(node_att.reshape(-1)[:N].cpu().numpy(), ub.batch.cpu().numpy(), B, **levels)
        assert np.array_equal(stack.node_level[:N].cpu().numpy(), level)
        ei = ub.edge_index.cpu().numpy()
        assert (sv[:, 3] == 0).all() and (sv[:, 2] == B).all() and sv[0].tolist() == [N, ub.num_edges, B, 0]
        assert (sv[1:1 + S, 0] + sv[1 + S:, 0] == N).all()
        for s in range(S):
            m = level <= s
            assert sv[1 + s, 0] == m.sum() and sv[1 + s, 1] == (m[ei[0]] & m[ei[1]]).sum() and sv[1 + S + s, 1] == (~m[ei[0]] & ~m[ei[1]]).sum()
        c, q = fco.rows(logits.cpu().numpy(), stack.graphs_per_variant, S, B)
        cls.append(c)
        p.append(q)
        kept_e += sv[1:1 + S, 1]
        kept_n += sv[1:1 + S, 0]
        edges, nodes = edges + int(sv[0, 1]), nodes + int(sv[0, 0])
        top = max(top, float(logits.view(V, stack.graphs_per_variant, -1)[:, :B].abs().max()))
        # the eager function on the same batch and the same scores: its own collation, node capacity N + 2
        res = G.explanation_node_fidelity_curve(gsat.clf, ub, node_att.reshape(-1)[:N].contiguous(), **levels)
        assert res["kept_node_fraction"].tolist() == [int(k) / N for k in sv[1:1 + S, 0]]
        assert res["kept_fraction"].tolist() == [int(k) / ub.num_edges for k in sv[1:1 + S, 1]]
        for key in eager:
            eager[key] += res[key].cpu().numpy() * B
    assert gsat.training
    cls, p = np.concatenate(cls), np.concatenate(p)
    want = fco.compute(cls, p, S, kept_e, edges, values)
    for key in fco.EXACT_KEYS:                                                         # integers and their quotients: exact
        assert got[key] == want[key], (key, got[key], want[key])
    assert got["kept_node_fraction"] == [int(k) / nodes for k in kept_n]               # the host's level rule = the sums of stack.valid[:, 0]
    n = len(IDS)
    for key in fco.PROB_KEYS:                                                          # the bound of tests/test_gpu_fidelity_curve_log.py
        a, b = np.atleast_1d(got[key]), np.atleast_1d(want[key])
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 2 * (P_RTOL + n * 2.0 ** -53), (key, got[key], want[key])
    # softmax and sigmoid are 1-Lipschitz in the logits: the forward tolerance carries over to the means of the probabilities
    for key in eager:
        assert np.max(np.abs(np.asarray(got[key]) - eager[key] / n)) <= TOL * top, (key, got[key], eager[key] / n)
    assert not rc.overflowed()
    G.clear_cache()


def test_a_node_curve_epoch_does_not_disturb_training(dev):
    """Three replayed training steps with a replayed node-curve epoch after each, and the same steps without: parameters, BatchNorm
    buffers, Adam state, the device seed state and torch's generator states are bitwise equal, and so are the losses."""
    import dp_gsat_amd as G
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    steps = [IDS[:16], IDS[16:32], IDS[8:24]]
    runs, losses = [], []
    for with_curve in (True, False):
        torch.manual_seed(99)
        torch.cuda.manual_seed(99)
        G.ops.device_seed(dev)              # the seed stream re-bases itself from the CPU generator after a manual_seed: once here in BOTH runs
        gsat, _ = _gsat(dev, "PNA", False, graphs)
        torch.manual_seed(7)
        rs = G.ReplayedStep(gsat, ds, SLOTS)
        rc = G.ReplayedFidelityCurve(gsat, ds, SLOTS, ratios=[0.2, 0.5, 0.8], unit="node") if with_curve else None
        pin_seed_stream(dev, 0x5EED)
        seen = []
        for epoch, ids in enumerate(steps):
            seen.append(rs.step(ids, epoch).clone())
            if rc is not None:
                res = rc.run(np.asarray(IDS))
                assert np.isfinite(res["fidelity_plus"]).all() and res["n"] == len(IDS) and gsat.training
                assert all(a < b for a, b in zip(res["kept_node_fraction"], res["kept_node_fraction"][1:]))
        torch.cuda.synchronize()
        runs.append(_training_state(gsat, dev))
        losses.append(torch.stack([l.reshape(()) for l in seen]))
    (a, seed_a, cuda_a, cpu_a), (b, seed_b, cuda_b, cpu_b) = runs
    assert set(a) == set(b) and any(k.startswith("adam.") for k in a) and any("running_mean" in k for k in a)
    assert seed_a == seed_b and seed_a[1] > 0                              # the training steps drew, the curve epochs did not
    assert torch.equal(cuda_a, cuda_b) and torch.equal(cpu_a, cpu_b) and torch.equal(losses[0], losses[1])
    for key in a:
        assert torch.equal(a[key], b[key]), key
    G.clear_cache()


def test_node_unit_refusals(dev, monkeypatch):
    import dp_gsat_amd as G
    from dp_gsat_amd import explain
    from dp_gsat_amd.encoders import BatchNorm1d
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat, _ = _gsat(dev, "PNA", False, graphs)
    edge_model, _ = _gsat(dev, "GIN", True, graphs)
    modes = [m.training for m in gsat.modules()]

    def refused(match, model=gsat, dataset=ds, unit="node", **kw):
        with pytest.raises(ValueError, match=match):
            G.ReplayedFidelityCurve(model, dataset, SLOTS, unit=unit, **kw)
        assert not G.graph_index.sync_free() and [m.training for m in gsat.modules()] == modes

    refused("node-attention model", model=edge_model, ks=[5])
    refused("unit must be", unit="graph", ks=[5])
    refused("multi-label", model=G.GSAT(gsat.clf, gsat.extractor, G.Criterion(2, True), None, learn_edge_att=False), ks=[5])
    bns = [m for m in gsat.modules() if isinstance(m, BatchNorm1d)]
    bns[0].sync_group = True
    refused("sync_group", ks=[5])
    del bns[0].sync_group
    shared = {"learn_edge_att": False, "extractor_dropout_p": 0.5}
    mcfg = dict(pred_loss_coef=1, info_loss_coef=1, fix_r=False, decay_interval=10, decay_r=0.1, final_r=0.5)
    dual = G.DualGSAT(gsat.clf, G.ExtractorMLP(H, shared, "primal").to(dev), None, gsat.clf, G.ExtractorMLP(H, shared, "dual").to(dev), None,
                      mcfg, mcfg, False, False)
    refused("DualGSAT", model=dual, ks=[5])
    with monkeypatch.context() as mp:                                                  # a dataset whose largest graph the fused ranking cannot take
        mp.setattr(explain, "rank_edges_lds_cap", lambda: int(ds.node_counts.max()) - 1)
        refused("nodes, above rank_edges_lds_cap", ks=[5])
    assert not G.graph_index.sync_free() and gsat.training
    G.clear_cache()


def test_unit_edge_is_the_class_as_it_was(dev):
    """``unit="edge"`` and no keyword: the same kernel nodes in the captured graph, bitwise equal scores and published tensors."""
    import dp_gsat_amd as G
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat, _ = _gsat(dev, "PNA", False, graphs)                                        # a node-attention model: its lifted product is ranked
    out = []
    for kw in (dict(), dict(unit="edge")):
        graph = tl.kept_debug_graph()
        rc = G.ReplayedFidelityCurve(gsat, ds, SLOTS, ratios=[0.3, 0.7], graph=graph, **kw)
        assert rc.unit == "edge"
        res = rc.run(np.asarray(IDS))
        assert "kept_node_fraction" not in res
        rc.step(IDS[:SLOTS], 0)
        out.append((res, tl.library_kernels(tl.kernel_nodes(_dump(graph))), rc.logits.clone(), rc.edge_level.clone(), rc.edge_att.clone(),
                    rc.stack.edge_index.clone(), rc.stack.valid.clone()))
    (res_a, names_a, *ta), (res_b, names_b, *tb) = out
    assert res_a == res_b and names_a == names_b and not any("k_stkn_" in n for n in names_a)
    assert all(torch.equal(x, y) for x, y in zip(ta, tb))
    G.clear_cache()


LINE = re.compile(r"^epoch +(\d+)  train loss (-?[0-9.]+)  test acc ([0-9.]+)  attention ROC-AUC vs motif edges ([0-9.]+)  prec@5 ([0-9.]+)$")
LEVEL = re.compile(r"^      fidelity@([0-9.]+)  kept ([0-9.]+)  kept nodes ([0-9.]+)  fidelity_plus (-?[0-9.]+)  fidelity_minus (-?[0-9.]+)  "
                   r"flip_plus ([0-9.]+)  flip_minus ([0-9.]+)$")


def _example(*extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_ba2motifs.py"), "--graph", "--ragged", "--graphs", "200",
                           "--epochs", "2", "--batch-size", "32", "--hidden", "32", "--fidelity-curve", "0.2,0.5,0.8", "--fidelity-unit", "node",
                           *extra], capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_example_prints_a_node_curve_and_passes_the_refusal_through(dev):
    out = _example("--node-attention")
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 4 and LINE.match(lines[0]), lines
    nodes_before = 0.0
    for line, ratio in zip(lines[1:], (0.2, 0.5, 0.8)):
        m = LEVEL.match(line)
        assert m, line
        level, kept, kept_nodes, plus, minus, flip_plus, flip_minus = (float(v) for v in m.groups())
        assert level == ratio and all(math.isfinite(v) for v in (kept, kept_nodes, plus, minus, flip_plus, flip_minus))
        assert ratio <= kept_nodes + 5e-4 and nodes_before < kept_nodes <= 1.0          # ceil(ratio * N_g) nodes of every graph: increasing
        assert 0.0 <= kept <= 1.0 and -1.0 <= plus <= 1.0 and -1.0 <= minus <= 1.0 and 0.0 <= flip_plus <= 1.0 and 0.0 <= flip_minus <= 1.0
        nodes_before = kept_nodes
    refused = _example()                                                               # an edge-attention model: the class's own refusal
    assert refused.returncode != 0 and "node-attention model" in refused.stderr, refused.stderr[-2000:]
