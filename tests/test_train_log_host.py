"""not gpu: the host side of the training-pass log -- constructor arguments are refused before anything touches a device, the step
bodies append what they should to the logs they should (the library call is replaced, as in tests/test_eval_log_host.py the oracle
stands in for it), epoch_scores() merges the dual scores, and the dot reader of tests/train_log.py."""
import inspect

import pytest
import torch

from tests import train_log as tl


def test_constructor_arguments_are_refused_before_anything_else():
    import dp_gsat_amd as G
    for kw, match in ((dict(log_k=0), "log_k"), (dict(log_k=-1), "log_k"), (dict(log_k=True), "log_k"), (dict(log_k=1.5), "log_k"),
                      (dict(log_k=5, bins=0), "bins"), (dict(log_k=5, bins=10 ** 6), "bins")):
        with pytest.raises(ValueError, match=match):          # no model, no dataset: nothing else was looked at
            G.ReplayedStep(None, None, 4, **kw)
        with pytest.raises(ValueError, match=match):
            G.ReplayedDualStep(None, None, None, 4, **kw)
    with pytest.raises(ValueError, match="score_dual"):
        G.ReplayedDualStep(None, None, None, 4, score_dual=True)
    for cls, extra in ((G.ReplayedStep, ()), (G.ReplayedDualStep, ("score_dual",))):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["log_k"].default is None and sig["bins"].default == 64
        assert sig["max_graphs"].default is None and sig["max_edges"].default is None
        assert all(sig[name].default is False for name in extra)
        assert callable(cls.begin_epoch) and callable(cls.epoch_scores)


class _FakeLog:
    k = 5

    def __init__(self, scores=None):
        self.appended, self.resets, self.scores = [], 0, scores

    def append(self, att, data, logits, losses):
        self.appended.append((att, data, logits, losses))

    def reset(self):
        self.resets += 1

    def compute(self):
        return dict(self.scores)


def _bare(cls, **attrs):
    obj = object.__new__(cls)
    for key, v in attrs.items():
        setattr(obj, key, v)
    return obj


@pytest.mark.parametrize("with_dual", [False, True])
def test_append_training_makes_the_logs_once_and_appends_detached_outputs(monkeypatch, with_dual):
    from dp_gsat_amd import replay
    import dp_gsat_amd as G
    made = []

    def new_logs(ev, count, logits, k, bins, max_graphs, max_edges):
        made.append((count, tuple(logits.shape), k, bins, max_graphs, max_edges))
        return [_FakeLog() for _ in range(count)]

    monkeypatch.setattr(replay, "_new_logs", new_logs)
    rs = _bare(G.ReplayedStep, log=None, dual_log=None, _log_sizes=(5, 32, 10, None))
    w = torch.ones(3, 1, requires_grad=True)
    att, logits = w * 0.5, w[:2] * 2.0
    dual_att = torch.full((3, 1), 0.25) if with_dual else None
    ld = {"loss": torch.tensor(3.0), "pred": torch.tensor(1.0, dtype=torch.float64), "info": torch.tensor(2.0)}
    batch = object()
    for _ in range(2):
        losses = replay._append_training(rs, att, dual_att, batch, logits, ld)
    assert made == [(2 if with_dual else 1, (2, 1), 5, 32, 10, None)], "the logs are made by the first call alone"
    assert losses.dtype == torch.float32 and losses.tolist() == [3.0, 1.0, 2.0]
    assert len(rs.log.appended) == 2 and (rs.dual_log is None) == (not with_dual)
    a, b, z, l = rs.log.appended[-1]
    assert b is batch and not a.requires_grad and not z.requires_grad and torch.equal(a, att.detach()) and torch.equal(z, logits.detach())
    assert torch.equal(l, losses)
    if with_dual:
        a, b, z, l = rs.dual_log.appended[-1]
        assert a is dual_att and b is batch and torch.equal(z, logits.detach()) and torch.equal(l, losses)


def test_begin_epoch_and_epoch_scores():
    import dp_gsat_amd as G
    primal = {"att_auroc": 0.75, "precision@5": 0.5, "delta_kl": 1.0, "avg_signal_att_weights": 0.8, "avg_bkg_att_weights": 0.3,
              "clf_acc": 0.9, "clf_roc": 0.95, "loss": 1.5, "pred": 0.5, "info": 1.0}
    dual = dict(primal, att_auroc=0.25, delta_kl=2.0, clf_acc=-1.0, loss=-1.0)
    rs = _bare(G.ReplayedDualStep, log=_FakeLog(primal), dual_log=_FakeLog(dual))
    rs.begin_epoch()
    assert rs.log.resets == 1 and rs.dual_log.resets == 1
    got = rs.epoch_scores()
    assert {k: v for k, v in got.items() if not k.startswith("dual_")} == primal
    assert {k for k in got if k.startswith("dual_")} == {"dual_att_auroc", "dual_precision@5", "dual_delta_kl", "dual_avg_signal_att_weights",
                                                         "dual_avg_bkg_att_weights"}, "only the attention scores of the second log"
    assert got["dual_att_auroc"] == 0.25 and got["dual_delta_kl"] == 2.0
    single = _bare(G.ReplayedStep, log=_FakeLog(primal), dual_log=None)
    assert single.epoch_scores() == primal
    for cls in (G.ReplayedStep, G.ReplayedDualStep):
        none = _bare(cls, log=None, dual_log=None)
        none.begin_epoch()                                    # nothing to empty
        with pytest.raises(ValueError, match="without log_k"):
            none.epoch_scores()


DOT = r'''digraph dot {
"graph_0_node_0"[style="bold"shape="record"label="{
KERNEL
| {ID | 0 | _ZN4gsat13k_ragged_scanEPKliS1_S1_lPlS2_S2_S2_Ph\<\<\<(1,1,1),(256,1,1),(0,0,0),0\>\>\>}
| {cooperative | 0}
}"];
"graph_0_node_1"[style="solid"shape="record"label="{
MEMCPY
| {{ID | node handle} | {1 | 0x7bd74c0105b0}}
| {kind | DtoD}
}"];
"graph_0_node_2"[style="bold"shape="record"label="{
KERNEL
| {ID | 2 | _ZN2at6native29vectorized_elementwise_kernelILi4ENS0_11FillFunctorIfEESt5arrayIPcLm1EEEEviT0_T1_\<\<\<(1,1,1),(256,1,1),(0,0,0),0\>\>\>}
}"];
"graph_0_node_0" -> "graph_0_node_1";
}'''


def test_kernel_nodes_reads_a_dump_in_node_order(tmp_path):
    assert tl.kernel_nodes(None) is None and tl.kernel_nodes("digraph { }") is None
    names = tl.kernel_nodes(DOT)
    assert names == ["_ZN4gsat13k_ragged_scanEPKliS1_S1_lPlS2_S2_S2_Ph",
                     "_ZN2at6native29vectorized_elementwise_kernelILi4ENS0_11FillFunctorIfEESt5arrayIPcLm1EEEEviT0_T1_"]
    assert tl.library_kernels(names) == names[:1]
    path = tmp_path / "kernels.txt"
    path.write_text("# torch 9.9.9+x\n# a comment\n" + "\n".join(names) + "\n")
    assert tl.read_kernel_list(str(path)) == ("9.9.9+x", names)


def test_recorded_kernel_lists_are_whole():
    """The lists of tests/golden/ the GPU test compares with: a version line, the library's collation first, its criterion, no append."""
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for backbone in ("GIN", "PNA"):
        version, names = tl.read_kernel_list(os.path.join(golden, f"replayed_step_kernels_{backbone}.txt"))
        lib = tl.library_kernels(names)
        assert version and len(names) > len(lib) > 50
        assert "k_ragged_scan" in names[0] and any("k_crit_" in n for n in lib) and not any("k_log_" in n for n in lib)
