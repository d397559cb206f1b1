"""host: the components oracle (tests/components_oracle.py) against scipy and against hand-written answers, and the argument checks of
dp_gsat_amd.level_components and its relatives that need no device."""
import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from tests import components_oracle as co


def _random_batch(rng, G, max_nodes, S):
    sizes = rng.randint(0, max_nodes + 1, size=G)
    batch = np.repeat(np.arange(G), sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    src, dst = [], []
    for g in range(G):
        n = sizes[g]
        if n == 0:
            continue
        m = rng.randint(0, 2 * n + 1)
        src.append(starts[g] + rng.randint(0, n, size=m))
        dst.append(starts[g] + rng.randint(0, n, size=m))                 # self-loops, duplicates and one-directional edges occur
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]) if src else np.zeros((2, 0), np.int64)
    perm = rng.permutation(ei.shape[1])                                   # edges are not stored graph by graph
    ei = ei[:, perm].astype(np.int64)
    level = rng.randint(0, S + 1, size=ei.shape[1]).astype(np.uint8)
    return ei, batch, level


def _scipy_rows(ei, batch, G, level, S):
    """[G, S, 5] from scipy: components among the touched nodes, kept, big_edges, touched, big_nodes, graph by graph and level by level."""
    out = np.zeros((G, S, 5), np.int32)
    N = len(batch)
    eg = batch[ei[0]] if ei.shape[1] else np.zeros(0, np.int64)
    for g in range(G):
        for s in range(S):
            keep = (eg == g) & (level <= s)
            u, v = ei[0, keep], ei[1, keep]
            touched = np.unique(np.concatenate([u, v]))
            if len(touched) == 0:
                continue
            _, lab = connected_components(coo_matrix((np.ones(len(u)), (u, v)), shape=(N, N)), directed=False)
            comp_of = lab[touched]
            out[g, s] = [len(np.unique(comp_of)), len(u), np.bincount(lab[u]).max(), len(touched), np.bincount(comp_of).max()]
    return out


@pytest.mark.parametrize("seed", range(6))
def test_oracle_equals_scipy_on_random_batches(seed):
    rng = np.random.RandomState(100 + seed)
    S = [1, 3, 16, 4, 2, 7][seed]
    G = 9
    ei, batch, level = _random_batch(rng, G, 12, S)
    got = co.batch_components(ei, batch, G, level, S)
    want = _scipy_rows(ei, batch, G, level, S)
    assert np.array_equal(got["per_graph"], want)
    acc = np.zeros((S, 8), np.int64)
    for g in range(G):
        for s in range(S):
            r = want[g, s]
            acc[s] += [1, r[0], r[1], r[2], r[3], r[4], int(r[0] == 1), 0]
    assert np.array_equal(got["acc"], acc)
    # labels of the last level: nodes share a label iff scipy puts them into one component, and the label is the smallest id
    keep = level < S
    _, lab = connected_components(coo_matrix((np.ones(keep.sum()), (ei[0, keep], ei[1, keep])), shape=(len(batch),) * 2), directed=False)
    nc = got["node_comp"]
    on = nc >= 0
    assert set(np.flatnonzero(on)) == set(np.concatenate([ei[0, keep], ei[1, keep]]))
    for c in np.unique(lab[on]):
        members = np.flatnonzero(on & (lab == c))
        assert np.all(nc[members] == members.min())


def _one_graph(n, edges, levels, S, **kw):
    ei = np.array(edges, np.int64).reshape(-1, 2).T
    return co.batch_components(ei, np.zeros(n, np.int64), 1, np.array(levels, np.uint8), S, **kw)


def test_hand_written_answers():
    # two triangles, joined by an edge of the last level
    tri = [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (2, 3)]
    r = _one_graph(6, tri, [0, 0, 0, 1, 1, 1, 2], 3)
    assert r["per_graph"][0].tolist() == [[1, 3, 3, 3, 3], [2, 6, 3, 6, 3], [1, 7, 7, 6, 6]]
    assert r["acc"].tolist() == [[1, 1, 3, 3, 3, 3, 1, 0], [1, 2, 6, 3, 6, 3, 0, 0], [1, 1, 7, 7, 6, 6, 1, 0]]
    assert r["node_comp"].tolist() == [0] * 6 and r["edge_big"].tolist() == [1] * 7
    # the same without the bridge: a tie of two components with three kept slots each goes to the smaller label
    r = _one_graph(7, tri[:6], [0] * 6, 1)
    assert r["per_graph"][0].tolist() == [[2, 6, 3, 6, 3]]
    assert r["node_comp"].tolist() == [0, 0, 0, 3, 3, 3, -1] and r["edge_big"].tolist() == [1, 1, 1, 0, 0, 0]
    # a self-loop only: one touched node, one component, one kept slot; it joins nothing
    r = _one_graph(3, [(1, 1)], [0], 2)
    assert r["per_graph"][0].tolist() == [[1, 1, 1, 1, 1]] * 2 and r["node_comp"].tolist() == [-1, 1, -1] and r["edge_big"].tolist() == [1]
    # a duplicated edge counts twice as a slot and once as a connection
    r = _one_graph(3, [(0, 2), (0, 2), (2, 0)], [0, 0, 0], 1)
    assert r["per_graph"][0].tolist() == [[1, 3, 3, 2, 2]] and r["node_comp"].tolist() == [0, -1, 0]
    # a one-directional path 3 -> 2 -> 1 -> 0 is one component; its second half arrives one level later
    r = _one_graph(4, [(3, 2), (2, 1), (1, 0)], [0, 1, 1], 2)
    assert r["per_graph"][0].tolist() == [[1, 1, 1, 2, 2], [1, 3, 3, 4, 4]] and r["node_comp"].tolist() == [0, 0, 0, 0]
    # nothing kept: zeros, counted as a graph, not connected; a byte of S or above is in no level
    r = _one_graph(2, [(0, 1)], [2], 2)
    assert r["per_graph"][0].tolist() == [[0] * 5] * 2 and r["acc"].tolist() == [[1, 0, 0, 0, 0, 0, 0, 0]] * 2
    assert r["node_comp"].tolist() == [-1, -1] and r["edge_big"].tolist() == [0]


def test_valid_word_and_skips():
    ei = np.array([[0, 1, 2, 3, 4, 5], [1, 0, 3, 2, 5, 4]], np.int64)
    batch = np.array([0, 0, 1, 1, 2, 2], np.int64)
    level = np.zeros(6, np.uint8)
    full = co.batch_components(ei, batch, 3, level, 1)
    assert full["acc"].tolist() == [[3, 3, 6, 6, 6, 6, 3, 0]]
    two = co.batch_components(ei, batch, 3, level, 1, valid=[4, 4, 2, 0])
    assert two["acc"].tolist() == [[2, 2, 4, 4, 4, 4, 2, 0]] and two["per_graph"][2].tolist() == [[0] * 5]
    assert two["node_comp"].tolist() == [0, 0, 2, 2, -1, -1]
    cut = co.batch_components(ei, batch, 3, level, 1, valid=[6, 3, 3, 0])          # slot 3 and beyond are never read
    assert cut["per_graph"][:, 0].tolist() == [[1, 2, 2, 2, 2], [1, 1, 1, 2, 2], [0, 0, 0, 0, 0]]
    assert not co.batch_components(ei, batch, 3, level, 1, valid=[6, 6, 3, 1])["acc"].any()
    # a bound below the second graph's size: that graph alone is skipped
    batch2 = np.array([0, 0, 1, 1, 1, 2], np.int64)
    ei2 = np.array([[0, 2, 3, 5], [1, 3, 4, 5]], np.int64)
    r = co.batch_components(ei2, batch2, 3, np.zeros(4, np.uint8), 1, max_seg_nodes=2)
    assert r["per_graph"][:, 0].tolist() == [[1, 1, 1, 2, 2], [-1] * 5, [1, 1, 1, 1, 1]] and r["acc"].tolist() == [[2, 2, 2, 2, 3, 3, 2, 1]]
    # an edge that leaves its graph skips the graph of its source
    r = co.batch_components(np.array([[0, 2], [1, 1]], np.int64), np.array([0, 0, 1], np.int64), 2, np.zeros(2, np.uint8), 1)
    assert r["per_graph"][:, 0].tolist() == [[1, 1, 1, 2, 2], [-1] * 5] and r["acc"][0, 7] == 1


def test_levels_restatement_is_nested():
    rng = np.random.RandomState(5)
    ei, batch, _ = _random_batch(rng, 5, 9, 1)
    att = rng.randint(0, 4, size=ei.shape[1]) / 4.0                               # ties
    lv = co.levels_of(att, ei, batch, 5, ratios=[0.2, 0.5, 1.0])
    eg = batch[ei[0]]
    for g in range(5):
        n = int((eg == g).sum())
        for s, r in enumerate([0.2, 0.5, 1.0]):
            assert int(((eg == g) & (lv <= s)).sum()) == int(np.ceil(n * r))


def test_python_argument_checks_need_no_device():
    import dp_gsat_amd as G
    from dp_gsat_amd import explain
    from dp_gsat_amd._lib import GsatHipError
    ei = torch.tensor([[0, 1], [1, 0]])
    batch = torch.zeros(2, dtype=torch.int64)
    lv = torch.zeros(2, dtype=torch.uint8)
    cap = G.components_lds_cap()
    assert cap >= 4096 and 1 <= explain.components_wave_nodes() < cap
    for bad in (lambda: G.level_components(ei, batch, lv, 0), lambda: G.level_components(ei, batch, lv, 17),
                lambda: G.level_components(ei, batch, lv.to(torch.int32), 1), lambda: G.level_components(ei, batch, lv[:1], 1),
                lambda: G.level_components(ei.to(torch.int32), batch, lv, 1),
                lambda: G.level_components(ei, batch, lv, 1, max_seg_nodes=cap + 1),
                lambda: G.level_components(ei, batch, lv, 1, max_seg_nodes=-1),
                lambda: G.level_components(ei, batch, lv, 2, out=torch.zeros(2, 3, dtype=torch.int64)),
                lambda: G.level_components_reset(torch.zeros(2, 3, dtype=torch.int64)),
                lambda: G.largest_component_mask(ei, batch, torch.zeros(3, dtype=torch.bool)),
                lambda: G.component_labels(ei, batch, torch.zeros(2)),
                lambda: explain.check_levels(None, None)):
        with pytest.raises(ValueError):
            bad()
    for cpu in (lambda: G.level_components(ei, batch, lv, 1), lambda: G.largest_component_mask(ei, batch, torch.ones(2, dtype=torch.bool)),
                lambda: G.component_labels(ei, batch, torch.ones(2, dtype=torch.bool))):
        with pytest.raises(GsatHipError):
            cpu()
    s = explain.connectivity_scores([[2, 3, 10, 6, 8, 5, 1, 0], [0] * 8])
    assert s == {"components": [1.5, 0.0], "largest_edge_share": [0.6, 0.0], "largest_node_share": [0.625, 0.0],
                 "connected_fraction": [0.5, 0.0], "n": 2}
    assert co.scores([[2, 3, 10, 6, 8, 5, 1, 0], [0] * 8]) == s
