"""not gpu: the capacity bound and the padding layout of fixed-capacity batches (numpy restatement in tests/padded_oracle.py), and the
case tables of tests/test_gpu_padded.py vetted on the host."""
import numpy as np
import pytest
import torch

from tests import padded_oracle as po


def test_capacity_for_matches_numpy():
    import dp_gsat_amd as G
    graphs = po.mutag_graphs(128)
    n, e = po.sizes(graphs)
    ds = G.PackedDataset.from_data_list(graphs, "cpu")
    for k in (1, 5, 16, 128, 500):
        want = po.capacity_for(n, e, k)
        assert ds.capacity_for(k) == want
        assert want[0] == np.sort(n)[-min(k, 128):].sum() + 2 and want[1] == np.sort(e)[-min(k, 128):].sum()
    assert ds.capacity_for(16) is ds.capacity_for(16)          # cached: the host read happens once
    with pytest.raises(ValueError):
        ds.capacity_for(0)
    rng = np.random.RandomState(0)                             # a bound: no batch of k distinct graphs exceeds it
    for _ in range(50):
        ids = rng.choice(128, 16, replace=False)
        N, E = po.totals(graphs, ids)
        assert N + 2 <= ds.capacity_for(16)[0] and E <= ds.capacity_for(16)[1]


def test_padding_layout_invariants():
    graphs = po.mutag_graphs(**po.LAYOUT_GRAPHS)
    assert graphs[11].x.shape[0] == 1 and graphs[11].edge_index.shape[1] == 0 and 11 in po.LAYOUT_IDS
    assert po.LAYOUT_IDS != sorted(po.LAYOUT_IDS)
    N, E = po.totals(graphs, po.LAYOUT_IDS)
    cases = po.layout_cases()
    want_pads = {"tight": (2, 0), "odd_self_loop": (5, 9), "duplicated": (2, 40), "wide": (30, 7)}
    for name, cap in cases.items():
        lay = po.collate_padded(graphs, po.LAYOUT_IDS, cap)
        assert lay["valid"].tolist() == [N, E, 5, 0]
        assert (cap[0] - N, cap[1] - E) == want_pads[name]
        po.check_invariants(lay, cap)
        pad = lay["edge_index"][:, E:]
        if name == "odd_self_loop":
            assert pad[0, -1] == pad[1, -1] and (pad[0, :-1] != pad[1, :-1]).all()        # one self loop, in the last slot
        if name == "duplicated":
            assert sorted(np.bincount(pad[1] - N).tolist()) == [20, 20]                   # every pair twenty times: a high in-degree row
        if name == "wide":
            assert lay["batch"][N:].tolist() == [5] * 30
    for cap in [(N + 1, E), (N + 2, E - 1)]:                   # does not fit: all padding, flagged, still a valid layout
        lay = po.collate_padded(graphs, po.LAYOUT_IDS, cap)
        assert lay["valid"].tolist() == [0, 0, 5, 1]
        po.check_invariants(lay, cap)


def test_replay_id_sets_fit_the_capacity():
    graphs = po.mutag_graphs(**po.STEP_GRAPHS)
    n, e = po.sizes(graphs)
    assert e[5] % 2 == 1 and (np.delete(e, 5) % 2 == 0).all()
    cap = po.capacity_for(n, e, po.STEP_BATCH)
    assert cap[1] % 2 == 0                                     # graph 5 is not among the sixteen largest
    seen = set()
    for ids in po.STEP_IDS:
        assert len(ids) == po.STEP_BATCH == len(set(ids)) and max(ids) < len(graphs)
        N, E = po.totals(graphs, ids)
        assert N + 2 <= cap[0] and E <= cap[1]
        seen.add((N, E))
    assert len(seen) == 3
    e_pads = [cap[1] - po.totals(graphs, ids)[1] for ids in po.STEP_IDS]
    assert [p % 2 for p in e_pads] == [0, 1, 0]
    for g in graphs:                                           # every graph's edge set is symmetric, the self loop included
        ei = g.edge_index.numpy()
        assert sorted(map(tuple, ei.T.tolist())) == sorted(map(tuple, ei[::-1].T.tolist()))


def test_padded_context_is_scoped():
    import dp_gsat_amd as G
    assert G.current_padding() is None
    with pytest.raises(ValueError):
        with G.padded(torch.zeros(4, dtype=torch.int32)):      # the counts live on the device
            pass
    assert G.current_padding() is None
