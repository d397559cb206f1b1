"""not gpu: the pieces the four replayed classes share that need no device -- the training-state keeper, the capture mode and the id
loading of ``step`` -- on CPU tensors."""
from types import SimpleNamespace as NS

import pytest
import torch

from dp_gsat_amd import graph_index, replay


class _Boom(Exception):
    pass


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(4, 6), torch.nn.BatchNorm1d(6), torch.nn.ReLU(), torch.nn.Linear(6, 2))


def _train_once(net, opts):
    loss = net(torch.randn(8, 4)).square().sum()
    for opt in opts:
        opt.zero_grad()
    loss.backward()
    for opt in opts:
        opt.step()


# ---- 1. the training-state keeper ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fails", [False, True])
def test_kept_training_state_puts_everything_back_in_place(fails):
    net = _net().train()
    stepped = torch.optim.Adam(net[0].parameters(), lr=0.1)
    fresh = torch.optim.Adam(list(net[1].parameters()) + list(net[3].parameters()), lr=0.1)
    _train_once(net, [stepped])                                            # ``stepped`` has state on entry, ``fresh`` has none
    assert len(stepped.state) == 2 and len(fresh.state) == 0
    tensors = dict(net.named_parameters())
    tensors.update(net.named_buffers())
    assert "1.running_mean" in tensors and "1.num_batches_tracked" in tensors
    for i, p in enumerate(net[0].parameters()):
        for key in ("exp_avg", "exp_avg_sq", "step"):
            tensors[f"adam{i}.{key}"] = stepped.state[p][key]
    before = {k: (v.detach().clone(), v.data_ptr()) for k, v in tensors.items()}
    try:
        with replay._kept_training_state(net, (stepped, fresh)):
            _train_once(net, [stepped, fresh])
            assert not torch.equal(tensors["0.weight"], before["0.weight"][0])
            assert not torch.equal(tensors["1.running_mean"], before["1.running_mean"][0])
            assert not torch.equal(tensors["adam0.exp_avg"], before["adam0.exp_avg"][0]) and len(fresh.state) == 4
            if fails:
                raise _Boom()
    except _Boom:
        assert fails
    else:
        assert not fails
    now = dict(net.named_parameters())
    now.update(net.named_buffers())
    for i, p in enumerate(net[0].parameters()):
        for key in ("exp_avg", "exp_avg_sq", "step"):
            now[f"adam{i}.{key}"] = stepped.state[p][key]
    assert set(now) == set(before)
    for key, (value, address) in before.items():
        assert torch.equal(now[key], value) and now[key].data_ptr() == address, key
    created = [v for p in fresh.state for v in fresh.state[p].values() if isinstance(v, torch.Tensor)]
    assert len(created) == 12
    for v in created:
        assert not bool(v.any())


# ---- 2. the capture mode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("evaluating", [False, True])
@pytest.mark.parametrize("was_sync_free", [False, True])
@pytest.mark.parametrize("was_loss_dict", [False, True])
def test_capture_mode_is_put_back_under_an_exception(evaluating, was_sync_free, was_loss_dict):
    net = _net().train()
    net[1].eval()                                                          # a mix of training flags
    net.sync_loss_dict = was_loss_dict
    modes = [m.training for m in net.modules()]
    assert modes == [True, True, False, True, True]
    entry = graph_index.sync_free()
    graph_index.set_sync_free(was_sync_free)
    try:
        with pytest.raises(_Boom):
            with replay._capture_mode(net, evaluating):
                assert graph_index.sync_free() and net.sync_loss_dict is False
                assert [m.training for m in net.modules()] == ([False] * 5 if evaluating else modes)
                graph_index._CACHE["left behind by the block"] = None
                raise _Boom()
        assert graph_index.sync_free() is was_sync_free and net.sync_loss_dict is was_loss_dict
        assert [m.training for m in net.modules()] == modes
        assert len(graph_index._CACHE) == 0
    finally:
        graph_index.set_sync_free(entry)
        graph_index._CACHE.clear()


def test_the_eager_tail_mode_leaves_sync_free_alone():
    net = _net().train()
    net[3].eval()
    net.sync_loss_dict = True
    modes = [m.training for m in net.modules()]
    was = graph_index.sync_free()
    with pytest.raises(_Boom):
        with replay._forward_mode(net, True):
            assert not any(m.training for m in net.modules()) and net.sync_loss_dict is False and graph_index.sync_free() is was
            raise _Boom()
    assert [m.training for m in net.modules()] == modes and net.sync_loss_dict is True


# ---- 3. id loading -----------------------------------------------------------------------------------------------------------------------------------
def _stub(ragged, batch_size=5):
    return NS(graph_ids=torch.full((batch_size,), 77, dtype=torch.int64), batch_size=batch_size, ragged=ragged)


def test_exact_count_id_loading():
    stub = _stub(False)
    for ids in ([0, 1, 2], list(range(6)), []):
        with pytest.raises(ValueError, match="captured for 5 graphs"):
            replay._Replayed._load_ids(stub, ids)
    assert stub.graph_ids.tolist() == [77] * 5                             # a refusal writes nothing
    replay._Replayed._load_ids(stub, torch.tensor([[9, 8, 7, 6, 5]]))
    assert stub.graph_ids.tolist() == [9, 8, 7, 6, 5]


def test_ragged_id_loading():
    stub = _stub(True)
    for ids in ([], list(range(6))):
        with pytest.raises(ValueError, match="1 to 5"):
            replay._Replayed._load_ids(stub, ids)
    assert stub.graph_ids.tolist() == [77] * 5
    replay._Replayed._load_ids(stub, [4, 3, 2])
    assert stub.graph_ids.tolist() == [4, 3, 2, -1, -1]
    replay._Replayed._load_ids(stub, [1, 2, 3, 4, 5])
    assert stub.graph_ids.tolist() == [1, 2, 3, 4, 5]
    replay._Replayed._load_ids(stub, torch.tensor([6, -1, -1, -1, -1]))   # a row of budget_batches carries its own -1s
    assert stub.graph_ids.tolist() == [6, -1, -1, -1, -1]
