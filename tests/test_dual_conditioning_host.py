"""not gpu: tests.dual_oracle.widest_fp32_gradients, which the replayed dual/primal step test takes its fp32 references from, on the
oracle alone.  It may only widen the slack where the reference itself is uncertain: a GIN step takes no scatter mean, so its references
must come back bit for bit; on a PNA step with the default dual features the widened reference is never closer to fp64 than the plain
one, and the weights in front of the dual std layers move by far more than the plain evaluation's own distance."""
import torch

from tests import dual_oracle as do
from tests import padded_oracle as po


def _step_args(backbone, ids):
    graphs = do.labelled_graphs(**po.STEP_GRAPHS)
    omods, _ = do.models("cpu", backbone, graphs)
    states = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in omods]
    upb, udb, N, E = do.host_pair(graphs, ids)
    g = torch.Generator().manual_seed(5)
    pu, dU = torch.rand(N, 1, generator=g).clamp_(1e-10, 1 - 1e-10), torch.rand(E, 1, generator=g)
    pm = [(torch.rand(N, 2 * do.H, generator=g) > .5).float(), (torch.rand(N, do.H, generator=g) > .5).float()]
    dm = [(torch.rand(E, 2 * do.H, generator=g) > .5).float(), (torch.rand(E, do.H, generator=g) > .5).float()]
    return omods, (omods, states, upb, udb, False, 0.9, pu, dU, pm, dm)


def test_widest_fp32_references_widen_only_what_the_reference_leaves_open():
    omods, args = _step_args("GIN", po.STEP_IDS[0])
    r32, r64 = do.oracle_step(*args)
    wide = do.widest_fp32_gradients(r32, r64, *args, draws=2)
    assert all(torch.equal(a, b) for a, b in zip(wide[3], r32[3])) and wide[:3] == r32[:3]
    omods, args = _step_args("PNA", po.STEP_IDS[0])
    names, _ = do.names_and_params(omods)
    r32, r64 = do.oracle_step(*args)
    wide = do.widest_fp32_gradients(r32, r64, *args)
    dist = lambda r: {n: float((a.double() - c).abs().max()) for n, a, c in zip(names, r[3], r64[3])}
    plain, widened = dist(r32), dist(wide)
    assert all(widened[n] >= plain[n] for n in names)
    n = "dclf.node_encoder.weight"                                  # in front of the dual std layers: 4.9e-6 against 1.4e-4
    assert widened[n] > 5 * plain[n], (plain[n], widened[n])
