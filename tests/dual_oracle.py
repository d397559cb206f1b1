"""Helpers of the padded dual/primal tests: graph lists with edge labels, the four modules next to their oracle twins, and the oracle's
DualGSAT step on UNPADDED batches in fp32 and fp64."""
import copy
from types import SimpleNamespace as NS

import torch

from oracle import bookkeeping as obk
from oracle import modules as om
from oracle import ops as oops
from tests import padded_oracle as po
from tests.util import TOL, close

H = 16
MCFG = dict(pred_loss_coef=1, info_loss_coef=1, fix_r=False, decay_interval=10, decay_r=0.1, final_r=0.5)
SHARED = {"learn_edge_att": False, "extractor_dropout_p": 0.5}


def labelled_graphs(**kw):
    """tests.padded_oracle.mutag_graphs with a 0/1 label on every edge (about a third are 1)."""
    graphs = po.mutag_graphs(**kw)
    gen = torch.Generator().manual_seed(7)
    for g in graphs:
        g.edge_label = (torch.rand(g.edge_index.shape[1], generator=gen) > 0.67).float()
    return graphs


def host_pair(graphs, ids, dual_x=None):
    """The unpadded primal and dual batches of ``ids`` built on the host, as PackedDataset.collate gives them: (primal, dual, N, E)."""
    de = dual_edges(graphs)
    eoff = [0]
    for g in graphs:
        eoff.append(eoff[-1] + int(g.edge_index.shape[1]))
    xs, eis, bs, els, dxs, deis, dbs = [], [], [], [], [], [], []
    no = eo = 0
    for k, g in enumerate(ids):
        gr = graphs[g]
        n, e = int(gr.x.shape[0]), int(gr.edge_index.shape[1])
        xs.append(gr.x); eis.append(gr.edge_index + no); bs += [k] * n; els.append(gr.edge_label)
        dxs.append(torch.cat([gr.x[gr.edge_index[0]], gr.x[gr.edge_index[1]]], 1) if dual_x is None else dual_x[eoff[g]:eoff[g + 1]])
        deis.append(torch.from_numpy(de[g]) + eo); dbs += [k] * e
        no, eo = no + n, eo + e
    y = torch.cat([graphs[g].y for g in ids])
    primal = NS(x=torch.cat(xs), edge_index=torch.cat(eis, 1), batch=torch.tensor(bs), y=y, edge_label=torch.cat(els))
    dual = NS(x=torch.cat(dxs), edge_index=torch.cat(deis, 1), batch=torch.tensor(dbs), y=y)
    return primal, dual, no, eo


def dual_edges(graphs):
    """Per graph: the dual edge list dp_gsat_amd.line_graph gives (local ids) -- oracle.bookkeeping.line_graph_by_source, which takes the
    source nodes in order of first appearance, on the edges stably sorted by source, so that the groups come in ascending node order
    with their edges in edge order, mapped back to the original edge numbers."""
    out = []
    for g in graphs:
        perm = torch.argsort(g.edge_index[0], stable=True)
        d = obk.line_graph_by_source(g.edge_index[:, perm])
        out.append(perm.numpy()[d] if d.size else d)
    return out


def pair_totals(graphs, ids):
    """(N, E, E_dual) of the batch ``ids``."""
    N, E = po.totals(graphs, ids)
    d = dual_edges(graphs)
    return N, E, int(sum(d[g].shape[1] for g in ids))


def models(dev, backbone, graphs):
    """(oracle modules [pc, pe, dc, de], device modules [pc, pe, dc, de]) with equal parameters."""
    import dp_gsat_amd as G
    deg_p = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=g.x.shape[0]) for g in graphs]), minlength=10)
    deg_d = torch.bincount(torch.cat([torch.bincount(torch.from_numpy(d[1]), minlength=g.edge_index.shape[1])
                                      for g, d in zip(graphs, dual_edges(graphs))]), minlength=10)
    out_o, out_d = [], []
    for x_dim, deg, side in ((14, deg_p, "primal"), (28, deg_d, "dual")):
        cfg = dict(model_name=backbone, n_layers=2, hidden_size=H, dropout_p=0.0, use_edge_attr=False,
                   aggregators=["mean", "min", "max", "std"], scalers=False, deg=deg)
        oclf = {"GIN": om.GIN, "PNA": om.PNA}[backbone](x_dim, 0, 2, False, cfg)
        oext = om.ExtractorMLP(H, False)
        clf = G.get_model(x_dim, 0, 2, False, cfg, dev)
        clf.load_state_dict(oclf.state_dict())
        ext = G.ExtractorMLP(H, SHARED, side).to(dev)
        ext.load_state_dict({side + "_" + k: v for k, v in oext.state_dict().items()})
        out_o += [oclf, oext]
        out_d += [clf, ext]
    return out_o, out_d


def names_and_params(mods):
    tags = ("pclf.", "pext.", "dclf.", "dext.")
    names = [t + n for t, m in zip(tags, mods) for n, _ in m.named_parameters()]
    return names, [p for m in mods for p in m.parameters()]


def state_of(mods):
    """CPU copies of the four device modules' state dicts, the extractors' keys without their primal_ / dual_ prefix."""
    out = []
    for m, prefix in zip(mods, ("", "primal_", "", "dual_")):
        out.append({k[len(prefix):]: v.detach().clone().cpu() for k, v in m.state_dict().items()})
    return out


def oracle_step(omods, states, upb, udb, mixed, dual_r, pu, dU, pm, dm, dtypes=(torch.float32, torch.float64)):
    """The oracle's DualGSAT step on the unpadded CPU batches from ``states``: dt -> (primal_edge_att, loss, primal logits, gradients of the
    four modules in order, the two backbones' state dicts afterwards).  The oracle mixes for epoch > 50 and takes a fixed dual r."""
    runs = {}
    dcfg = dict(MCFG, fix_r=float(dual_r))
    for dt in dtypes:
        mods = [copy.deepcopy(m) for m in omods]
        for m, sd in zip(mods, states):
            m.load_state_dict(sd)
        mods = [m.to(dt) for m in mods]
        pd = NS(x=upb.x.to(dt), edge_index=upb.edge_index, batch=upb.batch, edge_attr=None, y=upb.y.to(dt), edge_label=upb.edge_label.to(dt))
        dd = NS(x=udb.x.to(dt), edge_index=udb.edge_index, batch=udb.batch, edge_attr=None, y=udb.y.to(dt))
        og = om.DualGSAT(mods[0], mods[1], mods[2], mods[3], MCFG, dcfg, False, False).train()
        att, loss, _, logits = og.dual_forward_pass(pd, dd, 60 if mixed else 3, True, pu.to(dt), dU.to(dt), [m.to(dt) for m in pm],
                                                    [m.to(dt) for m in dm])
        loss.backward()
        runs[dt] = (att.detach(), loss.detach(), logits.detach(), [p.grad for m in mods for p in m.parameters()],
                    [{k: v.detach().clone() for k, v in mods[i].state_dict().items()} for i in (0, 2)])
    return runs.get(torch.float32), runs.get(torch.float64)


def widest_fp32_gradients(r32, r64, *step_args, draws=4):
    """``r32`` with every gradient replaced by the fp32 evaluation of the oracle that lies farthest from fp64, among the plain one and
    ``draws`` evaluations whose scatter means (the mean and mean-of-squares of PNA's std, and nothing else) are off by one fp32 ulp with a
    seeded random sign per entry.  tests.util.close grants 4x |ref - ref64| as slack for the reference's own rounding; one fp32 evaluation
    measures that only if another valid one lands about as close.  The kernels do not divide as the reference does: they multiply by
    fl(1 / n) and accumulate squares with fma (csrc/pna_math.h, "at most one ulp"), so means one ulp apart are the difference between
    two correct implementations.  Where var = E[m^2] - E[m]^2 cancels below the 1e-5 under the root (near-duplicate messages: the
    default dual features of two edges leaving one atom differ in one column) that ulp is amplified by 1 / std^3 -- the conditioning
    tests/test_gpu_pna.py weighs with std_conditioning -- and adds up over a batch in the weights in front of the layer.  A GIN step never
    takes a scatter mean: its references come back unchanged (tests/test_dual_conditioning_host.py)."""
    grads = list(r32[3])
    dist = [float((a.double() - c).abs().max()) for a, c in zip(grads, r64[3])]
    plain = oops.scatter_mean
    for seed in range(draws):
        gen = torch.Generator().manual_seed(seed)

        def one_ulp_off(src, index, dim_size):
            out = plain(src, index, dim_size)
            sign = (torch.randint(0, 3, out.shape, generator=gen) - 1).to(out.dtype)
            return out * (1 + sign * 2.0 ** -23)

        oops.scatter_mean = one_ulp_off
        try:
            q32, _ = oracle_step(*step_args, dtypes=(torch.float32,))
        finally:
            oops.scatter_mean = plain
        for k, (b, c) in enumerate(zip(q32[3], r64[3])):
            d = float((b.double() - c).abs().max())
            if d > dist[k]:
                grads[k], dist[k] = b, d
    return r32[:3] + (grads,) + r32[4:]


def check_step(got_att, got_loss, got_logits, mods, r32, r64, E, B, what):
    (a32, l32, z32, g32, s32), (a64, l64, z64, g64, s64) = r32, r64
    close(got_loss.reshape(()), l32.reshape(()), TOL, ref64=l64.reshape(()), what=what + "loss")
    close(got_att[:E], a32, TOL, ref64=a64, what=what + "primal_edge_att")
    close(got_logits[:B], z32, TOL, ref64=z64, what=what + "clf_logits")
    names, params = names_and_params(mods)
    assert len(params) == len(g32)
    for n, p, q32, q64 in zip(names, params, g32, g64):
        if q32 is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        assert p.grad is not None, n
        close(p.grad, q32, TOL, ref64=q64, what=what + "grad " + n)
    for clf, t32, t64, side in ((mods[0], s32[0], s64[0], "primal "), (mods[2], s32[1], s64[1], "dual ")):
        sd = clf.state_dict()
        stats = [k for k in sd if "running_" in k]
        assert stats
        for k in stats:
            close(sd[k], t32[k], TOL, ref64=t64[k], what=what + side + k)
        for k in sd:
            if k.endswith("num_batches_tracked"):
                assert int(sd[k]) == int(t32[k]), side + k


def f1_reference(p, y, m, gout=1.0):
    """fp64 restatement of src/run_gsat.py:151-180 over the first m entries, with autograd: (loss, dp[:m])."""
    a = p[:m].double().reshape(-1).clone().requires_grad_(True)
    b = y[:m].double().reshape(-1)
    if m == 0:
        return torch.ones((), dtype=torch.float64), a.detach()
    eps = 1e-6
    TP, P, G = (a * b).sum(), a.sum(), b.sum()
    precision, recall = TP / (P + eps), TP / (G + eps)
    f1 = 2 * precision * recall / (precision + recall + eps)
    loss = (1 - f1) + a.abs().mean()
    (loss * gout).backward()
    return loss.detach(), a.grad
