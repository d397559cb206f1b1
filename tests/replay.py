"""Helpers of the replayed-step tests: capture a step as bench.py does, record and predict the device seed words a replay draws,
regenerate the Philox inputs the kernels drew from them, evaluate the bench's scope-A step with the oracle, and build fresh batches of
an exact (N, E, G) to feed a captured graph."""
import numpy as np
import torch

from oracle import bookkeeping as obk
from oracle import modules as om
from oracle import ops as oops

_M64 = (1 << 64) - 1


def capture(fn):
    """bench.py's captured(): three eager warm-up calls of ``fn`` on a side stream, then one torch.cuda.graph capture; returns the graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def seed_next_ref(base, counter):
    """The word gsat_seed_next writes for the state (base, counter) it reads (it stores counter + 1 back): splitmix64 of
    base + (counter + 1) * golden, top bit cleared."""
    c = (int(counter) + 1) & _M64
    z = (int(base) + c * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return z & 0x7FFFFFFFFFFFFFFF


def seed_state(dev):
    """(base, counter) of the device seed stream of ``dev``, read now."""
    from dp_gsat_amd.ops import device_seed_state
    st = device_seed_state(dev)
    assert st is not None, "the device seed stream has not been used yet"
    base, counter = st.tolist()
    return base & _M64, counter


def pin_seed_stream(dev, base):
    """Restart the device seed stream of ``dev`` at (base, 0): the words a replay draws then do not depend on which tests ran before."""
    from dp_gsat_amd.ops import device_seed_state
    device_seed_state(dev).copy_(torch.tensor([int(base), 0], dtype=torch.int64))


class SeedRecorder:
    """Wraps ``device_seed`` where it is bound (dp_gsat_amd.gsat at import, dp_gsat_amd.ops for the ops and the call-time import in
    encoders.py) and records, in call order, the seed tensors handed out while a stream capture runs.  After a replay, ``words()`` are
    the seed words that replay used."""

    def __init__(self):
        self.tensors = []

    def __enter__(self):
        from dp_gsat_amd import gsat, ops
        self._mods = (gsat, ops)
        self._orig = ops.device_seed

        def recording(device):
            t = self._orig(device)
            if torch.cuda.is_current_stream_capturing():
                self.tensors.append(t)
            return t

        for m in self._mods:
            m.device_seed = recording
        return self

    def __exit__(self, *exc):
        for m in self._mods:
            m.device_seed = self._orig
        return False

    def words(self):
        return [int(t.item()) for t in self.tensors]

    def check(self, base, counter):
        """Every recorded word equals the host prediction from the state (base, counter) read before the replay."""
        got = self.words()
        want = [seed_next_ref(base, counter + i) for i in range(len(got))]
        assert got == want, f"device seed words {got} != host prediction {want}"
        return got


def philox_inputs(seed, M, C1, C2, p, dev):
    """What the extractor kernels draw in-kernel for ``seed``: keep-masks (Philox streams 1, 2) and the concrete noise u (stream 4),
    as CPU tensors [(M, C1), (M, C2)], [M, 1]."""
    from dp_gsat_amd._lib import call, ptr, stream
    m1 = torch.empty(M, C1, device=dev)
    m2 = torch.empty(M, C2, device=dev)
    u = torch.empty(M, 1, device=dev)
    call("gsat_philox_keep_mask", int(seed), 1, M, C1, float(p), ptr(m1), stream())
    call("gsat_philox_keep_mask", int(seed), 2, M, C2, float(p), ptr(m2), stream())
    call("gsat_philox_noise", int(seed), M, ptr(u), stream())
    return [m1.cpu(), m2.cpu()], u.cpu()


def scope_a_reference(wl, data, emb, xs, ees, gouts, u, masks, ext_state, dtype):
    """The bench's scope-A step (bench.HotPath.compute) on the oracle in ``dtype``: every output by the name HotPath.outputs() uses
    (``edge_att`` in node mode too, the lifted [E, 1] tensor)."""
    import bench
    H, L, edge = wl["H"], wl["L"], wl["edge_att"]
    N = data.batch.shape[0]
    ext = om.ExtractorMLP(H, edge).to(dtype).train()
    ext.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in ext_state.items()})
    e = emb.detach().cpu().to(dtype).clone().requires_grad_(True)
    xl = [t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in xs]
    eel = [t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in ees] if ees is not None else None
    logits = ext(e, data.edge_index, data.batch, masks=[m.to(dtype) for m in masks])
    att = oops.concrete_sample(logits, u.to(dtype), True)
    if edge:
        rev = torch.from_numpy(obk.reverse_edge_perm(data.edge_index, N)) if obk.is_undirected(data.edge_index, N) else None
        ea = oops.symmetrise(att, rev)
    else:
        ea = oops.lift_node_att_to_edge_att(att, data.edge_index)
    outs = []
    for l in range(L):
        if wl["backbone"] == "PNA":
            outs.append(oops.pna_aggregate(xl[l], data.edge_index, ea, bench.PNA_AGGR, ["identity"], {"lin": 1.0, "log": 1.0}))
        elif eel is not None:
            outs.append(oops.gine_aggregate(xl[l], data.edge_index, eel[l], ea))
        else:
            outs.append(oops.gin_aggregate(xl[l], data.edge_index, ea))
    torch.autograd.backward(outs, [t.detach().cpu().to(dtype) for t in gouts])
    res = dict(att_log_logits=logits, att=att, edge_att=ea, grad_emb=e.grad)
    for l in range(L):
        res[f"out_l{l}"] = outs[l]
        res[f"grad_x_l{l}"] = xl[l].grad
        if eel is not None:
            res[f"grad_edge_emb_l{l}"] = eel[l].grad
    for n, p in ext.named_parameters():
        res["grad_ext." + n] = p.grad
    return {k: v.detach() for k, v in res.items()}


def fresh_batch(like, seed, undirected, sizes=None, hub_edges=0, redirect=0):
    """A batch with exactly ``like``'s N, E and G (and edge_attr width): graph sizes drawn at random (or ``sizes``), edges inside their
    graphs in random order, reverse pairs when ``undirected`` (plus one self loop when E is odd), ``hub_edges`` edges (both directions
    when undirected) into node 0 of graph 0, and one edge of ``redirect`` reverse pairs pointed elsewhere (the edge set stops being
    symmetric)."""
    from dp_gsat_amd.synth import Batch
    rng = np.random.RandomState(seed)
    N, E, G = int(like.batch.shape[0]), int(like.edge_index.shape[1]), int(like.num_graphs)
    if sizes is None:
        cuts = np.sort(rng.choice(np.arange(1, N - G + 1), G - 1, replace=False)) if G > 1 else np.zeros(0, np.int64)
        sizes = np.diff(np.concatenate([[0], cuts, [N - G]])) + 1          # every graph has at least one node
        rng.shuffle(sizes)
    sizes = np.array(sizes, dtype=np.int64)
    if hub_edges and sizes[0] < 2:
        k = int(np.argmax(sizes))
        sizes[0], sizes[k] = sizes[k], sizes[0]
    assert sizes.sum() == N and sizes.size == G and (sizes >= 1).all()
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    multi = np.flatnonzero(sizes >= 2)
    w = sizes[multi] / sizes[multi].sum()
    per = 2 if undirected else 1
    n_loops = E % 2 if undirected else 0
    n_hub = hub_edges
    n_rand = (E - n_loops - per * n_hub) // per
    assert n_rand >= 0
    gs = multi[rng.choice(multi.size, n_rand, p=w)]
    a = rng.randint(0, sizes[gs])
    b = (a + rng.randint(1, sizes[gs])) % sizes[gs]                        # b != a: no self loops among the random edges
    src, dst = off[gs] + a, off[gs] + b
    hub_src = rng.randint(1, sizes[0], n_hub)
    src = np.concatenate([src, hub_src])
    dst = np.concatenate([dst, np.zeros(n_hub, np.int64)])
    if undirected:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    if n_loops:
        v = int(rng.randint(0, N))
        src, dst = np.concatenate([src, [v]]), np.concatenate([dst, [v]])
    if redirect:
        for k in rng.choice(n_rand, redirect, replace=False):          # the first edge of a pair: its reverse stays unmatched
            g = int(np.searchsorted(off, dst[k], side="right") - 1)
            if sizes[g] >= 3:                                               # another node of the same graph, not the source
                c = int(rng.randint(0, sizes[g]))
                while off[g] + c in (src[k], dst[k]):
                    c = int(rng.randint(0, sizes[g]))
                dst[k] = off[g] + c
    perm = rng.permutation(src.size)
    ei = torch.from_numpy(np.stack([src[perm], dst[perm]]).astype(np.int64)).contiguous()
    assert ei.shape[1] == E
    batch = torch.from_numpy(np.repeat(np.arange(G, dtype=np.int64), sizes))
    ea = None
    if like.edge_attr is not None:
        ea = torch.from_numpy(rng.randn(E, like.edge_attr.shape[1]).astype(np.float32))
    return Batch(x=like.x, edge_index=ei, batch=batch, edge_attr=ea, y=like.y, num_graphs=G)
