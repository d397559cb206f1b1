"""CPU oracle of gsat_level_components (dp_gsat_amd.level_components and what is built on it): numpy and a plain union-find, nothing
from the package.  It restates the contract of include/gsat_hip.h:

* level ``s`` keeps the edge slots with ``level[e] <= s`` (a byte of ``S`` or above is in no level); direction is ignored, a self-loop
  joins nothing, the touched nodes of a level are the endpoints of its kept slots;
* per looked-at graph and level the five counts (components, kept, big_edges, touched, big_nodes), zeros with nothing kept;
* ``acc[s] += (1, components, kept, big_edges, touched, big_nodes, components == 1, 0)`` per counted graph, ``acc[0][7]`` counts the
  skipped graphs;
* ``valid`` = (N_real, E_real, B, overflow): only graphs below ``clamp(valid[2], 0, G)`` are looked at, none with ``valid[3]``; an edge
  at or beyond ``clamp(valid[1], 0, E)`` is never read and kept at no level;
* a graph is skipped whole (-1 rows, ``acc[0][7]``) when it has more nodes than ``max_seg_nodes``, when its node or slot range is not
  inside [0, N] / [0, E], when a slot names an edge outside [0, E), or when a read edge has an endpoint outside its node range;
* of the LAST level: ``node_comp`` = the smallest batch-global node id of the node's component, -1 untouched; ``edge_big`` = 1 iff the
  slot is kept and lies in the component with the most kept slots, ties to the smaller label, 0 for every other read slot;
* whatever is not looked at (and node_comp / edge_big of a skipped graph, edge_big at or beyond valid[1]) keeps what the caller put there.
"""
import numpy as np


def segments(edge_index, batch, G):
    """(node_ptr int32[G + 1], edge_ptr int32[G + 1], edge_order int32[E]) of a sorted ``batch`` vector: the edges grouped by the
    graph of their SOURCE node, in edge order inside a graph."""
    edge_index, batch = np.asarray(edge_index, np.int64).reshape(2, -1), np.asarray(batch, np.int64)
    node_ptr = np.zeros(G + 1, np.int32)
    node_ptr[1:] = np.cumsum(np.bincount(batch, minlength=G)[:G])
    eg = batch[edge_index[0]] if edge_index.shape[1] else np.zeros(0, np.int64)
    edge_ptr = np.zeros(G + 1, np.int32)
    edge_ptr[1:] = np.cumsum(np.bincount(eg, minlength=G)[:G])
    return node_ptr, edge_ptr, np.argsort(eg, kind="stable").astype(np.int32)


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def graph_components(n, u, v, lvl, S):
    """One graph with local endpoints ``u``, ``v`` and level bytes ``lvl`` per slot: (rows int[S][5], labels of the last level (local,
    -1 untouched), the local root of the largest component of the last level or -1)."""
    parent, touched = list(range(n)), [False] * n
    rows, best = [], -1
    for s in range(S):
        for a, b, l in zip(u, v, lvl):
            if l == s:
                touched[a] = touched[b] = True
                ra, rb = _find(parent, a), _find(parent, b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)          # the root is always the smallest id of its component
        cn, ce = {}, {}
        for x in range(n):
            if touched[x]:
                r = _find(parent, x)
                cn[r] = cn.get(r, 0) + 1
        for a, b, l in zip(u, v, lvl):
            if l <= s:
                r = _find(parent, a)
                ce[r] = ce.get(r, 0) + 1
        big_e = max(ce.values(), default=0)
        rows.append([len(cn), sum(ce.values()), big_e, sum(cn.values()), max(cn.values(), default=0)])
        if s == S - 1 and big_e > 0:
            best = min(r for r, c in ce.items() if c == big_e)
    labels = [_find(parent, x) if touched[x] else -1 for x in range(n)]
    return rows, labels, best


def level_components(edge_index, N, node_ptr, edge_ptr, edge_order, G, level, S, max_seg_nodes, valid=None, per_graph=None, acc=None,
                     node_comp=None, edge_big=None):
    """The four outputs as the kernel leaves them, starting from the caller's arrays (copied; defaults: zeros for ``acc``, -7 / -7 / 9
    sentinels for per_graph / node_comp / edge_big): dict(per_graph int32[G, S, 5], acc int64[S, 8], node_comp int32[N], edge_big
    uint8[E])."""
    edge_index = np.asarray(edge_index, np.int64).reshape(2, -1)
    E = edge_index.shape[1]
    level = np.asarray(level, np.uint8).reshape(-1)
    per_graph = np.full((G, S, 5), -7, np.int32) if per_graph is None else np.array(per_graph, np.int32)
    acc = np.zeros((S, 8), np.int64) if acc is None else np.array(acc, np.int64)
    node_comp = np.full(N, -7, np.int32) if node_comp is None else np.array(node_comp, np.int32)
    edge_big = np.full(E, 9, np.uint8) if edge_big is None else np.array(edge_big, np.uint8)
    Gv, Ev = G, E
    if valid is not None:
        Gv = 0 if valid[3] else min(max(int(valid[2]), 0), G)
        Ev = min(max(int(valid[1]), 0), E)
    for g in range(Gv):
        nlo, nhi, elo, ehi = int(node_ptr[g]), int(node_ptr[g + 1]), int(edge_ptr[g]), int(edge_ptr[g + 1])
        n = nhi - nlo
        ok = 0 <= nlo <= nhi <= N and 0 <= elo <= ehi <= E and n <= max_seg_nodes
        slots, u, v, lvl = [], [], [], []
        if ok:
            for i in range(elo, ehi):
                e = int(edge_order[i])
                if not 0 <= e < E:
                    ok = False
                    break
                if e >= Ev:
                    continue
                a, b = int(edge_index[0, e]) - nlo, int(edge_index[1, e]) - nlo
                if not (0 <= a < n and 0 <= b < n):
                    ok = False
                    break
                slots.append(e); u.append(a); v.append(b); lvl.append(int(level[e]) if level[e] < S else 255)
        if not ok:
            per_graph[g] = -1
            acc[0, 7] += 1
            continue
        rows, labels, best = graph_components(n, u, v, lvl, S)
        per_graph[g] = rows
        for s, r in enumerate(rows):
            acc[s] += [1, r[0], r[1], r[2], r[3], r[4], int(r[0] == 1), 0]
        node_comp[nlo:nhi] = [nlo + l if l >= 0 else -1 for l in labels]
        for e, a, l in zip(slots, u, lvl):
            edge_big[e] = 1 if (l < S and best >= 0 and labels[a] == best) else 0
    return dict(per_graph=per_graph, acc=acc, node_comp=node_comp, edge_big=edge_big)


def batch_components(edge_index, batch, G, level, S, max_seg_nodes=None, ranked_graphs=None, valid=None):
    """What ``dp_gsat_amd.level_components(..., per_graph=True, labels=True)`` returns for a fresh ``out``: the Python layer starts from
    zero rows, -1 labels and a False mask, and takes the batch's largest node count when no bound is given."""
    batch = np.asarray(batch, np.int64)
    node_ptr, edge_ptr, order = segments(edge_index, batch, G)
    if max_seg_nodes is None:
        max_seg_nodes = int(np.diff(node_ptr).max()) if G else 0
    looked = G if ranked_graphs is None else ranked_graphs
    E = np.asarray(edge_index).reshape(2, -1).shape[1]
    return level_components(edge_index, len(batch), node_ptr, edge_ptr, order, looked, level, S, max_seg_nodes, valid,
                            per_graph=np.zeros((looked, S, 5), np.int32), node_comp=np.full(len(batch), -1, np.int32),
                            edge_big=np.zeros(E, np.uint8))


def scores(acc):
    """The dict of ``dp_gsat_amd.explain.connectivity_scores`` from an accumulator int64[S, 8]."""
    ratio = lambda a, b: a / b if b else 0.0
    acc = np.asarray(acc, np.int64).tolist()
    return {"components": [ratio(c[1], c[0]) for c in acc], "largest_edge_share": [ratio(c[3], c[2]) for c in acc],
            "largest_node_share": [ratio(c[5], c[4]) for c in acc], "connected_fraction": [ratio(c[6], c[0]) for c in acc],
            "n": int(acc[0][0])}


def levels_of(att, edge_index, batch, G, ks=None, ratios=None):
    """uint8[E] of ``explanation_levels``: the smallest level whose top-k (or top-ceil(ratio * E_g)) of the edge's graph holds it --
    higher attention first, equal attention -> lower edge id first."""
    att = np.asarray(att, np.float64).reshape(-1)
    _, edge_ptr, order = segments(edge_index, batch, G)
    cuts = ks if ks is not None else ratios
    S = len(cuts)
    level = np.full(att.shape[0], S, np.uint8)
    for g in range(G):
        ids = order[edge_ptr[g]:edge_ptr[g + 1]].astype(np.int64)
        ranked = ids[np.lexsort((ids, -att[ids]))]
        for s in range(S - 1, -1, -1):
            keep = int(cuts[s]) if ks is not None else int(np.ceil(np.float64(len(ids)) * np.float64(cuts[s])))
            level[ranked[:keep]] = s
    return level
