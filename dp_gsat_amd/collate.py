"""Device-resident dataset + batch assembly.

The reference collates on the host for every batch (PyG ``DataLoader`` -> ``Batch.from_data_list``,
src/utils/get_data_loaders.py:130-145) and then copies the batch to the device (src/run_gsat.py:654).  Here the whole
dataset is packed once into HBM (molhiv: 41 k graphs ~ 1 M nodes ~ 70 MB) and a batch is assembled by two small
kernels from a list of graph ids: no host work, no PCIe traffic per step.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from ._lib import call, ptr, stream
from .synth import Batch


class PaddedBatch(Batch):
    """A batch of fixed capacity (``PackedDataset.collate_padded``): the ``B`` real graphs first, then one padding graph ``B`` that holds
    the unused node rows and edge slots, so ``num_graphs = B + 1``.  Besides the fields of ``collate``'s batch it carries ``valid``
    (int32[4] on the device: N_real, E_real, B, overflow), ``capacity = (N_cap, E_cap)``, ``node_src_row`` / ``edge_src_slot`` (the
    dataset row / slot of every node / edge, -1 for padding) and optionally ``r`` (one device float: the info loss's r) and ``pair`` (the
    other batch of a ``collate_padded_pair``).  A ``ragged`` batch (``collate_padded(..., ragged=True)``) has ``B`` graph slots of which only
    the first ``valid[2]`` are filled."""


def _take_padded(table, index):
    """table[index] with zero rows where index is -1.  A table without rows (a batch without edges) gives zero rows only: there every
    index is -1, and the clamped gather would read row 0 of nothing."""
    if table is None:
        return None
    if int(table.shape[0]) == 0:
        return table.new_zeros((int(index.shape[0]),) + tuple(table.shape[1:]))
    out = table.index_select(0, index.clamp(min=0))
    return out.masked_fill_((index < 0).view((-1,) + (1,) * (out.dim() - 1)), 0)


class PackedDataset:
    def __init__(self, x_all, edge_index_local_all, node_ptr_all, edge_ptr_all, y_all, edge_attr_all=None, edge_label_all=None):
        self.x_all, self.edge_local_all = x_all.contiguous(), edge_index_local_all.contiguous()
        self.node_ptr_all, self.edge_ptr_all = node_ptr_all.contiguous(), edge_ptr_all.contiguous()
        self.y_all, self.edge_attr_all, self.edge_label_all = y_all, edge_attr_all, edge_label_all
        self.num_graphs = int(node_ptr_all.shape[0]) - 1
        self.node_counts = self.node_ptr_all[1:] - self.node_ptr_all[:-1]
        self.edge_counts = self.edge_ptr_all[1:] - self.edge_ptr_all[:-1]
        self._capacities = {}
        self._host_counts = None

    @classmethod
    def from_data_list(cls, graphs: Sequence, device) -> "PackedDataset":
        """graphs: objects with .x, .edge_index (local ids), .y and optionally .edge_attr / .edge_label (one-off, host side)."""
        n = torch.tensor([g.x.shape[0] for g in graphs], dtype=torch.int64)
        e = torch.tensor([g.edge_index.shape[1] for g in graphs], dtype=torch.int64)
        zero = torch.zeros(1, dtype=torch.int64)
        cat = lambda name: torch.cat([getattr(g, name) for g in graphs], dim=0).to(device) if getattr(graphs[0], name, None) is not None else None
        return cls(cat("x"), torch.cat([g.edge_index for g in graphs], dim=1).to(device), torch.cat([zero, n.cumsum(0)]).to(device),
                   torch.cat([zero, e.cumsum(0)]).to(device), cat("y"), cat("edge_attr"), cat("edge_label"))

    def collate(self, graph_ids: torch.Tensor, sizes: Optional[tuple] = None) -> Batch:
        """Batch of the graphs ``graph_ids`` (int64, on the device, any order).  ``sizes=(N, E)`` skips the one host sync
        that reads the batch's node / edge totals."""
        ids = graph_ids.to(self.x_all.device, torch.int64).contiguous()
        G = int(ids.shape[0])
        dev = ids.device
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        out_node_ptr = torch.cat([zero, self.node_counts[ids].cumsum(0)])
        out_edge_ptr = torch.cat([zero, self.edge_counts[ids].cumsum(0)])
        if sizes is None:
            N, E = (int(v) for v in torch.stack([out_node_ptr[-1], out_edge_ptr[-1]]).tolist())
        else:
            N, E = sizes
        batch = torch.empty(N, dtype=torch.int64, device=dev)
        node_src = torch.empty(N, dtype=torch.int64, device=dev)
        edge_index = torch.empty(2, E, dtype=torch.int64, device=dev)
        edge_src = torch.empty(E, dtype=torch.int64, device=dev)
        call("gsat_collate", ptr(ids), G, ptr(self.node_ptr_all), ptr(self.edge_ptr_all), ptr(self.edge_local_all),
             int(self.edge_local_all.shape[1]), ptr(out_node_ptr), ptr(out_edge_ptr), N, E, ptr(batch), ptr(node_src),
             ptr(edge_index), ptr(edge_src), stream())
        take = lambda t, idx: None if t is None else t.index_select(0, idx)
        return Batch(x=self.x_all.index_select(0, node_src), edge_index=edge_index, batch=batch, y=take(self.y_all, ids),
                     edge_attr=take(self.edge_attr_all, edge_src), edge_label=take(self.edge_label_all, edge_src), num_graphs=G)


    def capacity_for(self, batch_size: int) -> tuple:
        """(N_cap, E_cap) that no batch of ``batch_size`` distinct graphs exceeds: the sums of the ``batch_size`` largest node counts
        (+ 2 padding nodes) and edge counts.  One host read the first time a batch size is asked for."""
        k = min(int(batch_size), self.num_graphs)
        if k < 1:
            raise ValueError("capacity_for needs a batch of at least one graph")
        if k not in self._capacities:
            n, e = torch.stack([self.node_counts.topk(k).values.sum(), self.edge_counts.topk(k).values.sum()]).tolist()
            self._capacities[k] = (int(n) + 2, int(e))
        return self._capacities[k]

    def budget_batches(self, perm, capacity: tuple, max_graphs: int, dual: Optional["PackedDataset"] = None) -> torch.Tensor:
        """The graphs ``perm`` (ids in visiting order) packed into batches of a node / edge budget, PyG's ``DynamicBatchSampler``: int64
        [num_batches, max_graphs] on the device, one row per batch -- ``collate_padded(row, capacity, ragged=True)`` -- with -1 in the
        unused slots.  In ``perm``'s order a graph opens a new batch when adding it would break ``nodes + 2 <= N_cap``, ``edges <=
        E_cap`` or ``count <= max_graphs``: every batch fits, the order is kept and no batch could have taken its successor's first
        graph.  A graph that fits no batch alone raises ValueError.

        Host work: two cumulative sums over ``perm`` and three searches per batch, on a host copy of the graphs' sizes that is made the
        first time (this dataset's only host read here).

        ``dual`` (this dataset's dual, ``check_pair`` runs first): the rows for ``collate_padded_pair(self, dual, row, capacity,
        ragged=True)``.  ``capacity`` is then ``(N_cap, E_cap, E_dual_cap)`` and ``dual_edges <= E_dual_cap`` is a third budget: a third
        cumulative sum and a fourth search per batch, on a host copy of the dual's edge counts that is made once."""
        if dual is not None:
            self.check_pair(dual)
            if len(capacity) != 3:
                raise ValueError("budget_batches: with a dual the capacity is (N_cap, E_cap, E_dual_cap)")
        N_cap, E_cap, slots = int(capacity[0]), int(capacity[1]), int(max_graphs)
        if slots < 1:
            raise ValueError("budget_batches needs at least one graph slot per batch")
        if self._host_counts is None:
            both = torch.stack([self.node_counts, self.edge_counts]).cpu().numpy()
            self._host_counts = (both[0].copy(), both[1].copy())
        if dual is not None and dual._host_counts is None:
            both = torch.stack([dual.node_counts, dual.edge_counts]).cpu().numpy()
            dual._host_counts = (both[0].copy(), both[1].copy())
        import numpy as np
        p = torch.as_tensor(perm).reshape(-1).cpu().numpy().astype(np.int64)
        if p.size and (p.min() < 0 or p.max() >= self.num_graphs):
            raise ValueError("budget_batches: graph ids must lie in [0, num_graphs)")
        # (running totals over perm, budget) of every size a batch is limited in
        sums = [(self._host_counts[0], N_cap - 2), (self._host_counts[1], E_cap)]
        if dual is not None:
            sums.append((dual._host_counts[1], int(capacity[2])))
        sums = [(np.concatenate([[0], np.cumsum(c[p])]), room) for c, room in sums]
        starts, s, n = [], 0, int(p.size)
        while s < n:
            # the first position whose running total exceeds the budget ends the batch (side="right": equality still fits)
            end = min([int(np.searchsorted(c, c[s] + room, side="right")) - 1 for c, room in sums] + [s + slots, n])
            if end <= s:
                g = int(p[s])
                size = f"{int(self._host_counts[0][g])} nodes + 2 padding nodes, {int(self._host_counts[1][g])} edges"
                if dual is None:
                    raise ValueError(f"budget_batches: graph {g} ({size}) does not fit the capacity (N_cap, E_cap) = ({N_cap}, {E_cap})")
                raise ValueError(f"budget_batches: graph {g} ({size}, {int(dual._host_counts[1][g])} dual edges) does not fit the capacity "
                                 f"(N_cap, E_cap, E_dual_cap) = ({N_cap}, {E_cap}, {int(capacity[2])})")
            starts.append(s)
            s = end
        starts = np.asarray(starts + [n], dtype=np.int64)
        out = np.full((len(starts) - 1, slots), -1, dtype=np.int64)
        if n:
            length = np.diff(starts)
            row = np.repeat(np.arange(len(length)), length)
            out[row, np.arange(n) - starts[row]] = p
        return torch.from_numpy(out).to(self.x_all.device)

    def pair_capacity_for(self, dual: "PackedDataset", batch_size: int) -> tuple:
        """(N_cap, E_cap, E_dual_cap) of ``collate_padded_pair`` that no batch of ``batch_size`` distinct graphs exceeds: ``capacity_for`` of
        this (primal) dataset and the sum of the ``batch_size`` largest dual edge counts.  The dual node capacity is always E_cap + 2."""
        n, e = self.capacity_for(batch_size)
        return (n, e, dual.capacity_for(batch_size)[1])

    def check_pair(self, dual: "PackedDataset") -> None:
        """Raise ValueError unless ``dual`` has one node per edge of this dataset, graph by graph (one host read; remembered)."""
        if getattr(dual, "_primal", None) is self:
            return
        if dual.num_graphs != self.num_graphs or not bool(torch.equal(dual.node_counts, self.edge_counts.to(dual.node_counts.device))):
            raise ValueError("not a dual of this dataset: its graphs' node counts must be this dataset's edge counts "
                             "(PackedDataset.line_graph_dataset builds one)")
        dual._primal = self

    def line_graph_dataset(self, dual_x: Optional[torch.Tensor] = None) -> "PackedDataset":
        """The dual dataset: graph g is the directed line graph (``line_graph``'s rule) of graph g; its node k is primal edge k of graph g,
        so ``node_counts`` are this dataset's ``edge_counts`` and ``collate_padded_pair`` lines primal edge slots up with dual node rows.
        Dual edges carry ids local to their graph, ``y`` is shared.  ``dual_x`` [E_all, F]: dual node features; default [x[src] || x[dst]]
        (float ``x`` only).  Built by ONE line-graph pass over the whole packed dataset and one host read (the dual's size)."""
        from .graph_index import BatchIndex
        dev = self.x_all.device
        G, N_all, E_all = self.num_graphs, int(self.x_all.shape[0]), int(self.edge_local_all.shape[1])
        edge_graph = torch.repeat_interleave(torch.arange(G, device=dev), self.edge_counts, output_size=E_all)
        ei = (self.edge_local_all + self.node_ptr_all[edge_graph]).contiguous()                 # global node ids
        ix = BatchIndex(ei, N_all)                  # local: the index of a whole dataset has no place in the per-batch cache
        counts = torch.empty(N_all, dtype=torch.int64, device=dev)
        call("gsat_line_graph_pair_counts", ptr(ix.rowptr_src), N_all, ptr(counts), stream())
        pair_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), counts.cumsum(0)])
        num_pairs, fewest = torch.stack([pair_ptr[-1], self.edge_counts.min() if G else pair_ptr[-1] + 1]).tolist()
        if G and fewest == 0:
            raise ValueError("a graph without edges has an empty line graph: drop it before building the dual dataset")
        dual_ei = torch.empty(2, 2 * num_pairs, dtype=torch.int64, device=dev)
        call("gsat_line_graph", ptr(ix.rowptr_src), ptr(ix.eid_by_src), ptr(pair_ptr), N_all, num_pairs, ptr(dual_ei), stream())
        # dual edges come out by source node, hence graph by graph: graph g owns the pairs of its nodes
        dual_edge_ptr = 2 * pair_ptr[self.node_ptr_all]
        dual_local = dual_ei - self.edge_ptr_all[edge_graph[dual_ei[0]]]
        if dual_x is None:
            if not self.x_all.is_floating_point():
                raise ValueError("line_graph_dataset: pass dual_x for a dataset with categorical node features")
            dual_x = torch.cat([self.x_all[ei[0]], self.x_all[ei[1]]], dim=1)
        elif int(dual_x.shape[0]) != E_all:
            raise ValueError("dual_x needs one row per primal edge")
        dual = PackedDataset(dual_x.to(dev), dual_local, self.edge_ptr_all, dual_edge_ptr, self.y_all)
        dual._primal = self
        return dual

    def collate_padded(self, graph_ids: torch.Tensor, capacity: tuple, ragged: bool = False) -> PaddedBatch:
        """``collate(graph_ids)`` into tensors of the fixed shape ``capacity = (N_cap, E_cap)``: rows < N_real, slots < E_real and graphs
        < B are bit-identical to ``collate``; the remaining rows are zero-feature nodes of a padding graph ``B`` and the remaining slots
        a symmetric edge set among them (include/gsat_hip.h: gsat_collate_padded).  At least two padding nodes always remain.  A batch
        that does not fit raises ValueError -- in sync-free mode nothing is read back: ``valid[3]`` is set and the batch is all padding.
        No host decision is taken, so the call can be captured into a hipGraph; run the model on the result through
        ``GSAT.forward_pass`` or inside ``dp_gsat_amd.padded(batch.valid, batch.capacity)``.

        ``ragged=True``: ``graph_ids`` are ``B`` graph SLOTS and a negative id is an empty one; empty slots must be trailing.  The batch
        still has ``num_graphs = B + 1`` (the padding graph is graph ``B``); the graphs of the empty slots have no node and no edge and a
        zero ``y`` row, and ``valid[2]`` is the number of filled slots, counted on the device, so that one captured step takes any
        number of graphs up to ``B`` (``GSAT.forward_pass`` hands it to the criterion).  A filled slot after an empty one makes the batch
        an overflow like one that does not fit, and so does an id that is not below the dataset's graph count: everything is padding and
        ``valid == (0, 0, 0, 1)``.  The batch carries ``ragged = True``."""
        return self._collate_padded(graph_ids, capacity, ragged=bool(ragged))

    def _collate_padded(self, graph_ids, capacity, spoil=None, check=True, ragged=False, scan=None) -> PaddedBatch:
        """``collate_padded``; ``spoil`` (a 0-dim bool on the device) makes the batch an overflow whatever its size -- the joint verdict of a
        fixed-count pair: the node total handed to the kernel is raised by the capacity, which fails its ``N + 2 <= N_cap`` test, and an
        overflow batch reads neither scan.  ``check=False`` leaves the host read of the overflow word to the caller.  ``scan`` (ragged
        only): ``(out_node_ptr, out_edge_ptr, state, safe_ids, empty)`` made by the caller -- ``gsat_ragged_pair_scan``'s, whose state
        carries the joint verdict of a ragged pair -- in place of this batch's own ``gsat_ragged_scan``."""
        from .graph_index import sync_free
        ids = graph_ids.to(self.x_all.device, torch.int64).contiguous()
        B, dev = int(ids.shape[0]), ids.device
        N_cap, E_cap = int(capacity[0]), int(capacity[1])
        if B < 1 or N_cap < 2 or E_cap < 0:
            raise ValueError("collate_padded needs at least one graph and a capacity of at least two nodes")
        state = empty = None
        if ragged:
            # one launch: both scans with the empty slots counting nothing (the collation kernel gives them no row and never looks their
            # id up), the number of filled slots, and whether a filled slot sits behind an empty one -- the verdict stays on the device
            if spoil is not None:
                raise ValueError("a ragged batch takes no torch-made overflow verdict (a ragged pair's is in its scan's state)")
            if scan is not None:
                out_node_ptr, out_edge_ptr, state, safe, empty = scan
            else:
                out_node_ptr, out_edge_ptr = (torch.empty(B + 1, dtype=torch.int64, device=dev) for _ in range(2))
                state, safe = torch.empty(2, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
                empty = torch.empty(B, dtype=torch.bool, device=dev)
                call("gsat_ragged_scan", ptr(ids), B, ptr(self.node_ptr_all), ptr(self.edge_ptr_all), self.num_graphs, ptr(out_node_ptr),
                     ptr(out_edge_ptr), ptr(state), ptr(safe), ptr(empty), stream())
            ids = safe
        else:
            zero = torch.zeros(1, dtype=torch.int64, device=dev)
            out_node_ptr = torch.cat([zero, self.node_counts[ids].cumsum(0)])
            out_edge_ptr = torch.cat([zero, self.edge_counts[ids].cumsum(0)])
        if spoil is not None:
            out_node_ptr[B] += spoil.to(torch.int64) * N_cap
        batch = torch.empty(N_cap, dtype=torch.int64, device=dev)
        node_src = torch.empty(N_cap, dtype=torch.int64, device=dev)
        edge_index = torch.empty(2, E_cap, dtype=torch.int64, device=dev)
        edge_src = torch.empty(E_cap, dtype=torch.int64, device=dev)
        valid = torch.empty(4, dtype=torch.int32, device=dev)
        tail = (ptr(self.node_ptr_all), ptr(self.edge_ptr_all), ptr(self.edge_local_all), int(self.edge_local_all.shape[1]), ptr(out_node_ptr),
                ptr(out_edge_ptr), N_cap, E_cap, ptr(batch), ptr(node_src), ptr(edge_index) if E_cap else None,
                ptr(edge_src) if E_cap else None, ptr(valid), stream())
        if ragged:
            call("gsat_collate_padded_ragged", ptr(ids), B, ptr(state), *tail)
        else:
            call("gsat_collate_padded", ptr(ids), B, *tail)
        if check and not sync_free():
            n, e, _, overflow = valid.tolist()           # the one host read, where collate reads its sizes
            if overflow:
                raise ValueError(f"collate_padded: the batch does not fit the capacity (N_cap, E_cap) = ({N_cap}, {E_cap}) "
                                 "(two padding nodes must remain)")
        y = None
        if self.y_all is not None:
            rows = self.y_all.index_select(0, ids)
            if ragged:
                rows.masked_fill_(empty.view((-1,) + (1,) * (rows.dim() - 1)), 0)
            y = torch.cat([rows, self.y_all.new_zeros((1,) + tuple(self.y_all.shape[1:]))])
        extra = dict(ragged=True) if ragged else {}
        return PaddedBatch(x=_take_padded(self.x_all, node_src), edge_index=edge_index, batch=batch, y=y,
                           edge_attr=_take_padded(self.edge_attr_all, edge_src), edge_label=_take_padded(self.edge_label_all, edge_src),
                           num_graphs=B + 1, valid=valid, capacity=(N_cap, E_cap), node_src_row=node_src, edge_src_slot=edge_src, **extra)


def collate_padded_pair(primal: PackedDataset, dual: PackedDataset, graph_ids: torch.Tensor, capacity: Optional[tuple] = None,
                        ragged: bool = False):
    """``(pb, db)``: the graphs ``graph_ids`` of a dataset and of its dual (``primal.line_graph_dataset()``) as fixed-capacity batches that
    line up -- ``pb = primal.collate_padded(ids, (N_cap, E_cap))`` and ``db = dual.collate_padded(ids, (E_cap + 2, E_dual_cap))``, so dual
    node row k < E_cap is primal edge slot k (the + 2: the padding nodes every padded batch keeps).  ``capacity = (N_cap, E_cap,
    E_dual_cap)`` defaults to ``primal.pair_capacity_for(dual, len(graph_ids))``.  ``pb.pair is db`` and ``db.pair is pb``:
    ``DualGSAT.dual_forward_pass`` takes padded batches only as such a pair.

    Overflow is joint and decided on the device: if either batch does not fit, BOTH are all padding with ``valid[3] == 1`` (ValueError
    outside sync-free mode, after one host read).

    ``ragged=True``: ``graph_ids`` are ``B`` graph slots with the empty ones (negative ids) trailing, as in ``collate_padded(...,
    ragged=True)``; both batches carry ``ragged = True``, ``num_graphs = B + 1`` and zero ``y`` rows in the empty slots, and ``pb.valid ==
    (N, E, b, 0)``, ``db.valid == (E, E_dual, b, 0)`` with ``b`` the filled slots, counted on the device.  ONE launch
    (``gsat_ragged_pair_scan``) makes the three scans and the joint verdict -- a budget exceeded, a filled slot behind an empty one, an id
    that is not below the dataset's graph count -- and both collations read it: an overflow pair is all padding with ``valid == (0, 0,
    0, 1)`` on both sides.  Nothing depends on the batch from the host."""
    from .graph_index import sync_free
    primal.check_pair(dual)
    ids = torch.as_tensor(graph_ids).to(primal.x_all.device, torch.int64).contiguous()
    if capacity is None:
        capacity = primal.pair_capacity_for(dual, int(ids.shape[0]))
    N_cap, E_cap, Ed_cap = (int(c) for c in capacity)
    if ragged:
        B, dev = int(ids.shape[0]), ids.device
        if B < 1:
            raise ValueError("collate_padded_pair needs at least one graph slot")
        node_ptr, edge_ptr, dual_edge_ptr = (torch.empty(B + 1, dtype=torch.int64, device=dev) for _ in range(3))
        state, safe = torch.empty(2, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
        empty = torch.empty(B, dtype=torch.bool, device=dev)
        call("gsat_ragged_pair_scan", ptr(ids), B, ptr(primal.node_ptr_all), ptr(primal.edge_ptr_all), ptr(dual.edge_ptr_all),
             primal.num_graphs, N_cap, E_cap, Ed_cap, ptr(node_ptr), ptr(edge_ptr), ptr(dual_edge_ptr), ptr(state), ptr(safe), ptr(empty),
             stream())
        pb = primal._collate_padded(ids, (N_cap, E_cap), check=False, ragged=True, scan=(node_ptr, edge_ptr, state, safe, empty))
        db = dual._collate_padded(ids, (E_cap + 2, Ed_cap), check=False, ragged=True, scan=(edge_ptr, dual_edge_ptr, state, safe, empty))
    else:
        n, e, ed = primal.node_counts[ids].sum(), primal.edge_counts[ids].sum(), dual.edge_counts[ids].sum()
        spoil = (n + 2 > N_cap) | (e > E_cap) | (ed > Ed_cap)
        pb = primal._collate_padded(ids, (N_cap, E_cap), spoil, check=False)
        db = dual._collate_padded(ids, (E_cap + 2, Ed_cap), spoil, check=False)
    pb.pair, db.pair = db, pb
    if not sync_free() and int(pb.valid[3]):
        raise ValueError(f"collate_padded_pair: the batch does not fit the capacity (N_cap, E_cap, E_dual_cap) = ({N_cap}, {E_cap}, {Ed_cap}) "
                         "(two padding nodes must remain)")
    return pb, db


def line_graph(edge_index: torch.Tensor, num_nodes: int, batch: Optional[torch.Tensor] = None):
    """Dual graph of the fork on the device: returns (dual_edge_index int64[2, E_d], dual_batch int64[E] or None).
    Dual node k is primal directed edge k (so primal edge attention and dual node attention align, src/run_gsat.py:253);
    dual edges join primal edges leaving the same node (src/datasets/mutag_dual.py:345-377)."""
    from .graph_index import get_index
    ix = get_index(edge_index, num_nodes)
    dev = edge_index.device
    counts = torch.empty(num_nodes, dtype=torch.int64, device=dev)
    call("gsat_line_graph_pair_counts", ptr(ix.rowptr_src), num_nodes, ptr(counts), stream())
    pair_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), counts.cumsum(0)])
    num_pairs = int(pair_ptr[-1].item())
    dual_ei = torch.empty(2, 2 * num_pairs, dtype=torch.int64, device=dev)
    call("gsat_line_graph", ptr(ix.rowptr_src), ptr(ix.eid_by_src), ptr(pair_ptr), num_nodes, num_pairs, ptr(dual_ei), stream())
    dual_batch = None if batch is None else batch[edge_index[0]]
    return dual_ei, dual_batch


def line_graph_undirected(edge_index: torch.Tensor, num_nodes: int, batch: Optional[torch.Tensor] = None,
                          x: Optional[torch.Tensor] = None, motif_start: Optional[int] = None):
    """Dual graph with one node per UNDIRECTED primal edge, on the device -- the rule of the fork's ba_2motifs dual dataset
    (src/datasets/ba_2motifs_dual.py:35-62): edges numbered by (smaller, larger) endpoint in row-major order, dual nodes
    adjacent when the primal edges share an endpoint, dual edge list in (i, j) row-major order.

    Returns a ``Batch`` with ``edge_index`` (dual, int64 [2, E_d]), ``und_index`` (int64 [2, M]: endpoints a < b of every dual
    node), ``und_of_edge`` (int64 [E]: dual node of every primal directed edge, -1 for self loops), and when the inputs are
    given: ``batch`` (graph of every dual node), ``x`` = [x[a] || x[b]] (:48) and ``node_label`` = 1 iff both endpoints have
    local id >= ``motif_start`` (:46-47, 20 for BA-2motifs).  Raises ValueError if some edge has no reverse."""
    from .graph_index import call_size
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
        raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
    ei = edge_index.contiguous()
    dev, E, N = ei.device, int(ei.shape[1]), int(num_nodes)
    i32 = lambda n: torch.empty(max(int(n), 1), dtype=torch.int32, device=dev)
    keys = torch.empty(max(E, 1), dtype=torch.int64, device=dev)          # uint64 keys: same bytes
    rowptr, und_of_slot, und_of_edge, und_src, und_dst = i32(N + 1), i32(E), i32(E), i32(E), i32(E)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    wb = max(call_size("gsat_und_edges_workspace_bytes", E), 256)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    call("gsat_und_edges", ptr(ei), E, N, ptr(keys), ptr(rowptr), ptr(und_of_slot), ptr(und_of_edge), ptr(und_src), ptr(und_dst),
         ptr(status), ptr(ws), wb, stream())
    M, asym, bad = status[:3].tolist()
    if bad:
        raise ValueError("edge_index contains node ids outside [0, num_nodes)")
    if asym:
        raise ValueError("line_graph_undirected needs a symmetric edge set: %d directed edges have no reverse" % asym)
    counts = torch.zeros(M, dtype=torch.int64, device=dev)
    call("gsat_und_line_graph_counts", ptr(rowptr), ptr(und_of_slot), ptr(und_src), ptr(und_dst), M, ptr(counts), stream())
    dual_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), counts.cumsum(0)])
    total = int(dual_ptr[-1].item())
    dual_ei = torch.empty(2, total, dtype=torch.int64, device=dev)
    call("gsat_und_line_graph", ptr(rowptr), ptr(und_of_slot), ptr(und_src), ptr(und_dst), ptr(dual_ptr), M, total, ptr(dual_ei), stream())
    a, b = und_src[:M].long(), und_dst[:M].long()
    out = Batch(edge_index=dual_ei, und_index=torch.stack([a, b]), und_of_edge=und_of_edge[:E].long(), batch=None, x=None,
                node_label=None, edge_attr=None, num_dual_nodes=M)
    if batch is not None:
        out.batch = batch[a]
    if x is not None:
        out.x = torch.cat([x[a], x[b]], dim=1)
    if motif_start is not None:
        if batch is None:
            raise ValueError("motif labels need the batch vector (local node ids)")
        G = int(batch.max().item()) + 1 if batch.numel() else 0
        node_ptr = torch.zeros(G + 1, dtype=torch.int64, device=dev)
        node_ptr[1:] = torch.bincount(batch, minlength=G).cumsum(0)
        la, lb = a - node_ptr[batch[a]], b - node_ptr[batch[b]]
        out.node_label = ((la >= motif_start) & (lb >= motif_start)).float()
    return out
