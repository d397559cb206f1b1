"""A training step over a real dataset as replays of ONE captured hipGraph.

A captured step bakes N, E and G into every launch, and real batches differ in N and E from step to step.  ``ReplayedStep`` collates
every batch to a fixed capacity (PackedDataset.collate_padded) inside the captured graph, so that a step is: copy the graph ids, set
r, replay.  The padding is arithmetically inert.
"""
from __future__ import annotations

from typing import Optional

import torch

from .graph_index import clear_cache, set_sync_free, sync_free
from .gsat import get_r
from .ops import edge_tensor


class ReplayedStep:
    """``ReplayedStep(gsat, dataset, batch_size, capacity=None)``: captures clear_cache, collate_padded, forward_pass,
    zero_grad(set_to_none=True), backward and optimizer.step() of ``gsat`` on ``dataset`` (a PackedDataset) once, after three warm-up
    runs on a side stream.  ``gsat.optimizer`` must be capturable (``torch.optim.Adam(..., capturable=True)``).  The warm-up runs
    train on graphs 0 .. batch_size-1; parameters, buffers and optimizer state are put back afterwards, so capturing does not train.

    ``capacity`` defaults to ``dataset.capacity_for(batch_size)``, which no batch of distinct graphs exceeds; with a tighter one,
    ``check_epoch`` tells (one host read) whether an epoch's batches fit.  A tail batch of fewer than ``batch_size`` graphs is the
    caller's to run eagerly with ``dataset.collate``.

    A batch that does not fit the capacity is NOT skipped: the kernel turns it into an all-padding batch and the replay still runs,
    which pulls the BatchNorm running statistics towards 0 and takes an optimizer step on the gradients of empty graphs.  Nothing is
    read back per step, so the overflow word of every replay is OR-ed into one device flag: ``overflowed()`` (one host read, e.g. once
    per epoch) tells whether any step since the last call overflowed.  ``check_epoch`` before the epoch avoids it altogether.

    After a step: ``loss`` (device scalar), ``clf_logits`` [B + 1, C], ``batch`` (the PaddedBatch, ``batch.valid`` holds the counts) and,
    with ``keep_edge_att=True``, ``edge_att`` [E_cap, 1] -- all of capacity shape and overwritten by the next replay.
    ``graph``: an own ``torch.cuda.CUDAGraph`` to capture into (one with debug mode on, to dump it)."""

    def __init__(self, gsat, dataset, batch_size: int, capacity: Optional[tuple] = None, keep_edge_att: bool = False, graph=None):
        opt = gsat.optimizer
        if opt is None or not all(g.get("capturable", False) for g in opt.param_groups):
            raise ValueError("ReplayedStep needs a capturable optimizer, e.g. torch.optim.Adam(params, capturable=True, fused=True)")
        if getattr(gsat.criterion, "multi_label", False):
            raise ValueError("a padded batch cannot take the multi-label criterion (its boolean indexing is not capturable)")
        self.gsat, self.dataset, self.batch_size = gsat, dataset, int(batch_size)
        if not 1 <= self.batch_size <= dataset.num_graphs:
            raise ValueError("batch_size must be between 1 and the dataset's graph count")
        self.capacity = tuple(int(c) for c in capacity) if capacity is not None else dataset.capacity_for(self.batch_size)
        dev = dataset.x_all.device
        self.graph_ids = torch.arange(self.batch_size, dtype=torch.int64, device=dev)
        self.r = torch.full((1,), float(self._r_of(0)), dtype=torch.float32, device=dev)
        self.keep_edge_att = bool(keep_edge_att)
        self.batch = self.loss = self.clf_logits = self.edge_att = None
        self._overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        self.graph = graph if graph is not None else torch.cuda.CUDAGraph()
        self._capture()

    def _r_of(self, epoch):
        g = self.gsat
        return get_r(g.decay_interval, g.decay_r, epoch, final_r=g.final_r)

    def run_once(self):
        """The step body (what the graph holds), run on the current stream."""
        gsat = self.gsat
        clear_cache()
        b = self.dataset.collate_padded(self.graph_ids, self.capacity)
        b.r = self.r
        self._overflow.bitwise_or_(b.valid[3:4])
        att, loss, _, logits = gsat.forward_pass(b, 0, True)
        gsat.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        gsat.optimizer.step()
        self.batch, self.loss, self.clf_logits = b, loss.detach(), logits.detach()
        if self.keep_edge_att:
            self.edge_att = edge_tensor(att).detach()

    def _capture(self):
        gsat, opt = self.gsat, self.gsat.optimizer
        tensors = [t for t in list(gsat.parameters()) + list(gsat.buffers())]
        saved = [t.detach().clone() for t in tensors]
        had_state = {id(p): {k: v.clone() for k, v in opt.state[p].items() if isinstance(v, torch.Tensor)}
                     for grp in opt.param_groups for p in grp["params"] if p in opt.state}
        was_sync_free, was_loss_dict = sync_free(), gsat.sync_loss_dict
        set_sync_free(True)
        gsat.sync_loss_dict = False
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    self.run_once()
            torch.cuda.current_stream().wait_stream(side)
            if int(self.batch.valid[3]) != 0:
                raise ValueError(f"ReplayedStep: graphs 0..{self.batch_size - 1} do not fit the capacity {self.capacity}")
            with torch.cuda.graph(self.graph):
                self.run_once()
        finally:
            set_sync_free(was_sync_free)
            gsat.sync_loss_dict = was_loss_dict
            clear_cache()
            with torch.no_grad():          # also when capturing failed; in place: the graph holds these addresses
                for t, s in zip(tensors, saved):
                    t.copy_(s)
                for grp in opt.param_groups:
                    for p in grp["params"]:
                        for k, v in opt.state.get(p, {}).items():
                            if isinstance(v, torch.Tensor):
                                old = had_state.get(id(p), {}).get(k)
                                v.copy_(old) if old is not None else v.zero_()
                self._overflow.zero_()

    def step(self, graph_ids, epoch: int) -> torch.Tensor:
        """One training step on the graphs ``graph_ids`` (exactly ``batch_size`` ids; tensor, array or list) with r = get_r(epoch).
        Returns the device loss; nothing is read back."""
        ids = torch.as_tensor(graph_ids)
        if ids.numel() != self.batch_size:
            raise ValueError(f"ReplayedStep was captured for {self.batch_size} graphs per step, got {ids.numel()}")
        self.graph_ids.copy_(ids.reshape(-1), non_blocking=True)
        self.r.fill_(float(self._r_of(epoch)))
        self.graph.replay()
        return self.loss

    def overflowed(self) -> bool:
        """True if a step since the last call (or since capture) got a batch that did not fit the capacity.  One host read; clears
        the flag."""
        seen = bool(int(self._overflow))
        self._overflow.zero_()
        return seen

    def check_epoch(self, perm) -> None:
        """Raise ValueError if a full batch of the epoch ``perm`` (graph ids in visiting order) exceeds the capacity: the (N, E) totals of
        every ``perm[k * batch_size : (k + 1) * batch_size]`` are taken on the device and read back once."""
        ds, B = self.dataset, self.batch_size
        p = torch.as_tensor(perm).to(ds.x_all.device, torch.int64).reshape(-1)
        full = int(p.numel()) // B
        if full == 0:
            return
        p = p[: full * B].view(full, B)
        n, e = torch.stack([ds.node_counts[p].sum(1).max(), ds.edge_counts[p].sum(1).max()]).tolist()
        if n + 2 > self.capacity[0] or e > self.capacity[1]:
            raise ValueError(f"a batch of this epoch needs (N, E) = ({n} + 2 padding nodes, {e}), above the capacity {self.capacity}")
