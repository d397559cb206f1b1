"""Restatements for the ragged-batch tests: the budget batching rule in numpy (one Python step per graph: the thing
PackedDataset.budget_batches must not do) and the three criterion modes of gsat_criterion_* in fp64 over the first b rows."""
import numpy as np
import torch

# the cases the host and the GPU tests share: po.mutag_graphs(**po.STEP_GRAPHS), 16 slots
RAGGED_SLOTS = 16
RAGGED_CAPACITY = (300, 620)
RAGGED_SIZES = [7, 10, 10, 6, 9, 6]
TIGHT_CAPACITY = (260, 540)
TIGHT_SIZES = [7, 9, 10, 3, 10, 6, 3]


def budget_batches(node_counts, edge_counts, perm, capacity, max_graphs):
    """Lists of graph ids: in ``perm``'s order a graph opens a new batch when adding it would break nodes + 2 <= N_cap, edges <= E_cap or
    count <= max_graphs."""
    out, cur, n, e = [], [], 0, 0
    for g in perm:
        gn, ge = int(node_counts[g]), int(edge_counts[g])
        if gn + 2 > capacity[0] or ge > capacity[1]:
            raise ValueError(f"graph {g} fits no batch")
        if cur and (n + gn + 2 > capacity[0] or e + ge > capacity[1] or len(cur) + 1 > max_graphs):
            out.append(cur)
            cur, n, e = [], 0, 0
        cur.append(int(g))
        n, e = n + gn, e + ge
    return out + [cur] if cur else out


def rows_to_lists(rows):
    """The [num_batches, max_graphs] tensor of budget_batches as lists of ids; asserts that the -1 slots are trailing."""
    out = []
    for row in np.asarray(rows.cpu()).tolist():
        k = sum(1 for v in row if v >= 0)
        assert all(v >= 0 for v in row[:k]) and all(v == -1 for v in row[k:]), row
        out.append(row[:k])
    return out


def criterion64(logits, target, mode, b=None):
    """fp64 loss of gsat_criterion_fwd over the rows < b (None: all), differentiable in ``logits``: mode 0 mean of max(z, 0) - z y +
    log1p(exp(-|z|)); mode 1 mean over rows of logsumexp(z) - z[y]; mode 2 mode 0's term over the non-NaN targets.  An empty selection
    gives 0 (the divisor is clamped to 1)."""
    G = logits.shape[0]
    b = G if b is None else min(max(int(b), 0), G)
    z = logits[:b].double()
    t = target[:b].double()
    if mode == 1:
        if b == 0:
            return z.sum() * 0.0
        m = z.max(dim=1, keepdim=True).values.detach()
        lse = (z - m).exp().sum(1).log() + m[:, 0]
        return (lse - z.gather(1, t.long().view(-1, 1))[:, 0]).sum() / b
    t = t.reshape(z.shape)
    keep = ~torch.isnan(t) if mode == 2 else torch.ones_like(t, dtype=torch.bool)
    term = z.clamp(min=0) - z * torch.where(keep, t, torch.zeros_like(t)) + torch.log1p(torch.exp(-z.abs()))
    return torch.where(keep, term, torch.zeros_like(term)).sum() / max(int(keep.sum()), 1)


def criterion_case(G, C, mode, seed):
    """fp32 (logits [G, C], target) of a criterion test: logits N(0, 2) with a few entries at +-100 (a naive log(1 + exp(z)) overflows
    there); mode 0 / 2 targets in {0, 1}, mode 2 with about 30 % NaN, an all-NaN column (C > 1) and an all-NaN row; mode 1 class indices."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(G, C, generator=g) * 2.0
    flat = z.view(-1)
    flat[::7] = 100.0
    flat[3::11] = -100.0
    if mode == 1:
        return z, torch.randint(0, C, (G,), generator=g).float()
    y = (torch.rand(G, C, generator=g) < 0.5).float()
    if mode == 2:
        y[torch.rand(G, C, generator=g) < 0.3] = float("nan")
        if C > 1:
            y[:, C - 1] = float("nan")
        y[G // 2] = float("nan")
    return z, y
