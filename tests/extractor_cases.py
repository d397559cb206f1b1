"""Seeded inputs of the extractor path tests (tests/test_gpu_extractor_paths.py, tests/test_extractor_cases_host.py): the batch tables,
every tensor a case feeds the kernels, and the caps on the reference's own fp32 rounding that the comparisons rest on.  Inputs only; the
reference is tests/extractor_oracle.py."""
import functools

import numpy as np
import torch

from tests.graphs import shuffle_edges
from tests.util import TOL

P_DROP = 0.5


def sized_batch(sizes, seed, undirected=True, isolated=True):
    """Random trees + a few extra edges with the given node counts per graph (0 allowed: an empty graph)."""
    rng = np.random.RandomState(seed)
    src, dst, batch, off = [], [], [], 0
    for g, n in enumerate(sizes):
        es = set()
        for v in range(1, n):
            if isolated and rng.rand() < 0.04:
                continue
            es.add((int(rng.randint(0, v)), v))
        for _ in range(int(0.12 * n)):
            a, b = rng.randint(0, max(n, 1), size=2)
            if a != b:
                es.add((int(min(a, b)), int(max(a, b))))
        for (u, v) in sorted(es):
            src += [u + off, v + off] if undirected else [u + off]
            dst += [v + off, u + off] if undirected else [v + off]
        batch += [g] * n
        off += n
    ei = torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1)
    return ei, torch.tensor(batch, dtype=torch.int64), off


def edge_sized_batch(edge_counts, seed):
    """Graphs with exactly the given numbers of DIRECTED edges (the rows of edge mode): a random tree on e // 2 + 1 nodes, every tree
    edge once, then the reverses of the first e - (n - 1) of them.  0 edges: one isolated node (an empty graph of edge mode whose node
    still owns a row of demb)."""
    rng = np.random.RandomState(seed)
    src, dst, batch, off = [], [], [], 0
    for g, e in enumerate(edge_counts):
        n = (e + 1) // 2 + 1 if e > 0 else 1
        tree = [(int(rng.randint(0, v)), v) for v in range(1, n)]
        es = tree + [(v, u) for (u, v) in tree[:e - len(tree)]]
        assert len(es) == e and len(set(es)) == e
        src += [u + off for u, _ in es]
        dst += [v + off for _, v in es]
        batch += [g] * n
        off += n
    ei = torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1)
    return ei, torch.tensor(batch, dtype=torch.int64), off


# ---- the two families -------------------------------------------------------------------------------------------------------------
# "regular": every graph has at least MIN_ROWS rows in the mode under test (an empty graph is allowed), so that the InstanceNorm backward
# is well conditioned and the fp32 reference sits within TOL / 4 of the fp64 one: this family carries the numerical claim.  The row counts
# sit on the sizes the kernels branch on -- node counts in node mode, directed-edge counts in edge mode.
MIN_ROWS = 4
BOUNDARY_ROWS = {
    32: "16 row slots x SB_RC = 2 rows kept in registers by the segmented kernels", 33: "one row past it",
    64: "forward tile of RM = 64 rows (NRB = 1)", 65: "one row past it",
    128: "forward RM = 128, backward B_RM = 128, the 128-edge tile of edge mode", 129: "one row past it",
    257: "one graph above 2 * RM: walked in slabs (a 'big' tile)",
    0: "an empty graph",
}
REGULAR = {"boundaries": [4, 5, 32, 33, 64, 65, 128, 129, 257, 0, 12, 40]}       # 4 + 5 + 12 (+ 32): several small graphs in one tile
# "tiny": graphs of 0, 1, 2 and 3 rows among ordinary ones (node counts; in edge mode their trees give 0, 2, 4, ... rows).  A 2-row graph
# whose rows differ by ~sqrt(eps) in a channel has 1/sigma ~ 300 there, and the fp32 reference's own rounding reaches 1e-3 of a gradient's
# scale: this family finds unwritten rows, rows of the wrong graph and broken tile packing, at the caps below.
TINY = {
    "molecules": [25, 31, 12, 40, 96, 7, 18, 22, 64, 33, 29, 3, 2, 51, 17, 128, 1, 0, 45],
    "tiny": [0, 1, 1, 2, 1, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 5, 0],
}
FAMILIES = {"regular": REGULAR, "tiny": TINY}

FWD_WIDTHS = (8, 16, 40, 64, 80, 128, 256)        # C2 = 8 .. 256: the head kernel's 4 / 8 / 16 / 32 / 64 lanes per row; C1 a multiple of 64 or not
BWD_WIDTHS = (16, 64, 80, 128)                    # the fused backward's ncht = 2 / 4 / 8, padded C2p at 16 and 80
BWD_STAGED_WIDTHS = (8,) + BWD_WIDTHS + (256,)
TINY_WIDTHS = (16, 64)
# one-launch forward only: the widths at which its tile shape changes (gsat_attn_paths; tests/test_extractor_cases_host.py keeps the table
# below equal to what the library reports).  nrb: 64-row blocks per row wave, ncbw: 32-column blocks of layer 2 per column wave, pqg: P | Q
# through global memory is available (edge mode), x6: split-bf16 x 6 products are available
FUSED_EXTRA_WIDTHS = (136, 192, 232)
FUSED_FWD_EXPECT = {
    # node mode
    (False, 8): dict(nrb=2, ncbw=1, pqg=0, x6=0), (False, 16): dict(nrb=2, ncbw=1, pqg=0, x6=1), (False, 40): dict(nrb=2, ncbw=1, pqg=0, x6=0),
    (False, 64): dict(nrb=2, ncbw=1, pqg=0, x6=1), (False, 80): dict(nrb=2, ncbw=1, pqg=0, x6=1), (False, 128): dict(nrb=2, ncbw=1, pqg=0, x6=1),
    (False, 136): dict(nrb=1, ncbw=2, pqg=0, x6=0),        # the first width with 64-row tiles
    (False, 192): dict(nrb=1, ncbw=2, pqg=0, x6=0), (False, 232): dict(nrb=1, ncbw=2, pqg=0, x6=0), (False, 256): dict(nrb=1, ncbw=2, pqg=0, x6=0),
    # edge mode
    (True, 8): dict(nrb=2, ncbw=1, pqg=1, x6=0), (True, 16): dict(nrb=2, ncbw=1, pqg=1, x6=1), (True, 40): dict(nrb=2, ncbw=1, pqg=1, x6=0),
    (True, 64): dict(nrb=2, ncbw=1, pqg=1, x6=1), (True, 80): dict(nrb=2, ncbw=1, pqg=1, x6=1), (True, 128): dict(nrb=2, ncbw=1, pqg=1, x6=1),
    (True, 136): dict(nrb=2, ncbw=2, pqg=1, x6=0),         # two column blocks per wave, still 128-row tiles
    (True, 192): dict(nrb=2, ncbw=2, pqg=0, x6=0),         # the first width at which P | Q only fit in the tile
    (True, 232): dict(nrb=1, ncbw=2, pqg=0, x6=0),         # the first width with 64-row tiles
    (True, 256): dict(nrb=1, ncbw=2, pqg=0, x6=0),
}
# the fused backward's template (layer-1 chunks) per (edge_mode, H); widths missing here are beyond it (C2 > 128) and fall back to the staged kernels
FUSED_BWD_NCHT = {(False, 8): 2, (False, 16): 2, (False, 64): 2, (False, 80): 4, (False, 128): 4,
                  (True, 8): 2, (True, 16): 2, (True, 64): 4, (True, 80): 8, (True, 128): 8}
DUAL_GEMM_MAX_H = 128         # the dual tile kernels hold C2 (layer 2) / H (layer 1) <= 128 columns; wider: the separate GEMMs

FWD_TENSORS = ("logits", "att", "P", "Q", "a1", "h2", "mean1", "var1", "mean2", "var2")
GRAD_TENSORS = ("demb", "dW1", "db1", "dW2", "db2", "dW3", "db3")

# ---- caps on 4 * |r32 - r64|max / max(1, |r64|max), the slack the project's comparison rule adds for the fp32 reference's own rounding ---
# A cap is a condition on the reference alone (tests/test_extractor_cases_host.py asserts it without a GPU), never a measurement of a kernel.
CAP_REGULAR = TOL                 # measured |r32 - r64| / scale over every regular case, width, mode, train / eval: see REGULAR_GAP_MEASURED
CAP_FORWARD = 2 * TOL             # forward tensors of any batch
# worst |r32 - r64|max / scale over the regular family (all FWD_WIDTHS, both modes, train and eval), measured on the CPU reference
REGULAR_GAP_MEASURED = {"forward": 2.1e-6, "gradients": 1.06e-5}       # x 4 = 4.3e-5 <= CAP_REGULAR; the large case: 3.8e-7 / 1.2e-5
# tiny family, gradients: worst |r32 - r64|max / scale per tensor over both lists, TINY_WIDTHS, both modes, train and eval, measured on the
# CPU reference with the seeds below; the cap is 4 x 2 x that (the factor 2: another BLAS thread count sums in another order)
# (forward tensors of the tiny family, same measurement: at most 3.4e-5, on a1; x 4 = 1.4e-4 <= CAP_FORWARD)
TINY_GAP_MEASURED = {"demb": 6.93e-4, "dW1": 6.99e-4, "db1": 4.9e-6, "dW2": 4.94e-4, "db2": 1.14e-5, "dW3": 2.52e-5, "db3": 2.7e-6}
CAP_TINY_GRAD = {k: max(CAP_REGULAR, 8.0 * v) for k, v in TINY_GAP_MEASURED.items()}       # never below the regular family's cap


def cap_for(family, tensor):
    if family == "regular":
        return CAP_REGULAR
    return CAP_FORWARD if tensor in FWD_TENSORS else CAP_TINY_GRAD[tensor]


def widths(edge_mode, H):
    """(C0, C1, C2) of ExtractorMLP(H, edge_mode)."""
    return (2 * H, 4 * H, H) if edge_mode else (H, 2 * H, H)


def make_params(H, edge_mode, seed):
    g = torch.Generator().manual_seed(seed)
    C0, C1, C2 = widths(edge_mode, H)
    mk = lambda *s: torch.randn(*s, generator=g) / (s[-1] ** 0.5)
    return (mk(C1, C0), mk(C1) * 0.1, mk(C2, C1), mk(C2) * 0.1, mk(1, C2), mk(1) * 0.1)


def _finish(ei, batch, N, G_, H, edge_mode, training, seed, redraw=0):
    """Every tensor of one step from one generator: embedding, masks, noise, upstream gradients; the weights from a second one (CPU, fp32)."""
    g = torch.Generator().manual_seed(1000 * seed + H + 100003 * redraw)
    _, C1, C2 = widths(edge_mode, H)
    M = ei.shape[1] if edge_mode else N
    emb = torch.randn(N, H, generator=g)
    masks = u = None
    if training:
        masks = ((torch.rand(M, C1, generator=g) > P_DROP).float(), (torch.rand(M, C2, generator=g) > P_DROP).float())
        u = torch.rand(M, generator=g).clamp_(1e-6, 1 - 1e-6)
    dlogits, datt = torch.randn(M, generator=g), torch.randn(M, generator=g)
    rows = torch.bincount(batch[ei[0]] if edge_mode else batch, minlength=G_)
    return dict(ei=ei, batch=batch, N=N, G=G_, M=M, H=H, edge_mode=edge_mode, training=training, emb=emb,
                params=make_params(H, edge_mode, seed + 11), masks=masks, u=u, dlogits=dlogits, datt=datt, rows=rows)


SEEDS = {"regular": 3, "tiny": 5, "large": 7}

# ReLU is not differentiable at 0: a pre-activation whose centred value lies within the kernels' fp32 rounding of 0 (K <= 1024 term sums of
# O(1) values: a few 1e-7) may get another sign on the GPU than in fp64, and that one element then moves dW1 by 1e-2 of its scale (seen on
# the CPU between the fp32 and the fp64 reference at C1 = 1024, 8e5 elements).  Such inputs test nothing, so every case keeps the centred
# pre-activations of both layers, in fp64, at least RELU_MARGIN away from 0 (exact zeros -- the rows of one-row graphs -- aside: ReLU'(0) = 0
# everywhere).  Where the first draw of a case misses the margin or a cap, REDRAW names the draw that meets them (found on the CPU reference
# alone: the first of 0, 1, 2, ... that passes tests/test_extractor_cases_host.py).
RELU_MARGIN = 2e-6
# the large cases have 6.3e6 (H = 64) and 1.3e7 (H = 128) pre-activations, the closest of which lies 1e-7 to 2e-7 from 0 in a typical draw:
# each takes the draw with the widest margin of the first 80 / 40 (their layer products are sums of K = 64 .. 256 terms, rounding ~1e-7)
LARGE_RELU_MARGIN = {64: 8e-7, 128: 3.5e-7}
REDRAW = {
    ("regular", "boundaries", False, 16, False, False): 2,
    ("regular", "boundaries", False, 64, False, False): 1,
    ("regular", "boundaries", False, 80, True, False): 2,
    ("regular", "boundaries", False, 80, False, False): 2,
    ("regular", "boundaries", False, 128, True, False): 2,
    ("regular", "boundaries", False, 256, True, False): 1,
    ("regular", "boundaries", False, 256, False, False): 5,
    ("regular", "boundaries", True, 80, True, False): 1,
    ("regular", "boundaries", True, 80, True, True): 1,
    ("regular", "boundaries", True, 80, False, False): 1,
    ("regular", "boundaries", True, 80, False, True): 1,
    ("regular", "boundaries", True, 128, True, False): 1,
    ("regular", "boundaries", True, 128, True, True): 1,
    ("regular", "boundaries", True, 128, False, False): 1,
    ("regular", "boundaries", True, 128, False, True): 1,
    ("regular", "boundaries", True, 256, True, False): 1,
    ("regular", "boundaries", True, 256, True, True): 3,
    ("regular", "boundaries", True, 256, False, False): 1,
    ("regular", "boundaries", True, 256, False, True): 1,
    ("tiny", "molecules", True, 64, False, False): 4,
    ("large", 64): 12,
    ("large", 128): 17,
}


@functools.lru_cache(maxsize=None)
def make_case(family, name, edge_mode, H, training, sorted_edges=False):
    """One case of a family's table.  ``sorted_edges``: keep the edges grouped by graph (edge-mode rows contiguous per graph: the kernels
    may run without a row order); otherwise they are shuffled."""
    sizes = FAMILIES[family][name]
    seed = SEEDS[family]
    if family == "regular" and edge_mode:
        ei, batch, N = edge_sized_batch(sizes, seed)
    else:
        ei, batch, N = sized_batch(sizes, seed, isolated=(family != "regular"))
    if not sorted_edges:
        ei = shuffle_edges(ei, seed)
    c = _finish(ei, batch, N, len(sizes), H, edge_mode, training, seed, REDRAW.get((family, name, edge_mode, H, training, sorted_edges), 0))
    c.update(family=family, name=name, sorted_edges=sorted_edges)
    return c


LARGE_ROWS = 32768            # the row count from which the library takes the one-launch forward by itself (node mode, H % 16 == 0)
LARGE_WIDTHS = (64, 128)      # 64: the automatic one-launch forward; 128: also the paired backward GEMMs (whole 128-column tiles of dW)


@functools.lru_cache(maxsize=None)
def make_large_case(H=64):
    """Node mode, at least LARGE_ROWS rows in graphs of 16 to 40 nodes, training: the default large-batch step."""
    rng = np.random.RandomState(SEEDS["large"])
    sizes = []
    while sum(sizes) < LARGE_ROWS:
        sizes.append(int(rng.randint(16, 41)))
    ei, batch, N = sized_batch(sizes, SEEDS["large"], isolated=False)
    c = _finish(ei, batch, N, len(sizes), H, False, True, SEEDS["large"], REDRAW.get(("large", H), 0))
    c.update(family="regular", name="large", sorted_edges=True)
    return c


def all_cases():
    """(family, name, edge_mode, H, training, sorted_edges) of every table case at every width and mode the GPU tests use."""
    out = []
    for family, table in FAMILIES.items():
        hs = sorted(set(FWD_WIDTHS) | set(FUSED_EXTRA_WIDTHS) | set(BWD_STAGED_WIDTHS)) if family == "regular" else TINY_WIDTHS
        for name in table:
            for edge_mode in (False, True):
                for H in hs:
                    for training in (True, False):
                        out.append((family, name, edge_mode, H, training, False))
                        if family == "regular" and edge_mode and H in FWD_WIDTHS:
                            out.append((family, name, edge_mode, H, training, True))
    return out
