"""Stand-in for torch-scatter 2.0.9's ``scatter`` (documented behaviour; ATen only)."""
import torch

__standin__ = True


def _broadcast(index, src, dim):
    if dim < 0:
        dim = src.dim() + dim
    if index.dim() == 1:
        for _ in range(dim):
            index = index.unsqueeze(0)
    while index.dim() < src.dim():
        index = index.unsqueeze(-1)
    return index.expand(src.size())


def scatter(src, index, dim=-1, out=None, dim_size=None, reduce="sum"):
    """Reduces ``src`` along ``dim`` into the slots named by ``index``: sum / add, mean (sum over the count clamped to
    1), min, max (the values; a slot nothing is scattered to stays 0)."""
    if out is not None:
        raise NotImplementedError("the reference never passes out=")
    if dim < 0:
        dim = src.dim() + dim
    idx = _broadcast(index, src, dim)
    if dim_size is None:
        dim_size = int(index.max()) + 1 if index.numel() > 0 else 0
    shape = list(src.size())
    shape[dim] = dim_size
    zeros = torch.zeros(shape, dtype=src.dtype, device=src.device)
    if reduce in ("sum", "add"):
        return zeros.scatter_add(dim, idx, src)
    if reduce == "mean":
        total = zeros.scatter_add(dim, idx, src)
        ones = torch.ones(index.size(0), dtype=src.dtype, device=src.device)
        count = torch.zeros(dim_size, dtype=src.dtype, device=src.device).scatter_add(0, index, ones).clamp(min=1)
        return total / _broadcast(count, total, dim)
    if reduce in ("min", "max"):
        return zeros.scatter_reduce(dim, idx, src, "amin" if reduce == "min" else "amax", include_self=False)
    raise ValueError(reduce)
