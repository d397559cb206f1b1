"""Stand-in for torch-sparse 0.6.12's ``transpose`` (documented behaviour)."""
import torch

__standin__ = True


def transpose(index, value, m, n, coalesced=True):
    """Swaps the two index rows.  ``coalesced=False`` (the reference's call): nothing else, the values stay in place.
    ``coalesced=True``: also sorts by the new (row, col); duplicate entries, which coalescing would add up, are refused."""
    row, col = index[0], index[1]
    index = torch.stack([col, row], dim=0)
    if not coalesced:
        return index, value
    size = int(index.max()) + 1 if index.numel() else 1
    key = index[0] * size + index[1]
    if torch.unique(key).numel() != key.numel():
        raise NotImplementedError("duplicate entries")
    perm = key.argsort()
    return index[:, perm], (None if value is None else value[perm])
