"""torch_geometric.nn: the conv bases, InstanceNorm, BatchNorm and the two global pools (2.0.3, documented behaviour)."""
import torch
import torch.nn.functional as F

from torch_geometric.nn.conv import GINConv, GINEConv, LEConv, MessagePassing  # noqa: F401
from torch_scatter import scatter


class InstanceNorm(torch.nn.Module):
    """Per graph and channel: (x - mean) / sqrt(biased variance + eps), by ATen's ``F.instance_norm`` on each graph's rows.
    Defaults (the reference's use): no affine parameters, no running statistics, so train and eval compute the same."""

    def __init__(self, in_channels, eps=1e-5, momentum=0.1, affine=False, track_running_stats=False):
        super().__init__()
        if affine or track_running_stats:
            raise NotImplementedError("the reference constructs InstanceNorm(channels) only")
        self.in_channels, self.eps = in_channels, eps

    def forward(self, x, batch=None):
        if batch is None:
            batch = torch.zeros(x.size(0), dtype=torch.long, device=x.device)
        out = torch.zeros_like(x)
        for g in range(int(batch.max()) + 1 if batch.numel() else 0):
            rows = (batch == g).nonzero().view(-1)
            if rows.numel() == 1:           # one row: x - mean = 0 (F.instance_norm refuses a single element)
                continue
            if rows.numel() > 1:
                y = F.instance_norm(x.index_select(0, rows).t().unsqueeze(0), eps=self.eps)
                out = out.index_copy(0, rows, y.squeeze(0).t())
        return out


class BatchNorm(torch.nn.Module):
    """Thin wrapper that keeps ``torch.nn.BatchNorm1d`` as ``.module``."""

    def __init__(self, in_channels, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.module = torch.nn.BatchNorm1d(in_channels, eps, momentum, affine, track_running_stats)

    def reset_parameters(self):
        self.module.reset_parameters()

    def forward(self, x):
        return self.module(x)


def _num_graphs(batch, size):
    return int(batch.max()) + 1 if size is None else size


def global_add_pool(x, batch, size=None):
    return scatter(x, batch, dim=0, dim_size=_num_graphs(batch, size), reduce="add")


def global_mean_pool(x, batch, size=None):
    return scatter(x, batch, dim=0, dim_size=_num_graphs(batch, size), reduce="mean")
