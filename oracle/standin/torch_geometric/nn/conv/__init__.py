"""MessagePassing and the three base convolutions the reference subclasses (torch-geometric 2.0.3, documented behaviour).

Only what the reference reaches: ``aggr`` 'add' (any reduce of ``scatter``) or None, flow source_to_target, dense
``edge_index`` [2, E].  Constructor arguments and attribute names are PyG's, so ``state_dict`` keys are unchanged.
"""
import inspect

import torch
from torch.nn import Linear

from torch_geometric.nn.inits import reset
from torch_scatter import scatter


class MessagePassing(torch.nn.Module):
    def __init__(self, aggr="add", flow="source_to_target", node_dim=-2):
        super().__init__()
        if flow != "source_to_target":
            raise NotImplementedError(flow)
        self.aggr, self.flow, self.node_dim = aggr, flow, node_dim

    def propagate(self, edge_index, size=None, **kwargs):
        """message -> aggregate -> update.  A ``message`` argument ``name_j`` / ``name_i`` is ``kwargs[name]`` gathered at
        the source row ``edge_index[0]`` / the target row ``edge_index[1]`` (of a pair, its first / second member); every
        other argument is passed through by name, its default standing in when it was not given."""
        j, i = 0, 1
        size = [None, None] if size is None else list(size)
        args = {}
        for name, param in inspect.signature(self.message).parameters.items():
            if name[-2:] in ("_i", "_j"):
                side = j if name[-2:] == "_j" else i
                data = kwargs.get(name[:-2], inspect.Parameter.empty)
                if isinstance(data, (tuple, list)):
                    data = data[side]
                if isinstance(data, torch.Tensor):
                    if size[side] is None:
                        size[side] = data.size(self.node_dim)
                    elif size[side] != data.size(self.node_dim):
                        raise ValueError("inconsistent sizes")
                    data = data.index_select(self.node_dim, edge_index[side])
            else:
                data = kwargs.get(name, inspect.Parameter.empty)
            if data is inspect.Parameter.empty:
                if param.default is inspect.Parameter.empty:
                    raise TypeError(f"propagate: required message argument {name!r} is missing")
                data = param.default
            args[name] = data
        size[0] = size[1] if size[0] is None else size[0]
        size[1] = size[0] if size[1] is None else size[1]
        out = self.message(**args)
        out = self.aggregate(out, edge_index[i], dim_size=size[i])
        return self.update(out)

    def message(self, x_j):
        return x_j

    def aggregate(self, inputs, index, dim_size=None):
        return scatter(inputs, index, dim=self.node_dim, dim_size=dim_size, reduce=self.aggr)

    def update(self, inputs):
        return inputs


class GINConv(MessagePassing):
    def __init__(self, nn, eps=0.0, train_eps=False, **kwargs):
        kwargs.setdefault("aggr", "add")
        super().__init__(**kwargs)
        self.nn = nn
        self.initial_eps = eps
        if train_eps:
            self.eps = torch.nn.Parameter(torch.Tensor([eps]))
        else:
            self.register_buffer("eps", torch.Tensor([eps]))
        self.reset_parameters()

    def reset_parameters(self):
        reset(self.nn)
        self.eps.data.fill_(self.initial_eps)


class GINEConv(MessagePassing):
    def __init__(self, nn, eps=0.0, train_eps=False, edge_dim=None, **kwargs):
        kwargs.setdefault("aggr", "add")
        super().__init__(**kwargs)
        self.nn = nn
        self.initial_eps = eps
        if train_eps:
            self.eps = torch.nn.Parameter(torch.Tensor([eps]))
        else:
            self.register_buffer("eps", torch.Tensor([eps]))
        if edge_dim is not None:
            first = self.nn[0] if hasattr(self.nn, "__getitem__") else self.nn
            in_channels = first.in_features if hasattr(first, "in_features") else first.in_channels
            self.lin = Linear(edge_dim, in_channels)
        else:
            self.lin = None
        self.reset_parameters()

    def reset_parameters(self):
        reset(self.nn)
        self.eps.data.fill_(self.initial_eps)
        if self.lin is not None:
            self.lin.reset_parameters()


class LEConv(MessagePassing):
    """x_i' = lin3(x_i) + sum_j e_ji (lin1(x_j) - lin2(x_i)); lin1 and lin3 carry the bias, lin2 has none."""

    def __init__(self, in_channels, out_channels, bias=True, **kwargs):
        kwargs.setdefault("aggr", "add")
        super().__init__(**kwargs)
        self.in_channels, self.out_channels = in_channels, out_channels
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        self.lin1 = Linear(in_channels[0], out_channels, bias=bias)
        self.lin2 = Linear(in_channels[1], out_channels, bias=False)
        self.lin3 = Linear(in_channels[1], out_channels, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        self.lin1.reset_parameters()
        self.lin2.reset_parameters()
        self.lin3.reset_parameters()
