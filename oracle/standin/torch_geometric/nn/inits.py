"""torch_geometric.nn.inits.reset."""


def reset(nn):
    """Calls ``reset_parameters`` on ``nn`` or, for a container, on each of its children."""
    def _reset(item):
        if hasattr(item, "reset_parameters"):
            item.reset_parameters()

    if nn is not None:
        if hasattr(nn, "children") and len(list(nn.children())) > 0:
            for item in nn.children():
                _reset(item)
        else:
            _reset(nn)
