"""CPU oracle of dp_gsat_amd.subgraph (numpy): the contract of gsat_subgraph_index restated -- order-preserving selection of nodes and
edges with relabelling by rank (PyG subgraph(..., relabel_nodes=True) semantics in node mode)."""
import numpy as np


def subgraph_oracle(edge_index, N, batch, node_ptr, keep, mode, drop_isolated=True):
    """mode "edge": keep[E] (nonzero = keep); kept nodes = endpoints of kept edges (drop_isolated) or all nodes.  mode "node": keep[N];
    an edge is kept iff both endpoints are.  Returns a dict of node_id, edge_id, edge_index, batch, node_ptr, edge_mask, counts."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    keep = np.asarray(keep).reshape(-1) != 0
    if mode == "edge":
        emask = keep.copy()
        nmask = np.ones(N, dtype=bool)
        if drop_isolated:
            nmask[:] = False
            nmask[ei[0][emask]] = True
            nmask[ei[1][emask]] = True
    else:
        nmask = keep.copy()
        emask = nmask[ei[0]] & nmask[ei[1]]
    node_id = np.flatnonzero(nmask).astype(np.int64)
    edge_id = np.flatnonzero(emask).astype(np.int64)
    rank = np.concatenate([[0], np.cumsum(nmask)]).astype(np.int64)          # exclusive scan, rank[N] = N'
    out = {"node_id": node_id, "edge_id": edge_id, "edge_index": rank[ei[:, edge_id]].reshape(2, -1),
           "edge_mask": emask.astype(np.uint8), "counts": (len(node_id), len(edge_id))}
    out["batch"] = np.asarray(batch, dtype=np.int64)[node_id] if batch is not None else None
    out["node_ptr"] = rank[np.asarray(node_ptr, dtype=np.int64)].astype(np.int32) if node_ptr is not None else None
    return out


def node_ptr_of(batch, G):
    return np.concatenate([[0], np.cumsum(np.bincount(np.asarray(batch, dtype=np.int64), minlength=G))]).astype(np.int32)


def extract_batch(b, keep, mode, drop_isolated=True):
    """The oracle applied to a synth.Batch on the host: a Batch of torch CPU tensors with the attributes gathered."""
    import torch
    from dp_gsat_amd.synth import Batch
    G = b.num_graphs
    o = subgraph_oracle(b.edge_index.numpy(), b.num_nodes, b.batch.numpy(), node_ptr_of(b.batch.numpy(), G), keep, mode, drop_isolated)
    nid, eid = torch.from_numpy(o["node_id"]), torch.from_numpy(o["edge_id"])
    ea = b.get("edge_attr")
    return Batch(x=b.x[nid], edge_index=torch.from_numpy(np.ascontiguousarray(o["edge_index"])), batch=torch.from_numpy(o["batch"]),
                 edge_attr=None if ea is None else ea[eid], y=b.y, num_graphs=G), o
