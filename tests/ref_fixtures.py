"""Loaders of tests/golden/ref_*: recordings of the reference's own classes (oracle/record_reference.py).  Data only: neither the
reference nor the recording stand-in is imported here, so the GPU tests can use it."""
import functools
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUTPUTS = ("emb", "att_log_logits", "att", "edge_att", "clf_logits", "loss", "pred", "info")


@functools.lru_cache(maxsize=None)
def settings():
    with open(os.path.join(GOLD, "ref_cases.json")) as f:
        return json.load(f)


def case_names():
    return list(settings()["cases"])


def _load(path):
    z = np.load(path)
    return {k: torch.from_numpy(z[k]) for k in z.files}


@functools.lru_cache(maxsize=None)
def load_case(name):
    """NS(s=settings, a=arrays of ref_<name>.npz, grad32, grad64).  Shared by the tests of a module: read only."""
    a = _load(os.path.join(GOLD, f"ref_{name}.npz"))
    a["edge_index"], a["batch"] = a["edge_index"].long(), a["batch"].long()
    return NS(name=name, s=settings()["cases"][name], a=a, grad32=_load(os.path.join(GOLD, f"ref_{name}.grad32.npz")),
              grad64=_load(os.path.join(GOLD, f"ref_{name}.grad64.npz")))


@functools.lru_cache(maxsize=None)
def load_operators():
    return _load(os.path.join(GOLD, "ref_operators.npz"))


@functools.lru_cache(maxsize=None)
def load_dual():
    """ref_dual.npz: one dual/primal step of src/run_gsat.py (node attention on both graphs)."""
    a = _load(os.path.join(GOLD, "ref_dual.npz"))
    for k in ("p.edge_index", "p.batch", "d.edge_index", "d.batch"):
        a[k] = a[k].long()
    return a


def model_config(c):
    s = c.s
    cfg = dict(model_name=s["backbone"], n_layers=s["n_layers"], hidden_size=s["H"], dropout_p=0.0, use_edge_attr=True,
               atom_encoder=s.get("atom_encoder", False))
    if s["backbone"] == "PNA":
        cfg.update(aggregators=s["aggregators"], scalers=s["scalers"], deg=c.a["deg"])
    return cfg


def state(c, part):
    prefix = f"state.{part}."
    return {k[len(prefix):]: v for k, v in c.a.items() if k.startswith(prefix)}


def batch(c, dtype=torch.float32):
    """The recorded batch as the attribute bag ``forward_pass`` reads; floating inputs in ``dtype``."""
    from dp_gsat_amd.synth import Batch
    cast = lambda t: t.to(dtype) if t is not None and t.is_floating_point() else t
    return Batch(x=cast(c.a["x"]), edge_index=c.a["edge_index"], batch=c.a["batch"], edge_attr=cast(c.a.get("edge_attr")), y=cast(c.a["y"]))


def draws(c, dtype=torch.float32):
    return c.a["u"].to(dtype), [c.a["mask1"].to(dtype), c.a["mask2"].to(dtype)]
