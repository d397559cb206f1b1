"""Inert placeholders for names the reference only drags in (datasets, loaders, plotting, chemistry)."""
import importlib
import sys
import types


class _Inert:
    """Usable as a base class and as a default value; instantiating a bare placeholder is an error."""
    _placeholder = True

    def __init__(self, *args, **kwargs):
        if "_placeholder" in vars(type(self)):
            raise RuntimeError("a placeholder of the recording stand-in was instantiated: %s" % type(self).__name__)


def make(name):
    return type(name, (_Inert,), {"_placeholder": True})


def module_getattr(attr):
    """PEP 562 hook: every public attribute of a placeholder module is a placeholder class of that name."""
    if attr.startswith("__"):
        raise AttributeError(attr)
    return make(attr)


def install(name):
    """Registers an empty placeholder module ``name`` (dotted allowed) unless the real one imports.  True if installed."""
    if name in sys.modules:
        return False
    try:
        importlib.import_module(name)
        return False
    except ImportError:
        pass
    mod = types.ModuleType(name)
    mod.__getattr__ = module_getattr
    mod.__path__ = []
    mod.__standin__ = True
    sys.modules[name] = mod
    parent, _, leaf = name.rpartition(".")
    if parent and parent in sys.modules:
        setattr(sys.modules[parent], leaf, mod)
    return True
