"""Only dragged in by the reference's dataset and loader modules: inert placeholders."""
from _placeholder import module_getattr as __getattr__  # noqa: F401
