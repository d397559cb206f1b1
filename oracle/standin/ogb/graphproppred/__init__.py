"""PygGraphPropPredDataset / Evaluator are only dragged in: inert placeholders."""
from _placeholder import module_getattr as __getattr__  # noqa: F401
