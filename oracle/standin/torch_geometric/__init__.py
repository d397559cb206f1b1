"""Stand-in for the part of torch-geometric 2.0.3 that the reference's model path imports (see ../README.md)."""
__version__ = "2.0.3+standin"
__standin__ = True
