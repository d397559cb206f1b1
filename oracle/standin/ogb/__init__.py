"""Stand-in for the part of ogb 1.3.2 that the reference's model path imports (see ../README.md)."""
__version__ = "1.3.2+standin"
__standin__ = True
