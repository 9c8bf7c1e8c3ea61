"""Argument checks shared by the host-side classes."""


def as_int(name, v):
    """`v` as an int, or ValueError naming the argument: bools and non-integral numbers are refused"""
    try:
        ok = not isinstance(v, bool) and int(v) == v
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return int(v)
