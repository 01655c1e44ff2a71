"""Holder of the ``paddle`` stand-in (see paddle/__init__.py).  This directory is never on sys.path by default."""
import contextlib
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))


@contextlib.contextmanager
def on_path(*more):
    """``with on_path(): import paddle`` -- puts the stand-in (and the directories in ``more``, e.g. a checkout of the reference) first on
    sys.path; afterwards takes them off again and drops every module that was loaded meanwhile from those directories, ``paddle`` included."""
    dirs = [_HERE] + [os.path.abspath(d) for d in more]
    before = set(sys.modules)
    for d in dirs:
        sys.path.insert(0, d)
    try:
        yield
    finally:
        for d in dirs:
            sys.path.remove(d)
        for k in set(sys.modules) - before:
            f = getattr(sys.modules[k], "__file__", None) or ""
            if any(os.path.abspath(f).startswith(d + os.sep) for d in dirs):
                del sys.modules[k]
