"""ACF_ALT_LIB=path: load that build of libacf_apr.so in place of the package's,
for same-box A/Bs and bit comparisons of two builds in otherwise equal processes."""
import ctypes
import importlib
import os


def use_alt_lib(pkg):
    """Point `pkg`._native at $ACF_ALT_LIB when it is set; returns the path or None."""
    alt = os.environ.get("ACF_ALT_LIB")
    if alt:
        nat = importlib.import_module(pkg + "._native")
        lib = ctypes.CDLL(alt)
        for fname, (res, args) in nat.SIGNATURES.items():
            if hasattr(lib, fname):
                fn = getattr(lib, fname)
                fn.restype, fn.argtypes = res, args
        nat._lib = lib
    return alt
