"""What every ctypes binding of the package shares: attaching prototypes, turning a status into the module's error, owning
a C handle, and the array preambles of add() and search().

A module that binds a header consists of its PROTOS, its error class, `_lib = binder(PROTOS, tag, load_library)`,
`_check = checker(...)` and Handle subclasses.  Ownership: the Python object whose `_owned` is true destroys the C handle,
once, in close(); on any other object close() does nothing.  Ownership leaves an object only through _disown() (another
handle's C side took this one over: the object stays a view of it until that owner closes and clears it) or _take()
(another Python object did), and an object that has given it away refuses to give it away again.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np


def attach(lib, protos) -> None:
    """restype / argtypes of every prototype; a symbol the library lacks raises AttributeError naming it."""
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


def binder(protos, tag: str, load, also=()):
    """The module's `_lib()`: load() with `protos` attached, once per library object (the flag lives on it, so a library
    loaded from an explicit path gets its own).  `also`: the `_lib` of modules whose prototypes this one calls too."""
    flag = f"_{tag}_ready"

    def _lib():
        lib = load()
        if not getattr(lib, flag, False):
            attach(lib, protos)
            for other in also:
                other()
            setattr(lib, flag, True)
        return lib

    return _lib


def checker(error_class, label: str, last_error_name: Optional[str], with_code: bool = False):
    """The module's `_check(lib, rc)`: a status other than 0 raises error_class("<label> error <rc>: <last error>"), or
    error_class(rc, <last error>) for a class that keeps the code.  last_error_name None: `_check(lib, rc, last_error)`,
    for a module that reports through the last_error function of whichever prefix it called."""
    def raise_(rc, text):
        raise error_class(rc, text) if with_code else error_class(f"{label} error {rc}: {text}")

    if last_error_name is None:
        def _check(lib, rc: int, last_error) -> None:
            if rc != 0:
                raise_(rc, last_error().decode())
    else:
        def _check(lib, rc: int) -> None:
            if rc != 0:
                raise_(rc, getattr(lib, last_error_name)().decode())
    return _check


class Handle:
    """Base of every class that owns a C handle: `_h`, `_owned`, and in the subclass `_destroy` (the symbol that frees the
    handle) and `_lib` (the module's, as a staticmethod)."""

    _h = None
    _owned = True
    _destroy = ""
    _lib = None

    def _closed(self) -> None:
        """Hook: what else close() does once it has destroyed the handle."""

    def close(self) -> None:
        if self._h and self._owned:
            h, self._h = self._h, None
            getattr(self._lib(), self._destroy)(h)
            self._closed()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _owning(self) -> None:
        if not self._owned:
            raise ValueError(f"this {type(self).__name__} has given its handle away: it is destroyed by its new owner")

    def _disown(self) -> None:
        """Another handle took this one over and destroys it with itself: it stays usable here, close() does nothing."""
        self._owning()
        self._owned = False

    def _take(self, other: "Handle") -> None:
        """Moves other's handle, and the duty to destroy it, here; `other` is left closed."""
        other._owning()
        self._h, self._owned = other._h, True
        other._h, other._owned = None, False


def rows(a, d: Optional[int] = None) -> np.ndarray:
    """fp32 C-contiguous [n, d]; a 1-D input is one row."""
    v = np.ascontiguousarray(a, np.float32)
    if v.ndim == 1:
        v = v[None, :]
    if v.ndim != 2 or (d is not None and v.shape[1] != d):
        raise ValueError(f"expected rows of dimension {d}, got shape {v.shape}")
    return v


def result_triple(nq: int, k: int, clamp: bool = False):
    """(ids int64 [nq, k], dist fp32 [nq, k], cnt int32 [nq]), zero-filled; clamp: k < 0 gives width 0, for the library to
    refuse, not numpy."""
    if clamp:
        k = max(k, 0)
    return np.zeros((nq, k), np.int64), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)


def ids_or_none(ids, n: int, what: str = "vector") -> Optional[np.ndarray]:
    """The optional ids of add(): int64 [n], or None."""
    if ids is None:
        return None
    idp = np.ascontiguousarray(ids, np.int64)
    if idp.shape != (n,):
        raise ValueError(f"one id per {what}")
    return idp


def ptr(a: Optional[np.ndarray]):
    """The address of an array, or None (a NULL argument)."""
    return None if a is None else a.ctypes.data
