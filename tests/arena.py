"""Guarded buffers for the extent, isolation and alignment tests (a helper module, not a conftest).

An ``Arena`` is one allocation laid out as ``guard | body | guard``: the body is what a caller hands to the library (a column of
n_rows values, an output table), each guard is at least ``GUARD`` = 2 048 elements -- two of the largest row tiles, the 1 024 rows
of the K3c / K4c kernels -- and the body starts on a 16-byte boundary (plus ``shift`` elements where a test wants it off the grid).

Input arenas carry the test's data in the body and a fill of the test's choice in the guards: a kernel that reads past a column's
extent then sees NaN in one run and 7.0 in the next, and two runs that are bit-equal did not use what they read.  Output arenas are
filled completely, body and guards, with a sentinel bit pattern that no kernel produces and no input contains (a quiet NaN with a
payload for the floats, 0x5a.. for the integers): ``check_guards`` finds a store outside the extent, ``check_written`` an element the
call left alone.  Every sentinel comparison is made on integer views, never with float equality.

``arena_engine()`` gives an ``Engine`` whose instance attribute ``_alloc`` is an ``ArenaAllocator``: every entry that allocates its
outputs through ``self._alloc`` then writes into guarded arenas, with no change to the product."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

GUARD = 2048

# dtype -> (integer view, sentinel)
SENTINELS = {
    np.dtype(np.float32): (np.dtype(np.int32), 0x7FC5A5A5),
    np.dtype(np.float64): (np.dtype(np.int64), 0x7FF85A5A5A5A5A5A),
    np.dtype(np.int32): (np.dtype(np.int32), 0x5A5A5A5A),
    np.dtype(np.int64): (np.dtype(np.int64), 0x5A5A5A5A5A5A5A5A),
    np.dtype(np.uint8): (np.dtype(np.uint8), 0x5A),
}


def _torch_dtype(dt: np.dtype):
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
            np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8}[dt]


def _numpy_dtype(dt) -> np.dtype:
    if torch is not None and isinstance(dt, torch.dtype):
        return np.dtype({torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64,
                         torch.uint8: np.uint8}[dt])
    return np.dtype(dt)


class Arena:
    """guard | body | guard in one allocation, host (numpy) or device (torch).  ``body`` is a view of the allocation."""

    def __init__(self, shape, dtype, device: bool = False, guard: int = GUARD, shift: int = 0):
        self.shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        self.dtype = _numpy_dtype(dtype)
        self.device = bool(device)
        self.idtype, self.sentinel = SENTINELS[self.dtype]
        isz = self.dtype.itemsize
        n = int(np.prod(self.shape, dtype=np.int64))
        total = 2 * guard + n + 2 * (16 // isz) + abs(int(shift))
        if device:
            self.raw = torch.empty(total, dtype=_torch_dtype(self.dtype), device="cuda")
            ptr = self.raw.data_ptr()
        else:
            self.raw = np.empty(total, dtype=self.dtype)
            ptr = self.raw.ctypes.data
        assert ptr % isz == 0
        self.lo = guard + ((-(ptr + guard * isz)) % 16) // isz + int(shift)
        self.hi = self.lo + n
        assert self.lo >= guard and total - self.hi >= guard
        self.fill_sentinel()

    # ------------------------------------------------------------------ views
    @property
    def body(self):
        return self.raw[self.lo:self.hi].reshape(self.shape)

    @property
    def body_address(self) -> int:
        return (self.raw.data_ptr() if self.device else self.raw.ctypes.data) + self.lo * self.dtype.itemsize

    def host(self) -> np.ndarray:
        """the body as a numpy array on the host (a copy)"""
        a = self.raw.cpu().numpy() if self.device else self.raw
        return np.array(a[self.lo:self.hi].reshape(self.shape), copy=True)

    def ints(self) -> np.ndarray:
        """the whole allocation as integers on the host"""
        a = self.raw.cpu().numpy() if self.device else self.raw
        return a.view(self.idtype)

    # ------------------------------------------------------------------ fills
    def _iview(self):
        if self.device:
            return self.raw if self.dtype == np.uint8 else self.raw.view(_torch_dtype(self.idtype))
        return self.raw.view(self.idtype)

    def fill_sentinel(self) -> "Arena":
        v = self._iview()
        if self.device:
            v.fill_(self.sentinel)
        else:
            v[:] = self.sentinel
        return self

    def fill_guards(self, value) -> "Arena":
        self.raw[:self.lo] = value
        self.raw[self.hi:] = value
        return self

    def set_body(self, values) -> "Arena":
        values = np.array(values, dtype=self.dtype, copy=True).reshape(-1)      # (a copy: torch wants a writable array)
        assert values.size == self.hi - self.lo, (values.size, self.hi - self.lo)
        if self.device:
            self.raw[self.lo:self.hi] = torch.from_numpy(values).to(self.raw.device)
        else:
            self.raw[self.lo:self.hi] = values
        return self


def input_arena(values, fill, device: bool = False, shift: int = 0) -> Arena:
    values = np.asarray(values)
    return Arena(values.shape, values.dtype, device=device, shift=shift).set_body(values).fill_guards(fill)


def output_arena(shape, dtype, device: bool = False, shift: int = 0) -> Arena:
    return Arena(shape, dtype, device=device, shift=shift)


def check_guards(a: Arena, what: str = "") -> None:
    """every guard element still holds the sentinel"""
    v = a.ints()
    before, after = np.flatnonzero(v[:a.lo] != a.sentinel), np.flatnonzero(v[a.hi:] != a.sentinel)
    if before.size or after.size:
        raise AssertionError(f"{what}: {before.size} guard elements in front of the body and {after.size} behind it were overwritten; "
                             f"offsets from the body's start {(before[:8] - a.lo).tolist()}, from its end {after[:8].tolist()}")


def check_written(a: Arena, what: str = "", defined=None) -> None:
    """no body element (of those ``defined`` marks, all by default) still holds the sentinel"""
    left = a.ints()[a.lo:a.hi] == a.sentinel
    if defined is not None:
        left &= np.asarray(defined, dtype=bool).reshape(-1)
    if left.any():
        idx = np.flatnonzero(left)
        raise AssertionError(f"{what}: {idx.size} of {left.size} body elements were never written; first {idx[:8].tolist()}")


def check_untouched(a: Arena, what: str = "") -> None:
    """body and guards all still hold the sentinel (a call that was rejected wrote nothing)"""
    bad = np.flatnonzero(a.ints() != a.sentinel)
    if bad.size:
        raise AssertionError(f"{what}: {bad.size} elements were written by a rejected call; first at {(bad[:8] - a.lo).tolist()} from the body's start")


class ArenaAllocator:
    """Stands in for ``Engine._alloc``: every output is the body of a sentinel-filled arena.  ``begin()`` before a call re-arms the
    arenas of the previous call and hands them out again in the same order, so that two calls write into the same guarded buffers."""

    def __init__(self):
        self.arenas: List[Arena] = []
        self._next = 0

    def begin(self, fresh: bool = False) -> None:
        if fresh:
            self.arenas = []
        self._next = 0
        for a in self.arenas:
            a.fill_sentinel()

    def __call__(self, dev, dt, shape, like=None):
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        dt = _numpy_dtype(dt)
        if self._next < len(self.arenas):
            a = self.arenas[self._next]
            assert (a.shape, a.dtype, a.device) == (shape, dt, bool(dev)), "begin(fresh=True) before a call of another shape"
        else:
            a = Arena(shape, dt, device=bool(dev))
            self.arenas.append(a)
        self._next += 1
        return a.body

    def used(self) -> List[Arena]:
        return self.arenas[:self._next]

    def check(self, what: str = "") -> None:
        for i, a in enumerate(self.used()):
            tag = f"{what} output #{i} {a.dtype} {a.shape}"
            check_guards(a, tag)
            check_written(a, tag)


def arena_engine(device: int = 0):
    """an Engine whose outputs come from an ArenaAllocator (``eng.arena``)"""
    from polars_ols_amd import Engine

    eng = Engine(device)
    eng.arena = ArenaAllocator()
    eng._alloc = eng.arena                    # instance attribute: shadows the method for this engine only
    return eng


class Frame:
    """A group-sorted frame whose every column is an input arena: ``y``, ``cols``, optional ``w`` (weights), ``valid`` (uint8) and
    any further float columns in ``extra`` (a GLM offset, instruments, further targets).  ``guards(fill)`` re-fills every float
    column's guards; the validity bytes get 0 where the floats get NaN and 1 otherwise."""

    def __init__(self, y, cols: Sequence, offs, w=None, valid=None, extra: Optional[Dict[str, Sequence]] = None, device: bool = True,
                 fill=np.nan):
        self.offs = np.asarray(offs, dtype=np.int64)
        self.np = {"y": np.asarray(y), "cols": [np.asarray(c) for c in cols], "w": None if w is None else np.asarray(w),
                   "valid": None if valid is None else np.asarray(valid, dtype=np.uint8),
                   "extra": {k: [np.asarray(c) for c in v] for k, v in (extra or {}).items()}}
        mk = lambda a: input_arena(a, fill, device=device)  # noqa: E731
        self._y = mk(self.np["y"])
        self._cols = [mk(c) for c in self.np["cols"]]
        self._w = mk(self.np["w"]) if w is not None else None
        self._valid = input_arena(self.np["valid"], 0, device=device) if valid is not None else None
        self._extra = {k: [mk(c) for c in v] for k, v in self.np["extra"].items()}
        self.guards(fill)

    def floats(self) -> List[Arena]:
        out = [self._y] + self._cols + ([self._w] if self._w is not None else [])
        for v in self._extra.values():
            out += v
        return out

    def guards(self, fill) -> "Frame":
        for a in self.floats():
            a.fill_guards(fill)
        if self._valid is not None:
            self._valid.fill_guards(0 if fill != fill else 1)
        return self

    def load(self, y=None, cols=None, w=None, extra: Optional[Dict[str, Sequence]] = None) -> "Frame":
        """overwrite column bodies in place (same arenas, same addresses); None leaves a column as it is"""
        if y is not None:
            self._y.set_body(y)
        for a, c in zip(self._cols, cols or []):
            a.set_body(c)
        if w is not None:
            self._w.set_body(w)
        for k, v in (extra or {}).items():
            for a, c in zip(self._extra[k], v):
                a.set_body(c)
        return self

    y = property(lambda self: self._y.body)
    cols = property(lambda self: [a.body for a in self._cols])
    w = property(lambda self: None if self._w is None else self._w.body)
    valid = property(lambda self: None if self._valid is None else self._valid.body)

    def extra(self, key) -> list:
        return [a.body for a in self._extra[key]]


def bits(a) -> np.ndarray:
    """an output (numpy or torch, any of the arena dtypes) as integers on the host, for bit comparisons"""
    a = a.detach().cpu().numpy() if (torch is not None and isinstance(a, torch.Tensor)) else np.asarray(a)
    return np.ascontiguousarray(a).view(SENTINELS[a.dtype][0])


def f64(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if (torch is not None and isinstance(a, torch.Tensor)) else np.asarray(a)
    return a.astype(np.float64) if a.dtype.kind == "f" else a
