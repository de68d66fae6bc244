"""A guarded arena for footprint tests (a helper module, not a conftest).

The parity suite compares `[0, w) x h` of every output plane with the oracle. This module checks the rest of the
contract that include/vszip_hip.h states next to `vszip_plane` ("Plane memory: what a call reads and writes"):

  * one allocation per case, filled completely with a poison byte; the case's planes are carved out of it, each with
    a guard band before and after it, so an overrun lands in memory the test owns and is seen, never faulted on;
  * after the call the whole arena comes back in one copy and is compared byte for byte with the image the contract
    predicts: poison everywhere, inputs (and the live neighbours of a window) as uploaded, `[0, w) x h` of each
    output equal to the oracle;
  * every case runs twice, with poison 0x00 and 0xFF (0xFF.. is a NaN in f16 / f32 and the peak of every integer
    type) and identical inputs inside `[0, w) x h`; outputs and scalars of the two runs must be bit-identical.

How the guard is sized. The widest single access in csrc/ is 16 bytes a lane (dwordx4 / uint4, 16 u8 or 8 u16
samples), 1 KiB for a wave of 64 lanes; the ring kernels' halo lanes and the tile kernels' aprons reach at most one
such lane group left and right of a row, and the row-direction halos (BoxBlur radius, Bilateral radius, EEDI3's four
cubic rows, CLAHE's tile rows) are clamped to rows of the plane, so the furthest plausible stray access is a few rows
of the widest plane or a wave's worth of vector lanes. The guard is therefore

    max(4 KiB, GUARD_ROWS (= 8) rows of the widest pitch in the case), rounded up to 256 bytes,

before the first plane, between any two, and after the last: four waves of 16-byte lanes, or eight whole rows,
whichever is more. An access further out than that is not a tail or halo mistake but a wrong pointer, and the
allocation is sized so that even `h x pitch` of a window plane (which starts x0 samples into its parent) stays inside.

The arena talks to memory through four operations (alloc, fill, copy_in, copy_out). `DeviceBackend` does them with
the library's own vszip_dev_alloc / vszip_dev_memset / vszip_copy_*; `NumpyBackend` is host memory, so that the
checker itself is tested without a GPU (tests/test_guarded_cpu.py).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

GUARD_MIN = 4096
GUARD_ROWS = 8
SLOT_ALIGN = 256  # hipMalloc's alignment: what every other test's planes start at
POISONS = (0x00, 0xFF)

# Clause 3 of the header's contract ("Written extent") is strict: a call writes [0, w) of each of an output's h
# rows and nothing else. Were it ever to grant the one exception the contract allows (stores up to the end of the
# 16-byte group that holds column w - 1, inside the row's own pitch, only for a 16-byte aligned base and pitch),
# this is the only switch: the exemption below is computed from that rule, never per kernel.
TAIL_GROUP_GRANTED = False


class FootprintError(AssertionError):
    pass


@dataclass
class PlaneSpec:
    """One plane of a case.

    role     "in" (uploaded, must come back unchanged), "out" (starts as poison, or as the parent's live samples for
             a window; must come back as `expect`), "inout" (dst == src: uploaded, must come back as `expect`)
    pitch    row pitch in samples (>= w, or >= the parent's width for a window)
    shift    bytes added to the plane's 256-byte aligned slot (base alignment)
    data     (h, w) samples of an "in" / "inout" plane
    window   None, or (H, W, y0, x0): the plane is [y0:y0+h, x0:x0+w] of a larger H x W picture with the same pitch,
             whose other samples hold `neighbours` (live content that a call must neither depend on nor change)
    poison_rows  rows of an input that are NOT inputs of the call (EEDI3 with dh = 0: the rows of parity `field`):
             they hold poison instead of `data`
    """
    name: str
    role: str
    h: int
    w: int
    dtype: object
    pitch: int
    shift: int = 0
    data: np.ndarray | None = None
    window: tuple | None = None
    neighbours: np.ndarray | None = None
    poison_rows: tuple = ()
    # filled in by Arena
    base: int = field(default=0, repr=False)     # byte offset of sample (0, 0) in the arena
    region: tuple = field(default=(0, 0), repr=False)  # [start, end) bytes of the memory the case declares for this plane

    def __post_init__(self):
        self.dtype = np.dtype(self.dtype)
        assert self.role in ("in", "out", "inout")
        if self.window is None:
            assert self.pitch >= self.w
        else:
            H, W, y0, x0 = self.window
            assert self.pitch >= W and y0 + self.h < H and x0 + self.w <= W  # < H: h x pitch from the window's base stays in the parent
        if self.role != "out":
            assert self.data is not None and self.data.shape == (self.h, self.w) and self.data.dtype == self.dtype

    @property
    def isz(self) -> int:
        return self.dtype.itemsize

    @property
    def pitch_bytes(self) -> int:
        return self.pitch * self.isz

    def aligned16(self, arena_ptr: int) -> bool:
        return (arena_ptr + self.base) % 16 == 0 and self.pitch_bytes % 16 == 0


class NumpyBackend:
    """Host memory behind the arena's four operations: the checker's own test bed."""

    def alloc(self, nbytes: int) -> int:
        raw = np.empty(nbytes + SLOT_ALIGN, np.uint8)
        off = (-raw.ctypes.data) % SLOT_ALIGN
        self._raw, self.mem = raw, raw[off:off + nbytes]
        return self.mem.ctypes.data

    def fill(self, byte: int):
        self.mem[:] = byte

    def copy_in(self, image: np.ndarray):
        self.mem[:] = image

    def copy_out(self) -> np.ndarray:
        return self.mem.copy()

    def free(self):
        self.mem = self._raw = None


class DeviceBackend:
    """Device memory through the library's own allocation and copy entry points (a request this small is far below
    VSZIP_PLACEMENT_MIN_MIB: a plain hipMalloc)."""

    def __init__(self, dev):
        self.dev, self.ptr, self.n = dev, None, 0

    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self.dev.check(self.dev.lib.vszip_dev_alloc(self.dev.ctx, nbytes, C.byref(p)))
        self.ptr, self.n = p.value, nbytes
        return self.ptr

    def fill(self, byte: int):
        self.dev.check(self.dev.lib.vszip_dev_memset(self.dev.ctx, C.c_void_p(self.ptr), byte, self.n))
        self.dev.sync()

    def copy_in(self, image: np.ndarray):
        assert image.dtype == np.uint8 and image.size == self.n and image.flags.c_contiguous
        self.dev.check(self.dev.lib.vszip_copy_h2d_2d(self.dev.ctx, C.c_void_p(self.ptr), self.n, image.ctypes.data, self.n, self.n, 1))
        self.dev.sync()

    def copy_out(self) -> np.ndarray:
        out = np.empty(self.n, np.uint8)
        self.dev.sync()
        self.dev.check(self.dev.lib.vszip_copy_d2h_2d(self.dev.ctx, out.ctypes.data, self.n, C.c_void_p(self.ptr), self.n, self.n, 1))
        self.dev.sync()
        return out

    def free(self):
        if self.ptr:
            self.dev.sync()
            self.dev.lib.vszip_dev_free(self.dev.ctx, C.c_void_p(self.ptr))
            self.ptr = None


def _up(n: int, a: int) -> int:
    return -(-n // a) * a


class Arena:
    """One allocation holding every plane of a case in the order given, guards in between."""

    def __init__(self, backend, specs, poison: int):
        self.backend, self.specs, self.poison = backend, list(specs), poison
        assert len({s.name for s in self.specs}) == len(self.specs)
        widest = max(s.pitch_bytes for s in self.specs)
        self.guard = _up(max(GUARD_MIN, GUARD_ROWS * widest), SLOT_ALIGN)
        off = self.guard
        for s in self.specs:
            assert 0 <= s.shift < SLOT_ALIGN
            start = off + s.shift
            if s.window is None:
                s.base = start
                nbytes = s.h * s.pitch_bytes  # what the contract says the caller owns: h x stride
            else:
                H, W, y0, x0 = s.window
                s.base = start + (y0 * s.pitch + x0) * s.isz
                nbytes = H * s.pitch_bytes
            s.region = (start, start + nbytes)
            off = _up(start + nbytes, SLOT_ALIGN) + self.guard
        self.nbytes = off
        self.ptr = backend.alloc(self.nbytes)
        backend.fill(poison)
        self.image = np.full(self.nbytes, poison, np.uint8)  # what was uploaded
        for s in self.specs:
            if s.window is not None:
                H, W, y0, x0 = s.window
                assert s.neighbours is not None and s.neighbours.shape == (H, W) and s.neighbours.dtype == s.dtype
                self._rows(self.image, s.region[0], s.pitch_bytes, H, W * s.isz)[:] = s.neighbours.view(np.uint8).reshape(H, W * s.isz)
            if s.role != "out":
                v = self._rows(self.image, s.base, s.pitch_bytes, s.h, s.w * s.isz)
                v[:] = np.ascontiguousarray(s.data).view(np.uint8).reshape(s.h, s.w * s.isz)
                for r in s.poison_rows:
                    v[r] = poison
        backend.copy_in(self.image)

    @staticmethod
    def _rows(image: np.ndarray, base: int, pitch_bytes: int, h: int, wbytes: int) -> np.ndarray:
        """writable (h, wbytes) byte view of a pitched plane inside the image"""
        return np.lib.stride_tricks.as_strided(image[base:], shape=(h, wbytes), strides=(pitch_bytes, 1))

    def address(self, name: str) -> int:
        return self.ptr + self.spec(name).base

    def spec(self, name: str) -> PlaneSpec:
        return next(s for s in self.specs if s.name == name)

    def close(self):
        self.backend.free()

    # -- the check ------------------------------------------------------------
    def _where(self, s: PlaneSpec, byte: int) -> str:
        off = byte - s.base
        end = s.h * s.pitch_bytes
        if off < 0:
            return f"{-off} bytes before the plane"
        if off >= end:
            return f"{off - end + 1} bytes past the end (h x stride = {end} bytes)"
        row, col = off // s.pitch_bytes, (off % s.pitch_bytes) // s.isz
        return f"row {row}, column {col}" + ("" if col < s.w else f" (outside w = {s.w}, pitch {s.pitch})")

    def _nearest(self, byte: int) -> PlaneSpec:
        def dist(s):
            lo, hi = s.region
            return 0 if lo <= byte < hi else (lo - byte if byte < lo else byte - hi + 1)
        return min(self.specs, key=dist)

    def check(self, got: np.ndarray, expect: dict, grant_tail: bool = TAIL_GROUP_GRANTED, same=None) -> dict:
        """Compare the arena after the call with what the contract predicts. expect: name -> (h, w) oracle output of every
        "out" / "inout" plane. same(name, got, want) -> bool replaces bit equality for one output (a filter whose
        neighbouring test module compares with a tolerance); there is none today. -> name -> (h, w) output as read back."""
        assert got.dtype == np.uint8 and got.size == self.nbytes
        want = self.image.copy()
        care = np.ones(self.nbytes, bool)
        outs = {}
        for s in self.specs:
            if s.role == "in":
                continue
            wb = s.w * s.isz
            self._rows(care, s.base, s.pitch_bytes, s.h, wb)[:] = False  # judged against the oracle below
            outs[s.name] = np.ascontiguousarray(self._rows(got, s.base, s.pitch_bytes, s.h, wb)).view(s.dtype).reshape(s.h, s.w)
            if grant_tail and s.aligned16(self.ptr):
                tail = min(_up(wb, 16), s.pitch_bytes) - wb
                if tail > 0:
                    np.lib.stride_tricks.as_strided(care[s.base + wb:], shape=(s.h, tail), strides=(s.pitch_bytes, 1))[:] = False
        bad = np.flatnonzero((got != want) & care)
        if bad.size:
            first = int(bad[0])
            s = self._nearest(first)
            inside = s.role == "in" and 0 <= first - s.base < s.h * s.pitch_bytes and ((first - s.base) % s.pitch_bytes) < s.w * s.isz
            what = "input plane modified" if inside else "write outside [0, w) x h"
            raise FootprintError(f"plane '{s.name}' ({s.role}, {s.h}x{s.w} {s.dtype}, pitch {s.pitch}, base % 16 = {(self.ptr + s.base) % 16}): {what}: "
                                 f"first at {self._where(s, first)}; {bad.size} bytes differ (poison 0x{self.poison:02X}, "
                                 f"found 0x{int(got[first]):02X}, expected 0x{int(want[first]):02X})")
        for s in self.specs:
            if s.role == "in":
                continue
            assert s.name in expect, f"no expected output for plane '{s.name}'"
            g, e = outs[s.name], np.ascontiguousarray(expect[s.name])
            assert e.shape == g.shape and e.dtype == g.dtype, (s.name, e.shape, e.dtype)
            ok = same(s.name, g, e) if same is not None else np.array_equal(g.view(np.uint8), e.view(np.uint8))
            if not ok:
                d = np.argwhere(g.view(np.uint8).reshape(s.h, -1) != e.view(np.uint8).reshape(s.h, -1))
                r, c = int(d[0][0]), int(d[0][1]) // s.isz
                raise FootprintError(f"plane '{s.name}' ({s.h}x{s.w} {s.dtype}, pitch {s.pitch}, base % 16 = {(self.ptr + s.base) % 16}): output differs from the "
                                     f"oracle: first at row {r}, column {c}; {len(d)} bytes differ (poison 0x{self.poison:02X})")
        return outs


def _scalars_bits(v):
    """scalars of a call as bytes, so that two runs compare bit for bit (NaN == NaN, -0.0 != 0.0)"""
    if v is None:
        return b""
    return np.asarray(v, np.float64).tobytes() if not isinstance(v, (bytes, bytearray)) else bytes(v)


def run_case(make_backend, make_specs, call, expect, grant_tail: bool = TAIL_GROUP_GRANTED, check_scalars=None, same=None):
    """The whole protocol for one case.

    make_backend()            -> a fresh backend (one allocation per run)
    make_specs()              -> the case's PlaneSpecs, in arena order (called once per run: same inputs both times)
    call(arena)               -> runs the filter on arena.address(name) pointers; returns its scalars or None
    expect                    name -> oracle output for every "out" / "inout" plane (or a callable(specs) -> such a dict)
    check_scalars(scalars)    asserts the returned scalars against the oracle (readers)
    """
    runs = []
    for poison in POISONS:
        specs = make_specs()
        arena = Arena(make_backend(), specs, poison)
        try:
            scalars = call(arena)
            got = arena.backend.copy_out()
        finally:
            arena.close()
        exp = expect(specs) if callable(expect) else expect
        outs = arena.check(got, exp, grant_tail, same)
        if check_scalars is not None:
            check_scalars(scalars)
        runs.append((outs, _scalars_bits(scalars), scalars))
    (o0, s0, v0), (o1, s1, v1) = runs
    for name in o0:
        a, b = o0[name].view(np.uint8), o1[name].view(np.uint8)
        if not np.array_equal(a, b):
            s = next(x for x in specs if x.name == name)
            d = np.argwhere(a.reshape(s.h, -1) != b.reshape(s.h, -1))
            raise FootprintError(f"plane '{name}': output depends on bytes outside [0, w) x h of the inputs: poison 0x00 and 0xFF give different "
                                 f"samples, first at row {int(d[0][0])}, column {int(d[0][1]) // s.isz}; {len(d)} bytes differ")
    if s0 != s1:
        raise FootprintError(f"scalars depend on bytes outside [0, w) x h of the inputs: {v0!r} under poison 0x00, {v1!r} under 0xFF")
    return runs[0][0], v0
