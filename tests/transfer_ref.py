"""The transfer function of include/cvr.h restated in numpy fp32, independent of the library, and
the media of the transfer tests (tests/test_transfer_cpu.py, tests/test_gpu_transfer.py).

classify() is the written statement: every operation is a separate float32 numpy call, so nothing
is fused, and the results are the bits cvr_classify_host and the build kernels must return.  (Where
a table entry is NaN, linear interpolation yields a NaN whose sign and payload IEEE 754 leaves
open: same_bits() lets two NaNs be equal there and compares every other value's bits.)"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import devmed
import media

f32 = np.float32


def classify(scalar, table, lo, hi, ceil=False, density_u=False):
    """(density scalar.shape, albedo scalar.shape + (4,)) of a u8 / u16 / i16 / f32 array."""
    s = np.asarray(scalar).astype(np.float32)          # exact for the integer types
    table = np.asarray(table, np.float32)
    n = table.shape[0]
    with np.errstate(all="ignore"):
        t = (s - f32(lo)) / (f32(hi) - f32(lo))
        u = np.where(t > f32(0), t, f32(0)).astype(np.float32)   # NaN > 0 is false: 0
        u = np.where(u < f32(1), u, f32(1)).astype(np.float32)
        x = u * f32(n - 1)
        if ceil:
            i = np.minimum(np.ceil(x).astype(np.int64), n - 1)
            e = table[i]
        else:
            i = np.minimum(np.floor(x).astype(np.int64), n - 2)
            fr = (x - i.astype(np.float32))[..., None]
            a, b = table[i], table[i + 1]
            d = b - a
            p = fr * d
            e = a + p
    e = e.astype(np.float32)
    albedo = np.ones(s.shape + (4,), np.float32)
    albedo[..., :3] = e[..., :3]
    density = u if density_u else e[..., 3]
    return np.ascontiguousarray(density, np.float32), albedo


def same_bits(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(((got.view(np.uint32) == want.view(np.uint32)) | both_nan).all())


# ------------------------------------------------------------------- cases --
# scalar: (z, y, x) array; the medium's box and scale; sparse: built with CVR_DEVMED_SPARSE.
Case = namedtuple("Case", "scalar table lo hi ceil density_u box_min box_max scale sparse")
UNIT = ((-0.5,) * 3, (0.5,) * 3)


def table7(seed=41, zero_first=False):
    """7 entries: random colours, densities rising from 0.05 (or 0) to 1."""
    rng = np.random.default_rng(seed)
    t = np.empty((7, 4), np.float32)
    t[:, :3] = 0.2 + 0.8 * rng.random((7, 3), dtype=np.float32)
    t[:, 3] = np.linspace(0.0 if zero_first else 0.05, 1.0, 7, dtype=np.float32)
    return t


def quantise(d, dtype):
    """The density of a medium in [0, 1] as u8, u16 or i16 (zeros stay the type's lowest code)."""
    if dtype == np.uint8:
        return np.rint(d * f32(255)).astype(np.uint8)
    q = np.rint(d.astype(np.float64) * 65535).astype(np.int64)
    return q.astype(np.uint16) if dtype == np.uint16 else (q - 32768).astype(np.int16)


def planted_u16(name):
    """The planted grid of devmed.sparse_grid(name) as u16: zero, -0 and NaN voxels are code 0,
    every positive voxel a code >= 1; voxel (0,0,0), whose albedo is the background, is code 0."""
    D, _, md = devmed.sparse_grid(name, True)
    with np.errstate(invalid="ignore"):
        pos = D > 0
    q = np.zeros(D.shape, np.uint16)
    q[pos] = np.maximum(np.ceil(D[pos].astype(np.float64) / float(D[pos].max()) * 65535), 1).astype(np.uint16)
    q[0, 0, 0] = 0
    return q


def _sparse_table(kind):
    t = table7(43, zero_first=True)
    if kind == "zero":        # entry 0: density 0, the background's colour
        pass
    elif kind == "dense":     # entry 0 has a density: every voxel does, every leaf exists
        t[0, 3] = f32(0.02)
    else:                     # one colour: no leaf differs through its albedo, no albedo pool
        t[:, :3] = np.array([0.8, 0.6, 0.4], np.float32)
    return t


def _random40(dtype, lo, hi, table=None, ceil=False):
    m = media.random40()
    return Case(quantise(m.density, dtype), table7() if table is None else table, lo, hi, ceil, False, *UNIT, m.scale,
                False)


def _ramp4096():
    """16^3 u16 voxels, voxel k = 16 k, and a 4096-entry table over 0 .. 16 * 4095: voxel k lands
    on entry k (or an ulp beside it), so every entry is read."""
    k = np.arange(4096, dtype=np.uint32)
    rng = np.random.default_rng(47)
    t = np.empty((4096, 4), np.float32)
    t[:, :3] = 0.2 + 0.8 * rng.random((4096, 3), dtype=np.float32)
    t[:, 3] = rng.random(4096, dtype=np.float32)
    return Case((k * 16).astype(np.uint16).reshape(16, 16, 16), t, 0.0, 16.0 * 4095, False, False, *UNIT, 40.0, False)


def _unaligned(dtype):
    rng = np.random.default_rng(53)
    hi = 255 if dtype == np.uint8 else 65535
    s = rng.integers(0, hi + 1, (5, 7, 13)).astype(dtype)
    s[rng.random(s.shape) < 0.3] = 0
    return Case(s, table7(), 0.1 * hi, 0.9 * hi, False, False, *UNIT, media.SCALE, False)


def _f32(m, lo, hi):
    return Case(m.density, table7(), lo, hi, False, False, m.box_min, m.box_max, m.scale, False)


def _uniform_rgb():
    t = table7()
    t[:, :3] = np.array([0.9, 0.55, 0.3], np.float32)
    return _random40(np.uint8, 0.0, 255.0, t)


def _bucky():
    import cudavolumerenderer_amd as cvr
    sc = cvr.Scene.synthetic("bucky")
    raw = np.frombuffer(sc.raw_bytes, np.uint8).reshape(32, 32, 32).copy()
    md = sc.medium
    c = Case(raw, cvr.raw_transfer_table(), 0.0, float(raw.max()), True, True, tuple(md.box_min), tuple(md.box_max),
             float(md.scale), False)
    sc.close()
    return c


def _sparse(name, kind):
    return Case(planted_u16(name), _sparse_table(kind), 0.0, 65535.0, False, False, *UNIT, media.SCALE, True)


CASES = {
    "spikes_f32": lambda: _f32(media.spikes(), 0.01, 0.6),      # both clamps occur (asserted on the CPU)
    "offgrid_f32": lambda: _f32(media.offgrid(), 0.1, 0.8),
    "random40_u8": lambda: _random40(np.uint8, 10.0, 240.0),
    "random40_u16": lambda: _random40(np.uint16, 1000.0, 60000.0),
    "random40_i16": lambda: _random40(np.int16, -30000.0, 30000.0),
    "unaligned_u8": lambda: _unaligned(np.uint8),
    "unaligned_u16": lambda: _unaligned(np.uint16),
    "ramp4096_u16": _ramp4096,
    "two_entries": lambda: _random40(np.uint8, 0.0, 255.0, table7()[[0, 6]]),
    "two_entries_ceil": lambda: _random40(np.uint8, 0.0, 255.0, table7()[[0, 6]], ceil=True),
    "uniform_rgb": _uniform_rgb,
    "bucky": _bucky,
    "sparse_small_zero": lambda: _sparse("sparse_small", "zero"),
    "sparse_es4_zero": lambda: _sparse("sparse_es4", "zero"),
    "sparse_small_dense": lambda: _sparse("sparse_small", "dense"),
    "sparse_small_one_colour": lambda: _sparse("sparse_small", "one_colour"),
}
# byte offset of the scalar tensor into its allocation (the unaligned head and tail)
OFFSET = {"unaligned_u8": 1, "unaligned_u16": 2}


@lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@lru_cache(maxsize=None)
def classified(name):
    """(density, albedo, max density) of a case by the numpy statement; computed once."""
    c = case(name)
    d, a = classify(c.scalar, c.table, c.lo, c.hi, c.ceil, c.density_u)
    d.setflags(write=False)
    a.setflags(write=False)
    return d, a, float(np.nanmax(np.maximum(d, 0)))


@lru_cache(maxsize=None)
def reference(name, fmt):
    """The oracle's records over the classified arrays as format fmt stores them; computed once."""
    c = case(name)
    d, a, md = classified(name)
    return devmed.oracle_records(d, a, md, fmt, c.box_min, c.box_max, c.scale)
