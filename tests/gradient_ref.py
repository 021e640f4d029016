"""The gradient-magnitude transfer function of include/cvr.h restated in numpy fp32, independent
of the library, and the media of its tests (tests/test_gradient_transfer_cpu.py,
tests/test_gpu_gradient_transfer.py).

classify() is the written statement: every operation is a separate float32 numpy call, so nothing
is fused, and the results are the bits cvr_classify_gradient_host and the build kernels must
return (numpy's float32 sqrt and divide are correctly rounded).  same_bits, table7 and quantise
are tests/transfer_ref.py's."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import devmed
import media
from transfer_ref import UNIT, quantise, same_bits, table7  # noqa: F401  (re-exported)

f32 = np.float32


def _axis(S, axis, h1, h2):
    """One gradient component: (S(p) - S(m)) * k along `axis`, k the central factor where both
    neighbours exist and the one-sided one on a face."""
    n = S.shape[axis]
    c = np.arange(n)
    cm = np.where(c > 0, c - 1, c)
    cp = np.where(c + 1 < n, c + 1, c)
    k = np.where(cp - cm == 2, f32(h2), f32(h1)).astype(np.float32)
    shape = [1, 1, 1]
    shape[axis] = n
    diff = np.take(S, cp, axis=axis) - np.take(S, cm, axis=axis)
    return (diff * k.reshape(shape)).astype(np.float32)


def magnitude(scalar, spacing=(1.0, 1.0, 1.0)):
    S = np.asarray(scalar).astype(np.float32)              # exact for the integer types
    sx, sy, sz = (f32(v) for v in spacing)
    with np.errstate(all="ignore"):
        gx = _axis(S, 2, f32(1) / sx, f32(0.5) / sx)
        gy = _axis(S, 1, f32(1) / sy, f32(0.5) / sy)
        gz = _axis(S, 0, f32(1) / sz, f32(0.5) / sz)
        xx, yy, zz = gx * gx, gy * gy, gz * gz
        q = (xx + yy) + zz
        return np.sqrt(q).astype(np.float32)


def coordinates(scalar, table, lo, hi, glo, ghi, spacing=(1.0, 1.0, 1.0)):
    """(u, v, i, j, f, h, magnitude) of every voxel."""
    S = np.asarray(scalar).astype(np.float32)
    m, n = np.asarray(table).shape[:2]
    mag = magnitude(scalar, spacing)
    with np.errstate(all="ignore"):
        t = (S - f32(lo)) / (f32(hi) - f32(lo))
        u = np.where(t > f32(0), t, f32(0)).astype(np.float32)   # NaN > 0 is false: 0
        u = np.where(u < f32(1), u, f32(1)).astype(np.float32)
        w = (mag - f32(glo)) / (f32(ghi) - f32(glo))
        v = np.where(w > f32(0), w, f32(0)).astype(np.float32)
        v = np.where(v < f32(1), v, f32(1)).astype(np.float32)
        xt = u * f32(n - 1)
        yt = v * f32(m - 1)
        i = np.minimum(np.floor(xt).astype(np.int64), n - 2)
        j = np.minimum(np.floor(yt).astype(np.int64), m - 2)
        f = xt - i.astype(np.float32)
        h = yt - j.astype(np.float32)
    return u, v, i, j, f.astype(np.float32), h.astype(np.float32), mag


def classify(scalar, table, lo, hi, glo, ghi, spacing=(1.0, 1.0, 1.0)):
    """(density, albedo, magnitude) of a (z, y, x) u8 / u16 / i16 / f32 array; table (m, n, 4)."""
    table = np.asarray(table, np.float32)
    _, _, i, j, f, h, mag = coordinates(scalar, table, lo, hi, glo, ghi, spacing)
    f, h = f[..., None], h[..., None]
    with np.errstate(all="ignore"):
        P, Q, R, W = table[j, i], table[j, i + 1], table[j + 1, i], table[j + 1, i + 1]
        d = Q - P
        p = f * d
        a = P + p
        d = W - R
        p = f * d
        b = R + p
        d = b - a
        p = h * d
        e = (a + p).astype(np.float32)
    albedo = np.ones(mag.shape + (4,), np.float32)
    albedo[..., :3] = e[..., :3]
    return np.ascontiguousarray(e[..., 3], np.float32), albedo, mag


# ------------------------------------------------------------------- cases --
# scalar: (z, y, x); table (m, n, 4); sparse: built with CVR_DEVMED_SPARSE.
Case = namedtuple("Case", "scalar table lo hi glo ghi spacing box_min box_max scale sparse")


def table2d(m=5, n=7, seed=61, zero_first=False):
    """m rows of n entries: random colours, densities rising along both axes from 0.05 (or 0 at
    entry (0, 0)) to 1."""
    rng = np.random.default_rng(seed)
    t = np.empty((m, n, 4), np.float32)
    t[..., :3] = 0.2 + 0.8 * rng.random((m, n, 3), dtype=np.float32)
    t[..., 3] = np.linspace(0.05, 1.0, m * n, dtype=np.float32).reshape(m, n)
    if zero_first:
        t[0, 0, 3] = 0.0
    return t


def _random40(dtype, lo, hi, ghi):
    m = media.random40()
    return Case(quantise(m.density, dtype), table2d(), lo, hi, 0.0, ghi, (1.0, 1.0, 1.0), *UNIT, m.scale, False)


def _offgrid():
    m = media.offgrid()
    return Case(m.density, table2d(), 0.1, 0.8, 0.02, 0.4, (1.0, 0.5, 2.0), m.box_min, m.box_max, m.scale, False)


def _thin(shape, dtype, seed=67):
    """A field with short axes: random codes, about a third zeros."""
    rng = np.random.default_rng(seed)
    top = 255 if dtype == np.uint8 else 65535
    s = rng.integers(0, top + 1, shape).astype(dtype)
    s[rng.random(shape) < 0.3] = 0
    return Case(s, table2d(), 0.1 * top, 0.9 * top, 0.05 * top, 0.8 * top, (1.0, 1.0, 1.0), *UNIT, media.SCALE, False)


def _nonfinite():
    """f32 11 x 9 x 10 with one NaN, one +inf and one -inf voxel, apart from each other."""
    rng = np.random.default_rng(71)
    s = rng.random((11, 9, 10), dtype=np.float32)
    s[rng.random(s.shape) < 0.3] = 0.0
    s[2, 2, 2] = np.nan
    s[5, 5, 5] = np.inf
    s[8, 6, 3] = -np.inf
    return Case(s, table2d(), 0.1, 0.8, 0.05, 0.45, (1.0, 1.0, 1.0), *UNIT, media.SCALE, False)


def _full_lds():
    """n * m = 4096 (n 128, m 32) on a 16^3 u16 field: smooth ramps (small gradients, every value)
    and random voxels (large gradients), with the extreme codes planted so that the first and the
    last cell of both table axes are read."""
    rng = np.random.default_rng(73)
    z, y, x = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    s = (x * 4000 + y * 200 + z * 10).astype(np.uint16)
    noisy = rng.random(s.shape) < 0.3
    s[noisy] = rng.integers(0, 65536, int(noisy.sum())).astype(np.uint16)
    s[0:3, 0:3, 0:3] = 0            # a constant corner: value 0, gradient 0 at (0, 0, 0)
    s[13:16, 13:16, 13:16] = 65535  # the same at the far corner: value 65535, gradient 0
    t = np.empty((32, 128, 4), np.float32)
    t[..., :3] = 0.2 + 0.8 * rng.random((32, 128, 3), dtype=np.float32)
    t[..., 3] = 0.05 + 0.95 * rng.random((32, 128), dtype=np.float32)
    return Case(s, t, 0.0, 65535.0, 0.0, 20000.0, (1.0, 1.0, 1.0), *UNIT, 40.0, False)


def halo_field():
    """(z, y, x) = (24, 24, 21) u16, all zero except voxel (x, y, z) = (7, 7, 7) = 65535."""
    s = np.zeros((24, 24, 21), np.uint16)
    s[7, 7, 7] = 65535
    return s


def _halo(kind):
    t = table2d(seed=79, zero_first=True)   # entry (0, 0): density 0; every other entry > 0
    if kind == "one_colour":
        t[..., :3] = np.array([0.8, 0.6, 0.4], np.float32)
    elif kind == "positive":
        t[0, 0, 3] = f32(0.02)
    # glo 0: only a voxel of value 0 and gradient exactly 0 takes entry (0, 0) alone
    return Case(halo_field(), t, 0.0, 65535.0, 0.0, 40000.0, (1.0, 1.0, 1.0), *UNIT, media.SCALE, True)


CASES = {
    "random40_u8": lambda: _random40(np.uint8, 10.0, 240.0, 150.0),
    "random40_u16": lambda: _random40(np.uint16, 1000.0, 60000.0, 40000.0),
    "random40_i16": lambda: _random40(np.int16, -30000.0, 30000.0, 40000.0),
    "offgrid_f32": _offgrid,
    "thin523_u8": lambda: _thin((3, 5, 523), np.uint8),
    "thin523_u16": lambda: _thin((3, 5, 523), np.uint16),
    "two_planes_u16": lambda: _thin((2, 9, 33), np.uint16),
    "one_plane_u8": lambda: _thin((1, 9, 33), np.uint8),
    "one_column_u8": lambda: _thin((9, 33, 1), np.uint8),
    "nonfinite_f32": _nonfinite,
    "full_lds_u16": _full_lds,
    "halo": lambda: _halo("zero"),
    "halo_one_colour": lambda: _halo("one_colour"),
    "halo_positive": lambda: _halo("positive"),
}
# byte offset of the scalar tensor into its allocation (the unaligned head and tail)
OFFSET = {"thin523_u8": 1, "thin523_u16": 2}
# the host statement is compared with the restatement on these shapes too (CPU only)
THIN_SHAPES = [(1, 9, 33), (9, 1, 33), (9, 33, 1), (2, 9, 33), (3, 5, 523)]


@lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@lru_cache(maxsize=None)
def classified(name):
    """(density, albedo, max density) of a case by the numpy statement; computed once."""
    c = case(name)
    d, a, _ = classify(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)
    d.setflags(write=False)
    a.setflags(write=False)
    with np.errstate(invalid="ignore"):
        return d, a, float(np.nanmax(np.maximum(d, 0)))


@lru_cache(maxsize=None)
def reference(name, fmt):
    """The oracle's records over the classified arrays as format fmt stores them; computed once."""
    c = case(name)
    d, a, md = classified(name)
    return devmed.oracle_records(d, a, md, fmt, c.box_min, c.box_max, c.scale)
