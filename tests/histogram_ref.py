"""The field statistics and value-gradient histograms of include/cvr.h restated in numpy fp32,
independent of the library, and the fields of their tests (tests/test_field_histogram_cpu.py,
tests/test_gpu_field_histogram.py).

The gradient magnitude is gradient_ref.magnitude (the restatement the 2-D classification is tested
against); u, v, the bin rule, the order-preserving key and the statistics are written again here.
Every operation is a separate float32 numpy call, so nothing is fused.  References are computed
once per (field, bin shape) and handed out read-only."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import gradient_ref as gr

f32 = np.float32
Stats = namedtuple("Stats", "vmin vmax gmax nan_values nan_gradients")


# ------------------------------------------------------------ the statement --
def unit(s, lo, hi):
    """u of the values s over [lo, hi] (v of the magnitudes over [glo, ghi]); a NaN gives 0."""
    s = np.asarray(s, np.float32)
    with np.errstate(all="ignore"):
        t = ((s - f32(lo)) / (f32(hi) - f32(lo))).astype(np.float32)
        u = np.where(t > f32(0), t, f32(0)).astype(np.float32)
        return np.where(u < f32(1), u, f32(1)).astype(np.float32)


def bin_of(c, k):
    """The nearest of k nodes to the coordinates c in [0, 1], ties upward."""
    x = (np.asarray(c, np.float32) * f32(k - 1)).astype(np.float32)
    i0 = np.minimum(np.floor(x).astype(np.int64), k - 1)
    f = (x - i0.astype(np.float32)).astype(np.float32)
    return np.minimum(i0 + (f >= f32(0.5)), k - 1)


def histogram(scalar, n, m, lo, hi, glo=None, ghi=None, spacing=(1.0, 1.0, 1.0), mag=None):
    """(m, n) uint32 counts of a (z, y, x) array."""
    S = np.asarray(scalar).astype(np.float32)
    i = bin_of(unit(S, lo, hi), n)
    if m > 1:
        mag = gr.magnitude(scalar, spacing) if mag is None else mag
        i = bin_of(unit(mag, glo, ghi), m) * n + i
    return np.bincount(i.reshape(-1), minlength=n * m).astype(np.uint32).reshape(m, n)


def key(bits):
    """uint32 float bits -> uint32 keys that order as the values do, -0 below +0."""
    bits = np.asarray(bits, np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.uint32(k)
    return np.uint32(k ^ (np.uint32(0x80000000) if k >> np.uint32(31) else np.uint32(0xFFFFFFFF)))


def stats(scalar, spacing=(1.0, 1.0, 1.0), mag=None):
    S = np.ascontiguousarray(np.asarray(scalar).astype(np.float32))
    mag = gr.magnitude(scalar, spacing) if mag is None else mag
    ok, gok = ~np.isnan(S), ~np.isnan(mag)
    k = key(S.view(np.uint32))[ok]
    vmin = unkey(k.min()).view(np.float32) if k.size else f32(np.inf)
    vmax = unkey(k.max()).view(np.float32) if k.size else f32(-np.inf)
    gmax = mag[gok].max() if gok.any() else f32(0)
    return Stats(f32(vmin), f32(vmax), f32(gmax), int((~ok).sum()), int((~gok).sum()))


def same_stats(got, want):
    """Counts equal, floats equal as bits."""
    bits = [np.array([float(s.vmin), float(s.vmax), float(s.gmax)], np.float32).view(np.uint32) for s in (got, want)]
    return bool((bits[0] == bits[1]).all()) and tuple(got[3:]) == tuple(want[3:])


# ------------------------------------------------------------------ fields --
# scalar: (z, y, x); lo..hi and glo..ghi: the ranges the histograms are taken over
Field = namedtuple("Field", "scalar lo hi glo ghi spacing")
ONE = (1.0, 1.0, 1.0)


def _from_case(name):
    c = gr.case(name)
    return Field(c.scalar, c.lo, c.hi, c.glo, c.ghi, c.spacing)


def _thin(shape, dtype=np.uint16, seed=83):
    c = gr._thin(shape, dtype, seed)
    return Field(c.scalar, c.lo, c.hi, c.glo, c.ghi, ONE)


def _constant():
    return Field(np.full((32, 64, 128), 77, np.uint8), 0.0, 255.0, 0.0, 100.0, ONE)


def _alternating():
    s = np.full((32, 64, 128), 20, np.uint8)
    s[:, :, 1::2] = 200
    return Field(s, 0.0, 255.0, 0.0, 200.0, ONE)


def _nonfinite():
    """f32 (9, 10, 70): NaN, +-inf and +-0 in the interior and on faces; two +inf voxels two apart
    along x, so the voxel between them has an inf - inf (NaN) gradient; x = 70 puts the second
    wave's first lane beside the first wave's last."""
    rng = np.random.default_rng(89)
    s = rng.random((9, 10, 70), dtype=np.float32)
    s[rng.random(s.shape) < 0.3] = 0.0
    s[rng.random(s.shape) < 0.1] = -0.0
    s[4, 4, 4] = np.nan
    s[0, 0, 0] = np.nan          # a corner
    s[4, 5, 30] = np.inf
    s[4, 5, 32] = np.inf         # (4, 5, 31): inf - inf along x
    s[8, 9, 69] = np.inf         # the far corner
    s[2, 7, 63] = -np.inf        # a wave's last lane
    s[6, 0, 64] = -np.inf        # the next wave's first lane, on the y face
    s[3, 3, 10] = -0.0
    s[3, 3, 11] = 0.0
    return Field(s, 0.1, 0.8, 0.05, 0.45, ONE)


def _all_nan():
    return Field(np.full((3, 4, 5), np.nan, np.float32), 0.0, 1.0, 0.0, 1.0, ONE)


def geo():
    import cudavolumerenderer_amd as cvr
    return cvr.field_geometry()


def more_tasks_shape():
    """(z, y, x): more walk tasks than the grid's cap, so workgroups take a second trip."""
    g = geo()
    return (g["walk_z"] + 1, g["walk_tasks"] + 9, 8)


def one_trip_1d():
    """u8 voxels of one trip of the 1-D grid at its cap: 256 lanes of 16 bytes per workgroup."""
    return geo()["hist1d_grid"] * 256 * 16


def _more_tasks():
    rng = np.random.default_rng(97)
    s = rng.integers(0, 256, more_tasks_shape()).astype(np.uint8)
    s[rng.random(s.shape) < 0.5] = 0
    return Field(s, 0.0, 255.0, 0.0, 180.0, ONE)


def _long_1d():
    rng = np.random.default_rng(101)
    n = one_trip_1d() + 37
    s = rng.integers(0, 256, n).astype(np.uint8)
    s[rng.random(n) < 0.6] = 3
    return Field(s.reshape(1, 1, n), 0.0, 255.0, 0.0, 1.0, ONE)


FIELDS = {
    "random40_u8": lambda: _from_case("random40_u8"),
    "random40_u16": lambda: _from_case("random40_u16"),
    "random40_i16": lambda: _from_case("random40_i16"),
    "offgrid_f32": lambda: _from_case("offgrid_f32"),      # spacing (1, 0.5, 2)
    "runs_u16": lambda: _thin((35, 3, 321)),               # two x-runs, three z-chunks, both ragged
    "one_voxel_u8": lambda: Field(np.array([[[9]]], np.uint8), 0.0, 255.0, 0.0, 1.0, ONE),
    "constant_u8": _constant,
    "alternating_u8": _alternating,
    "nonfinite_f32": _nonfinite,
    "all_nan_f32": _all_nan,
    "more_tasks_u8": _more_tasks,
    "long_1d_u8": _long_1d,
}
for _k, _shape in enumerate(gr.THIN_SHAPES):
    FIELDS["thin%d_u16" % _k] = (lambda shape: lambda: _thin(shape))(_shape)
    FIELDS["thin%d_u8" % _k] = (lambda shape: lambda: _thin(shape, np.uint8))(_shape)
THIN = sorted(k for k in FIELDS if k.startswith("thin")) + ["one_voxel_u8"]

RANDOM = ["random40_u8", "random40_u16", "random40_i16", "offgrid_f32"]
# 128 x 128: the LDS limit exactly; 129 x 127 = 16383: one bin short of it, with odd sides; 129 x 128:
# the first shape past it (global atomics); 256 x 256: the largest
BINS_2D = [(2, 2), (7, 5), (128, 128), (129, 127), (129, 128), (256, 256)]
BINS_1D = [(2, 1), (256, 1), (65536, 1)]
SMALL_BINS = [(7, 5), (256, 1)]
# (field, n, m) of every histogram the two test files compare
HISTOGRAMS = ([(f, n, m) for f in RANDOM for n, m in BINS_2D + BINS_1D]
              + [(f, n, m) for f in THIN + ["runs_u16", "nonfinite_f32", "all_nan_f32"] for n, m in SMALL_BINS]
              + [("more_tasks_u8", 7, 5), ("more_tasks_u8", 129, 128)]
              + [(f, n, n) for f in ("constant_u8", "alternating_u8") for n in (64, 256)]
              + [("long_1d_u8", 256, 1)])
STATS = RANDOM + THIN + ["runs_u16", "nonfinite_f32", "all_nan_f32", "more_tasks_u8", "constant_u8"]


@lru_cache(maxsize=None)
def field(name):
    f = FIELDS[name]()
    f.scalar.setflags(write=False)
    return f


@lru_cache(maxsize=None)
def mag_of(name):
    f = field(name)
    m = gr.magnitude(f.scalar, f.spacing)
    m.setflags(write=False)
    return m


@lru_cache(maxsize=None)
def ref_histogram(name, n, m):
    f = field(name)
    h = histogram(f.scalar, n, m, f.lo, f.hi, f.glo, f.ghi, f.spacing, mag_of(name) if m > 1 else None)
    h.setflags(write=False)
    return h


@lru_cache(maxsize=None)
def ref_stats(name):
    f = field(name)
    return stats(f.scalar, f.spacing, mag_of(name))


def ident(case):
    return "%s-%dx%d" % case
