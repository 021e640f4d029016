"""The labelled classification of include/cvr.h (CVR_HAS_LABELS) restated in numpy fp32,
independent of the library, and the media of the label tests (tests/test_labels_cpu.py,
tests/test_gpu_labels.py); plain numpy, no GPU.

classify() is the written statement: j = L < m ? L : 0, then the CVR_HAS_TRANSFER statement
(tests/transfer_ref.py's classify, every operation a separate float32 numpy call) on row j.  Nothing
is shared with the C++.

The fixtures are made so that a mis-paired voxel shows: labels are independent per voxel (not
blocky) over 0..m-1 with a sprinkling of bytes >= m, 255 among them, and every row of a table is a
random table of its own seed (tables(); devmed.unusual_table is a sparse medium, not a transfer
table, so the rows are made here), so a wrong row, or a label taken from the voxel beside, changes
stored bits.  test_labels_cpu.py shows that with a row swap."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import build_scale as bs
import media
import transfer_ref as tr

f32 = np.float32
RES = (37, 29, 23)          # (nx, ny, nz): ragged; u8 and u16 get a head, a partial last 64-group run and a tail
SHAPE = RES[::-1]
TINY = (2, 2, 3)            # (z, y, x): 12 voxels, less than one 16-byte group of u8: head only


def classify(scalar, labels, table, lo, hi, ceil=False, density_u=False):
    """(density, albedo, counts) of a scalar array, a uint8 array of the same shape and an
    (m, n, 4) table."""
    scalar, labels = np.asarray(scalar), np.asarray(labels)
    table = np.asarray(table, np.float32)
    assert labels.dtype == np.uint8 and labels.shape == scalar.shape and table.ndim == 3
    m = table.shape[0]
    row = np.where(labels < m, labels, 0)
    density = np.empty(scalar.shape, np.float32)
    albedo = np.empty(scalar.shape + (4,), np.float32)
    for j in np.unique(row):
        at = row == j
        density[at], albedo[at] = tr.classify(scalar[at], table[j], lo, hi, ceil, density_u)
    return density, albedo, np.bincount(labels.reshape(-1), minlength=256).astype(np.uint64)


# ---------------------------------------------------------------- fixtures --
def tables(m, n=7, seed=500):
    """(m, n, 4): row j a random table of seed + j: colours in 0.2..1, densities in 0..1, rising
    on average, entry 0 not zero."""
    t = np.empty((m, n, 4), np.float32)
    for j in range(m):
        rng = np.random.default_rng(seed + j)
        t[j, :, :3] = 0.2 + 0.8 * rng.random((n, 3), dtype=np.float32)
        t[j, :, 3] = np.linspace(0.05, 1.0, n, dtype=np.float32) * (0.5 + 0.5 * rng.random(n, dtype=np.float32))
    return t


def labels_iid(shape, m, seed, stray=0.04):
    """Independent per voxel over 0..m-1; with m < 256 about `stray` of them are bytes >= m (255
    always among them)."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, m, shape).astype(np.uint8)
    if m < 256:
        out = rng.random(shape) < stray
        lab[out] = rng.integers(m, 256, int(out.sum())).astype(np.uint8)
        flat = lab.reshape(-1)
        flat[flat.size // 2] = 255
    return lab


def field(dtype, shape=SHAPE, seed=601):
    """Random codes over the type's range with 30 % at its lowest code; f32: 0..1."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        s = rng.random(shape, dtype=np.float32)
        s[rng.random(shape) < 0.3] = 0.0
        return s
    info = np.iinfo(dtype)
    s = rng.integers(info.min, info.max + 1, shape).astype(dtype)
    s[rng.random(shape) < 0.3] = info.min
    return s


def window(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return 0.1, 0.8
    info = np.iinfo(dtype)
    return info.min + 0.1 * (info.max - info.min), info.min + 0.9 * (info.max - info.min)


Case = namedtuple("Case", "scalar labels table lo hi ceil density_u sparse")
Case.__new__.__defaults__ = (False, False, False)


def _ragged(dtype, m=5, ceil=False):
    lo, hi = window(dtype)
    return Case(field(dtype), labels_iid(SHAPE, m, 611), tables(m), lo, hi, ceil)


def _tiny():
    return Case(field(np.uint8, TINY, 603), labels_iid(TINY, 3, 613, stray=0.2), tables(3), 20.0, 230.0)


HIDDEN = 2                   # the label whose row hides its segment in the sparse cases
# leaf-aligned boxes (z, y, x slices) whose voxels all carry HIDDEN: whole leaves that must not exist
HIDDEN_BOXES = ((slice(0, 8), slice(8, 24), slice(8, 24)), (slice(16, 23), slice(0, 8), slice(24, 37)))


def _sparse(kind, voxel0=HIDDEN):
    """A 4-row table whose row HIDDEN is (one colour, density 0) throughout; voxel 0 carries
    `voxel0`, so with HIDDEN that colour is the background and a leaf of HIDDEN voxels alone does
    not exist.  "one_colour": every row has that colour, so no leaf differs through its albedo."""
    m = 4
    t = tables(m, seed=520)
    colour = np.array([0.8, 0.6, 0.4], np.float32)
    t[HIDDEN, :, :3] = colour
    t[HIDDEN, :, 3] = 0.0
    if kind == "one_colour":
        t[:, :, :3] = colour
    lab = labels_iid(SHAPE, m, 617)
    for box in HIDDEN_BOXES:
        lab[box] = HIDDEN
    lab[0, 0, 0] = voxel0
    lo, hi = window(np.uint16)
    return Case(field(np.uint16, seed=605), lab, t, lo, hi, False, False, True)


def _full_table():
    """16 x 256 entries, the whole LDS budget, with labels over all 256 bytes."""
    return Case(field(np.uint8, seed=607), labels_iid(SHAPE, 256, 619), tables(256, 16, 1000), 10.0, 240.0)


def _uniform_rgb():
    t = tables(5, seed=540)
    t[:, :, :3] = np.array([0.9, 0.55, 0.3], np.float32)
    c = _ragged(np.uint8)
    return c._replace(table=t)


def _mostly_one():
    """99 % of the voxels carry label 1: the counters' contended case."""
    rng = np.random.default_rng(623)
    lab = np.ones(SHAPE, np.uint8)
    other = rng.random(SHAPE) < 0.01
    lab[other] = rng.integers(0, 256, int(other.sum())).astype(np.uint8)
    return _ragged(np.uint16)._replace(labels=lab)


def _overflow(what, sparse):
    """Row 3 alone holds a value above 65504 (density or green), in an entry that some voxel of
    label 3 reaches: format 1 must refuse, naming what the device call on the host arrays names."""
    c = _sparse("zero") if sparse else _ragged(np.uint16, m=4)
    t = c.table.copy()
    t[3, 4, 3 if what == "density" else 1] = f32(70000.0)
    return c._replace(table=t)


def _m1(sparse):
    """One row: the statement is cvr_set_medium_scalar's whatever the labels hold."""
    base = tr.case("sparse_small_zero") if sparse else None
    if sparse:
        return Case(base.scalar, labels_iid(base.scalar.shape, 7, 631), base.table[None], base.lo, base.hi, False, False,
                    True)
    c = _ragged(np.uint16)
    return c._replace(table=tr.table7()[None], labels=labels_iid(SHAPE, 9, 633))


# --- past one pass of the grids (tests/build_scale.py's shapes, from the library's caps)
def scale_dense_shape():
    """The labelled dense pair takes k_classified's trips: 64 groups of 16 u8 voxels per wave."""
    return bs.scalar_shape("scalar_u8_8m")


def _scale_dense():
    shape = scale_dense_shape()
    s = field(np.uint8, shape, 641)
    return Case(s, labels_iid(shape, 6, 643), tables(6, 64, 560), 25.0, 230.0)


def _scale_sparse():
    """build_scale's sparse field (code 0 in the blanked leaves and at voxel 0) under independent
    labels; entry 0 of every row is (one colour, 0), so code 0 is background under any label."""
    s = bs._sparse_codes(np.uint8)
    t = tables(6, 64, 580)
    t[:, 0, :3] = t[0, 0, :3]
    t[:, 0, 3] = 0.0
    return Case(s, labels_iid(s.shape, 6, 647), t, 0.0, 255.0, False, False, True)


CASES = {
    "ragged_u8": lambda: _ragged(np.uint8), "ragged_u16": lambda: _ragged(np.uint16),
    "ragged_i16": lambda: _ragged(np.int16), "ragged_f32": lambda: _ragged(np.float32),
    "ragged_u8_ceil": lambda: _ragged(np.uint8, ceil=True),
    "tiny_u8": _tiny,
    "sparse_hidden": lambda: _sparse("zero"), "sparse_one_colour": lambda: _sparse("one_colour"),
    "sparse_voxel0_row1": lambda: _sparse("zero", voxel0=1),
    "full_table": _full_table, "uniform_rgb": _uniform_rgb, "mostly_one": _mostly_one,
    "overflow_density": lambda: _overflow("density", False), "overflow_colour": lambda: _overflow("colour", False),
    "overflow_density_sparse": lambda: _overflow("density", True),
    "overflow_colour_sparse": lambda: _overflow("colour", True),
    "m1": lambda: _m1(False), "m1_sparse": lambda: _m1(True),
    "scale_dense_u8": _scale_dense, "scale_sparse_u8": _scale_sparse,
}


@lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    for a in (c.scalar, c.labels, c.table):
        a.setflags(write=False)
    return c


@lru_cache(maxsize=8)
def classified(name):
    """(density, albedo, counts) of a case by the numpy statement; read-only."""
    c = case(name)
    out = classify(c.scalar, c.labels, c.table, c.lo, c.hi, c.ceil, c.density_u)
    for a in out:
        a.setflags(write=False)
    return out


@lru_cache(maxsize=8)
def host(name):
    """(density, albedo, counts) of a case by the library's host statement; read-only."""
    import cudavolumerenderer_amd as cvr
    c = case(name)
    out = cvr.classify_labels_host(c.scalar, c.labels, c.table, c.lo, c.hi, ceil=c.ceil, density_u=c.density_u)
    for a in out:
        a.setflags(write=False)
    return out


SCALE = media.SCALE
