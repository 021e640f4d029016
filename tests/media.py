"""Small synthetic media shared by the tests (plain numpy, no library call).

dense_arrays / sparse_arrays: the half-format scenes (a dense 19x13x11 grid, a
sparse 20x12x28 index box).  The others are the brick-bound media of
tests/test_bounds_model.py and tests/test_gpu_bounds_model.py: each is built to
make one kind of bound mistake change the number of cells fetched."""
import ctypes as C
from collections import namedtuple

import numpy as np

SCALE = 100.0

# A dense medium: density (nz, ny, nx), albedo (nz, ny, nx, 4), majorant, box, scale.
Dense = namedtuple("Dense", "density albedo max_density box_min box_max scale")
# A sparse medium (cvr_sparse_medium_desc layout): res (nx, ny, nz), table (lz, ly, lx) u32,
# leaf density (n, 512), leaf albedo (n, 512, 4) or None, background albedo, majorant.
Sparse = namedtuple("Sparse", "res table leaf_density leaf_albedo albedo_bg max_density")


# ------------------------------------------------- the half-format scenes ---
def dense_arrays(md_case="max", uniform=False, seed=7):
    """A dense 19x13x11 grid, no multiple of the 4^3 brick, ~40 % zeros, with planted fp16
    subnormal / flush-to-zero / tie values: (density, albedo, max_density), unrounded."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = 11, 13, 19
    d = rng.random((nz, ny, nx), dtype=np.float32)
    d[rng.random(d.shape) < 0.4] = 0.0
    d[5, 6, 9] = 1e-6              # an fp16 subnormal
    d[5, 6, 10] = 1e-8             # rounds to 0
    d[4, 6, 9] = 0.5 + 2.0 ** -12  # a tie (to even: 0.5)
    a = np.ones((nz, ny, nx, 4), np.float32)
    if uniform:
        a[..., :3] = np.float32(0.9)
    else:
        a[..., :3] = 0.2 + 0.8 * rng.random((nz, ny, nx, 3), dtype=np.float32)
    if md_case == "max":
        md = float(d.max())
    elif md_case == "up":      # f16(0.3) = 0.30004883 > 0.3
        d *= np.float32(0.29)
        md = float(np.float32(0.3))
    else:                      # f16(0.9) = 0.89990234 < 0.9
        d *= np.float32(0.89)
        md = float(np.float32(0.9))
    return d, a, md


def sparse_arrays(with_albedo=True, seed=11):
    """Index box 20x12x28 -> 3x2x4 leaves, about half absent, the z = 3 slab and most of z = 2
    empty, so that whole super-bricks (here: leaves) hold no cell leaf."""
    rng = np.random.default_rng(seed)
    res = (20, 12, 28)
    lx, ly, lz = 3, 2, 4
    present = np.zeros((lz, ly, lx), bool)
    present[0] = [[1, 0, 1], [1, 1, 0]]
    present[1] = [[0, 1, 1], [1, 0, 1]]
    present[2] = [[0, 0, 0], [0, 0, 1]]
    table = np.full((lz, ly, lx), 0xFFFFFFFF, np.uint32)
    table[present] = np.arange(present.sum(), dtype=np.uint32)
    n = int(present.sum())
    dens = rng.random((n, 512), dtype=np.float32)
    dens[rng.random(dens.shape) < 0.4] = 0.0
    dens[0, 73] = 1e-6
    dens[0, 74] = 1e-8
    dens[1, 200] = 0.5 + 2.0 ** -12
    alb = None
    if with_albedo:
        alb = np.ones((n, 512, 4), np.float32)
        alb[..., :3] = 0.2 + 0.8 * rng.random((n, 512, 3), dtype=np.float32)
    bg = (0.7, 0.55, 0.33, 1.0)
    return res, table, dens, alb, bg, float(dens.max())


def sparse_desc(cvr, res, table, dens, alb, bg, md):
    from cudavolumerenderer_amd._lib import SparseMediumDesc
    table = np.ascontiguousarray(table, np.uint32)
    dens = np.ascontiguousarray(dens, np.float32)
    alb = None if alb is None else np.ascontiguousarray(alb, np.float32)
    s = SparseMediumDesc()
    s.res[:] = res
    s.leaf_dims[:] = table.shape[::-1]
    s.leaf_table = table.ctypes.data_as(C.POINTER(C.c_uint32))
    s.n_leaves = dens.shape[0]
    s.leaf_density = dens.ctypes.data_as(C.POINTER(C.c_float))
    if alb is not None:
        s.leaf_albedo = alb.ctypes.data_as(C.POINTER(C.c_float))
    s.albedo_background[:] = bg
    s.box_min[:] = (-0.5,) * 3
    s.box_max[:] = (0.5,) * 3
    s.scale = SCALE
    s.max_density = md
    s.g = 0.0
    s.roughness[:] = (0.1, 0.1)
    s.eta = np.float32(np.float32(1.05) / np.float32(1.01))
    return s, (table, dens, alb)


# ------------------------------------------------- the brick-bound media ----
def _bound_value(c):  # the table under test, restated in tests/bounds_model.py
    return np.array([(c << 19) + (112 << 23)], np.uint32).view(np.float32)[0]


def _albedo(rng, shape):
    a = np.ones(shape + (4,), np.float32)
    a[..., :3] = 0.2 + 0.8 * rng.random(shape + (3,), dtype=np.float32)
    return a


def _dense(d, a, md, box_min=(-0.5,) * 3, box_max=(0.5,) * 3, scale=SCALE):
    return Dense(d, a, float(md), tuple(box_min), tuple(box_max), float(scale))


STAIRCASE_CODES = range(150, 210)
STAIRCASE_BOX_MAX = (0.59, 0.60, 0.64)


def staircase(seed=21):
    """21x17x13 voxels, res - 1 a multiple of 4 on every axis, so every axis ends in a one-cell-thick
    last brick.  Every 4^3 brick has a peak voxel (its second voxel per axis, or its only one) holding
    bound_value(c), the float32 below or the one above, for c = 150..209 spread over the bricks;
    the brick's other voxels are random values below 0.9 of the peak, and the voxels on the planes
    shared with the previous bricks (coordinates that are multiples of 4) below the lowest peak.
    max_density = 1: many distinct codes, and maxima exactly on and around the code values."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = 21, 17, 13
    bx, by, bz = 6, 5, 4
    combos = [(c, v) for c in STAIRCASE_CODES for v in (-1, 0, 1)]
    pick = rng.permutation(len(combos))[:bx * by * bz]
    low = np.float32(0.9) * _bound_value(STAIRCASE_CODES[0])
    d = np.zeros((nz, ny, nx), np.float32)
    peaks = []
    for i, k in enumerate(pick):
        c, v = combos[k]
        peak = _bound_value(c)
        peak = np.nextafter(peak, np.float32(v * 4), dtype=np.float32) if v else peak
        peak = min(peak, np.float32(1))
        x0, y0, z0 = 4 * (i % bx), 4 * ((i // bx) % by), 4 * (i // (bx * by))
        x1, y1, z1 = min(x0 + 4, nx), min(y0 + 4, ny), min(z0 + 4, nz)
        blk = d[z0:z1, y0:y1, x0:x1]
        blk[...] = np.float32(0.9) * peak * rng.random(blk.shape, dtype=np.float32)
        blk[0, :, :] = low * rng.random(blk[0, :, :].shape, dtype=np.float32)
        blk[:, 0, :] = low * rng.random(blk[:, 0, :].shape, dtype=np.float32)
        blk[:, :, 0] = low * rng.random(blk[:, :, 0].shape, dtype=np.float32)
        peaks.append((min(z0 + 1, nz - 1), min(y0 + 1, ny - 1), min(x0 + 1, nx - 1), peak))
    for z, y, x, peak in peaks:
        d[z, y, x] = peak
    return _dense(d, _albedo(rng, d.shape), 1.0, (-0.5,) * 3, STAIRCASE_BOX_MAX)


SPIKES = [(0, 0, 0), (21, 17, 13), (4, 8, 4), (8, 4, 8), (12, 12, 4), (16, 8, 12), (20, 16, 12), (8, 16, 0),
          (20, 4, 8)]


def spikes(seed=22):
    """22x18x14 voxels, a background of 0.05 random, and single voxels of 1.0 at brick corners
    (coordinates that are multiples of 4; also voxel (0,0,0) and the far corner).  A spike is covered
    by the windows of up to 8 bricks of 4^3 cells and is the maximum of 7 of them only through the
    +1 voxel of the window."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = 22, 18, 14
    d = np.float32(0.05) * rng.random((nz, ny, nx), dtype=np.float32)
    for x, y, z in SPIKES:
        d[z, y, x] = 1.0
    return _dense(d, _albedo(rng, d.shape), 1.0)


def random40():
    """The 19x13x11 grid with 40 % zeros (dense_arrays): ragged sizes, no multiple of any brick."""
    d, a, md = dense_arrays("max")
    return _dense(d, a, md)


def offgrid(seed=23):
    """A 14x10x12 grid in the box (-0.3, -0.2, -0.4)..(0.5, 0.4, 0.8), scale 40.  Under the default
    worldToAABB (Q4: p - min/extent) many Woodcock points fall off the cell grid, some at negative
    coordinates, and many in the last cell layer; with CVR_OPT_WORLD_TO_AABB 1 none does."""
    rng = np.random.default_rng(seed)
    d = rng.random((12, 10, 14), dtype=np.float32)
    d[rng.random(d.shape) < 0.3] = 0.0
    return _dense(d, _albedo(rng, d.shape), d.max(), (-0.3, -0.2, -0.4), (0.5, 0.4, 0.8), 40.0)


def sparse_small(with_albedo=True):
    """sparse_arrays as a Sparse: es = 3, one super-brick is one leaf."""
    return Sparse(*sparse_arrays(with_albedo))


ES4_LEAVES = [(8, 7, 3), (9, 7, 3),            # (x, y, z) leaf coordinates; these two share a super-brick
              (7, 8, 4), (8, 8, 4), (9, 9, 3), (6, 6, 2), (10, 8, 5), (8, 5, 4), (5, 9, 3),
              (16, 8, 4)]                      # the last leaf column, alone in the ragged super-brick column


def sparse_es4(seed=24):
    """An index box of 136x128x64 voxels = 17x16x8 leaves, whose padded leaf grid (32x16x8) exceeds
    the mask's 2048 bits: es = 4, a super-brick is 2x2x2 leaves.  Ten leaves are present, nine near
    the centre under thin densities (few fetches, few segments: the brick-word bounds are tight),
    with clear super-bricks above and below them along the camera's axis."""
    rng = np.random.default_rng(seed)
    res = (136, 128, 64)
    table = np.full((8, 16, 17), 0xFFFFFFFF, np.uint32)
    for i, (x, y, z) in enumerate(ES4_LEAVES):
        table[z, y, x] = i
    n = len(ES4_LEAVES)
    dens = np.float32(0.15) * rng.random((n, 512), dtype=np.float32)  # thin: few fetches and segments
    dens[rng.random(dens.shape) < 0.3] = 0.0
    alb = np.ones((n, 512, 4), np.float32)
    alb[..., :3] = 0.2 + 0.8 * rng.random((n, 512, 3), dtype=np.float32)
    return Sparse(res, table, dens, alb, (0.7, 0.55, 0.33, 1.0), 1.0)


DENSE_MEDIA = {"staircase": staircase, "spikes": spikes, "random40": random40, "offgrid": offgrid}
SPARSE_MEDIA = {"sparse_small": sparse_small, "sparse_es4": sparse_es4}
