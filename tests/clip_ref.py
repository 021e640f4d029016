"""The clip region's statement (include/cvr.h, CVR_HAS_CLIP) restated in numpy, and the regions
the clip tests share (tests/test_clip_cpu.py, tests/test_gpu_clip.py); plain numpy, no GPU.

keep_mask evaluates the written statement with float32 operations in the stated order: integer
comparisons for the crop box, and per plane t = ((A * x + B * y) + C * z) + D with every product
and every sum rounded to float32, kept iff t >= 0.  clip applies it to a density and an albedo
grid: a clipped voxel gets density +0 and the 16 bytes of the unclipped voxel (0, 0, 0)'s albedo."""
from collections import namedtuple

import numpy as np

f32 = np.float32
RES = (37, 29, 21)  # (nx, ny, nz): ragged, 5 x 4 x 3 leaves with partial last ones

Region = namedtuple("Region", "lo hi planes")
Region.__new__.__defaults__ = (None, None, ())


def keep_mask(res, lo=None, hi=None, planes=()):
    """(z, y, x) bool: the voxels of a grid of res = (nx, ny, nz) the region keeps."""
    nx, ny, nz = res
    lo = (0, 0, 0) if lo is None else lo
    hi = res if hi is None else tuple(min(int(h), int(n)) for h, n in zip(hi, res))
    # (broadcast axes: every element still sees the same float32 operations in the same order)
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.int64), np.arange(ny, dtype=np.int64),
                          np.arange(nx, dtype=np.int64), indexing="ij", sparse=True)
    keep = np.ones((nz, ny, nx), bool)
    keep &= (x >= lo[0]) & (x < hi[0]) & (y >= lo[1]) & (y < hi[1]) & (z >= lo[2]) & (z < hi[2])
    xf, yf, zf = x.astype(f32), y.astype(f32), z.astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for A, B, C, D in planes:
            ax, by, cz = f32(A) * xf, f32(B) * yf, f32(C) * zf
            t = ((ax + by) + cz) + f32(D)
            assert t.dtype == f32
            keep &= t >= f32(0)
    return keep


def clip(density, albedo, region):
    """(keep (z, y, x) bool, density, albedo) of the region over (z, y, x) and (z, y, x, 4) float32
    grids; either grid may be None."""
    src = density if density is not None else albedo[..., 0]
    nz, ny, nx = src.shape
    keep = keep_mask((nx, ny, nz), region.lo, region.hi, region.planes)
    d = a = None
    if density is not None:
        d = np.array(density, np.float32, copy=True)
        d[~keep] = f32(0)
    if albedo is not None:
        a = np.array(albedo, np.float32, copy=True)
        a[~keep] = np.array(albedo[0, 0, 0], np.float32, copy=True)
    return keep, d, a


# ------------------------------------------------------------------ regions --
CROP = Region((3, 9, 2), (30, 17, 40))                    # off the leaf grid, hi past res in z
EMPTY_CROP = Region((5, 5, 5), (5, 5, 5))
OBLIQUE = Region(planes=((0.6, -0.35, 0.72, -9.3),))
SLAB = Region(planes=((1.0, 1.0, 0.25, -20.0), (-1.0, -1.0, -0.25, 45.5)))
CROP_SLAB = Region(CROP.lo, CROP.hi, SLAB.planes)
KEEP_ALL_PLANE = Region(planes=((0.0, 0.0, 1.0, 5.0),))
KEEP_NONE_PLANE = Region(planes=((0.0, 0.0, -1.0, -1.0),))
LATTICE_TIE = Region(planes=((1.0, -1.0, 0.0, 0.0),))     # t == 0 on the whole lattice plane x == y: kept
NEG_ZERO_D = Region(planes=((0.0, -1.0, 0.0, -0.0),))     # t = +-0 at y == 0: kept; negative elsewhere
EIGHT = Region(planes=((1.0, 0.0, 0.0, -2.0), (-1.0, 0.0, 0.0, 33.0), (0.0, 1.0, 0.0, -1.5), (0.0, -1.0, 0.0, 26.25),
                       (0.0, 0.0, 1.0, -1.0), (0.0, 0.0, -1.0, 18.0), (0.37, 0.41, 0.83, -11.0),
                       (-0.5, 0.25, -0.125, 21.0)))
ALL_CLIPPED = Region((0, 0, 0), (37, 29, 21), ((0.0, 0.0, -1.0, -1.0),))

CPU_REGIONS = {"crop": CROP, "empty_crop": EMPTY_CROP, "oblique": OBLIQUE, "slab": SLAB, "keep_all": KEEP_ALL_PLANE,
               "keep_none": KEEP_NONE_PLANE, "lattice_tie": LATTICE_TIE, "neg_zero_d": NEG_ZERO_D, "eight": EIGHT}
GPU_REGIONS = {"crop": CROP, "oblique": OBLIQUE, "crop_slab": CROP_SLAB, "all_clipped": ALL_CLIPPED}


def arrays(res=RES, seed=211):
    """(density (z, y, x), albedo (z, y, x, 4)) float32 with 40 % zero densities and a varying w."""
    nx, ny, nz = res
    rng = np.random.default_rng(seed)
    d = rng.random((nz, ny, nx), dtype=np.float32)
    d[rng.random((nz, ny, nx), dtype=np.float32) < 0.4] = 0.0
    a = (0.2 + 0.8 * rng.random((nz, ny, nx, 4), dtype=np.float32)).astype(np.float32)
    return d, a
