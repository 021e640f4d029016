"""Media that take the medium build kernels past one pass of their grids, and their references
(tests/test_build_scale_cpu.py, tests/test_gpu_build_scale.py); plain numpy, no GPU.

Every kernel of cvr_medium_build.hip loops over a capped grid.  The caps are read from the library
(cvr_debug_build_geometry, geo() here) and every shape below is derived from them: the smallest
ragged grid (odd sizes, no multiple of a leaf or a vector) that crosses the threshold by at least
one wave of work.  tests/test_build_scale_cpu.py asserts each crossing, so a raised cap fails
there and never silently shrinks what the GPU tests cover.  With today's caps (scan grid 2048,
stream grid 8192, scan tile 2048, 4096 gradient tasks of 16 planes, 256-voxel leaf-flag runs):

  case              (z, y, x)        voxels     what loops
  dense_2m          (127, 129, 129)  2 113 407  k_scan_density's float4 loop (> 4 * 2048 * 256) with a
                                                3-voxel scalar tail; k_scan_albedo 5 trips; k_to_half
                                                of the albedo 5 trips, of the density and
                                                k_fill_albedo 2
  scalar_u8_8m      (203, 205, 205)  8 531 075  k_classified<u8>'s 16-byte body loop (> 16 * 524 288)
  scalar_u16_4m     (161, 163, 163)  4 277 609  k_classified<u16>'s body loop (> 8 * 524 288)
  scalar_i16_4m     (161, 163, 163)  4 277 609  k_classified<i16>'s; the field has negative codes
  scalar_f32_512k   (81, 83, 83)       558 009  k_classified<f32>'s one-voxel-per-lane loop
  gradient_u16_4m   (260, 257, 70)   4 677 400  k_gradient: 1 * 257 * 17 = 4369 tasks > 4096 under the
                                                XCD turn; a wave boundary inside the 70-voxel row; a
                                                last z chunk of 4 planes
  gradient_u16_x3   (33, 129, 523)   2 226 411  3 * 129 * 3 = 1161 tasks on a grid of 1160
  sparse_4m         (131, 117, 261)  4 000 347  17 x 15 x 33 = 8415 leaves, 4.1 scan tiles; nx > 256:
                                                k_leaf_flags and the gather with xc = 1, a last leaf of
                                                5 voxels in x; > 4096 leaves stored: k_gather_leaves'
                                                second trip (> 8192 * 256 pool voxels)

(k_gradient's grid is rounded down to a multiple of 8, so the small fields of
tests/test_gpu_gradient_transfer.py take its second trip as well, on 8 workgroups, where the XCD
turn of the block index is the identity; here the trip is taken at the cap and at 1160 workgroups,
where the turn permutes them.)

The integer scalar cases also come one element into their allocation (a 15- or 7-voxel head
before the first 16-byte group).  The plants of dense_2m are made by index from the caps (the
first voxel of the float4 loop's second trip, the last float4, the scalar tail).  sparse_4m blanks
leaves by index: one whole scan tile, one 256-flag step of another, while the leaves on either
side of the tile boundaries (2047, 2048, 4095) and the last leaf exist.

References are the existing numpy statements, unchanged: transfer_ref.classify,
gradient_ref.classify, devmed.leaf_rule and bounds_model; each is computed once per case.

Not covered, each needing a field of about 2^30 voxels: k_scan_sums past 1024 tiles and the 2^20
cap of the k_leaf_flags grid, driven from a voxel source.  The scan kernels themselves run at 8192
tiles through the cell-leaf path in tests/test_gpu_limits.py."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import devmed
import gradient_ref as gr
import media
import transfer_ref as tr

f32 = np.float32
WAVE = 64


@lru_cache(maxsize=None)
def geo():
    import cudavolumerenderer_amd as cvr
    return cvr.build_geometry()


def ragged_box(at_least, ok=lambda n: True):
    """The smallest (s, s + 2, s + 2), s odd, of at least `at_least` voxels whose count passes `ok`."""
    s = 3
    while s * (s + 2) * (s + 2) < at_least or not ok(s * (s + 2) * (s + 2)):
        s += 2
    return (s, s + 2, s + 2)


def trip(items_per_workgroup_trip=256):
    """Items that one trip of a scan_grid-capped kernel takes."""
    return geo()["scan_grid"] * items_per_workgroup_trip


# ------------------------------------------------------------------ dense_2m --
def dense_shape():
    # one more wave of float4 than the first trip holds, and a scalar tail
    return ragged_box(4 * (trip() + WAVE), lambda n: n % 4 != 0)


DensePlants = namedtuple("DensePlants", "trip2_first last_float4 tail n")


def dense_plants():
    """Voxel indices by their place in k_scan_density's loops."""
    z, y, x = dense_shape()
    n = z * y * x
    return DensePlants(4 * trip(), 4 * (n // 4 - 1) + 3, n - 1, n)


@lru_cache(maxsize=None)
def dense_base():
    """(density, albedo, max density): 40 % zeros, densities below 1.  Read-only; copy to plant."""
    rng = np.random.default_rng(101)
    shape = dense_shape()
    d = rng.random(shape, dtype=np.float32)
    d[rng.random(shape, dtype=np.float32) < 0.4] = 0.0
    a = np.ones(shape + (4,), np.float32)
    a[..., :3] = 0.2 + 0.8 * rng.random(shape + (3,), dtype=np.float32)
    d.setflags(write=False)
    a.setflags(write=False)
    return d, a, float(d.max())


PEAK = 7.5


def dense_with_maximum(where):
    """dense_base's density with the maximum PEAK planted at `where` ("trip2_first" or "tail"), a
    NaN and a larger negative value beside it."""
    p = dense_plants()
    d = dense_base()[0].copy()
    flat = d.reshape(-1)
    at = getattr(p, where)
    step = 1 if where == "trip2_first" else -1
    flat[at] = f32(PEAK)
    flat[at + step] = f32(np.nan)
    flat[at + 2 * step] = f32(-9.0)
    return d


def dense_overflow(kind):
    """(density, the index the refusal must name, its value).  "two_trips": two values that round
    to infinity, the larger index in workgroup 0's second trip, the smaller in the first trip of
    one of the last workgroups launched; "last_trip": one, in the last float4."""
    p = dense_plants()
    d = dense_base()[0].copy()
    flat = d.reshape(-1)
    if kind == "two_trips":
        small = 4 * ((geo()["scan_grid"] - 48) * 256 + 9) + 2
        flat[p.trip2_first + 4 * 3 + 1] = f32(-70000.0)
        flat[small] = f32(65520.0)
        return d, small, 65520.0
    flat[p.last_float4] = f32(1e6)
    return d, p.last_float4, 1e6


def uniform_albedo(kind):
    """(albedo over dense_base's density, format, expected albedo_uniform): 0.9 everywhere but
    for one voxel of k_scan_albedo's last trip."""
    z, y, x = dense_shape()
    a = np.ones((z, y, x, 4), np.float32)
    a[..., :3] = f32(0.9)
    flat = a.reshape(-1, 4)
    n = flat.shape[0]
    assert n - 6 >= (n - 1) // trip() * trip()  # the last trip
    if kind == "uniform":
        return a, 0, 1
    if kind == "last_voxel":
        flat[n - 1, 1] = f32(0.5)
        return a, 0, 0
    if kind == "round_apart":       # 0.9005 -> 0.90039063, 0.9 -> 0.89990234
        flat[n - 5, 2] = f32(0.9005)
        return a, 1, 0
    assert kind == "round_together"  # 0.9 and its successor share a half
    flat[n - 6, 0] = np.nextafter(f32(0.9), f32(1))
    return a, 1, 1


# -------------------------------------------------------------- scalar cases --
def table64(seed=103):
    rng = np.random.default_rng(seed)
    t = np.empty((64, 4), np.float32)
    t[:, :3] = 0.2 + 0.8 * rng.random((64, 3), dtype=np.float32)
    t[:, 3] = np.linspace(0.0, 1.0, 64, dtype=np.float32) * (0.5 + 0.5 * rng.random(64, dtype=np.float32))
    return t


SCALAR_DTYPES = {"scalar_u8_8m": np.uint8, "scalar_u16_4m": np.uint16, "scalar_i16_4m": np.int16,
                 "scalar_f32_512k": np.float32, "scalar_u8_8m_ceil": np.uint8}
# voxels before the first 16-byte group when the tensor starts one element into its allocation
HEAD = {"scalar_u8_8m": 15, "scalar_u16_4m": 7, "scalar_i16_4m": 7}


def scalar_shape(name):
    size = np.dtype(SCALAR_DTYPES[name]).itemsize
    per_group = 16 // size if size < 4 else 1   # voxels of one 16-byte load; f32: one voxel per lane
    # the head and tail of an offset tensor leave the body a group short: one more wave covers it
    return ragged_box(per_group * (trip() + 2 * WAVE))


def _scalar_case(name):
    dtype = SCALAR_DTYPES[name]
    shape = scalar_shape(name)
    rng = np.random.default_rng(107)
    if dtype == np.float32:
        s = rng.random(shape, dtype=np.float32)
        lo, hi = 0.1, 0.8
    else:
        info = np.iinfo(dtype)
        s = rng.integers(info.min, info.max + 1, shape).astype(dtype)
        lo, hi = info.min + 0.1 * (info.max - info.min), info.min + 0.9 * (info.max - info.min)
    s[rng.random(shape, dtype=np.float32) < 0.3] = 0 if dtype != np.int16 else np.iinfo(np.int16).min
    return tr.Case(s, table64(), lo, hi, name.endswith("_ceil"), False, *tr.UNIT, media.SCALE, False)


# ------------------------------------------------------------ gradient cases --
def gradient_shape(name):
    g = geo()
    if name == "gradient_u16_x3":
        return (33, 129, 523)
    ny = 257
    nzc = g["gradient_tasks"] // ny + 2           # one y-row of tasks more than the grid holds
    return ((nzc - 1) * g["gradient_z"] + 4, ny, WAVE + 6)


def gradient_tasks(shape):
    """(tasks, workgroups) of k_gradient's launch on a (z, y, x) field."""
    g = geo()
    nz, ny, nx = shape
    tasks = -(-nx // 256) * ny * -(-nz // g["gradient_z"])
    grid = min(tasks, g["gradient_tasks"])
    return tasks, (grid & ~7) if grid >= 8 else grid


def table8x32(seed=109):
    return gr.table2d(8, 32, seed)


def _gradient_case(name):
    shape = gradient_shape(name)
    rng = np.random.default_rng(113)
    # smooth ramps under noise: small and large gradients both occur
    z, y, x = np.meshgrid(*(np.arange(v) for v in shape), indexing="ij", sparse=True)
    s = ((x * 37 + y * 101 + z * 53) % 60000).astype(np.uint16)
    noisy = rng.random(shape, dtype=np.float32) < 0.3
    s[noisy] = rng.integers(0, 65536, int(noisy.sum())).astype(np.uint16)
    return gr.Case(s, table8x32(), 1000.0, 60000.0, 0.0, 30000.0, (1.0, 0.5, 2.0), *tr.UNIT, media.SCALE, False)


# ----------------------------------------------------------------- sparse_4m --
def sparse_leaf_dims():
    """(lz, ly, lx): one leaf more in x than a k_leaf_flags task takes, and more than 4 scan tiles."""
    g = geo()
    lx = g["leaf_run_leaves"] + 1
    a = 1
    while a * (a + 2) * lx <= 4 * g["scan_tile"] + WAVE:
        a += 2
    return (a + 2, a, lx)


def sparse_shape():
    lz, ly, lx = sparse_leaf_dims()
    return (lz * 8 - 5, ly * 8 - 3, lx * 8 - 3)   # the last leaf holds 3 x 5 x 5 voxels (z, y, x)


SPARSE_PLANTS = {"albedo": 100, "negzero": 101, "nan": 102, "corner": 103}  # leaf indices, blanked first


@lru_cache(maxsize=None)
def sparse_exists():
    """The leaves of sparse_4m by leaf index: about 80 % of those outside the blanked ranges."""
    g = geo()
    tile = g["scan_tile"]
    lz, ly, lx = sparse_leaf_dims()
    n = lz * ly * lx
    rng = np.random.default_rng(127)
    e = rng.random(n) < 0.8
    e[2 * tile:3 * tile] = False                    # a whole scan tile without a leaf
    e[tile + 3 * 256:tile + 4 * 256] = False        # a 256-flag step without one
    e[[0, tile - 1, tile, 2 * tile - 1, n - 1]] = True
    for kind, leaf in SPARSE_PLANTS.items():
        e[leaf] = kind != "negzero"
    e.setflags(write=False)
    return e


def _leaf_mask(exists):
    """exists (by leaf index) as a (z, y, x) voxel mask over the grid."""
    lz, ly, lx = sparse_leaf_dims()
    nz, ny, nx = sparse_shape()
    m = exists.reshape(lz, ly, lx)
    return np.repeat(np.repeat(np.repeat(m, 8, 0), 8, 1), 8, 2)[:nz, :ny, :nx]


def _plant_voxel(leaf, far=False):
    lz, ly, lx = sparse_leaf_dims()
    x, y, z = leaf % lx, (leaf // lx) % ly, leaf // (lx * ly)
    return (8 * z + 7, 8 * y + 7, 8 * x + 7) if far else (8 * z + 1, 8 * y + 2, 8 * x + 1)


@lru_cache(maxsize=None)
def sparse_arrays():
    """(density, albedo, max density) of sparse_4m as arrays, with devmed's plants: a leaf that
    exists through one albedo voxel, a -0 that makes none, a NaN and a far-corner voxel that do."""
    shape = sparse_shape()
    rng = np.random.default_rng(131)
    plain = sparse_exists().copy()
    plain[list(SPARSE_PLANTS.values())] = False
    keep = _leaf_mask(plain)
    d = f32(0.6) * rng.random(shape, dtype=np.float32)
    d[rng.random(shape, dtype=np.float32) < 0.4] = 0.0
    d[~keep] = 0.0
    bg = np.array([0.7, 0.55, 0.33, 1.0], np.float32)
    a = np.ones(shape + (4,), np.float32)
    a[..., :3] = 0.2 + 0.8 * rng.random(shape + (3,), dtype=np.float32)
    a[~keep] = bg
    a[0, 0, 0] = bg
    d[0, 0, 1] = f32(0.25)   # (leaf 0 exists whatever voxel 0 holds)
    a[_plant_voxel(SPARSE_PLANTS["albedo"])][:3] = (0.25, 0.5, 0.75)
    d[_plant_voxel(SPARSE_PLANTS["negzero"])] = f32(-0.0)
    d[_plant_voxel(SPARSE_PLANTS["nan"])] = f32(np.nan)
    d[_plant_voxel(SPARSE_PLANTS["corner"], far=True)] = f32(0.125)
    d.setflags(write=False)
    a.setflags(write=False)
    return d, a, float(np.nanmax(d))


def _sparse_codes(dtype):
    """sparse_4m as a scalar field: code 0 in the blanked leaves and at voxel 0, codes >= 1 in
    most voxels of the others (the planted leaves become plain ones and the -0's stays blank: a
    scalar has no -0 or NaN)."""
    shape = sparse_shape()
    rng = np.random.default_rng(137)
    top = np.iinfo(dtype).max
    s = rng.integers(1, top + 1, shape).astype(dtype)
    s[rng.random(shape, dtype=np.float32) < 0.4] = 0
    s[~_leaf_mask(sparse_exists())] = 0
    s[0, 0, 0] = 0
    s[0, 0, 1] = top
    return s


def _sparse_scalar_case():
    t = table64(139)
    t[0, 3] = 0.0            # code 0: density 0 and the background's colour
    return tr.Case(_sparse_codes(np.uint8), t, 0.0, 255.0, False, False, *tr.UNIT, media.SCALE, True)


def _sparse_gradient_case():
    """Column 0 of the table is (background, 0) in every row, so a voxel of code 0 classifies to
    the background whatever its gradient: the blanked leaves stay empty, while the voxels beside
    them take their stencil's neighbours from leaves that do not exist."""
    t = table8x32(149)
    t[:, 0, :3] = t[0, 0, :3]
    t[:, 0, 3] = 0.0
    return gr.Case(_sparse_codes(np.uint16), t, 0.0, 65535.0, 0.0, 30000.0, (1.0, 1.0, 1.0), *tr.UNIT, media.SCALE,
                   True)


# ------------------------------------------------------------------ registry --
SCALAR_CASES = ("scalar_u8_8m", "scalar_u16_4m", "scalar_i16_4m", "scalar_f32_512k", "scalar_u8_8m_ceil")
GRADIENT_CASES = ("gradient_u16_4m", "gradient_u16_x3")


@lru_cache(maxsize=None)
def case(name):
    """The tr.Case or gr.Case of a classified case."""
    if name in SCALAR_CASES:
        return _scalar_case(name)
    if name in GRADIENT_CASES:
        return _gradient_case(name)
    return _sparse_scalar_case() if name == "sparse_4m_u8" else _sparse_gradient_case()


def is_gradient(name):
    return name in GRADIENT_CASES or name == "sparse_4m_u16g"


@lru_cache(maxsize=3)
def classified(name):
    """(density, albedo, max density) of a case by the numpy statement ("sparse_4m": the arrays
    themselves).  The last few are kept: the tests take a case's formats and variants in a row."""
    if name == "sparse_4m":
        return sparse_arrays()
    c = case(name)
    if is_gradient(name):
        d, a, _ = gr.classify(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)
    else:
        d, a = tr.classify(c.scalar, c.table, c.lo, c.hi, c.ceil, c.density_u)
    d.setflags(write=False)
    a.setflags(write=False)
    with np.errstate(invalid="ignore"):
        return d, a, float(np.nanmax(np.maximum(d, 0)))


@lru_cache(maxsize=2)
def leaves(name):
    """devmed.leaf_rule of a sparse case's classified arrays."""
    d, a, _ = classified(name)
    return devmed.leaf_rule(d, a)


def host_classified(cvr, name):
    """The library's host statement of a classified case: (density, albedo)."""
    c = case(name)
    if is_gradient(name):
        return cvr.classify_gradient_host(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)[:2]
    return cvr.classify_host(c.scalar, c.table, c.lo, c.hi, ceil=c.ceil, density_u=c.density_u)
