"""The cases at the limits of the walk's 24- and 32-bit index arithmetic, shared by
tests/test_limits_cpu.py (sharpness of the inputs on the oracle's evaluation log, the host pins) and
tests/test_gpu_limits.py (GPU == oracle at the limit, refusals past it).  Plain numpy, no library call.

Media: mostly empty grids whose stored region lies at the far end of the axes, where the products the
kernels form with 24-bit multiplies (cvr_walk.h dense_cell, woodcock_point) are largest.  Woodcock
tracking takes scale * max_density steps per unit of empty box, so a medium here is a slab about
scale * width = 15 mean free paths thick directly behind the face the camera looks through, and
sparse_long_x's box is thin across the view (a path scattered back leaves through a side).  Every
medium renders 32x32 pixels x 4 samples = 4096 paths, seed 7, like tests/params.py.

Launches (on params.blob16): tiles of 2^24 pixels, path ids up to 2^32 - 64, seeds whose sum with the
path id crosses 2^31 and 2^32, and 2^20 samples in one block-ordered launch."""
from collections import namedtuple

import numpy as np

import media
import params

NO_LEAF = 0xFFFFFFFF
W = H = 32
SAMPLES = params.SAMPLES
SEED = params.SEED
N_PATHS = W * H * SAMPLES
MAX_EVALS = 2_000_000        # per traced case (so that the GPU tests stay at seconds)
MIN_SHARP = 1000             # evaluations that would change under a narrower multiply
ALBEDO_BG = (0.75, 0.5, 0.875, 1.0)   # exact in binary16
EMASK_BITS = 2048            # cvr::kEmaskWords * 32
CORNER_FOV = 40.0            # from 0.02 outside the face: the rays cover the 0.0156-wide region's top

# kind "sparse": medium a media.Sparse, stored the (n, 3) leaf coordinates (x, y, z) of its slots;
# kind "dense": medium a media.Dense, stored None.  bound_shift: CVR_OPT_BOUNDS or None (default).
# eye / at / up / fov: params.look_at.  scale, box: the medium's.
MediumCase = namedtuple("MediumCase", "kind medium stored scale box_min box_max bound_shift eye at up fov")


def _quantised(rng, shape, zeros=0.3):
    """Random densities k / 1024 (exact in binary16: the half format stores them unchanged), `zeros`
    of them 0."""
    d = rng.integers(1, 1024, shape).astype(np.float32) / np.float32(1024)
    d[rng.random(shape) < zeros] = 0.0
    return d


def _sparse_slab(table_shape, x0, y0, z0, nx, ny, nz, seed, albedo=True):
    """A leaf table (lz, ly, lx) of NO_LEAF with the nx x ny x nz leaves from (x0, y0, z0) stored."""
    rng = np.random.default_rng(seed)
    lz, ly, lx = table_shape
    table = np.full(table_shape, NO_LEAF, np.uint32)
    n = nx * ny * nz
    table[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx] = np.arange(n, dtype=np.uint32).reshape(nz, ny, nx)
    zz, yy, xx = np.meshgrid(np.arange(z0, z0 + nz), np.arange(y0, y0 + ny), np.arange(x0, x0 + nx), indexing="ij")
    stored = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1)
    dens = _quantised(rng, (n, 512))
    alb = None
    if albedo:
        alb = np.ones((n, 512, 4), np.float32)
        alb[..., :3] = rng.integers(512, 1024, (n, 512, 3)).astype(np.float32) / np.float32(1024)
    return media.Sparse((8 * lx, 8 * ly, 8 * lz), table, dens, alb, ALBEDO_BG, 1.0), stored


def _corner_camera(res, cells, axis, box_min=(-0.5,) * 3, box_max=(0.5,) * 3, back=0.02):
    """Eye just outside the + face of `axis`, looking down that axis onto the centre of the region
    that ends at the far corner of the two other axes and is cells[k] cells wide there (a whole
    axis: its centre)."""
    at = [0.0, 0.0, 0.0]
    for k in range(3):
        lo = 1.0 - cells[k] / (res[k] - 1.0)               # in box coordinates [0, 1]
        mid = 0.5 * (max(lo, 0.0) + 1.0)
        at[k] = box_min[k] + mid * (box_max[k] - box_min[k])
    eye = list(at)
    eye[axis] = box_max[axis] + back
    at[axis] = 0.5 * (box_min[axis] + box_max[axis])
    up = (0, 1, 0) if axis != 1 else (1, 0, 0)
    return tuple(eye), tuple(at), up


def sparse_xy_limit(bshift=3):
    """Leaf table (2, ly, lx) with bnx * bny = (lx 2^(3 - bshift)) (ly 2^(3 - bshift)) the largest
    product below 2^24 with ly a power of two: 8^3 bricks (2, 4096, 4095), 4^3 (2, 2048, 2047),
    2^3 (2, 1024, 1023).  The last 64 x 64 x 2 leaves are stored."""
    ly = 4096 >> (3 - bshift)
    lx = ly - 1
    m, stored = _sparse_slab((2, ly, lx), lx - 64, ly - 64, 0, 64, 64, 2, seed=31 + bshift)
    eye, at, up = _corner_camera(m.res, (512, 512, 16), 2)
    # the slab is 512 cells of 8 lx wide: scale * width = 15.6 at 8^3 bricks
    return MediumCase("sparse", m, stored, 1000.0 * (lx / 4095.0), (-0.5,) * 3, (0.5,) * 3,
                      None if bshift == 3 else bshift, eye, at, up, CORNER_FOV)


def sparse_long_x():
    """One axis of more than 2^24 cells: leaf table (2, 1, 2^21 + 8192), res (2^24 + 65536, 8, 16),
    the last 8192 x 1 x 2 leaves stored (x cells 2^24 ..), no albedo pool.  The box is 1 x 0.01 x 0.01:
    a path that scatters back leaves through a side after a few steps, not after scale steps."""
    lx = (1 << 21) + 8192
    m, stored = _sparse_slab((2, 1, lx), 1 << 21, 0, 0, 8192, 1, 2, seed=41, albedo=False)
    box_min, box_max = (-0.5, -0.005, -0.005), (0.5, 0.005, 0.005)
    eye, at, up = _corner_camera(m.res, (65536, 8, 16), 0, box_min, box_max)
    return MediumCase("sparse", m, stored, 4000.0, box_min, box_max, None, eye, at, up, 12.0)


def sparse_long_z():
    """The longest z axis: leaf table (2^24, 1, 1), res (8, 8, 2^27), so that the z multiplicands of the
    brick word and leaf indices reach 2^24 - 1.  The last 8192 leaves are stored (z cells 2^27 - 65536 ..,
    where a float addresses every eighth cell), no albedo pool; the box is 0.01 x 0.01 x 1."""
    lz = 1 << 24
    m, stored = _sparse_slab((lz, 1, 1), 0, 0, lz - 8192, 1, 1, 8192, seed=42, albedo=False)
    box_min, box_max = (-0.005, -0.005, -0.5), (0.005, 0.005, 0.5)
    eye, at, up = _corner_camera(m.res, (8, 8, 65536), 2, box_min, box_max)
    return MediumCase("sparse", m, stored, 32000.0, box_min, box_max, None, eye, at, up, 12.0)


def sparse_thin_mask():
    """Leaf table (1, 1, 2^16): two axes give the empty-region mask no bits (es = 8, a super-brick is
    32 leaves of the x axis).  2048 leaves are stored, ending 64 leaves (two clear super-bricks)
    before the + x face the camera looks through."""
    lx = 1 << 16
    m, stored = _sparse_slab((1, 1, lx), lx - 2048 - 64, 0, 0, 2048, 1, 1, seed=43)
    box_min, box_max = (-0.5, -0.005, -0.005), (0.5, 0.005, 0.005)
    eye, at, up = _corner_camera(m.res, (8 * (2048 + 64), 8, 8), 0, box_min, box_max)
    return MediumCase("sparse", m, stored, 500.0, box_min, box_max, None, eye, at, up, 12.0)


def _dense_block(shape, block, seed):
    """density (nz, ny, nx) zero but for `block` (a tuple of slices) of quantised random values, and
    a uniform albedo (exact in binary16)."""
    rng = np.random.default_rng(seed)
    d = np.zeros(shape, np.float32)
    d[block] = _quantised(rng, d[block].shape)
    a = np.full(shape + (4,), 1.0, np.float32)
    a[..., :3] = ALBEDO_BG[:3]
    return media.Dense(d, a, 1.0, (-0.5,) * 3, (0.5,) * 3, 1000.0)


def dense_xy_limit():
    """4095 x 4096 x 2 voxels (rx * ry = 2^24 - 4096), a 64 x 64 block at the far x / y corner in
    both z layers."""
    m = _dense_block((2, 4096, 4095), (slice(None), slice(4096 - 64, None), slice(4095 - 64, None)), 51)
    eye, at, up = _corner_camera((4095, 4096, 2), (64, 64, 2), 2)
    return MediumCase("dense", m, None, 1000.0, m.box_min, m.box_max, None, eye, at, up, CORNER_FOV)


def dense_yz_limit():
    """2 x 4096 x 4095 voxels (ry * rz = 2^24 - 4096), a 64 x 64 block at the far y / z corner in
    both x layers."""
    m = _dense_block((4095, 4096, 2), (slice(4095 - 64, None), slice(4096 - 64, None), slice(None)), 52)
    eye, at, up = _corner_camera((2, 4096, 4095), (2, 64, 64), 0)
    return MediumCase("dense", m, None, 1000.0, m.box_min, m.box_max, None, eye, at, up, CORNER_FOV)


MEDIA = {
    "sparse_xy_limit": sparse_xy_limit,
    "sparse_xy_limit_b2": lambda: sparse_xy_limit(2),
    "sparse_xy_limit_b1": lambda: sparse_xy_limit(1),
    "sparse_long_x": sparse_long_x,
    "sparse_long_z": sparse_long_z,
    "sparse_thin_mask": sparse_thin_mask,
    "dense_xy_limit": dense_xy_limit,
    "dense_yz_limit": dense_yz_limit,
}
SPARSE = [k for k in MEDIA if k.startswith("sparse")]
DENSE = [k for k in MEDIA if k.startswith("dense")]


def res_of(case):
    if case.kind == "sparse":
        return tuple(int(v) for v in case.medium.res)
    nz, ny, nx = case.medium.density.shape
    return nx, ny, nz


def camera(case):
    return params.look_at(case.eye, case.at, case.up, fov=case.fov, full=(W, H))


def make_oracle(oracle_mod, case):
    """The oracle over the case's medium; a dense case's arrays (0.7 GB) are handed over uncopied."""
    m = case.medium
    if case.kind == "sparse":
        return oracle_mod.Oracle.from_leaves(m.res, m.table, m.leaf_density, m.leaf_albedo, m.albedo_bg,
                                             case.box_min, case.box_max, case.scale, m.max_density)
    return oracle_mod.Oracle.over(m.density, m.albedo, case.box_min, case.box_max, case.scale, m.max_density)


def make_launch(oracle_mod, case, kernel=2, seed=SEED):
    cam = camera(case)
    return oracle_mod.Oracle.launch(cam.inv_view, cam.r2v, (W, H), (W, H), (0, 0), kernel, seed)


# ------------------------------------------- the index arithmetic, restated ----
def brick_shift(case):
    """The brick size the library uses: sparse 8 cells (CVR_OPT_BOUNDS 1..3: that), dense 4."""
    if case.kind == "sparse":
        return 3 if case.bound_shift is None else min(case.bound_shift, 3)
    return 2 if case.bound_shift is None else case.bound_shift


def in_grid(case, evals):
    """(mask of the logged evaluations whose lower corner lies in the grid, their integer cell
    coordinates x1, y1, z1 as int64)."""
    rx, ry, rz = res_of(case)
    cx, cy, cz = (evals[k].astype(np.float64) for k in ("cx", "cy", "cz"))
    ok = (cx >= 0) & (cx < rx) & (cy >= 0) & (cy < ry) & (cz >= 0) & (cz < rz)
    f = [np.floor(np.where(ok, c, 0)).astype(np.int64) for c in (cx, cy, cz)]
    return ok, f[0], f[1], f[2]


def brick_terms(case, x1, y1, z1):
    """The two products of the brick index bz * (bnx bny) + by * bnx + bx (woodcock_point)."""
    s = brick_shift(case)
    rx, ry, _ = res_of(case)
    bnx, bny = (rx + (1 << s) - 1) >> s, (ry + (1 << s) - 1) >> s
    return (z1 >> s) * (bnx * bny), (y1 >> s) * bnx


def cell_terms(case, x1, y1, z1):
    """The two products of a dense cell index z1 * (rx ry) + y1 * rx + x1 (dense_cell)."""
    rx, ry, _ = res_of(case)
    return z1 * (rx * ry), y1 * rx


def emask_model(case):
    """The empty-region mask of a sparse case as cvr_set_medium_sparse derives it: (es, lx, ly, lz,
    bits) with a super-brick 2^es cells per axis, lx / ly / lz mask bits per axis and `bits` the set
    of set bit indices: the super-bricks holding a cell leaf (a leaf one of whose 8 forward
    neighbours, itself included, is stored)."""
    lz_n, ly_n, lx_n = case.medium.table.shape

    def log2up(v):
        return int(v - 1).bit_length()

    es, lx, ly, lz = 3, log2up(lx_n), log2up(ly_n), log2up(lz_n)
    while lx + ly + lz > log2up(EMASK_BITS):
        es += 1
        lx, ly, lz = max(lx - 1, 0), max(ly - 1, 0), max(lz - 1, 0)
    k = es - 3
    bits = set()
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                c = case.stored - np.array([dx, dy, dz])
                c = c[(c >= 0).all(axis=1)]
                b = ((c[:, 2] >> k) << (lx + ly)) | ((c[:, 1] >> k) << lx) | (c[:, 0] >> k)
                bits.update(int(v) for v in np.unique(b))
    return es, lx, ly, lz, bits


def super_brick(case, x1, y1, z1):
    es, lx, ly, _, _ = emask_model(case)
    return ((z1 >> es) << (lx + ly)) | ((y1 >> es) << lx) | (x1 >> es)


# ------------------------------------------------------------- launches ----
WIDE_TILE = (1 << 21, 8)         # 2^24 pixels
TALL_TILE = (24, 699048)         # 16 777 152 pixels, a width that is no power of two
TILES = {"wide_tile": WIDE_TILE, "tall_tile": TALL_TILE}
TOP_TILE = (24, 8)
TOP_ITERATIONS = 22_369_621      # n_paths = 4 294 967 232 = 2^32 - 64
TOP_N = TOP_TILE[0] * TOP_TILE[1] * TOP_ITERATIONS
TOP_RANGES = {
    "last_samples": (TOP_N - 4 * 192, 4 * 192),      # whole samples: the pixel-block order
    "unaligned_end": (TOP_N - 1000, 1000),           # path-id order
    "straddle_2_31": ((1 << 31) - 512, 1024),
}
SEED_SIGN = 0x7FFFFF00           # seed + id crosses 2^31 at id 256
SEED_WRAP = 0xFFFFFF00           # ... 2^32 at id 256
MAX_SAMPLES_TILE = (8, 8)
MAX_SAMPLES = 1 << 20


def tile_hit_camera(tile, hit=0.03):
    """A camera at (0, 0, 4) looking at blob16 under which about `hit` of the tile's rays meet the
    box: the long image axis spans tan = +-0.14 / hit, the short one its share by the pixel count
    (square pixels)."""
    w, h = tile
    t_long = 0.14 / hit
    r2v = (t_long, t_long * h / w) if w >= h else (t_long * w / h, t_long)
    eye = (0.0, 0.0, 4.0)
    return params.Camera(params.inv_view(params.look_at_R(eye, (0, 0, 0)), eye), np.array(r2v, np.float32))


# -------------------------------------------------------------- fastdiv ----
def fastdiv_divisors():
    d = {1, 2, 3, 5, 7, 24, 192, 1 << 26, (1 << 32) - 1}
    for k in range(1, 32):
        d.update({(1 << k) - 1, 1 << k, (1 << k) + 1})
    rng = np.random.default_rng(61)
    # half of them small (tile widths, block counts), half over the whole range
    d.update(int(v) for v in rng.integers(1, 1 << 16, 100))
    d.update(int(v) for v in rng.integers(1, 1 << 32, 100))
    return sorted(v for v in d if 1 <= v < (1 << 32))


def fastdiv_dividends(d, seed=62):
    u = {0, 1, d - 1, d, d + 1, (1 << 32) - 1}
    for target in (1 << 31, 1 << 32):
        m = (target // d) * d
        u.update({m - d - 1, m - d, m - 1, m, m + 1, m + d - 1, m + d, m + d + 1})
    u = np.array(sorted(v for v in u if 0 <= v < (1 << 32)), np.uint32)
    rng = np.random.default_rng(seed)
    return np.concatenate([u, rng.integers(0, 1 << 32, 10_000, dtype=np.uint64).astype(np.uint32)])
