"""Media and the numpy statement of the leaf rule for the device-medium tests
(tests/test_device_medium_cpu.py, tests/test_gpu_device_medium.py); plain numpy and the oracle,
no GPU.

leaf_rule restates cvr.h's dense -> 8^3 leaves rule (cvr_scene_sparse_medium's, and
cvr_set_medium_device's with CVR_DEVMED_SPARSE): leaves in z, y, x order, x fastest; a leaf
exists iff an in-grid voxel has density != 0.0f (-0: no, NaN: yes) or 16 albedo bytes other than
voxel (0,0,0)'s; padding voxels hold (0, background); the albedo pool is dropped when no voxel
differs from the background."""
from functools import lru_cache

import numpy as np

import media

NO_LEAF = 0xFFFFFFFF
TILE = (32, 32)
ITERS = 4
N = TILE[0] * TILE[1] * ITERS  # 4096 paths
SEED = 3


def leaf_rule(density, albedo):
    """(density (z, y, x), albedo (z, y, x, 4)) -> media.Sparse without a majorant."""
    density = np.ascontiguousarray(density, np.float32)
    albedo = np.ascontiguousarray(albedo, np.float32)
    nz, ny, nx = density.shape
    lz, ly, lx = (nz + 7) // 8, (ny + 7) // 8, (nx + 7) // 8
    bg = albedo[0, 0, 0].copy()
    D = np.zeros((lz * 8, ly * 8, lx * 8), np.float32)
    A = np.empty((lz * 8, ly * 8, lx * 8, 4), np.float32)
    A[:] = bg
    D[:nz, :ny, :nx] = density
    A[:nz, :ny, :nx] = albedo
    differs = (A.view(np.uint32) != bg.view(np.uint32)).any(axis=3)  # bytes, not values
    with np.errstate(invalid="ignore"):
        live = (D != np.float32(0)) | differs                        # NaN != 0, -0 == 0

    def by_leaf(a):  # (lz, ly, lx, 512 [, 4]) with the pool's voxel order (z, y, x; x fastest)
        tail = a.shape[3:]
        a = a.reshape((lz, 8, ly, 8, lx, 8) + tail)
        a = np.moveaxis(a, (0, 2, 4), (0, 1, 2))
        return a.reshape((lz, ly, lx, 512) + tail)

    exists = by_leaf(live).any(axis=3)
    table = np.full((lz, ly, lx), NO_LEAF, np.uint32)
    table[exists] = np.arange(int(exists.sum()), dtype=np.uint32)
    leaf_density = np.ascontiguousarray(by_leaf(D)[exists])
    leaf_albedo = np.ascontiguousarray(by_leaf(A)[exists]) if differs.any() else None
    return media.Sparse((nx, ny, nz), table, leaf_density, leaf_albedo, tuple(float(v) for v in bg), None)


def densify(sp):
    """The dense grid of a media.Sparse: (density (z, y, x), albedo (z, y, x, 4)), cut to res."""
    nx, ny, nz = sp.res
    lz, ly, lx = sp.table.shape
    D = np.zeros((lz * 8, ly * 8, lx * 8), np.float32)
    A = np.empty((lz * 8, ly * 8, lx * 8, 4), np.float32)
    A[:] = np.asarray(sp.albedo_bg, np.float32)
    for z, y, x in zip(*np.nonzero(sp.table != NO_LEAF)):
        s = sp.table[z, y, x]
        D[z * 8:z * 8 + 8, y * 8:y * 8 + 8, x * 8:x * 8 + 8] = sp.leaf_density[s].reshape(8, 8, 8)
        if sp.leaf_albedo is not None:
            A[z * 8:z * 8 + 8, y * 8:y * 8 + 8, x * 8:x * 8 + 8] = sp.leaf_albedo[s].reshape(8, 8, 8, 4)
    return np.ascontiguousarray(D[:nz, :ny, :nx]), np.ascontiguousarray(A[:nz, :ny, :nx])


# Planted voxels per sparse medium: leaf coordinates (x, y, z) of four leaves its table leaves
# empty.  "albedo": the leaf exists only through one albedo voxel; "negzero": its only non-zero
# bits are a -0.0, which makes no leaf; "nan": one NaN, which makes one; "corner": one non-zero
# voxel at the leaf's far corner.
PLANTS = {
    "sparse_small": {"albedo": (0, 0, 3), "negzero": (1, 0, 3), "nan": (2, 1, 3), "corner": (0, 0, 2)},
    "sparse_es4": {"albedo": (3, 3, 1), "negzero": (4, 4, 1), "nan": (12, 10, 6), "corner": (2, 12, 5)},
}


@lru_cache(maxsize=None)
def sparse_grid(name, with_albedo=True):
    """The densified sparse medium `name` of tests/media.py with the planted voxels:
    (density, albedo, max_density).  Without varying albedo there is no albedo plant."""
    sp = media.sparse_small(with_albedo) if name == "sparse_small" else media.sparse_es4()
    D, A = densify(sp)
    nz, ny, nx = D.shape
    A[0, 0, 0] = np.asarray(sp.albedo_bg, np.float32)  # the rule's background is voxel (0,0,0)'s albedo
    for kind, (lx, ly, lz) in PLANTS[name].items():
        assert sp.table[lz, ly, lx] == NO_LEAF, (name, kind)
        x, y, z = 8 * lx + 1, 8 * ly + 2, 8 * lz + 1
        if kind == "albedo":
            if sp.leaf_albedo is not None:
                A[z, y, x, :3] = (0.25, 0.5, 0.75)
        elif kind == "negzero":
            D[z, y, x] = np.float32(-0.0)
        elif kind == "nan":
            D[z, y, x] = np.float32(np.nan)
        else:
            x, y, z = 8 * lx + 7, 8 * ly + 7, 8 * lz + 7
            D[z, y, x] = np.float32(0.125)
        assert x < nx and y < ny and z < nz, (name, kind)
    return D, A, float(sp.max_density)


@lru_cache(maxsize=None)
def unusual_table(seed=31):
    """A media.Sparse that cvr_set_medium_sparse allows and the leaf rule never makes: a ragged
    20x12x10 grid (3x2x2 leaves, 7 stored), slots in reverse leaf order, the last two stored
    entries both naming slot 0; the three leaves at the far (y, z) edge have no cell leaf."""
    rng = np.random.default_rng(seed)
    present = np.array([[[1, 0, 1], [0, 1, 1]], [[1, 1, 0], [1, 0, 0]]], bool)  # (z, y, x)
    n = int(present.sum()) - 1
    table = np.full(present.shape, NO_LEAF, np.uint32)
    table[present] = np.maximum(n - 1 - np.arange(n + 1), 0).astype(np.uint32)
    dens = np.float32(0.05) * rng.random((n, 512), dtype=np.float32)
    dens[rng.random(dens.shape) < 0.4] = 0.0
    alb = np.ones((n, 512, 4), np.float32)
    alb[..., :3] = 0.2 + 0.8 * rng.random((n, 512, 3), dtype=np.float32)
    return media.Sparse((20, 12, 10), table, dens, alb, (0.7, 0.55, 0.33, 1.0), float(dens.max()))


@lru_cache(maxsize=None)
def centre_voxel():
    """A 5^3 grid of density 1 at scale 4 (free paths of a quarter of the box) whose albedo is
    0.9 but for the centre voxel's 0.2: a medium that a wrongly "uniform" albedo renders otherwise."""
    d = np.ones((5, 5, 5), np.float32)
    a = np.ones((5, 5, 5, 4), np.float32)
    a[..., :3] = np.float32(0.9)
    a[2, 2, 2, :3] = np.float32(0.2)
    return media.Dense(d, a, 1.0, (-0.5,) * 3, (0.5,) * 3, 4.0)


def _cvr():
    import cudavolumerenderer_amd as cvr
    cvr.load()
    return cvr


def md_eff(md):
    return max(float(np.float32(md)), float(_cvr().half_round(np.array([md], np.float32))[0]))


def oracle_records(density, albedo, max_density, fmt=0, box_min=(-0.5,) * 3, box_max=(0.5,) * 3, scale=media.SCALE):
    """Records of path ids [0, N) of the TILE launch over the dense grid as format `fmt` stores it."""
    import oracle
    cvr = _cvr()
    if fmt:
        density, albedo, max_density = cvr.half_round(density), cvr.half_round(albedo), md_eff(max_density)
    orc = oracle.Oracle(density, albedo, box_min, box_max, scale, max_density)
    iv, r2v = cvr.default_camera(*TILE)
    return orc.trace_paths(orc.launch(iv, r2v, TILE, TILE, (0, 0), 2, SEED), 0, N)


@lru_cache(maxsize=None)
def dense_reference(name, fmt):
    m = centre_voxel() if name == "centre_voxel" else media.DENSE_MEDIA[name]()
    return oracle_records(m.density, m.albedo, m.max_density, fmt, m.box_min, m.box_max, m.scale)


@lru_cache(maxsize=None)
def sparse_reference(name, with_albedo, fmt):
    D, A, md = sparse_grid(name, with_albedo)
    return oracle_records(D, A, md, fmt)
