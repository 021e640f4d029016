"""The view passes (cvr_features, cvr_preview) on the limit media of tests/limits.py: the references and
the sharpness measures shared by tests/test_view_limits_cpu.py and tests/test_gpu_view_limits.py.
Plain numpy, no library call.

A sparse limit medium has up to 2^33 voxels and cannot be densified, so its reference is the numpy
restatement over the leaf fetch (features_ref.features_fetch, preview_ref.preview_fetch with
features_ref.leaf_fetch), restricted to the stored leaves' bounding box (leaf_support: the samples
outside add nothing).  A dense limit medium's reference is the host statement; the restatement only
provides its tap log."""
import numpy as np

import features_ref
import limits
import preview_ref

LIGHT = (0.3, 1.0, -0.4)
T_STOP, MAX_STEPS = 1.0 / 256.0, 65536
# (full resolution, tile, offset): the case's own 32x32 view, and the same camera as a tile that is
# ragged against the wave's 8x8 blocks
VIEWS = {"full": ((32, 32), (32, 32), (0, 0)), "tile": ((64, 64), (32, 24), (3, 5))}
M23 = (1 << 23) - 1


def step_of(case):
    """Sparse cases step 8 cells, the largest step cvr_features_desc accepts (the numpy march takes up
    to 8300 steps in the stored region of the long media), dense ones 1."""
    return 8.0 if case.kind == "sparse" else 1.0


def fetches(case):
    """(res, density fetch, albedo fetch, support) of a limit case."""
    m = case.medium
    if case.kind == "sparse":
        dens, alb = features_ref.leaf_fetch(m.res, m.table, m.leaf_density, m.leaf_albedo, m.albedo_bg)
        return tuple(int(v) for v in m.res), dens, alb, features_ref.leaf_support(m.table)
    return features_ref.array_fetch(m.density, m.albedo) + (None,)


def ref_features(case, view="full", taps=None, sums=None):
    res, dens, alb, support = fetches(case)
    full, tile, off = VIEWS[view]
    cam = limits.camera(case)
    return features_ref.features_fetch(res, dens, alb, case.box_min, case.box_max, case.scale, cam.inv_view, cam.r2v, full,
                                       tile, off, 0, step_of(case), T_STOP, MAX_STEPS, taps=taps, support=support, sums=sums)


def ref_features_and_unshaded(case, view="full"):
    """(the feature planes, the unshaded preview over a black background) from one march: the two
    passes take the same samples and sum the same products (preview_ref.unshaded_from)."""
    sums = {}
    planes = ref_features(case, view, sums=sums)
    return planes, preview_ref.unshaded_from(sums)


def ref_preview(case, shaded, view="full", taps=None):
    """Shaded: one directional light (LIGHT), the default shading; unshaded: PREVIEW_UNSHADED."""
    res, dens, alb, support = fetches(case)
    full, tile, off = VIEWS[view]
    cam = limits.camera(case)
    kw = dict(light=LIGHT, flags=0) if shaded else dict(flags=preview_ref.UNSHADED)
    return preview_ref.preview_fetch(res, dens, alb, case.box_min, case.box_max, case.scale, case.medium.max_density,
                                     cam.inv_view, cam.r2v, full, tile, off, 0, step_of(case), T_STOP, MAX_STEPS, taps=taps,
                                     support=support, **kw)


def in_grid_taps(case, taps):
    """The logged corners that lie in the grid (the ones FeatureDeviceTexels::cell is asked for), as
    int64 x1, y1, z1."""
    t = np.concatenate(taps).astype(np.int64)
    ok = ((t >= 0) & (t < np.array(limits.res_of(case)))).all(axis=1)
    return t[ok, 0], t[ok, 1], t[ok, 2]


def _cut(v):
    return v & M23


def narrowed(case, x1, y1, z1):
    """Per tap, whether the storage index differs when formed with (every multiplicand of its two
    products cut to 23 bits, every product cut to 23 bits, the added x term's coordinate cut to 23
    bits).  The index: a sparse case's brick word bz (bnx bny) + by bnx + bx of coordinates >> brick
    shift (limits.brick_terms), a dense case's cell z1 (rx ry) + y1 rx + x1 (limits.cell_terms)."""
    rx, ry, _ = limits.res_of(case)
    if case.kind == "sparse":
        s = limits.brick_shift(case)
        bnx, bny = (rx + (1 << s) - 1) >> s, (ry + (1 << s) - 1) >> s
        zt, yt = limits.brick_terms(case, x1, y1, z1)
        xt = x1 >> s
        multiplicands = _cut(z1 >> s) * _cut(bnx * bny) + _cut(y1 >> s) * _cut(bnx)
        x_cut = _cut(x1) >> s
    else:
        zt, yt = limits.cell_terms(case, x1, y1, z1)
        xt = x1
        multiplicands = _cut(z1) * _cut(rx * ry) + _cut(y1) * _cut(rx)
        x_cut = _cut(x1)
    return zt + yt != multiplicands, zt + yt != _cut(zt) + _cut(yt), xt != x_cut


def mask_variants(case, x1, y1, z1):
    """Per tap of a sparse case: (the empty-region mask's bit index changes when its y and z shifts
    are swapped, ... when the super-brick shift is taken as 3).  (Using the z shift's value for the y
    shift alone changes nothing on a limit medium whose mask has y bits: their z axis has none, the z
    super-brick is 0.  media.sparse_es4 shows that fault, tests/test_gpu_view_storage.py.)"""
    es, lx, ly, _, _ = limits.emask_model(case)
    true = limits.super_brick(case, x1, y1, z1)
    swapped = ((z1 >> es) << lx) | ((y1 >> es) << (lx + ly)) | (x1 >> es)
    shift3 = ((z1 >> 3) << (lx + ly)) | ((y1 >> 3) << lx) | (x1 >> 3)
    return true != swapped, true != shift3
