"""The references of tests/test_gpu_view_limits.py are right, and its inputs are sharp (no GPU).

The fetch form (features_ref.features_fetch, preview_ref.preview_fetch): over the leaf fetch of
media.sparse_small() and media.sparse_es4() it must equal the array form over the densified medium
and cvr.features_host / cvr.preview_host on it, bit for bit (shaded and unshaded, cameras "oblique"
and "inside", a half step), with and without the restriction to the leaves' bounding box
(features_ref.support_skip), whose tap log must be a part of the unrestricted one.

Sharpness, on the tap log of each limit case's reference (view_limits.ref_features; the integer
corners of the density samples that lie in the grid, which FeatureDeviceTexels::cell indexes the
storage with): at least limits.MIN_SHARP taps whose brick-word or cell index changes when the
multiplicands of its two products are cut to 23 bits ("mult"), when the products are ("prod"), when
the coordinate of the added x term is ("x"), and, for the sparse cases, whose mask bit changes when
the mask's y and z shifts are swapped ("swap") and when its super-brick shift is taken as 3
("shift").  Which of these a case can show follows from its construction; the others are asserted
to be 0, so that this table cannot go out of date:
  sparse_xy_limit, _b2, _b1   mult (bnx bny >= 2^23), prod, swap (emask_model (10|9|8, 5, 5, 0)), shift
  sparse_long_z               mult (z1 >> 3 >= 2^23), prod, shift; swap is a no-op: emask_model
                              (16, 0, 0, 11), lx = ly = 0
  sparse_long_x               x (x1 >= 2^24) and shift only: no multiplicand or product reaches 2^23
                              (bnx bny = 2^21 + 8192, bz <= 1), so the case exercises no multiply; swap is
                              a no-op: emask_model (14, 11, 0, 0), ly = lz = 0
  sparse_thin_mask            shift only: the grid has 2^19 x 8 x 8 cells, nothing reaches 2^23; swap is a
                              no-op: emask_model (8, 11, 0, 0), ly = lz = 0.  The case is there for its mask
                              geometry (es = 8, two axes without bits)
  dense_xy_limit, _yz_limit   prod (y1 rx, z1 rx ry >= 2^23); the multiplicands stay below 2^13
Measured (taps in the grid; then every count that is not 0 equals it):
  sparse_xy_limit 45849   sparse_xy_limit_b2 67928   sparse_xy_limit_b1 70853   sparse_long_x 8424672
  sparse_long_z 8443420   sparse_thin_mask 2080906   dense_xy_limit 864764      dense_yz_limit 855740

The tap log itself (which samples the blocked march of features_ref.march counts as taken) is
compared with a plain step-by-step loop written out here, on media.sparse_es4().

Opacity: at least 95 % of each case's 1024 reference pixels have W > 0.  Measured: 100 % in all
eight cases."""
import numpy as np
import pytest

import devmed
import features_ref
import limits
import media
import params
import preview_ref
import view_limits
from test_denoise_cpu import bits

F = np.float32
GEOMETRY = ((64, 48), (40, 24), (8, 8))
SMALL = {"sparse_small": media.sparse_small, "sparse_es4": media.sparse_es4}
# (step, t_stop, max_steps)
MARCHES = {"unit": (1.0, 1.0 / 256.0, 4096), "half": (0.5, 0.0, 4096)}


# ------------------------------------------------------------ the fetch form --
@pytest.fixture(scope="module")
def small():
    cache = {}

    def get(name):
        if name not in cache:
            sp = SMALL[name]()
            cache[name] = (sp, devmed.densify(sp))
        return cache[name]

    return get


def leaf_args(sp):
    dens, alb = features_ref.leaf_fetch(sp.res, sp.table, sp.leaf_density, sp.leaf_albedo, sp.albedo_bg)
    return tuple(int(v) for v in sp.res), dens, alb


def tap_set(taps):
    return set(map(tuple, np.concatenate(taps).tolist())) if taps else set()


@pytest.mark.parametrize("march", list(MARCHES))
@pytest.mark.parametrize("camera", ["oblique", "inside"])
@pytest.mark.parametrize("name", list(SMALL))
def test_features_leaf_fetch_equals_arrays_and_host(cvr, small, name, camera, march):
    sp, (D, A) = small(name)
    full, tile, off = GEOMETRY
    cam = params.camera(camera, full)
    tail = (cam.inv_view, cam.r2v, full, tile, off, 0) + MARCHES[march]
    box = ((-0.5,) * 3, (0.5,) * 3, media.SCALE)
    log_a, log_l, log_s = [], [], []
    arr = features_ref.features(D, A, *box, *tail, taps=log_a)
    leaf = features_ref.features_fetch(*leaf_args(sp), *box, *tail, taps=log_l)
    cut = features_ref.features_fetch(*leaf_args(sp), *box, *tail, taps=log_s, support=features_ref.leaf_support(sp.table))
    m, keep = cvr.medium_from_arrays(D, A, scale=media.SCALE, max_density=sp.max_density)
    host = cvr.features_host(m, cam.inv_view, cam.r2v, full, tile, off, 0, cvr.FeaturesDesc(*MARCHES[march]))
    for what, got in (("arrays", arr), ("leaf fetch", leaf), ("leaf fetch, support", cut)):
        assert np.array_equal(bits(got[0]), bits(host[0])) and np.array_equal(bits(got[1]), bits(host[1])), what
    assert (host[0][..., 3] > 0).sum() > 50
    assert tap_set(log_a) == tap_set(log_l) and sum(map(len, log_a)) == sum(map(len, log_l))
    assert tap_set(log_s) <= tap_set(log_l) and 0 < sum(map(len, log_s)) <= sum(map(len, log_l))
    if name == "sparse_es4" and camera == "inside":  # (sparse_small is smaller than the margin: nothing to pass by)
        assert sum(map(len, log_s)) < sum(map(len, log_l))


@pytest.mark.parametrize("shaded", [True, False], ids=["shaded", "unshaded"])
@pytest.mark.parametrize("camera,march", [("oblique", "unit"), ("inside", "unit"), ("oblique", "half")])
@pytest.mark.parametrize("name", list(SMALL))
def test_preview_leaf_fetch_equals_arrays_and_host(cvr, small, name, camera, march, shaded):
    sp, (D, A) = small(name)
    full, tile, off = GEOMETRY
    cam = params.camera(camera, full)
    kw = dict(light=view_limits.LIGHT, flags=0) if shaded else dict(flags=preview_ref.UNSHADED)
    tail = (cam.inv_view, cam.r2v, full, tile, off, 0) + MARCHES[march]
    box = ((-0.5,) * 3, (0.5,) * 3, media.SCALE, sp.max_density)
    arr = preview_ref.preview(D, A, *box, *tail, **kw)
    leaf = preview_ref.preview_fetch(*leaf_args(sp), *box, *tail, **kw)
    cut = preview_ref.preview_fetch(*leaf_args(sp), *box, *tail, support=features_ref.leaf_support(sp.table), **kw)
    m, keep = cvr.medium_from_arrays(D, A, scale=media.SCALE, max_density=sp.max_density)
    desc = cvr.PreviewDesc(cvr.FeaturesDesc(*MARCHES[march]), **kw)
    host = cvr.preview_host(m, cam.inv_view, cam.r2v, full, tile, off, 0, desc)
    for what, got in (("arrays", arr), ("leaf fetch", leaf), ("leaf fetch, support", cut)):
        assert np.array_equal(bits(got), bits(host)), what
    assert (host[..., 3] > 0).sum() > 50
    if not shaded:  # the unshaded preview composited from the feature march's sums: the same bits
        sums = {}
        features_ref.features_fetch(*leaf_args(sp), *box[:3], *tail, sums=sums)
        assert np.array_equal(bits(preview_ref.unshaded_from(sums)), bits(host))


def plain_features_taps(res, density, box_min, box_max, scale, inv_view, r2v, full, tile, offset, step, t_stop, max_steps):
    """The density samples the feature pass takes, by the plain loop of the text: one step at a time
    over the pixels that are still marching.  -> ((n, 3) int32 corners, the final T per pixel)."""
    from features_ref import chord, floor_i32, fma, minnum, rays, trilinear
    fres = np.array(res, F)
    bmin, bmax = np.asarray(box_min, F), np.asarray(box_max, F)
    e = bmax - bmin
    shift, g = bmin / e, np.array([r - 1 for r in res], F)
    cell = e / fres
    delta = F(step) * minnum(minnum(cell[0], cell[1]), cell[2])
    o, d = rays(inv_view, r2v, full, tile, offset)
    has, t0, t1 = chord(o, d, bmin, bmax)
    q = np.ceil((t1 - t0) / delta).astype(F)
    n = np.where(has, np.where(q < F(max_steps), np.where(q > 0, q, 0), max_steps), 0).astype(np.int64)
    T = np.ones(d.shape[0], F)
    live = n > 0
    taps = []
    for i in range(int(n.max(initial=0))):
        t = t0 + (F(i) + F(0.5)) * delta
        live &= (i < n) & (t < t1)
        k = np.nonzero(live)[0]
        if not k.size:
            break
        p = (o + t[k][:, None] * d[k]).astype(F)
        cg = fma(p - shift, g, F(0))
        taps.append(np.stack([floor_i32(cg[:, a]) for a in range(3)], axis=1).astype(np.int32))
        s = (F(scale) * trilinear(density, cg[:, 0], cg[:, 1], cg[:, 2], res)) * delta
        hit = s > 0
        kh = k[hit]
        w = T[kh] * (s[hit] / (F(1) + s[hit]))
        T[kh] = T[kh] - w
        live[kh[T[kh] < F(t_stop)]] = False
    return np.concatenate(taps), T


@pytest.mark.parametrize("camera", ["oblique", "inside"])
@pytest.mark.parametrize("name", list(SMALL))
def test_tap_log_equals_plain_loop(small, name, camera):
    """The blocked march logs exactly the samples the plain loop takes (as multisets: rays that end
    with T < t_stop inside a block log nothing after their end), with and without a support."""
    sp, _ = small(name)
    full, tile, off = GEOMETRY
    cam = params.camera(camera, full)
    res, dens, alb = leaf_args(sp)
    march = MARCHES["unit"]
    want, T = plain_features_taps(res, dens, (-0.5,) * 3, (0.5,) * 3, media.SCALE, cam.inv_view, cam.r2v, full, tile, off, *march)
    log, sums = [], {}
    features_ref.features_fetch(res, dens, alb, (-0.5,) * 3, (0.5,) * 3, media.SCALE, cam.inv_view, cam.r2v, full, tile, off, 0,
                                *march, taps=log, sums=sums)
    got = np.concatenate(log)
    order = lambda a: a[np.lexsort(a.T)]  # noqa: E731
    assert got.shape == want.shape and np.array_equal(order(got), order(want))
    assert np.array_equal(bits(sums["T"]), bits(T))
    if name == "sparse_small":
        assert (T < march[1]).sum() > 50   # rays that end early: the log stops with them
    cut = []
    features_ref.features_fetch(res, dens, alb, (-0.5,) * 3, (0.5,) * 3, media.SCALE, cam.inv_view, cam.r2v, full, tile, off, 0,
                                *march, taps=cut, support=features_ref.leaf_support(sp.table))
    cut = np.concatenate(cut)
    # what the support passes by are whole samples of the plain loop, none of them of a stored leaf
    u_all, c_all = np.unique(want, axis=0, return_counts=True)
    u_cut, c_cut = np.unique(cut, axis=0, return_counts=True)
    all_counts = {tuple(r): int(c) for r, c in zip(u_all.tolist(), c_all)}
    assert all(all_counts.get(tuple(r), 0) == int(c) for r, c in zip(u_cut.tolist(), c_cut))


def test_leaf_fetch_values():
    """NO_LEAF: density 0, the background albedo; a stored leaf: the pool's voxel."""
    sp = media.sparse_small()
    dens, alb = features_ref.leaf_fetch(sp.res, sp.table, sp.leaf_density, sp.leaf_albedo, sp.albedo_bg)
    D, A = devmed.densify(sp)
    z, y, x = (v.ravel() for v in np.meshgrid(*(np.arange(n) for n in D.shape), indexing="ij"))
    assert np.array_equal(bits(dens(x, y, z)), bits(D.ravel()))
    assert np.array_equal(bits(alb(x, y, z)), bits(A.reshape(-1, 4)[:, :3]))
    gone = sp.table[z >> 3, y >> 3, x >> 3] == features_ref.NO_LEAF
    assert gone.sum() > 1000 and not dens(x, y, z)[gone].any()
    assert (alb(x, y, z)[gone] == np.asarray(sp.albedo_bg, F)[:3]).all()
    none, bg = features_ref.leaf_fetch(sp.res, sp.table, sp.leaf_density, None, sp.albedo_bg)
    assert (bg(x, y, z) == np.asarray(sp.albedo_bg, F)[:3]).all()


# ------------------------------------------------------- the limit cases ----
@pytest.fixture(scope="module")
def logs():
    """name -> (case, feat_rgba of the reference, (x1, y1, z1) of its in-grid taps), marched once."""
    cache = {}

    def get(name):
        if name not in cache:
            case = limits.MEDIA[name]()
            taps = []
            rgba, _ = view_limits.ref_features(case, "full", taps)
            grid = view_limits.in_grid_taps(case, taps)
            if case.kind == "dense":  # keep the shape, not the 0.7 GB of arrays
                shape = case.medium.density.shape
                case = case._replace(medium=case.medium._replace(density=np.broadcast_to(F(0), shape), albedo=None))
            cache[name] = (case, rgba, grid)
        return cache[name]

    return get


# name -> (mult, prod, x, swap, shift): which narrowings the case's construction can show
KINDS = ("mult", "prod", "x", "swap", "shift")
CAN_SHOW = {
    "sparse_xy_limit": (1, 1, 0, 1, 1), "sparse_xy_limit_b2": (1, 1, 0, 1, 1), "sparse_xy_limit_b1": (1, 1, 0, 1, 1),
    "sparse_long_x": (0, 0, 1, 0, 1), "sparse_long_z": (1, 1, 0, 0, 1), "sparse_thin_mask": (0, 0, 0, 0, 1),
    "dense_xy_limit": (0, 1, 0, 0, 0), "dense_yz_limit": (0, 1, 0, 0, 0),
}
MASK_MODELS = {"sparse_long_x": (14, 11, 0, 0), "sparse_long_z": (16, 0, 0, 11), "sparse_thin_mask": (8, 11, 0, 0)}


@pytest.mark.parametrize("name", list(limits.MEDIA))
def test_taps_are_sharp(logs, name):
    case, _, (x1, y1, z1) = logs(name)
    counts = [int(v.sum()) for v in view_limits.narrowed(case, x1, y1, z1)]
    if case.kind == "sparse":
        counts += [int(v.sum()) for v in view_limits.mask_variants(case, x1, y1, z1)]
        if name in MASK_MODELS:  # the swap is a no-op by construction: lx = ly = 0 or ly = lz = 0
            assert limits.emask_model(case)[:4] == MASK_MODELS[name]
    else:
        counts += [0, 0]
    print(f"{name}: {x1.size} taps in the grid; " + ", ".join(f"{k} {c}" for k, c in zip(KINDS, counts)))
    for can, count, what in zip(CAN_SHOW[name], counts, KINDS):
        if can:
            assert count >= limits.MIN_SHARP, what
        else:
            assert count == 0, what   # (by construction: the docstring's table is not out of date)


@pytest.mark.parametrize("name", list(limits.MEDIA))
def test_reference_is_opaque(logs, name):
    _, rgba, _ = logs(name)
    share = float((rgba[..., 3] > 0).mean())
    print(f"{name}: {100 * share:.1f} % of the pixels have W > 0")
    assert rgba.shape == (32, 32, 4) and share >= 0.95


@pytest.mark.parametrize("name", limits.DENSE)
def test_dense_restatement_equals_host(cvr, name):
    """The dense cases' reference is the host statement; the restatement that logs their taps
    returns the same bits."""
    case = limits.MEDIA[name]()
    m = case.medium
    desc, keep = cvr.medium_from_arrays(m.density, m.albedo, case.box_min, case.box_max, case.scale, m.max_density)
    cam = limits.camera(case)
    march = cvr.FeaturesDesc(view_limits.step_of(case), view_limits.T_STOP, view_limits.MAX_STEPS)
    for view, (full, tile, off) in view_limits.VIEWS.items():
        host = cvr.features_host(desc, cam.inv_view, cam.r2v, full, tile, off, 0, march)
        ref = view_limits.ref_features(case, view)
        assert np.array_equal(bits(ref[0]), bits(host[0])) and np.array_equal(bits(ref[1]), bits(host[1])), view
    for shaded in (True, False):
        kw = dict(light=view_limits.LIGHT, flags=0) if shaded else dict(flags=1)
        host = cvr.preview_host(desc, cam.inv_view, cam.r2v, (32, 32), None, (0, 0), 0, cvr.PreviewDesc(march, **kw))
        assert np.array_equal(bits(view_limits.ref_preview(case, shaded)), bits(host)), shaded
