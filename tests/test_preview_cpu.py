"""The shaded preview pass (CVR_HAS_PREVIEW inside ABI 6), the parts that need no GPU: the surface,
the refusals in the header's order, cvr_preview_host against the independent numpy restatement of
tests/preview_ref.py, and what the picture must show.

preview_host == restatement: preview_ref states every operation of include/cvr.h (the fused
multiply-adds of the trilinear through features_ref's exact fp64 construction), so all four planes
are compared bit for bit (uint32 views), never within a tolerance.

Media: blob16 and the ragged 24x17x19 grid of tests/test_gpu_features.py (built here by the same
recipe).  Cameras: "oblique", "inside" and the pencil "pencil_in".  Tiles: 13x7 and 40x24 at offset
(8, 8) of 64x48.

Shading acts (test_shading_acts): the default shaded image (headlight, 0.3 / 0.7 / 0.2, exponent 2^4,
knee 0.05) differs in bits from the unshaded one in at least 90 % of the pixels with alpha > 0.
Measured with this statement: 100 % in all four cases (765, 960, 801 and 960 lit pixels).

The light has a direction (test_light_has_a_direction): blob16, "oblique", 64x64, specular 0; with
the light along +camera-right the right half is brighter relative to the unshaded image than the
left, r_R - r_L >= 0.1, and the other way round with the light along -camera-right.  Measured with
this statement: +0.1928 and +0.2431 (the prototype of the statement gave +0.19 and +0.24)."""
import ctypes as C
import os
from functools import lru_cache

import numpy as np
import pytest

import params
import preview_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
F = np.float32
UNIT = ((-0.5,) * 3, (0.5,) * 3)
BOX = (params._BOX_ALL["box_min"], params._BOX_ALL["box_max"])
FULL = (64, 48)
SMALL_TILES = [((13, 7), (8, 8)), ((40, 24), (8, 8))]
CAMERAS = ["oblique", "inside", "pencil_in"]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@lru_cache(maxsize=None)
def arrays(name):
    """(density (z, y, x), albedo (z, y, x, 4)): blob16, or the ragged 24 x 17 x 19 grid of
    tests/test_gpu_features.py (3 x 3 x 3 leaves, 11 of them empty, the others partly)."""
    if name == "blob16":
        d, a = params.blob16()
    else:
        rng = np.random.default_rng(5)
        d = rng.random((19, 17, 24), dtype=F)
        d[rng.random(d.shape) < 0.5] = 0.0
        d[:8, :, 16:] = 0.0
        d[8:16, 8:16, 8:16] = 0.0
        d[16:, :8, :] = 0.0
        d[:, 16:, :8] = 0.0
        a = np.ones(d.shape + (4,), F)
        a[..., :3] = (0.7, 0.55, 0.33)
        a[..., :3] = np.where((d > 0)[..., None], 0.2 + 0.8 * rng.random(d.shape + (3,), dtype=F), a[..., :3])
        a[0, 0, 0, :3] = (0.7, 0.55, 0.33)
        d[0, 0, 0] = 0.0
    d, a = np.ascontiguousarray(d, F), np.ascontiguousarray(a, F)
    for x in (d, a):
        x.setflags(write=False)
    return d, a


# name -> (PreviewDesc keywords, march (step, t_stop, max_steps), box, world_to_aabb)
DESCS = {
    "headlight_k0": (dict(specular=0.2, shininess_log2=0), (1.0, 1.0 / 256.0, 4096), UNIT, 0),
    "headlight_k4": (dict(specular=0.2, shininess_log2=4), (1.0, 1.0 / 256.0, 4096), UNIT, 0),
    "directional": (dict(light=(0.3, 1.0, -0.4), specular=0.0), (1.0, 1.0 / 256.0, 4096), UNIT, 0),
    "directional_specular": (dict(light=(-1.0, 0.2, 0.5), specular=0.4, shininess_log2=3), (1.0, 1.0 / 256.0, 4096), UNIT, 0),
    "unshaded": (dict(flags=preview_ref.UNSHADED), (1.0, 1.0 / 256.0, 4096), UNIT, 0),
    "background": (dict(background=(0.25, 0.5, 0.125), knee=0.2), (1.0, 1.0 / 256.0, 4096), UNIT, 0),
    "half_step": (dict(), (0.5, 0.0, 4096), UNIT, 0),
    "box_w2a": (dict(background=(0.1, 0.0, 0.3)), (1.0, 1.0 / 256.0, 4096), BOX, 1),
}


def make_desc(cvr, kw, march=(1.0, 1.0 / 256.0, 4096)):
    return cvr.PreviewDesc(cvr.FeaturesDesc(*march), **kw)


def host(cvr, name, camera, full, tile=None, offset=(0, 0), kw=None, march=(1.0, 1.0 / 256.0, 4096), box=UNIT, w2a=0,
         max_density=1.0):
    d, a = arrays(name)
    m, keep = cvr.medium_from_arrays(d, a, box[0], box[1], scale=params.SCALE, max_density=max_density)
    cam = params.camera(camera, full)
    return cvr.preview_host(m, cam.inv_view, cam.r2v, full, tile, offset, w2a, make_desc(cvr, kw or {}, march))


def ref(name, camera, full, tile=None, offset=(0, 0), kw=None, march=(1.0, 1.0 / 256.0, 4096), box=UNIT, w2a=0,
        max_density=1.0):
    d, a = arrays(name)
    cam = params.camera(camera, full)
    kw = dict(kw or {})
    if "flags" not in kw:
        kw["flags"] = 0 if "light" in kw else preview_ref.HEADLIGHT
    return preview_ref.preview(d, a, box[0], box[1], params.SCALE, max_density, cam.inv_view, cam.r2v, full, tile or full,
                               offset, w2a, march[0], march[1], march[2], **kw)


# ----------------------------------------------------------------- surface --
def test_surface(cvr):
    lib = cvr.load()
    for name in ("cvr_preview_host", "cvr_preview_buffers", "cvr_preview"):
        assert hasattr(lib, name), name
    assert C.sizeof(cvr.PreviewDesc) == 64
    assert [f for f, _ in cvr.PreviewDesc._fields_] == ["march", "light", "ambient", "diffuse", "specular",
                                                        "shininess_log2", "knee", "background", "flags"]
    d = cvr.PreviewDesc()
    assert (d.march.step, d.march.t_stop, d.march.max_steps, d.march.flags) == (1.0, 1.0 / 256.0, 4096, 0)
    assert (d.ambient, d.diffuse, d.specular, d.shininess_log2, d.knee) == (F(0.3), F(0.7), F(0.2), 4, F(0.05))
    assert tuple(d.background) == (0.0, 0.0, 0.0) and d.flags == cvr.PREVIEW_HEADLIGHT == 2 and cvr.PREVIEW_UNSHADED == 1
    assert cvr.PreviewDesc(light=(1, 0, 0)).flags == 0
    for name in ("preview", "preview_buffers"):
        assert hasattr(cvr.Context, name), name
    hdr = open(os.path.join(ROOT, "include", "cvr.h")).read()
    assert "#define CVR_HAS_PREVIEW 1" in hdr
    assert lib.cvr_abi_version() == 6  # an addition within ABI 6


# ------------------------------------------------- host == the restatement --
@pytest.mark.parametrize("name", ["blob16", "ragged"])
@pytest.mark.parametrize("desc", list(DESCS))
def test_host_matches_restatement(cvr, name, desc):
    kw, march, box, w2a = DESCS[desc]
    lit = 0
    for camera in CAMERAS:
        for tile, off in SMALL_TILES:
            got = host(cvr, name, camera, FULL, tile, off, kw, march, box, w2a)
            want = ref(name, camera, FULL, tile, off, kw, march, box, w2a)
            assert np.array_equal(bits(got[..., 3]), bits(want[..., 3])), f"{camera} {tile}: alpha"
            assert np.array_equal(bits(got[..., :3]), bits(want[..., :3])), f"{camera} {tile}: rgb"
            lit += int((got[..., 3] > 0).sum())
    assert lit > 500


def test_max_density_scales_the_knee(cvr):
    """knee_abs is knee times the majorant over the finest cell: another max_density, another blend."""
    one = host(cvr, "blob16", "oblique", FULL, (40, 24), (8, 8))
    two = host(cvr, "blob16", "oblique", FULL, (40, 24), (8, 8), max_density=2.5)
    want = ref("blob16", "oblique", FULL, (40, 24), (8, 8), max_density=2.5)
    assert np.array_equal(bits(two), bits(want)) and not np.array_equal(bits(one), bits(two))


# ------------------------------------------ unshaded == the feature pass ----
@pytest.mark.parametrize("name", ["blob16", "ragged"])
@pytest.mark.parametrize("camera", ["oblique", "inside"])
def test_unshaded_is_the_feature_pass(cvr, name, camera):
    d, a = arrays(name)
    m, keep = cvr.medium_from_arrays(d, a, scale=params.SCALE, max_density=1.0)
    cam = params.camera(camera, FULL)
    feat, _ = cvr.features_host(m, cam.inv_view, cam.r2v, FULL, (40, 24), (8, 8))
    prev = host(cvr, name, camera, FULL, (40, 24), (8, 8), dict(flags=cvr.PREVIEW_UNSHADED))
    assert np.array_equal(bits(prev[..., 3]), bits(feat[..., 3]))
    nz = prev[..., 3] != 0
    assert nz.sum() > 500
    mean = prev[..., :3][nz] / prev[..., 3][nz][:, None]
    assert np.array_equal(bits(mean), bits(feat[..., :3][nz]))
    assert not prev[~nz].any()


# ------------------------------------------------------------ shading acts --
@pytest.mark.parametrize("name", ["blob16", "ragged"])
@pytest.mark.parametrize("camera", ["oblique", "inside"])
def test_shading_acts(cvr, name, camera):
    shaded = host(cvr, name, camera, FULL, (40, 24), (8, 8))
    flat = host(cvr, name, camera, FULL, (40, 24), (8, 8), dict(flags=cvr.PREVIEW_UNSHADED))
    assert np.array_equal(bits(shaded[..., 3]), bits(flat[..., 3]))  # the light does not change the opacity
    lit = flat[..., 3] > 0
    differs = (bits(shaded[..., :3]) != bits(flat[..., :3])).any(-1)
    print(f"{name} {camera}: {int(lit.sum())} lit pixels, {int((differs & lit).sum())} of them differ from the unshaded image")
    assert lit.sum() > 500 and (differs & lit).sum() >= 0.9 * lit.sum()


def test_light_has_a_direction(cvr):
    full = (64, 64)
    cam = params.camera("oblique", full)
    right = np.asarray(cam.inv_view, F).reshape(3, 4)[:, 0]
    flat = host(cvr, "blob16", "oblique", full, kw=dict(flags=cvr.PREVIEW_UNSHADED))[..., :3].astype(np.float64)

    def ratios(light):
        img = host(cvr, "blob16", "oblique", full, kw=dict(light=tuple(light), specular=0.0))[..., :3].astype(np.float64)
        return img[:, :32].sum() / flat[:, :32].sum(), img[:, 32:].sum() / flat[:, 32:].sum()

    l1, r1 = ratios(right)
    l2, r2 = ratios(-right)
    print(f"light along +right: r_R - r_L = {r1 - l1:+.4f}; along -right: r_L - r_R = {l2 - r2:+.4f}")
    assert r1 - l1 >= 0.1 and l2 - r2 >= 0.1


@pytest.mark.parametrize("name", ["blob16", "ragged"])
@pytest.mark.parametrize("camera", ["oblique", "inside"])
def test_no_energy_is_added(cvr, name, camera):
    """ambient + diffuse <= 1 and specular 0: f <= 1, so every e_c is a convex mix of c_c and at most c_c."""
    flat = host(cvr, name, camera, FULL, (40, 24), (8, 8), dict(flags=cvr.PREVIEW_UNSHADED))
    for kw in (dict(specular=0.0), dict(specular=0.0, light=(0.2, -1.0, 0.3)), dict(specular=0.0, ambient=0.5, diffuse=0.5)):
        shaded = host(cvr, name, camera, FULL, (40, 24), (8, 8), kw)
        assert (shaded[..., :3].astype(np.float64) <= flat[..., :3].astype(np.float64) * (1 + 1e-5)).all(), kw


# -------------------------------------------------------------- background --
@pytest.mark.parametrize("camera", ["oblique"] + params.ALL_MISS)
def test_background(cvr, camera):
    bg = (0.25, 0.5, 0.125)
    full = (32, 32) if camera == "oblique" else (3, 3)
    for kw in (dict(background=bg), dict(background=bg, flags=cvr.PREVIEW_UNSHADED)):
        img = host(cvr, "blob16", camera, full, kw=kw)
        cam = params.camera(camera, full)
        o, d = preview_ref.rays(cam.inv_view, cam.r2v, full, full, (0, 0))
        has = preview_ref.chord(o, d, np.array(UNIT[0], F), np.array(UNIT[1], F))[0].reshape(full[1], full[0])
        assert (~has).any() and (has.any() or camera in params.ALL_MISS)
        assert np.array_equal(bits(img[~has]), bits(np.broadcast_to(np.array(bg + (0.0,), F), img[~has].shape)))
        if has.any():  # over the medium the background shows through by the transmittance left
            assert (img[has][:, 3] > 0).any() and (img[..., 3] <= 1).all()


# ---------------------------------------------------------------- refusals --
def test_refusals_in_the_headers_order(cvr):
    lib = cvr.load()
    d, a = arrays("blob16")
    m, keep = cvr.medium_from_arrays(d, a, scale=params.SCALE, max_density=1.0)
    cam = params.camera("oblique", (8, 8))
    iv = np.ascontiguousarray(cam.inv_view, F)
    r2v = np.ascontiguousarray(cam.r2v, F)
    fr = np.array([8, 8], F)
    out = np.zeros((8, 8, 4), F)
    fp = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    nan, inf = float("nan"), float("inf")
    P, M = cvr.PreviewDesc, cvr.FeaturesDesc

    def call(desc=None, med=m, w=8, h=8, w2a=0, dst=out, null_desc=False):
        desc = P() if desc is None else desc
        return lib.cvr_preview_host(None if med is None else C.byref(med), fp(iv), fp(r2v), fp(fr), w, h, 0, 0, w2a,
                                    None if null_desc else C.byref(desc), None if dst is None else dst.ctypes.data)

    def message(desc):
        with pytest.raises(cvr.CvrError) as e:
            cvr.preview_host(m, iv, r2v, (8, 8), desc=desc)
        assert e.value.code == INVALID
        return str(e.value)

    assert call() == 0 and call(w2a=1) == 0
    for ok in (P(flags=3), P(flags=1, light=(nan, 0, 0)), P(flags=2, light=(0, 0, 0)), P(ambient=0.0, diffuse=0.0, specular=0.0),
               P(shininess_log2=0), P(shininess_log2=10), P(knee=0.0), P(background=(3.0, 0.0, 1e6)), P(light=(0, 0, 1e-18)),
               P(ambient=4.0, diffuse=2.0)):
        assert call(ok) == 0
    # 1. a NULL descriptor
    assert call(null_desc=True) == INVALID
    # 2. the march checks of cvr_features
    for bad in (M(0.1249), M(8.001), M(nan), M(1.0, -0.001), M(1.0, 1.0), M(1.0, nan), M(1.0, 0.5, 0), M(1.0, 0.5, 65537),
                M(1.0, 0.5, 4096, 1)):
        assert call(P(bad)) == INVALID, (bad.step, bad.t_stop, bad.max_steps, bad.flags)
    # 3. unknown flag bits
    for flags in (4, 8, 1 << 31, 7):
        assert call(P(flags=flags)) == INVALID, flags
    # 4. the weights
    for field in ("ambient", "diffuse", "specular"):
        for v in (-0.001, nan, inf, -inf):
            assert call(P(**{field: v})) == INVALID, (field, v)
    # 5. the exponent
    assert call(P(shininess_log2=11)) == INVALID and call(P(shininess_log2=1 << 31)) == INVALID
    # 6. the knee
    for v in (-0.001, nan, inf):
        assert call(P(knee=v)) == INVALID, v
    # 7. the background
    for k in range(3):
        for v in (-0.5, nan, inf):
            bg = [0.0, 0.0, 0.0]
            bg[k] = v
            assert call(P(background=bg)) == INVALID, bg
    # 8. the light, read only without both flags
    for light in ((0, 0, 0), (nan, 1, 0), (0, inf, 0), (0, 0, -inf), (-0.0, 0.0, -0.0), (0, 1e-30, 0), (1e30, 0, 0)):
        assert call(P(light=light)) == INVALID, light
        assert call(P(light=light, flags=1)) == 0 and call(P(light=light, flags=2)) == 0
    # the order: of two faults the earlier one in the list is the one reported
    bad_light = dict(light=(0, 0, 0), flags=0)
    assert "step" in message(P(M(9.0), flags=4))
    assert "flags" in message(P(flags=4, ambient=-1.0))
    assert "ambient" in message(P(ambient=-1.0, shininess_log2=11))
    assert "shininess" in message(P(shininess_log2=11, knee=-1.0))
    assert "knee" in message(P(knee=-1.0, background=(-1, 0, 0)))
    assert "background" in message(P(background=(0, -1, 0), **bad_light))
    assert "light" in message(P(**bad_light))
    # and what cvr_features_host refuses besides
    assert call(med=None) == INVALID and call(dst=None) == INVALID
    assert call(w=0) == INVALID and call(h=0) == INVALID and call(w2a=2) == INVALID
    assert call(w=4097, h=4096) == INVALID
    for field in ("density", "albedo"):
        m2, keep2 = cvr.medium_from_arrays(d, a, scale=params.SCALE, max_density=1.0)
        setattr(m2, field, None)
        assert call(med=m2) == INVALID
