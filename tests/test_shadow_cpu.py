"""The light volume and the shadowed preview (CVR_HAS_SHADOWS inside ABI 6), the parts that need no
GPU: the surface, cvr_light_volume_host and cvr_preview_shadowed_host against the independent numpy
restatement of tests/shadow_ref.py, the exact properties the statement was written for, what the
picture must show, and the refusals in the header's order.

host == restatement: shadow_ref states every operation of include/cvr.h, so volumes and images are
compared bit for bit (uint32 views), never within a tolerance.  Media: blob16 and the ragged
24x17x19 grid of tests/test_preview_cpu.py.  Light grids 1x1x1, 13x11x9 and the medium's own res; the
lights (0, 0, 1) and (0.3, 1.0, -0.4); the unit box, the non-unit box with world_to_aabb 1, a half
step and t_stop 0.

Shadows have a side (test_shadows_have_a_side): blob16, "oblique", 64x64, specular 0, shadow 1, the
default 8x8x8 grid.  r = the mean over the pixels with alpha > 0 of a half of (sum of shadowed rgb /
sum of unshadowed rgb); with the light along +camera-right the left half (away from the light) is
darker, r_R - r_L, and with the light along -camera-right the right half, r_L - r_R.  Measured with
this statement: +0.2811 and +0.2969; the test requires half of each, 0.140 and 0.148.

Shadows act where shading cannot (test_shadows_act_in_a_homogeneous_medium): a 12^3 grid of one
density has no gradient anywhere (the clamped taps repeat the value), so the default shaded preview
is the unshaded one in bits on every pixel, while the shadowed one is darker on every pixel with
alpha > 0: measured 1417 of 1417."""
import ctypes as C
import os

import numpy as np
import pytest

import params
import shadow_ref
from test_preview_cpu import BOX, FULL, UNIT, arrays, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
F = np.float32
TILE, OFF = (40, 24), (8, 8)
LIGHTS = [(0.0, 0.0, 1.0), (0.3, 1.0, -0.4)]
MARCH = (1.0, 1.0 / 256.0, 4096)
# name -> (march (step, t_stop, max_steps), box, world_to_aabb)
VARIANTS = {
    "unit": (MARCH, UNIT, 0),
    "box_w2a": (MARCH, BOX, 1),
    "half_step": ((0.5, 1.0 / 256.0, 4096), UNIT, 0),
    "t_stop_0": ((1.0, 0.0, 4096), UNIT, 0),
}


def medium(cvr, name, box=UNIT, max_density=1.0):
    d, a = arrays(name)
    return cvr.medium_from_arrays(d, a, box[0], box[1], scale=params.SCALE, max_density=max_density)


def volume(cvr, name, res, light, march=MARCH, box=UNIT, w2a=0):
    m, keep = medium(cvr, name, box)
    vd = cvr.LightVolumeDesc(res, light, cvr.FeaturesDesc(*march))
    return vd, cvr.light_volume_host(m, vd, w2a)


def shadowed(cvr, name, camera, vd, S, shadow, kw=None, march=MARCH, box=UNIT, w2a=0, full=FULL, tile=TILE, off=OFF):
    m, keep = medium(cvr, name, box)
    cam = params.camera(camera, full)
    kw = dict(kw or {})
    kw.setdefault("flags", 0)
    desc = cvr.PreviewDesc(cvr.FeaturesDesc(*march), **kw)
    return cvr.preview_shadowed_host(m, cam.inv_view, cam.r2v, full, vd, S, tile, off, w2a, desc, shadow)


def plain(cvr, name, camera, kw, march=MARCH, box=UNIT, w2a=0, full=FULL, tile=TILE, off=OFF):
    m, keep = medium(cvr, name, box)
    cam = params.camera(camera, full)
    return cvr.preview_host(m, cam.inv_view, cam.r2v, full, tile, off, w2a, cvr.PreviewDesc(cvr.FeaturesDesc(*march), **kw))


# ----------------------------------------------------------------- surface --
def test_surface(cvr):
    lib = cvr.load()
    for name in ("cvr_light_volume_host", "cvr_build_light_volume", "cvr_light_volume_default_res", "cvr_light_volume_info",
                 "cvr_copy_light_volume", "cvr_clear_light_volume", "cvr_preview_shadowed_host",
                 "cvr_preview_shadowed_buffers", "cvr_preview_shadowed"):
        assert hasattr(lib, name), name
    assert C.sizeof(cvr.LightVolumeDesc) == 48 and C.sizeof(cvr.LightVolumeInfo) == 40
    assert [f for f, _ in cvr.LightVolumeDesc._fields_] == ["res", "flags", "light", "reserved", "march"]
    d = cvr.LightVolumeDesc((3, 4, 5), (1, 2, 3))
    assert tuple(d.res) == (3, 4, 5) and tuple(d.light) == (1.0, 2.0, 3.0) and d.flags == 0
    assert (d.march.step, d.march.t_stop, d.march.max_steps, d.march.flags) == (1.0, 1.0 / 256.0, 4096, 0)
    for name in ("build_light_volume", "light_volume", "light_volume_info", "clear_light_volume", "preview_shadowed",
                 "preview_shadowed_buffers"):
        assert hasattr(cvr.Context, name), name
    hdr = open(os.path.join(ROOT, "include", "cvr.h")).read()
    assert "#define CVR_HAS_SHADOWS 1" in hdr
    assert lib.cvr_abi_version() == 6  # an addition within ABI 6


# ------------------------------------------------- host == the restatement --
@pytest.mark.parametrize("name", ["blob16", "ragged"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_host_matches_restatement(cvr, name, variant):
    march, box, w2a = VARIANTS[variant]
    d, a = arrays(name)
    shadowed_nodes = lit = 0
    for res in ((1, 1, 1), (13, 11, 9), d.shape[::-1]):
        for n, light in enumerate(LIGHTS):
            vd, S = volume(cvr, name, res, light, march, box, w2a)
            want = shadow_ref.light_volume(d, box[0], box[1], params.SCALE, res, light, w2a, *march)
            assert np.array_equal(bits(S), bits(want)), f"volume {res} {light}"
            shadowed_nodes += int((S < 1).sum())
            # the pass on that volume: shaded and unshaded, both cameras, shadow 0.5 and 1
            for camera, kw, shadow in (("oblique", dict(specular=0.3, shininess_log2=3, background=(0.25, 0.5, 0.125)), 0.5),
                                       ("inside", dict(flags=1) if n else dict(), 1.0)):
                got = shadowed(cvr, name, camera, vd, S, shadow, kw, march, box, w2a)
                cam = params.camera(camera, FULL)
                ref = shadow_ref.preview_shadowed(d, a, box[0], box[1], params.SCALE, 1.0, cam.inv_view, cam.r2v, FULL, TILE, S,
                                                  light, shadow, OFF, w2a, *march, **kw)
                assert np.array_equal(bits(got[..., 3]), bits(ref[..., 3])), f"{res} {light} {camera}: alpha"
                assert np.array_equal(bits(got[..., :3]), bits(ref[..., :3])), f"{res} {light} {camera}: rgb"
                lit += int((got[..., 3] > 0).sum())
    assert shadowed_nodes > 1000 and lit > 3000


# -------------------------------------------------------- exact properties --
@pytest.mark.parametrize("name", ["blob16", "ragged"])
@pytest.mark.parametrize("camera", ["oblique", "inside"])
def test_exact_properties(cvr, name, camera):
    light = LIGHTS[1]
    vd, S = volume(cvr, name, (13, 11, 9), light)
    assert (S >= 0).all() and (S <= 1).all() and (S < 0.5).any()
    for kw in (dict(), dict(flags=cvr.PREVIEW_UNSHADED), dict(specular=0.0, background=(0.25, 0.5, 0.125))):
        base = plain(cvr, name, camera, dict(kw, light=light, flags=kw.get("flags", 0)))
        # shadow = 0: cvr_preview's bits with the volume's light; the descriptor's own light is not read
        zero = shadowed(cvr, name, camera, vd, S, 0.0, dict(kw, light=(9.0, 9.0, 9.0)))
        assert np.array_equal(bits(zero), bits(base)), kw
        assert (base[..., 3] > 0).sum() > 500
        for shadow in (0.5, 1.0):
            img = shadowed(cvr, name, camera, vd, S, shadow, kw)
            assert np.array_equal(bits(img[..., 3]), bits(base[..., 3])), (kw, shadow)  # the alpha plane
            assert (img[..., :3] <= base[..., :3]).all(), (kw, shadow)  # fp32 multiply and add are monotone
            assert (img[..., :3] < base[..., :3]).any()
        half, full = (shadowed(cvr, name, camera, vd, S, s, kw) for s in (0.5, 1.0))
        assert (full[..., :3] <= half[..., :3]).all()


def test_empty_medium_casts_no_shadow(cvr):
    d, a = arrays("blob16")
    m, keep = cvr.medium_from_arrays(np.zeros_like(d), a, scale=params.SCALE, max_density=1.0)
    vd = cvr.LightVolumeDesc((13, 11, 9), LIGHTS[1])
    assert np.array_equal(bits(cvr.light_volume_host(m, vd)), bits(np.ones((9, 11, 13), F)))
    # S = 1 everywhere gives V = 1: the unshadowed image in bits, whatever the strength
    ones = np.ones((9, 11, 13), F)
    for camera in ("oblique", "inside"):
        for kw in (dict(), dict(flags=cvr.PREVIEW_UNSHADED)):
            base = plain(cvr, "ragged", camera, dict(kw, light=LIGHTS[1], flags=kw.get("flags", 0)))
            assert np.array_equal(bits(shadowed(cvr, "ragged", camera, vd, ones, 1.0, kw)), bits(base))


# --------------------------------------------- what the picture must show ---
def test_shadows_have_a_side(cvr):
    full = (64, 64)
    cam = params.camera("oblique", full)
    right = np.asarray(cam.inv_view, F).reshape(3, 4)[:, 0]

    def ratios(light):
        light = tuple(float(v) for v in light)
        vd, S = volume(cvr, "blob16", (8, 8, 8), light)
        kw = dict(specular=0.0)
        base = plain(cvr, "blob16", "oblique", dict(kw, light=light), full=full, tile=None, off=(0, 0))
        img = shadowed(cvr, "blob16", "oblique", vd, S, 1.0, kw, full=full, tile=None, off=(0, 0))
        on = base[..., 3] > 0
        r = np.where(on, img[..., :3].astype(np.float64).sum(-1) / np.where(on, base[..., :3].astype(np.float64).sum(-1), 1), 0)
        return r[:, :32].sum() / on[:, :32].sum(), r[:, 32:].sum() / on[:, 32:].sum()

    l1, r1 = ratios(right)
    l2, r2 = ratios(-right)
    print(f"light along +right: r_R - r_L = {r1 - l1:+.4f}; along -right: r_L - r_R = {l2 - r2:+.4f}")
    assert r1 - l1 >= 0.140 and l2 - r2 >= 0.148


def test_shadows_act_in_a_homogeneous_medium(cvr):
    d = np.full((12, 12, 12), 0.5, F)
    a = np.ones(d.shape + (4,), F)
    a[..., :3] = (0.7, 0.55, 0.33)
    m, keep = cvr.medium_from_arrays(d, a, scale=params.SCALE, max_density=1.0)
    cam = params.camera("oblique", FULL)
    lit = cvr.preview_host(m, cam.inv_view, cam.r2v, FULL)
    flat = cvr.preview_host(m, cam.inv_view, cam.r2v, FULL, desc=cvr.PreviewDesc(flags=cvr.PREVIEW_UNSHADED))
    assert np.array_equal(bits(lit), bits(flat))  # no gradient: the light of CVR_HAS_PREVIEW does nothing here
    vd = cvr.LightVolumeDesc((6, 6, 6), LIGHTS[1])
    S = cvr.light_volume_host(m, vd)
    img = cvr.preview_shadowed_host(m, cam.inv_view, cam.r2v, FULL, vd, S)
    on = flat[..., 3] > 0
    darker = (img[..., :3] < flat[..., :3]).all(-1)
    print(f"{int(on.sum())} pixels with alpha > 0, {int((darker & on).sum())} of them darker under shadows")
    assert on.sum() > 500 and (darker & on).sum() == on.sum()
    assert np.array_equal(bits(img[~on]), bits(flat[~on]))


# ---------------------------------------------------------------- refusals --
def test_refusals_in_the_headers_order(cvr):
    lib = cvr.load()
    m, keep = medium(cvr, "blob16")
    cam = params.camera("oblique", (8, 8))
    iv = np.ascontiguousarray(cam.inv_view, F)
    r2v = np.ascontiguousarray(cam.r2v, F)
    fr = np.array([8, 8], F)
    out = np.zeros((8, 8, 4), F)
    vol = np.ones((3, 3, 3), F)
    big = np.zeros(4 * 4 * 4, F)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    nan, inf = float("nan"), float("inf")
    P, M, V = cvr.PreviewDesc, cvr.FeaturesDesc, cvr.LightVolumeDesc
    good = V((3, 3, 3), (0, 0, 1))

    def build(desc=None, med=m, w2a=0, dst=big, null_desc=False):
        desc = V((4, 4, 4), (0, 0, 1)) if desc is None else desc
        return lib.cvr_light_volume_host(None if med is None else C.byref(med), w2a, None if null_desc else C.byref(desc),
                                         None if dst is None else dst.ctypes.data)

    def build_message(desc):
        with pytest.raises(cvr.CvrError) as e:
            cvr.light_volume_host(m, desc)
        assert e.value.code == INVALID
        return str(e.value)

    assert build() == 0 and build(w2a=1) == 0 and build(V((1, 1, 1), (0, 0, 1e-18))) == 0
    # 1. a NULL descriptor; 2. flags; 3. res; 4. the light; 5. the march
    assert build(null_desc=True) == INVALID
    for flags in (1, 2, 1 << 31):
        assert build(V((4, 4, 4), (0, 0, 1), flags=flags)) == INVALID
    for res in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (1025, 1, 1), (1, 1025, 1), (1, 1, 1 << 31), (1024, 1024, 129), (512, 513, 512)):
        assert build(V(res, (0, 0, 1))) == INVALID, res
    for light in ((0, 0, 0), (nan, 1, 0), (0, inf, 0), (0, 0, -inf), (-0.0, 0.0, -0.0), (0, 1e-30, 0), (1e30, 0, 0)):
        assert build(V((4, 4, 4), light)) == INVALID, light
    for bad in (M(0.1249), M(8.001), M(nan), M(1.0, -0.001), M(1.0, 1.0), M(1.0, 0.5, 0), M(1.0, 0.5, 65537), M(1.0, 0.5, 4096, 1)):
        assert build(V((4, 4, 4), (0, 0, 1), bad)) == INVALID
    assert "flags" in build_message(V((0, 4, 4), (0, 0, 0), M(9.0), flags=1))
    assert "res" in build_message(V((0, 4, 4), (0, 0, 0), M(9.0)))
    assert "2^27" in build_message(V((1024, 1024, 129), (0, 0, 0), M(9.0)))
    assert "light" in build_message(V((4, 4, 4), (0, 0, 0), M(9.0)))
    assert "step" in build_message(V((4, 4, 4), (0, 0, 1), M(9.0)))
    assert build(med=None) == INVALID and build(dst=None) == INVALID and build(w2a=2) == INVALID

    def call(desc=None, shadow=0.5, vd=good, med=m, w=8, h=8, w2a=0, dst=out, volume=vol, null_desc=False):
        desc = P(flags=0) if desc is None else desc
        return lib.cvr_preview_shadowed_host(None if med is None else C.byref(med), fp(iv), fp(r2v), fp(fr), w, h, 0, 0, w2a,
                                             None if null_desc else C.byref(desc), None if vd is None else C.byref(vd),
                                             None if volume is None else volume.ctypes.data, C.c_float(shadow),
                                             None if dst is None else dst.ctypes.data)

    def message(desc, shadow=0.5, vd=good):
        with pytest.raises(cvr.CvrError) as e:
            cvr.preview_shadowed_host(m, iv, r2v, (8, 8), vd, vol, desc=desc, shadow=shadow)
        assert e.value.code == INVALID
        return str(e.value)

    assert call() == 0 and call(w2a=1) == 0 and call(shadow=0.0) == 0 and call(shadow=1.0) == 0
    # the descriptor's light is neither read nor judged
    for light in ((0, 0, 0), (nan, 1, 0), (0, inf, 0)):
        assert call(P(light=light, flags=0)) == 0 and call(P(light=light, flags=1)) == 0
    # 1. what cvr_preview refuses: a NULL descriptor, the march, unknown flags, weights, exponent, knee, background
    assert call(null_desc=True) == INVALID
    for bad in (M(0.1249), M(1.0, 1.0), M(1.0, 0.5, 0), M(1.0, 0.5, 4096, 1)):
        assert call(P(bad, flags=0)) == INVALID
    assert call(P(flags=4)) == INVALID and call(P(flags=0, ambient=-1.0)) == INVALID and call(P(flags=0, diffuse=nan)) == INVALID
    assert call(P(flags=0, shininess_log2=11)) == INVALID and call(P(flags=0, knee=inf)) == INVALID
    assert call(P(flags=0, background=(0, -1, 0))) == INVALID
    # 2. the headlight
    assert call(P()) == INVALID and call(P(flags=2)) == INVALID and call(P(flags=3)) == INVALID
    # 3. the strength
    for s in (-0.001, 1.001, nan, inf, -inf):
        assert call(shadow=s) == INVALID, s
    # the order: of two faults the earlier one in the list is the one reported
    assert "step" in message(P(M(9.0), flags=6))
    assert "flags" in message(P(flags=6))
    assert "background" in message(P(flags=2, background=(0, -1, 0)))
    assert "HEADLIGHT" in message(P(flags=2), shadow=2.0)
    assert "shadow" in message(P(flags=0), shadow=2.0, vd=V((0, 3, 3), (0, 0, 1)))
    # and the volume's descriptor, the arrays and the tile
    assert call(vd=None) == INVALID and call(vd=V((0, 3, 3), (0, 0, 1))) == INVALID and call(vd=V((3, 3, 3), (0, 0, 0))) == INVALID
    assert call(volume=None) == INVALID and call(med=None) == INVALID and call(dst=None) == INVALID
    assert call(w=0) == INVALID and call(h=0) == INVALID and call(w2a=2) == INVALID and call(w=4097, h=4096) == INVALID
    with pytest.raises(cvr.CvrError):  # the binding checks the array against the descriptor's res
        cvr.preview_shadowed_host(m, iv, r2v, (8, 8), good, np.ones((3, 3, 4), F))
