"""The field projections (CVR_HAS_FIELD_PROJECT inside ABI 6), the parts that need no GPU: the
surface, cvr_field_project_host against the independent numpy restatement of tests/project_ref.py,
what the picture must show, and the ten refusals in the header's order.

field_project_host == restatement: project_ref states every operation of include/cvr.h (the fused
multiply-adds of the trilinear through features_ref's exact fp64 construction), so the rgba, value
and depth planes are compared bit for bit (uint32 views), never within a tolerance.

Fields (z, y, x): a ragged 37x29x23 one of each scalar type, a 5x1x3 one (an axis of one voxel), a
2x2x2 one, an f32 one with NaN and +-inf voxels and one that is all NaN.  Cameras: "oblique" (eye
outside), "inside", and two that miss the box.  Tile: the ragged 19x13 at offset (8, 8) of 64x48.

The ramp (test_ramp_isosurface): S = x on 17^3 voxels in the unit box, so the isosurface is the plane
x = iso - 0.5.  A hit found by the march lies in a bracket (ta, tb] of width delta / 2^refine that
contains the plane's t, so |t_hit - t_plane| <= delta / 2^refine + slack.  The slack: t_i, p, the
coordinate and the ramp's voxels are at most 16 fp32 roundings of quantities below 4, half an ulp
(2^-23) each, 2^-19 in x, over |d_x| >= 0.9 for this camera: 2^-18 in t.
The ramp's gradient is (1, 0, 0) up to rounding, so a surface is fully lit (nl = 1) where the ray
enters it, which is where S grows along the ray: the eye on the -x side looking along +x.  There
the centre pixel is (ambient + diffuse) colour within 16 half-ulps of quantities at most 1, 2^-20
(the gradient's three differences and divisions, its length, the normal, the dot product, f and the
product with the colour).  With the view direction -x itself the ray enters through the cut face
x = +0.5, S falls along it, nl = 0 and the centre pixel is ambient colour: asserted as well.

The window (test_window): the value plane does not depend on the window, and rgba = u(value) colour
with u of the header computed here from the value plane: exact, compared in bits ("clamp the
projection").  "Project the clamped field" is not the same number: a trilinear sample of clamped
voxels differs from the clamped sample.  For a window that holds the field's minimum, clamping the
voxels from above can only lower a sample (every lerp is monotone in its taps, in fp32 too), so the
clamped field's u is <= the original's per pixel, with equality on a field inside the window; both
are asserted."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import params
import project_ref
from features_ref import rays

INVALID = -1
F = np.float32
UNIT = ((-0.5,) * 3, (0.5,) * 3)
BOX = (params._BOX_ALL["box_min"], params._BOX_ALL["box_max"])
FULL, TILE, OFFSET = (64, 48), (19, 13), (8, 8)
MODES = ["max", "min", "mean", "iso"]
TYPES = ["float32", "uint8", "uint16", "int16"]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def away(full):
    return params.look_at((0, 0, 4), (0, 0, 8), full=full)


def camera(name, full):
    return away(full) if name == "away" else params.camera(name, full)


@lru_cache(maxsize=None)
def field(name):
    """A (z, y, x) field by name: ragged_<dtype>, thin (5x1x3 u16), cube (2x2x2 f32), nan, allnan."""
    rng = np.random.default_rng(11)
    if name.startswith("ragged_"):
        dtype = np.dtype(name[7:])
        if dtype == np.float32:
            a = rng.random((23, 29, 37), dtype=F)
        else:
            info = np.iinfo(dtype)
            a = rng.integers(info.min, info.max + 1, (23, 29, 37)).astype(dtype)
    elif name == "thin":
        a = rng.integers(0, 65536, (3, 1, 5)).astype(np.uint16)
    elif name == "cube":
        a = rng.random((2, 2, 2), dtype=F)
    elif name == "nan":
        a = rng.random((3, 4, 5), dtype=F)
        a[0, 1, 2], a[1, 3, 1], a[2, 1, 3], a[2, 3, 4] = np.nan, np.inf, -np.inf, np.nan
    elif name == "allnan":
        a = np.full((3, 4, 5), np.nan, F)
    else:
        raise KeyError(name)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def span(a):
    """(lo, hi, iso): a window inside the field's range and a level that cuts it."""
    if a.dtype == np.float32:
        return 0.2, 0.8, 0.6
    info = np.iinfo(a.dtype)
    w = float(info.max) - float(info.min)
    return info.min + 0.2 * w, info.min + 0.8 * w, info.min + 0.6 * w


def both(cvr, a, mode, cam="oblique", box=UNIT, full=FULL, tile=TILE, offset=OFFSET, **kw):
    """(host planes, restatement planes) of one case; kw: ProjectDesc keywords."""
    lo, hi, iso = span(a)
    kw = dict(dict(lo=lo, hi=hi, iso=iso), **kw)
    c = camera(cam, full)
    got = cvr.field_project_host(a, c.inv_view, c.r2v, full, cvr.ProjectDesc(mode, box[0], box[1], **kw), tile, offset)
    rk = dict(kw)
    if "flags" not in rk:
        rk["flags"] = 0 if "light" in rk else project_ref.HEADLIGHT
    want = project_ref.project(a, MODES.index(mode), box[0], box[1], c.inv_view, c.r2v, full, tile, offset, **rk)
    return got, want


def assert_planes(got, want, what):
    for name, g, w in zip(("rgba", "value", "depth"), got, want):
        assert g.shape == w.shape, f"{what}: {name} shape"
        assert np.array_equal(bits(g), bits(w)), f"{what}: {name}"


# ----------------------------------------------------------------- surface --
def test_surface(cvr):
    lib = cvr.load()
    for name in ("cvr_field_project_host", "cvr_field_project_buffers", "cvr_field_project"):
        assert hasattr(lib, name), name
    assert C.sizeof(cvr.ProjectDesc) == 112 and lib.cvr_abi_version() == 6
    d = cvr.ProjectDesc()
    assert (d.step, d.max_steps, d.refine, d.flags, d.shininess_log2) == (1.0, 4096, 4, cvr.PROJECT_HEADLIGHT, 4)
    assert (F(d.ambient), F(d.diffuse), F(d.specular)) == (F(0.3), F(0.7), F(0.2))
    assert tuple(d.colour) == (1.0, 1.0, 1.0) and tuple(d.background) == (0.0, 0.0, 0.0)


# ------------------------------------------- host == restatement, in bits ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", TYPES)
def test_types_and_modes(cvr, dtype, mode):
    got, want = both(cvr, field("ragged_" + dtype), mode, background=(0.25, 0.5, 0.125), colour=(0.9, 0.6, 0.3))
    assert_planes(got, want, f"{dtype} {mode}")
    alpha = got[0][..., 3]
    assert (alpha == 1).sum() > 50 and (alpha == 0).sum() > 5  # the tile sees the box and its outside


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["thin", "cube", "nan", "allnan"])
def test_small_and_nan_fields(cvr, name, mode):
    a = field(name)
    kw = dict(lo=0.2, hi=0.8, iso=0.6) if name in ("nan", "allnan") else {}
    for cam in ("oblique", "inside"):
        got, want = both(cvr, a, mode, cam, background=(0.25, 0.5, 0.125), **kw)
        assert_planes(got, want, f"{name} {mode} {cam}")
        if name == "allnan":  # every pixel is the background with alpha 0
            assert (got[0] == np.array([0.25, 0.5, 0.125, 0.0], F)).all() and not got[1].any() and not got[2].any()
        elif cam == "inside" and name != "nan" and mode != "iso":  # every ray has a chord and a sample
            assert (got[0][..., 3] == 1).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cam", ["inside", "pencil_out", "away"])
def test_cameras(cvr, cam, mode):
    got, want = both(cvr, field("ragged_uint8"), mode, cam, background=(0.5, 0.0, 1.0))
    assert_planes(got, want, f"{cam} {mode}")
    if cam != "inside":
        assert (got[0] == np.array([0.5, 0.0, 1.0, 0.0], F)).all()
    elif mode != "iso":
        assert (got[0][..., 3] == 1).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kw", [dict(box=BOX), dict(step=0.5), dict(step=2.0), dict(max_steps=5),
                                dict(box=BOX, step=0.125, max_steps=40, full=(19, 13), tile=(19, 13), offset=(0, 0))],
                         ids=["box", "half_step", "double_step", "truncated", "whole_image"])
def test_box_step_and_truncation(cvr, kw, mode):
    kw = dict(kw)
    geometry = {k: kw.pop(k) for k in ("box", "full", "tile", "offset") if k in kw}
    a = field("ragged_int16")
    got, want = both(cvr, a, mode, **geometry, **kw)
    assert_planes(got, want, f"{kw} {mode}")
    if kw.get("max_steps") == 5 and mode == "max":  # the march is cut short: the full one finds more
        full = both(cvr, a, mode)[0]
        assert (full[1] >= got[1]).all() and (full[1] > got[1]).any()


@pytest.mark.parametrize("kw", [dict(refine=0), dict(refine=4), dict(refine=8), dict(light=(0.3, 1.0, -0.4)),
                                dict(light=(-1.0, 0.2, 0.5), specular=0.4, shininess_log2=3), dict(shininess_log2=0),
                                dict(shininess_log2=10), dict(specular=0.0)],
                         ids=["refine0", "refine4", "refine8", "directional", "directional_specular", "k0", "k10", "matte"])
def test_iso_descriptors(cvr, kw):
    for name in ("ragged_float32", "ragged_uint16"):
        got, want = both(cvr, field(name), "iso", colour=(0.9, 0.6, 0.3), **kw)
        assert_planes(got, want, f"{name} {kw}")
        assert (got[0][..., 3] == 1).sum() > 50


def test_iso_misses_and_cut_faces(cvr):
    a = field("ragged_uint8")
    c = params.camera("oblique", FULL)
    chord = both(cvr, a, "max")[0][0][..., 3] == 1
    # above the field's maximum: a miss everywhere
    got, want = both(cvr, a, "iso", iso=float(a.max()) + 0.5, background=(0.1, 0.2, 0.3))
    assert_planes(got, want, "iso above the maximum")
    assert (got[0] == np.array([0.1, 0.2, 0.3, 0.0], F)).all() and not got[1].any() and not got[2].any()
    # at and below its minimum: every chord pixel hits at t_0, the sample MIN and MAX see first
    for iso in (float(a.min()), float(a.min()) - 3.0):
        got, want = both(cvr, a, "iso", iso=iso)
        assert_planes(got, want, "iso at the minimum")
        assert np.array_equal(got[0][..., 3] == 1, chord)
        first = both(cvr, a, "max", max_steps=1)[0]
        assert np.array_equal(bits(got[2]), bits(first[2])) and np.array_equal(bits(got[1]), bits(first[1]))


# ------------------------------------------------ what the picture must show --
RAMP_N = 17


def ramp():
    x = (np.arange(RAMP_N, dtype=F) / F(RAMP_N - 1)).astype(F)
    return np.ascontiguousarray(np.broadcast_to(x, (RAMP_N,) * 3))


@pytest.mark.parametrize("refine", [0, 4, 8])
def test_ramp_isosurface(cvr, refine):
    full = (33, 33)
    iso, amb, dif, col = 0.3, 0.3, 0.6, np.array([0.9, 0.6, 0.3], F)
    cam = params.look_at((-3, 0, 0), (0, 0, 0), full=full)
    desc = cvr.ProjectDesc("iso", iso=iso, refine=refine, ambient=amb, diffuse=dif, specular=0.0, colour=col)
    rgba, value, depth = cvr.field_project_host(ramp(), cam.inv_view, cam.r2v, full, desc)
    o, d = rays(cam.inv_view, cam.r2v, full, full, (0, 0))
    o, d = o.astype(np.float64), d.astype(np.float64)
    assert (d[:, 0] >= 0.9).all()
    t_plane = ((iso - 0.5) - o[0]) / d[:, 0]
    at = o + t_plane[:, None] * d
    on_plane = (np.abs(at[:, 1:]) < 0.45).all(axis=1)  # the ray meets the plane well inside the box
    assert on_plane.sum() > 100
    delta = 1.0 / RAMP_N
    slack = 2.0 ** -18
    t_hit = depth.ravel().astype(np.float64) * np.sqrt(3.0)
    err = np.abs(t_hit - t_plane)[on_plane]
    print(f"refine {refine}: largest |t_hit - t_plane| {err.max():.3e}, bound {delta / 2 ** refine + slack:.3e}")
    assert (rgba.reshape(-1, 4)[on_plane, 3] == 1).all()
    assert (err <= delta / 2 ** refine + slack + 3 * 2.0 ** -24 * 4).all()  # (+ the depth plane's own division)
    assert (np.abs(value.ravel()[on_plane] - iso) <= delta / 2 ** refine + 2.0 ** -19).all()
    # the centre pixel looks along +x exactly: fully lit
    centre = rgba[16, 16, :3].astype(np.float64)
    want = (np.float64(F(amb)) + np.float64(F(dif))) * col.astype(np.float64)
    print(f"centre pixel {centre}, ambient + diffuse {want}")
    assert np.abs(centre - want).max() <= 2.0 ** -20
    # the view direction -x: the cut face, S falls along the ray, no diffuse light
    back = params.look_at((3, 0, 0), (0, 0, 0), full=full)
    rgba, value, depth = cvr.field_project_host(ramp(), back.inv_view, back.r2v, full, desc)
    assert rgba[16, 16, 3] == 1 and value[16, 16] > 0.9
    assert np.abs(rgba[16, 16, :3].astype(np.float64) - np.float64(F(amb)) * col).max() <= 2.0 ** -20


def test_bright_voxel(cvr):
    n, full = 17, (33, 33)
    vox = (11, 5, 8)  # x, y, z
    a = np.zeros((n, n, n), F)
    a[vox[2], vox[1], vox[0]] = 1.0
    pos = np.array(vox, np.float64) / (n - 1) - 0.5  # voxel i sits at node i / (res - 1) of the box
    eye = np.array([2.1, 1.3, -1.7])
    cam = params.look_at(tuple(eye), tuple(pos), full=full)
    step = 0.125
    rgba, value, depth = cvr.field_project_host(a, cam.inv_view, cam.r2v, full, cvr.ProjectDesc("max", step=step))
    o, d = rays(cam.inv_view, cam.r2v, full, full, (0, 0))
    o, d = o.astype(np.float64), d.astype(np.float64)
    along = (pos - o) @ d.T
    dist = np.linalg.norm((o + along[:, None] * d) - pos, axis=1)
    nearest = int(np.argmin(dist))
    order = np.sort(dist)
    assert nearest == 16 * 33 + 16 and order[0] < 0.05 / (n - 1) and order[1] > 0.4 / (n - 1)  # the setup: a clear nearest ray
    assert int(np.argmax(value)) == nearest and value.ravel()[nearest] > 0.8
    delta = step / n
    assert abs(float(depth.ravel()[nearest]) * np.sqrt(3.0) - np.linalg.norm(pos - eye)) <= delta


@pytest.mark.parametrize("dtype", TYPES)
def test_min_below_max(cvr, dtype):
    a = field("ragged_" + dtype)
    c = params.camera("oblique", FULL)
    lo, hi, _ = span(a)
    out = {m: cvr.field_project_host(a, c.inv_view, c.r2v, FULL, cvr.ProjectDesc(m, lo=lo, hi=hi), (40, 24), OFFSET)
           for m in ("min", "max")}
    seen = out["max"][0][..., 3] == 1
    assert seen.sum() > 200
    assert (out["min"][1] <= out["max"][1]).all() and (out["min"][1][seen] < out["max"][1][seen]).any()
    assert (out["min"][0][..., :3] <= out["max"][0][..., :3]).all()


def test_window(cvr):
    a = field("ragged_uint8")
    c = params.camera("oblique", FULL)
    col = np.array([0.9, 0.6, 0.3], F)

    def run(arr, lo, hi):
        return cvr.field_project_host(arr, c.inv_view, c.r2v, FULL, cvr.ProjectDesc("max", lo=lo, hi=hi, colour=col), (40, 24), OFFSET)

    wide, win = run(a, 0.0, 255.0), run(a, 60.0, 180.0)
    assert np.array_equal(bits(wide[1]), bits(win[1])) and np.array_equal(bits(wide[2]), bits(win[2]))
    # clamp the projection: exact
    t = (win[1] - F(60.0)) / (F(180.0) - F(60.0))
    u = np.where(t > 0, t, F(0)).astype(F)
    u = np.where(u < 1, u, F(1)).astype(F)
    seen = win[0][..., 3] == 1
    assert np.array_equal(bits(win[0][..., :3][seen]), bits((u[..., None] * col)[seen]))
    assert (u[seen] == 1).any() and (u[seen] < 1).any()
    # project the clamped field: never above, for a window that holds the minimum
    top = run(a, 0.0, 180.0)
    clamped = run(np.minimum(a, 180).astype(np.uint8), 0.0, 180.0)
    assert (clamped[0][..., :3] <= top[0][..., :3]).all() and (clamped[1] <= 180).all()
    assert (clamped[1] <= top[1]).all()
    # ... and the same bits on a field that lies inside the window
    inside = np.clip(a, 60, 180).astype(np.uint8)
    x, y = run(inside, 60.0, 180.0), run(np.clip(inside, 60, 180).astype(np.uint8), 60.0, 180.0)
    assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(x, y))


# ---------------------------------------------------------------- refusals --
def test_refusals_in_order(cvr):
    """Each call breaks rule k and every later rule it can: the message is rule k's."""
    lib = cvr.load()
    a = np.ascontiguousarray(field("ragged_uint16"))
    c = params.camera("oblique", FULL)
    iv, r2v = np.ascontiguousarray(c.inv_view, F), np.ascontiguousarray(c.r2v, F)
    fr = np.array(FULL, F)
    out = np.zeros(4 * 4 + 8, F)
    start = (-out.ctypes.data // 4) % 4
    rgba = out.ctypes.data + 4 * start  # 16-byte aligned
    nan, inf = float("nan"), float("inf")

    def fdesc(**kw):
        f = cvr.FieldDesc()
        f.res[:] = kw.get("res", (37, 29, 23))
        f.scalar_type = kw.get("scalar_type", cvr.SCALAR_U16)
        f.scalar = kw.get("scalar", a.ctypes.data)
        f.reserved = kw.get("reserved", 0)
        return f

    def call(f, d, rgba_ptr=rgba, camera_ok=True):
        fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        rc = lib.cvr_field_project_host(None if f is None else C.byref(f), None if d is None else C.byref(d),
                                        fp(iv) if camera_ok else None, fp(r2v), fp(fr), 2, 2, 0, 0, rgba_ptr, None, None)
        return rc, (lib.cvr_last_error(None) or b"").decode()

    P = cvr.ProjectDesc
    later = dict(box_max=(0.5, -0.5, 0.5), step=9.0, lo=1.0, hi=1.0, colour=(-1, 1, 1))  # rules 4, 5, 6, 8 broken
    cases = [
        ("NULL argument", fdesc(res=(0, 1, 1)), None, rgba),                                                # 1
        ("NULL argument", None, P("max"), rgba),
        ("empty field", fdesc(res=(37, 0, 23), scalar_type=9), P(7, **later), 0),                           # 2
        ("more than 2^32 - 1", fdesc(res=(65536, 65536, 1), scalar_type=9, scalar=0), P(7, **later), 0),
        ("scalar_type", fdesc(scalar_type=4), P("max", **later), 0),                                        # 3
        ("unknown mode", fdesc(), P(4, **later), 0),
        ("unknown flags", fdesc(), P("max", flags=2, **later), 0),
        ("reserved", fdesc(reserved=1), P("max", **later), 0),
        ("box axis 1", fdesc(), P("max", **later), 0),                                                      # 4
        ("box axis 0", fdesc(), P("max", box_min=(nan, 0, 0), step=9.0), 0),
        ("step", fdesc(), P("max", step=9.0, lo=1.0, hi=1.0, colour=(-1, 1, 1)), 0),                        # 5
        ("step", fdesc(), P("iso", step=0.1, iso=nan), 0),
        ("max_steps", fdesc(), P("max", max_steps=0, lo=1.0, hi=1.0), 0),
        ("max_steps", fdesc(), P("max", max_steps=65537, lo=1.0, hi=1.0), 0),
        ("window", fdesc(), P("max", lo=1.0, hi=1.0, colour=(-1, 1, 1)), 0),                                # 6
        ("window", fdesc(), P("mean", lo=0.0, hi=inf, colour=(-1, 1, 1)), 0),
        ("window", fdesc(), P("min", lo=nan, hi=1.0), 0),
        ("iso", fdesc(), P("iso", iso=inf, refine=9, colour=(-1, 1, 1)), 0),                                # 7
        ("refine", fdesc(), P("iso", refine=9, ambient=-1.0, colour=(-1, 1, 1)), 0),
        ("ambient", fdesc(), P("iso", diffuse=nan, shininess_log2=11, colour=(-1, 1, 1)), 0),
        ("shininess_log2", fdesc(), P("iso", shininess_log2=11, light=(0, 0, 0), colour=(-1, 1, 1)), 0),
        ("light", fdesc(), P("iso", light=(0, 0, 0), colour=(-1, 1, 1)), 0),
        ("light", fdesc(), P("iso", light=(1e-30, 0, 0)), 0),
        ("colour", fdesc(), P("iso", colour=(1, 1, -0.5)), 0),                                              # 8
        ("colour", fdesc(), P("max", background=(0, inf, 0)), 0),
        ("scalar is NULL", fdesc(scalar=0), P("max"), rgba + 4),                                            # 9
        ("out_rgba is NULL", fdesc(scalar=a.ctypes.data + 1), P("max"), 0),
        ("scalar must be 2-byte aligned", fdesc(scalar=a.ctypes.data + 1), P("max"), rgba + 4),             # 10
        ("out_rgba must be 16-byte aligned", fdesc(), P("max"), rgba + 4),
    ]
    for what, f, d, ptr in cases:
        rc, msg = call(f, d, ptr)
        assert rc == INVALID and what in msg, (what, rc, msg)
    rc, msg = call(fdesc(), P("max"), rgba, camera_ok=False)
    assert rc == INVALID and "NULL argument" in msg
    # what a mode does not read is not judged
    assert call(fdesc(), P("max", iso=nan, refine=99, light=(0, 0, 0), ambient=-1.0, shininess_log2=99), rgba)[0] == 0
    assert call(fdesc(), P("iso", lo=nan, hi=nan), rgba)[0] == 0
    # the tile is judged between rules 8 and 9
    fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    assert lib.cvr_field_project_host(C.byref(fdesc(scalar=0)), C.byref(P("max")), fp(iv), fp(r2v), fp(fr), 0, 2, 0, 0, 0,
                                      None, None) == INVALID
    assert "tile" in lib.cvr_last_error(None).decode()
