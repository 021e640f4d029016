"""The primary-ray feature pass and the feature-guided filter, the parts that need no GPU: the surface
(CVR_HAS_FEATURES inside ABI 6), the refusals, cvr_features_host against the independent numpy
restatement of tests/features_ref.py and against the unchanged oracle's density and box test, exact
cases, cvr_denoise_guided_host against an fp64 model and against cvr_denoise_host, and the experiment
that says the guide is worth having.

features_host == restatement: features_ref states every operation of include/cvr.h, the fused
multiply-adds of the trilinear included (an exact fp64 construction), so all five planes are compared
bit for bit.  (A restatement with plain products instead would differ per lerp by one rounding,
2^-24 relative, three levels deep: 3 * 2^-24 of the largest albedo per sample and as much in the
weighted mean; opacity and depth would stop being exact too.  Bit equality asks more than that bound.)

Guided filter against the fp64 model: the colour-only filter's tolerances (tests/test_denoise_cpu.py:
1.76e-6 colour, 4.16e-8 variance) plus what the guide adds.  The factor 1 / (g g) of a tap weight takes
at most 16 fp32 roundings (3 + 1 + 1 differences, 2 sums and 3 quotients for the terms; 3 squares, 2
sums, the + 1, g g, the quotient), a relative weight error d <= 16 * 2^-24 = 9.5e-7.  A pass's colour is
a ratio of weighted sums, so weights off by d move it by at most d times the colour range (1.5), its
variance (weights squared, values up to 0.2) by at most 2 d 0.2; over at most 6 passes: colour
1.76e-6 + 6 * 1.5 * 9.5e-7 = 1.03e-5, variance 4.16e-8 + 6 * 0.4 * 9.5e-7 = 2.33e-6.  Measured here
over all cases: colour 4.8e-7, variance 2.6e-8.

Does it denoise better (test_guided_beats_colour_only): 64x64, camera "oblique", regenerationSK, seed
7, 8 samples against the fp64 mean of 2048 oracle samples, relMSE as tests/test_denoise_cpu.py.  On the
two-hue blob (two albedos of equal fp32 luminance) colour-only 0.04314, guided (defaults 0.4, 0.1,
0.4) 0.02062; on blob16 colour-only 0.01220, guided 0.01089.  The grid the defaults came from:
profiles/features/README.md."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import features_ref
import params
from parity_util import NTHREADS
from test_denoise_cpu import (COLOUR_TOL, G3, H5, K_LUMA, VAR_TOL, model_prepare, pixel_counts, plant_invalid,
                              random_sums, shift, two_count_map)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
F = np.float32
UNIT = ((-0.5,) * 3, (0.5,) * 3)
GUIDED_COLOUR_TOL = COLOUR_TOL + 6 * 1.5 * 16 * 2.0 ** -24
GUIDED_VAR_TOL = VAR_TOL + 6 * 0.4 * 16 * 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def medium(cvr, density, albedo, box=UNIT, scale=params.SCALE):
    return cvr.medium_from_arrays(density, albedo, box[0], box[1], scale=scale, max_density=1.0)


def host(cvr, density, albedo, cam, full, tile=None, offset=(0, 0), box=UNIT, w2a=0, desc=None, scale=params.SCALE):
    m, keep = medium(cvr, density, albedo, box, scale)
    return cvr.features_host(m, cam.inv_view, cam.r2v, full, tile, offset, w2a, desc)


def ref(density, albedo, cam, full, tile=None, offset=(0, 0), box=UNIT, w2a=0, scale=params.SCALE, **kw):
    return features_ref.features(density, albedo, box[0], box[1], scale, cam.inv_view, cam.r2v, full, tile or full,
                                 offset, w2a, **kw)


# ----------------------------------------------------------------- surface --
def test_surface(cvr):
    lib = cvr.load()
    for name in ("cvr_features_host", "cvr_features_buffers", "cvr_features", "cvr_denoise_guided_host",
                 "cvr_denoise_guided_buffers", "cvr_denoise_guided"):
        assert hasattr(lib, name), name
    assert C.sizeof(cvr.FeaturesDesc) == 16 and C.sizeof(cvr.DenoiseGuidedDesc) == 32
    assert [f for f, _ in cvr.FeaturesDesc._fields_] == ["step", "t_stop", "max_steps", "flags"]
    assert [f for f, _ in cvr.DenoiseGuidedDesc._fields_] == ["base", "sigma_albedo", "sigma_depth", "sigma_alpha",
                                                              "flags"]
    d = cvr.FeaturesDesc()
    assert (d.step, d.t_stop, d.max_steps, d.flags) == (1.0, 1.0 / 256.0, 4096, 0)
    g = cvr.DenoiseGuidedDesc()
    assert (g.base.passes, g.base.sigma, g.base.floor, g.flags) == (5, 4.0, F(0.01), 0)
    assert (g.sigma_albedo, g.sigma_depth, g.sigma_alpha) == (F(0.4), F(0.1), F(0.4))
    for name in ("features", "features_buffers", "denoise_guided", "denoise_guided_buffers"):
        assert hasattr(cvr.Context, name), name
    assert hasattr(cvr.AdaptiveSession, "denoised_guided")
    hdr = open(os.path.join(ROOT, "include", "cvr.h")).read()
    assert "#define CVR_HAS_FEATURES 1" in hdr
    assert lib.cvr_abi_version() == 6  # an addition within ABI 6


def test_header_hides_features_from_abi5(tmp_path):
    def compiles(src, *flags):
        f = tmp_path / "t.c"
        f.write_text('#include "cvr.h"\n' + src)
        r = subprocess.run(["cc", "-std=c11", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            *flags, str(f)], capture_output=True, text=True, timeout=60)
        return r.returncode == 0, r.stderr

    use = ("#ifndef CVR_HAS_FEATURES\n#error \"no features\"\n#endif\n"
           "int f(cvr_ctx* c, const cvr_medium_desc* m, float* s) { cvr_features_desc d = {1.0f, 0.0f, 4096, 0};\n"
           "  cvr_denoise_guided_desc g = {{5, 4.0f, 0.01f, 0}, 0.4f, 0.1f, 0.4f, 0};\n"
           "  return cvr_features_host(m, s, s, s, 8, 8, 0, 0, 0, &d, s, s) + cvr_features_buffers(c, &d, s, s)\n"
           "         + cvr_features(c, &d, s, s, 256) + cvr_denoise_guided_host(s, s, 8, 8, 8, 0, &g, s, s, s, 0)\n"
           "         + cvr_denoise_guided_buffers(c, s, s, 8, 8, 8, 0, &g, s, s, s, 0)\n"
           "         + cvr_denoise_guided(c, &g, &d, 8, s, 256); }\n")
    assert compiles(use)[0]
    assert compiles(use, "-DCVR_ABI_TARGET=6")[0]
    for typ in ("cvr_features_desc", "cvr_denoise_guided_desc"):
        ok, err = compiles(typ + " d;\n", "-DCVR_ABI_TARGET=5")
        assert not ok and typ in err
    ok, _ = compiles("#ifdef CVR_HAS_FEATURES\n#error \"declared\"\n#endif\n", "-DCVR_ABI_TARGET=5")
    assert ok


# ---------------------------------------------------------------- refusals --
def test_features_refusals(cvr):
    lib = cvr.load()
    d, a = params.blob16()
    m, keep = medium(cvr, d, a)
    cam = params.camera("oblique", (8, 8))
    iv = np.ascontiguousarray(cam.inv_view, F)
    r2v = np.ascontiguousarray(cam.r2v, F)
    fr = np.array([8, 8], F)
    rgba, depth = np.zeros((8, 8, 4), F), np.zeros((8, 8), F)
    fp = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731

    def call(desc=None, med=m, iv_=iv, r_=r2v, fr_=fr, w=8, h=8, w2a=0, out=rgba, dep=depth, null_desc=False):
        desc = cvr.FeaturesDesc() if desc is None else desc
        return lib.cvr_features_host(None if med is None else C.byref(med), fp(iv_), fp(r_), fp(fr_), w, h, 0, 0, w2a,
                                     None if null_desc else C.byref(desc), None if out is None else out.ctypes.data,
                                     None if dep is None else dep.ctypes.data)

    assert call() == 0 and call(dep=None) == 0 and call(w2a=1) == 0
    for ok in (cvr.FeaturesDesc(0.125), cvr.FeaturesDesc(8.0), cvr.FeaturesDesc(1.0, 0.0), cvr.FeaturesDesc(1.0, 0.5, 1),
               cvr.FeaturesDesc(1.0, 0.5, 65536)):
        assert call(ok) == 0, (ok.step, ok.t_stop, ok.max_steps)
    nan, inf = float("nan"), float("inf")
    for bad in (cvr.FeaturesDesc(0.1249), cvr.FeaturesDesc(8.001), cvr.FeaturesDesc(0.0), cvr.FeaturesDesc(-1.0),
                cvr.FeaturesDesc(nan), cvr.FeaturesDesc(inf), cvr.FeaturesDesc(1.0, -0.001), cvr.FeaturesDesc(1.0, 1.0),
                cvr.FeaturesDesc(1.0, nan), cvr.FeaturesDesc(1.0, inf), cvr.FeaturesDesc(1.0, 0.5, 0),
                cvr.FeaturesDesc(1.0, 0.5, 65537), cvr.FeaturesDesc(1.0, 0.5, 4096, 1)):
        assert call(bad) == INVALID, (bad.step, bad.t_stop, bad.max_steps, bad.flags)
    assert call(med=None) == INVALID and call(iv_=None) == INVALID and call(r_=None) == INVALID
    assert call(fr_=None) == INVALID and call(out=None) == INVALID and call(null_desc=True) == INVALID
    assert call(w=0) == INVALID and call(h=0) == INVALID and call(w2a=2) == INVALID
    assert call(w=4097, h=4096) == INVALID  # more than 2^24 pixels (refused before anything is written)
    for field in ("density", "albedo"):
        m2, keep2 = medium(cvr, d, a)
        setattr(m2, field, None)
        assert call(med=m2) == INVALID
    m2, keep2 = medium(cvr, d, a)
    m2.res[1] = 0
    assert call(med=m2) == INVALID
    with pytest.raises(cvr.CvrError) as e:
        cvr.features_host(m, iv, r2v, (8, 8), desc=cvr.FeaturesDesc(9.0))
    assert e.value.code == INVALID and "step" in str(e.value)


def test_guided_refusals(cvr):
    lib = cvr.load()
    h, w = 8, 16
    s1, s2 = random_sums(h, w, 8, 31)
    f4, fz = np.zeros((h, w, 4), F), np.zeros((h, w), F)
    out, var = np.zeros((h, w, 4), F), np.zeros((h, w), F)
    counts = np.full((1, 2), 8, np.uint32)
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731

    def call(desc=None, sum_=s1, m2=s2, ww=w, hh=h, n=8, cnt=None, fr=f4, fd=fz, dst=out, dvar=var, null_desc=False):
        desc = cvr.DenoiseGuidedDesc() if desc is None else desc
        return lib.cvr_denoise_guided_host(p(sum_), p(m2), ww, hh, n, p(cnt), None if null_desc else C.byref(desc), p(fr),
                                           p(fd), p(dst), p(dvar))

    G, D = cvr.DenoiseGuidedDesc, cvr.DenoiseDesc
    assert call() == 0 and call(dvar=None) == 0 and call(cnt=counts, n=0) == 0
    assert call(G(None, 0.0, -1.0, 0.0)) == 0 and call(G(None, -float("inf"), 0.1, 0.1)) == 0
    nan, inf = float("nan"), float("inf")
    for bad in (G(D(0)), G(D(7)), G(D(5, 4.0, 0.0)), G(D(5, 4.0, nan)), G(D(5, -1.0)), G(D(5, inf)), G(D(5, 4.0, 0.01, 1)),
                G(None, nan), G(None, inf), G(None, 0.1, nan), G(None, 0.1, inf), G(None, 0.1, 0.1, nan),
                G(None, 0.1, 0.1, inf), G(None, 0.1, 0.1, 0.1, 1)):
        assert call(bad) == INVALID, (bad.base.passes, bad.sigma_albedo, bad.sigma_depth, bad.sigma_alpha, bad.flags)
    assert call(sum_=None) == INVALID and call(m2=None) == INVALID and call(dst=None) == INVALID
    assert call(fr=None) == INVALID and call(fd=None) == INVALID and call(null_desc=True) == INVALID
    assert call(n=1) == INVALID and call(ww=0) == INVALID and call(hh=0) == INVALID
    assert call(cnt=counts, ww=12, hh=8) == INVALID
    assert call(ww=4097, hh=4096) == INVALID
    with pytest.raises(cvr.CvrError) as e:
        cvr.denoise_guided_host(s1, s2, f4, fz[:4], 8)
    assert e.value.code == INVALID


# ------------------------------------------------- host == the restatement --
@pytest.mark.parametrize("camera", ["oblique", "inside"] + params.PENCILS)
def test_host_matches_restatement(cvr, camera):
    d, a = params.blob16()
    full = (32, 32)
    cam = params.camera(camera, full)
    rgba, depth = host(cvr, d, a, cam, full)
    r_rgba, r_depth = ref(d, a, cam, full)
    assert (bits(rgba[..., 3]) == bits(r_rgba[..., 3])).all() and (bits(depth) == bits(r_depth)).all()
    assert (bits(rgba[..., :3]) == bits(r_rgba[..., :3])).all()
    if camera in params.ALL_MISS:
        assert not rgba.any() and not depth.any()
    else:
        assert (rgba[..., 3] > 0.3).any() and (rgba[..., 3] <= 1).all() and (depth >= 0).all()
        assert ((rgba[..., 3] > 0) == (depth > 0)).all()


def test_tile_at_an_offset(cvr):
    d, a = params.blob16()
    cam = params.camera("oblique", (64, 48))
    whole = host(cvr, d, a, cam, (64, 48))
    part = host(cvr, d, a, cam, (64, 48), (13, 7), (8, 8))
    assert (bits(part[0]) == bits(whole[0][8:15, 8:21])).all() and (bits(part[1]) == bits(whole[1][8:15, 8:21])).all()
    assert part[0][..., 3].any()


@pytest.mark.parametrize("w2a", [0, 1])
def test_non_unit_box(cvr, w2a):
    d, a = params.blob16()
    box = (params._BOX_ALL["box_min"], params._BOX_ALL["box_max"])
    cam = params.camera("oblique", (32, 32))
    rgba, depth = host(cvr, d, a, cam, (32, 32), box=box, w2a=w2a)
    r_rgba, r_depth = ref(d, a, cam, (32, 32), box=box, w2a=w2a)
    assert (bits(rgba) == bits(r_rgba)).all() and (bits(depth) == bits(r_depth)).all()
    assert (rgba[..., 3] > 0.3).any()
    other = host(cvr, d, a, cam, (32, 32), box=box, w2a=1 - w2a)
    assert not (bits(rgba) == bits(other[0])).all()  # quirk Q4 is visible in this box


# ------------------------------------------------------- ties to the oracle --
def test_density_is_the_oracles(cvr, oracle_mod):
    """32 pixels whose every step takes its density from oracle.density_at (the unchanged oracle's
    interpolated density at the coordinate p - shift): the restatement still gives the host's bits."""
    d, a = params.blob16()
    full, tile, off = (64, 64), (8, 4), (28, 30)
    case = params.Case({}, "oblique", 0, full, tile, off)
    orc = params.make_oracle(oracle_mod, case)
    cam = params.camera("oblique", full)
    calls = []

    def density_at(c):
        calls.append(len(c))
        return np.array([orc.density_at(p) for p in c], F)

    rgba, depth = host(cvr, d, a, cam, full, tile, off)
    r_rgba, r_depth = ref(d, a, cam, full, tile, off, density_at=density_at)
    assert sum(calls) > 32 * 8 and (rgba[..., 3] > 0.5).all()
    assert (bits(rgba[..., 3]) == bits(r_rgba[..., 3])).all() and (bits(depth) == bits(r_depth)).all()
    assert (bits(rgba) == bits(r_rgba)).all()


@pytest.mark.parametrize("camera", ["oblique", "inside"] + params.PENCILS)
def test_no_chord_where_the_oracle_misses(cvr, oracle_mod, camera):
    d, a = params.blob16()
    full = (24, 24) if camera in ("oblique", "inside") else (3, 3)
    case = params.Case({}, camera, 0, full, full, (0, 0))
    orc = params.make_oracle(oracle_mod, case)
    cam = params.camera(camera, full)
    rgba, depth = host(cvr, d, a, cam, full)
    o, dirs = features_ref.rays(cam.inv_view, cam.r2v, full, full, (0, 0))
    hit = np.array([orc.aabb(o, dd)[0] for dd in dirs]).reshape(full[1], full[0])
    assert not rgba[~hit].any() and not depth[~hit].any()
    if camera in params.ALL_MISS:
        assert not hit.any()
    elif camera == "oblique":
        assert hit.any() and (~hit).any() and (rgba[..., 3] > 0).any()


# ------------------------------------------------------------- exact cases --
def test_homogeneous_medium(cvr):
    """Density 0.5 and albedo (0.5, 0.25, 1) everywhere: powers of two, for which the trilinear is
    exact (lerp(c, c) = fl(c (f + fl(1 - f))), and f + fl(1 - f) lies within 2^-25 of 1, which rounds
    back to c).  So every step has s = (scale 0.5) delta and W is 1 - (1 + s)^-n, evaluated by the
    pass's own fp32 recurrence, bit for bit; the albedo is the constant (asserted: within 2 ulp)."""
    d = np.full((16, 16, 16), 0.5, F)
    a = np.ones((16, 16, 16, 4), F)
    a[..., :3] = (0.5, 0.25, 1.0)
    full = (32, 32)
    cam = params.camera("oblique", full)
    desc = cvr.FeaturesDesc(1.0, 0.0)
    rgba, depth = host(cvr, d, a, cam, full, desc=desc)
    o, dirs = features_ref.rays(cam.inv_view, cam.r2v, full, full, (0, 0))
    has, t0, t1 = features_ref.chord(o, dirs, np.array(UNIT[0], F), np.array(UNIT[1], F))
    delta = F(1.0) / F(16)
    with np.errstate(invalid="ignore"):
        n = np.where(has, np.ceil((t1 - t0) / delta), 0).astype(int)
    n = np.array([sum(1 for i in range(k) if t0[j] + (F(i) + F(0.5)) * delta < t1[j]) for j, k in enumerate(n)])
    s = (F(params.SCALE) * F(0.5)) * delta
    W = {0: F(0)}
    T, acc = F(1), F(0)
    for k in range(1, int(n.max()) + 1):
        w = T * (s / (F(1) + s))
        acc, T = acc + w, T - w
        W[k] = acc
    expect = np.array([W[k] for k in n], F).reshape(32, 32)
    assert n.max() >= 16 and (n == 0).any()
    assert (bits(rgba[..., 3]) == bits(expect)).all()
    lit = rgba[..., 3] > 0
    for c, v in enumerate((0.5, 0.25, 1.0)):
        ulp = np.spacing(F(v))
        assert (np.abs(rgba[..., c][lit] - F(v)) <= 2 * ulp).all()
    assert not rgba[~lit].any() and not depth[~lit].any()


def test_zero_medium(cvr):
    d, a = params.blob16()
    rgba, depth = host(cvr, np.zeros_like(d), a, params.camera("oblique", (16, 16)), (16, 16))
    assert (bits(rgba) == 0).all() and (bits(depth) == 0).all()


def test_early_stop_changes_opacity_by_less_than_t_stop(cvr):
    d, a = params.blob16()
    cam = params.camera("oblique", (32, 32))
    full_march = host(cvr, d, a, cam, (32, 32), desc=cvr.FeaturesDesc(1.0, 0.0))[0][..., 3]
    stopped = host(cvr, d, a, cam, (32, 32), desc=cvr.FeaturesDesc(1.0, 1.0 / 256.0))[0][..., 3]
    diff = full_march.astype(np.float64) - stopped
    assert (diff >= 0).all() and (diff < 1.0 / 256.0).all() and (diff > 0).any()


def test_max_steps_caps_the_march(cvr):
    d, a = params.blob16()
    cam = params.camera("oblique", (32, 32))
    capped = host(cvr, d, a, cam, (32, 32), desc=cvr.FeaturesDesc(0.125, 0.0, 16))
    free = host(cvr, d, a, cam, (32, 32), desc=cvr.FeaturesDesc(0.125, 0.0, 4096))
    r_rgba, r_depth = ref(d, a, cam, (32, 32), step=0.125, t_stop=0.0, max_steps=16)
    assert (bits(capped[0]) == bits(r_rgba)).all() and (bits(capped[1]) == bits(r_depth)).all()
    # 16 steps of 1/8 cell cover 2 of the chord's up to ~28 cells: the capped march is a prefix of
    # the free one (t_stop 0), so it never has more opacity, and less wherever the ray goes on
    # into the blob
    cw, fw = capped[0][..., 3], free[0][..., 3]
    lit = fw > 0.5
    assert (cw <= fw).all() and lit.any() and (cw[lit] < fw[lit]).all()


# ------------------------------------------------------ the guided filter ---
def model_pass_guided(c, v, step, sigma, floor, f4, fz, sig):
    """test_denoise_cpu.model_pass with the guide's factor 1 / (g g) on a valid centre's weights, fp64."""
    valid = ~(v < 0)
    lum = c @ K_LUMA
    gs, gw = np.zeros_like(v), np.zeros_like(v)
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            vq = shift(v, j, i, -1.0)
            ok = ~(vq < 0)
            gs += np.where(ok, G3[j + 1] * G3[i + 1] * vq, 0.0)
            gw += np.where(ok, G3[j + 1] * G3[i + 1], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = sigma * np.sqrt(gs / gw) + floor
    cs, vs, ws = np.zeros_like(c), np.zeros_like(v), np.zeros_like(v)
    for j in range(-2, 3):
        for i in range(-2, 3):
            vq = shift(v, j * step, i * step, -1.0)
            cq = shift(c, j * step, i * step, 0.0)
            fq = shift(f4, j * step, i * step, 0.0)
            zq = shift(fz, j * step, i * step, 0.0)
            ok = ~(vq < 0)
            hw = H5[j + 2] * H5[i + 2]
            fa = np.abs(fq[..., :3] - f4[..., :3]).sum(-1) / sig[0] if sig[0] > 0 else 0.0
            fd = np.abs(zq - fz) / sig[1] if sig[1] > 0 else 0.0
            fo = np.abs(fq[..., 3] - f4[..., 3]) / sig[2] if sig[2] > 0 else 0.0
            g = 1.0 + fa * fa + fd * fd + fo * fo
            with np.errstate(invalid="ignore", divide="ignore"):
                a = np.abs(cq @ K_LUMA - lum) / den
                u = 1.0 + a * a
                wt = np.where(ok, np.where(valid, hw / (u * u) / (g * g), hw), 0.0)
            cs += wt[..., None] * cq
            vs += wt * wt * np.where(ok, vq, 0.0)
            ws += wt
    has = ws > 0
    wsafe = np.where(has, ws, 1.0)
    return np.where(has[..., None], cs / wsafe[..., None], 0.0), np.where(has, vs / (wsafe * wsafe), -1.0)


def model_guided(s1, s2, n, f4, fz, desc):
    s1, s2 = np.asarray(s1, F), np.asarray(s2, F)
    n = pixel_counts(n, *s1.shape[:2])
    c, v = model_prepare(s1, s2, n)
    sig = [float(F(x)) for x in (desc.sigma_albedo, desc.sigma_depth, desc.sigma_alpha)]
    for k in range(desc.base.passes):
        c, v = model_pass_guided(c, v, 1 << k, float(F(desc.base.sigma)), float(F(desc.base.floor)),
                                 f4.astype(np.float64), fz.astype(np.float64), sig)
    with np.errstate(invalid="ignore"):
        a = np.where(n >= 2, s1[..., 3].astype(np.float64) / np.maximum(n, 1), 0.0)
    return np.concatenate([c, a[..., None]], -1), v


def feature_planes(h, w, seed):
    """Planes with a vertical and a horizontal edge and smooth parts: (h, w, 4) in [0, 1], (h, w)."""
    rng = np.random.default_rng(seed)
    f4 = rng.random((h, w, 4), dtype=F) * F(0.05)
    f4[:, w // 2:, :3] += F(0.6)
    f4[h // 2:, :, 3] += F(0.5)
    fz = (np.linspace(0, 1, w, dtype=F)[None, :] * np.ones((h, 1), F)).astype(F)
    return f4, fz


@pytest.mark.parametrize("n,seed", [(2, 11), (8, 12), (20, 13), ("map", 14)])
def test_guided_host_matches_model(cvr, n, seed):
    h, w = 16, 24
    counts = two_count_map(h, w) if n == "map" else None
    s1, s2 = random_sums(h, w, counts if n == "map" else n, seed)
    f4, fz = feature_planes(h, w, seed)
    worst_c = worst_v = 0.0
    for passes in range(1, 7):
        for sig in ((0.4, 0.1, 0.4), (0.1, 0.0, 0.05), (0.0, 0.05, -1.0)):
            desc = cvr.DenoiseGuidedDesc(cvr.DenoiseDesc(passes), *sig)
            kw = dict(block_samples=counts) if counts is not None else dict(n_samples=n)
            rgba, var = cvr.denoise_guided_host(s1, s2, f4, fz, desc=desc, **kw)
            m_rgba, m_var = model_guided(s1, s2, counts if counts is not None else n, f4, fz, desc)
            assert np.isfinite(rgba).all() and (var >= 0).all()
            worst_c = max(worst_c, float(np.abs(rgba - m_rgba).max()))
            worst_v = max(worst_v, float(np.abs(var - m_var).max()))
    print(f"n={n}: largest deviation from the fp64 model: colour {worst_c:.3g}, variance {worst_v:.3g}")
    assert worst_c <= GUIDED_COLOUR_TOL and worst_v <= GUIDED_VAR_TOL
    # the guide does something: the default sigmas change the result of the colour-only filter
    plain, _ = cvr.denoise_host(s1, s2, None if counts is not None else n, counts)
    guided, _ = cvr.denoise_guided_host(s1, s2, f4, fz, None if counts is not None else n, counts)
    assert np.abs(plain - guided).max() > 1e-3


def test_guide_off_is_the_colour_only_filter(cvr):
    h, w = 16, 24
    counts = two_count_map(h, w)
    s1, s2 = random_sums(h, w, counts, 21)
    b1, b2, bad_counts, planted = plant_invalid(s1, s2, counts)
    f4, fz = feature_planes(h, w, 5)
    for passes in range(1, 7):
        base = cvr.DenoiseDesc(passes)
        for sig in ((0.0, 0.0, 0.0), (-1.0, 0.0, -0.5)):
            off = cvr.DenoiseGuidedDesc(base, *sig)
            for args in ((s1, s2, 8, None), (s1, s2, None, counts), (b1, b2, None, bad_counts), (b1, b2, 8, None)):
                want = cvr.denoise_host(*args, desc=base)
                got = cvr.denoise_guided_host(args[0], args[1], f4, fz, args[2], args[3], desc=off)
                assert (bits(got[0]) == bits(want[0])).all() and (bits(got[1]) == bits(want[1])).all(), passes


def test_guided_constant_image_is_exact(cvr):
    """A constant 0.5 (a power of two: every weighted sum is 0.5 times the sum of the weights, exactly)
    stays 0.5 under any feature planes, and its variance +0."""
    side = 16
    s1 = np.full((side, side, 4), 8 * 0.5, F)
    s2 = np.full((side, side, 4), 8 * 0.25, F)
    rng = np.random.default_rng(3)
    f4, fz = rng.random((side, side, 4), dtype=F), rng.random((side, side), dtype=F)
    for passes in range(1, 7):
        rgba, var = cvr.denoise_guided_host(s1, s2, f4, fz, 8, desc=cvr.DenoiseGuidedDesc(cvr.DenoiseDesc(passes)))
        assert (rgba == F(0.5)).all() and (bits(var) == 0).all(), passes


# ------------------------------------------------- does it denoise better ---
def equal_luma_green():
    """g2 with luma(0.2, g2, 0.2) == luma(0.9, 0.2, 0.2) in fp32 (about 0.408): the nearest such float."""
    luma = lambda r, g, b: (F(0.2126) * F(r) + F(0.7152) * F(g)) + F(0.0722) * F(b)  # noqa: E731
    target = luma(0.9, 0.2, 0.2)
    c = np.arange(-4096, 4097)
    cand = (F(0.408).view(np.uint32) + c).astype(np.uint32).view(F)
    ok = cand[np.array([luma(0.2, g, 0.2) == target for g in cand])]
    assert ok.size
    return ok[np.argmin(np.abs(ok - F(0.408)))]


def two_hue_blob():
    d, a = params.blob16()
    a = np.ones_like(a)
    a[:, :, :8, :3] = (0.9, 0.2, 0.2)
    a[:, :, 8:, :3] = (0.2, equal_luma_green(), 0.2)
    return d, a.astype(F)


def denoise_experiment(cvr, oracle_mod, density, albedo):
    """-> relMSE of (the 8-sample mean, cvr_denoise_host, cvr_denoise_guided_host with the defaults)."""
    W = H = 64
    P = W * H
    case = params.Case({}, "oblique", 0, (W, H), (W, H), (0, 0))
    orc = params.make_oracle(oracle_mod, case, density, albedo)
    L = params.make_launch(oracle_mod, case, 2)

    def fp64_sums(a):
        r = orc.trace_paths(L, a[0] * P, (a[1] - a[0]) * P)
        esc = (r["flags"] & 1) != 0
        ids, T = r["image_id"][esc], r["T"][esc].astype(np.float64)
        return np.stack([np.bincount(ids, T[:, c], P) for c in range(3)], -1)

    NS, per = 2048, 2048 // 16
    with ThreadPoolExecutor(NTHREADS) as ex:
        truth = sum(ex.map(fp64_sums, [(s, s + per) for s in range(0, NS, per)])) / NS
    truth = truth.reshape(H, W, 3)
    n = 8
    recs = orc.trace_paths(L, 0, n * P)
    s1, s2 = np.zeros((P, 4), F), np.zeros((P, 4), F)
    for s in range(n):
        r = recs[s * P:(s + 1) * P]
        esc = (r["flags"] & 1) != 0
        ids, T = r["image_id"][esc], r["T"][esc].astype(F)
        s1[ids, :3] += T
        s2[ids, :3] += T * T
        s2[ids, 3] += 1
    s1, s2 = s1.reshape(H, W, 4), s2.reshape(H, W, 4)

    def relmse(x):
        err = ((x[..., :3].astype(np.float64) - truth) ** 2).sum(-1)
        return float((err / (truth.mean(-1) ** 2 + 0.01)).mean())

    cam = params.camera("oblique", (W, H))
    f4, fz = host(cvr, density, albedo, cam, (W, H))
    return (relmse(s1 / F(n)), relmse(cvr.denoise_host(s1, s2, n)[0]),
            relmse(cvr.denoise_guided_host(s1, s2, f4, fz, n)[0]))


def test_guided_beats_colour_only(cvr, oracle_mod):
    d, a = two_hue_blob()
    lum = (F(0.2126) * a[..., 0] + F(0.7152) * a[..., 1]) + F(0.0722) * a[..., 2]
    assert (bits(lum) == bits(lum)[0, 0, 0]).all()  # one luminance, two hues
    noisy, plain, guided = denoise_experiment(cvr, oracle_mod, d, a)
    print(f"two-hue blob: relMSE noisy {noisy:.5f} colour-only {plain:.5f} guided {guided:.5f}")
    assert guided < plain
    noisy, plain, guided = denoise_experiment(cvr, oracle_mod, *params.blob16())
    print(f"blob16: relMSE noisy {noisy:.5f} colour-only {plain:.5f} guided {guided:.5f}")
