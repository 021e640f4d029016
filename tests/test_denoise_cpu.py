"""The variance-guided denoiser, the parts that need no GPU: its surface (CVR_HAS_DENOISE inside
ABI 6), and the host statement cvr_denoise_host against an independent numpy fp64 model of the
filter include/cvr.h writes out, on exact cases, edges, invalid pixels and an oracle render.

Model tolerance (test_host_matches_model): the host computes in fp32, the model in fp64, from
the same fp32 sums.  Largest deviation measured here over all cases (24x16 pixels, N = 2, 8,
20 and a two-count block map, passes 1..6): 4.39e-7 in colour (values up to 1.5) and 1.04e-8
in the variance (values up to 0.2), both at N = 2.  Asserted: 4x that, 1.76e-6 and 4.16e-8 (the
convention of tests/test_params_cpu.py).

It denoises (test_denoises_oracle_render): blob16, oblique camera, 64x64, regenerationSK, seed
7, 8 samples, against the fp64 mean of 2048 oracle samples: relMSE 0.09577 -> 0.01220, ratio
0.1274 (the fp64 model of the same sums: 0.1274); asserted <= 0.2."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import params
from parity_util import NTHREADS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
COLOUR_TOL, VAR_TOL = 1.76e-6, 4.16e-8

# ------------------------------------------------------------- the fp64 model --
K_LUMA = np.array([0.2126, 0.7152, 0.0722], np.float32).astype(np.float64)
G3 = (1 / 4, 1 / 2, 1 / 4)
H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def shift(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx], `fill` where that lies outside the image."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def pixel_counts(n, h, w):
    """(h, w) samples per pixel from a uniform count or a (h / 8, w / 8) block map."""
    n = np.asarray(n)
    return np.broadcast_to(n, (h, w)) if n.ndim == 0 else np.repeat(np.repeat(n, 8, axis=0), 8, axis=1)


def model_prepare(s1, s2, n):
    s1 = s1.astype(np.float64)[..., :3]
    s2 = s2.astype(np.float64)[..., :3]
    valid = (n >= 2) & np.isfinite(s1).all(-1) & np.isfinite(s2).all(-1)
    N = np.where(valid, n, 2).astype(np.float64)[..., None]
    with np.errstate(invalid="ignore", over="ignore"):
        m = s1 / N
        vc = np.maximum(s2 / N - m * m, 0.0) / (N - 1.0)
    v = (K_LUMA * K_LUMA * np.where(valid[..., None], vc, 0.0)).sum(-1)
    return np.where(valid[..., None], m, 0.0), np.where(valid, v, -1.0)


def model_pass(c, v, step, sigma, floor):
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
            ok = ~(vq < 0)
            hw = H5[j + 2] * H5[i + 2]
            with np.errstate(invalid="ignore", divide="ignore"):
                a = np.abs(cq @ K_LUMA - lum) / den
                u = 1.0 + a * a
                wt = np.where(ok, np.where(valid, hw / (u * u), hw), 0.0)
            cs += wt[..., None] * cq
            vs += wt * wt * np.where(ok, vq, 0.0)
            ws += wt
    has = ws > 0
    wsafe = np.where(has, ws, 1.0)
    return np.where(has[..., None], cs / wsafe[..., None], 0.0), np.where(has, vs / (wsafe * wsafe), -1.0)


def model_denoise(s1, s2, n, passes=5, sigma=4.0, floor=0.01):
    """The filter of include/cvr.h in fp64.  s1, s2: (h, w, 4) fp32 sums; n: a count or a block
    map -> (rgba (h, w, 4), var (h, w))."""
    s1, s2 = np.asarray(s1, np.float32), np.asarray(s2, np.float32)
    n = pixel_counts(n, *s1.shape[:2])
    c, v = model_prepare(s1, s2, n)
    for k in range(passes):
        c, v = model_pass(c, v, 1 << k, float(np.float32(sigma)), float(np.float32(floor)))
    with np.errstate(invalid="ignore"):
        a = np.where(n >= 2, s1[..., 3].astype(np.float64) / np.maximum(n, 1), 0.0)
    return np.concatenate([c, a[..., None]], -1), v


# ------------------------------------------------------------------ inputs --
def random_sums(h, w, n, seed):
    """fp32 sums of n samples per pixel (n: a count or a (h / 8, w / 8) block map) of T in
    [0, 1.5) with 20 % zeros, summed sample by sample as the kernel sums them; the w components
    hold the non-zero samples."""
    rng = np.random.default_rng(seed)
    cnt = pixel_counts(n, h, w)
    s1 = np.zeros((h, w, 4), np.float32)
    s2 = np.zeros((h, w, 4), np.float32)
    for k in range(int(cnt.max())):
        hit = (rng.random((h, w, 1)) < 0.8) & (k < cnt)[..., None]
        T = ((rng.random((h, w, 3), dtype=np.float32) * np.float32(1.5)) * hit).astype(np.float32)
        s1[..., :3] += T
        s2[..., :3] += T * T
        s1[..., 3] += hit[..., 0]
        s2[..., 3] += hit[..., 0]
    return s1, s2


def plant_invalid(s1, s2, counts):
    """A NaN in S1, an inf in S2 and a block with one sample.  -> (s1, s2, counts, planted (h, w) bool)."""
    s1, s2, counts = s1.copy(), s2.copy(), np.array(counts, np.uint32)
    h, w = s1.shape[:2]
    s1[3, 4, 1] = np.nan
    s2[h - 6, 2, 0] = np.inf
    counts[-1, -1] = 1
    planted = np.zeros((h, w), bool)
    planted[3, 4] = planted[h - 6, 2] = True
    planted[h - 8:, w - 8:] = True
    return s1, s2, counts, planted


def two_count_map(h, w, a=8, b=20):
    m = np.full((h // 8, w // 8), a, np.uint32)
    m[:, w // 16:] = b
    m[0, 0] = b
    return m


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------- surface --
def test_surface(cvr):
    lib = cvr.load()
    for name in ("cvr_denoise_host", "cvr_denoise_buffers", "cvr_denoise"):
        assert hasattr(lib, name), name
    assert C.sizeof(cvr.DenoiseDesc) == 16
    assert [f for f, _ in cvr.DenoiseDesc._fields_] == ["passes", "sigma", "floor", "flags"]
    d = cvr.DenoiseDesc()
    assert (d.passes, d.sigma, d.floor, d.flags) == (5, 4.0, np.float32(0.01), 0)
    hdr = open(os.path.join(ROOT, "include", "cvr.h")).read()
    assert "#define CVR_HAS_DENOISE 1" in hdr
    assert lib.cvr_abi_version() == 6  # an addition within ABI 6


def test_header_hides_denoise_from_abi5(tmp_path):
    def compiles(src, *flags):
        f = tmp_path / "t.c"
        f.write_text('#include "cvr.h"\n' + src)
        r = subprocess.run(["cc", "-std=c11", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            *flags, str(f)], capture_output=True, text=True, timeout=60)
        return r.returncode == 0, r.stderr

    use = ("#ifndef CVR_HAS_DENOISE\n#error \"no denoiser\"\n#endif\n"
           "int f(cvr_ctx* c, float* s) { cvr_denoise_desc d = {5, 4.0f, 0.01f, 0};\n"
           "  return cvr_denoise_host(s, s, 8, 8, 8, 0, &d, s, 0) + cvr_denoise_buffers(c, s, s, 8, 8, 8, 0, &d, s, 0)\n"
           "         + cvr_denoise(c, &d, 8, s, 256); }\n")
    assert compiles(use)[0]
    assert compiles(use, "-DCVR_ABI_TARGET=6")[0]
    ok, err = compiles("cvr_denoise_desc d;\n", "-DCVR_ABI_TARGET=5")
    assert not ok and "cvr_denoise_desc" in err
    ok, _ = compiles("#ifdef CVR_HAS_DENOISE\n#error \"declared\"\n#endif\n", "-DCVR_ABI_TARGET=5")
    assert ok


# ------------------------------------------------------- host == fp64 model --
MODEL_CASES = [(2, 11), (8, 12), (20, 13), ("map", 14)]


@pytest.mark.parametrize("n,seed", MODEL_CASES)
def test_host_matches_model(cvr, n, seed):
    h, w = 16, 24
    counts = two_count_map(h, w) if n == "map" else None
    s1, s2 = random_sums(h, w, counts if n == "map" else n, seed)
    worst_c = worst_v = 0.0
    for passes in range(1, 7):
        desc = cvr.DenoiseDesc(passes)
        if counts is None:
            rgba, var = cvr.denoise_host(s1, s2, n, desc=desc)
            ref, rvar = model_denoise(s1, s2, n, passes)
        else:
            rgba, var = cvr.denoise_host(s1, s2, block_samples=counts, desc=desc)
            ref, rvar = model_denoise(s1, s2, counts, passes)
        assert np.isfinite(rgba).all() and (var >= 0).all()
        worst_c = max(worst_c, float(np.abs(rgba - ref).max()))
        worst_v = max(worst_v, float(np.abs(var - rvar).max()))
    print(f"n={n}: largest deviation from the fp64 model: colour {worst_c:.3g}, variance {worst_v:.3g}")
    assert worst_c <= COLOUR_TOL and worst_v <= VAR_TOL


# ------------------------------------------------------------------- exact --
@pytest.mark.parametrize("side", [16, 8])
def test_constant_image_is_exact(cvr, side):
    """All weights are multiples of 1/256 and every sum is exact.  At 8x8 every pixel is within 2
    of a border in every pass, and steps >= 4 keep the centre tap only."""
    s1 = np.full((side, side, 4), 8 * 0.75, np.float32)
    s2 = np.full((side, side, 4), 8 * 0.5625, np.float32)
    for passes in range(1, 7):
        rgba, var = cvr.denoise_host(s1, s2, 8, desc=cvr.DenoiseDesc(passes))
        assert (rgba == np.float32(0.75)).all(), passes
        assert (bits(var) == 0).all(), passes  # +0.0
        ref, rvar = model_denoise(s1, s2, 8, passes)
        assert (ref == 0.75).all() and (rvar == 0).all()


def test_step_edge_is_kept(cvr):
    """Left half 0.25, right half 0.75, zero variance: den = floor = 0.01 and a = 0.5 / 0.01 = 50, so
    a tap across the edge weighs at most (55/9) / (1 + a^2)^2 ~ 1e-6 of the pixel's own side (all 25
    kernel weights over the smallest possible own-side sum, the centre's 9/64), moves the pixel by
    at most half the step height times that, ~5e-7, per pass and < 2.5e-6 in five."""
    h, w = 16, 32
    val = np.where(np.arange(w) < w // 2, np.float32(0.25), np.float32(0.75))
    img = np.broadcast_to(val[None, :, None], (h, w, 4)).astype(np.float32)
    s1, s2 = img * np.float32(8), img * img * np.float32(8)
    rgba, var = cvr.denoise_host(s1, s2, 8, desc=cvr.DenoiseDesc(5, 4.0, 0.01))
    assert np.abs(rgba - img).max() < 1e-5
    assert (var == 0).all()


# ---------------------------------------------------------- invalid pixels --
def test_invalid_pixels(cvr):
    h, w = 16, 24
    clean_counts = two_count_map(h, w)
    s1, s2 = random_sums(h, w, clean_counts, 21)
    b1, b2, counts, planted = plant_invalid(s1, s2, clean_counts)
    far = np.ones((h, w), bool)  # more than 2 away (in x or in y) from every planted pixel
    for y, x in zip(*np.nonzero(planted)):
        far[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = False
    assert far.sum() > 100
    # one pass reaches 2 pixels
    clean, cvar = cvr.denoise_host(s1, s2, block_samples=clean_counts, desc=cvr.DenoiseDesc(1))
    rgba, var = cvr.denoise_host(b1, b2, block_samples=counts, desc=cvr.DenoiseDesc(1))
    assert np.isfinite(rgba).all() and np.isfinite(var).all()
    assert (bits(rgba)[far] == bits(clean)[far]).all() and (bits(var)[far] == bits(cvar)[far]).all()
    assert not (bits(rgba) == bits(clean)).all()
    # the default filter: every planted pixel is in-painted
    rgba, var = cvr.denoise_host(b1, b2, block_samples=counts)
    assert np.isfinite(rgba).all() and np.isfinite(var).all()
    assert (var[planted] >= 0).all() and (rgba[planted][:, :3] > 0).all()
    assert (rgba[h - 8:, w - 8:, 3] == 0).all()  # the w channel of a block with N < 2
    ref, rvar = model_denoise(b1, b2, counts)
    assert np.abs(rgba - ref).max() <= COLOUR_TOL and np.abs(var - rvar).max() <= VAR_TOL
    # nothing valid anywhere
    allbad = s1.copy()
    allbad[..., :3] = np.nan
    rgba, var = cvr.denoise_host(allbad, s2, 8)
    assert (rgba[..., :3] == 0).all() and (var == -1).all()
    rgba, var = cvr.denoise_host(s1, s2, block_samples=np.ones_like(clean_counts))
    assert (rgba == 0).all() and (var == -1).all()


# ----------------------------------------------------------- it denoises ----
def test_denoises_oracle_render(cvr, oracle_mod):
    W = H = 64
    P = W * H
    case = params.Case({}, "oblique", 0, (W, H), (W, H), (0, 0))
    orc = params.make_oracle(oracle_mod, case)
    L = params.make_launch(oracle_mod, case, 2)

    def fp64_sums(a):  # samples [a, b) of every pixel, summed in fp64
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
    s1 = np.zeros((P, 4), np.float32)
    s2 = np.zeros((P, 4), np.float32)
    for s in range(n):  # sample by sample in fp32, as tests/test_gpu_adaptive.py's Sums
        r = recs[s * P:(s + 1) * P]
        esc = (r["flags"] & 1) != 0
        ids, T = r["image_id"][esc], r["T"][esc].astype(np.float32)
        assert len(np.unique(ids)) == len(ids)
        s1[ids, :3] += T
        s2[ids, :3] += T * T
        s2[ids, 3] += 1
    s1, s2 = s1.reshape(H, W, 4), s2.reshape(H, W, 4)

    def relmse(x):
        err = ((x[..., :3].astype(np.float64) - truth) ** 2).sum(-1)
        return float((err / (truth.mean(-1) ** 2 + 0.01)).mean())

    noisy = relmse(s1 / np.float32(n))
    rgba, _ = cvr.denoise_host(s1, s2, n)
    den = relmse(rgba)
    model = relmse(model_denoise(s1, s2, n)[0])
    print(f"relMSE noisy {noisy:.5f} denoised {den:.5f} ratio {den / noisy:.4f} (fp64 model {model / noisy:.4f})")
    assert den <= 0.2 * noisy


# --------------------------------------------------------------- refusals --
def test_refusals(cvr):
    lib = cvr.load()
    h, w = 8, 16
    s1, s2 = random_sums(h, w, 8, 31)
    out = np.zeros((h, w, 4), np.float32)
    var = np.zeros((h, w), np.float32)
    counts = np.full((1, 2), 8, np.uint32)

    def call(desc=None, sum_=s1, m2=s2, ww=w, hh=h, n=8, cnt=None, dst=out, dvar=var, null_desc=False):
        desc = cvr.DenoiseDesc() if desc is None else desc
        return lib.cvr_denoise_host(None if sum_ is None else sum_.ctypes.data, None if m2 is None else m2.ctypes.data,
                                    ww, hh, n, None if cnt is None else cnt.ctypes.data,
                                    None if null_desc else C.byref(desc), None if dst is None else dst.ctypes.data,
                                    None if dvar is None else dvar.ctypes.data)

    assert call() == 0 and call(dvar=None) == 0 and call(cnt=counts, n=0) == 0
    assert call(cvr.DenoiseDesc(5, 0.0)) == 0  # sigma 0 is allowed: den = floor
    for bad in (cvr.DenoiseDesc(0), cvr.DenoiseDesc(7), cvr.DenoiseDesc(5, 4.0, 0.0), cvr.DenoiseDesc(5, 4.0, -0.01),
                cvr.DenoiseDesc(5, 4.0, float("nan")), cvr.DenoiseDesc(5, 4.0, float("inf")), cvr.DenoiseDesc(5, -1.0),
                cvr.DenoiseDesc(5, float("nan")), cvr.DenoiseDesc(5, float("inf")), cvr.DenoiseDesc(5, 4.0, 0.01, 1)):
        assert call(bad) == INVALID, (bad.passes, bad.sigma, bad.floor, bad.flags)
    assert call(sum_=None) == INVALID and call(m2=None) == INVALID and call(dst=None) == INVALID
    assert call(null_desc=True) == INVALID
    assert call(n=1) == INVALID and call(n=0) == INVALID
    assert call(ww=0) == INVALID and call(hh=0) == INVALID
    # a map over sides that are not multiples of 8 (the buffers are large enough for 12x8 and 8x12)
    assert call(cnt=counts, ww=12, hh=8) == INVALID and call(cnt=counts, ww=8, hh=12) == INVALID
    assert call(ww=12, hh=8) == 0  # without a map any shape passes
    with pytest.raises(cvr.CvrError) as e:
        cvr.denoise_host(s1, s2, 1)
    assert e.value.code == INVALID and "2 samples" in str(e.value)
    with pytest.raises(cvr.CvrError) as e:
        cvr.denoise_host(s1, s2, 8, desc=cvr.DenoiseDesc(9))
    assert e.value.code == INVALID and "passes" in str(e.value)
