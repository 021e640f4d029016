"""Adaptive sampling, the parts that need no GPU: ABI 6 and its constants, and the noise
metric cvr_block_error against a numpy fp64 model of its definition (include/cvr.h).

Metric tolerance: |delta| <= 1e-6 absolute + 1e-9 relative.  With identical fp32 inputs the
two sides differ by fp64 rounding (and, on the device, fused multiply-adds) only, which
perturbs v_c by a few 2^-53 m^2; the sqrt turns that into at most about 1e-7 m / (sum m +
floor) <= 1e-7, and 1e-6 is that with a factor of ten.  Reordering the 64-term mean adds
<= 63 * 2^-53 relative."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL, RTOL = 1e-6, 1e-9


def model_pixel_error(s1, s2, n, floor):
    """e_pixel of include/cvr.h in numpy fp64: (..., 4) fp32 sums -> (...) errors."""
    s1 = np.asarray(s1, np.float32).astype(np.float64)[..., :3]
    s2 = np.asarray(s2, np.float32).astype(np.float64)[..., :3]
    N = np.float64(n)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = s1 / N
        v = np.maximum(0.0, s2 / N - m * m) / (N - 1.0)
        e = np.sqrt(v.sum(axis=-1)) / (m.sum(axis=-1) + np.float64(np.float32(floor)))
    bad = np.isnan(s1).any(axis=-1) | np.isnan(s2).any(axis=-1)
    return np.where(bad, np.inf, e)


def model_block_error(s1, s2, n, floor):
    return float(model_pixel_error(s1, s2, n, floor).mean())


def close(a, b):
    if np.isinf(a) or np.isinf(b):
        return a == b
    return abs(a - b) <= ATOL + RTOL * abs(b)


def test_abi_and_constants(cvr):
    lib = cvr.load()
    assert lib.cvr_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "cvr.h")).read()
    assert re.search(r"#define CVR_ABI_VERSION 6\b", hdr)
    assert re.search(r"CVR_OPT_MOMENTS\s*=\s*31\b", hdr) and cvr.OPT_MOMENTS == 31
    assert "6: CVR_OPT_MOMENTS, cvr_copy_moments, cvr_block_error, cvr_adaptive_*" in hdr
    # the structs as the header lays them out: 3 u32 + 2 float; 3 u32 (+ pad), u64, 2 double, i32 (+ pad)
    assert C.sizeof(cvr.AdaptiveDesc) == 20
    assert C.sizeof(cvr.AdaptiveResult) == 48
    body = re.search(r"typedef struct cvr_adaptive_desc \{(.*?)\} cvr_adaptive_desc;", hdr, re.S).group(1)
    assert [f for f, _ in cvr.AdaptiveDesc._fields_] == re.findall(r"^\s*(?:uint32_t|float) (\w+);", body, re.M)
    assert cvr.AdaptiveResult.paths.offset == 16 and cvr.AdaptiveResult.max_error.offset == 24
    assert cvr.AdaptiveResult.done.offset == 40
    for name in ("cvr_copy_moments", "cvr_block_error", "cvr_adaptive_begin", "cvr_adaptive_pass",
                 "cvr_adaptive_maps", "cvr_adaptive_image", "cvr_adaptive_end", "cvr_render_adaptive"):
        assert hasattr(lib, name), name
    d = cvr.AdaptiveDesc(8, 32, 4, 0.1, 0.01)
    assert (d.min_iterations, d.max_iterations, d.pass_iterations) == (8, 32, 4)
    assert d.target == np.float32(0.1) and d.floor == np.float32(0.01)


def test_header_abi_target(tmp_path):
    """CVR_ABI_TARGET 5 holds a host to the ABI 5 surface: the ABI 6 declarations are left out
    (a use fails to compile) and CVR_ABI_VERSION is 5; by default the header declares ABI 6."""
    import subprocess

    def compiles(src, *flags):
        f = tmp_path / "t.c"
        f.write_text('#include "cvr.h"\n' + src)
        r = subprocess.run(["cc", "-std=c11", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            *flags, str(f)], capture_output=True, text=True, timeout=60)
        return r.returncode == 0, r.stderr

    use6 = ("int f(cvr_ctx* c, float* s) { cvr_adaptive_desc d = {8, 32, 4, 0.1f, 0.01f}; cvr_adaptive_result r;\n"
            "  return cvr_copy_moments(c, s, s) + cvr_render_adaptive(c, &d, s, 4, &r, 0); }\n")
    use5 = "int g(const float* a, float* b) { return cvr_half_round(a, b, 1) + CVR_OPT_MEDIUM_FORMAT; }\n"
    is_v = "_Static_assert(CVR_ABI_VERSION == %d, \"version\");\n"
    assert compiles(is_v % 6 + use5 + use6)[0]
    assert compiles(is_v % 6 + use5 + use6, "-DCVR_ABI_TARGET=6")[0]
    assert compiles(is_v % 5 + use5, "-DCVR_ABI_TARGET=5")[0]
    ok, err = compiles(use6, "-DCVR_ABI_TARGET=5")
    assert not ok and "cvr_adaptive_desc" in err
    ok, err = compiles(use5, "-DCVR_ABI_TARGET=4")
    assert not ok and "CVR_ABI_TARGET must be 5 or 6" in err


@pytest.mark.parametrize("n", [2, 8, 20, 32])
@pytest.mark.parametrize("floor", [0.01, 0.0, 1.0])
def test_block_error_random_sums(cvr, n, floor):
    rng = np.random.default_rng(1000 * n + int(100 * floor))
    # n samples of T in [0, 1.5) per pixel and channel, summed as the kernel sums them (fp32)
    T = (rng.random((n, 64, 4), dtype=np.float32) * np.float32(1.5)) * (rng.random((n, 64, 1)) < 0.8)
    T = T.astype(np.float32)
    T[:, 5] = 0  # a black pixel
    s1 = np.zeros((64, 4), np.float32)
    s2 = np.zeros((64, 4), np.float32)
    for k in range(n):
        s1 += T[k]
        s2 += T[k] * T[k]
    got = cvr.block_error(s1, s2, n, floor)
    ref = model_block_error(s1, s2, n, floor) if floor > 0 else None
    if floor == 0.0:  # a black pixel with floor 0: the zero denominator counts as error 0
        e = model_pixel_error(s1, s2, n, floor)
        black = (s1[:, :3] == 0).all(axis=1)
        assert black[5] and np.isnan(e[black]).all()
        e[black] = 0.0
        ref = float(e.mean())
    assert np.isfinite(got) and got > 0
    assert close(got, ref), (got, ref)
    # one pixel at a time: the per-pixel term itself
    ep = model_pixel_error(s1, s2, n, 0.01)
    for i in (0, 17, 63):
        assert close(cvr.block_error(s1[i:i + 1], s2[i:i + 1], n, 0.01), float(ep[i]))


def test_block_error_equal_samples_is_exactly_zero(cvr):
    # values whose squares are exact in fp32 (multiples of 1/64 below 2): S2 / N == m^2 exactly
    rng = np.random.default_rng(5)
    t = (rng.integers(0, 128, (64, 4)) / 64.0).astype(np.float32)
    for n in (2, 8, 32):
        s1 = np.zeros_like(t)
        s2 = np.zeros_like(t)
        for _ in range(n):
            s1 += t
            s2 += t * t
        assert cvr.block_error(s1, s2, n, 0.01) == 0.0
        assert model_block_error(s1, s2, n, 0.01) == 0.0


def test_block_error_nan_pixel_is_inf(cvr):
    rng = np.random.default_rng(6)
    s1 = rng.random((64, 4), dtype=np.float32) * 8
    s2 = rng.random((64, 4), dtype=np.float32) * 8
    assert np.isfinite(cvr.block_error(s1, s2, 8, 0.01))
    for arr, ch in ((s1, 0), (s1, 2), (s2, 1)):
        a, b = s1.copy(), s2.copy()
        (a if arr is s1 else b)[40, ch] = np.nan
        assert cvr.block_error(a, b, 8, 0.01) == np.inf
        assert model_block_error(a, b, 8, 0.01) == np.inf
    # the unused w components do not enter
    a = s1.copy()
    a[3, 3] = np.nan
    assert close(cvr.block_error(a, s2, 8, 0.01), model_block_error(s1, s2, 8, 0.01))


def test_block_error_arguments(cvr):
    lib = cvr.load()
    s = np.ones((64, 4), np.float32)
    out = C.c_double(-1.0)
    fp = s.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.cvr_block_error(fp, fp, 64, 1, 0.01, C.byref(out)) == -1  # CVR_ERR_INVALID
    assert lib.cvr_block_error(fp, fp, 64, 0, 0.01, C.byref(out)) == -1
    assert lib.cvr_block_error(None, fp, 64, 8, 0.01, C.byref(out)) == -1
    assert lib.cvr_block_error(fp, fp, 64, 8, 0.01, None) == -1
    assert out.value == -1.0
    with pytest.raises(cvr.CvrError) as e:
        cvr.block_error(s, s, 1, 0.01)
    assert e.value.code == -1 and "2 samples" in str(e.value)
    assert lib.cvr_block_error(fp, fp, 64, 2, 0.01, C.byref(out)) == 0


def test_cli_lists_noise_target():
    import subprocess
    cli = os.path.join(ROOT, "cudavolumerenderer_amd", "cvr")
    out = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    ext = out[out.index("Extensions:"):]
    assert "--noise-target F" in ext and "--min-iterations N (=8)" in ext and "--pass-iterations N (=4)" in ext
    r = subprocess.run([cli, "--interactive", "0", "--synthetic", "bucky", "-r", "64", "-i", "32", "--noise-target",
                        "0.1", "--number-of-tiles", "2", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--noise-target renders one tile on one device" in r.stderr
