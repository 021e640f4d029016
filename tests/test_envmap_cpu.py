"""Environment-map lighting, the parts that need no GPU: the C surface (CVR_HAS_ENVMAP within
ABI 6) and the host statement of the lookup, cvr_environment_eval_host.

The statement (include/cvr.h) is checked for its stated properties on maps of 2x2, 7x5 and 64x32
texels (a constant map returns exactly its constant for every direction, NaN and infinite ones
included; the seam reads columns W-1 and 0; the poles read rows 0 and H-1 alone) and against an
fp64 restatement with math.atan2 / acos within a bound derived in test_against_fp64's docstring.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from envmap_util import ROT, SIZES, random_dirs, special_dirs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cvr.h")


# ------------------------------------------------------------------ surface --
def test_header_declares_the_surface_within_abi_6(cvr):
    src = open(HEADER).read()
    assert re.search(r"^#define CVR_HAS_ENVMAP 1$", src, flags=re.M)
    inside = src[src.index("#if CVR_ABI_VERSION >= 6\n/* ---- adaptive"):src.index("#endif /* CVR_ABI_VERSION >= 6 */")]
    assert "#define CVR_HAS_ENVMAP 1" in inside
    assert cvr.load().cvr_abi_version() == 6


NAMES = ["cvr_set_environment", "cvr_clear_environment", "cvr_environment_info", "cvr_environment_eval_host",
         "cvr_environment_eval_host_fn", "cvr_environment_eval", "cvr_trace_env", "cvr_read_image", "cvr_free_image"]


def test_symbols_are_exported(cvr):
    nm = subprocess.check_output(["nm", "-D", "--defined-only", cvr.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (cvr_\w+)", nm))
    assert set(NAMES) <= exported, sorted(set(NAMES) - exported)


PROBE = r"""
#include <stdio.h>
#include "cvr.h"
int main(void) {
#ifdef CVR_HAS_ENVMAP
  printf("%d %zu %zu %zu\n", CVR_ABI_VERSION, sizeof(cvr_environment_desc), sizeof(struct cvr_environment_info),
         sizeof(cvr_env_record));
#else
  printf("%d none\n", CVR_ABI_VERSION);
#endif
  return 0;
}
"""


def _probe(tmp_path, *flags):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), *flags,
                           str(src), "-o", str(exe)])
    return subprocess.check_output([str(exe)], text=True).split()


def test_struct_sizes_equal_the_headers(cvr, tmp_path):
    from cudavolumerenderer_amd import _lib
    got = _probe(tmp_path)
    assert got == ["6", str(C.sizeof(_lib.EnvironmentDesc)), str(C.sizeof(_lib.EnvironmentInfo)),
                   str(C.sizeof(_lib.EnvRecord))]
    assert got[1:] == ["64", "24", "48"]


def test_abi_target_5_declares_nothing(tmp_path):
    assert _probe(tmp_path, "-DCVR_ABI_TARGET=5") == ["5", "none"]
    use = tmp_path / "use.c"
    use.write_text('#include "cvr.h"\nint f(cvr_ctx* c) { return cvr_clear_environment(c); }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Werror=implicit-function-declaration", "-DCVR_ABI_TARGET=5", "-I",
                        os.path.join(ROOT, "include"), "-c", str(use), "-o", str(tmp_path / "use.o")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "cvr_clear_environment" in r.stderr


# --------------------------------------------------------- the host statement --
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("rot", [None, ROT], ids=["identity", "rotated"])
def test_constant_map_returns_its_constant(cvr, size, rot):
    W, H = size
    const = np.array([0.3, 1.7, 123.456], np.float32)
    img = np.broadcast_to(const, (H, W, 3)).copy()
    dirs = np.concatenate([special_dirs(), random_dirs(2000)])
    out = cvr.environment_eval_host(img, dirs, rotation=rot)
    assert (out.view(np.uint32) == const.view(np.uint32)).all()
    # the scale is applied to the texel, once: fl(scale c)
    out = cvr.environment_eval_host(img, dirs, scale=0.37, rotation=rot)
    assert (out.view(np.uint32) == (np.float32(0.37) * const).view(np.uint32)).all()


def column_weights(cvr, W, H, d):
    """The weight every column has in direction d's lookup: maps whose column c alone is 1."""
    w = np.zeros(W, np.float32)
    for c in range(W):
        img = np.zeros((H, W, 3), np.float32)
        img[:, c] = 1.0
        w[c] = cvr.environment_eval_host(img, np.array([d], np.float32))[0, 0]
    return w


def row_weights(cvr, W, H, d):
    w = np.zeros(H, np.float32)
    for r in range(H):
        img = np.zeros((H, W, 3), np.float32)
        img[r] = 1.0
        w[r] = cvr.environment_eval_host(img, np.array([d], np.float32))[0, 0]
    return w


@pytest.mark.parametrize("size", SIZES)
def test_seam_reads_the_last_and_the_first_column(cvr, size):
    W, H = size
    for d in ((0.0, 0.0, 1.0), (-0.0, 0.0, 1.0)):
        w = column_weights(cvr, W, H, d)
        inner = np.delete(w, [0, W - 1]) if W > 2 else np.zeros(0)
        assert (inner == 0).all(), (d, w)
        assert w[0] > 0.25 and w[W - 1] > 0.25 and abs(float(w[0]) + float(w[W - 1]) - 1.0) <= 2.0 ** -22, (d, w)


@pytest.mark.parametrize("size", SIZES)
def test_poles_read_one_row_alone(cvr, size):
    W, H = size
    for x in (0.0, -0.0, 1e-30):
        top = row_weights(cvr, W, H, (x, 1.0, 0.0))
        bottom = row_weights(cvr, W, H, (x, -1.0, -0.0))
        assert top[0] == 1.0 and (top[1:] == 0).all(), top
        assert bottom[H - 1] == 1.0 and (bottom[:-1] == 0).all(), bottom


def test_centre_of_a_texel_returns_it(cvr):
    """u = (x + 0.5) / W, v = (y + 0.5) / H lands on texel (x, y): the -Z axis is the centre column
    of an odd width and +Y the top, the Mitsuba envmap convention."""
    W, H = 7, 5
    rng = np.random.default_rng(1)
    img = rng.random((H, W, 3), dtype=np.float32)
    out = cvr.environment_eval_host(img, np.array([[0.0, 0.0, -1.0]], np.float32))[0]
    np.testing.assert_allclose(out, img[2, 3], rtol=0, atol=2e-6)
    out = cvr.environment_eval_host(img, np.array([[1.0, 0.0, 0.0]], np.float32))[0]  # +X: u = 3/4
    x = 0.75 * W - 0.5
    fx = x - math.floor(x)
    want = (1 - fx) * img[2, int(x)].astype(np.float64) + fx * img[2, int(x) + 1]
    np.testing.assert_allclose(out, want, rtol=0, atol=2e-6)


def lookup_fp64(img, e):
    """The statement in fp64 from the rotated direction e (n, 3), with math.atan2 / acos."""
    H, W = img.shape[:2]
    im = img.astype(np.float64)
    out = np.zeros((len(e), 3))
    for i, (ex, ey, ez) in enumerate(e.astype(np.float64)):
        u = math.atan2(ex, -ez) / (2.0 * math.pi) + 0.5
        v = math.acos(min(max(ey, -1.0), 1.0)) / math.pi
        x, y = u * W - 0.5, v * H - 0.5
        x0, y0 = math.floor(x), math.floor(y)
        fx, fy = x - x0, y - y0
        xa, xb = (W - 1 if x0 < 0 else x0), (0 if x0 + 1 >= W else x0 + 1)
        ya, yb = (0 if y0 < 0 else y0), (H - 1 if y0 + 1 >= H else y0 + 1)
        t = im[ya, xa] + fx * (im[ya, xb] - im[ya, xa])
        b = im[yb, xa] + fx * (im[yb, xb] - im[yb, xa])
        out[i] = t + fy * (b - t)
    return out


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("rot", [None, ROT], ids=["identity", "rotated"])
def test_against_fp64(cvr, oracle_mod, size, rot):
    """|statement - fp64 lookup| <= (du W Gx + dv H Gy) + 8 * 2^-24 * M on random smooth maps, where

      e = R d is computed here in fp32 exactly as the statement does (multiply, multiply, add,
        multiply, add; numpy's float32 operations are the same IEEE ones), so both sides start
        from the same e;
      du = max |det_atan2f(e_x, -e_z) - atan2| / (2 pi) + 2 * 2^-24: the measured error of the
        angle (against fp64 on this test's own directions, through the oracle's det_atan2f, which
        is the same cvr_detmath.h definition), one rounding of the fused multiply-add into u
        (u <= 1: half an ulp is <= 2^-25) and one of x = fma(u, W, -0.5) relative to W (2^-24),
        rounded up; dv likewise from det_acosf and 1 / pi (the product's and y's roundings);
      each of du, dv is capped at 4 * 2^-24, four ulp of a coordinate in [0.5, 1): det_atan2f's
        documented 3 ulp at pi is 3 * 2^-22 / (2 pi) = 1.14e-7 and det_acosf's 2 ulp at pi is
        2 * 2^-22 / pi = 1.5e-7, both below the cap 2.38e-7 with the roundings added; a larger
        measured error fails the test before the bound is used;
      the bilinear interpolant is continuous, through the wrap of u and the clamp of v too, and
        changes by at most the largest adjacent-texel difference per texel step: Gx over
        horizontal neighbours (the wrap pair included), Gy over vertical ones, so a coordinate
        error of du W texels moves it by at most du W Gx;
      the interpolation itself is three fused multiply-adds and three subtractions on values
        <= M = the largest texel: 8 roundings of at most 2^-24 M bound it generously.
    """
    W, H = size
    rng = np.random.default_rng(W * 100 + H)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W, 3), np.float32)
    for c in range(3):  # smooth, periodic in x: two low-frequency waves and a little texture
        img[..., c] = (1.5 + np.sin(2 * np.pi * (xx + 0.5) / W + c) * np.cos(np.pi * (yy + 0.5) / H)
                       + 0.05 * rng.random((H, W))).astype(np.float32)
    d = random_dirs(4096, seed=W)
    R = np.eye(3, dtype=np.float32) if rot is None else rot
    f = np.float32
    e = np.stack([(f(R[k, 0]) * d[:, 0] + f(R[k, 1]) * d[:, 1]) + f(R[k, 2]) * d[:, 2] for k in range(3)], axis=1)
    assert e.dtype == np.float32
    got = cvr.environment_eval_host(img, d, rotation=rot).astype(np.float64)
    ref = lookup_fp64(img, e)

    ang = oracle_mod.detmath(5, -e[:, 2], e[:, 0]).astype(np.float64)  # det_atan2f(y = e_x, x = -e_z)
    ang_ref = np.array([math.atan2(a, -b) for a, b in zip(e[:, 0].astype(np.float64), e[:, 2].astype(np.float64))])
    ey = np.clip(e[:, 1], f(-1), f(1))
    ac = oracle_mod.detmath(4, ey).astype(np.float64)
    ac_ref = np.arccos(ey.astype(np.float64))
    du = np.abs(ang - ang_ref).max() / (2 * math.pi) + 2 * 2.0 ** -24
    dv = np.abs(ac - ac_ref).max() / math.pi + 2 * 2.0 ** -24
    cap = 4 * 2.0 ** -24
    assert du <= cap and dv <= cap, (du, dv)
    im = img.astype(np.float64)
    gx = np.abs(im - np.roll(im, 1, axis=1)).max()
    gy = np.abs(im[1:] - im[:-1]).max()
    bound = du * W * gx + dv * H * gy + 8 * 2.0 ** -24 * im.max()
    err = np.abs(got - ref).max()
    print(f"{W}x{H} {'rotated' if rot is not None else 'identity'}: du {du:.3e} dv {dv:.3e} "
          f"bound {bound:.3e} worst error {err:.3e}")
    assert err <= bound, (err, bound)


def test_callback_form_equals_the_array_form(cvr):
    W, H = 7, 5
    rng = np.random.default_rng(3)
    img = rng.random((H, W, 3), dtype=np.float32)
    dirs = np.concatenate([special_dirs()[::7], random_dirs(200)])
    a = cvr.environment_eval_host(img, dirs, rotation=ROT)
    b = cvr.environment_eval_host_fn(W, H, lambda x, y: img[y, x], dirs, rotation=ROT)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()


def test_bad_descriptors_are_invalid(cvr):
    ok = np.ones((4, 4, 3), np.float32)
    d = random_dirs(4)
    for img in (np.ones((1, 4, 3), np.float32), np.ones((4, 1, 3), np.float32), np.ones((4, 4, 2), np.float32),
                np.ones((4, 4, 5), np.float32), np.ones((2, 16385, 3), np.float32)):
        with pytest.raises(cvr.CvrError) as e:
            cvr.environment_eval_host(img, d)
        assert e.value.code == -1
    for scale in (-1.0, float("nan"), float("inf")):
        with pytest.raises(cvr.CvrError) as e:
            cvr.environment_eval_host(ok, d, scale=scale)
        assert e.value.code == -1
    with pytest.raises(cvr.CvrError) as e:
        cvr.environment_eval_host(ok, d, rotation=[1, 0, 0, 0, float("nan"), 0, 0, 0, 1])
    assert e.value.code == -1
