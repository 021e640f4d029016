"""cvr_half_round (host only): the rounding of the half medium format
(CVR_OPT_MEDIUM_FORMAT 1) is IEEE binary16 round-to-nearest-even with
subnormals kept, bit for bit numpy's float32 -> float16 -> float32, so that a
caller (and tests/test_gpu_half_medium.py) can build the fp32 medium a
half-format render is bit-identical to.  Also the new public surface: option
number, ABI version, exported symbols, the CLI switch."""
import ctypes as C
import os
import re
import subprocess
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cudavolumerenderer_amd", "cvr")


def _numpy_round(x):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # 65520 -> inf is the point
        return x.astype(np.float16).astype(np.float32)


def _assert_same(cvr, x, what):
    x = np.asarray(x, np.float32)
    got, exp = cvr.half_round(x), _numpy_round(x)
    assert got.dtype == np.float32 and got.shape == x.shape
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)) & ~nan)[0]
    assert bad.size == 0, f"{what}: {bad.size} differ, first x={x[bad[0]]!r} got {got[bad[0]]!r} want {exp[bad[0]]!r}"


def test_special_values(cvr):
    vals = [0.0, -0.0,
            2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 1e-6, 6e-8, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25,  # subnormals
            2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24,  # ties and just above
            2.0 ** -26, 1e-8, -1e-8, 1e-30,  # below 2^-25: zero
            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 0.5 + 2.0 ** -12,  # ties
            0.9, 0.3, -0.7, 1.0, 2047.5, 2048.5,
            65504.0, 65519.99, 65520.0, -65519.99, -65520.0, 70000.0, 1e30,
            np.inf, -np.inf, np.nan]
    _assert_same(cvr, vals, "special values")
    r = cvr.half_round(np.array(vals, np.float32))
    x = np.array(vals, np.float32)
    assert r[x == np.float32(65519.99)][0] == 65504.0 and np.isinf(r[x == 65520.0][0])
    assert r[x == np.float32(1e-8)][0] == 0.0 and r[x == np.float32(1e-6)][0] != 0.0
    assert r[x == np.float32(1 + 2.0 ** -11)][0] == 1.0  # tie to even: down
    assert r[x == np.float32(1 + 3 * 2.0 ** -11)][0] == np.float32(1 + 2.0 ** -9)  # tie to even: up
    assert np.signbit(r[1]) and r[1] == 0.0


def test_random_unit_interval(cvr):
    rng = np.random.default_rng(20240607)
    _assert_same(cvr, rng.random(100000, dtype=np.float32), "random [0, 1]")


def test_every_half_and_every_tie(cvr):
    """Every finite half is a fixed point; every midpoint between neighbours goes to the even one."""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
    assert np.array_equal(cvr.half_round(h).view(np.uint32), h.view(np.uint32))
    mid = ((h[:-1].astype(np.float64) + h[1:].astype(np.float64)) / 2).astype(np.float32)  # exact in fp32
    _assert_same(cvr, mid, "midpoints")
    _assert_same(cvr, np.nextafter(mid, np.float32(np.inf)), "just above midpoints")
    _assert_same(cvr, np.nextafter(mid, np.float32(-np.inf)), "just below midpoints")
    _assert_same(cvr, -mid, "negative midpoints")


def test_shapes_and_in_place(cvr):
    a = np.random.default_rng(3).random((3, 5, 7), dtype=np.float32)
    assert cvr.half_round(a).shape == a.shape
    assert cvr.half_round(np.zeros(0, np.float32)).size == 0
    lib = cvr.load()
    b = a.copy().ravel()
    p = b.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.cvr_half_round(p, p, b.size) == 0  # in == out
    assert np.array_equal(b, _numpy_round(a).ravel())
    assert lib.cvr_half_round(None, None, 4) == -1  # CVR_ERR_INVALID


def test_public_surface(cvr):
    assert cvr.OPT_MEDIUM_FORMAT == 30 and (cvr.FORMAT_F32, cvr.FORMAT_F16) == (0, 1)
    lib = cvr.load()
    assert lib.cvr_abi_version() >= 5
    nm = subprocess.check_output(["nm", "-D", "--defined-only", cvr.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (cvr_\w+)", nm))
    assert {"cvr_half_round", "cvr_medium_info"} <= exported
    hdr = open(os.path.join(ROOT, "include", "cvr.h")).read()
    assert re.search(r"CVR_OPT_MEDIUM_FORMAT\s*=\s*30\b", hdr) and re.search(r"#define CVR_ABI_VERSION 5\b", hdr)
    # struct cvr_medium_info as the binding declares it
    assert C.sizeof(cvr.MediumInfo) == 48


def test_cli_lists_medium_format():
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    ext = out[out.index("Extensions:"):]
    assert "--medium-format float|half" in ext
    r = subprocess.run([CLI, "--interactive", "0", "--synthetic", "bucky", "--medium-format", "bf16"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--medium-format must be float or half" in r.stderr
