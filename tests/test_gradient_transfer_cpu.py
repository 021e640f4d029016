"""Gradient-magnitude transfer functions (cvr_classify_gradient_host, cvr_set_medium_gradient), the
parts that need no GPU: the ABI surface, the host statement against the numpy restatement of
tests/gradient_ref.py bit for bit, properties of the gradient, the full-LDS table, the refusals of
the descriptor, the wrapper's and the CLI's argument checks, and that the media of
tests/test_gpu_gradient_transfer.py make the oracle's paths both escape and collide."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import devmed
import gradient_ref as gr
import media
import transfer_ref as tr
from test_device_medium_cpu import FakeDevice, FakeTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cudavolumerenderer_amd", "cvr")
INVALID = -1
f32 = np.float32


# ----------------------------------------------------------------- surface --
def test_surface(cvr):
    lib = cvr.load()
    for name in ("cvr_classify_gradient_host", "cvr_set_medium_gradient", "cvr_set_medium_scene_gradient"):
        assert hasattr(lib, name), name
    assert C.sizeof(cvr.GradientTransferDesc) == 56 and C.sizeof(cvr.GradientMediumDesc) == 136
    assert [getattr(cvr.GradientTransferDesc, f).offset for f in ("n", "m", "flags", "reserved", "table", "lo", "hi",
                                                                  "glo", "ghi", "spacing")] == \
        [0, 4, 8, 12, 16, 24, 28, 32, 36, 40]
    assert [getattr(cvr.GradientMediumDesc, f).offset for f in ("res", "flags", "d_scalar", "scalar_type", "transfer",
                                                                "box_min", "box_max", "scale", "eta")] == \
        [0, 12, 16, 24, 32, 88, 100, 112, 132]
    hdr = open(os.path.join(ROOT, "include", "cvr.h")).read()
    assert "#define CVR_HAS_GRADIENT_TRANSFER 1" in hdr
    assert lib.cvr_abi_version() == 6  # an addition within ABI 6


def test_header_declares_the_descriptors_within_abi6(tmp_path):
    def compiles(src, *flags):
        f = tmp_path / "t.c"
        f.write_text('#include "cvr.h"\n' + src)
        r = subprocess.run(["cc", "-std=c11", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            *flags, str(f)], capture_output=True, text=True, timeout=60)
        return r.returncode == 0, r.stderr

    use = ("#ifndef CVR_HAS_GRADIENT_TRANSFER\n#error \"no gradient transfer\"\n#endif\n"
           "_Static_assert(sizeof(cvr_gradient_transfer_desc) == 56, \"56 bytes\");\n"
           "_Static_assert(sizeof(cvr_gradient_medium_desc) == 136, \"136 bytes\");\n"
           "int f(cvr_ctx* c, const cvr_scene* sc, const void* p, const float* t, float* o) {\n"
           "  cvr_gradient_medium_desc d = {{8, 8, 8}, CVR_DEVMED_SPARSE, p, CVR_SCALAR_U16, 0,\n"
           "    {7, 5, 0, 0, t, 0.0f, 1.0f, 0.0f, 2.0f, {1, 1, 1}}, {0, 0, 0}, {1, 1, 1}, 100.0f, 0.0f, 0.0f,\n"
           "    {0.1f, 0.1f}, 1.04f};\n"
           "  return cvr_set_medium_gradient(c, &d) + cvr_classify_gradient_host(p, CVR_SCALAR_I16, d.res, &d.transfer,\n"
           "    o, o, o) + cvr_set_medium_scene_gradient(c, sc, &d.transfer, 0); }\n")
    ok, err = compiles(use)
    assert ok, err
    ok, err = compiles("cvr_gradient_medium_desc d;\n", "-DCVR_ABI_TARGET=5")
    assert not ok and "cvr_gradient_medium_desc" in err
    ok, _ = compiles("#ifdef CVR_HAS_GRADIENT_TRANSFER\n#error \"declared\"\n#endif\n", "-DCVR_ABI_TARGET=5")
    assert ok


# ------------------------------------------------- the statement, bit for bit --
def assert_host_is_the_statement(cvr, c, what):
    gd, ga, gm = cvr.classify_gradient_host(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)
    wd, wa, wm = gr.classify(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)
    assert gd.dtype == ga.dtype == gm.dtype == np.float32 and ga.shape == c.scalar.shape + (4,), what
    assert gr.same_bits(gm, wm), what       # (a NaN magnitude's sign and payload are IEEE 754's to choose)
    assert gd.tobytes() == wd.tobytes() and ga.tobytes() == wa.tobytes(), what
    assert (ga[..., 3] == 1).all(), what
    return gd, ga, gm


@pytest.mark.parametrize("name", ["random40_u8", "random40_u16", "random40_i16", "offgrid_f32"])
def test_host_equals_the_numpy_statement(cvr, name):
    c = gr.case(name)
    _, _, i, j, _, _, _ = gr.coordinates(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)
    m, n = c.table.shape[:2]
    assert set(np.unique(i)) == set(range(n - 1)) and set(np.unique(j)) == set(range(m - 1)), name  # every cell
    assert_host_is_the_statement(cvr, c, name)


@pytest.mark.parametrize("shape", gr.THIN_SHAPES)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int16])
def test_host_equals_the_numpy_statement_on_thin_axes(cvr, shape, dtype):
    """Axes of 1, 2 and 3 voxels: no difference, only one-sided ones, one central one."""
    rng = np.random.default_rng(83)
    info = np.iinfo(dtype)
    s = rng.integers(info.min, info.max + 1, shape).astype(dtype)
    span = float(info.max) - float(info.min)
    c = gr.Case(s, gr.table2d(), info.min + 0.1 * span, info.min + 0.9 * span, 0.02 * span, 0.7 * span,
                (1.0, 2.0, 0.5), *gr.UNIT, media.SCALE, False)
    _, _, gm = assert_host_is_the_statement(cvr, c, f"{shape} {np.dtype(dtype).name}")
    assert (gm > 0).any()
    for axis in range(3):                     # an axis of one voxel adds nothing to the gradient
        if shape[axis] == 1:
            sp = list(c.spacing)
            sp[2 - axis] = 7.0
            other = cvr.classify_gradient_host(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, sp)[2]
            assert other.tobytes() == gm.tobytes()


def test_non_finite_scalars(cvr):
    c = gr.case("nonfinite_f32")
    assert c.scalar.shape == (11, 9, 10)
    assert np.isnan(c.scalar).sum() == 1 and np.isposinf(c.scalar).sum() == 1 and np.isneginf(c.scalar).sum() == 1
    u, v, _, _, _, _, mag = gr.coordinates(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)
    with np.errstate(invalid="ignore"):
        w = (mag - f32(c.glo)) / (f32(c.ghi) - f32(c.glo))
        t = (c.scalar - f32(c.lo)) / (f32(c.hi) - f32(c.lo))
        # both clamps of v: by value (w < 0, w > 1), by a NaN magnitude (0) and by an infinite one (1)
        assert (w < 0).any() and (w > 1).any() and np.isnan(mag).any() and np.isposinf(mag).any()
        assert (v[np.isnan(mag)] == 0).all() and (v[np.isposinf(mag)] == 1).all()
        # both clamps of u: by value, by the NaN and -inf voxels (0) and by the +inf voxel (1)
        assert (t < 0).any() and (t > 1).any()
        assert (u[np.isnan(c.scalar)] == 0).all() and (u[np.isneginf(c.scalar)] == 0).all()
        assert (u[np.isposinf(c.scalar)] == 1).all()
    assert u.min() == 0 and u.max() == 1 and v.min() == 0 and v.max() == 1
    gd, ga, _ = assert_host_is_the_statement(cvr, c, "non-finite")
    assert np.isfinite(gd).all() and np.isfinite(ga).all()   # a finite table gives finite outputs


# -------------------------------------------------------------- properties --
def test_constant_field_has_no_gradient(cvr):
    for dtype, value in ((np.uint8, 200), (np.int16, -1234), (np.float32, 0.37)):
        s = np.full((5, 6, 7), value, dtype)
        mag = cvr.classify_gradient_host(s, gr.table2d(), 0.0, 255.0, 0.0, 1.0, (0.3, 1.7, 2.9))[2]
        assert mag.tobytes() == np.zeros(s.shape, np.float32).tobytes()     # +0 exactly


def test_ramp_gradient_is_the_stated_rounding(cvr):
    """S = c x with spacing (2, 1, 1): fl(fl(2c) fl(0.5f / 2)) inside, fl(c fl(1.0f / 2)) on the two x faces."""
    for c in (f32(0.3), f32(7.0), f32(1.0e-3)):
        x = np.arange(9, dtype=np.float32)
        row = (c * x).astype(np.float32)
        s = np.broadcast_to(row, (4, 5, 9)).copy()
        mag = cvr.classify_gradient_host(s, gr.table2d(), 0.0, 1.0, 0.0, 1.0, (2.0, 1.0, 1.0))[2]
        h1, h2 = f32(1.0) / f32(2.0), f32(0.5) / f32(2.0)
        want = np.empty(9, np.float32)
        want[1:-1] = (row[2:] - row[:-2]) * h2
        want[0] = (row[1] - row[0]) * h1
        want[-1] = (row[-1] - row[-2]) * h1
        want = np.sqrt(((want * want) + f32(0)) + f32(0))
        assert (mag == want).all() and mag.tobytes() == np.broadcast_to(want, s.shape).tobytes()
    # with c a power of two every product c x is exact, and the property is the issue's literally
    c = f32(0.25)
    s = np.broadcast_to((c * np.arange(9, dtype=np.float32)).astype(np.float32), (4, 5, 9)).copy()
    mag = cvr.classify_gradient_host(s, gr.table2d(), 0.0, 1.0, 0.0, 1.0, (2.0, 1.0, 1.0))[2]
    inside, face = f32(f32(2) * c) * (f32(0.5) / f32(2)), c * (f32(1.0) / f32(2))
    assert (mag[..., 1:-1] == inside).all() and (mag[..., 0] == face).all() and (mag[..., -1] == face).all()


def test_equal_rows_give_the_1d_classification(cvr):
    """With table7 as every row the 2-D result is classify_host's linear one, bit for bit: a = P +
    f (Q - P) in both rows, and e = a + h (a - a) = a + h 0 = a.  This holds for tables without -0
    entries and finite results: a = -0 would give -0 + +0 = +0, an infinite a gives inf - inf."""
    row = tr.table7()
    assert not np.signbit(row).any()
    table = np.repeat(row[None], 6, axis=0)
    for name in ("random40_u8", "random40_u16", "random40_i16"):
        c = gr.case(name)
        d2, a2, mag = cvr.classify_gradient_host(c.scalar, table, c.lo, c.hi, 0.0, c.ghi)
        d1, a1 = cvr.classify_host(c.scalar, row, c.lo, c.hi)
        assert len(np.unique(mag)) > 100
        assert d2.tobytes() == d1.tobytes() and a2.tobytes() == a1.tobytes(), name


def test_full_lds_table(cvr):
    c = gr.case("full_lds_u16")
    m, n = c.table.shape[:2]
    assert (m, n) == (32, 128) and n * m == 4096 and c.scalar.shape == (16, 16, 16) and c.scalar.dtype == np.uint16
    _, _, i, j, _, _, _ = gr.coordinates(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)
    counts = {"i = n - 2": int((i == n - 2).sum()), "j = m - 2": int((j == m - 2).sum()),
              "i = 0": int((i == 0).sum()), "j = 0": int((j == 0).sum())}
    assert all(v > 0 for v in counts.values()), counts
    assert ((i == n - 2) & (j == m - 2)).any() and ((i == 0) & (j == 0)).any()   # the table's first and last entry
    assert_host_is_the_statement(cvr, c, "128 x 32 table")


def test_any_output_may_be_null(cvr):
    lib = cvr.load()
    c = gr.case("two_planes_u16")
    s = np.ascontiguousarray(c.scalar)
    tab = np.ascontiguousarray(c.table)
    t = cvr.GradientTransferDesc(tab.shape[1], tab.shape[0], 0, 0, tab.ctypes.data, c.lo, c.hi, c.glo, c.ghi)
    t.spacing[:] = c.spacing
    res = (C.c_uint32 * 3)(*s.shape[::-1])
    wd, wa, wm = gr.classify(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)
    d, a, g = np.empty(s.shape, np.float32), np.empty(s.shape + (4,), np.float32), np.empty(s.shape, np.float32)
    call = lambda *out: lib.cvr_classify_gradient_host(s.ctypes.data, cvr.SCALAR_U16, res, C.byref(t), *out)  # noqa: E731
    assert call(d.ctypes.data, None, None) == 0 and call(None, a.ctypes.data, None) == 0
    assert call(None, None, g.ctypes.data) == 0 and call(None, None, None) == 0
    assert d.tobytes() == wd.tobytes() and a.tobytes() == wa.tobytes() and g.tobytes() == wm.tobytes()


# ---------------------------------------------------------------- refusals --
def test_descriptor_refusals(cvr):
    s = np.arange(60, dtype=np.uint8).reshape(3, 4, 5)
    good = gr.table2d()
    nan, inf = float("nan"), float("inf")
    bad = [
        ("n * m", dict(table=good[:, :1])), ("n * m", dict(table=good[:1])),
        ("n * m", dict(table=np.zeros((33, 128, 4), np.float32))), ("n * m", dict(table=np.zeros((2, 2049, 4), np.float32))),
        ("hi > lo", dict(lo=1.0, hi=1.0)), ("hi > lo", dict(lo=2.0, hi=1.0)), ("finite", dict(lo=nan)),
        ("finite", dict(hi=inf)), ("finite", dict(lo=-inf)),
        ("ghi > glo", dict(glo=1.0, ghi=1.0)), ("ghi > glo", dict(glo=2.0, ghi=1.0)), ("glo >= 0", dict(glo=-0.5)),
        ("gradient range", dict(glo=nan)), ("gradient range", dict(ghi=inf)),
        ("spacing[0]", dict(spacing=(0.0, 1.0, 1.0))), ("spacing[1]", dict(spacing=(1.0, -1.0, 1.0))),
        ("spacing[2]", dict(spacing=(1.0, 1.0, nan))), ("spacing[2]", dict(spacing=(1.0, 1.0, inf))),
    ]
    for word, kw in bad:
        args = dict(table=good, lo=0.0, hi=59.0, glo=0.0, ghi=10.0)
        args.update(kw)
        with pytest.raises(cvr.CvrError) as e:
            cvr.classify_gradient_host(s, **args)
        assert e.value.code == INVALID and word in str(e.value), (kw, str(e.value))
    # the order is the header's: table size, flags / reserved, NULL table, lo / hi, glo / ghi, spacing
    with pytest.raises(cvr.CvrError) as e:
        cvr.classify_gradient_host(s, good[:1], 2.0, 1.0, 3.0, 2.0, (0.0, 1.0, 1.0))
    assert "n * m" in str(e.value)
    with pytest.raises(cvr.CvrError) as e:
        cvr.classify_gradient_host(s, good, 2.0, 1.0, 3.0, 2.0, (0.0, 1.0, 1.0))
    assert "hi > lo" in str(e.value)
    with pytest.raises(cvr.CvrError) as e:
        cvr.classify_gradient_host(s, good, 0.0, 1.0, 3.0, 2.0, (0.0, 1.0, 1.0))
    assert "ghi > glo" in str(e.value)
    lib = cvr.load()
    out = np.empty(60, np.float32)
    res = (C.c_uint32 * 3)(5, 4, 3)
    tab = np.ascontiguousarray(good)

    def desc(flags=0, reserved=0, table=tab.ctypes.data):
        t = cvr.GradientTransferDesc(7, 5, flags, reserved, table, 0.0, 59.0, 0.0, 10.0)
        t.spacing[:] = (1.0, 1.0, 1.0)
        return t

    for t in (desc(flags=1), desc(flags=2), desc(reserved=1), desc(table=None)):
        assert lib.cvr_classify_gradient_host(s.ctypes.data, cvr.SCALAR_U8, res, C.byref(t), out.ctypes.data, None,
                                              None) == INVALID
    t = desc()
    assert lib.cvr_classify_gradient_host(s.ctypes.data, cvr.SCALAR_U8, res, C.byref(t), out.ctypes.data, None, None) == 0
    assert lib.cvr_classify_gradient_host(s.ctypes.data, 4, res, C.byref(t), out.ctypes.data, None, None) == INVALID
    assert lib.cvr_classify_gradient_host(None, cvr.SCALAR_U8, res, C.byref(t), out.ctypes.data, None, None) == INVALID
    assert lib.cvr_classify_gradient_host(s.ctypes.data, cvr.SCALAR_U8, None, C.byref(t), out.ctypes.data, None,
                                          None) == INVALID
    assert lib.cvr_classify_gradient_host(s.ctypes.data, cvr.SCALAR_U8, res, None, out.ctypes.data, None, None) == INVALID
    assert lib.cvr_set_medium_gradient(None, None) == INVALID
    assert lib.cvr_set_medium_scene_gradient(None, None, None, 0) == INVALID
    for bad_table in (np.zeros((5, 7, 3), np.float32), np.zeros((7, 4), np.float32)):
        with pytest.raises(ValueError):
            cvr.classify_gradient_host(s, bad_table, 0.0, 59.0, 0.0, 10.0)
    with pytest.raises(ValueError):
        cvr.classify_gradient_host(s.astype(np.int32), good, 0.0, 59.0, 0.0, 10.0)
    with pytest.raises(ValueError):
        cvr.classify_gradient_host(s.ravel(), good, 0.0, 59.0, 0.0, 10.0)
    with pytest.raises(ValueError):
        cvr.classify_gradient_host(s, good, 0.0, 59.0, 0.0, 10.0, spacing=(1.0, 1.0))


def test_wrapper_checks_arguments_first(cvr):
    ctx = cvr.Context.__new__(cvr.Context)  # no GPU: no library context behind it
    ctx._h, ctx.device = None, 0
    table = gr.table2d()
    bad = [
        ("dtype", dict(scalar=FakeTensor((4, 5, 6), dtype="torch.float16"))),
        ("contiguous", dict(scalar=FakeTensor((4, 5, 6), dtype="torch.uint8", contiguous=False))),
        ("shape", dict(scalar=FakeTensor((4, 5), dtype="torch.int16"))),
        ("cuda:0", dict(scalar=FakeTensor((4, 5, 6), device=FakeDevice("cuda", 1)))),
        ("res", dict(scalar=1 << 20, scalar_type=cvr.SCALAR_U8)),
        ("scalar_type", dict(scalar=1 << 20, res=(4, 5, 6))),
        ("table", dict(scalar=FakeTensor((4, 5, 6)), table=np.zeros((7, 4), np.float32))),
        ("spacing", dict(scalar=FakeTensor((4, 5, 6)), spacing=(1.0,))),
    ]
    for word, kw in bad:
        args = dict(table=table, lo=0.0, hi=1.0, glo=0.0, ghi=1.0)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            ctx.set_medium_gradient(args.pop("scalar"), args.pop("table"), **args)
        assert word in str(e.value), (word, str(e.value))
    ctx._h = None


# --------------------------------------------------------------------- CLI --
def cli(*args):
    r = subprocess.run([CLI, "--interactive", "0", *args], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stderr


def test_cli_transfer2d_argument_errors(tmp_path):
    """Every one is found before a device is touched."""
    good = tmp_path / "good.txt"
    good.write_text("# n m\n2 2\n\n0 0 0 0\n1 0.5 0.25 1\n# row 1\n0 0 0 0.5\n1 1 1 1\n")
    rng = ("--gradient-range", "0", "100")

    def err_of(*args):
        code, err = cli(*args)
        assert code == 2 and "[ConfigParser] Error:" in err, (args, code, err)
        return err

    assert "--transfer2d applies to Raw scenes only" in err_of("--synthetic", "hetvol", "--transfer2d", str(good), *rng)
    assert "needs --gradient-range" in err_of("--synthetic", "bucky", "--transfer2d", str(good))
    assert "excludes --transfer" in err_of("--synthetic", "bucky", "--transfer2d", str(good), *rng, "--transfer",
                                           str(good))
    assert "applies to --transfer2d only" in err_of("--synthetic", "bucky", *rng)
    assert "cannot read" in err_of("--synthetic", "bucky", "--transfer2d", str(tmp_path / "absent.txt"), *rng)
    assert "required argument" in err_of("--synthetic", "bucky", "--transfer2d")
    assert "needs 2 values" in err_of("--synthetic", "bucky", "--transfer2d", str(good), "--gradient-range", "1")
    assert "0 <= GLO < GHI" in err_of("--synthetic", "bucky", "--transfer2d", str(good), "--gradient-range", "5", "5")
    assert "needs 3 values" in err_of("--synthetic", "bucky", "--transfer2d", str(good), *rng, "--voxel-spacing", "1", "1")
    assert "--voxel-spacing must be" in err_of("--synthetic", "bucky", "--transfer2d", str(good), *rng,
                                               "--voxel-spacing", "1", "0", "1")
    files = {
        "nosize.txt": ("0 0 0 0\n1 1 1 1\n", "not 'n m'"),
        "small.txt": ("1 4\n0 0 0 0\n", "n >= 2"),
        "big.txt": ("128 33\n", "n*m <= 4096"),
        "three.txt": ("2 2\n0 0 0 0\n1 1 1\n", "line 3"),
        "few.txt": ("2 2\n0 0 0 0\n1 1 1 1\n0 0 0 0\n", "fewer than"),
        "many.txt": ("2 2\n" + "0.5 0.5 0.5 1\n" * 5, "more than"),
        "empty.txt": ("# nothing\n\n", "no 'n m' line"),
    }
    for name, (text, word) in files.items():
        f = tmp_path / name
        f.write_text(text)
        assert word in err_of("--synthetic", "bucky", "--transfer2d", str(f), *rng), name


# ------------------------------------------- the media of the GPU tests ------
def test_cases_cover_what_they_are_for():
    for name in ("thin523_u8", "thin523_u16"):
        assert gr.case(name).scalar.shape == (3, 5, 523) and gr.OFFSET[name] == gr.case(name).scalar.itemsize
    assert gr.case("two_planes_u16").scalar.shape == (2, 9, 33)
    assert gr.case("one_plane_u8").scalar.shape == (1, 9, 33) and gr.case("one_column_u8").scalar.shape == (9, 33, 1)
    assert gr.case("offgrid_f32").box_min != gr.UNIT[0]
    # the halo: four of the 27 leaves exist, three of them through the gradient alone
    c = gr.case("halo")
    assert c.scalar.shape == (24, 24, 21) and c.glo == 0 and int((c.scalar != 0).sum()) == 1 and c.scalar[7, 7, 7] == 65535
    assert c.table[0, 0, 3] == 0 and (np.delete(c.table[..., 3].ravel(), 0) > 0).all()
    d, a, _ = gr.classified("halo")
    sp = devmed.leaf_rule(d, a)
    assert sp.table.shape == (3, 3, 3) and sp.leaf_density.shape[0] == 4 and sp.leaf_albedo is not None
    exist = {(x, y, z) for z, y, x in zip(*np.nonzero(sp.table != devmed.NO_LEAF))}
    assert exist == {(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)}
    for x, y, z in exist - {(0, 0, 0)}:
        assert not c.scalar[8 * z:8 * z + 8, 8 * y:8 * y + 8, 8 * x:8 * x + 8].any()     # zero scalars only
    assert c.scalar.shape[2] % 8 != 0                                                    # x ends in a partial leaf
    sp = devmed.leaf_rule(*gr.classified("halo_one_colour")[:2])
    assert sp.leaf_density.shape[0] == 4 and sp.leaf_albedo is None
    assert devmed.leaf_rule(*gr.classified("halo_positive")[:2]).leaf_density.shape[0] == 27


@pytest.mark.parametrize("name", sorted(gr.CASES))
def test_oracle_paths_escape_and_collide(cvr, oracle_mod, name):
    """The GPU tests compare against these records: they must show escapes and real collisions."""
    ref = gr.reference(name, 0)
    assert (ref["flags"] & 1).any() and (ref["n_albedo"] > 0).any(), name
    assert not (ref["flags"] & 1).all(), name
