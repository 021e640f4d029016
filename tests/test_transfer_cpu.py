"""Transfer functions (cvr_classify_host, cvr_raw_transfer_table, cvr_set_medium_scalar), the
parts that need no GPU: the host statement against the numpy restatement of tests/transfer_ref.py
bit for bit, the Raw rule against the scene loader, the refusals of the descriptor, the wrapper's
and the CLI's argument checks, the ABI surface, and that the media of tests/test_gpu_transfer.py
make the oracle's paths both escape and collide."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import transfer_ref as tr
from test_device_medium_cpu import FakeDevice, FakeTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cudavolumerenderer_amd", "cvr")
INVALID = -1
f32 = np.float32


# ----------------------------------------------------------------- surface --
def test_surface(cvr):
    lib = cvr.load()
    for name in ("cvr_classify_host", "cvr_raw_transfer_table", "cvr_set_medium_scalar",
                 "cvr_set_medium_scene_transfer"):
        assert hasattr(lib, name), name
    assert C.sizeof(cvr.TransferDesc) == 24 and C.sizeof(cvr.ScalarMediumDesc) == 104
    assert [getattr(cvr.ScalarMediumDesc, f).offset for f in ("res", "flags", "d_scalar", "scalar_type", "transfer",
                                                               "box_min", "box_max", "scale", "eta")] == \
        [0, 12, 16, 24, 32, 56, 68, 80, 100]
    assert (cvr.SCALAR_F32, cvr.SCALAR_U8, cvr.SCALAR_U16, cvr.SCALAR_I16) == (0, 1, 2, 3)
    assert (cvr.TF_CEIL, cvr.TF_DENSITY_U) == (1, 2)
    hdr = open(os.path.join(ROOT, "include", "cvr.h")).read()
    assert "#define CVR_HAS_TRANSFER 1" in hdr
    assert lib.cvr_abi_version() == 6  # an addition within ABI 6


def test_header_declares_the_descriptors_within_abi6(tmp_path):
    def compiles(src, *flags):
        f = tmp_path / "t.c"
        f.write_text('#include "cvr.h"\n' + src)
        r = subprocess.run(["cc", "-std=c11", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            *flags, str(f)], capture_output=True, text=True, timeout=60)
        return r.returncode == 0, r.stderr

    use = ("#ifndef CVR_HAS_TRANSFER\n#error \"no transfer\"\n#endif\n"
           "_Static_assert(sizeof(cvr_transfer_desc) == 24, \"24 bytes\");\n"
           "_Static_assert(sizeof(cvr_scalar_medium_desc) == 104, \"104 bytes\");\n"
           "int f(cvr_ctx* c, const void* p, const float* t, float* o) { cvr_scalar_medium_desc d = {{8, 8, 8},\n"
           "  CVR_DEVMED_SPARSE, p, CVR_SCALAR_U16, 0, {7, CVR_TF_CEIL | CVR_TF_DENSITY_U, t, 0.0f, 1.0f}, {0, 0, 0},\n"
           "  {1, 1, 1}, 100.0f, 0.0f, 0.0f, {0.1f, 0.1f}, 1.04f};\n"
           "  return cvr_set_medium_scalar(c, &d) + cvr_classify_host(p, CVR_SCALAR_I16, 1, &d.transfer, o, o)\n"
           "    + cvr_raw_transfer_table(o); }\n")
    ok, err = compiles(use)
    assert ok, err
    ok, err = compiles("cvr_scalar_medium_desc d;\n", "-DCVR_ABI_TARGET=5")
    assert not ok and "cvr_scalar_medium_desc" in err
    ok, _ = compiles("#ifdef CVR_HAS_TRANSFER\n#error \"declared\"\n#endif\n", "-DCVR_ABI_TARGET=5")
    assert ok


# ------------------------------------------------- the statement, bit for bit --
def scalars(dtype, lo, hi, rng):
    """Values below lo, above hi, equal to both, around them, and random ones; f32: NaN and infinities too."""
    if dtype == np.float32:
        edge = [lo, hi, np.nextafter(f32(lo), f32(-np.inf)), np.nextafter(f32(hi), f32(np.inf)), lo - 5, hi + 5,
                np.nan, np.inf, -np.inf, 0.0, -0.0]
        body = lo - 1 + (hi - lo + 2) * rng.random(2000, dtype=np.float32)
        return np.concatenate([np.array(edge, np.float32), body.astype(np.float32)])
    info = np.iinfo(dtype)
    edge = [info.min, info.max, int(lo), int(hi), int(lo) - 1, int(hi) + 1, int(lo) + 1, int(hi) - 1]
    body = rng.integers(info.min, info.max + 1, 2000)
    return np.clip(np.concatenate([np.array(edge, np.int64), body]), info.min, info.max).astype(dtype)


def tables(n, rng):
    plain = np.empty((n, 4), np.float32)
    plain[:] = rng.random((n, 4), dtype=np.float32)
    odd = plain.copy()                      # NaN and negative entries
    odd[0, 1] = np.nan
    odd[n - 1, 3] = -2.5
    odd[n // 2, 0] = -0.75
    if n > 2:
        odd[n // 2, 3] = np.nan
    return {"plain": plain, "nan_negative": odd}


RANGES = {np.uint8: (17.0, 201.0), np.uint16: (1000.0, 60000.0), np.int16: (-12000.0, 9000.0),
          np.float32: (-0.25, 1.5)}


@pytest.mark.parametrize("n", [2, 7, 4096])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int16, np.float32])
def test_classify_host_equals_the_numpy_statement(cvr, dtype, n):
    rng = np.random.default_rng(1000 + n)
    lo, hi = RANGES[dtype]
    s = scalars(dtype, lo, hi, rng)
    below, above = (s.astype(np.float64) < lo).sum(), (s.astype(np.float64) > hi).sum()
    assert below and above and (s == dtype(lo)).any() and (s == dtype(hi)).any()
    for kind, table in tables(n, rng).items():
        for ceil in (False, True):
            for density_u in (False, True):
                what = f"{np.dtype(dtype).name} n {n} table {kind} ceil {ceil} density_u {density_u}"
                gd, ga = cvr.classify_host(s, table, lo, hi, ceil=ceil, density_u=density_u)
                wd, wa = tr.classify(s, table, lo, hi, ceil, density_u)
                assert gd.dtype == ga.dtype == np.float32 and ga.shape == s.shape + (4,)
                if ceil or kind == "plain":   # no arithmetic on a NaN entry: every bit is stated
                    assert gd.tobytes() == wd.tobytes() and ga.tobytes() == wa.tobytes(), what
                else:
                    assert tr.same_bits(gd, wd) and tr.same_bits(ga, wa), what
                assert (ga[..., 3] == 1).all(), what
                if density_u:
                    assert gd.min() == 0 and gd.max() == 1 and not np.isnan(gd).any(), what  # a NaN scalar gives 0
                if kind == "nan_negative":
                    assert np.isnan(ga).any() and (gd < 0).any() == (not density_u), what  # the entries are reached


def test_either_output_may_be_null(cvr):
    lib = cvr.load()
    s = np.arange(50, dtype=np.uint8)
    table = tr.table7()
    t = cvr.TransferDesc(7, 0, table.ctypes.data, 0.0, 49.0)
    wd, wa = tr.classify(s, table, 0.0, 49.0)
    d, a = np.empty(50, np.float32), np.empty((50, 4), np.float32)
    assert lib.cvr_classify_host(s.ctypes.data, cvr.SCALAR_U8, 50, C.byref(t), d.ctypes.data, None) == 0
    assert lib.cvr_classify_host(s.ctypes.data, cvr.SCALAR_U8, 50, C.byref(t), None, a.ctypes.data) == 0
    assert d.tobytes() == wd.tobytes() and a.tobytes() == wa.tobytes()
    assert lib.cvr_classify_host(s.ctypes.data, cvr.SCALAR_U8, 50, C.byref(t), None, None) == 0


# ------------------------------------------------------------- the Raw rule --
def test_raw_table_is_the_loader_s(cvr):
    """green -> red over 20 entries, red -> blue over 80, entry i of a ramp a + i (b - a) / 100."""
    t = cvr.raw_transfer_table()
    assert t.shape == (100, 4) and (t[:, 3] == 1).all()
    green, red, blue = (np.array(c, np.float32) for c in ((0.02, 0.2, 0.02), (1, 0.02, 0.02), (0, 0.02, 1)))
    want = np.ones((100, 4), np.float32)
    for i in range(20):
        want[i, :3] = green + f32(i) * (red - green) / f32(100)
    for i in range(80):
        want[20 + i, :3] = red + f32(i) * (blue - red) / f32(100)
    assert t.tobytes() == want.tobytes()


def test_raw_rule_is_pinned_to_the_loader(cvr):
    scene = cvr.Scene.synthetic("bucky")
    raw = np.frombuffer(scene.raw_bytes, np.uint8)
    d, a = cvr.classify_host(raw, cvr.raw_transfer_table(), lo=0.0, hi=float(raw.max()), ceil=True, density_u=True)
    assert d.tobytes() == np.ascontiguousarray(scene.density, np.float32).tobytes()
    assert a.tobytes() == np.ascontiguousarray(scene.albedo, np.float32).tobytes()
    assert len(np.unique(a.reshape(-1, 4), axis=0)) > 10  # the table's ramps are in use
    scene.close()


# ---------------------------------------------------------------- refusals --
def test_descriptor_refusals(cvr):
    s = np.arange(10, dtype=np.uint8)
    good = tr.table7()
    for kw in (dict(table=good[:1]), dict(table=np.zeros((4097, 4), np.float32)), dict(lo=1.0, hi=1.0),
               dict(lo=2.0, hi=1.0), dict(lo=np.nan), dict(hi=np.inf), dict(lo=-np.inf)):
        args = dict(table=good, lo=0.0, hi=9.0)
        args.update(kw)
        with pytest.raises(cvr.CvrError) as e:
            cvr.classify_host(s, **args)
        assert e.value.code == INVALID, kw
    lib = cvr.load()
    out = np.empty(10, np.float32)
    for t in (cvr.TransferDesc(7, 4, good.ctypes.data, 0.0, 9.0),   # an unknown flag
              cvr.TransferDesc(7, 0, None, 0.0, 9.0)):              # no table
        assert lib.cvr_classify_host(s.ctypes.data, cvr.SCALAR_U8, 10, C.byref(t), out.ctypes.data, None) == INVALID
    t = cvr.TransferDesc(7, 0, good.ctypes.data, 0.0, 9.0)
    assert lib.cvr_classify_host(s.ctypes.data, 4, 10, C.byref(t), out.ctypes.data, None) == INVALID  # scalar_type
    assert lib.cvr_classify_host(None, cvr.SCALAR_U8, 10, C.byref(t), out.ctypes.data, None) == INVALID
    assert lib.cvr_classify_host(s.ctypes.data, cvr.SCALAR_U8, 10, None, out.ctypes.data, None) == INVALID
    assert lib.cvr_set_medium_scalar(None, None) == INVALID
    assert lib.cvr_raw_transfer_table(None) == INVALID
    for bad in (np.zeros((7, 3), np.float32), np.zeros(28, np.float32)):
        with pytest.raises(ValueError):
            cvr.classify_host(s, bad, 0.0, 9.0)
    with pytest.raises(ValueError):
        cvr.classify_host(s.astype(np.int32), good, 0.0, 9.0)


def test_wrapper_checks_arguments_first(cvr):
    ctx = cvr.Context.__new__(cvr.Context)  # no GPU: no library context behind it
    ctx._h, ctx.device = None, 0
    table = tr.table7()
    bad = [
        ("dtype", dict(scalar=FakeTensor((4, 5, 6), dtype="torch.float16"))),
        ("dtype", dict(scalar=FakeTensor((4, 5, 6), dtype="torch.int32"))),
        ("contiguous", dict(scalar=FakeTensor((4, 5, 6), dtype="torch.uint8", contiguous=False))),
        ("shape", dict(scalar=FakeTensor((4, 5), dtype="torch.int16"))),
        ("shape", dict(scalar=FakeTensor((4, 5, 6), dtype="torch.uint16"), res=(4, 5, 6))),
        ("cuda:0", dict(scalar=FakeTensor((4, 5, 6), device=FakeDevice("cuda", 1)))),
        ("cuda:0", dict(scalar=FakeTensor((4, 5, 6), device=FakeDevice("cpu", None)))),
        ("res", dict(scalar=1 << 20, scalar_type=cvr.SCALAR_U8)),
        ("scalar_type", dict(scalar=1 << 20, res=(4, 5, 6))),
        ("table", dict(scalar=FakeTensor((4, 5, 6)), table=np.zeros((7, 3), np.float32))),
    ]
    for word, kw in bad:
        args = dict(table=table, lo=0.0, hi=1.0)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            ctx.set_medium_scalar(args.pop("scalar"), args.pop("table"), **args)
        assert word in str(e.value), (word, str(e.value))
    ctx._h = None


# --------------------------------------------------------------------- CLI --
def cli(*args):
    r = subprocess.run([CLI, "--interactive", "0", *args], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stderr


def test_cli_transfer_argument_errors(tmp_path):
    """Every one is found before a device is touched."""
    good = tmp_path / "good.txt"
    good.write_text("# r g b density\n0 0 0 0\n\n1 0.5 0.25 1\n")
    code, err = cli("--synthetic", "hetvol", "--transfer", str(good))
    assert code == 2 and "--transfer applies to Raw scenes only" in err, err
    code, err = cli("--synthetic", "bucky", "--transfer", str(tmp_path / "absent.txt"))
    assert code == 2 and "cannot read" in err, err
    code, err = cli("--synthetic", "bucky", "--transfer", str(good), "--transfer-mode", "cubic")
    assert code == 2 and "--transfer-mode must be linear or ceil" in err, err
    code, err = cli("--synthetic", "bucky", "--transfer")
    assert code == 2 and "required argument" in err, err
    three = tmp_path / "three.txt"
    three.write_text("0 0 0 0\n1 1 1\n")
    code, err = cli("--synthetic", "bucky", "--transfer", str(three))
    assert code == 2 and "line 2" in err and "r g b density" in err, err
    five = tmp_path / "five.txt"
    five.write_text("0 0 0 0\n1 1 1 1 1\n")
    code, err = cli("--synthetic", "bucky", "--transfer", str(five))
    assert code == 2 and "line 2" in err, err
    one = tmp_path / "one.txt"
    one.write_text("0 0 0 0\n")
    code, err = cli("--synthetic", "bucky", "--transfer", str(one))
    assert code == 2 and "1 entries" in err and "2..4096" in err, err
    many = tmp_path / "many.txt"
    many.write_text("0.5 0.5 0.5 1\n" * 4097)
    code, err = cli("--synthetic", "bucky", "--transfer", str(many))
    assert code == 2 and "4097 entries" in err, err


# ------------------------------------------- the media of the GPU tests ------
def test_cases_cover_what_they_are_for():
    c = tr.case("spikes_f32")
    assert (c.scalar < f32(c.lo)).any() and (c.scalar > f32(c.hi)).any()       # both clamps
    c = tr.case("offgrid_f32")
    assert (c.scalar < f32(c.lo)).any() and (c.scalar > f32(c.hi)).any()
    for name in ("random40_u8", "random40_u16", "random40_i16"):
        c = tr.case(name)
        assert (c.scalar < c.lo).any() and (c.scalar > c.hi).any(), name
    assert tr.case("random40_i16").scalar.min() < 0
    # the ramp reads every one of the 4096 entries
    c = tr.case("ramp4096_u16")
    x = (c.scalar.astype(np.float32) / f32(c.hi)) * f32(4095)
    i = np.minimum(np.floor(x).astype(np.int64), 4094).ravel()
    fr = x.ravel() - i.astype(np.float32)
    used = set(i[fr < 1].tolist()) | set((i[fr > 0] + 1).tolist())
    assert used == set(range(4096))
    for name in ("unaligned_u8", "unaligned_u16"):
        assert tr.case(name).scalar.shape == (5, 7, 13)
    d, a, _ = tr.classified("uniform_rgb")
    assert len(np.unique(a.reshape(-1, 4), axis=0)) == 1 and len(np.unique(d)) > 10
    # the sparse tables: zeros stay empty under "zero", nothing does under "dense"
    d, a, _ = tr.classified("sparse_small_zero")
    assert (d == 0).any() and (a[d == 0] == a[0, 0, 0]).all() and (d[tr.case("sparse_small_zero").scalar > 0] > 0).all()
    assert (tr.classified("sparse_small_dense")[0] > 0).all()
    assert len(np.unique(tr.classified("sparse_small_one_colour")[1].reshape(-1, 4), axis=0)) == 1


@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_oracle_paths_escape_and_collide(cvr, oracle_mod, name):
    """The GPU tests compare against these records: they must show escapes and real collisions."""
    ref = tr.reference(name, 0)
    assert (ref["flags"] & 1).any() and (ref["n_albedo"] > 0).any(), name
    assert not (ref["flags"] & 1).all(), name
