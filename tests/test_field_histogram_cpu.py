"""Field statistics and value-gradient histograms on the CPU: cvr_field_stats_host and
cvr_field_histogram_host against the numpy restatement (tests/histogram_ref.py), the bin rule
against the classification's own coordinates, the refusals in the header's order, and the kernels'
launch geometry against the shapes the GPU tests use.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import gradient_ref as gr
import histogram_ref as hr

INVALID = -1


def host_histogram(cvr, name, n, m):
    f = hr.field(name)
    return cvr.field_histogram_host(f.scalar, n, m, lo=f.lo, hi=f.hi, glo=f.glo, ghi=f.ghi, spacing=f.spacing)


# ------------------------------------------------------ host against numpy --
@pytest.mark.parametrize("case", hr.HISTOGRAMS, ids=hr.ident)
def test_host_histogram_equals_numpy(cvr, case):
    name, n, m = case
    got = host_histogram(cvr, name, n, m)
    assert got.dtype == np.uint32 and got.shape == (m, n)
    assert np.array_equal(got, hr.ref_histogram(name, n, m))
    assert int(got.sum(dtype=np.uint64)) == hr.field(name).scalar.size


@pytest.mark.parametrize("name", hr.STATS)
def test_host_stats_equal_numpy(cvr, name):
    f = hr.field(name)
    got, want = cvr.field_stats_host(f.scalar, f.spacing), hr.ref_stats(name)
    assert hr.same_stats(got, want), (got, want)


def test_nonfinite_field_is_what_it_claims(cvr):
    """inf - inf magnitudes count in nan_gradients, +inf magnitudes in gmax, -0 orders below +0."""
    f = hr.field("nonfinite_f32")
    st = cvr.field_stats_host(f.scalar, f.spacing)
    mag = hr.mag_of("nonfinite_f32")
    assert np.isnan(mag[4, 5, 31]) and not np.isnan(f.scalar[4, 5, 31])
    assert st.nan_values == 2 and st.nan_gradients > st.nan_values
    assert st.vmin == -np.inf and st.vmax == np.inf and st.gmax == np.inf
    z = np.array([[[0.0, -0.0, 0.0]]], np.float32)
    st = cvr.field_stats_host(z)
    assert np.signbit(st.vmin) and not np.signbit(st.vmax) and st.vmin == 0 and st.vmax == 0
    st = cvr.field_stats_host(hr.field("all_nan_f32").scalar)
    assert (st.vmin, st.vmax, st.gmax, st.nan_values, st.nan_gradients) == (np.inf, -np.inf, 0.0, 60, 60)


# ---------------------------------------------- bin = nearest table entry --
@pytest.mark.parametrize("name", ["random40_u8", "random40_u16", "random40_i16", "offgrid_f32", "nonfinite_f32"])
def test_bin_is_the_nearest_table_entry(cvr, name):
    """For every voxel, bin_i == min(i + (f >= 0.5), n - 1) with the classification's own cell i and
    weight f (gradient_ref.coordinates), and likewise j: the histogram's bins are the table's nodes."""
    c = gr.case(name)
    m, n = c.table.shape[:2]
    _, _, i, j, f, h, _ = gr.coordinates(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)
    bi = np.minimum(i + (f >= np.float32(0.5)), n - 1)
    bj = np.minimum(j + (h >= np.float32(0.5)), m - 1)
    want = np.bincount((bj * n + bi).reshape(-1), minlength=n * m).reshape(m, n)
    got = cvr.field_histogram_host(c.scalar, n, m, lo=c.lo, hi=c.hi, glo=c.glo, ghi=c.ghi, spacing=c.spacing)
    assert np.array_equal(got, want)


# ------------------------------------------------------- identity and ties --
@pytest.mark.parametrize("dtype,lo,hi,n", [(np.uint8, 0.0, 255.0, 256), (np.uint16, 0.0, 65535.0, 65536),
                                            (np.int16, -32768.0, 32767.0, 65536)])
def test_integer_codes_bin_to_themselves(cvr, dtype, lo, hi, n):
    codes = (np.arange(n, dtype=np.int64) + int(lo)).astype(dtype)
    field = np.concatenate([codes, codes[::3]]).reshape(1, 1, -1)     # every code, a third of them twice
    got = cvr.field_histogram_host(field, n, lo=lo, hi=hi)
    want = np.ones(n, np.uint32)
    want[::3] += 1
    assert np.array_equal(got[0], want)


def test_ties_go_upward(cvr):
    field = (np.arange(9, dtype=np.float32) / np.float32(8)).reshape(1, 3, 3)
    got = cvr.field_histogram_host(field, 5, lo=0.0, hi=1.0)
    # k / 8 -> bins 0 1 1 2 2 3 3 4 4
    assert got[0].tolist() == [1, 2, 2, 2, 2]


def test_out_of_range_values_fall_into_the_edge_bins(cvr):
    n = 6
    for value, want in [(-3.0, 0), (0.99, 0), (9.5, n - 1), (np.nan, 0), (np.inf, n - 1), (-np.inf, 0)]:
        field = np.full((2, 2, 2), value, np.float32)
        got = cvr.field_histogram_host(field, n, lo=1.0, hi=9.0)
        assert got[0, want] == 8 and got.sum() == 8, (value, got)
    # the gradient axis: an infinite magnitude falls into the last row, a NaN one into row 0
    field = np.zeros((1, 1, 5), np.float32)
    field[0, 0, 0] = np.inf
    got = cvr.field_histogram_host(field, 2, 3, lo=0.0, hi=1.0, glo=0.0, ghi=1.0)
    # voxel 0 (+inf, value bin 1): inf - inf along the one-voxel axes, a NaN magnitude (row 0);
    # voxel 1: (0 - inf) * 0.5 along x, an infinite one (row 2); the rest: 0 (row 0)
    assert got.tolist() == [[3, 1], [0, 0], [1, 0]]


# ---------------------------------------------------------------- refusals --
def descs(cvr, scalar=None, n=4, m=3):
    s = np.zeros((2, 3, 4), np.uint16) if scalar is None else scalar
    f = cvr.FieldDesc()
    f.res[:] = s.shape[::-1]
    f.scalar_type = cvr.SCALAR_U16
    f.scalar = s.ctypes.data
    f.spacing[:] = (1.0, 1.0, 1.0)
    h = cvr.HistogramDesc(n, m, 0, 0, 0.0, 1.0, 0.0, 1.0)
    return s, f, h


def set_res(f, *res):
    f.res[:] = res


def set_spacing(f, k, v):
    f.spacing[k] = v


# One breach of each rule in the header's order (rule 1, the NULL arguments, is tested apart): the
# edit of (field desc, histogram desc, counts flag) and a word of the message.
BREACHES = [
    ("2 zero extent", lambda f, h: set_res(f, 4, 0, 2), "empty field"),
    ("2 too many voxels", lambda f, h: set_res(f, 65536, 65536, 1), "more than 2^32 - 1"),
    ("3 scalar_type", lambda f, h: setattr(f, "scalar_type", 4), "unknown scalar_type"),
    ("3 field reserved", lambda f, h: setattr(f, "reserved", 1), "reserved"),
    ("3 flags", lambda f, h: setattr(h, "flags", 1), "flags"),
    ("4 n", lambda f, h: setattr(h, "n", 1), "bins"),
    ("4 n * m", lambda f, h: (setattr(h, "n", 257), setattr(h, "m", 256)), "bins"),
    ("5 hi <= lo", lambda f, h: setattr(h, "hi", 0.0), "value range"),
    ("5 lo not finite", lambda f, h: setattr(h, "lo", float("nan")), "value range"),
    ("6 glo < 0", lambda f, h: setattr(h, "glo", -1.0), "gradient range"),
    ("6 ghi <= glo", lambda f, h: setattr(h, "ghi", 0.0), "gradient range"),
    ("7 spacing", lambda f, h: set_spacing(f, 1, 0.0), "voxel spacing[1]"),
    ("7 spacing not finite", lambda f, h: set_spacing(f, 2, float("inf")), "voxel spacing[2]"),
    ("8 NULL scalar", lambda f, h: setattr(f, "scalar", None), "scalar is NULL"),
    ("8 NULL counts", "counts", "counts is NULL"),
    ("9 misaligned", lambda f, h: setattr(f, "scalar", f.scalar + 1), "2-byte aligned"),
]


def apply(breach, f, h):
    """Breaks one rule; returns whether the counts pointer is to be NULL."""
    if breach == "counts":
        return True
    breach(f, h)
    return False


def histogram_refusal(cvr, f, h, null_counts):
    lib = cvr.load()
    counts = np.zeros(65536, np.uint32)
    code = lib.cvr_field_histogram_host(C.byref(f), C.byref(h), None if null_counts else counts.ctypes.data)
    return code, (lib.cvr_last_error(None) or b"").decode()


@pytest.mark.parametrize("k", range(len(BREACHES)), ids=[b[0] for b in BREACHES])
def test_histogram_refusals(cvr, k):
    _keep, f, h = descs(cvr)
    name, breach, word = BREACHES[k]
    code, msg = histogram_refusal(cvr, f, h, apply(breach, f, h))
    assert code == INVALID and word in msg, (name, code, msg)


@pytest.mark.parametrize("k", range(len(BREACHES) - 1), ids=[b[0] for b in BREACHES[:-1]])
def test_the_earlier_of_two_broken_rules_is_reported(cvr, k):
    """Every breach together with each later one of another rule reports its own message."""
    name, breach, word = BREACHES[k]
    for later_name, later, later_word in BREACHES[k + 1:]:
        if later_name[0] == name[0]:
            continue
        _keep, f, h = descs(cvr)
        null = apply(later, f, h)
        null = apply(breach, f, h) or null
        code, msg = histogram_refusal(cvr, f, h, null)
        assert code == INVALID and word in msg, (name, later_name, msg)


def test_stats_refusals_and_null_arguments(cvr):
    lib = cvr.load()
    _keep, f, h = descs(cvr)
    st = cvr._lib.FieldStatsStruct()
    counts = np.zeros(12, np.uint32)
    assert lib.cvr_field_stats_host(None, C.byref(st)) == INVALID
    assert lib.cvr_field_stats_host(C.byref(f), None) == INVALID
    assert lib.cvr_field_histogram_host(None, C.byref(h), counts.ctypes.data) == INVALID
    assert lib.cvr_field_histogram_host(C.byref(f), None, counts.ctypes.data) == INVALID
    assert lib.cvr_field_stats_host(C.byref(f), C.byref(st)) == 0
    for name, breach, word in BREACHES:
        if name[0] in "2379" or name == "8 NULL scalar":
            _keep, f, h = descs(cvr)
            if name == "3 flags":
                continue
            breach(f, h)
            assert lib.cvr_field_stats_host(C.byref(f), C.byref(st)) == INVALID, name
            assert word in lib.cvr_last_error(None).decode(), name
    # m == 1: glo, ghi and the spacing are neither read nor judged
    _keep, f, h = descs(cvr, m=1)
    h.glo, h.ghi = float("nan"), -1.0
    f.spacing[:] = (0.0, float("nan"), -1.0)
    assert lib.cvr_field_histogram_host(C.byref(f), C.byref(h), counts.ctypes.data) == 0
    assert counts[:4].tolist() == [24, 0, 0, 0]
    # a NULL scalar is not looked at before the shape (rule 2 before rule 8)
    _keep, f, h = descs(cvr)
    f.scalar = None
    f.res[:] = (0, 1, 1)
    assert lib.cvr_field_stats_host(C.byref(f), C.byref(st)) == INVALID
    assert "empty field" in lib.cvr_last_error(None).decode()


def test_python_argument_checks(cvr):
    with pytest.raises(ValueError):
        cvr.field_histogram_host(np.zeros((2, 2, 2), np.float64), 4, lo=0, hi=1)
    with pytest.raises(ValueError):
        cvr.field_histogram_host(np.zeros((2, 2), np.uint8), 4, lo=0, hi=1)
    with pytest.raises(ValueError):
        cvr.field_histogram_host(np.zeros((2, 2, 2), np.uint8), 4, 2, lo=0, hi=1)   # m > 1 without glo, ghi
    with pytest.raises(ValueError):
        cvr.field_stats_host(np.zeros((2, 2, 2), np.uint8), spacing=(1, 1))


# ---------------------------------------------------------------- geometry --
def test_field_geometry_and_the_shapes_that_cross_it(cvr):
    """The constants the launches use are exported, and the sized fields of the GPU tests do cross
    them: a moved cap fails here instead of silently shrinking what those tests cover."""
    out = (C.c_uint32 * 8)()
    assert cvr.load().cvr_debug_field_geometry(out) == 0 and out[7] == 5
    assert cvr.load().cvr_debug_field_geometry(None) == INVALID
    g = cvr.field_geometry()
    assert [g[k] for k in ("walk_tasks", "walk_z", "hist1d_grid", "lds_bins", "max_bins")] == list(out[:5])
    # the bin shapes around the LDS limit and at the largest size
    assert 128 * 128 == g["lds_bins"] and 129 * 127 < g["lds_bins"] < 129 * 128 and 256 * 256 == g["max_bins"]
    assert (129, 128) in hr.BINS_2D and (128, 128) in hr.BINS_2D and (256, 256) in hr.BINS_2D
    # more walk tasks than workgroups, in both histogram kinds
    z, y, x = hr.field("more_tasks_u8").scalar.shape
    tasks = -(-x // 256) * y * -(-z // g["walk_z"])
    assert tasks > g["walk_tasks"] and z > g["walk_z"]
    assert ("more_tasks_u8", 7, 5) in hr.HISTOGRAMS and ("more_tasks_u8", 129, 128) in hr.HISTOGRAMS
    # (the LDS kind's grid is also held to voxels / bins workgroups: 7 x 5 leaves the cap in force)
    assert x * y * z // 35 > g["walk_tasks"]
    # two x-runs and three z-chunks, the last of each ragged
    z, y, x = hr.field("runs_u16").scalar.shape
    assert 256 < x < 512 and x % 256 and 2 * g["walk_z"] < z < 3 * g["walk_z"]
    # the 1-D grid at its cap takes a second trip
    n = hr.field("long_1d_u8").scalar.size
    assert g["hist1d_grid"] * 256 * 16 < n < g["hist1d_grid"] * 256 * 16 + 64 and n // 256 > g["hist1d_grid"]
    # one bin past any 16-bit counter
    assert hr.field("constant_u8").scalar.size == 262144


def test_the_build_and_the_field_kernels_report_one_walk(cvr):
    """k_gradient and k_field_walk run one walk (csrc/cvr_gradient.h): both geometry reports give
    its task cap and its z run."""
    b, f = cvr.build_geometry(), cvr.field_geometry()
    assert (b["gradient_tasks"], b["gradient_z"]) == (f["walk_tasks"], f["walk_z"])
