"""The labelled classification on the CPU: cvr_classify_labels_host against tests/labels_ref.py bit
for bit, m = 1 against cvr_classify_host, the label counts, the descriptor's refusals in the
header's order, that the fixtures see a wrong row, the wrapper's argument checks, and that the
media of tests/test_gpu_labels.py cross the build kernels' per-trip capacity."""
import ctypes as C

import numpy as np
import pytest

import build_scale as bs
import devmed
import labels_ref as lr
import transfer_ref as tr
from test_device_medium_cpu import FakeDevice, FakeTensor

INVALID = -1
f32 = np.float32


def test_surface(cvr):
    lib = cvr.load()
    for name in ("cvr_classify_labels_host", "cvr_set_medium_labeled", "cvr_medium_label_info",
                 "cvr_set_medium_scene_labels"):
        assert hasattr(lib, name), name
    assert C.sizeof(cvr.LabelTransferDesc) == 32 and C.sizeof(cvr.LabeledMediumDesc) == 120
    assert [getattr(cvr.LabelTransferDesc, f).offset for f in ("n", "m", "flags", "reserved", "table", "lo", "hi")] == \
        [0, 4, 8, 12, 16, 24, 28]
    assert cvr.LabeledMediumDesc.d_labels.offset == 112 and cvr.LabeledMediumDesc.transfer.offset == 32


# ----------------------------------------------------------- the statement --
def _special_scalars(dtype, shape, seed):
    """The field with NaN, infinities and values outside [lo, hi] (f32), or the type's extremes."""
    s = lr.field(dtype, shape, seed).copy()
    flat = s.reshape(-1)
    if s.dtype == np.float32:
        flat[:8] = [np.nan, np.inf, -np.inf, -3.0, 7.5, 0.1, 0.8, -0.0]
    else:
        info = np.iinfo(s.dtype)
        flat[:4] = [info.min, info.max, info.min + 1, info.max - 1]
    return s


@pytest.mark.parametrize("m", [1, 2, 5, 256])
@pytest.mark.parametrize("density_u", [False, True])
@pytest.mark.parametrize("ceil", [False, True])
@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int16", "float32"])
def test_host_statement_is_the_numpy_statement(cvr, dtype, ceil, density_u, m):
    shape = (5, 7, 13)
    s = _special_scalars(dtype, shape, 700 + m)
    lab = lr.labels_iid(shape, m, 710 + m, stray=0.2)
    if m < 256:
        assert (lab >= m).any() and (lab == 255).any() and (lab == m).any() or m == 1
        lab.reshape(-1)[3] = m           # the first byte the table has no row for
    table = lr.tables(m, 16 if m == 256 else 7, 720)
    lo, hi = lr.window(dtype)
    d, a, n = cvr.classify_labels_host(s, lab, table, lo, hi, ceil=ceil, density_u=density_u)
    wd, wa, wn = lr.classify(s, lab, table, lo, hi, ceil, density_u)
    assert d.dtype == np.float32 and d.shape == shape and a.shape == shape + (4,)
    assert tr.same_bits(d, wd) and tr.same_bits(a, wa)
    assert n.dtype == np.uint64 and (n == wn).all() and (n == np.bincount(lab.reshape(-1), minlength=256)).all()
    assert int(n.sum()) == lab.size


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int16", "float32"])
def test_one_row_is_the_scalar_statement_whatever_the_labels(cvr, dtype):
    s = _special_scalars(dtype, (5, 7, 13), 731)
    lo, hi = lr.window(dtype)
    table = tr.table7()
    for flags in ((False, False), (True, True)):
        wd, wa = cvr.classify_host(s, table, lo, hi, ceil=flags[0], density_u=flags[1])
        for lab in (np.zeros(s.shape, np.uint8), np.full(s.shape, 255, np.uint8), lr.labels_iid(s.shape, 200, 733)):
            d, a, _ = cvr.classify_labels_host(s, lab, table[None], lo, hi, ceil=flags[0], density_u=flags[1])
            assert tr.same_bits(d, wd) and tr.same_bits(a, wa)


def test_nothing_interpolates_across_rows(cvr):
    """A voxel of label j takes row j's entries alone: with rows of one value each, that value."""
    s = lr.field(np.uint16, (4, 5, 6), 741)
    lab = lr.labels_iid(s.shape, 4, 743, stray=0.0)
    table = np.empty((4, 3, 4), np.float32)
    for j in range(4):
        table[j] = f32(0.125) * (j + 1)
    d, a, _ = cvr.classify_labels_host(s, lab, table, 0.0, 65535.0)
    row = np.where(lab < 4, lab, 0).astype(np.float32)      # (255 is planted: row 0)
    assert (d == f32(0.125) * (row + 1)).all() and (a[..., 0] == d).all() and (a[..., 3] == 1).all()


@pytest.mark.parametrize("name", ["ragged_u8", "ragged_u16", "ragged_f32", "sparse_hidden", "full_table"])
def test_a_row_swap_changes_the_output(cvr, name):
    """The fixtures can see a wrong row: any two rows exchanged change stored bits."""
    c = lr.case(name)
    d, a, _ = lr.host(name)
    m = c.table.shape[0]
    for j, k in ((0, 1), (1, m - 1), (0, m - 1)):
        if j == k:
            continue
        t = c.table.copy()
        t[[j, k]] = t[[k, j]]
        d2, a2, _ = cvr.classify_labels_host(c.scalar, c.labels, t, c.lo, c.hi, ceil=c.ceil, density_u=c.density_u)
        assert d2.tobytes() != d.tobytes() and a2.tobytes() != a.tobytes(), (name, j, k)
    # and so does a label volume shifted by one voxel
    shifted = np.roll(c.labels.reshape(-1), 1).reshape(c.labels.shape)
    d3, a3, _ = cvr.classify_labels_host(c.scalar, shifted, c.table, c.lo, c.hi, ceil=c.ceil, density_u=c.density_u)
    assert d3.tobytes() != d.tobytes() and a3.tobytes() != a.tobytes(), name


@pytest.mark.parametrize("name", ["ragged_u8", "ragged_i16", "tiny_u8", "sparse_hidden", "full_table", "mostly_one"])
def test_the_gpu_cases_host_arrays_are_the_numpy_statement_s(cvr, name):
    d, a, n = lr.host(name)
    wd, wa, wn = lr.classified(name)
    assert d.tobytes() == wd.tobytes() and a.tobytes() == wa.tobytes() and (n == wn).all(), name


def test_null_outputs(cvr):
    lib = cvr.load()
    s, lab = lr.field(np.uint8, (2, 3, 5), 751), lr.labels_iid((2, 3, 5), 3, 753)
    tab = np.ascontiguousarray(lr.tables(3))
    t = cvr.LabelTransferDesc(7, 3, 0, 0, tab.ctypes.data, 0.0, 255.0)
    assert lib.cvr_classify_labels_host(s.ctypes.data, cvr.SCALAR_U8, lab.ctypes.data, s.size, C.byref(t), None, None,
                                        None) == 0
    counts = np.zeros(256, np.uint64)
    assert lib.cvr_classify_labels_host(s.ctypes.data, cvr.SCALAR_U8, lab.ctypes.data, s.size, C.byref(t), None, None,
                                        counts.ctypes.data) == 0
    assert (counts == np.bincount(lab.reshape(-1), minlength=256)).all()
    assert lib.cvr_classify_labels_host(None, cvr.SCALAR_U8, None, 0, C.byref(t), None, None, None) == 0   # no voxels
    assert lib.cvr_classify_labels_host(s.ctypes.data, cvr.SCALAR_U8, None, s.size, C.byref(t), None, None, None) == INVALID


# ---------------------------------------------------------------- refusals --
def test_descriptor_refusals_come_in_the_header_s_order(cvr):
    """Each bad descriptor is wrong in its own item and in every later one, and its own is named."""
    lib = cvr.load()
    s, lab = lr.field(np.uint8, (2, 3, 5), 761), lr.labels_iid((2, 3, 5), 3, 763)
    tab = np.ascontiguousarray(np.zeros((4096, 4), np.float32))
    nan = float("nan")

    def refused(n, m, flags, reserved, table, lo, hi, scalar_type=cvr.SCALAR_U8):
        t = cvr.LabelTransferDesc(n, m, flags, reserved, table, lo, hi)
        code = lib.cvr_classify_labels_host(s.ctypes.data, scalar_type, lab.ctypes.data, s.size, C.byref(t), None, None,
                                            None)
        assert code == INVALID
        return lib.cvr_last_error(None).decode()

    p = tab.ctypes.data
    assert "scalar_type" in refused(1, 0, 4, 1, None, 2.0, 1.0, scalar_type=4)       # 2, with 3..6 wrong too
    for n, m in ((1, 3), (7, 0), (7, 257), (2, 2049), (4097, 1), (16, 257)):         # 3, with 4..6 wrong too
        assert "n * m" in refused(n, m, 4, 1, None, 2.0, 1.0), (n, m)
    assert "flags" in refused(7, 3, 4, 0, None, 2.0, 1.0)                            # 4 (flags), 5 and 6 wrong too
    assert "reserved" in refused(7, 3, 0, 1, None, 2.0, 1.0)                         # 4 (reserved)
    assert "NULL" in refused(7, 3, 3, 0, None, 2.0, 1.0)                             # 5, with 6 wrong too
    for lo, hi in ((2.0, 1.0), (1.0, 1.0), (nan, 1.0), (0.0, float("inf"))):         # 6
        assert "hi > lo" in refused(7, 3, 3, 0, p, lo, hi), (lo, hi)
    # the limits themselves are allowed
    for n, m in ((2, 1), (16, 256), (4096, 1), (2, 256)):
        t = cvr.LabelTransferDesc(n, m, 3, 0, p, 0.0, 255.0)
        assert lib.cvr_classify_labels_host(s.ctypes.data, cvr.SCALAR_U8, lab.ctypes.data, s.size, C.byref(t), None,
                                            None, None) == 0, (n, m)


def test_wrapper_argument_checks(cvr):
    s, lab = lr.field(np.uint8, (2, 3, 5), 771), lr.labels_iid((2, 3, 5), 3, 773)
    with pytest.raises(ValueError, match="expected \\(m, n, 4\\)"):
        cvr.classify_labels_host(s, lab, lr.tables(3)[0], 0.0, 255.0)
    with pytest.raises(ValueError, match="labels"):
        cvr.classify_labels_host(s, lab.astype(np.uint16), lr.tables(3), 0.0, 255.0)
    with pytest.raises(ValueError, match="labels"):
        cvr.classify_labels_host(s, lab[:1], lr.tables(3), 0.0, 255.0)
    with pytest.raises(ValueError, match="scalar"):
        cvr.classify_labels_host(s.astype(np.float64), lab, lr.tables(3), 0.0, 255.0)
    # Context.set_medium_labeled judges its tensors before the library sees them
    ctx = cvr.Context.__new__(cvr.Context)
    ctx.device, ctx._h = 0, None
    dev = FakeDevice("cuda", 0)
    field = FakeTensor((2, 3, 5), "torch.uint8", device=dev)
    with pytest.raises(ValueError, match="labels: 29 elements"):
        ctx.set_medium_labeled(field, FakeTensor((29,), "torch.uint8", device=dev), lr.tables(3), lo=0.0, hi=255.0)
    with pytest.raises(ValueError, match="labels: dtype"):
        ctx.set_medium_labeled(field, FakeTensor((2, 3, 5), "torch.int8", device=dev), lr.tables(3), lo=0.0, hi=255.0)
    with pytest.raises(ValueError, match="labels: on"):
        ctx.set_medium_labeled(field, FakeTensor((30,), "torch.uint8", device=FakeDevice("cpu", None)), lr.tables(3), lo=0.0,
                               hi=255.0)
    with pytest.raises(ValueError, match="res is required"):
        ctx.set_medium_labeled(1234, 5678, lr.tables(3), lo=0.0, hi=255.0)


# ------------------------------------------------------------------- media --
def test_the_ragged_grid_has_a_head_a_partial_run_and_a_tail():
    """Of the scalar views at 0 and 1 elements: every one has a partial last run of 64 groups; per
    type one has a head and one a tail (u8 at 1: both; u16 at 0: a 7-voxel tail, at 1: a 7-voxel head)."""
    n = lr.SHAPE[0] * lr.SHAPE[1] * lr.SHAPE[2]
    for size in (1, 2):
        per_group = 16 // size
        heads, tails = [], []
        for offset_elems in (0, 1):
            head = ((16 - offset_elems * size) % 16) // size
            groups = (n - head) // per_group
            assert groups % 64 != 0 and groups > 64, (size, offset_elems)
            heads.append(head)
            tails.append(n - head - groups * per_group)
        assert heads[0] == 0 and heads[1] > 0 and max(tails) > 0, (size, heads, tails)
    assert lr.TINY[0] * lr.TINY[1] * lr.TINY[2] < 16


def test_the_sparse_fixture_hides_whole_leaves():
    c = lr.case("sparse_hidden")
    d, a, _ = lr.classified("sparse_hidden")
    sp = devmed.leaf_rule(d, a)
    nz, ny, nx = c.scalar.shape
    full = ((nz + 7) // 8) * ((ny + 7) // 8) * ((nx + 7) // 8)
    hidden = sum(((b[0].stop - b[0].start + 7) // 8) * ((b[1].stop - b[1].start) // 8) * ((b[2].stop - b[2].start + 7) // 8)
                 for b in lr.HIDDEN_BOXES)
    assert sp.leaf_density.shape[0] == full - hidden and hidden == 6
    assert sp.leaf_albedo is not None and c.labels[0, 0, 0] == lr.HIDDEN
    assert tuple(np.float32(v) for v in sp.albedo_bg[:3]) == tuple(c.table[lr.HIDDEN, 0, :3])
    one = devmed.leaf_rule(*lr.classified("sparse_one_colour")[:2])
    assert one.leaf_albedo is None and 0 < one.leaf_density.shape[0] < full
    # voxel 0 under another label: that row's colour at voxel 0's scalar is the background
    d1, a1, _ = lr.classified("sparse_voxel0_row1")
    assert a1[0, 0, 0].tobytes() != a[0, 0, 0].tobytes()
    assert devmed.leaf_rule(d1, a1).leaf_density.shape[0] == full   # the hidden colour now differs from it


def test_the_overflow_cases_reach_their_entry(cvr):
    for name, ch in (("overflow_density", None), ("overflow_colour", 1), ("overflow_density_sparse", None),
                     ("overflow_colour_sparse", 1)):
        c = lr.case(name)
        d, a, _ = lr.host(name)
        v = d if ch is None else a[..., ch]
        assert (v >= 65520).any() and (c.labels[v >= 65520] == 3).all(), name


def test_the_scale_cases_cross_one_trip(cvr):
    """A raised cap fails here and never silently shrinks what tests/test_gpu_labels.py covers."""
    g = bs.geo()
    z, y, x = lr.scale_dense_shape()
    n = z * y * x
    per_trip = g["scan_grid"] * 4 * 64      # 16-byte groups one trip of k_labeled's body loop takes
    for head in (0, 15):                    # the tensor at its allocation's start and one byte in
        groups = (n - head) // 16
        assert per_trip + 64 <= groups < 2 * per_trip, (groups, per_trip)
        assert (n - head - groups * 16) + head > 0
    c = lr.case("scale_sparse_u8")
    assert c.scalar.shape == bs.sparse_shape()
    exists = int(bs.sparse_exists().sum())
    assert exists * 512 > g["stream_grid"] * 256            # k_gather_leaves' second trip
    lz, ly, lx = bs.sparse_leaf_dims()
    assert lx > g["leaf_run_leaves"] and lz * ly * lx > 4 * g["scan_tile"]   # a second x run; > 4 scan tiles
