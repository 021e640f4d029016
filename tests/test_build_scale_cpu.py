"""The media of tests/build_scale.py against the launch geometry the library reports (no GPU).

Every case must cross the threshold it is named for by at least one wave of work, by the caps
cvr_debug_build_geometry reports: a changed cap fails here and never silently shrinks what
tests/test_gpu_build_scale.py covers.  The plants lie in the trip they claim, sparse_4m's leaves
are the intended ones by the numpy leaf rule, and at these sizes the library's host statements of
both transfer functions return the bits of the numpy restatements."""
import ctypes as C

import numpy as np
import pytest

import bounds_model as bm
import build_scale as bs
import devmed

WAVE = 64


def trips(items, per_trip):
    return -(-items // per_trip)


# ---------------------------------------------------------------- geometry --
def test_build_geometry_fills_what_it_says(cvr):
    out = (C.c_uint32 * 16)(*([0xDEADBEEF] * 16))
    assert cvr.load().cvr_debug_build_geometry(out) == 0
    assert out[15] == 14 and out[14] == 0 and all(v not in (0, 0xDEADBEEF) for v in out[:14]), list(out)
    g = cvr.build_geometry()
    assert list(g.values()) == list(out[:14])
    assert g["scan_tile"] % 256 == 0 and g["leaf_run_voxels"] == 8 * g["leaf_run_leaves"]
    assert g["scan_sums_chunk"] == 1024  # one workgroup's size: k_scan_sums takes one sum per work-item
    assert cvr.load().cvr_debug_build_geometry(None) < 0


def test_copy_medium_fails_cleanly_without_a_context(cvr):
    lib = cvr.load()
    lib.cvr_last_error.restype = C.c_char_p
    need = C.c_size_t(123)
    assert lib.cvr_debug_copy_medium(None, 0, None, 0, C.byref(need)) < 0
    assert lib.cvr_last_error(None)
    buf = (C.c_uint8 * 16)()
    assert lib.cvr_debug_copy_medium(None, 0, buf, 16, None) < 0
    assert len(cvr.MEDIUM_ARRAYS) == 11


# ------------------------------------------------------------------- dense --
def test_dense_2m_crosses_every_threshold_it_names():
    g = bs.geo()
    z, y, x = bs.dense_shape()
    n = z * y * x
    per_trip = g["scan_grid"] * 256
    assert n // 4 >= per_trip + WAVE and n % 4 != 0      # k_scan_density: a second float4 trip, a tail
    assert trips(n // 4, per_trip) == 2
    assert trips(n, per_trip) >= 5                       # k_scan_albedo
    half = g["to_half_grid"] * 256
    assert trips(4 * n, half) > 4 and trips(n, half) == 2  # k_to_half: albedo, density
    assert trips(n, g["stream_grid"] * 256) == 2         # k_fill_albedo
    assert all(v % 2 == 1 for v in (z, y, x))


def test_dense_2m_plants_lie_where_they_claim():
    g = bs.geo()
    p = bs.dense_plants()
    per_trip = g["scan_grid"] * 256
    n4 = p.n // 4
    assert p.trip2_first // 4 == per_trip and p.trip2_first % 4 == 0   # float4 index: trip 2, workgroup 0, lane 0
    assert p.last_float4 // 4 == n4 - 1 >= per_trip
    assert p.tail >= 4 * n4                                             # the scalar tail
    for where in ("trip2_first", "tail"):
        d = bs.dense_with_maximum(where).reshape(-1)
        at = getattr(p, where)
        assert d[at] == bs.PEAK == np.nanmax(d) and np.isnan(d).sum() == 1 and np.nanmin(d) == -9.0
        assert abs(int(np.nonzero(np.isnan(d))[0][0]) - at) == 1
    d, small, value = bs.dense_overflow("two_trips")
    hot = np.nonzero(np.abs(d.reshape(-1)) >= 65520)[0]
    assert len(hot) == 2 and hot[0] == small and d.reshape(-1)[small] == value
    # the named (smaller) index: first trip, a workgroup launched late; the larger: workgroup 0's second trip
    assert (hot[0] // 4) // 256 >= g["scan_grid"] - 64 and hot[0] // 4 < per_trip
    assert (hot[1] // 4 - per_trip) // 256 == 0
    d, at, value = bs.dense_overflow("last_trip")
    hot = np.nonzero(np.abs(d.reshape(-1)) >= 65520)[0]
    assert list(hot) == [at] and at // 4 >= per_trip
    for kind, differs in (("uniform", 0), ("last_voxel", 1), ("round_apart", 1), ("round_together", 1)):
        a, fmt, want = bs.uniform_albedo(kind)
        flat = a.reshape(-1, 4)
        rows = np.nonzero((flat != flat[0]).any(axis=1))[0]
        assert len(rows) == differs and all(r >= (p.n - 1) // per_trip * per_trip for r in rows), kind


def test_uniform_albedo_plants_round_as_named(cvr):
    for kind in ("round_apart", "round_together"):
        a, fmt, want = bs.uniform_albedo(kind)
        halves = np.unique(cvr.half_round(np.unique(a[..., :3])))
        assert fmt == 1 and len(np.unique(a[..., :3])) == 2 and len(halves) == (1 if want else 2), kind


# ------------------------------------------------------------------ scalar --
@pytest.mark.parametrize("name", ["scalar_u8_8m", "scalar_u16_4m", "scalar_i16_4m", "scalar_f32_512k"])
def test_scalar_case_crosses_its_threshold(name):
    g = bs.geo()
    c = bs.case(name)
    n, size = c.scalar.size, c.scalar.dtype.itemsize
    assert c.scalar.shape == bs.scalar_shape(name) and all(v % 2 == 1 for v in c.scalar.shape)
    if size == 4:
        assert n >= g["scan_grid"] * 256 + WAVE          # the one-voxel-per-lane loop's second trip
        return
    V = 16 // size
    for head in (0, bs.HEAD[name]):                        # aligned, and one element into the allocation
        groups = (n - head) // V
        assert groups >= g["scan_grid"] * 256 + WAVE, (name, head)
        assert head + (n - head - groups * V) > 0 or head == 0
    assert bs.HEAD[name] == 16 // size - 1
    assert len(c.table) == 64 and not c.ceil
    if name == "scalar_i16_4m":
        assert (c.scalar < 0).mean() > 0.3


# ---------------------------------------------------------------- gradient --
def test_gradient_cases_give_more_tasks_than_workgroups():
    g = bs.geo()
    nz, ny, nx = bs.gradient_shape("gradient_u16_4m")
    tasks, grid = bs.gradient_tasks((nz, ny, nx))
    assert grid == g["gradient_tasks"] and grid % 8 == 0 and tasks >= grid + ny   # a second trip, under the XCD turn
    assert WAVE < nx < 256 and nx % WAVE                                          # a wave boundary inside the row
    assert nz % g["gradient_z"] == 4
    nz, ny, nx = bs.gradient_shape("gradient_u16_x3")
    tasks, grid = bs.gradient_tasks((nz, ny, nx))
    assert -(-nx // 256) == 3 and -(-nz // g["gradient_z"]) == 3 and tasks == grid + 1 < g["gradient_tasks"]
    for name in bs.GRADIENT_CASES:
        c = bs.case(name)
        assert c.scalar.shape == bs.gradient_shape(name) and c.table.shape == (8, 32, 4)
        assert len(set(c.spacing)) == 3


# ------------------------------------------------------------------ sparse --
def test_sparse_4m_geometry():
    g = bs.geo()
    lz, ly, lx = bs.sparse_leaf_dims()
    nz, ny, nx = bs.sparse_shape()
    tile = g["scan_tile"]
    assert (lz, ly, lx) == tuple(-(-v // 8) for v in (nz, ny, nx))
    assert lz * ly * lx >= 4 * tile + WAVE                       # more than four scan tiles
    assert nx > g["leaf_run_voxels"] and lx == g["leaf_run_leaves"] + 1 and nx % 8 == 5
    e = bs.sparse_exists()
    stored = int(e.sum())
    assert stored > 4096 and stored * 512 >= g["stream_grid"] * 256 + WAVE   # k_gather_leaves' second trip
    assert 0.5 < stored / e.size < 0.7
    assert not e[2 * tile:3 * tile].any()                         # a whole tile without a leaf
    assert not e[tile + 768:tile + 1024].any() and e[tile:tile + 768].any() and e[tile + 1024:2 * tile].any()
    assert e[tile - 1] and e[tile] and e[2 * tile - 1] and e[-1] and e[3 * tile:].any()


@pytest.mark.parametrize("name", ["sparse_4m", "sparse_4m_u8", "sparse_4m_u16g"])
def test_sparse_4m_leaves_are_the_intended_ones(name):
    """By the numpy leaf rule over the case's (classified) arrays."""
    sp = bs.leaves(name)
    e = bs.sparse_exists()
    got = (sp.table != devmed.NO_LEAF).reshape(-1)
    assert np.array_equal(got, e), np.nonzero(got != e)[0][:10]
    assert sp.leaf_albedo is not None and sp.leaf_density.shape[0] == int(e.sum())
    # slots number the leaves in index order
    assert np.array_equal(sp.table.reshape(-1)[got], np.arange(int(e.sum()), dtype=np.uint32))
    if name == "sparse_4m":
        d = bs.classified(name)[0]
        assert np.isnan(d).sum() == 1 and (np.signbit(d) & (d == 0)).sum() == 1
    # some super-brick of the mask is clear, some leaf has no cell leaf
    cl = bm.cell_leaves(sp.table)
    assert 0 < int(cl.sum()) < sp.table.size


def test_sparse_gradient_voxels_read_into_absent_leaves():
    """Some classified voxel of a stored leaf has a stencil neighbour in a leaf that is not stored."""
    c = bs.case("sparse_4m_u16g")
    stored = bs._leaf_mask(bs.sparse_exists())
    live = (c.scalar != 0) & stored
    assert (live[:, :, 1:] & ~stored[:, :, :-1]).any() and (live[:-1] & ~stored[1:]).any()


# ---------------------------------------------------- the host statements ---
@pytest.mark.parametrize("name", bs.SCALAR_CASES + bs.GRADIENT_CASES + ("sparse_4m_u8", "sparse_4m_u16g"))
def test_host_statement_equals_numpy_at_full_size(cvr, name):
    """cvr_classify_host / cvr_classify_gradient_host return the numpy restatement's bits."""
    d, a = bs.host_classified(cvr, name)
    wd, wa, md = bs.classified(name)
    assert d.tobytes() == wd.tobytes(), name
    assert a.tobytes() == wa.tobytes(), name
    assert md > 0
