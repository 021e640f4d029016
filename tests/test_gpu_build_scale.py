"""The medium build kernels past one pass of their grids, judged on the stored arrays.

The media are tests/build_scale.py's: each is the smallest ragged grid that makes one kernel of
cvr_medium_build.hip loop over its capped grid (the crossings are asserted on the CPU, from the
caps the library reports, in tests/test_build_scale_cpu.py).  Per case and storage format two
contexts are built, H by the host upload of the reference arrays (cvr_set_medium, or
cvr_set_medium_sparse on the numpy leaf rule's leaves) and D by the device call under test, and:

  - every stored array of D, read back with cvr_debug_copy_medium, equals the reference byte for
    byte (a NaN of the reference may be any NaN): dense density and albedo; sparse leaf table,
    leaf density and leaf albedo pools with their padding voxels;
  - every stored array of D equals H's byte for byte, cells, bounds, brick words, cell-leaf slots
    and mask included, which kernels shared by both paths build; the cell-leaf count, slots and
    the mask also match tests/bounds_model.py;
  - cvr_medium_info, cvr_medium_layout, the 4096-path records and the counters are equal
    (assert_same_state), and for one format per source the records match the oracle over the
    reference grid.

The paths of a 4096-path launch touch a sliver of these grids; the read-back is what sees a store
kernel that skips or misplaces the voxels of its second trip."""
import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import bounds_model as bm
import build_scale as bs
import devmed
import media
from test_gpu_device_medium import (DEV, INVALID, STATE, assert_cell_leaves_and_mask, assert_records_equal,
                                    assert_same_state, device_dense, host_dense, new_ctx, ready, records, refusal,
                                    tensors)

pytestmark = pytest.mark.gpu

DENSE_ARRAYS = ("density", "albedo", "cells", "bounds")
SPARSE_ARRAYS = ("leaf_table", "leaf_density", "leaf_albedo", "cell_slots", "sparse_cells", "brick_words", "mask")


# ----------------------------------------------------------------- helpers --
def close(*ctxs):
    for c in ctxs:
        c.close()


def arrays(cvr, ctx):
    return {k: ctx.debug_medium_array(k) for k in cvr.MEDIUM_ARRAYS}


def stored(cvr, a, fmt):
    """A reference array as format fmt stores it."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    return cvr.half_round(a).astype(np.float16) if fmt else a  # (half values convert exactly)


def assert_stored(got, want, what):
    assert got is not None and got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() == want.tobytes():
        return
    bits = np.uint16 if got.dtype == np.float16 else np.uint32
    mism = np.nonzero((got.view(bits) != want.view(bits)) & ~(np.isnan(got) & np.isnan(want)))[0]
    assert mism.size == 0, (f"{what}: {mism.size} of {got.size} stored values differ from the reference, first at "
                            f"{mism[:4]}: {got[mism[:4]]} != {want[mism[:4]]}, last at {mism[-1]}")


def assert_same_arrays(cvr, host, dev, what, expect):
    """Every array of the two contexts, byte for byte; `expect`: the arrays the medium must have."""
    h, d = arrays(cvr, host), arrays(cvr, dev)
    for k in cvr.MEDIUM_ARRAYS:
        assert (d[k] is not None) == (h[k] is not None) == (k in expect), f"{what}: array {k}"
        if d[k] is None:
            continue
        assert d[k].dtype == h[k].dtype and d[k].shape == h[k].shape, f"{what}: array {k}"
        if d[k].tobytes() != h[k].tobytes():
            bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[d[k].dtype.itemsize]
            mism = np.nonzero(d[k].view(bits) != h[k].view(bits))[0]
            raise AssertionError(f"{what}: {k}: {mism.size} of {d[k].size} entries differ between the device build "
                                 f"and the host upload, first at {mism[:4]}, last at {mism[-1]}")
    return d


def check_dense(cvr, host, dev, d, a, fmt, what, ref=None):
    got = arrays(cvr, dev)
    assert_stored(got["density"], stored(cvr, d, fmt), what + ": density")
    assert_stored(got["albedo"], stored(cvr, a, fmt), what + ": albedo")
    assert_same_arrays(cvr, host, dev, what, DENSE_ARRAYS)
    lay = assert_same_state(host, dev, what, ref)
    assert lay["sparse"] == 0, what
    return lay


def host_leaves(cvr, sp, md, fmt, opts=()):
    ctx = new_ctx(cvr, fmt, opts)
    desc, keep = media.sparse_desc(cvr, sp.res, sp.table, sp.leaf_density, sp.leaf_albedo, sp.albedo_bg, md)
    ctx.set_medium_sparse(desc)
    return ready(cvr, ctx)


def check_sparse(cvr, host, dev, sp, fmt, what, ref=None):
    n_leaves = sp.leaf_density.shape[0]
    assert dev.medium_layout().n_leaves == n_leaves, what
    got = arrays(cvr, dev)
    mism = np.nonzero(got["leaf_table"] != sp.table.reshape(-1))[0]
    assert mism.size == 0, f"{what}: leaf table: {mism.size} entries differ from the leaf rule's, first at {mism[:4]}"
    assert_stored(got["leaf_density"], stored(cvr, sp.leaf_density, fmt), what + ": leaf density pool")
    if sp.leaf_albedo is not None:
        assert_stored(got["leaf_albedo"], stored(cvr, sp.leaf_albedo, fmt), what + ": leaf albedo pool")
    expect = [k for k in SPARSE_ARRAYS if k != "leaf_albedo" or sp.leaf_albedo is not None]
    assert_same_arrays(cvr, host, dev, what, expect)
    lay = assert_same_state(host, dev, what, ref)
    assert lay["sparse"] == 1 and lay["n_leaves"] == n_leaves, what
    bg = stored(cvr, np.array(sp.albedo_bg[:3], np.float32), fmt).astype(np.float32)
    assert lay["albedo_bg"] == [float(v) for v in bg], what
    for ctx in (host, dev):
        assert_cell_leaves_and_mask(cvr, ctx, sp.table, (), what)
    # the cell-leaf slots: 0 without a cell leaf, else 1 + the number of cell leaves before it
    cl = bm.cell_leaves(sp.table).reshape(-1)
    want = np.where(cl, np.cumsum(cl), 0).astype(np.uint32)
    assert np.array_equal(got["cell_slots"], want), what + ": cell-leaf slots"
    assert got["mask"].tolist() == lay["mask"], what
    assert got["sparse_cells"].size == lay["n_cell_leaves"] * 512 * 8
    return lay


def offset_tensor(s):
    """The field on the device, starting one element into its allocation."""
    s = np.ascontiguousarray(s)
    off = s.dtype.itemsize
    raw = torch.from_numpy(s.view(np.uint8).reshape(-1)).to(DEV)
    buf = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device=DEV)
    buf[off:off + raw.numel()] = raw
    t = buf[off:off + raw.numel()].view(getattr(torch, s.dtype.name)).view(s.shape)
    assert t.data_ptr() % 16 == off and t.is_contiguous()
    return t


def device_classified(cvr, name, fmt, offset=False):
    """Context D of a classified case: set_medium_scalar or set_medium_gradient, majorant found on the device."""
    c = bs.case(name)
    ctx = new_ctx(cvr, fmt)
    t = offset_tensor(c.scalar) if offset else torch.from_numpy(np.ascontiguousarray(c.scalar)).to(DEV)
    common = dict(lo=c.lo, hi=c.hi, sparse=c.sparse, box_min=c.box_min, box_max=c.box_max, scale=c.scale,
                  max_density=None)
    if bs.is_gradient(name):
        ctx.set_medium_gradient(t, c.table, glo=c.glo, ghi=c.ghi, spacing=c.spacing, **common)
    else:
        ctx.set_medium_scalar(t, c.table, ceil=c.ceil, density_u=c.density_u, **common)
    del t
    return ready(cvr, ctx)


def oracle_of(name, fmt):
    c = bs.case(name)
    d, a, md = bs.classified(name)
    return devmed.oracle_records(d, a, md, fmt, c.box_min, c.box_max, c.scale)


# ------------------------------------------------------------ dense arrays --
@pytest.mark.parametrize("fmt", [0, 1])
def test_dense_2m_arrays(cvr, oracle_mod, fmt):
    d, a, md = bs.dense_base()
    m = media.Dense(d, a, md, (-0.5,) * 3, (0.5,) * 3, media.SCALE)
    host, dev = host_dense(cvr, m, fmt), device_dense(cvr, m, fmt)
    lay = check_dense(cvr, host, dev, d, a, fmt, f"dense_2m format {fmt}",
                      devmed.oracle_records(d, a, md, fmt) if fmt == 0 else None)
    assert lay["albedo_uniform"] == 0
    close(host, dev)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("where", ["trip2_first", "tail"])
def test_dense_2m_majorant_is_the_planted_maximum(cvr, where, fmt):
    """The maximum at the first voxel of k_scan_density's second trip, or in its scalar tail, a NaN
    and a larger negative value beside it."""
    d, a = bs.dense_with_maximum(where), bs.dense_base()[1]
    m = media.Dense(d, a, bs.PEAK, (-0.5,) * 3, (0.5,) * 3, media.SCALE)
    host, dev = host_dense(cvr, m, fmt), device_dense(cvr, m, fmt, max_density=None)
    assert dev.medium_info().max_density_eff == devmed.md_eff(bs.PEAK) == bs.PEAK
    check_dense(cvr, host, dev, d, a, fmt, f"dense_2m maximum at {where} format {fmt}")
    close(host, dev)


@pytest.mark.parametrize("kind", ["two_trips", "last_trip"])
def test_dense_2m_half_overflow_names_the_smallest_index(cvr, kind):
    d, at, value = bs.dense_overflow(kind)
    a, md = bs.dense_base()[1:]
    host, dev = new_ctx(cvr, 1), new_ctx(cvr, 1)
    desc, keep = cvr.medium_from_arrays(d, a, (-0.5,) * 3, (0.5,) * 3, media.SCALE, md)
    hc, ht = refusal(cvr, lambda: host.set_medium(desc))
    td, ta = tensors(d, a)
    dc, dt = refusal(cvr, lambda: dev.set_medium_device(td, ta, scale=media.SCALE, max_density=md))
    assert (dc, dt) == (hc, ht) and dc == INVALID, (dt, ht)
    assert f"density value {value:g} at index {at} " in dt, dt
    # an albedo value, in k_scan_albedo's last trip, is named once the density is in range
    d2, a2 = bs.dense_base()[0], a.copy()
    a2.reshape(-1, 4)[-3, 1] = np.float32(-65536.0)
    ta, = tensors(a2)
    td, = tensors(d2)
    dc, dt = refusal(cvr, lambda: dev.set_medium_device(td, ta, scale=media.SCALE, max_density=md))
    assert dc == INVALID and f"albedo value -65536 at index {4 * (d2.size - 3) + 1} " in dt, dt
    close(host, dev)


@pytest.mark.parametrize("kind", ["uniform", "last_voxel", "round_apart", "round_together"])
def test_dense_2m_uniform_flag_follows_the_last_trip(cvr, kind):
    d, _, md = bs.dense_base()
    a, fmt, want = bs.uniform_albedo(kind)
    m = media.Dense(d, a, md, (-0.5,) * 3, (0.5,) * 3, media.SCALE)
    host, dev = host_dense(cvr, m, fmt), device_dense(cvr, m, fmt)
    lay = check_dense(cvr, host, dev, d, a, fmt, f"dense_2m albedo {kind}")
    assert lay["albedo_uniform"] == want, kind
    close(host, dev)


@pytest.mark.parametrize("fmt", [0, 1])
def test_dense_2m_const_albedo_fills_every_voxel(cvr, fmt):
    d, _, md = bs.dense_base()
    const = (0.9, 0.55, 0.3, 0.75)
    a = np.empty(d.shape + (4,), np.float32)
    a[:] = np.array(const, np.float32)
    m = media.Dense(d, a, md, (-0.5,) * 3, (0.5,) * 3, media.SCALE)
    # (with the uniform-albedo instance off the launches read the filled grid itself)
    off = ((cvr.OPT_UNIFORM_ALBEDO, 0),)
    host, dev = host_dense(cvr, m, fmt, off), device_dense(cvr, m, fmt, off, const_albedo=const)
    check_dense(cvr, host, dev, d, a, fmt, f"dense_2m const albedo format {fmt}")
    close(host, dev)


# ------------------------------------------------- classified, dense media --
CLASSIFIED = [(name, fmt, offset) for name in bs.SCALAR_CASES + bs.GRADIENT_CASES for fmt in (0, 1)
              for offset in ((False, True) if name in bs.HEAD else (False,))]
ORACLE_FORMAT = {"scalar_u8_8m": 1, "scalar_u16_4m": 0, "scalar_i16_4m": 1, "scalar_f32_512k": 0,
                 "scalar_u8_8m_ceil": 0, "gradient_u16_4m": 0, "gradient_u16_x3": 1}


@pytest.mark.parametrize("name,fmt,offset", CLASSIFIED)
def test_classified_dense(cvr, oracle_mod, name, fmt, offset):
    c = bs.case(name)
    d, a, md = bs.classified(name)
    m = media.Dense(d, a, md, c.box_min, c.box_max, c.scale)
    host, dev = host_dense(cvr, m, fmt), device_classified(cvr, name, fmt, offset)
    ref = oracle_of(name, fmt) if ORACLE_FORMAT[name] == fmt and not offset else None
    check_dense(cvr, host, dev, d, a, fmt, f"{name} format {fmt} offset {offset}", ref)
    assert dev.medium_info().max_density_eff == (devmed.md_eff(md) if fmt else np.float32(md))
    close(host, dev)


# ------------------------------------------------------------------ sparse --
def sparse_pair(cvr, name, fmt):
    d, a, md = bs.classified(name)
    sp = bs.leaves(name)
    host = host_leaves(cvr, sp, md, fmt)
    if name == "sparse_4m":
        dev = new_ctx(cvr, fmt)
        td, ta = tensors(d, a)
        dev.set_medium_device(td, ta, sparse=True, scale=media.SCALE, max_density=md)
        del td, ta
        ready(cvr, dev)
    else:
        dev = device_classified(cvr, name, fmt)
    return host, dev, sp


@pytest.mark.parametrize("name,fmt", [(n, f) for n in ("sparse_4m", "sparse_4m_u8", "sparse_4m_u16g") for f in (0, 1)])
def test_sparse_4m(cvr, oracle_mod, name, fmt):
    host, dev, sp = sparse_pair(cvr, name, fmt)
    d, a, md = bs.classified(name)
    ref = devmed.oracle_records(d, a, md, fmt) if fmt == (name == "sparse_4m_u8") else None
    lay = check_sparse(cvr, host, dev, sp, fmt, f"{name} format {fmt}", ref)
    assert lay["n_leaves"] == int(bs.sparse_exists().sum()) > 4096
    assert lay["n_cell_leaves"] - 1 < sp.table.size   # some leaf has no cell leaf
    close(host, dev)


# --------------------------------------------------------------- lifecycle --
def test_dense_sparse_dense_on_one_context_at_scale(cvr):
    d, a, md = bs.dense_base()
    m = media.Dense(d, a, md, (-0.5,) * 3, (0.5,) * 3, media.SCALE)
    dev = device_dense(cvr, m)
    first, first_arrays = records(dev), arrays(cvr, dev)
    assert_stored(first_arrays["density"], stored(cvr, d, 0), "dense")
    D, A, smd = bs.sparse_arrays()
    sp = bs.leaves("sparse_4m")
    td, ta = tensors(D, A)
    dev.set_medium_device(td, ta, sparse=True, scale=media.SCALE, max_density=smd)
    got = arrays(cvr, dev)
    assert all(got[k] is None for k in DENSE_ARRAYS) and all(got[k] is not None for k in SPARSE_ARRAYS)
    assert np.array_equal(got["leaf_table"], sp.table.reshape(-1))
    assert_stored(got["leaf_density"], stored(cvr, sp.leaf_density, 0), "dense -> sparse: leaf density pool")
    assert_stored(got["leaf_albedo"], stored(cvr, sp.leaf_albedo, 0), "dense -> sparse: leaf albedo pool")
    td, ta = tensors(d, a)
    dev.set_medium_device(td, ta, scale=media.SCALE, max_density=md)
    del td, ta
    again = arrays(cvr, dev)
    for k in cvr.MEDIUM_ARRAYS:
        assert (again[k] is None) == (first_arrays[k] is None), k
        assert again[k] is None or again[k].tobytes() == first_arrays[k].tobytes(), k
    assert records(dev).tobytes() == first.tobytes()
    dev.close()


# ------------------------------------------- the read-back at a known size --
@pytest.mark.parametrize("fmt", [0, 1])
def test_read_back_returns_the_inputs_of_small_media(cvr, fmt):
    """random40 and sparse_small, whose contents the suite already knows; a shared medium gives
    the source's arrays."""
    m = media.random40()
    host, dev = host_dense(cvr, m, fmt), device_dense(cvr, m, fmt)
    check_dense(cvr, host, dev, m.density, m.albedo, fmt, f"random40 format {fmt}")
    n = m.density.size
    got = arrays(cvr, dev)
    assert got["density"].size == n and got["albedo"].size == 4 * n and got["cells"].size == 8 * n
    assert got["bounds"].dtype == np.uint8 and got["bounds"][-1] == 255
    other = new_ctx(cvr, fmt)
    other.share_medium(dev)
    assert_same_arrays(cvr, dev, other, "shared dense medium", DENSE_ARRAYS)
    close(host, other)
    D, A, md = devmed.sparse_grid("sparse_small", True)
    sp = devmed.leaf_rule(D, A)
    host = host_leaves(cvr, sp, md, fmt)
    td, ta = tensors(D, A)
    dev.set_medium_device(td, ta, sparse=True, scale=media.SCALE, max_density=md)
    check_sparse(cvr, host, ready(cvr, dev), sp, fmt, f"sparse_small format {fmt}")
    other = new_ctx(cvr, fmt)
    other.share_medium(dev)
    assert_same_arrays(cvr, dev, other, "shared sparse medium", SPARSE_ARRAYS)
    close(host, dev, other)


def test_read_back_sizes_and_refusals(cvr):
    import ctypes as C
    lib = cvr.load()
    ctx = new_ctx(cvr)
    need = C.c_size_t(7)
    assert lib.cvr_debug_copy_medium(ctx._h, 0, None, 0, C.byref(need)) == STATE and need.value == 0
    m = media.random40()
    desc, keep = cvr.medium_from_arrays(m.density, m.albedo, m.box_min, m.box_max, m.scale, m.max_density)
    ctx.set_option(cvr.OPT_BOUNDS, 0)
    ctx.set_medium(desc)
    n = m.density.size
    buf = np.full(n, 3.0, np.float32)
    assert lib.cvr_debug_copy_medium(ctx._h, 0, buf.ctypes.data, 4 * n - 1, C.byref(need)) == INVALID
    assert need.value == 4 * n and (buf == 3.0).all()       # too small: the size is told, nothing is copied
    assert lib.cvr_debug_copy_medium(ctx._h, 0, buf.ctypes.data, 4 * n, C.byref(need)) == 0
    assert buf.tobytes() == m.density.tobytes()
    for which in (3, 4, 10):                                  # bounds off, a sparse array, the mask: absent
        need.value = 7
        assert lib.cvr_debug_copy_medium(ctx._h, which, None, 0, C.byref(need)) == 0 and need.value == 0
    assert lib.cvr_debug_copy_medium(ctx._h, 11, None, 0, C.byref(need)) == INVALID
    assert ctx.debug_medium_array("bounds") is None
    ctx.close()
