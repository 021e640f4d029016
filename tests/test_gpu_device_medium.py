"""Media built from device memory (cvr_set_medium_device) against the host uploads.

Each case builds two contexts over the same numpy arrays, one through cvr_set_medium or
cvr_set_medium_sparse (the host upload) and one through cvr_set_medium_device from torch
tensors, and asserts the same state: cvr_medium_info, cvr_medium_layout (leaves, cell leaves,
mask words, uniform albedo), the records of 4096 paths of the production launch bit for bit,
and the launch's counters with `fetches`.  The records are also compared with the oracle over
the dense grid, so the pair cannot agree on a wrong medium.  The two sparse uploads share the
cell-leaf and mask kernels, so each one's count, mask shift and mask words are also pinned to
tests/bounds_model.py (assert_cell_leaves_and_mask).  With CVR_DEVMED_SPARSE the host
side uploads the leaves that the numpy statement of the leaf rule (tests/devmed.py, checked on
the CPU in tests/test_device_medium_cpu.py) makes of the grid."""
import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import devmed
import media
from parity_util import COUNTERS

pytestmark = pytest.mark.gpu

INVALID, STATE, UNSUPPORTED = -1, -3, -5
DEV = "cuda:0"


# ----------------------------------------------------------------- helpers --
def tensors(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV) for a in arrays]


def new_ctx(cvr, fmt=0, opts=()):
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
    for k, v in opts:
        ctx.set_option(k, v)
    return ctx


def ready(cvr, ctx):
    iv, r2v = cvr.default_camera(*devmed.TILE)
    ctx.set_camera(iv, r2v, devmed.TILE)
    ctx.init()
    ctx.set_resolution(*devmed.TILE)
    ctx.set_offset(0, 0)
    ctx.set_iterations(devmed.ITERS)
    return ctx


def host_dense(cvr, m, fmt=0, opts=()):
    ctx = new_ctx(cvr, fmt, opts)
    desc, keep = cvr.medium_from_arrays(m.density, m.albedo, m.box_min, m.box_max, m.scale, m.max_density)
    ctx.set_medium(desc)
    return ready(cvr, ctx)


def device_dense(cvr, m, fmt=0, opts=(), const_albedo=None, max_density="given"):
    ctx = new_ctx(cvr, fmt, opts)
    d, a = tensors(m.density, None if const_albedo is not None else m.albedo)
    ctx.set_medium_device(d, a, const_albedo=const_albedo, box_min=m.box_min, box_max=m.box_max, scale=m.scale,
                          max_density=m.max_density if max_density == "given" else max_density)
    del d, a  # the context keeps its own copy
    return ready(cvr, ctx)


def host_sparse(cvr, D, A, md, fmt=0, opts=()):
    sp = devmed.leaf_rule(D, A)
    ctx = new_ctx(cvr, fmt, opts)
    desc, keep = media.sparse_desc(cvr, sp.res, sp.table, sp.leaf_density, sp.leaf_albedo, sp.albedo_bg, md)
    ctx.set_medium_sparse(desc)
    return ready(cvr, ctx), sp


def device_sparse(cvr, D, A, md, fmt=0, opts=(), const_albedo=None):
    ctx = new_ctx(cvr, fmt, opts)
    d, a = tensors(D, None if const_albedo is not None else A)
    ctx.set_medium_device(d, a, const_albedo=const_albedo, sparse=True, scale=media.SCALE, max_density=md)
    del d, a
    return ready(cvr, ctx)


def aim(ctx):
    ctx.set_resolution(*devmed.TILE)
    ctx.set_offset(0, 0)
    ctx.set_iterations(devmed.ITERS)
    ctx.set_seed(devmed.SEED)


def records(ctx):
    aim(ctx)
    ctx.set_path_range(0, devmed.N)
    return ctx.trace_launch(devmed.N)


def counters(ctx):
    aim(ctx)
    ctx.set_path_range(0, devmed.N)
    ctx.clear_output()
    ctx.launch_render()
    st = ctx.stats()
    return {k: getattr(st, k) for k in COUNTERS + ("fetches",)}


def assert_records_equal(g, c, what):
    assert len(g) == len(c) == devmed.N
    for f in ("image_id", "flags", "n_segments"):
        mism = np.nonzero(g[f] != c[f])[0]
        assert mism.size == 0, f"{what}: {f} differs for {mism.size} paths, first {mism[:5]}"
    tb, cb = g["T"].view(np.uint32), c["T"].view(np.uint32)
    both_nan = np.isnan(g["T"]) & np.isnan(c["T"])
    mism = np.nonzero(((tb != cb) & ~both_nan).any(axis=1))[0]
    assert mism.size == 0, f"{what}: T bits differ for {mism.size} paths, first {mism[:5]}"


def assert_same_state(host, dev, what, ref=None):
    """info, layout, records (and the oracle's, when given) and counters of two contexts."""
    hi, di = host.medium_info().as_dict(), dev.medium_info().as_dict()
    assert di == hi, f"{what}: medium_info {di} != {hi}"
    hl, dl = host.medium_layout().as_dict(), dev.medium_layout().as_dict()
    for k in hl:
        assert dl[k] == hl[k], f"{what}: medium_layout.{k}: {dl[k]} != {hl[k]}"
    rh, rd = records(host), records(dev)
    assert rd.tobytes() == rh.tobytes(), f"{what}: the two contexts' records differ"
    if ref is not None:
        assert_records_equal(rd, ref, what + ": device-built against the oracle")
        assert (ref["flags"] & 1).any() and (ref["n_albedo"] > 0).any(), what  # escapes and real collisions
    ch, cd = counters(host), counters(dev)
    assert cd == ch, f"{what}: counters {cd} != {ch}"
    assert cd["paths"] == devmed.N
    return hl


def refusal(cvr, call):
    with pytest.raises(cvr.CvrError) as e:
        call()
    return e.value.code, str(e.value)


def launch_code(cvr, ctx):
    ctx.set_resolution(*devmed.TILE)
    ctx.set_iterations(1)
    ctx.set_path_range(0, devmed.TILE[0] * devmed.TILE[1])
    return refusal(cvr, ctx.launch_render)[0]


# ------------------------------------------------------------------- dense --
@pytest.mark.parametrize("bounds", [0, 2, 3])
@pytest.mark.parametrize("cells", [1, 0])
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("name", ["random40", "staircase", "offgrid"])
def test_dense_equals_host_upload(cvr, oracle_mod, name, fmt, cells, bounds):
    m = media.DENSE_MEDIA[name]()
    opts = ((cvr.OPT_CELLS, cells), (cvr.OPT_BOUNDS, bounds))
    host, dev = host_dense(cvr, m, fmt, opts), device_dense(cvr, m, fmt, opts)
    lay = assert_same_state(host, dev, f"{name} format {fmt} cells {cells} bounds {bounds}",
                            devmed.dense_reference(name, fmt))
    assert lay["sparse"] == 0 and lay["albedo_uniform"] == 0 and lay["brick_shift"] == bounds
    assert (dev.medium_info().cells_bytes > 0) == bool(cells) and (dev.medium_info().bounds_bytes > 0) == bool(bounds)
    host.close()
    dev.close()


# ---------------------------------------------------------- uniform albedo --
def albedo_case(kind):
    """(albedo grid over dense_arrays' density, format, expected albedo_uniform)."""
    d, a, md = media.dense_arrays("max", uniform=True)  # rgb 0.9 everywhere, w 1
    if kind == "w_varies":
        a[..., 3] = np.random.default_rng(5).random(a.shape[:3], dtype=np.float32)
        return a, 0, 1
    if kind == "last_voxel":        # a scan that drops its tail calls this uniform
        a[-1, -1, -1, 1] = np.float32(0.5)
        return a, 0, 0
    if kind == "round_together":    # two fp32 values, one half: 0.9 and its successor -> 0.89990234
        a[3:7, :, :, 0] = np.nextafter(np.float32(0.9), np.float32(1))
        return a, 1, 1
    assert kind == "round_apart"    # 0.9005 -> 0.90039063
    a[5, 6, 7, 2] = np.float32(0.9005)
    return a, 1, 0


@pytest.mark.parametrize("kind", ["w_varies", "last_voxel", "round_together", "round_apart"])
def test_uniform_albedo_detection(cvr, kind):
    d, _, md = media.dense_arrays("max")
    a, fmt, want = albedo_case(kind)
    if kind == "round_together":
        r = cvr.half_round(np.array([0.9, np.nextafter(np.float32(0.9), np.float32(1))], np.float32))
        assert r[0] == r[1] and len(np.unique(a[..., 0])) == 2
    if kind == "round_apart":
        assert len(np.unique(cvr.half_round(a[..., 2]))) == 2
    m = media.Dense(d, a, md, (-0.5,) * 3, (0.5,) * 3, media.SCALE)
    host, dev = host_dense(cvr, m, fmt), device_dense(cvr, m, fmt)
    lay = assert_same_state(host, dev, kind)
    assert lay["albedo_uniform"] == want, kind
    host.close()
    dev.close()


def test_centre_voxel_is_not_uniform(cvr, oracle_mod):
    m = devmed.centre_voxel()
    host, dev = host_dense(cvr, m), device_dense(cvr, m)
    lay = assert_same_state(host, dev, "centre voxel", devmed.dense_reference("centre_voxel", 0))
    assert lay["albedo_uniform"] == 0
    host.close()
    dev.close()


@pytest.mark.parametrize("fmt", [0, 1])
def test_const_albedo_equals_the_filled_grid(cvr, fmt):
    d, _, md = media.dense_arrays("max")
    const = (0.9, 0.55, 0.3, 0.75)
    a = np.empty(d.shape + (4,), np.float32)
    a[:] = np.array(const, np.float32)
    m = media.Dense(d, a, md, (-0.5,) * 3, (0.5,) * 3, media.SCALE)
    ref = devmed.oracle_records(d, a, md, fmt)
    host, dev = host_dense(cvr, m, fmt), device_dense(cvr, m, fmt, const_albedo=const)
    lay = assert_same_state(host, dev, f"const albedo format {fmt}", ref)
    assert lay["albedo_uniform"] == 1
    # with the uniform-albedo instance off, the filled grid itself is read
    off = ((cvr.OPT_UNIFORM_ALBEDO, 0),)
    host2, dev2 = host_dense(cvr, m, fmt, off), device_dense(cvr, m, fmt, off, const_albedo=const)
    lay = assert_same_state(host2, dev2, f"const albedo format {fmt}, grid read", ref)
    assert lay["albedo_uniform"] == 0
    for c in (host, dev, host2, dev2):
        c.close()


# ---------------------------------------------------------------- majorant --
@pytest.mark.parametrize("fmt", [0, 1])
def test_majorant_found_on_the_device(cvr, fmt):
    d, a, _ = media.dense_arrays("max")
    d = d.copy()
    d[7, 3, 11] = np.float32(1.75)     # the maximum, away from either end
    d[2, 2, 2] = np.float32(np.nan)    # ignored
    d[2, 2, 3] = np.float32(-3.0)
    md = float(np.nanmax(d))
    assert md == 1.75
    m = media.Dense(d, a, md, (-0.5,) * 3, (0.5,) * 3, media.SCALE)
    host, dev = host_dense(cvr, m, fmt), device_dense(cvr, m, fmt, max_density=None)
    assert dev.medium_info().max_density_eff == np.float32(md)
    assert_same_state(host, dev, f"majorant format {fmt}")
    host.close()
    dev.close()


def test_density_four_bytes_off_alignment(cvr):
    """A density tensor that starts 4 bytes into its allocation (a view): format 1, so that the
    scan, the conversion and the overflow index all read it."""
    d, a, md = media.dense_arrays("max")
    m = media.Dense(d, a, md, (-0.5,) * 3, (0.5,) * 3, media.SCALE)
    host, dev = host_dense(cvr, m, 1), new_ctx(cvr, 1)
    base = torch.zeros(d.size + 1, dtype=torch.float32, device=DEV)
    base[1:] = torch.from_numpy(d.reshape(-1)).to(DEV)
    td = base[1:].view(d.shape)
    assert td.data_ptr() % 16 == 4 and td.is_contiguous()
    ta, = tensors(a)
    dev.set_medium_device(td, ta, scale=m.scale, max_density=None)
    assert_same_state(host, ready(cvr, dev), "unaligned density")
    base[1 + 1234] = 70000.0
    code, text = refusal(cvr, lambda: dev.set_medium_device(td, ta, scale=m.scale, max_density=md))
    assert code == INVALID and "density value 70000 at index 1234 " in text, text
    host.close()
    dev.close()


def test_majorant_of_an_all_zero_grid(cvr):
    d = np.zeros((5, 6, 7), np.float32)
    d[1, 1, 1] = np.float32(-0.0)
    d[2, 2, 2] = np.float32(-1.0)
    a = np.ones(d.shape + (4,), np.float32)
    m = media.Dense(d, a, 0.0, (-0.5,) * 3, (0.5,) * 3, media.SCALE)
    host, dev = host_dense(cvr, m), device_dense(cvr, m, max_density=None)
    hi, di = host.medium_info().as_dict(), dev.medium_info().as_dict()
    assert di == hi and di["max_density_eff"] == 0.0 and di["bounds_bytes"] == 0
    assert dev.medium_layout().as_dict() == host.medium_layout().as_dict()
    host.close()
    dev.close()


# ----------------------------------------------------------- half overflow --
@pytest.mark.parametrize("kind", ["density_twice", "albedo_only", "both"])
def test_half_overflow_names_what_the_host_names(cvr, kind):
    d, a, md = media.dense_arrays("max")
    d, a = d.copy(), a.copy()
    if kind in ("density_twice", "both"):
        d[8, 2, 5] = np.float32(65520.0)
        d[3, 9, 14] = np.float32(65520.0)   # the smaller flat index
    if kind in ("albedo_only", "both"):
        a[6, 1, 2, 2] = np.float32(-70000.0)
        a[1, 4, 4, 1] = np.float32(65520.0)  # the smaller one
    m = media.Dense(d, a, md, (-0.5,) * 3, (0.5,) * 3, media.SCALE)
    # from a context that renders: the refusal leaves it without a medium
    good = media.random40()
    host, dev = host_dense(cvr, good, 1), device_dense(cvr, good, 1)
    desc, keep = cvr.medium_from_arrays(m.density, m.albedo, m.box_min, m.box_max, m.scale, m.max_density)
    hc, ht = refusal(cvr, lambda: host.set_medium(desc))
    td, ta = tensors(d, a)
    dc, dt = refusal(cvr, lambda: dev.set_medium_device(td, ta, scale=m.scale, max_density=md))
    assert (dc, dt) == (hc, ht) and dc == INVALID
    flat = (3 * 13 + 9) * 19 + 14 if kind != "albedo_only" else ((1 * 13 + 4) * 19 + 4) * 4 + 1
    assert f"at index {flat} " in dt and ("density" if kind != "albedo_only" else "albedo") in dt, dt
    assert launch_code(cvr, dev) == STATE and launch_code(cvr, host) == STATE
    # format 0 takes the same arrays
    dev.set_option(cvr.OPT_MEDIUM_FORMAT, 0)
    dev.set_medium_device(td, ta, scale=m.scale, max_density=md)
    assert dev.medium_info().format == 0
    host.close()
    dev.close()


# ------------------------------------------------------------------ sparse --
def assert_cell_leaves_and_mask(cvr, ctx, table, opts, what):
    """The context's cell-leaf count, mask shift and 64 mask words against tests/bounds_model.py.
    Both uploads count the cell leaves and set the mask's bits with the same kernels, so their
    agreeing proves neither: the model is the independent statement of the rule.  The words are
    packed as MediumParams says: super-brick (sx, sy, sz) = leaf coordinates >> (es - 3) is bit
    sz << (lx + ly) | sy << lx | sx, in word bit >> 5, 2^lx and 2^ly the padded super-brick grid."""
    import bounds_model as bm
    lay = ctx.medium_layout().as_dict()
    assert lay["n_cell_leaves"] == int(bm.cell_leaves(table).sum()) + 1, what
    if dict(opts).get(cvr.OPT_BOUNDS) == 0:  # bounds off: no mask is built
        assert lay["mask_shift"] == 0 and not any(lay["mask"]), what
        return
    # (CVR_OPT_EMPTY_MASK 0 keeps the launches from reading the mask; it is built and reported all the same)
    es, mask = bm.sparse_mask(table)
    assert lay["mask_shift"] == es == bm.mask_shift(table.shape), what
    lx, ly = (max((int(n) - 1).bit_length() - (es - 3), 0) for n in (table.shape[2], table.shape[1]))
    words = [0] * 64
    for sz, sy, sx in zip(*np.nonzero(mask)):
        b = int(sz) << (lx + ly) | int(sy) << lx | int(sx)
        words[b >> 5] |= 1 << (b & 31)
    assert lay["mask"] == words, what


def sparse_case(cvr, name, with_albedo, fmt, opts, ref=True):
    D, A, md = devmed.sparse_grid(name, with_albedo)
    (host, sp), dev = host_sparse(cvr, D, A, md, fmt, opts), device_sparse(cvr, D, A, md, fmt, opts)
    what = f"{name} albedo {with_albedo} format {fmt} options {opts}"
    lay = assert_same_state(host, dev, what, devmed.sparse_reference(name, with_albedo, fmt) if ref else None)
    assert lay["sparse"] == 1 and lay["n_leaves"] == sp.leaf_density.shape[0], what
    assert (dev.medium_info().albedo_bytes > 0) == with_albedo
    assert_cell_leaves_and_mask(cvr, host, sp.table, opts, what + ": host upload")
    assert_cell_leaves_and_mask(cvr, dev, sp.table, opts, what + ": device build")
    host.close()
    dev.close()
    return lay, sp


@pytest.mark.parametrize("emask", [1, 0])
@pytest.mark.parametrize("name,with_albedo,fmt", [("sparse_small", True, 0), ("sparse_small", False, 0),
                                                  ("sparse_small", False, 1), ("sparse_es4", True, 0)])
def test_sparse_equals_host_upload_of_the_rule_s_leaves(cvr, oracle_mod, name, with_albedo, fmt, emask):
    import bounds_model as bm
    lay, sp = sparse_case(cvr, name, with_albedo, fmt, ((cvr.OPT_EMPTY_MASK, emask),))
    # the planted leaves are there (the rule's count is checked on the CPU), and the mask is the model's
    es, mask = bm.sparse_mask(sp.table)
    assert lay["mask_shift"] == es == (4 if name == "sparse_es4" else 3)
    assert any(lay["mask"]) and lay["n_cell_leaves"] > lay["n_leaves"]


@pytest.mark.parametrize("bounds", [1, 2, 3])
@pytest.mark.parametrize("name,fmt", [("sparse_small", 0), ("sparse_small", 1), ("sparse_es4", 0)])
def test_sparse_brick_sizes(cvr, oracle_mod, name, fmt, bounds):
    with_albedo = not fmt
    lay, _ = sparse_case(cvr, name, with_albedo, fmt, ((cvr.OPT_BOUNDS, bounds),))
    assert lay["brick_shift"] == bounds


def test_sparse_const_albedo_and_unbounded(cvr, oracle_mod):
    """CONST_ALBEDO: the constant is the background, leaves by density alone; bounds off: no mask."""
    D, _, md = devmed.sparse_grid("sparse_small", False)
    const = (0.7, 0.55, 0.33, 1.0)
    A = np.empty(D.shape + (4,), np.float32)
    A[:] = np.array(const, np.float32)
    for opts in ((), ((cvr.OPT_BOUNDS, 0),)):
        (host, sp), dev = host_sparse(cvr, D, A, md, 0, opts), device_sparse(cvr, D, None, md, 0, opts, const_albedo=const)
        lay = assert_same_state(host, dev, f"sparse const albedo {opts}", devmed.sparse_reference("sparse_small", False, 0))
        assert lay["albedo_bg"] == [float(np.float32(v)) for v in const[:3]]
        assert any(lay["mask"]) == (not opts)
        for ctx in (host, dev):
            assert_cell_leaves_and_mask(cvr, ctx, sp.table, opts, f"sparse const albedo {opts}")
        host.close()
        dev.close()


def test_host_upload_of_a_table_the_leaf_rule_never_makes(cvr, oracle_mod):
    """cvr_set_medium_sparse allows slots in any order and several entries naming one slot; the
    cell leaves and the mask come from the existence of entries alone.  A ragged 20x12x10 grid
    (3x2x2 leaves), slots in reverse leaf order, two entries sharing slot 0."""
    import bounds_model as bm
    sp = devmed.unusual_table()
    stored = sp.table[sp.table != devmed.NO_LEAF]
    assert sp.table.shape == (2, 2, 3) and (np.diff(stored.astype(np.int64)) <= 0).all()
    assert len(stored) == len(np.unique(stored)) + 1 == sp.leaf_density.shape[0] + 1
    D, A = devmed.densify(sp)
    assert D.shape == (10, 12, 20)
    ref = devmed.oracle_records(D, A, sp.max_density)
    assert (ref["flags"] & 1).any() and (ref["n_albedo"] > 0).any()  # escapes and real collisions
    ctx = new_ctx(cvr)
    desc, keep = media.sparse_desc(cvr, sp.res, sp.table, sp.leaf_density, sp.leaf_albedo, sp.albedo_bg, sp.max_density)
    ctx.set_medium_sparse(desc)
    ready(cvr, ctx)
    assert_records_equal(records(ctx), ref, "unusual table against the oracle")
    assert ctx.medium_layout().n_leaves == sp.leaf_density.shape[0]
    assert_cell_leaves_and_mask(cvr, ctx, sp.table, (), "unusual table")
    assert 1 < ctx.medium_layout().n_cell_leaves - 1 < sp.table.size  # some leaf has no cell leaf
    ctx.close()


def test_host_sparse_refusals_keep_their_order(cvr):
    """Table entry before half overflow, on a context that holds a format-1 medium: the first
    keeps that medium, the second leaves the context without one."""
    sp = media.sparse_small(True)
    ctx = new_ctx(cvr, 1)
    desc, keep = media.sparse_desc(cvr, sp.res, sp.table, sp.leaf_density, sp.leaf_albedo, sp.albedo_bg, sp.max_density)
    ctx.set_medium_sparse(desc)
    ready(cvr, ctx)
    before = records(ctx)
    hot = sp.leaf_density.copy()
    hot[5, 7] = np.float32(1e6)    # pool index 2567: past the first blocks the overflow search tests whole
    hot[7, 3] = np.float32(-7e4)   # a later one, not named
    bad = sp.table.copy()
    bad[sp.table != devmed.NO_LEAF] = hot.shape[0]  # every stored entry one past the pools
    desc, keep = media.sparse_desc(cvr, sp.res, bad, hot, sp.leaf_albedo, sp.albedo_bg, sp.max_density)
    code, text = refusal(cvr, lambda: ctx.set_medium_sparse(desc))
    assert code == INVALID and f"leaf table entry {hot.shape[0]} >= n_leaves {hot.shape[0]}" in text, text
    assert records(ctx).tobytes() == before.tobytes()  # the previous medium still renders
    desc, keep = media.sparse_desc(cvr, sp.res, sp.table, hot, sp.leaf_albedo, sp.albedo_bg, sp.max_density)
    code, text = refusal(cvr, lambda: ctx.set_medium_sparse(desc))
    assert code == INVALID and f"leaf density value 1e+06 at index {5 * 512 + 7} rounds to infinity" in text, text
    assert launch_code(cvr, ctx) == STATE
    ctx.close()


def test_sparse_half_overflow(cvr):
    """The message names the leaf pool's index, as cvr_set_medium_sparse does."""
    D, A, md = devmed.sparse_grid("sparse_small", True)
    D = D.copy()
    D[9, 3, 17] = np.float32(65520.0)    # leaf (2, 0, 1)
    D[2, 9, 1] = np.float32(-65536.0)    # leaf (0, 1, 0): an earlier slot, a larger flat index
    sp = devmed.leaf_rule(D, A)
    host, dev = new_ctx(cvr, 1), new_ctx(cvr, 1)
    desc, keep = media.sparse_desc(cvr, sp.res, sp.table, sp.leaf_density, sp.leaf_albedo, sp.albedo_bg, md)
    hc, ht = refusal(cvr, lambda: host.set_medium_sparse(desc))
    td, ta = tensors(D, A)
    dc, dt = refusal(cvr, lambda: dev.set_medium_device(td, ta, sparse=True, scale=media.SCALE, max_density=md))
    assert (dc, dt) == (hc, ht) and dc == INVALID and "leaf density" in dt and "-65536" in dt
    host.close()
    dev.close()


# --------------------------------------------------------------- lifecycle --
def test_dense_sparse_dense_on_one_context(cvr, oracle_mod):
    m = media.random40()
    D, A, md = devmed.sparse_grid("sparse_small", True)
    dev = device_dense(cvr, m)
    first = records(dev)
    td, ta = tensors(D, A)
    dev.set_medium_device(td, ta, sparse=True, scale=media.SCALE, max_density=md)
    assert dev.medium_layout().sparse == 1
    assert_records_equal(records(dev), devmed.sparse_reference("sparse_small", True, 0), "dense -> sparse")
    td, ta = tensors(m.density, m.albedo)
    dev.set_medium_device(td, ta, box_min=m.box_min, box_max=m.box_max, scale=m.scale, max_density=m.max_density)
    del td, ta
    assert dev.medium_layout().sparse == 0
    again = records(dev)
    assert again.tobytes() == first.tobytes()
    assert_records_equal(again, devmed.dense_reference("random40", 0), "sparse -> dense")
    dev.close()


@pytest.mark.parametrize("sparse", [False, True])
def test_share_medium_from_a_device_built_source(cvr, oracle_mod, sparse):
    if sparse:
        D, A, md = devmed.sparse_grid("sparse_small", True)
        src, ref = device_sparse(cvr, D, A, md), devmed.sparse_reference("sparse_small", True, 0)
    else:
        src, ref = device_dense(cvr, media.random40()), devmed.dense_reference("random40", 0)
    other = new_ctx(cvr)
    other.share_medium(src)
    ready(cvr, other)
    assert other.medium_info().as_dict() == src.medium_info().as_dict()
    assert other.medium_layout().as_dict() == src.medium_layout().as_dict()
    assert_records_equal(records(other), ref, "shared medium")
    other.close()
    src.close()


def test_refused_inside_an_adaptive_session(cvr):
    m = media.random40()
    dev = device_dense(cvr, m)
    before = records(dev)
    d, a = tensors(m.density, m.albedo)
    with dev.adaptive(cvr.AdaptiveDesc(8, 16, 4, -1.0, 0.01)):
        code, text = refusal(cvr, lambda: dev.set_medium_device(d, a, scale=m.scale, max_density=m.max_density))
        assert code == STATE and "adaptive session" in text and "cvr_set_medium_device" in text
    assert records(dev).tobytes() == before.tobytes()
    dev.close()


def test_null_pointers_and_flags(cvr):
    m = media.random40()
    dev = device_dense(cvr, m)
    before = records(dev)
    d, a = tensors(m.density, m.albedo)
    res = m.density.shape[::-1]
    for kw in (dict(density=0, albedo=a), dict(density=d, albedo=0), dict(density=0, const_albedo=(1, 1, 1, 1))):
        for sparse in (False, True):
            code, text = refusal(cvr, lambda: dev.set_medium_device(res=res, sparse=sparse, max_density=1.0, **kw))
            assert code == INVALID and "NULL" in text, text
    lib = cvr.load()
    desc = cvr.DeviceMediumDesc()
    desc.res[:] = res
    desc.flags = 8
    desc.d_density, desc.d_albedo = d.data_ptr(), a.data_ptr()
    assert lib.cvr_set_medium_device(dev._h, desc) == INVALID
    desc.flags = cvr.DEVMED_CONST_ALBEDO   # with an albedo array as well
    assert lib.cvr_set_medium_device(dev._h, desc) == INVALID
    assert records(dev).tobytes() == before.tobytes()  # the previous medium still renders
    dev.close()


SHAPE_REFUSALS = [
    # res, sparse, options, code, a word of the message
    ((0, 4, 4), False, (), INVALID, "empty grid"),
    ((4, 0, 4), True, (), INVALID, "empty grid"),
    ((4096, 4096, 1), False, (), UNSUPPORTED, "2^24"),
    ((1, 4096, 4096), False, (), UNSUPPORTED, "2^24"),
    ((65536, 1, 65536), False, (), INVALID, "2^32"),
    ((2048, 2048, 512), False, (), UNSUPPORTED, "2^31"),
    ((8 * 4096, 8 * 4096, 8), True, (), UNSUPPORTED, "2^24"),
    ((8, 8, 8 * ((1 << 24) + 1)), True, (), UNSUPPORTED, "2^24"),
    ((8 * 65536, 8 * 65536, 8), True, (), INVALID, "2^32"),
    ((8 * 2048, 8 * 2048, 8), True, (("OPT_BOUNDS", 2),), UNSUPPORTED, "2^24"),
]


@pytest.mark.parametrize("row", range(len(SHAPE_REFUSALS)))
def test_shape_refusals_are_the_host_calls(cvr, row):
    """Descriptors without arrays: the shape is judged from res alone, before any pointer."""
    import ctypes as C
    from cudavolumerenderer_amd._lib import SparseMediumDesc
    res, sparse, opts, code, word = SHAPE_REFUSALS[row]
    m = media.random40()
    opts = tuple((getattr(cvr, k), v) for k, v in opts)
    dev, host = device_dense(cvr, m, opts=opts), new_ctx(cvr, opts=opts)
    before = records(dev)
    if sparse:
        hd = SparseMediumDesc()
        hd.res[:] = res
        hd.leaf_dims[:] = [(v + 7) // 8 for v in res]
    else:
        hd = cvr.MediumDesc()
        hd.res[:] = res
    hd.box_min[:], hd.box_max[:] = (-0.5,) * 3, (0.5,) * 3
    hd.scale, hd.max_density, hd.eta = 100.0, 1.0, 1.04
    hc, ht = refusal(cvr, lambda: (host.set_medium_sparse if sparse else host.set_medium)(hd))
    dc, dt = refusal(cvr, lambda: dev.set_medium_device(0, 0, res=res, sparse=sparse, max_density=1.0))
    assert (dc, dt) == (hc, ht) and dc == code and word in dt, (dt, ht)
    assert records(dev).tobytes() == before.tobytes()  # the previous medium still renders
    # one step inside the guard, the call gets to its NULL check
    if code == UNSUPPORTED and not sparse and word == "2^24":
        inside = tuple(v - 1 if v == 4096 else v for v in res)
        dc, dt = refusal(cvr, lambda: dev.set_medium_device(0, 0, res=inside, max_density=1.0))
        assert dc == INVALID and "NULL" in dt
    host.close()
    dev.close()
