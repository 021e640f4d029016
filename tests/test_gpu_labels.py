"""Label volumes classified on the device (cvr_set_medium_labeled) against cvr_set_medium_device.

Each case builds two contexts.  A calls set_medium_labeled on the scalar and label tensors (under a
clip where the case has one).  B calls set_medium_device on the arrays cvr_classify_labels_host
makes of the same fields and table (clipped by tests/clip_ref.py where the case has a clip); those
arrays are compared with the numpy statement of tests/labels_ref.py on the CPU
(tests/test_labels_cpu.py).  The two must be in one state: cvr_medium_info, cvr_medium_layout, every
stored array byte for byte (cvr_debug_copy_medium), the 4096 records of the production launch and
its counters, and A's records are compared with the oracle over the host arrays.  A's label counts
(cvr_medium_label_info) must be the bincount of the kept voxels' label bytes.  There is no
tolerance anywhere.  The media are labels_ref's: labels independent per voxel, a random table per
row, so a wrong row or a label taken from the voxel beside changes stored bits."""
from functools import lru_cache

import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import clip_ref as cr
import devmed
import labels_ref as lr
import transfer_ref as tr
from test_cli_devices import run_cli
from test_gpu_clip import assert_same_arrays
from test_gpu_device_medium import (DEV, INVALID, STATE, assert_same_state, launch_code, new_ctx, ready, records, refusal,
                                    tensors)

pytestmark = pytest.mark.gpu

LABEL_OFFSETS = (0, 1, 2, 3, 4, 7, 8, 15)


# ----------------------------------------------------------------- helpers --
def view_at(a, offset_bytes):
    """The array on the device, starting offset_bytes into a 16-byte aligned allocation."""
    a = np.ascontiguousarray(a)
    raw = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(DEV)
    buf = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device=DEV)
    buf[offset_bytes:offset_bytes + raw.numel()] = raw
    t = buf[offset_bytes:offset_bytes + raw.numel()].view(getattr(torch, a.dtype.name)).view(a.shape)
    assert t.data_ptr() % 16 == offset_bytes and t.is_contiguous()
    return t


def set_labeled(ctx, c, scalar_t, label_t, max_density=None, **kw):
    args = dict(lo=c.lo, hi=c.hi, ceil=c.ceil, density_u=c.density_u, sparse=c.sparse, scale=lr.SCALE,
                max_density=max_density)
    args.update(kw)
    table = args.pop("table", c.table)
    ctx.set_medium_labeled(scalar_t, label_t, table, **args)


def context_a(cvr, c, fmt=0, opts=(), max_density=None, region=None, offsets=(0, 0)):
    ctx = new_ctx(cvr, fmt, opts)
    if region is not None:
        ctx.set_clip(region.lo, region.hi, region.planes)
    set_labeled(ctx, c, view_at(c.scalar, offsets[0] * c.scalar.dtype.itemsize), view_at(c.labels, offsets[1]),
                max_density)
    return ready(cvr, ctx)


def context_b(cvr, d, a, sparse, fmt=0, opts=(), max_density=None):
    ctx = new_ctx(cvr, fmt, opts)
    td, ta = tensors(d, a)
    ctx.set_medium_device(td, ta, sparse=sparse, scale=lr.SCALE, max_density=max_density)
    del td, ta
    return ready(cvr, ctx)


@lru_cache(maxsize=None)
def host_arrays(name, region_name=None):
    """(keep or None, density, albedo) that context B is built from; read-only, shared by the cases."""
    d, a, _ = lr.host(name)
    if region_name is None:
        return None, d, a
    keep, dc, ac = cr.clip(d, a, cr.GPU_REGIONS[region_name])
    for v in (keep, dc, ac):
        v.setflags(write=False)
    return keep, dc, ac


@lru_cache(maxsize=None)
def oracle_ref(name, region_name, fmt):
    _, d, a = host_arrays(name, region_name)
    with np.errstate(invalid="ignore"):
        return devmed.oracle_records(d, a, float(np.nanmax(np.maximum(d, 0))), fmt)


def assert_counts(ctx, c, keep, what):
    m, counts = ctx.medium_label_info()
    lab = c.labels if keep is None else c.labels[keep]
    want = np.bincount(lab.reshape(-1), minlength=256)
    assert m == c.table.shape[0], what
    assert (counts == want).all(), f"{what}: label counts differ at bytes {np.nonzero(counts != want)[0][:8]}"
    assert int(counts.sum()) == ctx.medium_clip_info()[1] == (c.labels.size if keep is None else int(keep.sum())), what


def pair(cvr, name, fmt, opts=(), max_density=None, region_name=None, offsets=(0, 0), oracle=True):
    c = lr.case(name)
    keep, d, a = host_arrays(name, region_name)
    what = f"{name} format {fmt} clip {region_name} offsets {offsets}"
    region = cr.GPU_REGIONS[region_name] if region_name else None
    ctx_a = context_a(cvr, c, fmt, opts, max_density, region, offsets)
    ctx_b = context_b(cvr, d, a, c.sparse, fmt, opts, max_density)
    lay = assert_same_state(ctx_b, ctx_a, what, oracle_ref(name, region_name, fmt) if oracle else None)
    assert lay["sparse"] == int(c.sparse), what
    assert_same_arrays(cvr, ctx_b, ctx_a, what)
    assert_counts(ctx_a, c, keep, what)
    assert ctx_b.medium_label_info()[0] == 0 and not ctx_b.medium_label_info()[1].any(), what
    return ctx_a, ctx_b, lay


def close(*ctxs):
    for c in ctxs:
        c.close()


def full_leaves(c):
    nz, ny, nx = c.scalar.shape
    return ((nz + 7) // 8) * ((ny + 7) // 8) * ((nx + 7) // 8)


# ------------------------------------------------- hand-round and alignment --
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("scalar_offset", [0, 1])
@pytest.mark.parametrize("name", ["ragged_u8", "ragged_u16", "ragged_i16", "ragged_f32"])
def test_dense_at_every_relative_misalignment(cvr, oracle_mod, name, scalar_offset, fmt):
    """The scalar view at 0 and 1 elements, the label view at each of 8 byte offsets: the first
    pair in full, the others on the same context B by info, arrays and counts."""
    a, b, lay = pair(cvr, name, fmt, offsets=(scalar_offset, LABEL_OFFSETS[0]))
    assert lay["albedo_uniform"] == 0
    assert a.medium_info().max_density_eff == b.medium_info().max_density_eff   # CVR_DEVMED_MAX_DENSITY
    c = lr.case(name)
    for off in LABEL_OFFSETS[1:]:
        what = f"{name} format {fmt} scalar at {scalar_offset} labels at {off}"
        set_labeled(a, c, view_at(c.scalar, scalar_offset * c.scalar.dtype.itemsize), view_at(c.labels, off))
        assert a.medium_info().as_dict() == b.medium_info().as_dict(), what
        assert_same_arrays(cvr, b, a, what)
        assert_counts(a, c, None, what)
    close(a, b)


@pytest.mark.parametrize("fmt", [0, 1])
def test_a_grid_smaller_than_one_group(cvr, fmt):
    """12 voxels of u8: head only, at every label offset."""
    c = lr.case("tiny_u8")
    _, d, al = host_arrays("tiny_u8")
    b = context_b(cvr, d, al, False, fmt)
    a = new_ctx(cvr, fmt)
    for so in (0, 1, 5):
        for off in LABEL_OFFSETS:
            set_labeled(a, c, view_at(c.scalar, so), view_at(c.labels, off))
            what = f"tiny format {fmt} scalar at {so} labels at {off}"
            assert a.medium_info().as_dict() == b.medium_info().as_dict(), what
            assert_same_arrays(cvr, b, a, what)
            assert_counts(a, c, None, what)
    close(a, b)


def test_ceil_mode(cvr, oracle_mod):
    a, b, _ = pair(cvr, "ragged_u8_ceil", 0, offsets=(1, 3))
    close(a, b)


# ------------------------------------------------------------------ sparse --
@pytest.mark.parametrize("fmt", [0, 1])
def test_hiding_a_segment_sheds_its_leaves(cvr, oracle_mod, fmt):
    a, b, lay = pair(cvr, "sparse_hidden", fmt, offsets=(1, 5))
    c = lr.case("sparse_hidden")
    want = devmed.leaf_rule(*lr.host("sparse_hidden")[:2]).leaf_density.shape[0]
    assert lay["n_leaves"] == a.medium_layout().n_leaves == want == full_leaves(c) - 6
    assert a.medium_info().albedo_bytes > 0
    colour = c.table[lr.HIDDEN, 0, :3]
    assert lay["albedo_bg"] == [float(v) for v in (cvr.half_round(colour) if fmt else colour)]
    close(a, b)


@pytest.mark.parametrize("fmt", [0, 1])
def test_sparse_one_colour_has_no_albedo_pool(cvr, oracle_mod, fmt):
    a, b, lay = pair(cvr, "sparse_one_colour", fmt)
    assert a.medium_info().albedo_bytes == b.medium_info().albedo_bytes == 0
    assert 0 < lay["n_leaves"] < full_leaves(lr.case("sparse_one_colour"))
    close(a, b)


@pytest.mark.parametrize("fmt", [0, 1])
def test_voxel_0_s_label_selects_the_background_row(cvr, oracle_mod, fmt):
    a, b, lay = pair(cvr, "sparse_voxel0_row1", fmt, offsets=(0, 2))
    bg = lr.host("sparse_voxel0_row1")[1][0, 0, 0, :3]
    assert lay["albedo_bg"] == [float(v) for v in (cvr.half_round(bg) if fmt else bg)]
    assert lay["albedo_bg"] != [float(v) for v in lr.case("sparse_voxel0_row1").table[lr.HIDDEN, 0, :3]]
    assert lay["n_leaves"] == full_leaves(lr.case("sparse_voxel0_row1"))   # the hidden colour differs from it
    close(a, b)


# ------------------------------------------------------------------- m = 1 --
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("name", ["m1", "m1_sparse"])
def test_one_row_equals_set_medium_scalar(cvr, oracle_mod, name, fmt):
    c = lr.case(name)
    a = context_a(cvr, c, fmt, offsets=(0, 3))
    s = new_ctx(cvr, fmt)
    t = view_at(c.scalar, 0)
    s.set_medium_scalar(t, c.table[0], lo=c.lo, hi=c.hi, sparse=c.sparse, scale=lr.SCALE)
    ready(cvr, s)
    lay = assert_same_state(s, a, f"{name} format {fmt}", oracle_ref(name, None, fmt))
    assert lay["sparse"] == int(c.sparse)
    assert_same_arrays(cvr, s, a, f"{name} format {fmt}")
    assert a.medium_label_info()[0] == 1 and s.medium_label_info()[0] == 0
    close(a, s)


# -------------------------------------------------------------- full table --
@pytest.mark.parametrize("region_name", [None, "crop"])
def test_a_full_lds_table(cvr, oracle_mod, region_name):
    """16 x 256 entries beside the counters, labels over all 256 bytes: dense and clipped dense."""
    a, b, _ = pair(cvr, "full_table", 0, region_name=region_name, offsets=(1, 7))
    assert (a.medium_label_info()[1] > 0).sum() > (200 if region_name is None else 100)
    close(a, b)


# ---------------------------------------------------------- derived values --
@pytest.mark.parametrize("fmt", [0, 1])
def test_given_majorant(cvr, oracle_mod, fmt):
    a, b, _ = pair(cvr, "ragged_u16", fmt, max_density=1.5, oracle=False)
    assert a.medium_info().max_density_eff == b.medium_info().max_density_eff == 1.5
    close(a, b)


@pytest.mark.parametrize("fmt", [0, 1])
def test_uniform_rgb_rows(cvr, oracle_mod, fmt):
    a, b, lay = pair(cvr, "uniform_rgb", fmt)
    assert lay["albedo_uniform"] == 1 and a.medium_layout().albedo_uniform == 1
    a2, b2, lay = pair(cvr, "uniform_rgb", fmt, ((cvr.OPT_UNIFORM_ALBEDO, 0),))
    assert lay["albedo_uniform"] == 0
    close(a, b, a2, b2)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("what", ["density", "colour"])
def test_half_overflow_under_one_label(cvr, what, sparse):
    """A row-3 entry of 70000 that only voxels of label 3 reach: code, message and index are the
    device call's on the host arrays."""
    name = f"overflow_{what}" + ("_sparse" if sparse else "")
    c = lr.case(name)
    _, d, al = host_arrays(name)
    good = lr.case("ragged_u16")
    a = context_a(cvr, good, 1)
    b = context_b(cvr, *host_arrays("ragged_u16")[1:], False, 1)
    td, ta = tensors(d, al)
    bc, bt = refusal(cvr, lambda: b.set_medium_device(td, ta, sparse=c.sparse, scale=lr.SCALE, max_density=None))
    st, lt = view_at(c.scalar, 2), view_at(c.labels, 5)
    ac, at = refusal(cvr, lambda: set_labeled(a, c, st, lt))
    assert (ac, at) == (bc, bt) and ac == INVALID and "rounds to infinity" in at, (at, bt)
    assert ("density" if what == "density" else "albedo") in at, at
    assert launch_code(cvr, a) == STATE and launch_code(cvr, b) == STATE  # left without a medium
    a.set_option(cvr.OPT_MEDIUM_FORMAT, 0)
    set_labeled(a, c, st, lt)
    assert a.medium_info().format == 0
    close(a, b)


# -------------------------------------------------------------------- clip --
@pytest.mark.parametrize("name,region_name,fmt", [("ragged_u8", "crop", 0), ("ragged_u16", "oblique", 1),
                                                  ("ragged_f32", "crop", 1), ("sparse_hidden", "crop", 1),
                                                  ("sparse_hidden", "oblique", 0)])
def test_clipped_build_equals_the_build_on_clipped_host_arrays(cvr, oracle_mod, name, region_name, fmt):
    assert lr.RES[:2] == cr.RES[:2] and lr.RES[2] >= cr.RES[2]   # the regions were made for this x, y extent
    a, b, _ = pair(cvr, name, fmt, region_name=region_name, offsets=(1, 3))
    keep = host_arrays(name, region_name)[0]
    assert 0 < keep.sum() < keep.size
    close(a, b)


# ------------------------------------------------------------------ counts --
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_counts_of_a_volume_that_is_mostly_one_label(cvr, sparse):
    c = lr.case("mostly_one")._replace(sparse=sparse)
    assert (c.labels == 1).mean() > 0.98
    a = new_ctx(cvr, 0)
    set_labeled(a, c, view_at(c.scalar, 0), view_at(c.labels, 1))
    assert_counts(a, c, None, f"mostly one label, sparse {sparse}")
    assert (a.medium_label_info()[1] == lr.host("mostly_one")[2]).all()
    a.close()


# ------------------------------------------------------------ second trips --
@pytest.mark.parametrize("region_name", [None, "crop"])
def test_dense_past_one_trip(cvr, region_name):
    """More 16-byte groups than one trip of the dense pair's grid takes, one byte into the
    allocation; the crop (x 3..30, y 9..17, z 2..) leaves whole runs of the first trip and of the
    second outside it."""
    c = lr.case("scale_dense_u8")
    d, al, _ = lr.host("scale_dense_u8")
    keep = None
    if region_name:
        keep, d, al = cr.clip(d, al, cr.GPU_REGIONS[region_name])
    a = context_a(cvr, c, 0, region=cr.GPU_REGIONS[region_name] if region_name else None, offsets=(1, 6))
    b = context_b(cvr, d, al, False, 0)
    what = f"scale_dense_u8 clip {region_name}"
    assert a.medium_info().as_dict() == b.medium_info().as_dict(), what
    assert_same_arrays(cvr, b, a, what)
    assert_counts(a, c, keep, what)
    assert records(a).tobytes() == records(b).tobytes(), what
    close(a, b)


def test_sparse_past_one_trip(cvr):
    c = lr.case("scale_sparse_u8")
    d, al, _ = lr.host("scale_sparse_u8")
    a = context_a(cvr, c, 0, offsets=(1, 2))
    b = context_b(cvr, d, al, True, 0)
    assert a.medium_info().as_dict() == b.medium_info().as_dict()
    assert a.medium_layout().as_dict() == b.medium_layout().as_dict()
    assert_same_arrays(cvr, b, a, "scale_sparse_u8")
    assert_counts(a, c, None, "scale_sparse_u8")
    assert records(a).tobytes() == records(b).tobytes()
    close(a, b)


# --------------------------------------------------------------- lifecycle --
@pytest.mark.parametrize("fmt", [0, 1])
def test_a_second_table_on_the_same_two_tensors(cvr, oracle_mod, fmt):
    first, second = lr.case("ragged_u8"), lr.case("uniform_rgb")     # the same fields, two tables
    assert first.scalar.tobytes() == second.scalar.tobytes() and first.labels.tobytes() == second.labels.tobytes()
    st, lt = view_at(first.scalar, 0), view_at(first.labels, 9)
    a = new_ctx(cvr, fmt)
    set_labeled(a, first, st, lt)
    ready(cvr, a)
    set_labeled(a, second, st, lt)
    b = context_b(cvr, *host_arrays("uniform_rgb")[1:], False, fmt)
    lay = assert_same_state(b, a, f"second table format {fmt}", oracle_ref("uniform_rgb", None, fmt))
    assert lay["albedo_uniform"] == 1
    assert_same_arrays(cvr, b, a, "second table")
    # sparse over dense, then dense again
    sp = lr.case("sparse_hidden")
    set_labeled(a, sp, view_at(sp.scalar, 0), view_at(sp.labels, 0))
    assert a.medium_layout().sparse == 1 and a.medium_label_info()[0] == 4
    set_labeled(a, second, st, lt)
    assert_same_arrays(cvr, b, a, "sparse -> dense")
    assert_counts(a, second, None, "sparse -> dense")
    close(a, b)


def test_invalid_descriptors_keep_the_previous_medium_in_the_header_s_order(cvr):
    c = lr.case("ragged_u16")
    a = context_a(cvr, c)
    before = records(a)
    st, lt = view_at(c.scalar, 0), view_at(c.labels, 0)
    lib = cvr.load()
    tab = np.ascontiguousarray(c.table)
    host = np.ascontiguousarray(c.scalar)
    nx, ny, nz = lr.RES

    def refused(res=(nx, ny, nz), flags=0, scalar_type=cvr.SCALAR_U16, n=7, m=5, tflags=0, reserved=0,
                table=tab.ctypes.data, d_scalar=st.data_ptr(), d_labels=lt.data_ptr(), lo=c.lo, hi=c.hi):
        d = cvr.LabeledMediumDesc()
        d.res[:] = res
        d.flags, d.d_scalar, d.d_labels, d.scalar_type = flags, d_scalar, d_labels, scalar_type
        d.transfer = cvr.LabelTransferDesc(n, m, tflags, reserved, table, lo, hi)
        d.box_min[:], d.box_max[:], d.scale, d.eta = (-0.5,) * 3, (0.5,) * 3, lr.SCALE, 1.04
        assert lib.cvr_set_medium_labeled(a._h, d) == INVALID
        assert records(a).tobytes() == before.tobytes()       # the previous medium still renders
        return lib.cvr_last_error(a._h).decode()

    # each call is wrong in its own item and in every later one
    later = dict(d_labels=host.ctypes.data)                                                   # 8
    assert "d_labels is not device-accessible" in refused(**later)
    later.update(d_scalar=st.data_ptr() + 1)                                                  # 7: misaligned
    assert "aligned" in refused(**later)
    assert "d_scalar is not device-accessible" in refused(**dict(later, d_scalar=host.ctypes.data))
    later.update(lo=2.0, hi=1.0)                                                              # 6
    assert "hi > lo" in refused(**later)
    for null in (dict(table=None), dict(d_scalar=None), dict(d_labels=None)):                 # 5
        assert "NULL" in refused(**dict(later, **null)), null
    later.update(table=None)
    for bad in (dict(tflags=4), dict(reserved=1)):                                            # 4
        assert "cvr_label_transfer_desc" in refused(**dict(later, **bad)), bad
    later.update(tflags=4, reserved=1)
    for n, m in ((1, 5), (7, 0), (7, 257), (17, 256)):                                        # 3
        assert "n * m" in refused(**dict(later, n=n, m=m)), (n, m)
    later.update(n=1, m=0)
    assert "scalar_type" in refused(**dict(later, scalar_type=4))                             # 2
    for flags in (cvr.DEVMED_CONST_ALBEDO, 8):
        assert "flags" in refused(**dict(later, flags=flags)), flags
    later.update(flags=8, scalar_type=4)
    assert "empty grid" in refused(**dict(later, res=(0, 4, 4)))                              # 1
    a.close()


def test_refused_inside_an_adaptive_session(cvr):
    c = lr.case("ragged_u16")
    a = context_a(cvr, c)
    before = records(a)
    st, lt = view_at(c.scalar, 0), view_at(c.labels, 0)
    with a.adaptive(cvr.AdaptiveDesc(8, 16, 4, -1.0, 0.01)):
        code, text = refusal(cvr, lambda: set_labeled(a, c, st, lt))
        assert code == STATE and "adaptive session" in text and "cvr_set_medium_labeled" in text
    assert records(a).tobytes() == before.tobytes()
    a.close()


def test_label_info_of_other_builds_and_of_a_shared_medium(cvr):
    c = lr.case("ragged_u8")
    fresh = new_ctx(cvr, 0)
    code, _ = refusal(cvr, fresh.medium_label_info)
    assert code == STATE                                                         # no medium
    a = context_a(cvr, c, offsets=(0, 1))
    other = new_ctx(cvr, 0)
    other.share_medium(a)
    assert_counts(other, c, None, "shared medium")                               # the source's counts
    # built by another call, on the same context: m = 0 and no counts
    a.set_medium_scalar(view_at(c.scalar, 0), c.table[0], lo=c.lo, hi=c.hi, scale=lr.SCALE)
    m, counts = a.medium_label_info()
    assert m == 0 and not counts.any()
    assert_counts(other, c, None, "shared medium after the source rebuilt")
    fresh.share_medium(a)
    assert fresh.medium_label_info()[0] == 0
    close(other, fresh, a)


def test_timing_groups_are_reported(cvr):
    c = lr.case("ragged_u16")
    a = new_ctx(cvr, 1, ((cvr.OPT_TIMING, 1),))
    set_labeled(a, c, view_at(c.scalar, 0), view_at(c.labels, 0))
    ms = a.device_medium_ms()
    assert ms[0] > 0 and ms[1] == 0 and ms[4] > 0 and ms[5] > 0, ms  # one scan, the store, cells + bounds
    sp = lr.case("sparse_hidden")
    set_labeled(a, sp, view_at(sp.scalar, 0), view_at(sp.labels, 0))
    ms = a.device_medium_ms()
    assert ms[0] == 0 and ms[2] > 0 and ms[3] > 0 and ms[4] > 0, ms     # sparse: no separate scan
    a.close()


# --------------------------------------------------------------------- CLI --
def _write_cli_inputs(tmp_path, table, labels):
    tf = tmp_path / "labels_tf.txt"
    m, n = table.shape[:2]
    tf.write_text("# n m, then r g b density\n%d %d\n" % (n, m) +
                  "".join("%.9g %.9g %.9g %.9g\n" % tuple(row) for row in table.reshape(-1, 4)))
    lab = tmp_path / "labels.raw"
    lab.write_bytes(labels.tobytes())
    return tf, lab


@pytest.mark.parametrize("mode", ["linear", "ceil"])
def test_cli_transfer_labels(cvr, tmp_path, mode):
    """cvr --synthetic bucky --transfer-labels: the image of a Python session making the same calls,
    bit for bit.  One iteration: a pixel is then one path's value, and no order of a sum over
    iterations (which two runs of one program need not share) enters the comparison."""
    W, H, iters = 64, 64, 1
    table = lr.tables(3, 7, 900)
    scene = cvr.Scene.synthetic("bucky")
    raw = np.frombuffer(scene.raw_bytes, np.uint8).reshape(32, 32, 32).copy()
    labels = lr.labels_iid(raw.shape, 3, 901)
    tf, lab = _write_cli_inputs(tmp_path, table, labels)
    img, out = run_cli(tmp_path, "labels", "--synthetic", "bucky", "--transfer-labels", str(tf), "--labels", str(lab),
                       "--transfer-mode", mode, "--field-stats", "-r", str(W), str(H), "-i", str(iters))
    md = scene.medium
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_medium_labeled(torch.from_numpy(raw).to(DEV), torch.from_numpy(labels).to(DEV), table, lo=0.0,
                           hi=float(raw.max()), ceil=(mode == "ceil"), box_min=tuple(md.box_min),
                           box_max=tuple(md.box_max), scale=md.scale, g=md.g, roughness=tuple(md.roughness), eta=md.eta)
    iv, r2v = scene.camera(W, H)
    ctx.set_camera(iv, r2v, (W, H))
    ctx.init()
    ref, _ = ctx.render_image(W, H, (1, 1), iters)
    scene.close()
    ctx.close()
    assert ref[..., :3].max() > 0
    assert np.ascontiguousarray(img, np.float32).tobytes() == np.ascontiguousarray(ref[..., :3], np.float32).tobytes()
    text = out if isinstance(out, str) else str(out)
    for b, k in enumerate(np.bincount(labels.reshape(-1), minlength=256)):
        if k:
            assert f"label {b}: {k}" in text, (b, k)


def test_cli_transfer_labels_errors(cvr, tmp_path):
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.abspath(cvr.__file__)), "cvr")
    table = lr.tables(2, 7, 910)
    labels = lr.labels_iid((32, 32, 32), 2, 911)
    tf, lab = _write_cli_inputs(tmp_path, table, labels)
    short = tmp_path / "short.raw"
    short.write_bytes(labels.tobytes()[:-1])
    one = tmp_path / "tf1.txt"
    one.write_text("".join("%.9g %.9g %.9g %.9g\n" % tuple(row) for row in tr.table7()))
    out = str(tmp_path / "o.ppm")
    for args, word in ((["--transfer-labels", str(tf), "--labels", str(short)], "labels"),
                       (["--transfer-labels", str(tf), "--labels", str(lab), "--transfer", str(one)], "--transfer"),
                       (["--transfer-labels", str(tf)], "--labels")):
        p = subprocess.run([cli, "--synthetic", "bucky", "-r", "32", "32", "-i", "1", "-o", out] + args,
                           capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and "[ConfigParser] Error:" in p.stderr + p.stdout and word in p.stderr + p.stdout, \
            (args, p.stderr)
