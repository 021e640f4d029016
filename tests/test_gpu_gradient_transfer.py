"""Scalar volumes classified on the device by value and gradient magnitude (cvr_set_medium_gradient)
against cvr_set_medium_device.

The scheme is tests/test_gpu_transfer.py's.  Each case builds two contexts: A through
set_medium_device on tensors of classify_gradient_host's output, B through set_medium_gradient on
the scalar tensor.  It asserts what assert_same_state of tests/test_gpu_device_medium.py asserts
(cvr_medium_info, cvr_medium_layout, the 4096 records of the production launch as equal bytes, the
launch's counters with `fetches`) and compares B's records with the oracle over the numpy
restatement's arrays, whose records show escapes and real collisions (checked on the CPU too,
tests/test_gradient_transfer_cpu.py).  The media are tests/gradient_ref.py's; the classified arrays
and the oracle's records are computed once."""

import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import devmed
import gradient_ref as gr
from parity_util import assert_pixels_close
from test_cli_devices import run_cli
from test_gpu_device_medium import (DEV, INVALID, STATE, assert_records_equal, assert_same_state, launch_code,
                                    new_ctx, ready, records, refusal, tensors)

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------- helpers --
def scalar_tensor(c, name=None):
    """The case's scalar field on the device; OFFSET cases start that many bytes into a larger buffer."""
    s = np.ascontiguousarray(c.scalar)
    off = gr.OFFSET.get(name, 0)
    if not off:
        return torch.from_numpy(s).to(DEV)
    raw = torch.from_numpy(s.view(np.uint8).reshape(-1).copy()).to(DEV)
    buf = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device=DEV)
    buf[off:off + raw.numel()] = raw
    t = buf[off:off + raw.numel()].view(getattr(torch, s.dtype.name)).view(s.shape)
    assert t.data_ptr() % 16 == off and t.is_contiguous()
    return t


def host_classified(cvr, c):
    return cvr.classify_gradient_host(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)[:2]


def context_a(cvr, c, fmt=0, opts=(), max_density=None):
    d, a = host_classified(cvr, c)
    ctx = new_ctx(cvr, fmt, opts)
    td, ta = tensors(d, a)
    ctx.set_medium_device(td, ta, sparse=c.sparse, box_min=c.box_min, box_max=c.box_max, scale=c.scale,
                          max_density=max_density)
    del td, ta
    return ready(cvr, ctx)


def set_gradient(ctx, c, t, max_density=None, **kw):
    args = dict(lo=c.lo, hi=c.hi, glo=c.glo, ghi=c.ghi, spacing=c.spacing, sparse=c.sparse, box_min=c.box_min,
                box_max=c.box_max, scale=c.scale, max_density=max_density)
    args.update(kw)
    table = args.pop("table", c.table)
    ctx.set_medium_gradient(t, table, **args)


def context_b(cvr, c, fmt=0, opts=(), max_density=None, name=None):
    ctx = new_ctx(cvr, fmt, opts)
    t = scalar_tensor(c, name)
    set_gradient(ctx, c, t, max_density)
    del t  # the context does not keep the field
    return ready(cvr, ctx)


def pair(cvr, name, fmt, opts=(), max_density=None):
    c = gr.case(name)
    a, b = context_a(cvr, c, fmt, opts, max_density), context_b(cvr, c, fmt, opts, max_density, name)
    lay = assert_same_state(a, b, f"{name} format {fmt} options {opts}", gr.reference(name, fmt))
    return a, b, lay


def close(*ctxs):
    for c in ctxs:
        c.close()


# ------------------------------------------------------------------- dense --
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("name", ["random40_u8", "random40_u16", "random40_i16", "offgrid_f32", "thin523_u8",
                                  "thin523_u16", "two_planes_u16", "one_plane_u8", "one_column_u8", "nonfinite_f32",
                                  "full_lds_u16"])
def test_dense_equals_the_device_call_on_classified_arrays(cvr, oracle_mod, name, fmt):
    """one_plane_u8 and one_column_u8 have an axis of one voxel, which cvr_set_medium accepts."""
    a, b, lay = pair(cvr, name, fmt)
    assert lay["sparse"] == 0 and lay["albedo_uniform"] == 0
    assert b.medium_info().max_density_eff == a.medium_info().max_density_eff  # CVR_DEVMED_MAX_DENSITY
    close(a, b)


def test_host_output_is_the_numpy_statement_s(cvr):
    """What context A is built from is what the oracle's reference is built from."""
    for name in ("random40_u16", "nonfinite_f32", "halo"):
        d, a = host_classified(cvr, gr.case(name))
        wd, wa, _ = gr.classified(name)
        assert d.tobytes() == wd.tobytes() and a.tobytes() == wa.tobytes(), name


@pytest.mark.parametrize("fmt", [0, 1])
def test_given_majorant(cvr, oracle_mod, fmt):
    c = gr.case("random40_u16")
    a, b = context_a(cvr, c, fmt, max_density=1.5), context_b(cvr, c, fmt, max_density=1.5)
    assert_same_state(a, b, f"given majorant format {fmt}")
    assert b.medium_info().max_density_eff == a.medium_info().max_density_eff == 1.5
    close(a, b)


@pytest.mark.parametrize("fmt", [0, 1])
def test_one_colour_table_dense_is_uniform(cvr, oracle_mod, fmt):
    c = gr.case("random40_u8")
    table = c.table.copy()
    table[..., :3] = np.array([0.9, 0.55, 0.3], np.float32)
    c = c._replace(table=table)
    a, b = context_a(cvr, c, fmt), context_b(cvr, c, fmt)
    lay = assert_same_state(a, b, f"one colour, dense, format {fmt}")
    assert lay["albedo_uniform"] == 1 and b.medium_layout().albedo_uniform == 1
    close(a, b)


# ------------------------------------------------------------------ sparse --
def full_leaves(c):
    nz, ny, nx = c.scalar.shape
    return ((nz + 7) // 8) * ((ny + 7) // 8) * ((nx + 7) // 8)


@pytest.mark.parametrize("fmt", [0, 1])
def test_sparse_halo_leaves_exist_through_the_gradient(cvr, oracle_mod, fmt):
    """One non-zero voxel at (7, 7, 7): its leaf and the three leaves of its +x, +y, +z neighbours,
    which hold zero scalars only (asserted on the CPU), and no other of the 27."""
    a, b, lay = pair(cvr, "halo", fmt)
    c = gr.case("halo")
    want = devmed.leaf_rule(*gr.classified("halo")[:2]).leaf_density.shape[0]
    assert want == 4 and full_leaves(c) == 27
    assert lay["sparse"] == 1 and lay["n_leaves"] == b.medium_layout().n_leaves == want
    assert b.medium_info().albedo_bytes > 0
    bg = cvr.half_round(c.table[0, 0, :3]) if fmt else c.table[0, 0, :3]  # entry (0, 0)'s colour, as stored
    assert lay["albedo_bg"] == [float(v) for v in bg]
    close(a, b)


@pytest.mark.parametrize("fmt", [0, 1])
def test_sparse_one_colour_has_no_albedo_pool(cvr, oracle_mod, fmt):
    a, b, lay = pair(cvr, "halo_one_colour", fmt)
    assert a.medium_info().albedo_bytes == b.medium_info().albedo_bytes == 0
    assert lay["n_leaves"] == 4
    close(a, b)


@pytest.mark.parametrize("fmt", [0, 1])
def test_sparse_positive_densities_make_every_leaf(cvr, oracle_mod, fmt):
    a, b, lay = pair(cvr, "halo_positive", fmt)
    assert lay["n_leaves"] == b.medium_layout().n_leaves == full_leaves(gr.case("halo_positive")) == 27
    close(a, b)


@pytest.mark.parametrize("fmt", [0, 1])
def test_sparse_random_field(cvr, oracle_mod, fmt):
    """The ragged random grid built sparse: every leaf kernel reads neighbours across leaf borders."""
    c = gr.case("random40_u16")._replace(sparse=True)
    a, b = context_a(cvr, c, fmt), context_b(cvr, c, fmt)
    lay = assert_same_state(a, b, f"random40_u16 sparse format {fmt}", gr.reference("random40_u16", fmt))
    assert lay["sparse"] == 1 and lay["n_leaves"] == full_leaves(c)
    close(a, b)


# ----------------------------------------------------------- half overflow --
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("what", ["density", "colour"])
def test_half_overflow_names_what_the_device_call_names(cvr, what, sparse):
    """A table entry of 70000 that some voxels reach: B's code and message are A's."""
    c = gr.case("halo" if sparse else "random40_u8")
    table = c.table.copy()
    # a whole table cell, so that voxels inside it interpolate between four entries of 70000: the
    # halo's neighbours of the one voxel have value 0 and a large gradient, cell (3, 0)
    cell = (slice(3, 5), slice(0, 2)) if sparse else (slice(3, 5), slice(4, 6))
    table[cell + (3 if what == "density" else 1,)] = np.float32(70000.0)
    c = c._replace(table=table)
    d, al = host_classified(cvr, c)
    assert ((d if what == "density" else al[..., 1]) >= 65520).any()
    good = gr.case("random40_u16")
    a, b = context_a(cvr, good, 1), context_b(cvr, good, 1)
    td, ta = tensors(d, al)
    ac, at = refusal(cvr, lambda: a.set_medium_device(td, ta, sparse=c.sparse, scale=c.scale, max_density=None))
    t = scalar_tensor(c)
    bc, bt = refusal(cvr, lambda: set_gradient(b, c, t))
    assert (bc, bt) == (ac, at) and bc == INVALID and "rounds to infinity" in bt, (bt, at)
    assert ("density" if what == "density" else "albedo") in bt, bt
    assert launch_code(cvr, a) == STATE and launch_code(cvr, b) == STATE  # left without a medium
    # format 0 takes the same field and table
    b.set_option(cvr.OPT_MEDIUM_FORMAT, 0)
    set_gradient(b, c, t)
    assert b.medium_info().format == 0
    close(a, b)


# ---------------------------------------------------------------- refusals --
def test_invalid_descriptors_keep_the_previous_medium(cvr):
    c = gr.case("random40_u16")
    b = context_b(cvr, c)
    before = records(b)
    t = scalar_tensor(c)
    res = c.scalar.shape[::-1]
    u16 = cvr.SCALAR_U16
    host = np.ascontiguousarray(c.scalar)
    nan, inf = float("nan"), float("inf")
    bad = [
        ("empty grid", lambda: set_gradient(b, c, t.data_ptr(), res=(0, 4, 4), scalar_type=u16)),            # 1
        ("scalar_type", lambda: set_gradient(b, c, t.data_ptr(), res=res, scalar_type=4)),                   # 2
        ("n * m", lambda: set_gradient(b, c, t, table=c.table[:, :1])),                                      # 3
        ("n * m", lambda: set_gradient(b, c, t, table=c.table[:1])),
        ("n * m", lambda: set_gradient(b, c, t, table=np.zeros((33, 128, 4), np.float32))),
        ("NULL", lambda: set_gradient(b, c, 0, res=res, scalar_type=u16)),                                   # 5
        ("hi > lo", lambda: set_gradient(b, c, t, lo=5.0, hi=5.0)),                                          # 6
        ("hi > lo", lambda: set_gradient(b, c, t, lo=6.0, hi=5.0)),
        ("finite", lambda: set_gradient(b, c, t, lo=nan)),
        ("finite", lambda: set_gradient(b, c, t, hi=inf)),
        ("ghi > glo", lambda: set_gradient(b, c, t, glo=5.0, ghi=5.0)),                                      # 7
        ("glo >= 0", lambda: set_gradient(b, c, t, glo=-1.0)),
        ("gradient range", lambda: set_gradient(b, c, t, ghi=inf)),
        ("gradient range", lambda: set_gradient(b, c, t, glo=nan)),
        ("spacing[0]", lambda: set_gradient(b, c, t, spacing=(0.0, 1.0, 1.0))),                              # 8
        ("spacing[1]", lambda: set_gradient(b, c, t, spacing=(1.0, -2.0, 1.0))),
        ("spacing[2]", lambda: set_gradient(b, c, t, spacing=(1.0, 1.0, inf))),
        ("spacing[2]", lambda: set_gradient(b, c, t, spacing=(1.0, 1.0, nan))),
        ("aligned", lambda: set_gradient(b, c, t.data_ptr() + 1, res=res, scalar_type=u16)),                 # 9
        ("aligned", lambda: set_gradient(b, c, t.data_ptr() + 2, res=res, scalar_type=cvr.SCALAR_F32)),
        ("not device-accessible", lambda: set_gradient(b, c, host.ctypes.data, res=res, scalar_type=u16)),
    ]
    for word, call in bad:
        code, text = refusal(cvr, call)
        assert code == INVALID and word in text, (word, text)
        assert records(b).tobytes() == before.tobytes(), word  # the previous medium still renders
    # unknown flags, CVR_DEVMED_CONST_ALBEDO among them; transfer flags and reserved; a NULL table
    lib = cvr.load()
    desc = cvr.GradientMediumDesc()
    desc.res[:] = res
    desc.d_scalar, desc.scalar_type = t.data_ptr(), u16
    tab = np.ascontiguousarray(c.table)
    m, n = tab.shape[:2]
    desc.transfer = cvr.GradientTransferDesc(n, m, 0, 0, tab.ctypes.data, c.lo, c.hi, c.glo, c.ghi)
    desc.transfer.spacing[:] = c.spacing
    desc.box_min[:], desc.box_max[:], desc.scale, desc.eta = c.box_min, c.box_max, c.scale, 1.04
    for flags in (cvr.DEVMED_CONST_ALBEDO, 8):
        desc.flags = flags
        assert lib.cvr_set_medium_gradient(b._h, desc) == INVALID
    desc.flags = 0
    for field in ("flags", "reserved"):                                                                      # 4
        for value in (1, 2):
            setattr(desc.transfer, field, value)
            assert lib.cvr_set_medium_gradient(b._h, desc) == INVALID
            setattr(desc.transfer, field, 0)
    desc.transfer.table = None
    assert lib.cvr_set_medium_gradient(b._h, desc) == INVALID
    assert records(b).tobytes() == before.tobytes()
    desc.transfer.table = tab.ctypes.data
    assert lib.cvr_set_medium_gradient(b._h, desc) == 0      # the descriptor itself is good
    # the order is the header's: each pair breaks two rules and the earlier one is named
    order = [
        ("empty grid", dict(scalar=0, res=(0, 4, 4), scalar_type=4)),                 # 1 before 2
        ("scalar_type", dict(scalar=t.data_ptr(), res=res, scalar_type=4, table=c.table[:1])),   # 2 before 3
        ("n * m", dict(scalar=0, res=res, scalar_type=u16, table=c.table[:1])),       # 3 before 5
        ("NULL", dict(scalar=0, res=res, scalar_type=u16, lo=2.0, hi=1.0)),           # 5 before 6
        ("hi > lo", dict(scalar=t, lo=2.0, hi=1.0, glo=-1.0)),                        # 6 before 7
        ("glo >= 0", dict(scalar=t, glo=-1.0, spacing=(0.0, 1.0, 1.0))),              # 7 before 8
        ("spacing[0]", dict(scalar=t.data_ptr() + 1, res=res, scalar_type=u16, spacing=(0.0, 1.0, 1.0))),  # 8 before 9
    ]
    for word, kw in order:
        kw = dict(kw)
        code, text = refusal(cvr, lambda: set_gradient(b, c, kw.pop("scalar"), **kw))
        assert code == INVALID and word in text, (word, text)
    b.close()


def test_refused_inside_an_adaptive_session(cvr):
    c = gr.case("random40_u16")
    b = context_b(cvr, c)
    before = records(b)
    t = scalar_tensor(c)
    with b.adaptive(cvr.AdaptiveDesc(8, 16, 4, -1.0, 0.01)):
        code, text = refusal(cvr, lambda: set_gradient(b, c, t))
        assert code == STATE and "adaptive session" in text and "cvr_set_medium_gradient" in text
    assert records(b).tobytes() == before.tobytes()
    b.close()


# ------------------------------------------------------- re-classification --
@pytest.mark.parametrize("fmt", [0, 1])
def test_a_second_table_on_the_same_tensor(cvr, oracle_mod, fmt):
    """set_medium_gradient twice on one context with two tables: the second state is a fresh context's."""
    first = gr.case("random40_u8")
    second = first._replace(table=gr.table2d(3, 9, seed=89), glo=5.0, ghi=90.0)
    t = scalar_tensor(first)
    b = new_ctx(cvr, fmt)
    set_gradient(b, first, t)
    assert_records_equal(records(ready(cvr, b)), gr.reference("random40_u8", fmt), "first table")
    set_gradient(b, second, t)
    fresh = context_b(cvr, second, fmt)
    a = context_a(cvr, second, fmt)
    assert_same_state(fresh, b, f"second table format {fmt}")
    assert_same_state(a, b, f"second table format {fmt} against the classified arrays")
    assert records(b).tobytes() != records(context_b(cvr, first, fmt)).tobytes()   # the table matters
    # and a sparse build over a dense one, then dense again
    sp = gr.case("halo")
    set_gradient(b, sp, scalar_tensor(sp))
    assert b.medium_layout().sparse == 1
    assert_records_equal(records(b), gr.reference("halo", fmt), "dense -> sparse")
    set_gradient(b, second, t)
    assert_same_state(fresh, b, f"sparse -> dense format {fmt}")
    close(a, b, fresh)


def test_timing_groups_are_reported(cvr):
    c = gr.case("random40_u16")
    b = new_ctx(cvr, 1, ((cvr.OPT_TIMING, 1),))
    set_gradient(b, c, scalar_tensor(c))
    ms = b.device_medium_ms()
    assert ms[0] > 0 and ms[1] == 0 and ms[4] > 0 and ms[5] > 0, ms  # one scan, the store, cells + bounds
    sp = gr.case("halo")
    set_gradient(b, sp, scalar_tensor(sp))
    ms = b.device_medium_ms()
    assert ms[0] == 0 and ms[2] > 0 and ms[3] > 0 and ms[4] > 0, ms     # sparse: no separate scan
    b.close()


# --------------------------------------------------------------------- CLI --
def test_cli_transfer2d(cvr, oracle_mod, tmp_path):
    """cvr --transfer2d writes the image of the oracle over classify_gradient_host's arrays (the
    comparison of test_cli_transfer), which a Python context given bucky's bytes also renders."""
    from parity_util import oracle_image
    W, H, iters = 64, 64, 4
    table = gr.table2d()
    m, n = table.shape[:2]
    glo, ghi, spacing = 2.0, 90.0, (1.0, 2.0, 0.5)
    path = tmp_path / "tf2d.txt"
    path.write_text(f"# n m\n{n} {m}\n" + "".join("%.9g %.9g %.9g %.9g\n" % tuple(row) for row in table.reshape(-1, 4)))
    img, _ = run_cli(tmp_path, "tf2d", "--synthetic", "bucky", "--transfer2d", str(path), "--gradient-range", str(glo),
                     str(ghi), "--voxel-spacing", *(str(v) for v in spacing), "-r", str(W), str(H), "-i", str(iters))
    scene = cvr.Scene.synthetic("bucky")
    raw = np.frombuffer(scene.raw_bytes, np.uint8).reshape(32, 32, 32)
    d, a, _ = cvr.classify_gradient_host(raw, table, 0.0, float(raw.max()), glo, ghi, spacing)
    md = scene.medium
    orc = oracle_mod.Oracle(d, a, tuple(md.box_min), tuple(md.box_max), md.scale, float(d.max()))
    iv, r2v = scene.camera(W, H)
    ref, _ = oracle_image(orc, iv, r2v, W, H, (1, 1), iters, 2)
    assert ref[..., :3].max() > 0
    assert_pixels_close(img, ref[..., :3], iters, "cvr --transfer2d against the oracle")
    # the Python context on the same bytes with the same arguments
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_medium_gradient(torch.from_numpy(raw.copy()).to(DEV), table, lo=0.0, hi=float(raw.max()), glo=glo, ghi=ghi,
                            spacing=spacing, box_min=tuple(md.box_min), box_max=tuple(md.box_max), scale=md.scale,
                            g=md.g, roughness=tuple(md.roughness), eta=md.eta)
    ctx.set_camera(iv, r2v, (W, H))
    ctx.init()
    py, _ = ctx.render_image(W, H, (1, 1), iters)
    scene.close()
    ctx.close()
    assert_pixels_close(img, py[..., :3], iters, "cvr --transfer2d against set_medium_gradient")
