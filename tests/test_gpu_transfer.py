"""Scalar volumes classified on the device (cvr_set_medium_scalar) against cvr_set_medium_device.

Each case builds two contexts: A through set_medium_device on tensors of classify_host's output,
B through set_medium_scalar on the scalar tensor.  It asserts what assert_same_state of
tests/test_gpu_device_medium.py asserts (cvr_medium_info, cvr_medium_layout, the 4096 records of
the production launch as equal bytes, the launch's counters with `fetches`) and compares B's
records with the oracle over the classified arrays, whose records show escapes and real
collisions (checked on the CPU too, tests/test_transfer_cpu.py).  The media are
tests/transfer_ref.py's; the classified arrays and the oracle's records are computed once."""

import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import devmed
import transfer_ref as tr
from parity_util import assert_pixels_close
from test_cli_devices import run_cli
from test_gpu_device_medium import (DEV, INVALID, STATE, assert_records_equal, assert_same_state, launch_code,
                                    new_ctx, ready, records, refusal, tensors)

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------- helpers --
def scalar_tensor(c, name=None):
    """The case's scalar field on the device; OFFSET cases start that many bytes into a larger buffer."""
    s = np.ascontiguousarray(c.scalar)
    off = tr.OFFSET.get(name, 0)
    if not off:
        return torch.from_numpy(s).to(DEV)
    raw = torch.from_numpy(s.view(np.uint8).reshape(-1).copy()).to(DEV)
    buf = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device=DEV)
    buf[off:off + raw.numel()] = raw
    t = buf[off:off + raw.numel()].view(getattr(torch, s.dtype.name)).view(s.shape)
    assert t.data_ptr() % 16 == off and t.is_contiguous()
    return t


def host_classified(cvr, c):
    return cvr.classify_host(c.scalar, c.table, c.lo, c.hi, ceil=c.ceil, density_u=c.density_u)


def context_a(cvr, c, fmt=0, opts=(), max_density=None):
    d, a = host_classified(cvr, c)
    ctx = new_ctx(cvr, fmt, opts)
    td, ta = tensors(d, a)
    ctx.set_medium_device(td, ta, sparse=c.sparse, box_min=c.box_min, box_max=c.box_max, scale=c.scale,
                          max_density=max_density)
    del td, ta
    return ready(cvr, ctx)


def set_scalar(ctx, c, t, max_density=None, **kw):
    args = dict(lo=c.lo, hi=c.hi, ceil=c.ceil, density_u=c.density_u, sparse=c.sparse, box_min=c.box_min,
                box_max=c.box_max, scale=c.scale, max_density=max_density)
    args.update(kw)
    table = args.pop("table", c.table)
    ctx.set_medium_scalar(t, table, **args)


def context_b(cvr, c, fmt=0, opts=(), max_density=None, name=None):
    ctx = new_ctx(cvr, fmt, opts)
    t = scalar_tensor(c, name)
    set_scalar(ctx, c, t, max_density)
    del t  # the context does not keep the field
    return ready(cvr, ctx)


def pair(cvr, name, fmt, opts=(), max_density=None):
    c = tr.case(name)
    a, b = context_a(cvr, c, fmt, opts, max_density), context_b(cvr, c, fmt, opts, max_density, name)
    lay = assert_same_state(a, b, f"{name} format {fmt} options {opts}", tr.reference(name, fmt))
    return a, b, lay


def close(*ctxs):
    for c in ctxs:
        c.close()


# ------------------------------------------------------------------- dense --
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("name", ["spikes_f32", "offgrid_f32", "random40_u8", "random40_u16", "random40_i16",
                                  "unaligned_u8", "unaligned_u16", "ramp4096_u16", "two_entries", "two_entries_ceil"])
def test_dense_equals_the_device_call_on_classified_arrays(cvr, oracle_mod, name, fmt):
    a, b, lay = pair(cvr, name, fmt)
    assert lay["sparse"] == 0 and lay["albedo_uniform"] == 0
    assert b.medium_info().max_density_eff == a.medium_info().max_density_eff  # CVR_DEVMED_MAX_DENSITY
    close(a, b)


@pytest.mark.parametrize("fmt", [0, 1])
def test_host_output_is_the_numpy_statement_s(cvr, fmt):
    """What context A is built from is what the oracle's reference is built from."""
    for name in ("random40_u16", "spikes_f32"):
        d, a = host_classified(cvr, tr.case(name))
        wd, wa, _ = tr.classified(name)
        assert d.tobytes() == wd.tobytes() and a.tobytes() == wa.tobytes(), name


@pytest.mark.parametrize("fmt", [0, 1])
def test_given_majorant(cvr, oracle_mod, fmt):
    """Without CVR_DEVMED_MAX_DENSITY the descriptor's max_density is taken, as the device call takes it."""
    c = tr.case("random40_u16")
    a, b = context_a(cvr, c, fmt, max_density=1.5), context_b(cvr, c, fmt, max_density=1.5)
    assert_same_state(a, b, f"given majorant format {fmt}")
    assert b.medium_info().max_density_eff == a.medium_info().max_density_eff == 1.5
    close(a, b)


@pytest.mark.parametrize("fmt", [0, 1])
def test_uniform_rgb_table(cvr, oracle_mod, fmt):
    a, b, lay = pair(cvr, "uniform_rgb", fmt)
    assert lay["albedo_uniform"] == 1 and b.medium_layout().albedo_uniform == 1
    off = ((cvr.OPT_UNIFORM_ALBEDO, 0),)
    a2, b2, lay = pair(cvr, "uniform_rgb", fmt, off)
    assert lay["albedo_uniform"] == 0 and b2.medium_layout().albedo_uniform == 0
    close(a, b, a2, b2)


@pytest.mark.parametrize("fmt", [0, 1])
def test_bucky_with_the_raw_table(cvr, oracle_mod, fmt):
    """CEIL | DENSITY_U over the scene's bytes: also the host upload of the loader's arrays."""
    a, b, lay = pair(cvr, "bucky", fmt, max_density=1.0)
    scene = cvr.Scene.synthetic("bucky")
    host = new_ctx(cvr, fmt)
    host.set_medium(scene.medium)
    assert_same_state(ready(cvr, host), b, f"bucky format {fmt}: host upload of scene.medium")
    scene.close()
    close(a, b, host)


# ------------------------------------------------------------------ sparse --
def full_leaves(c):
    nz, ny, nx = c.scalar.shape
    return ((nz + 7) // 8) * ((ny + 7) // 8) * ((nx + 7) // 8)


@pytest.mark.parametrize("name,fmt", [("sparse_small_zero", 0), ("sparse_small_zero", 1), ("sparse_es4_zero", 0),
                                      ("sparse_es4_zero", 1)])
def test_sparse_zero_entry_keeps_empty_leaves_empty(cvr, oracle_mod, name, fmt):
    a, b, lay = pair(cvr, name, fmt)
    c = tr.case(name)
    want = devmed.leaf_rule(*tr.classified(name)[:2]).leaf_density.shape[0]
    assert lay["sparse"] == 1 and lay["n_leaves"] == b.medium_layout().n_leaves == want < full_leaves(c)
    assert b.medium_info().albedo_bytes > 0
    bg = cvr.half_round(c.table[0, :3]) if fmt else c.table[0, :3]  # entry 0's colour, as the format stores it
    assert lay["albedo_bg"] == [float(v) for v in bg]
    close(a, b)


@pytest.mark.parametrize("fmt", [0, 1])
def test_sparse_dense_entry_makes_every_leaf(cvr, oracle_mod, fmt):
    a, b, lay = pair(cvr, "sparse_small_dense", fmt)
    assert lay["n_leaves"] == b.medium_layout().n_leaves == full_leaves(tr.case("sparse_small_dense"))
    close(a, b)


@pytest.mark.parametrize("fmt", [0, 1])
def test_sparse_one_colour_has_no_albedo_pool(cvr, oracle_mod, fmt):
    a, b, lay = pair(cvr, "sparse_small_one_colour", fmt)
    assert a.medium_info().albedo_bytes == b.medium_info().albedo_bytes == 0
    assert 0 < lay["n_leaves"] < full_leaves(tr.case("sparse_small_one_colour"))
    close(a, b)


# ----------------------------------------------------------- half overflow --
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("what", ["density", "colour"])
def test_half_overflow_names_what_the_device_call_names(cvr, what, sparse):
    """A table entry of 70000 that some voxels reach: B's code and message are A's."""
    c = tr.case("sparse_small_zero" if sparse else "random40_u8")
    table = c.table.copy()
    table[4, 3 if what == "density" else 1] = np.float32(70000.0)
    c = c._replace(table=table)
    d, al = host_classified(cvr, c)
    assert ((d if what == "density" else al[..., 1]) >= 65520).any()
    good = tr.case("random40_u16")
    a, b = context_a(cvr, good, 1), context_b(cvr, good, 1)
    td, ta = tensors(d, al)
    ac, at = refusal(cvr, lambda: a.set_medium_device(td, ta, sparse=c.sparse, scale=c.scale, max_density=None))
    t = scalar_tensor(c)
    bc, bt = refusal(cvr, lambda: set_scalar(b, c, t))
    assert (bc, bt) == (ac, at) and bc == INVALID and "rounds to infinity" in bt, (bt, at)
    assert ("density" if what == "density" else "albedo") in bt, bt
    assert launch_code(cvr, a) == STATE and launch_code(cvr, b) == STATE  # left without a medium
    # format 0 takes the same field and table
    b.set_option(cvr.OPT_MEDIUM_FORMAT, 0)
    set_scalar(b, c, t)
    assert b.medium_info().format == 0
    close(a, b)


# ---------------------------------------------------------------- refusals --
def test_invalid_descriptors_keep_the_previous_medium(cvr):
    c = tr.case("random40_u16")
    b = context_b(cvr, c)
    before = records(b)
    t = scalar_tensor(c)
    res = c.scalar.shape[::-1]
    u16 = cvr.SCALAR_U16
    host = np.ascontiguousarray(c.scalar)
    bad = [
        ("NULL", lambda: set_scalar(b, c, 0, res=res, scalar_type=u16)),
        ("2..4096", lambda: set_scalar(b, c, t, table=c.table[:1])),
        ("2..4096", lambda: set_scalar(b, c, t, table=np.zeros((4097, 4), np.float32))),
        ("hi > lo", lambda: set_scalar(b, c, t, lo=5.0, hi=5.0)),
        ("hi > lo", lambda: set_scalar(b, c, t, lo=6.0, hi=5.0)),
        ("finite", lambda: set_scalar(b, c, t, lo=float("nan"))),
        ("finite", lambda: set_scalar(b, c, t, hi=float("inf"))),
        ("scalar_type", lambda: set_scalar(b, c, t.data_ptr(), res=res, scalar_type=4)),
        ("aligned", lambda: set_scalar(b, c, t.data_ptr() + 1, res=res, scalar_type=u16)),
        ("aligned", lambda: set_scalar(b, c, t.data_ptr() + 2, res=res, scalar_type=cvr.SCALAR_F32)),
        ("not device-accessible", lambda: set_scalar(b, c, host.ctypes.data, res=res, scalar_type=u16)),  # a host pointer
        ("empty grid", lambda: set_scalar(b, c, t.data_ptr(), res=(0, 4, 4), scalar_type=u16)),
    ]
    for word, call in bad:
        code, text = refusal(cvr, call)
        assert code == INVALID and word in text, (word, text)
        assert records(b).tobytes() == before.tobytes(), word  # the previous medium still renders
    # unknown flags, CVR_DEVMED_CONST_ALBEDO among them, and an unknown transfer flag
    lib = cvr.load()
    desc = cvr.ScalarMediumDesc()
    desc.res[:] = res
    desc.d_scalar, desc.scalar_type = t.data_ptr(), u16
    tab = np.ascontiguousarray(c.table)
    desc.transfer = cvr.TransferDesc(7, 0, tab.ctypes.data, c.lo, c.hi)
    desc.box_min[:], desc.box_max[:], desc.scale, desc.eta = c.box_min, c.box_max, c.scale, 1.04
    for flags in (cvr.DEVMED_CONST_ALBEDO, 8):
        desc.flags = flags
        assert lib.cvr_set_medium_scalar(b._h, desc) == INVALID
    desc.flags, desc.transfer.flags = 0, 4
    assert lib.cvr_set_medium_scalar(b._h, desc) == INVALID
    desc.transfer.flags, desc.transfer.table = 0, None
    assert lib.cvr_set_medium_scalar(b._h, desc) == INVALID
    assert records(b).tobytes() == before.tobytes()
    # the shape is judged before any pointer, and the order is the contract's: with a NULL field
    # and a bad range, the NULL is named
    code, text = refusal(cvr, lambda: set_scalar(b, c, 0, res=(0, 4, 4), scalar_type=u16))
    assert code == INVALID and "empty grid" in text
    code, text = refusal(cvr, lambda: set_scalar(b, c, 0, res=res, scalar_type=u16, lo=2.0, hi=1.0))
    assert code == INVALID and "NULL" in text
    b.close()


def test_refused_inside_an_adaptive_session(cvr):
    c = tr.case("random40_u16")
    b = context_b(cvr, c)
    before = records(b)
    t = scalar_tensor(c)
    with b.adaptive(cvr.AdaptiveDesc(8, 16, 4, -1.0, 0.01)):
        code, text = refusal(cvr, lambda: set_scalar(b, c, t))
        assert code == STATE and "adaptive session" in text and "cvr_set_medium_scalar" in text
    assert records(b).tobytes() == before.tobytes()
    b.close()


# ------------------------------------------------------- re-classification --
@pytest.mark.parametrize("fmt", [0, 1])
def test_a_second_table_on_the_same_tensor(cvr, oracle_mod, fmt):
    """set_medium_scalar twice on one context with two tables: the second state is a fresh context's."""
    first, second = tr.case("random40_u8"), tr.case("uniform_rgb")  # the same field, two tables
    assert first.scalar.tobytes() == second.scalar.tobytes()
    t = scalar_tensor(first)
    b = new_ctx(cvr, fmt)
    set_scalar(b, first, t)
    assert_records_equal(records(ready(cvr, b)), tr.reference("random40_u8", fmt), "first table")
    set_scalar(b, second, t)
    fresh = context_b(cvr, second, fmt)
    lay = assert_same_state(fresh, b, f"second table format {fmt}", tr.reference("uniform_rgb", fmt))
    assert lay["albedo_uniform"] == 1
    # and a sparse build over a dense one, then dense again
    sp = tr.case("sparse_small_zero")
    set_scalar(b, sp, scalar_tensor(sp))
    assert b.medium_layout().sparse == 1
    assert_records_equal(records(b), tr.reference("sparse_small_zero", fmt), "dense -> sparse")
    set_scalar(b, second, t)
    assert_same_state(fresh, b, f"sparse -> dense format {fmt}")
    close(b, fresh)


def test_timing_groups_are_reported(cvr):
    c = tr.case("random40_u16")
    b = new_ctx(cvr, 1, ((cvr.OPT_TIMING, 1),))
    set_scalar(b, c, scalar_tensor(c))
    ms = b.device_medium_ms()
    assert ms[0] > 0 and ms[1] == 0 and ms[4] > 0 and ms[5] > 0, ms  # one scan, the store, cells + bounds
    sp = tr.case("sparse_small_zero")
    set_scalar(b, sp, scalar_tensor(sp))
    ms = b.device_medium_ms()
    assert ms[0] == 0 and ms[2] > 0 and ms[3] > 0 and ms[4] > 0, ms     # sparse: no separate scan
    b.close()


# --------------------------------------------------------------------- CLI --
@pytest.mark.parametrize("mode", ["linear", "ceil"])
def test_cli_transfer(cvr, oracle_mod, tmp_path, mode):
    from parity_util import oracle_image
    W, H, iters = 64, 64, 4
    table = tr.table7()
    path = tmp_path / "tf.txt"
    path.write_text("# r g b density\n" + "".join("%.9g %.9g %.9g %.9g\n" % tuple(row) for row in table))
    img, _ = run_cli(tmp_path, "tf", "--synthetic", "bucky", "--transfer", str(path), "--transfer-mode", mode,
                     "-r", str(W), str(H), "-i", str(iters))
    scene = cvr.Scene.synthetic("bucky")
    raw = np.frombuffer(scene.raw_bytes, np.uint8).reshape(32, 32, 32)
    d, a = cvr.classify_host(raw, table, 0.0, float(raw.max()), ceil=(mode == "ceil"))
    md = scene.medium
    orc = oracle_mod.Oracle(d, a, tuple(md.box_min), tuple(md.box_max), md.scale, float(d.max()))
    iv, r2v = scene.camera(W, H)
    ref, _ = oracle_image(orc, iv, r2v, W, H, (1, 1), iters, 2)
    scene.close()
    assert ref[..., :3].max() > 0
    assert_pixels_close(img, ref[..., :3], iters, f"cvr --transfer ({mode}) against the oracle")
