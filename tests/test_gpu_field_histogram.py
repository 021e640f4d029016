"""Field statistics and value-gradient histograms on the device (cvr_field_stats,
cvr_field_histogram, cvr_field_histogram_buffers) against the host statements: counts exactly,
statistics as bits.  The results are integer counts and order-independent extrema, so no
summation-order allowance exists.  The fields and the bin shapes are tests/histogram_ref.py's (the
host statements are compared with the numpy restatement on the same cases without a GPU,
tests/test_field_histogram_cpu.py); the host results are computed once per case."""
import re
import subprocess
from functools import lru_cache

import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import histogram_ref as hr
from test_cli_devices import CLI, run_cli
from test_gpu_device_medium import DEV, INVALID, new_ctx, ready, records, refusal

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------- helpers --
@pytest.fixture(scope="module")
def ctx(cvr):
    """One context without a medium: the calls take its device and stream and nothing else."""
    c = cvr.Context(0, "regenerationSK")
    yield c
    c.close()


def device_field(scalar, offset=0):
    """The (z, y, x) array on the device, `offset` bytes past a 16-byte boundary of its allocation."""
    s = np.ascontiguousarray(scalar)
    if not offset:
        return torch.from_numpy(s.copy()).to(DEV)
    raw = torch.from_numpy(s.view(np.uint8).reshape(-1).copy()).to(DEV)
    buf = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device=DEV)
    buf[offset:offset + raw.numel()] = raw
    t = buf[offset:offset + raw.numel()].view(getattr(torch, s.dtype.name)).view(s.shape)
    assert t.data_ptr() % 16 == offset and t.is_contiguous()
    return t


@lru_cache(maxsize=None)
def tensor_of(name):
    return device_field(hr.field(name).scalar)


@lru_cache(maxsize=None)
def host_histogram(name, n, m):
    import cudavolumerenderer_amd as cvr
    f = hr.field(name)
    h = cvr.field_histogram_host(f.scalar, n, m, lo=f.lo, hi=f.hi, glo=f.glo, ghi=f.ghi, spacing=f.spacing)
    h.setflags(write=False)
    return h


def device_histogram(ctx, name, n, m, t=None, **kw):
    f = hr.field(name)
    return ctx.field_histogram(tensor_of(name) if t is None else t, n, m, lo=f.lo, hi=f.hi, glo=f.glo, ghi=f.ghi,
                               spacing=f.spacing, **kw)


def assert_counts(got, want, what):
    assert got.dtype == np.uint32 and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d bins differ, first (j, i) = %s: device %d, host %d; sums %d and %d" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], got.sum(dtype=np.uint64),
        want.sum(dtype=np.uint64))


# -------------------------------------------------------------- histograms --
@pytest.mark.parametrize("case", hr.HISTOGRAMS, ids=hr.ident)
def test_device_histogram_equals_host(ctx, case):
    name, n, m = case
    want = host_histogram(name, n, m)
    got = device_histogram(ctx, name, n, m)
    assert_counts(got, want, hr.ident(case))
    assert int(got.sum(dtype=np.uint64)) == hr.field(name).scalar.size


# one bin shape per field through cvr_field_histogram_buffers, into a tensor full of garbage
BUFFERS = [("random40_u8", 7, 5), ("random40_u16", 129, 128), ("random40_i16", 256, 1), ("offgrid_f32", 128, 128),
           ("runs_u16", 7, 5), ("nonfinite_f32", 7, 5), ("more_tasks_u8", 7, 5), ("constant_u8", 256, 256),
           ("alternating_u8", 64, 64), ("long_1d_u8", 256, 1), ("thin4_u16", 256, 1), ("one_voxel_u8", 7, 5)]


@pytest.mark.parametrize("case", BUFFERS, ids=hr.ident)
def test_buffers_overwrite_every_word(ctx, case):
    name, n, m = case
    assert case in hr.HISTOGRAMS
    out = torch.full((m, n), -559038737, dtype=torch.int32, device=DEV)
    assert device_histogram(ctx, name, n, m, out=out) is out
    ctx.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert_counts(got, host_histogram(name, n, m), hr.ident(case) + " through _buffers")
    # an int address with res and scalar_type, as set_medium_gradient takes one
    f, t = hr.field(name), tensor_of(name)
    out.fill_(7)
    ctx.field_histogram(t.data_ptr(), n, m, lo=f.lo, hi=f.hi, glo=f.glo, ghi=f.ghi, spacing=f.spacing,
                        out=out.data_ptr(), res=f.scalar.shape[::-1],
                        scalar_type={"float32": 0, "uint8": 1, "uint16": 2, "int16": 3}[f.scalar.dtype.name])
    ctx.synchronize()
    assert_counts(out.cpu().numpy().view(np.uint32), host_histogram(name, n, m), hr.ident(case) + " by address")


def test_contended_bins_hold_their_counts(ctx):
    """A constant field puts 262144 voxels into one bin (past any 16-bit counter, every wave uniform);
    alternating values along x leave no wave uniform and split them over two."""
    got = device_histogram(ctx, "constant_u8", 64, 64)
    assert got.max() == 262144 and np.count_nonzero(got) == 1
    got = device_histogram(ctx, "alternating_u8", 256, 256)
    assert np.count_nonzero(got.sum(axis=0)) == 2 and got.sum(axis=0).max() == 131072


# ---------------------------------------------------------------- statistics --
@pytest.mark.parametrize("name", hr.STATS)
def test_device_stats_equal_host(cvr, ctx, name):
    f = hr.field(name)
    want = cvr.field_stats_host(f.scalar, f.spacing)
    got = ctx.field_stats(tensor_of(name), f.spacing)
    assert hr.same_stats(got, want), (name, got, want)


def test_nonfinite_statistics(cvr, ctx):
    """inf - inf magnitudes count in nan_gradients; -0 orders below +0 on the device too."""
    f = hr.field("nonfinite_f32")
    got = ctx.field_stats(tensor_of("nonfinite_f32"))
    assert got.nan_values == 2 and got.nan_gradients == int(np.isnan(hr.mag_of("nonfinite_f32")).sum())
    assert got.nan_gradients > int(np.isnan(f.scalar).sum()) and got.gmax == np.inf
    z = np.zeros((3, 4, 70), np.float32)
    z[1, 2, 65] = -0.0
    got = ctx.field_stats(device_field(z))
    assert np.signbit(got.vmin) and not np.signbit(got.vmax) and got.gmax == 0
    got = ctx.field_stats(tensor_of("all_nan_f32"))
    assert (got.vmin, got.vmax, got.gmax, got.nan_values, got.nan_gradients) == (np.inf, -np.inf, 0.0, 60, 60)


# -------------------------------------------------------------- wide loads --
@pytest.mark.parametrize("name,offset", [("thin4_u8", 1), ("thin4_u8", 15), ("thin4_u16", 2), ("runs_u16", 6)])
def test_unaligned_fields(cvr, ctx, name, offset):
    """The 1-D pass cuts a head, 16-byte groups and a tail from any element alignment; the walk and
    the statistics read single voxels."""
    f = hr.field(name)
    t = device_field(f.scalar, offset)
    for n, m in ((256, 1), (65536, 1), (7, 5)):
        want = cvr.field_histogram_host(f.scalar, n, m, lo=f.lo, hi=f.hi, glo=f.glo, ghi=f.ghi, spacing=f.spacing)
        assert_counts(device_histogram(ctx, name, n, m, t=t), want, "%s at byte %d, %d x %d" % (name, offset, n, m))
    assert hr.same_stats(ctx.field_stats(t, f.spacing), cvr.field_stats_host(f.scalar, f.spacing))


def test_short_fields_around_one_group(cvr, ctx):
    """Fewer voxels than the head, exactly one group, one group and a tail."""
    rng = np.random.default_rng(103)
    for count in (1, 5, 15, 16, 17, 31, 33):
        for offset in (0, 3, 15):
            s = rng.integers(0, 256, (1, 1, count)).astype(np.uint8)
            got = ctx.field_histogram(device_field(s, offset), 256, lo=0.0, hi=255.0)
            assert_counts(got, cvr.field_histogram_host(s, 256, lo=0.0, hi=255.0), "%d voxels at byte %d" % (count, offset))


# ------------------------------------------------------- context untouched --
def test_context_with_a_medium_is_untouched(cvr):
    import devmed
    import media
    m = media.random40()
    c = new_ctx(cvr)
    desc, _keep = cvr.medium_from_arrays(m.density, m.albedo, m.box_min, m.box_max, m.scale, m.max_density)
    c.set_medium(desc)
    ready(cvr, c)
    info, before = c.medium_info().as_dict(), records(c)
    assert len(before) == devmed.N == 4096
    f = hr.field("random40_u16")
    st = c.field_stats(tensor_of("random40_u16"), f.spacing)
    got = device_histogram(c, "random40_u16", 7, 5)
    assert hr.same_stats(st, cvr.field_stats_host(f.scalar, f.spacing))
    assert_counts(got, host_histogram("random40_u16", 7, 5), "on a context with a medium")
    assert c.medium_info().as_dict() == info
    assert before.tobytes() == records(c).tobytes()
    c.close()


def test_inside_an_adaptive_session(cvr):
    import media
    m = media.random40()
    c = new_ctx(cvr)
    desc, _keep = cvr.medium_from_arrays(m.density, m.albedo, m.box_min, m.box_max, m.scale, m.max_density)
    c.set_medium(desc)
    ready(cvr, c)
    f = hr.field("random40_u8")
    with c.adaptive(cvr.AdaptiveDesc(2, 6, 1, -1.0, 0.01)) as a:
        while not a.step().done:
            st = c.field_stats(tensor_of("random40_u8"), f.spacing)
            got = device_histogram(c, "random40_u8", 7, 5)
    assert hr.same_stats(st, cvr.field_stats_host(f.scalar, f.spacing))
    assert_counts(got, host_histogram("random40_u8", 7, 5), "inside an adaptive session")
    c.close()


# ---------------------------------------------------------------- refusals --
def test_pointer_refusals(cvr, ctx):
    f = hr.field("random40_u16")
    host = np.ascontiguousarray(f.scalar)
    res, kw = host.shape[::-1], dict(lo=f.lo, hi=f.hi, glo=f.glo, ghi=f.ghi)
    t = tensor_of("random40_u16")
    out = torch.zeros(35, dtype=torch.int32, device=DEV)
    host_out = np.zeros(35, np.uint32)
    code, msg = refusal(cvr, lambda: ctx.field_histogram(host.ctypes.data, 7, 5, res=res, scalar_type=cvr.SCALAR_U16, **kw))
    assert code == INVALID and "scalar is not device-accessible" in msg
    code, msg = refusal(cvr, lambda: ctx.field_stats(host.ctypes.data, res=res, scalar_type=cvr.SCALAR_U16))
    assert code == INVALID and "scalar is not device-accessible" in msg
    code, msg = refusal(cvr, lambda: ctx.field_histogram(t, 7, 5, out=host_out.ctypes.data, **kw))
    assert code == INVALID and "d_counts is not device-accessible" in msg
    code, msg = refusal(cvr, lambda: ctx.field_histogram(t.data_ptr() + 1, 7, 5, res=res, scalar_type=cvr.SCALAR_U16, **kw))
    assert code == INVALID and "2-byte aligned" in msg
    code, msg = refusal(cvr, lambda: ctx.field_histogram(t, 7, 5, out=out.data_ptr() + 2, **kw))
    assert code == INVALID and "d_counts must be 4-byte aligned" in msg
    # the descriptor's rules come first: a host address with hi <= lo reports the range
    code, msg = refusal(cvr, lambda: ctx.field_histogram(host.ctypes.data, 7, 5, res=res, scalar_type=cvr.SCALAR_U16,
                                                         lo=1.0, hi=1.0, glo=0.0, ghi=1.0))
    assert code == INVALID and "value range" in msg
    with pytest.raises(ValueError):
        ctx.field_histogram(t, 7, 5, out=torch.zeros(34, dtype=torch.int32, device=DEV), **kw)
    with pytest.raises(ValueError):
        ctx.field_stats(torch.from_numpy(host.copy()))   # a CPU tensor


# --------------------------------------------------------------------- CLI --
def test_cli_histogram_and_stats(cvr, tmp_path):
    """cvr --histogram --gradient-range auto --field-stats beside a render: the file's counts are
    field_histogram_host's on the scene's bytes with ghi the host gmax, the printed statistics the
    host's."""
    path = tmp_path / "hist.txt"
    _img, out = run_cli(tmp_path, "hist", "--synthetic", "bucky", "--histogram", str(path), "--histogram-bins", "16", "8",
                        "--gradient-range", "auto", "--field-stats", "-r", "64", "64", "-i", "2")
    raw = np.frombuffer(cvr.Scene.synthetic("bucky").raw_bytes, np.uint8).reshape(32, 32, 32)
    st = cvr.field_stats_host(raw)
    lines = path.read_text().splitlines()
    assert lines[0].split() == ["16", "8"] and len(lines) == 9
    got = np.array([[int(v) for v in ln.split()] for ln in lines[1:]], np.uint32)
    want = cvr.field_histogram_host(raw, 16, 8, lo=0.0, hi=float(raw.max()), glo=0.0, ghi=float(st.gmax))
    assert_counts(got, want, "cvr --histogram")
    m = re.search(r"field statistics\s*: values (\S+) \.\. (\S+), largest gradient magnitude (\S+), NaN values (\d+), "
                  r"NaN gradients (\d+)", out)
    assert m, out
    printed = cvr.FieldStats(np.float32(m.group(1)), np.float32(m.group(2)), np.float32(m.group(3)), int(m.group(4)),
                             int(m.group(5)))
    assert hr.same_stats(printed, st), (printed, st)


def test_cli_without_a_render(cvr, tmp_path):
    """--iterations 0: the field's numbers alone, no image; --histogram-bins N alone is the 1-D
    histogram and needs no gradient range."""
    path, out = tmp_path / "hist1d.txt", tmp_path / "none"
    r = subprocess.run([CLI, "--interactive", "0", "-o", str(out), "--synthetic", "bucky", "-i", "0", "--field-stats",
                        "--histogram", str(path), "--histogram-bins", "32", "--voxel-spacing", "1", "2", "0.5"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not list(tmp_path.glob("none*")) and "rendering time" not in r.stdout
    raw = np.frombuffer(cvr.Scene.synthetic("bucky").raw_bytes, np.uint8).reshape(32, 32, 32)
    lines = path.read_text().splitlines()
    assert lines[0].split() == ["32", "1"] and len(lines) == 2
    got = np.array([[int(v) for v in lines[1].split()]], np.uint32)
    assert_counts(got, cvr.field_histogram_host(raw, 32, lo=0.0, hi=float(raw.max())), "cvr --histogram, 1-D")
    st = cvr.field_stats_host(raw, (1.0, 2.0, 0.5))
    m = re.search(r"largest gradient magnitude (\S+),", r.stdout)
    assert m and np.float32(m.group(1)).view(np.uint32) == np.float32(st.gmax).view(np.uint32), r.stdout
    # a constant field has no automatic gradient range
    flat = tmp_path / "flat.raw"
    flat.write_bytes(bytes([5]) * 32 ** 3)
    r = subprocess.run([CLI, "--interactive", "0", "-o", str(out), "-s", str(flat), "--scene-type", "Raw", "-i", "0",
                        "--histogram", str(path), "--gradient-range", "auto"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--gradient-range auto" in r.stderr and "[ConfigParser] Error:" in r.stderr
