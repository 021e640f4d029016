"""The caller-stream contract of the device entry points (include/cvr.h): a context put
on a caller's stream with cvr_set_stream orders every call on that stream and on no other, the calls
documented as asynchronous do not wait for it, the calls documented as synchronous have drained it when
they return, and cvr_set_stream itself waits for the stream it leaves.

A. Asynchronous calls.  The context is on a picked side stream S (tests/stream_util.py: proven to run
   beside the context's own stream and the null stream).  The call is warmed once, synchronised; inputs
   and outputs are then poisoned with valid data (another field, other sums, NaN, 0xFFFFFFFF, 1e6) and S
   is held by a device-side delay with the real inputs or the output's clear queued behind it.  The call
   must return with the hold pending, and a clone queued on S afterwards must hold the reference's bits
   (uint32 views): the host statements where tests/test_gpu_project.py, test_gpu_features.py,
   test_gpu_preview.py, test_gpu_shadow.py and test_gpu_denoise.py offer them, else the same call run
   synchronised on the context's own stream.  A launch, copy or memset queued on another stream runs
   during the hold, against the poison or before the clear, and leaves other bits.
   Renders are 64x64 pixels at one sample per pixel: a pixel receives at most one contribution, so no
   order of additions is involved (tests/test_gpu_wpool_matrix.py).
B. Synchronous calls, with the context on its own stream, on the null stream and on a side stream:
   the stream is idle when the call returns, and the result has the own-stream result's bits.  The four
   device medium builds also have their sources overwritten on torch's default stream as soon as they
   return ("the arrays are only read and may be freed afterwards") and every stored array compared with
   the host upload's.
C. cvr_set_stream: CVR_ERR_STATE inside an adaptive session, NULL is the null stream,
   cvr_own_stream restores, cvr_destroy waits for a caller's stream, and leaving a stream waits for it.

Every call under test takes int device addresses: the bindings synchronise torch's current stream when
they are handed a tensor.  Enqueue times: printed by the module's report fixture (run with -s); the
longest observed on an MI355X host is recorded at stream_util.HOLD_MS."""
import ctypes as C

import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import devmed
import media
import stream_util as su
import test_gpu_preview as tprev
import test_gpu_shadow as tshadow
from cudavolumerenderer_amd._lib import blocks_to_host, image_to_host
from envmap_util import ROT, env_image
from parity_util import COUNTERS
from test_denoise_cpu import random_sums
from test_gpu_features import SCALE, SMALL_TILES, arrays, host_planes, make_ctx, planes_for, view
from test_gpu_project import LOOK, RAGGED, desc_for
from test_gpu_project import host as project_host
from test_gpu_project import view as project_view
from test_project_cpu import field

pytestmark = pytest.mark.gpu

STATE = -3
F = np.float32
NAN = float("nan")
W = H = 64
RENDER = ((W, H), (W, H), (0, 0))
TILE = SMALL_TILES[1]  # 40x24 at offset (8, 8) of 64x48


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def dev(a):
    """A numpy array on the device (a copy)."""
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def read(stream, *tensors):
    """Clones queued on `stream` now, as numpy arrays once the stream has run them."""
    with torch.cuda.stream(stream):
        clones = [t.clone() for t in tensors]
    stream.synchronize()
    out = [c.cpu().numpy() for c in clones]
    return out[0] if len(out) == 1 else out


def on_stream(cvr, ctx, avoid=()):
    s = su.pick_stream(cvr, ctx, avoid)
    ctx.set_stream(s.cuda_stream)
    return s


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if su.ENQUEUE_MS:
        worst = max(su.ENQUEUE_MS, key=su.ENQUEUE_MS.get)
        print(f"\nstreams: longest enqueue {su.ENQUEUE_MS[worst]:.2f} ms ({worst}); hold {su.HOLD_MS} ms; "
              + ", ".join(f"{k} {v:.2f}" for k, v in sorted(su.ENQUEUE_MS.items())))


# =========================================================== A. asynchronous calls ==
def test_field_project_buffers(cvr):
    a = field("ragged_uint16")
    other = np.ascontiguousarray(a[::-1, ::-1, ::-1])  # the poison: another field of the same type and shape
    res = a.shape[::-1]
    w, h = RAGGED[1]
    ctx = cvr.Context(0, "regenerationSK")
    try:
        project_view(ctx, "oblique", RAGGED)
        s = on_stream(cvr, ctx)
        real, t = dev(a), dev(other)
        descs = {m: desc_for(cvr, a, m, **LOOK) for m in ("max", "iso")}
        outs = {m: [torch.full((h, w, 4), NAN, device="cuda"), torch.full((h, w), NAN, device="cuda"),
                    torch.full((h, w), NAN, device="cuda")] for m in descs}

        def call(m):
            o = outs[m]
            ctx.field_project_buffers(t.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), descs[m],
                                      scalar_type=cvr.SCALAR_U16, res=res)

        for m in descs:  # warm, on the poison
            call(m)
        ctx.synchronize()
        torch.cuda.synchronize()

        def producer():
            t.copy_(real)
            for o in outs.values():
                for p in o:
                    p.fill_(NAN)

        hold = su.Hold(s, producer)
        for m in descs:
            hold.call(lambda: call(m), f"field_project_buffers {m}")
        for m in descs:
            want = project_host(cvr, a, descs[m], "oblique", RAGGED)
            poisoned = project_host(cvr, other, descs[m], "oblique", RAGGED)
            assert not same(want[0], poisoned[0])  # the poison shows
            for name, g, wnt in zip(("rgba", "value", "depth"), read(s, *outs[m]), want):
                assert same(g, wnt), f"{m}: {name}"
    finally:
        ctx.close()


def test_field_histogram_buffers(cvr):
    a = field("ragged_uint16")
    other = np.ascontiguousarray(a[::-1, ::-1, ::-1] // 3)
    res = a.shape[::-1]
    cases = {"1d": dict(n=64, m=1, lo=0.0, hi=65535.0),
             "2d": dict(n=32, m=8, lo=1000.0, hi=60000.0, glo=0.0, ghi=40000.0, spacing=(1.0, 0.5, 2.0))}
    ctx = cvr.Context(0, "regenerationSK")
    try:
        s = on_stream(cvr, ctx)
        real, t = dev(a), dev(other)
        outs = {k: torch.full((c["m"], c["n"]), -1, dtype=torch.int32, device="cuda") for k, c in cases.items()}

        def call(k):
            ctx.field_histogram(t.data_ptr(), out=outs[k].data_ptr(), scalar_type=cvr.SCALAR_U16, res=res, **cases[k])

        for k in cases:
            call(k)
        ctx.synchronize()
        torch.cuda.synchronize()

        def producer():
            t.copy_(real)
            for o in outs.values():
                o.fill_(-1)  # 0xFFFFFFFF

        hold = su.Hold(s, producer)
        for k in cases:
            hold.call(lambda: call(k), f"field_histogram_buffers {k}")
        for k, c in cases.items():
            want = cvr.field_histogram_host(a, **c)
            assert not np.array_equal(want, cvr.field_histogram_host(other, **c))
            got = read(s, outs[k]).view(np.uint32)
            assert int(want.sum()) == a.size and np.array_equal(got, want), k
    finally:
        ctx.close()


def test_features_and_preview_buffers(cvr):
    w, h = TILE[1]
    ctx = make_ctx(cvr, "ragged", False, 0, True)
    try:
        view(ctx, "oblique", TILE)
        s = on_stream(cvr, ctx)
        rgba, depth, prev = (torch.zeros((h, w, 4), device="cuda"), torch.zeros((h, w), device="cuda"),
                             torch.zeros((h, w, 4), device="cuda"))
        pdesc = tprev.make_desc(cvr, "headlight")
        calls = {"features_buffers": lambda: ctx.features_buffers(rgba.data_ptr(), depth.data_ptr()),
                 "preview_buffers": lambda: ctx.preview_buffers(prev.data_ptr(), pdesc)}
        for fn in calls.values():
            fn()
        ctx.synchronize()
        torch.cuda.synchronize()
        # the outputs are set to NaN behind the hold: a kernel that ran early is overwritten
        hold = su.Hold(s, lambda: [t.fill_(NAN) for t in (rgba, depth, prev)])
        for what, fn in calls.items():
            hold.call(fn, what)
        g4, gz, gp = read(s, rgba, depth, prev)
        w4, wz = host_planes("ragged", False, 0, "oblique", TILE)
        assert same(g4, w4) and same(gz, wz), "features_buffers"
        assert (w4[..., 3] > 0).sum() > 50
        assert same(gp, tprev.host_image("ragged", False, 0, "oblique", TILE, "headlight")), "preview_buffers"
    finally:
        ctx.close()


def test_light_volume_then_shadowed_preview(cvr):
    """build, preview back to back behind one hold, after a synchronised build for another light at the
    same resolution (no reallocation): a preview that overtakes the build reads the old volume."""
    w, h = TILE[1]
    grid, old_light = tshadow.GRIDS[0], (0.0, 0.0, 1.0)
    ctx = make_ctx(cvr, "ragged", False, 0, False)
    try:
        view(ctx, "oblique", TILE)
        md = float(ctx.medium_info().max_density_eff)
        s = on_stream(cvr, ctx)
        out = torch.zeros((h, w, 4), device="cuda")
        desc = tshadow.make_desc(cvr, "shaded")
        ctx.build_light_volume(old_light, grid)
        ctx.preview_shadowed_buffers(out.data_ptr(), desc, 0.7)
        ctx.synchronize()
        torch.cuda.synchronize()
        old = tshadow.host_image("ragged", 0, "oblique", TILE, "shaded", 0.7, md, grid, old_light)
        assert same(read(s, out), old)
        hold = su.Hold(s, lambda: out.fill_(NAN))
        hold.call(lambda: ctx.build_light_volume(tshadow.LIGHT, grid), "build_light_volume")
        hold.call(lambda: ctx.preview_shadowed_buffers(out.data_ptr(), desc, 0.7), "preview_shadowed_buffers")
        want = tshadow.host_image("ragged", 0, "oblique", TILE, "shaded", 0.7, md, grid, tshadow.LIGHT)
        assert not same(want, old)
        assert same(read(s, out), want)
        assert same(ctx.light_volume(), tshadow.host_volume("ragged", 0, grid, tshadow.LIGHT))
    finally:
        ctx.close()


def test_denoise_buffers(cvr):
    """sum, m2 and the feature planes are copied in behind the hold: prepare -> passes -> output through
    the context's scratch images, plain and guided back to back."""
    h, w = 40, 72
    s1, s2 = random_sums(h, w, 8, 100 + w)
    p1, p2 = random_sums(h, w, 8, 500 + w)  # the poison: other sums
    f4, fz = planes_for(h, w, w)
    q4, qz = planes_for(h, w, w + 1)
    q4, qz = np.ascontiguousarray(q4[::-1]), np.ascontiguousarray(qz[:, ::-1])
    desc, gdesc = cvr.DenoiseDesc(3), cvr.DenoiseGuidedDesc(cvr.DenoiseDesc(3))
    ctx = cvr.Context(0, "regenerationSK")
    try:
        s = on_stream(cvr, ctx)
        real = [dev(x) for x in (s1, s2, f4, fz)]
        d = [dev(x) for x in (p1, p2, q4, qz)]
        out, var = torch.zeros((h, w, 4), device="cuda"), torch.zeros((h, w), device="cuda")
        gout, gvar = torch.zeros((h, w, 4), device="cuda"), torch.zeros((h, w), device="cuda")
        calls = {
            "denoise_buffers": lambda: ctx.denoise_buffers(d[0].data_ptr(), d[1].data_ptr(), w, h, out.data_ptr(),
                                                           n_samples=8, desc=desc, out_var=var.data_ptr()),
            "denoise_guided_buffers": lambda: ctx.denoise_guided_buffers(
                d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), w, h, gout.data_ptr(), n_samples=8,
                desc=gdesc, out_var=gvar.data_ptr()),
        }
        for fn in calls.values():
            fn()
        ctx.synchronize()
        torch.cuda.synchronize()

        def producer():
            for t, r in zip(d, real):
                t.copy_(r)
            for t in (out, var, gout, gvar):
                t.fill_(NAN)

        hold = su.Hold(s, producer)
        for what, fn in calls.items():
            hold.call(fn, what)
        g, gv, gg, ggv = read(s, out, var, gout, gvar)
        want, wvar = cvr.denoise_host(s1, s2, 8, None, desc)
        assert not same(want, cvr.denoise_host(p1, p2, 8, None, desc)[0])
        assert same(g, want) and same(gv, wvar), "denoise_buffers"
        want, wvar = cvr.denoise_guided_host(s1, s2, f4, fz, 8, None, gdesc)
        assert same(gg, want) and same(ggv, wvar), "denoise_guided_buffers"
        assert not same(gg, g)
    finally:
        ctx.close()


# ---------------------------------------------------------------- launch_render --
def render_ctx(cvr, kind, seed=7, moments=False, src=None):
    """A 64x64, one-sample context over a dense medium, a sparse medium, or a dense medium under an
    environment map: three wave-pool instance families."""
    if src is not None:
        ctx = cvr.Context(0, "regenerationSK")
        ctx.share_medium(src)
    else:
        ctx = make_ctx(cvr, "ragged" if kind == "sparse" else "blob16", False, 0, kind == "sparse")
    view(ctx, "oblique", RENDER)
    ctx.set_iterations(1)
    ctx.set_seed(seed)
    if moments:
        ctx.set_option(cvr.OPT_MOMENTS, 1)
    if kind == "env":
        ctx.set_environment(env_image(64, 32), 1.0, ROT)
    ctx.init()
    return ctx


def serial_image(ctx):
    """The render, synchronised, on the stream the context is on: (H, W, 4) raw sums."""
    ctx.clear_output()
    ctx.launch_render()
    ctx.synchronize()
    return ctx.copy_output(W, H)


@pytest.mark.parametrize("kind", ["dense", "sparse", "env"])
def test_launch_render(cvr, kind):
    lib = cvr.load()
    ctx = render_ctx(cvr, kind)
    try:
        want = serial_image(ctx)  # on the context's own stream
        assert (want[..., 3] > 0).sum() > 500 and (want[..., :3] > 0).any()
        s = on_stream(cvr, ctx)
        assert same(serial_image(ctx), want)  # warm on S
        # into the caller's buffer, poisoned, its clear behind the hold
        acc = torch.full((H, W, 4), 1e6, device="cuda")
        torch.cuda.synchronize()
        ctx.set_output(acc.data_ptr())
        hold = su.Hold(s, acc.zero_)
        hold.call(ctx.launch_render, f"launch_render {kind}")
        assert same(read(s, acc), want), "set_output"
        # into the context's own buffer (it holds the warm render's sums), cvr_clear_output behind the
        # hold, then the two stores into pinned memory on S
        ctx.set_output(None)
        assert lib.cvr_output_ptr(ctx._h) != acc.data_ptr()
        with cvr.PinnedImage(W, H) as img, cvr.PinnedImage(W, H) as blk:
            img.array[:] = np.nan
            blk.array[:] = np.nan
            hold = su.Hold(s)
            hold.call(ctx.clear_output, "clear_output")
            hold.call(ctx.launch_render, f"launch_render {kind}")
            hold.call(lambda: image_to_host(ctx.output_ptr(), img.ptr.value, W * H * 4, 1.0, s.cuda_stream),
                      "image_to_host")
            hold.call(lambda: blocks_to_host(ctx.output_ptr(), blk.ptr.value, W, H, 0, 1, 1.0, s.cuda_stream),
                      "blocks_to_host")
            assert np.isnan(img.array).all() and np.isnan(blk.array).all()
            s.synchronize()
            assert same(img.array, want), "image_to_host"
            assert same(blk.array, want), "blocks_to_host"
    finally:
        ctx.close()


def test_launch_render_moments(cvr):
    ctx = render_ctx(cvr, "dense", moments=True)
    try:
        ctx.clear_output()
        ctx.launch_render()
        ctx.synchronize()
        w1, w2 = ctx.copy_moments()  # on the context's own stream
        assert (w2[..., 3] == 1).sum() > 500 and (w2[..., :3] > 0).any()
        s = on_stream(cvr, ctx)
        ctx.launch_render()  # warm on S; the buffer now holds two renders' sums
        ctx.synchronize()
        hold = su.Hold(s)
        hold.call(ctx.clear_output, "clear_output moments")
        hold.call(ctx.launch_render, "launch_render moments")
        s.synchronize()
        g1, g2 = ctx.copy_moments()
        assert same(g1, w1), "S1"
        assert same(g2, w2), "S2"
    finally:
        ctx.close()


def test_three_renders_in_flight(cvr):
    """bench.py's shape: three contexts share one medium, each on its own stream with its own hold and
    clear; all are launched before any is waited for; every image is the serial one."""
    owner = render_ctx(cvr, "dense", seed=11)
    ctxs = [owner] + [render_ctx(cvr, "dense", seed=12 + k, src=owner) for k in range(2)]
    try:
        want = [serial_image(c) for c in ctxs]
        assert not same(want[0], want[1]) and not same(want[1], want[2])
        streams = []
        for c in ctxs:
            streams.append(on_stream(cvr, c, streams))
            c.set_option(cvr.OPT_INFLIGHT, 3)
            assert same(serial_image(c), want[len(streams) - 1])  # warm on its stream
        accs = [torch.full((H, W, 4), 1e6, device="cuda") for _ in ctxs]
        torch.cuda.synchronize()
        for c, a in zip(ctxs, accs):
            c.set_output(a.data_ptr())
        holds = [su.Hold(s, a.zero_) for s, a in zip(streams, accs)]
        for k, (c, hd) in enumerate(zip(ctxs, holds)):
            hd.call(c.launch_render, "launch_render in flight")
        assert all(hd.pending() for hd in holds)
        clones = []
        for s, a in zip(streams, accs):
            with torch.cuda.stream(s):
                clones.append(a.clone())
        for s in streams:
            s.synchronize()
        for k, (g, wnt) in enumerate(zip(clones, want)):
            assert same(g.cpu().numpy(), wnt), f"context {k}"
    finally:
        for c in reversed(ctxs):
            c.close()


# ============================================================ B. synchronous calls ==
def put_on(cvr, ctx, which):
    """The context on its own stream, the null stream or a picked side stream -> that stream."""
    if which == "own":
        ctx.use_own_stream()
        return su.own_stream(cvr, ctx)
    if which == "null":
        ctx.set_stream(None)
        return torch.cuda.default_stream()
    return on_stream(cvr, ctx)


MEDIUM_RES = (24, 17, 19)  # the ragged grid of tests/test_gpu_features.py, (x, y, z)


def build_inputs(cvr, build):
    """(host arrays the build reads, their poison, (density, albedo) of the host statement, sparse, format,
    transfer table or None)."""
    rng = np.random.default_rng(9)
    shape = MEDIUM_RES[::-1]
    if build in ("dense", "sparse", "f16"):
        d, a = arrays("ragged", False, 0)
        src = [d, a]
        return src, [np.ascontiguousarray(x[::-1]) for x in src], (d, a), build == "sparse", int(build == "f16"), None
    fld = rng.integers(0, 256, shape, dtype=np.uint8)
    table = np.zeros((16, 4), F)
    table[:, :3] = 0.2 + 0.8 * rng.random((16, 3), dtype=F)
    table[4:, 3] = np.linspace(0.05, 1.0, 12, dtype=F)
    if build == "scalar":
        want = cvr.classify_host(fld, table, 0.0, 255.0)
        src = [fld]
    elif build == "gradient":
        table = np.stack([table * F(s) for s in (0.25, 0.5, 0.75, 1.0)])
        table[..., :3] = np.clip(table[..., :3] * 2, 0, 1)
        want = cvr.classify_gradient_host(fld, table, 0.0, 255.0, 0.0, 200.0)[:2]
        src = [fld]
    else:
        labels = rng.integers(0, 3, shape, dtype=np.uint8)
        table = np.stack([table, table[::-1] * F(0.5) + F(0.25), table * F(0.75)])
        table = np.clip(table, 0, 1).astype(F)
        want = cvr.classify_labels_host(fld, labels, table, 0.0, 255.0)[:2]
        src = [fld, labels]
    poison = [np.ascontiguousarray(x[::-1, ::-1]) for x in src]  # valid values of the same type (labels < 3)
    return src, poison, want, False, 0, table


def device_build(cvr, ctx, build, t, table):
    common = dict(res=MEDIUM_RES, scale=SCALE, max_density=1.0)
    p = [x.data_ptr() for x in t]
    if build in ("dense", "sparse", "f16"):
        ctx.set_medium_device(p[0], p[1], sparse=build == "sparse", **common)
    elif build == "scalar":
        ctx.set_medium_scalar(p[0], table, lo=0.0, hi=255.0, scalar_type=cvr.SCALAR_U8, **common)
    elif build == "gradient":
        ctx.set_medium_gradient(p[0], table, lo=0.0, hi=255.0, glo=0.0, ghi=200.0,
                                scalar_type=cvr.SCALAR_U8, **common)
    else:
        ctx.set_medium_labeled(p[0], p[1], table, lo=0.0, hi=255.0, scalar_type=cvr.SCALAR_U8, **common)


def stored(cvr, ctx):
    return {k: ctx.debug_medium_array(k) for k in cvr.MEDIUM_ARRAYS}


@pytest.mark.parametrize("build", ["dense", "sparse", "f16", "scalar", "gradient", "labeled"])
def test_medium_builds_on_a_callers_stream(cvr, build):
    src, poison, (d, a), sparse, fmt, table = build_inputs(cvr, build)
    host = cvr.Context(0, "regenerationSK")
    ctxs = [host]
    try:
        host.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
        if sparse:
            sp = devmed.leaf_rule(d, a)
            desc, keep = media.sparse_desc(cvr, sp.res, sp.table, sp.leaf_density, sp.leaf_albedo, sp.albedo_bg, 1.0)
            desc.scale = SCALE
            host.set_medium_sparse(desc)
        else:
            desc, keep = cvr.medium_from_arrays(d, a, scale=SCALE, max_density=1.0)
            host.set_medium(desc)
        want = stored(cvr, host)
        assert sum(v is not None for v in want.values()) >= 3
        for which in ("own", "null", "side"):
            ctx = cvr.Context(0, "regenerationSK")
            ctxs.append(ctx)
            ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
            s = put_on(cvr, ctx, which)
            t, bad = [dev(x) for x in src], [dev(x) for x in poison]
            torch.cuda.synchronize()
            device_build(cvr, ctx, build, t, table)
            idle = s.query()
            for x, y in zip(t, bad):  # "only read and may be freed afterwards": overwritten at once
                x.copy_(y)
            assert idle, f"{build} on the {which} stream: work is pending when the synchronous call has returned"
            torch.cuda.synchronize()
            got = stored(cvr, ctx)
            for k in cvr.MEDIUM_ARRAYS:
                assert (got[k] is None) == (want[k] is None), f"{build} {which}: array {k}"
                if got[k] is not None:
                    assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), \
                        f"{build} on the {which} stream: {k} differs from the host build's"
            assert ctx.medium_layout().as_dict() == host.medium_layout().as_dict()
    finally:
        for c in ctxs:
            c.close()


def sync_calls(cvr, which):
    """Every synchronous device call once, the context on stream `which`: {name: bytes}; after each
    call the stream is idle."""
    out = {}
    fld = field("ragged_uint16")
    ctx = make_ctx(cvr, "blob16")
    try:
        view(ctx, "oblique", RENDER)
        ctx.set_seed(5)
        ctx.set_iterations(2)  # two values added onto zero per pixel: fp32 addition commutes
        ctx.set_option(cvr.OPT_MOMENTS, 1)
        ctx.init()
        s = put_on(cvr, ctx, which)
        t = dev(fld)
        torch.cuda.synchronize()
        fkw = dict(scalar_type=cvr.SCALAR_U16, res=fld.shape[::-1])

        def record(name, value):
            assert s.query(), f"{name} on the {which} stream: work is pending when the synchronous call has returned"
            arrays_ = value if isinstance(value, (tuple, list)) else (value,)
            out[name] = b"".join(np.ascontiguousarray(x).tobytes() for x in arrays_ if x is not None)

        ctx.clear_output()
        ctx.launch_render()
        record("copy_output", ctx.copy_output(W, H))
        ctx.clear_output()
        ctx.launch_render()
        record("copy_moments", ctx.copy_moments())
        ctx.clear_output()
        ctx.launch_render()
        st = ctx.stats()
        record("stats", np.array([getattr(st, k) for k in COUNTERS], np.uint64))
        assert st.paths == W * H * 2
        record("trace_paths", ctx.trace_paths(0, 1024))
        record("features", ctx.features())
        record("preview", ctx.preview())
        record("denoise", ctx.denoise(n_samples=2))
        record("field_stats", np.array(ctx.field_stats(t.data_ptr(), **fkw), np.float64))
        record("field_histogram", ctx.field_histogram(t.data_ptr(), 32, 4, lo=0.0, hi=65535.0, glo=0.0, ghi=40000.0, **fkw))
        record("field_project", ctx.field_project(t.data_ptr(), desc_for(cvr, fld, "iso", **LOOK), **fkw))
        ctx.set_option(cvr.OPT_MOMENTS, 0)
        ctx.set_iterations(1)
        record("render_frame", ctx.render_frame()[0])
        ctx.set_seed(3)
        with ctx.adaptive(cvr.AdaptiveDesc(2, 6, 1, -1.0, 0.01)) as a:  # one sample per launch: reproducible sums
            while not a.step().done:
                assert s.query(), f"adaptive pass on the {which} stream"
            record("adaptive image", a.image())
            record("adaptive moments", ctx.copy_moments())
    finally:
        ctx.close()
    return out


@pytest.fixture(scope="module")
def own_results(cvr):
    return sync_calls(cvr, "own")


@pytest.mark.parametrize("which", ["null", "side"])
def test_synchronous_calls_on_a_callers_stream(cvr, own_results, which):
    got = sync_calls(cvr, which)
    assert set(got) == set(own_results) and len(got) == 13
    for name in own_results:
        assert len(got[name]) > 0 and got[name] == own_results[name], f"{name} on the {which} stream"


# ============================================================== C. cvr_set_stream ==
def test_set_stream_inside_a_session(cvr):
    lib = cvr.load()
    results = []
    for attempt in (False, True):
        ctx = make_ctx(cvr, "blob16")
        try:
            view(ctx, "oblique", RENDER)
            ctx.set_seed(3)
            ctx.init()
            side = su.pick_stream(cvr, ctx)
            with ctx.adaptive(cvr.AdaptiveDesc(2, 6, 1, -1.0, 0.01)) as a:
                while not a.step().done:
                    if attempt:
                        assert lib.cvr_set_stream(ctx._h, C.c_void_p(side.cuda_stream)) == STATE
                        assert lib.cvr_set_stream(ctx._h, None) == STATE
                        with pytest.raises(cvr.CvrError) as e:
                            ctx.use_own_stream()
                        assert e.value.code == STATE and "session" in str(e.value)
                results.append((a.image(),) + ctx.copy_moments())
        finally:
            ctx.close()
    for x, y in zip(*results):
        assert same(x, y)


def test_null_and_own_stream_selection(cvr):
    """NULL selects the null stream; cvr_own_stream's stream restores the default."""
    w, h = TILE[1]
    null = torch.cuda.default_stream()
    # a context whose own stream runs beside the null stream (the power of the first half): own streams
    # take the hardware queues in turn, so one of a few contexts qualifies; none is a failure
    tried = []
    for _ in range(8):
        tried.append(make_ctx(cvr, "ragged", False, 0, True))
        if su.runs_beside(null, [su.own_stream(cvr, tried[-1])]):
            break
    else:
        for c in tried:
            c.close()
        raise AssertionError("no context's own stream ran beside the null stream: the test would have no power")
    ctx = tried.pop()
    try:
        for c in tried:
            c.close()
        view(ctx, "oblique", TILE)
        side = on_stream(cvr, ctx)
        own = su.own_stream(cvr, ctx)
        rgba = torch.zeros((h, w, 4), device="cuda")
        ctx.features_buffers(rgba.data_ptr())
        ctx.synchronize()
        want = host_planes("ragged", False, 0, "oblique", TILE)[0]
        # the null stream: ordered behind a hold on it
        ctx.set_stream(None)
        torch.cuda.synchronize()
        hold = su.Hold(null, lambda: rgba.fill_(NAN))
        hold.call(lambda: ctx.features_buffers(rgba.data_ptr()), "features_buffers on the null stream")
        assert same(read(null, rgba), want)
        # back on its own stream: it runs at once, beside a hold on the side stream it has left
        ctx.use_own_stream()
        rgba.fill_(NAN)
        torch.cuda.synchronize()
        hold = su.Hold(side)
        hold.call(lambda: ctx.features_buffers(rgba.data_ptr()), "features_buffers on the own stream")
        own.synchronize()
        assert hold.pending()
        assert same(read(own, rgba), want)
        side.synchronize()
    finally:
        ctx.close()


def test_close_waits_for_the_callers_stream(cvr):
    ctx = render_ctx(cvr, "dense")
    try:
        want = serial_image(ctx)
        s = on_stream(cvr, ctx)
        assert same(serial_image(ctx), want)
        acc = torch.full((H, W, 4), 1e6, device="cuda")
        torch.cuda.synchronize()
        ctx.set_output(acc.data_ptr())
        hold = su.Hold(s, acc.zero_)
        hold.call(ctx.launch_render, "launch_render before close")
        ctx.close()
        assert not hold.pending() and s.query()
        assert same(read(s, acc), want)
    finally:
        ctx.close()


def test_leaving_a_stream_waits_for_it(cvr):
    """cvr_set_stream to another stream first waits for the stream it leaves (the context's queues and
    scratch are single-stream state); naming the stream in use waits for nothing."""
    ctx = render_ctx(cvr, "dense")
    try:
        want = serial_image(ctx)
        s1 = on_stream(cvr, ctx)
        s2 = su.pick_stream(cvr, ctx, [s1])
        assert same(serial_image(ctx), want)
        acc = torch.full((H, W, 4), 1e6, device="cuda")
        torch.cuda.synchronize()
        ctx.set_output(acc.data_ptr())
        hold = su.Hold(s1, acc.zero_)
        hold.call(ctx.launch_render, "launch_render before leaving")
        hold.call(lambda: ctx.set_stream(s1.cuda_stream), "set_stream to the stream in use")
        ctx.set_stream(s2.cuda_stream)
        assert s1.query() and not hold.pending()
        assert same(read(s2, acc), want)  # (s1 is idle: any stream reads the finished render)
        hold = su.Hold(s2, acc.zero_)  # and the context now runs on s2
        hold.call(ctx.launch_render, "launch_render after leaving")
        assert same(read(s2, acc), want)
    finally:
        ctx.close()
