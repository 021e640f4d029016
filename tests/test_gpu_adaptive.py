"""Adaptive sampling on the GPU: the second moments of the wave pool (CVR_OPT_MOMENTS), the
launch of a subset of blocks, the stepwise decisions of cvr_adaptive_pass against the
host statement of the metric, the final image and the refusals.

Everything is compared with the CPU oracle's per-path records of the same path ids: a
pixel's sums differ from the oracle's only in the order of the fp32 additions, so
|gpu - cpu| <= 2 (n - 1) 2^-24 max(|gpu|, |cpu|) + 1e-30 with n the pixel's own number of
contributions, NaN pixels coincide, and counts and counters are equal.

Shapes: 64x64 pixels (64 blocks of 8x8), bucky (32^3), manix at (64, 58, 64), the sparse
cloud at test_sparse.CLOUD_SMALL.  The oracle's records of a scene are traced once per
module and shared.

Stepwise decisions (test_stepwise_decisions), predicted on the CPU from the oracle's records
in fp64, not measured on a GPU: bucky (target 0.1) stops 32 / 4 / 4 blocks at 8 / 16 / 20
samples and runs 24 to 32; manix_small (target 0.02) stops 24 / 2 / 1 / 2 at 8 / 16 / 20 /
28 and runs 35 to 32; the smallest |e - target| over all checks is 7.5e-4 / 2.2e-4.  The
device's fp32 sums may move single errors, so only the coarse shape of the map is pinned
(the MI355X run gave exactly the predicted stops, 7 passes each)."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from parity_util import COUNTERS, NTHREADS, assert_counters_equal, assert_sums_close, oracle_for_scene  # noqa: F401
from test_sparse import CLOUD_SMALL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cudavolumerenderer_amd", "cvr")
W = H = 64
P = W * H
NB = (W // 8) * (H // 8)
ATOL, RTOL = 1e-6, 1e-9  # the metric tolerance (tests/test_adaptive_cpu.py)
SCENES = {"bucky": ("bucky", None), "manix_small": ("manix", (64, 58, 64)), "cloud": ("cloud", CLOUD_SMALL)}


# ----------------------------------------------------------------- helpers --
@pytest.fixture(scope="module")
def scenes(cvr):
    return {k: cvr.Scene.synthetic(n, 0, d) for k, (n, d) in SCENES.items()}


def make_ctx(cvr, scene, kernel="regenerationSK", seed=7, opts=(), fmt=0):
    ctx = cvr.Context(0, kernel)
    for k, v in opts:
        ctx.set_option(k, v)
    if fmt:
        ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
    if scene.is_sparse:
        ctx.set_medium_sparse(scene.sparse_medium)
    else:
        ctx.set_medium(scene.medium)
    iv, r2v = cvr.default_camera(W, H)
    ctx.set_camera(iv, r2v, (W, H))
    ctx.set_resolution(W, H)
    ctx.set_offset(0, 0)
    ctx.set_seed(seed)
    ctx.init()
    return ctx, iv, r2v


def half_oracle(cvr, oracle_mod, scene, md_eff):
    """The fp32 oracle of the cvr_half_round()ed medium with the majorant in use."""
    if scene.is_sparse:
        table, dens, alb, bg = scene.leaves()
        d = scene.sparse_medium
        return oracle_mod.Oracle.from_leaves(scene.dims, table, cvr.half_round(dens).reshape(-1, 512),
                                             None if alb is None else cvr.half_round(alb).reshape(-1, 512, 4),
                                             tuple(float(v) for v in cvr.half_round(np.array(bg, np.float32))),
                                             tuple(d.box_min), tuple(d.box_max), d.scale, md_eff, d.g,
                                             tuple(d.roughness), d.eta)
    m = scene.medium
    return oracle_mod.Oracle(cvr.half_round(scene.density), cvr.half_round(scene.albedo), tuple(m.box_min),
                             tuple(m.box_max), m.scale, md_eff, m.g, tuple(m.roughness), m.eta)


def trace(orc, L, n_samples):
    """The oracle's records of samples [0, n_samples) of the tile, traced in parallel chunks."""
    n = P * n_samples
    step = (n + NTHREADS - 1) // NTHREADS
    with ThreadPoolExecutor(NTHREADS) as ex:
        parts = list(ex.map(lambda a: orc.trace_paths(L, a, min(step, n - a)), range(0, n, step)))
    return np.concatenate(parts)


class Sums:
    """Per pixel, after every sample count: sum T, sum fl32(T T) and the escapes, summed sample
    by sample in fp32 (each sample touches a pixel once)."""

    def __init__(self, recs, n_samples):
        assert len(recs) == P * n_samples
        s1 = np.zeros((P, 3), np.float32)
        s2 = np.zeros((P, 3), np.float32)
        cnt = np.zeros(P, np.int64)
        self.s1, self.s2, self.cnt = [s1.copy()], [s2.copy()], [cnt.copy()]
        for s in range(n_samples):
            r = recs[s * P:(s + 1) * P]
            esc = (r["flags"] & 1) != 0
            ids = r["image_id"][esc]
            assert len(np.unique(ids)) == len(ids)
            T = r["T"][esc].astype(np.float32)
            s1[ids] += T
            s2[ids] += T * T
            cnt[ids] += 1
            self.s1.append(s1.copy())
            self.s2.append(s2.copy())
            self.cnt.append(cnt.copy())


def block_pixels(b):
    by, bx = divmod(b, W // 8)
    yy, xx = np.meshgrid(np.arange(8) + 8 * by, np.arange(8) + 8 * bx, indexing="ij")
    return (yy * W + xx).ravel()


BLOCK_PIX = [block_pixels(b) for b in range(NB)]


def metric_close(a, b):
    if np.isinf(a) or np.isinf(b):
        return a == b
    return abs(a - b) <= ATOL + RTOL * abs(b)


# ------------------------------------------------- 1. moments vs the oracle --
MOMENT_CASES = [
    ("bucky", "regenerationSK", 1, 0),
    ("bucky", "naiveSK", 1, 0),       # the scatter -eps instance
    ("bucky", "streamingSK", 1, 0),
    ("bucky", "regenerationSK", 0, 0),  # no density cells: the 8-tap gathers of the generic instance
    ("manix_small", "regenerationSK", 1, 0),
    ("manix_small", "naiveSK", 1, 1),   # the half format, read at run time
    ("cloud", "regenerationSK", 1, 0),  # the fp32 sparse instance
    ("cloud", "naiveSK", 1, 0),
]


@pytest.mark.parametrize("scene_key,kernel,cells,fmt", MOMENT_CASES)
def test_moments_match_oracle(cvr, oracle_mod, scenes, scene_key, kernel, cells, fmt):
    scene = scenes[scene_key]
    iters = 5
    ctx, iv, r2v = make_ctx(cvr, scene, kernel, opts=((cvr.OPT_CELLS, cells),), fmt=fmt)
    try:
        ctx.set_iterations(iters)
        ctx.set_option(cvr.OPT_MOMENTS, 1)
        ctx.clear_output()
        ctx.launch_render()
        st = ctx.stats()
        s1, s2 = ctx.copy_moments()
        orc = (half_oracle(cvr, oracle_mod, scene, ctx.medium_info().max_density_eff) if fmt
               else oracle_for_scene(oracle_mod, scene))
        L = orc.launch(iv, r2v, (W, H), (W, H), (0, 0), cvr.KERNELS.index(kernel), 7)
        ref = Sums(trace(orc, L, iters), iters)
        what = f"{scene_key} {kernel} cells={cells} fmt={fmt}"
        n = ref.cnt[iters]
        assert n.max() > 1
        got_n = s2.reshape(P, 4)[:, 3]
        assert (got_n == n.astype(np.float32)).all(), f"{what}: escape counts differ"
        assert st.escaped == n.sum()
        assert_sums_close(s1.reshape(P, 4)[:, :3], ref.s1[iters], n, what + ": sum T")
        assert_sums_close(s2.reshape(P, 4)[:, :3], ref.s2[iters], n, what + ": sum T^2")
        assert (s1.reshape(P, 4)[:, 3] == (n > 0)).all()
        # the framebuffer half and the counters are those of the same launch without moments
        ctx.set_option(cvr.OPT_MOMENTS, 0)
        ctx.clear_output()
        ctx.launch_render()
        st0 = ctx.stats()
        plain = ctx.copy_output(W, H)
        assert_sums_close(s1.reshape(P, 4)[:, :3], plain.reshape(P, 4)[:, :3], n, what + ": moments off")
        for k in COUNTERS + ("fetches",):
            assert getattr(st, k) == getattr(st0, k), f"{what}: counter {k}"
        with pytest.raises(cvr.CvrError) as e:
            ctx.copy_moments()
        assert e.value.code == -3
    finally:
        ctx.close()


# -------------------------------------- 2. the subset launch changes no path --
def test_never_stopping_session_is_the_plain_render(cvr, scenes):
    scene = scenes["bucky"]
    ctx, _, _ = make_ctx(cvr, scene)
    ref, _, _ = make_ctx(cvr, scene)
    try:
        with ctx.adaptive(cvr.AdaptiveDesc(8, 16, 4, -1.0, 0.01)) as a:
            res = a.step()
            assert (res.passes, res.blocks, res.blocks_active, res.paths, res.done) == (1, NB, NB, P * 8, 0)
            assert not a.step().done
            res = a.step()
            assert (res.passes, res.blocks_active, res.paths, res.done) == (3, 0, P * 16, 1)
            err, smp = a.maps()
            img = a.image()
            s1, _ = ctx.copy_moments()
        assert (smp == 16).all() and np.isfinite(err).all() and (err >= 0).all()
        assert a.stats.paths == P * 16
        ref.set_iterations(16)
        ref.clear_output()
        ref.launch_render()
        st = ref.stats()
        plain = ref.copy_output(W, H)
        n = np.full(P, 16)
        assert_sums_close(s1.reshape(P, 4)[:, :3], plain.reshape(P, 4)[:, :3], n, "subset launches")
        assert_sums_close(img.reshape(P, 4)[:, :3], (plain / np.float32(16)).reshape(P, 4)[:, :3], n, "image")
        for k in COUNTERS + ("fetches",):
            assert getattr(a.stats, k) == getattr(st, k), k
        ref.reset()
        assert ctx.get_seed() == ref.get_seed() == (7 + P * 16) & 0xFFFFFFFF
        assert ctx.resolution == (W, H)
    finally:
        ctx.close()
        ref.close()


# ------------------------------------ 3 + 4. stepwise decisions, final image --
STEP_CASES = {"bucky": 0.1, "manix_small": 0.02}
MAX_IT = 32


@pytest.fixture(scope="module")
def step_refs(cvr, oracle_mod, scenes):
    """Per scene: the oracle's sums after every sample count up to MAX_IT (seed 7, default camera)."""
    out = {}
    iv, r2v = cvr.default_camera(W, H)
    for key in STEP_CASES:
        orc = oracle_for_scene(oracle_mod, scenes[key])
        L = orc.launch(iv, r2v, (W, H), (W, H), (0, 0), 2, 7)
        out[key] = Sums(trace(orc, L, MAX_IT), MAX_IT)
    return out


def check_image(img, smp, ref, what):
    """Every block's pixels are the oracle's first n_b samples divided by n_b."""
    img = img.reshape(P, 4)
    for b in range(NB):
        nb = int(smp.ravel()[b])
        pix = BLOCK_PIX[b]
        want = ref.s1[nb][pix] / np.float32(nb)
        assert_sums_close(img[pix, :3], want, np.full(64, nb), f"{what}: block {b} at {nb} samples")


@pytest.mark.parametrize("scene_key", list(STEP_CASES))
def test_stepwise_decisions(cvr, scenes, step_refs, scene_key):
    target = STEP_CASES[scene_key]
    ctx, _, _ = make_ctx(cvr, scenes[scene_key])
    try:
        exempt = 0
        active = set(range(NB))
        prev = None
        stops = {}
        with ctx.adaptive(cvr.AdaptiveDesc(8, MAX_IT, 4, target, 0.01)) as a:
            with pytest.raises(cvr.CvrError) as e:  # a render call inside the session
                ctx.launch_render()
            assert e.value.code == -3 and "adaptive session" in str(e.value)
            while True:
                res = a.step()
                s1, s2 = ctx.copy_moments()
                err, smp = a.maps()
                s1f, s2f, errf, smpf = s1.reshape(P, 4), s2.reshape(P, 4), err.ravel(), smp.ravel()
                N = 8 + 4 * (res.passes - 1)
                # the blocks this pass sampled are exactly the ones expected to be active
                grew = {b for b in range(NB) if smpf[b] == N}
                assert grew == active, (res.passes, grew ^ active)
                if prev is not None:  # a stopped block's sums never change again, bitwise
                    for b in set(range(NB)) - grew:
                        pix = BLOCK_PIX[b]
                        assert (s1f[pix].view(np.uint32) == prev[0][pix].view(np.uint32)).all(), b
                        assert (s2f[pix].view(np.uint32) == prev[1][pix].view(np.uint32)).all(), b
                prev = (s1f.copy(), s2f.copy())
                nxt = set()
                for b in sorted(grew):
                    pix = BLOCK_PIX[b]
                    model = cvr.block_error(s1f[pix], s2f[pix], N, 0.01)
                    assert metric_close(errf[b], model), (b, N, errf[b], model)
                    if abs(model - target) <= 1e-6:
                        exempt += 1
                        if errf[b] > target and N < MAX_IT:  # either decision is right: follow the device's
                            nxt.add(b)
                        else:
                            stops[b] = N
                    elif model > target and N < MAX_IT:
                        nxt.add(b)
                    else:
                        stops[b] = N
                assert exempt <= 1, "more than one block within 1e-6 of the target"
                active = nxt
                assert res.blocks_active == len(active)
                assert res.paths == 64 * int(smpf.sum())
                assert metric_close(res.max_error, errf.max()) and metric_close(res.mean_error, errf.mean())
                assert res.done == (0 if active else 1)
                if res.done:
                    break
            with pytest.raises(cvr.CvrError) as e:  # a pass after done
                a.step()
            assert e.value.code == -3 and "done" in str(e.value)
            img = a.image()
            _, smp = a.maps()
        counts = np.array([stops[b] for b in range(NB)])
        print(f"{scene_key}: stops", {int(k): int((counts == k).sum()) for k in np.unique(counts)}, "passes", res.passes)
        assert (counts == 8).sum() >= 20
        assert ((counts > 8) & (counts < MAX_IT)).sum() >= 2
        assert (counts == MAX_IT).sum() >= 16
        assert (smp.ravel() == counts).all()
        check_image(img, smp, step_refs[scene_key], scene_key)
        assert ctx.get_seed() == (7 + P * MAX_IT) & 0xFFFFFFFF
    finally:
        ctx.close()


@pytest.mark.parametrize("scene_key,pinned", [("bucky", True), ("manix_small", False)])
def test_render_adaptive_image(cvr, scenes, step_refs, scene_key, pinned):
    ctx, _, _ = make_ctx(cvr, scenes[scene_key])
    pin = cvr.PinnedImage(W, H) if pinned else None
    try:
        if pin:
            pin.array[:] = np.nan
        img, res, err, smp = ctx.render_adaptive(cvr.AdaptiveDesc(8, MAX_IT, 4, STEP_CASES[scene_key], 0.01), pin)
        img = np.array(img, copy=True)
        assert res.done == 1 and res.blocks == NB and res.blocks_active == 0
        assert res.paths == 64 * int(smp.sum()) == ctx.adaptive_stats.paths
        assert smp.min() >= 8 and smp.max() == MAX_IT and (smp % 4 == 0).all()
        assert res.paths < P * MAX_IT
        stopped = smp.ravel() < MAX_IT
        assert (err.ravel()[stopped] <= STEP_CASES[scene_key]).all()
        check_image(img, smp, step_refs[scene_key], scene_key)
        assert ctx.get_seed() == (7 + P * MAX_IT) & 0xFFFFFFFF
    finally:
        if pin:
            pin.close()
        ctx.close()


# ------------------------------------------------------------- 5. refusals --
def plain_ok(cvr, ctx, orc, iv, r2v, kernel, what, seed=7):
    """The context still renders a plain image correctly (2 iterations against the oracle)."""
    iters = 2
    ctx.set_resolution(W, H)
    ctx.set_iterations(iters)
    ctx.set_seed(seed)
    ctx.clear_output()
    ctx.launch_render()
    st = ctx.stats()
    img = ctx.copy_output(W, H)
    L = orc.launch(iv, r2v, (W, H), (W, H), (0, 0), cvr.KERNELS.index(kernel), seed)
    ref, rst = orc.render(L, 0, P * iters, nthreads=NTHREADS)
    assert_counters_equal(st, rst, what)
    assert_sums_close(img.reshape(P, 4)[:, :3], ref.reshape(P, 4)[:, :3], np.full(P, iters), what)


def refused(cvr, fn, code, *words):
    with pytest.raises(cvr.CvrError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(cvr, oracle_mod, scenes):
    scene = scenes["bucky"]
    orc = oracle_for_scene(oracle_mod, scene)
    desc = cvr.AdaptiveDesc(8, 16, 4, 0.1, 0.01)
    UNSUP, STATE, INVALID = -5, -3, -1

    def begin(ctx):
        with ctx.adaptive(desc):
            pass

    ctx, iv, r2v = make_ctx(cvr, scene)
    other, _, _ = make_ctx(cvr, scene)
    try:
        # a 60x64 tile
        ctx.set_resolution(60, 64)
        refused(cvr, lambda: begin(ctx), UNSUP, "multiples of 8")
        plain_ok(cvr, ctx, orc, iv, r2v, "regenerationSK", "after 60x64")
        # a block shard
        ctx.set_block_shard(0, 2)
        refused(cvr, lambda: begin(ctx), UNSUP, "block shard")
        ctx.set_block_shard(0, 1)
        plain_ok(cvr, ctx, orc, iv, r2v, "regenerationSK", "after shard")
        # a path range
        ctx.set_iterations(4)
        ctx.set_path_range(P, P)
        refused(cvr, lambda: begin(ctx), UNSUP, "path range")
        ctx.set_path_range(0, 2 ** 64 - 1)
        # a caller's output buffer, with the session and with the option
        ctx.set_output(other.output_ptr())
        refused(cvr, lambda: begin(ctx), UNSUP, "output buffer")
        refused(cvr, lambda: ctx.set_option(cvr.OPT_MOMENTS, 1), UNSUP, "output buffer")
        ctx.set_output(None)
        ctx.set_option(cvr.OPT_MOMENTS, 1)
        refused(cvr, lambda: ctx.set_output(other.output_ptr()), UNSUP, "moments")
        refused(cvr, lambda: ctx.render_image(W, H, (1, 1), 2), UNSUP, "cvr_render_image")
        refused(cvr, lambda: ctx.render_frame(), UNSUP, "cvr_render_frame")
        refused(cvr, lambda: ctx.trace_launch(P * 4), UNSUP, "cvr_trace_launch")
        refused(cvr, lambda: ctx.set_option(cvr.OPT_MOMENTS, 2), INVALID)
        ctx.set_option(cvr.OPT_MOMENTS, 0)
        plain_ok(cvr, ctx, orc, iv, r2v, "regenerationSK", "after output buffer")
        # another scheduler, with the session and with the option
        ctx.set_option(cvr.OPT_SCHEDULER, 0)
        refused(cvr, lambda: begin(ctx), UNSUP, "scheduler")
        ctx.set_option(cvr.OPT_MOMENTS, 1)
        ctx.set_iterations(2)
        refused(cvr, ctx.launch_render, UNSUP, "scheduler")
        ctx.set_option(cvr.OPT_MOMENTS, 0)
        plain_ok(cvr, ctx, orc, iv, r2v, "regenerationSK", "scheduler 0")  # the persistent kernel itself
        ctx.set_option(cvr.OPT_SCHEDULER, 3)
        # bad descriptors
        for bad in (cvr.AdaptiveDesc(1, 16, 1, 0.1, 0.01), cvr.AdaptiveDesc(8, 18, 4, 0.1, 0.01),
                    cvr.AdaptiveDesc(6, 16, 4, 0.1, 0.01), cvr.AdaptiveDesc(8, 4, 4, 0.1, 0.01),
                    cvr.AdaptiveDesc(8, 16, 0, 0.1, 0.01), cvr.AdaptiveDesc(8, 16, 4, 0.1, -1.0)):
            with pytest.raises(cvr.CvrError) as e:
                with ctx.adaptive(bad):
                    pass
            assert e.value.code == INVALID
        # inside a session: render and option calls, then a pass after done
        with ctx.adaptive(desc) as a:
            refused(cvr, ctx.launch_render, STATE, "adaptive session")
            refused(cvr, lambda: ctx.set_option(cvr.OPT_MOMENTS, 0), STATE, "adaptive session")
            refused(cvr, lambda: ctx.render_frame(), STATE, "adaptive session")
            refused(cvr, lambda: ctx.set_iterations(3), STATE, "adaptive session")
            refused(cvr, lambda: begin(ctx), STATE, "already open")
            while not a.step().done:
                pass
            refused(cvr, a.step, STATE, "done")
            ctx.synchronize()
            assert ctx.stats().paths > 0
        refused(cvr, lambda: ctx._c(cvr.load().cvr_adaptive_pass(ctx._h, None)), STATE, "no adaptive session")
        refused(cvr, lambda: ctx._c(cvr.load().cvr_adaptive_end(ctx._h)), STATE, "no adaptive session")
        plain_ok(cvr, ctx, orc, iv, r2v, "regenerationSK", "after a session", seed=ctx.get_seed())
    finally:
        ctx.close()
        other.close()

    # naiveMK
    ctx, iv, r2v = make_ctx(cvr, scene, "naiveMK")
    try:
        refused(cvr, lambda: begin(ctx), UNSUP, "naiveMK")
        ctx.set_option(cvr.OPT_MOMENTS, 1)
        ctx.set_iterations(2)
        refused(cvr, ctx.launch_render, UNSUP, "naiveMK")
        ctx.set_option(cvr.OPT_MOMENTS, 0)
        plain_ok(cvr, ctx, orc, iv, r2v, "naiveMK", "naiveMK")
    finally:
        ctx.close()

    # a sparse half medium
    cloud = scenes["cloud"]
    ctx, iv, r2v = make_ctx(cvr, cloud, fmt=1)
    try:
        refused(cvr, lambda: begin(ctx), UNSUP, "sparse half")
        ctx.set_option(cvr.OPT_MOMENTS, 1)
        ctx.set_iterations(2)
        refused(cvr, ctx.launch_render, UNSUP, "sparse half")
        ctx.set_option(cvr.OPT_MOMENTS, 0)
        horc = half_oracle(cvr, oracle_mod, cloud, ctx.medium_info().max_density_eff)
        plain_ok(cvr, ctx, horc, iv, r2v, "regenerationSK", "sparse half")
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6. CLI --
def test_cli_noise_target(cvr, scenes, tmp_path):
    out = str(tmp_path / "adaptive")
    r = subprocess.run([CLI, "--interactive", "0", "--synthetic", "bucky", "-r", "64", "64", "-i", "32",
                        "--noise-target", "0.1", "-o", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert os.path.getsize(out + ".hdr") > 0 and os.path.getsize(out + "_samples.hdr") > 0
    m = re.search(r"adaptive render\s*: (\d+) passes, (\d+) paths traced \(([\d.]+)% of the uniform render's (\d+)\)",
                  r.stdout)
    assert m, r.stdout
    # the library's own run of the same render (the CLI's seed 0 and scene camera)
    scene = scenes["bucky"]
    ctx = cvr.Context(0, "regenerationSK")
    try:
        ctx.set_seed(0)
        ctx.set_medium(scene.medium)
        iv, r2v = scene.camera(W, H)
        ctx.set_camera(iv, r2v, (W, H))
        ctx.set_resolution(W, H)
        ctx.init()
        _, res, _, smp = ctx.render_adaptive(cvr.AdaptiveDesc(8, 32, 4, 0.1, 0.01))
    finally:
        ctx.close()
    assert (int(m.group(1)), int(m.group(2)), int(m.group(4))) == (res.passes, res.paths, P * 32)
    assert abs(float(m.group(3)) - 100.0 * res.paths / (P * 32)) <= 0.05
    assert res.paths == 64 * int(smp.sum()) < P * 32
