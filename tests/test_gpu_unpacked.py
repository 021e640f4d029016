"""The wave-pool kernels without packed fp32 render the bits they rendered with it.

cvr_wpool.hip is compiled with SLP vectorisation off and trilerp_cell uses plain
lerps: per component the same IEEE operations in the same
order, so nothing may change.  Every medium layout whose fetch block or register
allocation changed runs here against the CPU oracle: per-path records of the
production launch bit for bit (the record instances), the counters of a plain
launch and of the in-launch-output launch equal, their pixels within the
summation-order bound (parity_util).

Layouts: the default dense one (cells + brick bounds), the generic dense
instance (CVR_OPT_BOUNDS 0: wpool_select maps a dense medium without bounds to
kMedDense), a dense medium with a uniform albedo, a sparse medium, and the half
format dense and sparse.  Shapes are the smallest that still fetch cells and
run mixed event batches: the bucky proxy (32^3), the 19x13x11 uniform-albedo
grid and the 20x12x28 sparse index box of tests/media.py, 64x64 pixels, 2
iterations.  Each case asserts stats.fetches > 0 and stats.albedo > 0: a case
that never reaches the trilinear code proves nothing (a real collision needs a
fetched cell, so the oracle's albedo count shows it on the CPU:
tests/test_wpool_unpacked.py)."""
import functools

import numpy as np
import pytest

from media import SCALE, dense_arrays, sparse_arrays, sparse_desc
from parity_util import NTHREADS, assert_counters_equal, assert_pixels_close, gpu_range_render

W = H = 64
ITERS = 2
N = W * H * ITERS
SEED = 0
KID = 2  # regenerationSK
CASES = ("dense", "dense_generic", "dense_uniform", "sparse", "half_dense", "half_sparse")


def _md_eff(cvr, md):
    """The half format's majorant: max(max_density, f32(f16(max_density)))."""
    return max(float(np.float32(md)), float(cvr.half_round(np.array([md], np.float32))[0]))


def build_case(cvr, oracle_mod, name):
    """(configure(ctx) -> keep-alive objects, oracle) of a case; the oracle of a half case is
    the fp32 oracle of the rounded medium (tests/test_gpu_half_medium.py)."""
    half = name.startswith("half")
    rnd = cvr.half_round if half else (lambda a: a)
    if name.endswith("sparse"):
        res, table, dens, alb, bg, md = sparse_arrays(True)

        def configure(ctx):
            desc, keep = sparse_desc(cvr, res, table, dens, alb, bg, md)
            ctx.set_medium_sparse(desc)
            return desc, keep
        orc = oracle_mod.Oracle.from_leaves(res, table, rnd(dens), rnd(alb),
                                            tuple(float(v) for v in rnd(np.array(bg, np.float32))), scale=SCALE,
                                            max_density=_md_eff(cvr, md) if half else md)
        return configure, orc
    if name == "dense_uniform":
        d, a, md = dense_arrays("max", uniform=True)
        desc, keep = cvr.medium_from_arrays(d, a, scale=SCALE, max_density=md)
    else:
        scene = cvr.Scene.synthetic("bucky")
        d, a, md = np.array(scene.density), np.array(scene.albedo), scene.medium.max_density
        desc, keep = scene.medium, scene

    def configure(ctx):
        if name == "dense_generic":
            ctx.set_option(cvr.OPT_BOUNDS, 0)
        ctx.set_medium(desc)
        return desc, keep
    orc = oracle_mod.Oracle(rnd(d), rnd(a), tuple(desc.box_min), tuple(desc.box_max), desc.scale,
                            _md_eff(cvr, md) if half else md, desc.g, tuple(desc.roughness), desc.eta)
    return configure, orc


@functools.lru_cache(maxsize=None)
def reference(cvr, oracle_mod, name):
    """The oracle's records, unnormalised image and counters of a case's N paths (computed once)."""
    configure, orc = build_case(cvr, oracle_mod, name)
    iv, r2v = cvr.default_camera(W, H)
    L = orc.launch(iv, r2v, (W, H), (W, H), (0, 0), KID, SEED)
    rec = orc.trace_paths(L, 0, N)
    img, st = orc.render(L, 0, N, nthreads=NTHREADS)
    for a in (rec, img):
        a.setflags(write=False)
    return configure, iv, r2v, rec, img, st.as_dict()


def assert_reaches_the_trilinear_code(rec, stats, what):
    assert stats["albedo"] > 0 and stats["density"] > 0, what       # real collisions: cells were interpolated
    assert (rec["flags"] & 1).any() and (rec["flags"] == 0).any(), what  # escapes and roulette deaths: mixed batches


def _compare_records(g, c, what):
    assert len(g) == len(c)
    for f in ("image_id", "flags", "n_segments"):
        mism = np.nonzero(g[f] != c[f])[0]
        assert mism.size == 0, f"{what}: {f} differs for {mism.size} paths, first {mism[:5]}"
    both_nan = np.isnan(g["T"]) & np.isnan(c["T"])
    mism = np.nonzero(((g["T"].view(np.uint32) != c["T"].view(np.uint32)) & ~both_nan).any(axis=1))[0]
    assert mism.size == 0, f"{what}: T bits differ for {mism.size} paths, first {mism[:5]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_unpacked_layout_bit_exact(cvr, oracle_mod, name):
    configure, iv, r2v, rec, ref, rst = reference(cvr, oracle_mod, name)
    assert_reaches_the_trilinear_code(rec, rst, name)
    ctx = cvr.Context(0, "regenerationSK")
    if name.startswith("half"):
        ctx.set_option(cvr.OPT_MEDIUM_FORMAT, cvr.FORMAT_F16)
    keep = configure(ctx)  # noqa: F841  (the arrays behind the descriptor)
    ctx.set_camera(iv, r2v, (W, H))
    ctx.init()
    pin = cvr.PinnedImage(W, H)
    try:
        # the record instance: every path's record bit for bit
        ctx.set_resolution(W, H)
        ctx.set_offset(0, 0)
        ctx.set_iterations(ITERS)
        ctx.set_seed(SEED)
        ctx.set_path_range(0, N)
        _compare_records(ctx.trace_launch(N), rec, f"{name}: records")
        # the plain instance: counters equal, pixels within the summation-order bound
        acc, st = gpu_range_render(ctx, (W, H), (0, 0), ITERS, SEED, 0, N)
        print(f"{name}: fetches {st.fetches} density {st.density} albedo {st.albedo} steps {st.steps}")
        assert st.fetches > 0 and st.albedo > 0, f"{name}: never reached the trilinear code"
        assert_counters_equal(st, rst, f"{name}: launch")
        assert_pixels_close(acc[..., :3], ref[..., :3], ITERS, f"{name}: launch")
        # the in-launch-output instance (cvr_render_frame)
        ctx.set_seed(SEED)
        pin.array[:] = np.nan
        _, fst = ctx.render_frame(pin, 1)
        print(f"{name}: frame flush info {ctx.frame_flush_info()}")
        assert fst.fetches == st.fetches
        assert_counters_equal(fst, rst, f"{name}: render_frame")
        assert_pixels_close(pin.array[..., :3].copy(), ref[..., :3] / np.float32(ITERS), ITERS, f"{name}: render_frame")
    finally:
        pin.close()
        ctx.close()
