"""Every wave-pool kernel instance the library ships, run against the oracle (tests/wpool_matrix.py: one
entry per row of kWpoolTable; tests/test_wpool_matrix_cpu.py holds the entries against the table).

Per entry and case (box_all, inside_all of tests/params.py on the 16^3 blob), one context, two launches,
each on a grid of 8 waves (64 for cvr_render_frame's in-launch output, which needs more than 32), so that
every lane ends paths and is refilled many times: the refill, the regeneration burst and the drain run in
every instance, with whatever the instance adds at a path's end.

  1. 128x128 pixels x 1 sample (16384 paths, at least 256 per wave).  A pixel receives at most one
     contribution, so no order of additions is involved and everything is compared as uint32, without a
     tolerance: the framebuffer (the pinned image, S1 and S2 of the moments, the records, an environment's
     contributions through cvr_trace_env's chain as in tests/test_gpu_envmap.py), the counters, the word
     counts within the bounds of tests/bounds_model.py.
  2. the case's own 32x32 pixels x 4 samples, with the summation-order bound of tests/parity_util.py for
     each pixel's own number of contributions.

Before the first launch cvr_debug_last_wpool is CVR_ERR_STATE; after each it must name the entry's
declared instance and the grid asked for: a configuration that degrades to another row fails.

The oracle's records are traced once per (case, kernel id, medium variant, launch) and shared; the guards
against a vacuous pass (wpool_matrix.check_guards) hold for every reference made."""
import numpy as np
import pytest

import bounds_model as bm
import params
import wpool_matrix as wm
from envmap_util import ROT, env_image, record_sums
from params_ref import assert_frame, blob_leaves, sparse_blob
from parity_util import assert_counters_equal, assert_pixels_close, assert_sums_close
from test_gpu_records import _compare as compare_records

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def refs(cvr, oracle_mod):
    return wm.Refs(oracle_mod, cvr.half_round)


@pytest.fixture(scope="module")
def env():
    """(map, rotation) of tests/test_gpu_envmap.py's chain."""
    return env_image(64, 32), ROT


def make_ctx(cvr, e, case):
    p = params.medium_params(case)
    ctx = cvr.Context(0, e.kernel)
    try:
        ctx.set_option(cvr.OPT_WORLD_TO_AABB, case.w2a)
        ctx.set_option(cvr.OPT_GRID, wm.grid_of(e))
        for k, v in e.opts:
            ctx.set_option(getattr(cvr, k), v)
        if e.entry == "frame":
            ctx.set_option(cvr.OPT_FRAME_FLUSH, 1)
        blob = wm.upload_arrays(e.medium)
        if e.sparse:
            desc, keep = sparse_blob(cvr, blob, p)
            ctx.set_medium_sparse(desc)
        else:
            desc, keep = cvr.medium_from_arrays(blob[0], blob[1], p["box_min"], p["box_max"], params.SCALE,
                                                params.MAX_DENSITY, p["g"], p["roughness"], p["eta"])
            ctx.set_medium(desc)
        ctx._keep = (desc, keep, blob)
        if e.medium.endswith("half"):
            assert ctx.medium_info().max_density_eff == np.float32(wm.md_eff(cvr.half_round))
        ctx.init()
    except BaseException:
        ctx.close()
        raise
    return ctx


def set_launch(ctx, case, samples):
    cam = params.camera(case.camera, case.full)
    ctx.set_camera(cam.inv_view, cam.r2v, case.full)
    ctx.set_resolution(*case.tile)
    ctx.set_offset(*case.offset)
    ctx.set_iterations(samples)
    ctx.set_seed(params.SEED)
    ctx.set_path_range(0, params.n_paths(case, samples))


def assert_instance(ctx, e, n, what, per_wave=0):
    inst, grid = ctx.last_wpool()
    assert inst == e.instance, f"{what}: ran {inst}, the entry declares {e.instance}"
    assert grid == wm.grid_of(e), f"{what}: a grid of {grid} waves"
    assert n // grid >= per_wave, f"{what}: {n} paths on {grid} waves"


def scattered(image_id, values, px):
    """zeros + values at their pixels (ids distinct): what one atomic add per pixel leaves."""
    out = np.zeros((px,) + values.shape[1:], np.float32)
    assert len(np.unique(image_id)) == len(image_id)
    out[image_id] += values
    return out


# ------------------------------------------------------------------ the entry points --
def run_launch(cvr, ctx, e, case, samples, ref, what, refs, case_name):
    one = samples == 1
    px = case.tile[0] * case.tile[1]
    n = params.n_paths(case, samples)
    ctx.clear_output()
    ctx.launch_render()
    st = ctx.stats()
    assert_instance(ctx, e, n, what, wm.MIN_PATHS_PER_WAVE if one else 0)
    if wm.opt(e, "OPT_MOMENTS"):
        s1, s2 = ctx.copy_moments()
        s1, s2 = s1.reshape(px, 4), s2.reshape(px, 4)
        assert (s2[:, 3] == ref.cnt.astype(np.float32)).all(), f"{what}: escape counts differ"
        assert_frame(s1, st, ref, what + ": sum T")
        assert_sums_close(s2[:, :3], ref.s2, ref.cnt, what + ": sum T^2")
        if one:
            assert np.array_equal(bits(s1[:, :3]), bits(ref.s1)), f"{what}: S1 bits"
            assert np.array_equal(bits(s2[:, :3]), bits(ref.s2)), f"{what}: S2 bits"
        return
    out = ctx.copy_output(*case.tile).reshape(px, 4)
    assert_frame(out, st, ref, what)
    if one:
        assert np.array_equal(bits(out[:, :3]), bits(ref.s1)), f"{what}: framebuffer bits"
    if wm.opt(e, "OPT_COUNT_WORDS"):
        assert st.words > 0, what
        if one:
            check_words(cvr, e, st, ref, refs.evals(case_name, e.kernel, e.medium), what)
        # the same launch with the option off counts nothing (and runs the plain sparse instance)
        ctx.set_option(cvr.OPT_COUNT_WORDS, 0)
        ctx.clear_output()
        ctx.launch_render()
        st0 = ctx.stats()
        ctx.set_option(cvr.OPT_COUNT_WORDS, 1)
        assert st0.words == 0, f"{what}: words {st0.words} with the option off"
        assert_counters_equal(st0, ref.counters, what + " (not counting)")
        assert ctx.last_wpool()[0] == e.instance[:2] + (e.instance[2] & ~8,) + e.instance[3:]


def check_words(cvr, e, st, ref, evals, what):
    """cvr_stats.words within the model's bounds, as tests/test_gpu_bounds_model.py computes them: the
    default brick shift of a sparse medium, its empty-region mask on."""
    density, albedo, md = wm.medium_arrays(e.medium, cvr.half_round)
    table, dens, _ = blob_leaves((density, albedo))
    res = (16, 16, 16)
    bshift = bm.sparse_bshift(None)
    want = bm.expected_fetches(evals, res, bm.sparse_codes(res, table, dens, md, bshift), bshift)
    es, mask = bm.sparse_mask(table)
    lo, hi, segs = bm.word_bounds(evals, ref.recs, res, want, mask, es)
    print(f"{what}: words {st.words}, model [{lo}, {hi}] ({segs} segments); fetches {st.fetches}, model {want}")
    assert st.fetches == want, f"{what}: fetches {st.fetches}, model {want}"
    assert lo <= st.words <= hi, f"{what}: words {st.words} outside [{lo}, {hi}]"


def run_frame(cvr, ctx, e, case, samples, ref, what):
    px = case.tile[0] * case.tile[1]
    buf = cvr.PinnedImage(*case.tile)
    try:
        buf.array[:] = np.nan
        _, st = ctx.render_frame(buf, 1)
        img = buf.array.copy().reshape(px, 4)
    finally:
        buf.close()
    assert_instance(ctx, e, params.n_paths(case, samples), what, wm.MIN_PATHS_PER_WAVE if samples == 1 else 0)
    assert ctx.frame_flush_info() == ((case.tile[0] // 8) * (case.tile[1] // 8), 0), what
    assert_frame(img, st, ref, what, scale=samples, exact_w=samples == 1)
    if samples == 1:  # (the division by one sample is exact)
        assert np.array_equal(bits(img[:, :3]), bits(ref.s1)), f"{what}: image bits"


def run_trace(ctx, e, case, samples, ref, what):
    n = params.n_paths(case, samples)
    g = ctx.trace_launch(n)
    assert_instance(ctx, e, n, what, wm.MIN_PATHS_PER_WAVE if samples == 1 else 0)
    compare_records(g, ref.recs, what)


def run_env(ctx, e, case, samples, ref, what, env):
    img, rot = env
    one = samples == 1
    px = case.tile[0] * case.tile[1]
    n = params.n_paths(case, samples)
    ctx.set_environment(img, 1.0, rot)
    # cvr_trace_env's walk is the oracle's ...
    rec = ctx.trace_env(0, n)
    c = ref.recs
    for f in ("image_id", "flags", "n_segments"):
        assert np.array_equal(rec[f], c[f]), f"{what}: trace_env {f}"
    assert np.array_equal(bits(rec["T"]), bits(c["T"])), f"{what}: trace_env T"
    esc = (rec["flags"] & 1) == 1
    assert (rec["C"][~esc] == 0).all() and (rec["C"][esc] != c["T"][esc]).any(), what
    # ... and the production instance's framebuffer is its contributions
    ctx.clear_output()
    ctx.launch_render()
    st = ctx.stats()
    assert_instance(ctx, e, n, what, wm.MIN_PATHS_PER_WAVE if one else 0)
    assert_counters_equal(st, ref.counters, what)
    C32 = rec["C"].astype(np.float32)
    moments = bool(wm.opt(e, "OPT_MOMENTS"))
    if moments:
        s1, s2 = ctx.copy_moments()
        fb, s2 = s1.reshape(px, 4), s2.reshape(px, 4)
        assert (s2[:, 3] == ref.cnt.astype(np.float32)).all(), f"{what}: escape counts differ"
    else:
        fb = ctx.copy_output(*case.tile).reshape(px, 4)
    assert (fb[:, 3] == (ref.cnt > 0)).all(), f"{what}: w channel"
    if one:
        assert np.array_equal(bits(fb[:, :3]), bits(scattered(rec["image_id"][esc], C32[esc], px))), f"{what}: C bits"
        if moments:
            want2 = scattered(rec["image_id"][esc], (C32 * C32)[esc], px)
            assert np.array_equal(bits(s2[:, :3]), bits(want2)), f"{what}: S2 bits"
        return
    # (record_sums takes the samples in pixel order)
    assert np.array_equal(rec["image_id"].reshape(samples, px), np.tile(np.arange(px), (samples, 1))), what
    shape = (case.tile[1], case.tile[0], 3)
    assert_pixels_close(fb[:, :3].reshape(shape).astype(np.float64), record_sums(rec, case.tile, samples), samples, what)
    if moments:
        assert_pixels_close(s2[:, :3].reshape(shape).astype(np.float64),
                            record_sums(rec, case.tile, samples, square=True), samples, what + ": moments")


# --------------------------------------------------------------------------- the matrix --
@pytest.mark.parametrize("case_name", wm.CASES)
@pytest.mark.parametrize("entry", [e.name for e in wm.ENTRIES])
def test_instance_against_the_oracle(cvr, refs, env, entry, case_name):
    e = wm.BY_NAME[entry]
    ctx = make_ctx(cvr, e, params.CASES[case_name])
    try:
        with pytest.raises(cvr.CvrError) as err:
            ctx.last_wpool()
        assert err.value.code == -3  # CVR_ERR_STATE: no wave-pool launch yet
        for which in ("one", "acc"):
            case, samples = wm.launch_case(case_name, which)
            ref = refs.get(case_name, e.kernel, e.medium, which)
            what = f"{entry} {case_name} launch {which}"
            set_launch(ctx, case, samples)
            if e.entry == "launch":
                run_launch(cvr, ctx, e, case, samples, ref, what, refs, case_name)
            elif e.entry == "frame":
                run_frame(cvr, ctx, e, case, samples, ref, what)
            elif e.entry == "trace":
                run_trace(ctx, e, case, samples, ref, what)
            else:
                assert e.entry == "env"
                run_env(ctx, e, case, samples, ref, what, env)
    finally:
        ctx.close()
