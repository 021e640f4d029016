"""The wave pool's regeneration phase (csrc/cvr_wpool.hip, kBurst instances) against the oracle.

Camera paths are made in bursts across the whole wave before an event batch chooses its items:
a path that hits the box takes a free slot, a path that misses ends in the phase with no slot,
and when more paths hit than slots are free the burst commits a prefix and the cursor goes back
(csrc/cvr_regen_plan.h, tests/test_regen_plan.py).  That is scheduling: every path id is still
made exactly once, so per case
  1. the record instance's records (cvr_trace_launch) equal the oracle's bit for bit: image id,
     flags, segment count, the three T words;
  2. a plain launch's counters equal the sums over those records, and its pixels the per-pixel
     sums within 2 (n - 1) 2^-24 max(|gpu|, |cpu|) + 1e-30, n the pixel's own contributions.
Every case runs regenerationSK on the default scheduler with a dense medium and no moments,
environment or in-launch output, which is a kBurst instance, and asserts that the launch's
paths counter is the number of path ids asked for: they were all made, by the phase.

Medium and launch are tests/params.py's: the 16^3 blob, 32x32 pixels x 4 samples = 4096 paths.
Cameras: every ray misses (a pencil beside the box: the image is exactly the sample count);
every ray hits the front face from outside (with one wave, CVR_OPT_GRID 1, the pool's 115 slots
fill up and nearly every burst then has more hits than free slots: prefix commit and rewind);
the eye inside the box (hits go to the ready ring, no boundary event first); the default mix.
The oracle traces each camera's 4096 paths once per module; cases take slices of them."""
import numpy as np
import pytest

import params
from parity_util import COUNTERS, assert_counters_equal
from test_gpu_adaptive import assert_sums_close
from test_gpu_params import assert_records_equal

pytestmark = pytest.mark.gpu

N = params.W * params.H * params.SAMPLES
PX = params.W * params.H
KID = 2  # regenerationSK
CASE = params.CASES["default"]

CAMERAS = {
    "all_miss": lambda: params.camera("pencil_out"),
    # the eye 3.5 from the front face, half-angle 2.5 degrees: the image's corner reaches 0.22 < 0.5
    "all_hit": lambda: params.look_at((0, 0, 4), (0, 0, 0), fov=5.0),
    "inside": lambda: params.camera("inside"),
    "mix": lambda: params.camera("front"),
}


class Refs:
    def __init__(self, oracle_mod):
        self.oracle_mod = oracle_mod
        self.blob = params.blob16()
        self.cache = {}

    def get(self, cam):
        if cam not in self.cache:
            orc = params.make_oracle(self.oracle_mod, CASE, *self.blob)
            L = params.make_launch(self.oracle_mod, CASE, KID, cam=CAMERAS[cam]())
            recs = orc.trace_paths(L, 0, N)
            recs.setflags(write=False)
            self.cache[cam] = recs
        return self.cache[cam]


@pytest.fixture(scope="module")
def refs(oracle_mod):
    return Refs(oracle_mod)


def test_the_cameras_are_what_the_cases_need(refs):
    """From the oracle alone: all_miss and all_hit are total, inside starts inside (a path's first
    segment is then a Woodcock walk: steps before any boundary), mix has both kinds."""
    esc1 = {k: ((refs.get(k)["flags"] & 1) != 0) & (refs.get(k)["n_segments"] == 1) for k in CAMERAS}
    assert esc1["all_miss"].all()
    assert not esc1["all_hit"].any() and not esc1["inside"].any()
    assert 0.1 * N < esc1["mix"].sum() < 0.6 * N
    assert (refs.get("all_hit")["n_steps"] > 0).any() and (refs.get("inside")["n_steps"] > 0).mean() > 0.9


def expected(recs, ids):
    """Counters and per-pixel sums of the paths `ids` (added in path order, in fp32)."""
    r = recs[ids]
    esc = (r["flags"] & 1) != 0
    s1 = np.zeros((PX, 3), np.float32)
    cnt = np.zeros(PX, np.int64)
    np.add.at(s1, r["image_id"][esc], r["T"][esc].astype(np.float32))
    np.add.at(cnt, r["image_id"][esc], 1)
    counters = dict(paths=len(r), segments=int(r["n_segments"].sum()), steps=int(r["n_steps"].sum()),
                    density=int(r["n_density"].sum()), albedo=int(r["n_albedo"].sum()), escaped=int(esc.sum()),
                    truncated=int(((r["flags"] & 2) != 0).sum()))
    assert set(counters) == set(COUNTERS)
    return counters, s1, cnt


def make_ctx(cvr, refs, cam, opts):
    p = params.medium_params(CASE)
    c = CAMERAS[cam]()
    ctx = cvr.Context(0, "regenerationSK")
    for k, v in opts:
        ctx.set_option(getattr(cvr, k), v)
    desc, keep = cvr.medium_from_arrays(refs.blob[0], refs.blob[1], p["box_min"], p["box_max"], params.SCALE,
                                        params.MAX_DENSITY, p["g"], p["roughness"], p["eta"])
    ctx.set_medium(desc)
    ctx._keep = (desc, keep)
    ctx.set_camera(c.inv_view, c.r2v, CASE.full)
    ctx.set_resolution(*CASE.tile)
    ctx.set_offset(0, 0)
    ctx.set_iterations(params.SAMPLES)
    ctx.set_seed(params.SEED)
    ctx.init()
    return ctx


def run_case(cvr, refs, cam, opts=(), first=0, count=N, shard=None, what=""):
    """Records, then counters and pixels, of path ids [first, first + count) (shard: (rank, world),
    the block shard of that range, which must be whole samples)."""
    recs = refs.get(cam)
    what = f"{what or cam} {dict(opts)} [{first}, +{count}) shard {shard}"
    ctx = make_ctx(cvr, refs, cam, opts)
    try:
        ctx.set_path_range(first, count)
        if shard:
            from cudavolumerenderer_amd.distributed import block_shard_path_ids
            assert first == 0 and count == N
            ctx.set_block_shard(*shard)
            ids = np.asarray(block_shard_path_ids(params.W, params.H, params.SAMPLES, *shard))
            assert 0 < len(ids) < N
        else:
            ids = np.arange(first, first + count)
        g = ctx.trace_launch(count)
        assert_records_equal(g[ids - first], recs[ids], ("image_id", "flags", "n_segments"), what)
        if shard:
            rest = np.ones(count, bool)
            rest[ids - first] = False
            assert (g["n_segments"][rest] == 0).all(), f"{what}: paths outside the shard were made"
        ctx.clear_output()
        ctx.launch_render()
        out, st = ctx.copy_output(*CASE.tile).reshape(PX, 4), ctx.stats()
        counters, s1, cnt = expected(recs, ids)
        assert st.paths == len(ids), f"{what}: {st.paths} paths made of {len(ids)}"  # the phase ran
        assert_counters_equal(st, counters, what)
        assert_sums_close(out[:, :3], s1, cnt, what)
        assert (out[:, 3] == (cnt > 0)).all(), f"{what}: w channel"
        return out, st, cnt
    finally:
        ctx.close()


ONE_WAVE = (("OPT_GRID", 1),)


@pytest.mark.parametrize("grid", ["occupancy", "one_wave"])
@pytest.mark.parametrize("cam", list(CAMERAS))
def test_hit_rates(cvr, refs, cam, grid):
    out, st, cnt = run_case(cvr, refs, cam, ONE_WAVE if grid == "one_wave" else ())
    if cam == "all_miss":
        # no path ever takes a slot: one segment each, no step, and the image is the sample count
        assert st.segments == N and st.steps == 0 and st.escaped == N
        assert (out[:, :3] == np.float32(params.SAMPLES)).all()
    if cam in ("all_hit", "inside"):
        assert st.steps > 0 and st.segments > N


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("cam", ["mix", "all_hit"])
def test_path_counts(cvr, refs, cam, count):
    run_case(cvr, refs, cam, ONE_WAVE, 0, count)


@pytest.mark.parametrize("order", [0, 1])
def test_unaligned_range(cvr, refs, order):
    """A range that starts and ends inside a sample: the launch falls back to path-id order."""
    run_case(cvr, refs, "mix", (("OPT_SAMPLE_ORDER", order),), 1237, 2222)


@pytest.mark.parametrize("order", [0, 1])
def test_block_shard(cvr, refs, order):
    run_case(cvr, refs, "mix", (("OPT_SAMPLE_ORDER", order),), shard=(1, 3))


@pytest.mark.parametrize("grid", ["occupancy", "one_wave"])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("cam", ["mix", "all_miss", "all_hit"])
def test_sample_order(cvr, refs, cam, order, grid):
    """Order 1 puts a pixel's samples on neighbouring lanes and sums a burst's misses per pixel
    before the framebuffer atomics (in free slots borrowed from the stack); order 0 splats per lane."""
    opts = (("OPT_SAMPLE_ORDER", order),) + (ONE_WAVE if grid == "one_wave" else ())
    run_case(cvr, refs, cam, opts)


@pytest.mark.parametrize("chunk", [37, 100])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("cam", ["mix", "all_hit", "all_miss"])
def test_chunk_ends_and_exhaustion(cvr, refs, cam, order, chunk):
    """One wave, chunks that are no multiple of the burst width: the wave crosses a chunk end in
    most bursts (the second burst of a phase), dequeues 4096 / chunk times and meets the end of
    the last, short chunk, and then exhaustion, in mid-burst."""
    assert 64 % chunk != 0 and chunk % 64 != 0 and N % chunk != 0
    run_case(cvr, refs, cam, (("OPT_GRID", 1), ("OPT_CHUNK", chunk), ("OPT_SAMPLE_ORDER", order)))
