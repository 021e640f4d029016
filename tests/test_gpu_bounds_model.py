"""Brick bounds, cell fetches and brick words against the CPU model (tests/bounds_model.py).

The bound tables (k_build_bounds, k_build_sparse_bounds), the empty-region mask and the fetch
decision cannot be read back; what they decide can: cvr_stats.fetches must equal the model's
count over the oracle's evaluation log, for the whole launch and for each quarter of its path
ids, and cvr_stats.words of the counting launch must lie within the model's bounds.  Each
case uploads one of the media of tests/media.py, renders path ids [0, 8192) with the record
instance (cvr_trace_launch) and with the plain launch, and asserts records bit-equal to the
oracle, the seven counters equal, and the fetches equal to the model's.  What makes the media
sharp (a code one step off, a window one voxel short, a full mask all change the expected
numbers) is checked on the CPU in tests/test_bounds_model.py.

Format 1 (half storage) does not run the counting instance or the schedulers other than the
wave pool (CVR_ERR_UNSUPPORTED), so those cases are format 0 only."""
import numpy as np
import pytest

import bounds_model as bm
import bounds_ref as br
import media
from parity_util import assert_counters_equal

pytestmark = pytest.mark.gpu

KERNEL_IDS = {"naiveSK": 0, "naiveMK": 1, "regenerationSK": 2}


def compare_records(g, c, what, counts=False):
    assert len(g) == len(c)
    fields = ("image_id", "flags", "n_segments") + (("n_steps", "n_density", "n_albedo") if counts else ())
    for f in fields:
        mism = np.nonzero(g[f] != c[f])[0]
        assert mism.size == 0, f"{what}: {f} differs for {mism.size} paths, first {mism[:5]}"
    tb, cb = g["T"].view(np.uint32), c["T"].view(np.uint32)
    both_nan = np.isnan(g["T"]) & np.isnan(c["T"])
    mism = np.nonzero(((tb != cb) & ~both_nan).any(axis=1))[0]
    assert mism.size == 0, f"{what}: T bits differ for {mism.size} paths, first {mism[:5]}"
    assert (c["flags"] & 1).any() and (c["n_albedo"] > 0).any(), what  # escapes and real collisions


def make_ctx(cvr, name, kernel="regenerationSK", fmt=0, q4=0, opts=()):
    """A context over the unrounded medium `name` (format 1 rounds it on upload)."""
    m = br.medium(name)
    ctx = cvr.Context(0, kernel)
    ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
    ctx.set_option(cvr.OPT_WORLD_TO_AABB, q4)
    for k, v in opts:
        ctx.set_option(k, v)
    if isinstance(m, media.Dense):
        desc, keep = cvr.medium_from_arrays(m.density, m.albedo, m.box_min, m.box_max, m.scale, m.max_density)
        ctx.set_medium(desc)
    else:
        desc, keep = media.sparse_desc(cvr, m.res, m.table, m.leaf_density, m.leaf_albedo, m.albedo_bg, m.max_density)
        ctx.set_medium_sparse(desc)
    full, offset = br.view(name)
    iv, r2v = br.camera(full)
    ctx.set_camera(iv, r2v, full)
    ctx.init()
    ctx.set_resolution(*br.TILE)
    ctx.set_offset(*offset)
    ctx.set_iterations(br.ITERS)
    ctx.set_seed(br.SEED)
    return ctx


def launch(ctx, first, count):
    ctx.set_seed(br.SEED)
    ctx.set_path_range(first, count)
    ctx.clear_output()
    ctx.launch_render()
    return ctx.stats()


def check_case(ctx, ref, want, want_quarters, what, records="launch"):
    """records: "launch" the wave pool's record instance, "paths" the debug kernel (with counts)."""
    if records == "launch":
        ctx.set_path_range(0, br.N)
        compare_records(ctx.trace_launch(br.N), ref.records, what + ": trace_launch")
    else:
        compare_records(ctx.trace_paths(0, br.N), ref.records, what + ": trace_paths", counts=True)
    st = launch(ctx, 0, br.N)
    print(f"{what}: fetches {st.fetches} (model {want}), density {st.density} (oracle {ref.stats['density']})")
    assert_counters_equal(st, ref.stats, what)
    assert st.fetches == want, f"{what}: fetches {st.fetches}, model {want}"
    got = [launch(ctx, a, b - a).fetches for a, b in br.QUARTERS]
    print(f"{what}: quarter fetches {got} (model {want_quarters})")
    assert got == want_quarters, f"{what}: quarter fetches {got}, model {want_quarters}"
    return st


# ------------------------------------------------------- dense wave pool ----
DENSE_CASES = [("staircase", 0), ("spikes", 0), ("random40", 0), ("offgrid", 0), ("offgrid", 1)]


@pytest.mark.parametrize("cells", [1, 0])
@pytest.mark.parametrize("bounds", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("name,q4", DENSE_CASES)
def test_dense_fetches_equal_the_model(cvr, name, q4, bounds, cells):
    ref = br.reference(name, 0, q4)
    want, quarters = br.expected(name, 0, q4, 2, bounds)
    if bounds == 0:
        assert want == ref.stats["density"]
    ctx = make_ctx(cvr, name, q4=q4, opts=((cvr.OPT_BOUNDS, bounds), (cvr.OPT_CELLS, cells)))
    assert (ctx.medium_info().cells_bytes > 0) == bool(cells)
    assert (ctx.medium_info().bounds_bytes > 0) == bool(bounds)
    check_case(ctx, ref, want, quarters, f"{name} q4 {q4} bounds {bounds} cells {cells}")
    ctx.close()


@pytest.mark.parametrize("name", ["staircase", "spikes"])
def test_dense_half_format(cvr, name):
    ref = br.reference(name, 1)
    want, quarters = br.expected(name, 1)
    ctx = make_ctx(cvr, name, fmt=1)
    assert ctx.medium_info().max_density_eff == np.float32(br.medium(name, 1).max_density)
    check_case(ctx, ref, want, quarters, f"{name} half")
    ctx.close()


@pytest.mark.parametrize("kernel", ["naiveSK", "naiveMK"])
def test_dense_other_kernel_ids(cvr, kernel):
    """naiveSK (scatter -eps) and naiveMK (re-seeded segments) walk other paths over the same table."""
    kid = KERNEL_IDS[kernel]
    ref = br.reference("staircase", 0, 0, kid)
    assert ref.records.tobytes() != br.reference("staircase").records.tobytes()
    want, quarters = br.expected("staircase", 0, 0, kid)
    ctx = make_ctx(cvr, "staircase", kernel)
    # cvr_trace_launch does not trace naiveMK: its records come from the debug kernel
    check_case(ctx, ref, want, quarters, f"staircase {kernel}", records="paths" if kernel == "naiveMK" else "launch")
    ctx.close()


@pytest.mark.parametrize("scheduler", [0, 4])
def test_dense_other_schedulers(cvr, scheduler):
    """The persistent kernel and one path per work-item make the same fetch decisions."""
    ref = br.reference("staircase")
    want, quarters = br.expected("staircase")
    ctx = make_ctx(cvr, "staircase", opts=((cvr.OPT_SCHEDULER, scheduler),))
    check_case(ctx, ref, want, quarters, f"staircase scheduler {scheduler}", records="paths")
    ctx.close()


# ------------------------------------------------------ sparse wave pool ----
def sparse_opts(cvr, bounds, emask, count_words=0):
    opts = [(cvr.OPT_EMPTY_MASK, emask), (cvr.OPT_COUNT_WORDS, count_words)]
    if bounds is not None:
        opts.append((cvr.OPT_BOUNDS, bounds))
    return tuple(opts)


@pytest.mark.parametrize("emask", [1, 0])
@pytest.mark.parametrize("bounds", [None, 1, 2, 0])
@pytest.mark.parametrize("name,fmt", [("sparse_small", 0), ("sparse_small", 1), ("sparse_es4", 0)])
def test_sparse_fetches_and_words(cvr, name, fmt, bounds, emask):
    ref = br.reference(name, fmt)
    want, quarters = br.expected(name, fmt, 0, 2, bounds)
    if bounds == 0:
        assert want == ref.stats["density"]
    what = f"{name} format {fmt} bounds {bounds} mask {emask}"
    ctx = make_ctx(cvr, name, fmt=fmt, opts=sparse_opts(cvr, bounds, emask))
    st = check_case(ctx, ref, want, quarters, what)
    assert st.words == 0  # only the counting instance counts
    ctx.close()
    if fmt:
        return
    # the counting instance: the same launch, and its words within the model's bounds
    m = br.medium(name)
    es, mask = bm.sparse_mask(m.table)
    masked = emask and bounds != 0  # an unbounded medium has no mask: its empty words are not 0
    lo, hi, segs = bm.word_bounds(ref.evals, ref.records, ref.res, want, mask if masked else None, es)
    inside = int(bm.in_grid(ref.evals, ref.res).sum())
    ctx = make_ctx(cvr, name, opts=sparse_opts(cvr, bounds, emask, 1))
    st = launch(ctx, 0, br.N)
    print(f"{what}: words {st.words}, model [{lo}, {hi}] ({segs} segments, {inside} in-grid evaluations)")
    assert_counters_equal(st, ref.stats, what + " counting")
    assert st.fetches == want
    assert lo <= st.words <= hi, f"{what}: words {st.words} outside [{lo}, {hi}]"
    if masked and name == "sparse_es4":
        assert hi < inside  # so a mask with every bit set (words >= inside) cannot pass
    if not masked:
        assert lo == inside
    ctx.close()
