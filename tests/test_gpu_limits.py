"""GPU == oracle at the limits of the walk's 24- and 32-bit index arithmetic, and refusals past them.

The kernels index cells, bricks and brick words with 24-bit multiplies, path ids and queue heads with
32 bits, and pixels through a float; only the host guards (cvr_set_medium, cvr_set_medium_sparse,
cvr_set_resolution, cvr_set_iterations, the launch) keep the operands in range.  The cases of
tests/limits.py sit on the accepted side of each guard (tests/test_limits_cpu.py shows on the oracle's
evaluation log that the large products really occur) and are compared with the oracle under the
suite's contract: records bit-equal (cvr_trace_paths and the production wave pool's cvr_trace_launch),
counters equal, pixels within the fp32 summation-order bound (tests/parity_util.py).  The shapes just
past each guard must be refused with the stated code and a text that names the limit, before any array
is read (the descriptors point at one-element dummies), and leave the context usable."""
import ctypes as C
import time

import numpy as np
import pytest

import limits
import media
import params
from parity_util import NTHREADS, assert_counters_equal, assert_pixels_close, gpu_range_render
from test_gpu_params import Ref, assert_frame, assert_records_equal
from test_limits_cpu import check_fastdiv

pytestmark = pytest.mark.gpu

TRACE_FIELDS = ("image_id", "flags", "n_segments", "n_steps", "n_density", "n_albedo")
LAUNCH_FIELDS = ("image_id", "flags", "n_segments")
REF_CASE = params.CASES["default"]   # 32x32 pixels x 4 samples: the geometry of Ref


class Media:
    """The medium cases: the oracle's records of each (kept), and the arrays of the last one used
    (up to 0.7 GB: one at a time)."""

    def __init__(self, oracle_mod):
        self.oracle_mod = oracle_mod
        self.refs = {}
        self.last = (None, None)

    def case(self, name):
        if self.last[0] != name:
            self.last = (None, None)
            self.last = (name, limits.MEDIA[name]())
        return self.last[1]

    def ref(self, name):
        if name not in self.refs:
            case = self.case(name)
            orc = limits.make_oracle(self.oracle_mod, case)
            self.refs[name] = Ref(orc.trace_paths(limits.make_launch(self.oracle_mod, case), 0, limits.N_PATHS),
                                  REF_CASE)
        return self.refs[name]


@pytest.fixture(scope="module")
def med(oracle_mod):
    return Media(oracle_mod)


def medium_ctx(cvr, case, opts=(), fmt=0, kernel="regenerationSK"):
    ctx = cvr.Context(0, kernel)
    try:
        if case.bound_shift is not None:
            ctx.set_option(cvr.OPT_BOUNDS, case.bound_shift)
        for k, v in opts:
            ctx.set_option(getattr(cvr, k), v)
        if fmt:
            ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
        m = case.medium
        if case.kind == "sparse":
            desc, keep = media.sparse_desc(cvr, m.res, m.table, m.leaf_density, m.leaf_albedo, m.albedo_bg,
                                           m.max_density)
            desc.box_min[:] = case.box_min
            desc.box_max[:] = case.box_max
            desc.scale = case.scale
            ctx.set_medium_sparse(desc)
        else:
            desc, keep = cvr.medium_from_arrays(m.density, m.albedo, case.box_min, case.box_max, case.scale,
                                                m.max_density)
            ctx.set_medium(desc)
        cam = limits.camera(case)
        ctx.set_camera(cam.inv_view, cam.r2v, (limits.W, limits.H))
        ctx.set_resolution(limits.W, limits.H)
        ctx.set_iterations(limits.SAMPLES)
        ctx.set_seed(limits.SEED)
        ctx.init()
    except BaseException:
        ctx.close()
        raise
    return ctx


def launch_all(ctx):
    ctx.set_path_range(0, limits.N_PATHS)
    ctx.clear_output()
    ctx.launch_render()
    return ctx.copy_output(limits.W, limits.H), ctx.stats()


def check_medium(ctx, ref, what, traced=True):
    """Framebuffer and counters of a plain launch; and, on the wave pool, the production records."""
    out, st = launch_all(ctx)
    assert_frame(out, st, ref, what)
    if traced:
        ctx.set_path_range(0, limits.N_PATHS)
        assert_records_equal(ctx.trace_launch(limits.N_PATHS), ref.recs, LAUNCH_FIELDS, what + " trace_launch")
    return st


# ------------------------------------------------------------- media at the limit --
@pytest.mark.parametrize("name", list(limits.MEDIA))
def test_medium_at_limit(cvr, med, name):
    """The default instance: whole debug records, production records, framebuffer and counters."""
    ctx = medium_ctx(cvr, med.case(name))
    try:
        ref = med.ref(name)
        assert_records_equal(ctx.trace_paths(0, limits.N_PATHS), ref.recs, TRACE_FIELDS, name + " trace_paths")
        st = check_medium(ctx, ref, name)
        assert 0 < st.fetches < st.density   # the brick bounds settle some evaluations
    finally:
        ctx.close()


VARIANTS = {
    # id: (options, format, wave pool)
    "cells0": ((("OPT_CELLS", 0),), 0, True),
    "bounds0": ((("OPT_BOUNDS", 0),), 0, True),
    "half": ((), 1, True),
    "sched0": ((("OPT_SCHEDULER", 0),), 0, False),
    "sched4": ((("OPT_SCHEDULER", 4),), 0, False),
}
# bounds off builds a sparse medium's brick words at 4^3 cells: the grids of sparse_xy_limit and
# sparse_long_z, sized for 8^3, are then past the limit (test_sparse_refusals); sparse_xy_limit_b2 is
# the case at it
AT_8_ONLY = ("sparse_xy_limit", "sparse_long_z")
VARIANT_CASES = [(n, v) for n in limits.MEDIA for v in ("cells0", "bounds0") if not (n in AT_8_ONLY and v == "bounds0")]
VARIANT_CASES += [(n, "half") for n in ("dense_xy_limit", "dense_yz_limit", "sparse_xy_limit")]
VARIANT_CASES += [(n, v) for n in ("sparse_xy_limit", "dense_xy_limit") for v in ("sched0", "sched4")]


@pytest.mark.parametrize("name,variant", sorted(VARIANT_CASES))
def test_medium_variants(cvr, med, name, variant):
    opts, fmt, wpool = VARIANTS[variant]
    case = med.case(name)
    if variant == "bounds0" and case.bound_shift is not None:
        case = case._replace(bound_shift=None)
    ctx = medium_ctx(cvr, case, opts, fmt)
    try:
        ref = med.ref(name)   # (the media are exact in binary16: the same oracle for format 1)
        if fmt:
            assert ctx.medium_info().format == 1 and ctx.medium_info().max_density_eff == 1.0
        st = check_medium(ctx, ref, f"{name} {variant}", traced=wpool)
        if variant == "bounds0":
            assert st.fetches == st.density
        if variant in ("cells0", "half"):
            assert_records_equal(ctx.trace_paths(0, limits.N_PATHS), ref.recs, TRACE_FIELDS,
                                 f"{name} {variant} trace_paths")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", limits.SPARSE)
def test_mask_on_and_off(cvr, med, name):
    """The empty-region mask skips only words that are known: the same records and fetches."""
    fetches = []
    for mask in (1, 0):
        ctx = medium_ctx(cvr, med.case(name), (("OPT_EMPTY_MASK", mask),))
        try:
            fetches.append(check_medium(ctx, med.ref(name), f"{name} mask {mask}").fetches)
        finally:
            ctx.close()
    assert fetches[0] == fetches[1]


# ---------------------------------------------------------- launches at the limit --
class Blob:
    def __init__(self, oracle_mod):
        self.arrays = params.blob16()
        self.orc = params.make_oracle(oracle_mod, REF_CASE, *self.arrays)
        self.oracle_mod = oracle_mod

    def launch(self, cam, tile, seed, kernel=2):
        return self.oracle_mod.Oracle.launch(cam.inv_view, cam.r2v, tile, tile, (0, 0), kernel, seed)


@pytest.fixture(scope="module")
def blob(oracle_mod):
    return Blob(oracle_mod)


def blob_ctx(cvr, blob, cam, tile, iterations, seed=limits.SEED, opts=()):
    p = params.medium_params(REF_CASE)
    ctx = cvr.Context(0, "regenerationSK")
    try:
        for k, v in opts:
            ctx.set_option(getattr(cvr, k), v)
        desc, keep = cvr.medium_from_arrays(blob.arrays[0], blob.arrays[1], p["box_min"], p["box_max"], params.SCALE,
                                            params.MAX_DENSITY, p["g"], p["roughness"], p["eta"])
        ctx.set_medium(desc)
        ctx._keep = (desc, keep)
        ctx.set_camera(cam.inv_view, cam.r2v, tile)
        ctx.set_resolution(*tile)
        ctx.set_iterations(iterations)
        ctx.set_seed(seed)
        ctx.init()
    except BaseException:
        ctx.close()
        raise
    return ctx


def assert_count_image(ctx, tile, samples):
    """An all-miss launch adds (1, 1, 1) per path: integer sums below 2^24, exact in any order, so a
    unit mapped twice, never or to the wrong pixel changes an integer."""
    n = tile[0] * tile[1] * samples
    ctx.set_path_range(0, n)
    ctx.clear_output()
    ctx.launch_render()
    st = ctx.stats()
    out = ctx.copy_output(*tile)
    assert st.paths == n and st.escaped == n and st.segments == n
    wrong = np.nonzero((out[..., :3] != np.float32(samples)).any(axis=-1).ravel())[0]
    assert wrong.size == 0, f"{wrong.size} pixels do not hold {samples}: first {wrong[:4]}, {out.reshape(-1, 4)[wrong[:4]]}"
    return st


@pytest.mark.parametrize("name", list(limits.TILES))
def test_tile_count_image(cvr, blob, name):
    tile = limits.TILES[name]
    ctx = blob_ctx(cvr, blob, params.camera("pencil_out"), tile, 1)
    try:
        assert ctx.launch_blocks()[0] == tile[0] * tile[1] // 64   # the pixel-block order
        assert_count_image(ctx, tile, 1)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(limits.TILES))
def test_tile_hit_launch(cvr, blob, name):
    """A few percent of the rays hit blob16: the whole framebuffer against the oracle (the float pixel
    row of camera_ray at 2^24 pixels), and the records of the first and last 4096 ids."""
    tile = limits.TILES[name]
    n = tile[0] * tile[1]
    cam = limits.tile_hit_camera(tile)
    L = blob.launch(cam, tile, limits.SEED)
    t0 = time.time()
    ref, rst = blob.orc.render(L, 0, n, nthreads=NTHREADS)
    print(f"{name}: oracle render {time.time() - t0:.1f} s")
    assert 1.01 * n < rst.segments < 1.5 * n and rst.density > 0, "a few percent of the rays should hit blob16"
    ctx = blob_ctx(cvr, blob, cam, tile, 1)
    try:
        out, st = gpu_range_render(ctx, tile, (0, 0), 1, limits.SEED, 0, n)
        assert_counters_equal(st, rst, name)
        assert_pixels_close(out, ref, 1, name)
        for first in (0, n - 4096):
            assert_records_equal(ctx.trace_paths(first, 4096), blob.orc.trace_paths(L, first, 4096), TRACE_FIELDS,
                                 f"{name} ids {first}..")
    finally:
        ctx.close()


@pytest.mark.parametrize("rng", list(limits.TOP_RANGES))
def test_top_path_ids(cvr, blob, rng):
    """Path ids up to 2^32 - 65 (tile 24x8, 22 369 621 iterations): unit_to_path, path_begin's
    id / tile_px and the seed sum in u32."""
    first, count = limits.TOP_RANGES[rng]
    tile = limits.TOP_TILE
    cam = params.camera("front", tile)
    L = blob.launch(cam, tile, limits.SEED)
    ctx = blob_ctx(cvr, blob, cam, tile, limits.TOP_ITERATIONS)
    try:
        out, st = gpu_range_render(ctx, tile, (0, 0), limits.TOP_ITERATIONS, limits.SEED, first, count)
        assert ctx.launch_blocks()[0] == (3 if rng == "last_samples" else 0)   # block order / path-id order
        ref, rst = blob.orc.render(L, first, count)
        assert rst.paths == count and rst.density > 0
        assert_counters_equal(st, rst, rng)
        assert_pixels_close(out, ref, -(-count // 192), rng)
        recs = blob.orc.trace_paths(L, first, count)
        assert_records_equal(ctx.trace_paths(first, count), recs, TRACE_FIELDS, rng + " trace_paths")
        assert_records_equal(ctx.trace_launch(count), recs, LAUNCH_FIELDS, rng + " trace_launch")
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", [limits.SEED_SIGN, limits.SEED_WRAP])
def test_seed_crossings(cvr, blob, seed):
    """seed + path id crosses 2^31 (the sign-extended half of Q3 mid-launch) or 2^32 (the u32 wrap) at
    id 256; one cvr_reset from the wrapping seed wraps too."""
    tile = REF_CASE.tile
    cam = params.camera("front", tile)
    n = limits.N_PATHS
    ctx = blob_ctx(cvr, blob, cam, tile, limits.SAMPLES, seed)
    try:
        for s in (seed, (seed + n) & 0xFFFFFFFF):
            ref = Ref(blob.orc.trace_paths(blob.launch(cam, tile, s), 0, n), REF_CASE)
            assert ctx.get_seed() == s
            assert_records_equal(ctx.trace_paths(0, n), ref.recs, TRACE_FIELDS, f"seed {s:#x} trace_paths")
            ctx.set_path_range(0, n)
            assert_records_equal(ctx.trace_launch(n), ref.recs, LAUNCH_FIELDS, f"seed {s:#x} trace_launch")
            ctx.clear_output()
            ctx.launch_render()
            assert_frame(ctx.copy_output(*tile), ctx.stats(), ref, f"seed {s:#x}")
            if seed != limits.SEED_WRAP:
                break
            ctx.reset()   # regenerationSK: seed += n_paths, in u32
    finally:
        ctx.close()


@pytest.mark.parametrize("order", [0, 1])
def test_max_samples_count_image(cvr, blob, order):
    """2^20 samples in one block-ordered launch (unit_to_path's rem << 6 at 2^32 - 64), then 2^20 + 1,
    which must fall back to path-id order."""
    tile = limits.MAX_SAMPLES_TILE
    ctx = blob_ctx(cvr, blob, params.camera("pencil_out"), tile, limits.MAX_SAMPLES, opts=(("OPT_SAMPLE_ORDER", order),))
    try:
        assert ctx.launch_blocks()[0] == 1
        assert_count_image(ctx, tile, limits.MAX_SAMPLES)
        ctx.set_iterations(limits.MAX_SAMPLES + 1)
        ctx.set_path_range(0, 64 * (limits.MAX_SAMPLES + 1))
        assert ctx.launch_blocks()[0] == 0
        assert_count_image(ctx, tile, limits.MAX_SAMPLES + 1)
    finally:
        ctx.close()


def test_max_samples_records_and_frame(cvr, blob):
    """Ids from the middle and the end of the 2^26-path launch against the oracle, and one
    cvr_render_frame of it: the in-launch block count reaches its largest quota, 2^26."""
    tile = limits.MAX_SAMPLES_TILE
    n = 64 * limits.MAX_SAMPLES
    cam = params.camera("front", tile)
    L = blob.launch(cam, tile, limits.SEED)
    ctx = blob_ctx(cvr, blob, cam, tile, limits.MAX_SAMPLES)
    try:
        for first in (n // 2 - 2048, n - 4096):
            assert_records_equal(ctx.trace_paths(first, 4096), blob.orc.trace_paths(L, first, 4096), TRACE_FIELDS,
                                 f"max_samples ids {first}..")
    finally:
        ctx.close()
    ctx = blob_ctx(cvr, blob, params.camera("pencil_out"), tile, limits.MAX_SAMPLES)
    buf = cvr.PinnedImage(*tile)
    try:
        buf.array[:] = np.nan
        _, st = ctx.render_frame(buf, 1)
        assert ctx.frame_flush_info() == (1, 0)   # stored by the launch's flushers, no fallback copy
        assert st.paths == n and st.escaped == n
        assert (buf.array[..., :3] == 1.0).all()   # 2^20 / 2^20
    finally:
        buf.close()
        ctx.close()


def test_fastdiv_device(cvr):
    """cvr::fastdiv itself, in a trivial kernel, on the (d, u) sets of the host test."""
    check_fastdiv(cvr, 1)


# ------------------------------------------------------------------ past the limit --
INVALID, UNSUPPORTED = -1, -5


def dummy_dense(cvr, res):
    """A descriptor of `res` voxels over one-element arrays: valid only for calls that refuse it
    before they read."""
    from cudavolumerenderer_amd._lib import MediumDesc
    d, a = np.zeros(1, np.float32), np.ones(4, np.float32)
    m = MediumDesc()
    m.res[:] = res
    m.density = d.ctypes.data_as(C.POINTER(C.c_float))
    m.albedo = a.ctypes.data_as(C.POINTER(C.c_float))
    m.box_min[:] = (-0.5,) * 3
    m.box_max[:] = (0.5,) * 3
    m.scale, m.max_density, m.g, m.eta = 100.0, 1.0, 0.0, 1.04
    m.roughness[:] = (0.1, 0.1)
    return m, (d, a)


def dummy_sparse(cvr, leaf_dims, table=None, n_leaves=0):
    from cudavolumerenderer_amd._lib import SparseMediumDesc
    t = np.full(1, limits.NO_LEAF, np.uint32) if table is None else table
    d = np.zeros(512, np.float32)
    s = SparseMediumDesc()
    s.res[:] = [8 * v for v in leaf_dims]
    s.leaf_dims[:] = leaf_dims
    s.leaf_table = t.ctypes.data_as(C.POINTER(C.c_uint32))
    s.n_leaves = n_leaves
    s.leaf_density = d.ctypes.data_as(C.POINTER(C.c_float))
    s.albedo_background[:] = limits.ALBEDO_BG
    s.box_min[:] = (-0.5,) * 3
    s.box_max[:] = (0.5,) * 3
    s.scale, s.max_density, s.g, s.eta = 100.0, 1.0, 0.0, 1.04
    s.roughness[:] = (0.1, 0.1)
    return s, (t, d)


def refused(cvr, call, code, *words):
    with pytest.raises(cvr.CvrError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), f"the message does not name the limit ({w}): {e.value}"


@pytest.fixture()
def usable(cvr, blob):
    """A context rendering blob16, and a check that it still does, equal to the oracle."""
    tile = REF_CASE.tile
    cam = params.camera("front", tile)
    ctx = blob_ctx(cvr, blob, cam, tile, limits.SAMPLES)
    ref = Ref(blob.orc.trace_paths(blob.launch(cam, tile, limits.SEED), 0, limits.N_PATHS), REF_CASE)

    def check(reload_medium=False):
        if reload_medium:
            ctx.set_medium(ctx._keep[0])
        ctx.set_iterations(limits.SAMPLES)
        ctx.set_resolution(*tile)
        out, st = launch_all(ctx)
        assert_frame(out, st, ref, "after the refusal")

    yield ctx, check
    ctx.close()


DENSE_REFUSALS = {
    # res, options, code, words of the message
    "xy_2_24": ((4096, 4096, 1), (), UNSUPPORTED, ("2^24",)),
    "yz_2_24": ((1, 4096, 4096), (), UNSUPPORTED, ("2^24",)),
    "voxels_2_32": ((65536, 1, 65536), (), INVALID, ("2^32",)),
    "f32_cells_2_31": ((2048, 2048, 512), (), UNSUPPORTED, ("2^31", "CVR_OPT_MEDIUM_FORMAT", "CVR_OPT_CELLS",
                                                         "cvr_set_medium_sparse")),
}


@pytest.mark.parametrize("row", list(DENSE_REFUSALS))
def test_dense_refusals(cvr, usable, row):
    res, opts, code, words = DENSE_REFUSALS[row]
    ctx, check = usable
    desc, keep = dummy_dense(cvr, res)
    refused(cvr, lambda: ctx.set_medium(desc), code, *words)
    check()   # the previous medium still renders
    check(reload_medium=True)


def test_f32_cells_guard_is_narrow(cvr):
    """2^31 voxels are refused only as fp32 cells.  cvr_set_medium judges the shape before it looks at
    the arrays, so a descriptor without arrays tells which side of the guard a shape is on: past it
    the call ends at its NULL check (CVR_ERR_INVALID), with nothing allocated or read."""
    probes = [
        # res, options, format, refused by the guard
        ((2048, 2048, 512), (), 0, True),
        ((2048, 2048, 511), (), 0, False),                      # 2^31 - 2^22 voxels
        ((2048, 2048, 512), (("OPT_CELLS", 0),), 0, False),
        ((2048, 2048, 512), (), 1, False),
        ((2047, 2048, 1023), (), 1, False),                     # the half format up to the 2^32 guard
    ]
    for res, opts, fmt, guard in probes:
        ctx = cvr.Context(0, "regenerationSK")
        try:
            for k, v in opts:
                ctx.set_option(getattr(cvr, k), v)
            ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
            desc, keep = dummy_dense(cvr, res)
            desc.density = None
            desc.albedo = None
            if guard:
                refused(cvr, lambda: ctx.set_medium(desc), UNSUPPORTED, "2^31")
            else:
                refused(cvr, lambda: ctx.set_medium(desc), INVALID, "NULL")
        finally:
            ctx.close()


def test_sparse_refusals(cvr, usable):
    ctx, check = usable
    # CVR_OPT_BOUNDS untouched: 8^3 bricks.  Bricks per z layer: leaf table (1, 4096, 4096) is 2^24
    desc, keep = dummy_sparse(cvr, (4096, 4096, 1))
    refused(cvr, lambda: ctx.set_medium_sparse(desc), UNSUPPORTED, "2^24")
    # one more leaf along z than a 24-bit multiplicand holds (sparse_long_z, 2^24, is the largest accepted)
    desc, keep = dummy_sparse(cvr, (1, 1, (1 << 24) + 1))
    refused(cvr, lambda: ctx.set_medium_sparse(desc), UNSUPPORTED, "2^24")
    # a leaf table of 2^32 entries
    desc, keep = dummy_sparse(cvr, (65536, 65536, 1))
    refused(cvr, lambda: ctx.set_medium_sparse(desc), INVALID, "2^32")
    check()
    # the grids of sparse_xy_limit and sparse_long_z at 4^3 bricks (CVR_OPT_BOUNDS 2, or bounds off)
    for shift in (2, 0):
        ctx.set_option(cvr.OPT_BOUNDS, shift)
        for dims in ((4095, 4096, 2), (1, 1, 1 << 24)):
            desc, keep = dummy_sparse(cvr, dims)
            refused(cvr, lambda: ctx.set_medium_sparse(desc), UNSUPPORTED, "2^24")
    ctx.set_option(cvr.OPT_BOUNDS, 2)   # (the dense default, for the reload)
    check()
    check(reload_medium=True)


def test_sparse_guard_is_sharp(cvr):
    """Both sides of every term of the brick guard, per brick size.  cvr_set_medium_sparse judges the
    shape before it looks at the arrays, so a descriptor without arrays that is past the guard ends
    at the NULL check (CVR_ERR_INVALID) with nothing read or allocated."""
    probes = [
        # CVR_OPT_BOUNDS (None: untouched), leaf dims (x, y, z), refused by the guard
        (None, (4095, 4096, 2), False), (None, (4096, 4096, 1), True),
        (None, (1, 1, 1 << 24), False), (None, (1, 1, (1 << 24) + 1), True),
        (3, (1, 1, 1 << 24), False), (3, (1, 1, (1 << 24) + 1), True),
        (2, (2047, 2048, 2), False), (2, (2048, 2048, 1), True),
        (2, (1, 1, 1 << 23), False), (2, (1, 1, (1 << 23) + 1), True),
        (1, (1023, 1024, 2), False), (1, (1024, 1024, 1), True),
        (1, (1, 1, 1 << 22), False), (1, (1, 1, (1 << 22) + 1), True),
        (0, (2047, 2048, 2), False), (0, (2048, 2048, 1), True),       # bounds off: 4^3 bricks
        (0, (1, 1, 1 << 23), False), (0, (1, 1, (1 << 23) + 1), True),
        (2, (8, 8, 1 << 23), True),                                    # 16 x 16 x 2^24 = 2^32 bricks
    ]
    for shift, dims, guard in probes:
        ctx = cvr.Context(0, "regenerationSK")
        try:
            if shift is not None:
                ctx.set_option(cvr.OPT_BOUNDS, shift)
            desc, keep = dummy_sparse(cvr, dims)
            desc.leaf_table = None
            desc.leaf_density = None
            if guard:
                refused(cvr, lambda: ctx.set_medium_sparse(desc), UNSUPPORTED, "2^24")
            else:
                refused(cvr, lambda: ctx.set_medium_sparse(desc), INVALID, "NULL")
        finally:
            ctx.close()


def test_cell_leaf_refusal(cvr, usable):
    """Leaf table (256, 256, 256) with every entry slot 0: 2^24 cell leaves and the zero leaf, one more
    than the 24-bit slot of a brick word holds."""
    ctx, check = usable
    table = np.zeros(256 ** 3, np.uint32)
    desc, keep = dummy_sparse(cvr, (256, 256, 256), table, n_leaves=1)
    refused(cvr, lambda: ctx.set_medium_sparse(desc), UNSUPPORTED, "2^24", "cell leaves")
    check()


def test_launch_refusals(cvr, usable):
    ctx, check = usable
    refused(cvr, lambda: ctx.set_resolution((1 << 21) + 8, 8), INVALID, "2^24")
    ctx.set_resolution(*limits.TOP_TILE)
    ctx.set_iterations(limits.TOP_ITERATIONS)          # 2^32 - 64 paths: accepted
    refused(cvr, lambda: ctx.set_iterations(limits.TOP_ITERATIONS + 1), INVALID, "uint32")
    # a range that ends at 2^32: refused by the launch
    ctx.set_path_range((1 << 32) - 1000, 1000)
    refused(cvr, ctx.launch_render, INVALID, "32-bit")
    ctx.set_path_range((1 << 32) - 1001, 1000)         # ends at 2^32 - 1: clipped to n_paths, launched
    ctx.clear_output()
    ctx.launch_render()
    assert ctx.stats().paths == limits.TOP_N - ((1 << 32) - 1001)
    check()
