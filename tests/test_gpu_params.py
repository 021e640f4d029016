"""GPU == oracle over the BSDF, box and camera parameter space (tests/params.py).

Every other GPU parity test renders with g = 0, roughness (0.1, 0.1), eta = 1.05/1.01 and the default
camera (outside the box, nearly parallel rays down one axis).  The cases here reach the rest of the
event code: hg_sample with |g| > eps, the anisotropic project_roughness / ggx_sample_vndf, every
branch of fresnel_dielectric (eta == 1, eta < 1 with total internal reflection on entry, the host's
inv_eta), paths that start inside the box, rays with +-0 components and origins on the box's planes
(aabb_intersect's inf and NaN arithmetic through det_fminf / det_fmaxf), and the boundary normals a
wide or oblique camera produces (the 3-bit normal code of a pool slot, normalize3_unit_fast, the sign
shortcut of ggx_sample).

Per case (16^3 medium, 32x32 pixels x 4 samples = 4096 paths, or 3072 for the offset tile):
  1. the production wave pool's records (cvr_trace_launch, regenerationSK / sortingSK): image id,
     flags, the three T words as uint32 (NaN and -0 count) and the segment count equal the oracle's;
  2. the debug kernel's whole records (cvr_trace_paths, naiveSK / regenerationSK) equal the oracle's;
  3. a plain launch (naiveSK, naiveMK, regenerationSK): counters equal, pixels within
     2 (n - 1) 2^-24 max(|gpu|, |cpu|) + 1e-30 with n the pixel's own number of contributions, the
     NaN pattern equal.
For the combined cases (inside_all, box_all with both CVR_OPT_WORLD_TO_AABB values) check 3 also runs
on every other instance of the event code: schedulers 0, 1, 2 and 4, no density cells, no brick
bounds, the sparse upload with and without the empty-region mask, the half format, the moments
instance, cvr_render_frame's in-launch output and k_naive_mk.  The library refuses none of these.

The oracle's records of a case are traced once per module and shared."""
import numpy as np
import pytest

import params
# (shared with tests/test_gpu_wpool_matrix.py; tests/test_gpu_limits.py and test_gpu_regen_burst.py import them from here)
from params_ref import Ref, Refs, assert_frame, assert_records_equal, sparse_blob  # noqa: F401
from parity_util import assert_sums_close

pytestmark = pytest.mark.gpu

ALL_CASES = list(params.CASES)


@pytest.fixture(scope="module")
def refs(oracle_mod):
    return Refs(oracle_mod)


def make_ctx(cvr, refs, name, kernel, opts=(), fmt=0, sparse=False):
    case = params.CASES[name]
    p = params.medium_params(case)
    cam = params.camera(case.camera, case.full)
    ctx = cvr.Context(0, kernel)
    ctx.set_option(cvr.OPT_WORLD_TO_AABB, case.w2a)
    for k, v in opts:
        ctx.set_option(k, v)
    if fmt:
        ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
    if sparse:
        desc, keep = sparse_blob(cvr, refs.blob, p)
        ctx.set_medium_sparse(desc)
    else:
        desc, keep = cvr.medium_from_arrays(refs.blob[0], refs.blob[1], p["box_min"], p["box_max"], params.SCALE,
                                            params.MAX_DENSITY, p["g"], p["roughness"], p["eta"])
        ctx.set_medium(desc)
    ctx._keep = (desc, keep)
    ctx.set_camera(cam.inv_view, cam.r2v, case.full)
    ctx.set_resolution(*case.tile)
    ctx.set_offset(*case.offset)
    ctx.set_iterations(params.SAMPLES)
    ctx.set_seed(params.SEED)
    ctx.init()
    return ctx, case


def plain_launch(ctx, case):
    ctx.set_path_range(0, params.n_paths(case))
    ctx.clear_output()
    ctx.launch_render()
    return ctx.copy_output(*case.tile), ctx.stats()


# ------------------------------------------------------------ 1. production records --
@pytest.mark.parametrize("kernel", ["regenerationSK", "sortingSK"])
@pytest.mark.parametrize("name", ALL_CASES)
def test_production_records(cvr, refs, name, kernel):
    ctx, case = make_ctx(cvr, refs, name, kernel)
    try:
        n = params.n_paths(case)
        ctx.set_path_range(0, n)
        g = ctx.trace_launch(n)
        c = refs.get(name, cvr.KERNELS.index(kernel)).recs
        assert_records_equal(g, c, ("image_id", "flags", "n_segments"), f"{name} {kernel}")
    finally:
        ctx.close()


# ----------------------------------------------------------------- 2. debug records --
@pytest.mark.parametrize("kernel", ["naiveSK", "regenerationSK"])
@pytest.mark.parametrize("name", ALL_CASES)
def test_debug_records(cvr, refs, name, kernel):
    ctx, case = make_ctx(cvr, refs, name, kernel)
    try:
        g = ctx.trace_paths(0, params.n_paths(case))
        c = refs.get(name, cvr.KERNELS.index(kernel)).recs
        assert_records_equal(g, c, ("image_id", "flags", "n_segments", "n_steps", "n_density", "n_albedo"),
                             f"{name} {kernel}")
    finally:
        ctx.close()


# ------------------------------------------------------- 3. framebuffer and counters --
@pytest.mark.parametrize("kernel", ["naiveSK", "naiveMK", "regenerationSK"])
@pytest.mark.parametrize("name", ALL_CASES)
def test_framebuffer_and_counters(cvr, refs, name, kernel):
    ctx, case = make_ctx(cvr, refs, name, kernel)
    try:
        out, st = plain_launch(ctx, case)
        assert_frame(out, st, refs.get(name, cvr.KERNELS.index(kernel)), f"{name} {kernel}")
    finally:
        ctx.close()


# ------------------------------- 4. the combined cases on every other instance --------
def _opt(cvr, name):
    return getattr(cvr, name)


INSTANCES = {
    # id: (kernel, options, format, sparse)
    "sched0": ("regenerationSK", (("OPT_SCHEDULER", 0),), 0, False),
    "sched1": ("regenerationSK", (("OPT_SCHEDULER", 1),), 0, False),
    "sched2": ("regenerationSK", (("OPT_SCHEDULER", 2),), 0, False),
    "sched4": ("regenerationSK", (("OPT_SCHEDULER", 4),), 0, False),
    "cells0": ("regenerationSK", (("OPT_CELLS", 0),), 0, False),
    "bounds0": ("regenerationSK", (("OPT_BOUNDS", 0),), 0, False),
    "sparse_mask": ("regenerationSK", (("OPT_EMPTY_MASK", 1),), 0, True),
    "sparse_nomask": ("regenerationSK", (("OPT_EMPTY_MASK", 0),), 0, True),
    "half": ("regenerationSK", (), 1, False),
    "naive_mk_item": ("naiveMK", (("OPT_SCHEDULER", 4),), 0, False),  # k_naive_mk
}


@pytest.mark.parametrize("inst", list(INSTANCES))
@pytest.mark.parametrize("name", params.COMBINED)
def test_combined_instances(cvr, refs, name, inst):
    kernel, opts, fmt, sparse = INSTANCES[inst]
    ctx, case = make_ctx(cvr, refs, name, kernel, [(_opt(cvr, k), v) for k, v in opts], fmt, sparse)
    try:
        out, st = plain_launch(ctx, case)
        half = (cvr, ctx.medium_info().max_density_eff) if fmt else None
        assert_frame(out, st, refs.get(name, cvr.KERNELS.index(kernel), half), f"{name} {inst}")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", params.COMBINED)
def test_combined_moments(cvr, refs, name):
    """CVR_OPT_MOMENTS 1: sum T, sum T^2 and the escape counts, as test_moments_match_oracle."""
    ctx, case = make_ctx(cvr, refs, name, "regenerationSK")
    try:
        ctx.set_option(cvr.OPT_MOMENTS, 1)
        ctx.set_path_range(0, params.n_paths(case))
        ctx.clear_output()
        ctx.launch_render()
        st = ctx.stats()
        s1, s2 = ctx.copy_moments()
        ref = refs.get(name, 2)
        px = len(ref.cnt)
        assert ref.cnt.max() > 1
        assert (s2.reshape(px, 4)[:, 3] == ref.cnt.astype(np.float32)).all(), f"{name}: escape counts differ"
        assert_frame(s1, st, ref, f"{name} moments: sum T")
        assert_sums_close(s2.reshape(px, 4)[:, :3], ref.s2, ref.cnt, f"{name} moments: sum T^2")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", params.COMBINED)
def test_combined_render_frame(cvr, refs, name):
    """cvr_render_frame into a PinnedImage: the in-launch-output instance (all 16 blocks stored by the
    launch's flusher waves), normalised by the 4 samples."""
    ctx, case = make_ctx(cvr, refs, name, "regenerationSK", [(cvr.OPT_FRAME_FLUSH, 1)])
    buf = cvr.PinnedImage(*case.tile)
    try:
        buf.array[:] = np.nan
        _, st = ctx.render_frame(buf, 1)
        assert ctx.frame_flush_info() == ((case.tile[0] // 8) * (case.tile[1] // 8), 0)
        assert_frame(buf.array.copy(), st, refs.get(name, 2), f"{name} render_frame", scale=params.SAMPLES,
                     exact_w=False)
    finally:
        buf.close()
        ctx.close()
