"""The view passes over the brick and mask geometries of the storage.

cvr_features, cvr_preview, cvr_build_light_volume and cvr_preview_shadowed read the context's storage
through FeatureDeviceTexels (csrc/cvr_features_device.h).  tests/test_gpu_features.py and its
neighbours run them on media whose bricks are the defaults and whose mask has es = 3; here they run
on the small media of tests/media.py that have the other geometries, each compared bit for bit with
the host statements on the densified arrays:
  sparse_es4      the mask's super-brick is 2x2x2 leaves (es = 4); mask on and off; also CVR_FORMAT_F16
  sparse_small    CVR_OPT_BOUNDS 2 and 1 (bricks of 4^3 and 2^3 cells: more than one brick word per
                  leaf), and 0 (unbounded: no mask, the brick words still name the cell leaves)
  offgrid         a box that is no unit cube, CVR_OPT_WORLD_TO_AABB 0 (many points off the cell grid,
                  some at negative coordinates) and 1
  staircase       res - 1 a multiple of 4 on every axis: each ends in a one-cell-thick brick layer;
                  also CVR_FORMAT_F16
Before comparing, each context's cvr_medium_layout must show the geometry the case is there for;
every sparse case sets CVR_OPT_EMPTY_MASK itself (the layout reports the mask whether it is read or not).
Passes: features; the preview under a directional light; the light volume of 13x11x9 nodes under
that (oblique) light; the shadowed preview.  Cameras "oblique" and "inside", the 40x24 tile at
offset (8, 8) of 64x48."""
from functools import lru_cache

import numpy as np
import pytest
import torch  # noqa: F401  (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import devmed
import media
import params
from test_denoise_cpu import bits

pytestmark = pytest.mark.gpu

LIGHT = (0.3, 1.0, -0.4)
SRES = (13, 11, 9)
GEOMETRY = ((64, 48), (40, 24), (8, 8))
CAMERAS = ("oblique", "inside")

# id -> (medium, format, options, world_to_aabb, expected layout: brick_shift, mask_shift, mask present)
CASES = {
    "es4_mask1": ("sparse_es4", 0, (("OPT_EMPTY_MASK", 1),), 0, (3, 4, True)),
    "es4_mask0": ("sparse_es4", 0, (("OPT_EMPTY_MASK", 0),), 0, (3, 4, True)),   # built and reported, not read
    "es4_f16": ("sparse_es4", 1, (("OPT_EMPTY_MASK", 1),), 0, (3, 4, True)),
    "small_b2": ("sparse_small", 0, (("OPT_EMPTY_MASK", 1), ("OPT_BOUNDS", 2)), 0, (2, 3, True)),
    "small_b1": ("sparse_small", 0, (("OPT_EMPTY_MASK", 1), ("OPT_BOUNDS", 1)), 0, (1, 3, True)),
    "small_b0": ("sparse_small", 0, (("OPT_EMPTY_MASK", 1), ("OPT_BOUNDS", 0)), 0, (2, 0, False)),
    "offgrid_w2a0": ("offgrid", 0, (("OPT_WORLD_TO_AABB", 0),), 0, (2, 0, False)),
    "offgrid_w2a1": ("offgrid", 0, (("OPT_WORLD_TO_AABB", 1),), 1, (2, 0, False)),
    "staircase": ("staircase", 0, (), 0, (2, 0, False)),
    "staircase_f16": ("staircase", 1, (), 0, (2, 0, False)),
}


@lru_cache(maxsize=None)
def dense_arrays(name, fmt):
    """(the medium of tests/media.py, density (z, y, x), albedo (z, y, x, 4) as format `fmt` stores
    them, box_min, box_max, scale)."""
    import cudavolumerenderer_amd as cvr
    m = (media.SPARSE_MEDIA.get(name) or media.DENSE_MEDIA[name])()
    if name in media.SPARSE_MEDIA:
        d, a = devmed.densify(m)
        box = ((-0.5,) * 3, (0.5,) * 3, media.SCALE)
    else:
        d, a = m.density, m.albedo
        box = (m.box_min, m.box_max, m.scale)
    if fmt:
        d, a = cvr.half_round(d), cvr.half_round(a)
    return (m, np.ascontiguousarray(d, np.float32), np.ascontiguousarray(a, np.float32)) + box


def make_ctx(cvr, name, fmt, opts):
    m = dense_arrays(name, 0)[0]  # the context rounds by itself
    ctx = cvr.Context(0, "regenerationSK")
    try:
        ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
        for k, v in opts:
            ctx.set_option(getattr(cvr, k), v)
        if name in media.SPARSE_MEDIA:
            desc, keep = media.sparse_desc(cvr, *m)
            ctx.set_medium_sparse(desc)
        else:
            desc, keep = cvr.medium_from_arrays(m.density, m.albedo, m.box_min, m.box_max, m.scale, m.max_density)
            ctx.set_medium(desc)
    except BaseException:
        ctx.close()
        raise
    return ctx


def assert_layout(ctx, name, want):
    bshift, es, has_mask = want
    lay = ctx.medium_layout().as_dict()
    assert lay["sparse"] == int(name in media.SPARSE_MEDIA)
    assert lay["brick_shift"] == bshift, f"brick shift {lay['brick_shift']}, the case is there for {bshift}"
    assert lay["mask_shift"] == es, f"mask shift {lay['mask_shift']}, the case is there for {es}"
    assert any(lay["mask"]) == has_mask
    if name == "sparse_es4":  # more leaves than the mask has bits at es = 3, clear super-bricks among the set ones
        assert lay["n_leaves"] == len(media.ES4_LEAVES)


@pytest.mark.parametrize("case", list(CASES))
def test_passes_equal_host(cvr, case):
    name, fmt, opts, w2a, layout = CASES[case]
    _, d, a, box_min, box_max, scale = dense_arrays(name, fmt)
    ctx = make_ctx(cvr, name, fmt, opts)
    try:
        assert_layout(ctx, name, layout)
        info = ctx.medium_info()
        assert info.format == fmt
        md = float(info.max_density_eff)
        m, keep = cvr.medium_from_arrays(d, a, box_min, box_max, scale, md)
        full, tile, off = GEOMETRY
        shaded = cvr.PreviewDesc(light=LIGHT)
        # the light volume
        vd = ctx.build_light_volume(LIGHT, SRES)
        assert tuple(vd.res) == SRES
        S = cvr.light_volume_host(m, vd, w2a)
        got = ctx.light_volume()
        assert np.array_equal(bits(got), bits(S)), "light volume"
        assert (S < 0.9).sum() > 30  # (measured on the host statement: 53 nodes for sparse_es4, 917 and more for the others)
        lit = 0
        for camera in CAMERAS:
            cam = params.camera(camera, full)
            ctx.set_camera(cam.inv_view, cam.r2v, full)
            ctx.set_resolution(*tile)
            ctx.set_offset(*off)
            want = cvr.features_host(m, cam.inv_view, cam.r2v, full, tile, off, w2a)
            got = ctx.features()
            assert np.array_equal(bits(got[0]), bits(want[0])), f"{camera}: feat_rgba"
            assert np.array_equal(bits(got[1]), bits(want[1])), f"{camera}: feat_depth"
            lit += int((got[0][..., 3] > 0).sum())
            want = cvr.preview_host(m, cam.inv_view, cam.r2v, full, tile, off, w2a, shaded)
            assert np.array_equal(bits(ctx.preview(shaded)), bits(want)), f"{camera}: preview"
            want = cvr.preview_shadowed_host(m, cam.inv_view, cam.r2v, full, vd, S, tile, off, w2a, shaded, 0.7)
            assert np.array_equal(bits(ctx.preview_shadowed(shaded, 0.7)), bits(want)), f"{camera}: shadowed preview"
        assert lit > 100
    finally:
        ctx.close()
