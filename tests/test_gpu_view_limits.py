"""The view passes at the limits of the storage's 24- and 32-bit index arithmetic.

cvr_features and cvr_preview read the context's storage through FeatureDeviceTexels (csrc/
cvr_features_device.h), which forms the brick-word index, the empty-region mask's bit index and the
cell-leaf address itself and calls dense_cell, texel_density and texel_albedo (csrc/cvr_walk.h).  On
every medium of tests/limits.py (uploaded as tests/test_gpu_limits.py uploads it, with its own brick
size, box and scale), in CVR_FORMAT_F32 and CVR_FORMAT_F16 (the media are exact in binary16: one
reference), the sparse ones with CVR_OPT_EMPTY_MASK 1 and 0 and with CVR_OPT_CELLS 0 (the 8-tap
gather through texel_density), ctx.features(), ctx.preview() under one directional light and
ctx.preview() unshaded must return the bits of the reference: for a sparse case the numpy
restatement over the leaf fetch (tests/view_limits.py; tests/test_view_limits_cpu.py pins it to the
host statements and shows that its taps are sharp), for a dense case the host statement.  Views: the
case's own 32x32 one, and the same camera as a 32x24 tile at offset (3, 5) of a 64x64 image, ragged
against the wave's 8x8 blocks.  Every comparison is of bits.  A sparse case's feature planes and
unshaded preview come from one march of the reference (view_limits.ref_features_and_unshaded).

Every variant sets CVR_OPT_EMPTY_MASK itself, and cvr_medium_info must show cells, or none for
CVR_OPT_CELLS 0: a changed default fails here.

The light volume and the shadowed preview are not run here: the volume's nodes are spread over the
whole box, fewer than 0.1 % of them lie in or behind a limit medium's stored region, and a
comparison there would be of ones.  tests/test_gpu_view_storage.py covers them over the brick and
mask geometries."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import limits
import view_limits
from test_denoise_cpu import bits
from test_gpu_limits import medium_ctx

pytestmark = pytest.mark.gpu

# id -> options
VARIANTS = {"mask1": (("OPT_EMPTY_MASK", 1),), "mask0": (("OPT_EMPTY_MASK", 0),),
            "cells0": (("OPT_EMPTY_MASK", 1), ("OPT_CELLS", 0))}
PASSES = ("features", "shaded", "unshaded")


def march(cvr, case):
    return cvr.FeaturesDesc(view_limits.step_of(case), view_limits.T_STOP, view_limits.MAX_STEPS)


def preview_desc(cvr, case, shaded):
    if shaded:
        return cvr.PreviewDesc(march(cvr, case), light=view_limits.LIGHT)
    return cvr.PreviewDesc(march(cvr, case), flags=cvr.PREVIEW_UNSHADED)


class Media:
    """The limit cases: the references of each (kept: a few images), and the arrays of the last one
    used (up to 0.7 GB: one at a time)."""

    def __init__(self, cvr):
        self.cvr = cvr
        self.refs = {}
        self.last = (None, None)

    def case(self, name):
        if self.last[0] != name:
            self.last = (None, None)
            self.last = (name, limits.MEDIA[name]())
        return self.last[1]

    def ref(self, name):
        """view -> pass -> planes."""
        if name not in self.refs:
            case = self.case(name)
            self.refs[name] = {view: self._view(case, view) for view in view_limits.VIEWS}
        return self.refs[name]

    def _view(self, case, view):
        if case.kind == "sparse":
            planes, unshaded = view_limits.ref_features_and_unshaded(case, view)
            return {"features": planes, "unshaded": unshaded, "shaded": view_limits.ref_preview(case, True, view)}
        return {p: self._one(case, view, p) for p in PASSES}

    def _one(self, case, view, what):
        cvr = self.cvr
        m = case.medium
        desc, keep = cvr.medium_from_arrays(m.density, m.albedo, case.box_min, case.box_max, case.scale, m.max_density)
        cam = limits.camera(case)
        full, tile, off = view_limits.VIEWS[view]
        if what == "features":
            return cvr.features_host(desc, cam.inv_view, cam.r2v, full, tile, off, 0, march(cvr, case))
        return cvr.preview_host(desc, cam.inv_view, cam.r2v, full, tile, off, 0, preview_desc(cvr, case, what == "shaded"))


@pytest.fixture(scope="module")
def med(cvr):
    return Media(cvr)


def assert_geometry(ctx, case, fmt, cells):
    """The context has the geometry the case is there for."""
    lay = ctx.medium_layout().as_dict()
    assert lay["sparse"] == int(case.kind == "sparse") and lay["brick_shift"] == limits.brick_shift(case)
    if case.kind == "sparse":
        es, lx, ly, lz, mask_bits = limits.emask_model(case)
        assert lay["mask_shift"] == es
        words = [0] * 64
        for b in mask_bits:
            words[b >> 5] |= 1 << (b & 31)
        assert lay["mask"] == words
    info = ctx.medium_info()
    assert info.format == fmt and info.max_density_eff == 1.0
    assert (info.cells_bytes > 0) == cells, f"cells_bytes {info.cells_bytes}"


def check_views(cvr, ctx, case, ref, what):
    cam = limits.camera(case)
    for view, (full, tile, off) in view_limits.VIEWS.items():
        ctx.set_camera(cam.inv_view, cam.r2v, full)
        ctx.set_resolution(*tile)
        ctx.set_offset(*off)
        for p in PASSES:
            want = ref[view][p]
            if p == "features":
                got = ctx.features(march(cvr, case))
                assert np.array_equal(bits(got[0]), bits(want[0])), f"{what} {view}: feat_rgba"
                assert np.array_equal(bits(got[1]), bits(want[1])), f"{what} {view}: feat_depth"
                assert (got[0][..., 3] > 0).mean() >= 0.95
            else:
                got = ctx.preview(preview_desc(cvr, case, p == "shaded"))
                assert np.array_equal(bits(got[..., 3]), bits(want[..., 3])), f"{what} {view} {p}: alpha"
                assert np.array_equal(bits(got), bits(want)), f"{what} {view} {p}: rgb"


CASES = [(n, v) for n in limits.MEDIA for v in (VARIANTS if n in limits.SPARSE else ("default",))]


@pytest.mark.parametrize("fmt", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("name,variant", CASES)
def test_view_passes_at_limit(cvr, med, name, variant, fmt):
    case = med.case(name)
    ctx = medium_ctx(cvr, case, VARIANTS.get(variant, ()), fmt)
    try:
        assert_geometry(ctx, case, fmt, variant != "cells0")
        check_views(cvr, ctx, case, med.ref(name), f"{name} {variant} format {fmt}")
    finally:
        ctx.close()
