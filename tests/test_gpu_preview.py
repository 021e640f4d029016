"""The shaded preview pass on the GPU.  k_preview runs preview_pixel (csrc/cvr_preview.h), the
definition cvr_preview_host runs on the CPU: every comparison here is of bits (uint32 views), never
within a tolerance.

Media, storages, cameras and tiles are those of tests/test_gpu_features.py: blob16 (cells and bounds;
cells off; bounds off) and the ragged 24x17x19 grid dense and as a sparse upload (empty mask on, off,
without cells), each in CVR_FORMAT_F32 and CVR_FORMAT_F16 (the host then reads the cvr_half_round-ed
arrays and the majorant cvr_medium_info reports), with a varied and a uniform albedo; 13x7 and 40x24
tiles at offset (8, 8) of 64x48 for every camera, one 256x256 tile for "oblique".  All storages of one
medium are compared with the same host result: the pass does not depend on the storage.
Descriptors: the default (headlight, specular), a directional light without specular over a coloured
background, and unshaded."""
import ctypes as C
import os
from functools import lru_cache

import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import params
from test_denoise_cpu import bits
from test_gpu_denoise import read_pfm
from test_gpu_features import (BIG_TILE, CAMERAS, SCALE, SMALL_TILES, arrays, bucky_ctx, make_ctx, run_cli, storages,
                               view)

pytestmark = pytest.mark.gpu

STATE, INVALID = -3, -1
F = np.float32
# name -> PreviewDesc keywords
DESCS = {
    "headlight": dict(),
    "directional": dict(light=(0.3, 1.0, -0.4), specular=0.0, background=(0.25, 0.5, 0.125)),
    "unshaded": dict(flags=1),
}


def make_desc(cvr, name, march=(1.0, 1.0 / 256.0, 4096)):
    return cvr.PreviewDesc(cvr.FeaturesDesc(*march), **DESCS[name])


@lru_cache(maxsize=None)
def host_image(name, uniform, fmt, camera, geometry, desc, max_density=1.0, march=(1.0, 1.0 / 256.0, 4096)):
    import cudavolumerenderer_amd as cvr
    d, a = arrays(name, uniform, fmt)
    full, tile, off = geometry
    m, keep = cvr.medium_from_arrays(d, a, scale=SCALE, max_density=max_density)
    cam = params.camera(camera, full)
    img = cvr.preview_host(m, cam.inv_view, cam.r2v, full, tile, off, 0, make_desc(cvr, desc, march))
    img.setflags(write=False)
    return img


def assert_image(got, want, what):
    assert np.array_equal(bits(got[..., 3]), bits(want[..., 3])), what + ": alpha"
    assert np.array_equal(bits(got), bits(want)), what + ": rgb"


# ------------------------------------------------ device == host, bit for bit --
@pytest.mark.parametrize("storage", range(7))
@pytest.mark.parametrize("uniform", [False, True], ids=["varied", "uniform"])
@pytest.mark.parametrize("fmt", [0, 1], ids=["f32", "f16"])
def test_device_equals_host(cvr, storage, uniform, fmt):
    name, sparse, opts = storages(cvr)[storage]
    ctx = make_ctx(cvr, name, uniform, fmt, sparse, opts)
    try:
        md = float(ctx.medium_info().max_density_eff)
        lit = 0
        for desc in DESCS:
            for camera in CAMERAS:
                for geometry in SMALL_TILES:
                    view(ctx, camera, geometry)
                    got = ctx.preview(make_desc(cvr, desc))
                    assert_image(got, host_image(name, uniform, fmt, camera, geometry, desc, md), f"{desc} {camera} {geometry[1]}")
                    lit += int((got[..., 3] > 0).sum())
            view(ctx, "oblique", BIG_TILE)
            got = ctx.preview(make_desc(cvr, desc))
            assert_image(got, host_image(name, uniform, fmt, "oblique", BIG_TILE, desc, md), f"{desc} oblique 256x256")
            assert (got[..., 3] > 0.5).any() and (got[..., 3] == 0).any()
        assert lit > 3000
    finally:
        ctx.close()


# ----------------------------------------------------------- entry points ----
def test_buffers_and_host_destinations(cvr):
    ctx = make_ctx(cvr, "ragged", False, 0, True)
    try:
        geometry = SMALL_TILES[1]
        view(ctx, "oblique", geometry)
        w, h = geometry[1]
        for desc, march in (("headlight", (0.5, 0.25, 4096)), ("directional", (0.125, 0.0, 16)), ("unshaded", (8.0, 1.0 / 256.0, 3))):
            want = host_image("ragged", False, 0, "oblique", geometry, desc, 1.0, march)
            out = torch.full((h, w, 4), float("nan"), device="cuda")
            torch.cuda.synchronize()  # the context runs on its own stream
            ctx.preview_buffers(out, make_desc(cvr, desc, march))
            ctx.synchronize()
            assert_image(out.cpu().numpy(), want, f"buffers {desc}")
        # pageable, pinned and registered host memory: the same bits
        want = host_image("ragged", False, 0, "oblique", geometry, "headlight")
        assert_image(ctx.preview(), want, "pageable")
        lib = cvr.load()
        with cvr.PinnedImage(w, h) as pin:
            pin.array[:] = np.nan
            assert_image(np.array(ctx.preview(host_ptr=pin), copy=True), want, "pinned")
            d = cvr.PreviewDesc()
            assert lib.cvr_preview(ctx._h, C.byref(d), pin.ptr, pin.floats - 1) == INVALID
            assert lib.cvr_preview(ctx._h, None, pin.ptr, pin.floats) == INVALID
            assert lib.cvr_preview(ctx._h, C.byref(cvr.PreviewDesc(shininess_log2=11)), pin.ptr, pin.floats) == INVALID
        raw = np.full(w * h * 4 + 1024, np.nan, F)
        start = (-raw.ctypes.data // 4) % 1024  # a page-aligned window of the array
        reg = raw[start:start + w * h * 4].reshape(h, w, 4)
        rt = torch.cuda.cudart()
        assert int(rt.cudaHostRegister(reg.ctypes.data, reg.nbytes, 0)) == 0
        try:
            assert lib.cvr_preview(ctx._h, C.byref(cvr.PreviewDesc()), C.c_void_p(reg.ctypes.data), reg.size) == 0
            assert_image(reg, want, "registered")
        finally:
            rt.cudaHostUnregister(reg.ctypes.data)
        t = torch.zeros((h, w, 4), device="cuda")
        with pytest.raises(cvr.CvrError) as e:
            ctx.preview_buffers(t.data_ptr() + 4)
        assert e.value.code == INVALID and "aligned" in str(e.value)
        with pytest.raises(cvr.CvrError) as e:
            ctx.preview_buffers(t, cvr.PreviewDesc(cvr.FeaturesDesc(1.0, 1.0)))
        assert e.value.code == INVALID
        with pytest.raises(cvr.CvrError) as e:
            ctx.preview_buffers(t, cvr.PreviewDesc(light=(0, 0, 0)))
        assert e.value.code == INVALID and "light" in str(e.value)
    finally:
        ctx.close()
    empty = cvr.Context(0, "regenerationSK")
    try:
        with pytest.raises(cvr.CvrError) as e:
            empty.preview()
        assert e.value.code == STATE and "medium" in str(e.value)
    finally:
        empty.close()


# ------------------------------------------------------ the context is read --
def test_context_is_untouched(cvr, oracle_mod):
    W = H = 32
    geometry = ((W, H), (W, H), (0, 0))
    d, a = arrays("blob16", False, 0)
    ctx = make_ctx(cvr, "blob16")
    try:
        view(ctx, "oblique", geometry)
        ctx.set_seed(params.SEED)
        ctx.set_iterations(4)
        ctx.set_option(cvr.OPT_MOMENTS, 1)
        ctx.init()
        ctx.clear_output()
        ctx.launch_render()
        ctx.synchronize()
        s1, s2 = ctx.copy_moments()
        seed, st = ctx.get_seed(), ctx.stats().as_dict()
        for desc in DESCS:
            assert_image(ctx.preview(make_desc(cvr, desc)), host_image("blob16", False, 0, "oblique", geometry, desc), desc)
        a1, a2 = ctx.copy_moments()
        assert np.array_equal(bits(a1), bits(s1)) and np.array_equal(bits(a2), bits(s2))
        assert ctx.get_seed() == seed and ctx.stats().as_dict() == st and st["paths"] == W * H * 4
        # the next render's paths are the oracle's, as before
        case = params.Case({}, "oblique", 0, (W, H), (W, H), (0, 0))
        orc = oracle_mod.Oracle(d, a, (-0.5,) * 3, (0.5,) * 3, SCALE, 1.0, 0.0, (0.1, 0.1), params.DEFAULT_ETA)
        L = params.make_launch(oracle_mod, case, 2)
        got, want = ctx.trace_paths(0, 1024), orc.trace_paths(L, 0, 1024)
        assert (got["T"].view(np.uint32) == want["T"].view(np.uint32)).all()
        assert (got["n_segments"] == want["n_segments"]).all()
    finally:
        ctx.close()


def test_inside_an_adaptive_session(cvr):
    W = H = 32
    geometry = ((W, H), (W, H), (0, 0))
    want = host_image("blob16", False, 0, "oblique", geometry, "headlight")
    results = []
    for with_preview in (False, True):
        ctx = make_ctx(cvr, "blob16")
        try:
            view(ctx, "oblique", geometry)
            ctx.set_seed(3)
            ctx.init()
            with ctx.adaptive(cvr.AdaptiveDesc(2, 6, 1, -1.0, 0.01)) as a:  # one sample per launch: reproducible sums
                while not a.step().done:
                    if with_preview:
                        assert_image(ctx.preview(), want, "inside the session")
                img = a.image()
                s1, s2 = ctx.copy_moments()
            results.append((img, s1, s2))
        finally:
            ctx.close()
    for x, y in zip(*results):
        assert np.array_equal(bits(x), bits(y))


# ------------------------------------------- shared and classified media -----
def test_shared_and_classified_media(cvr):
    owner = make_ctx(cvr, "ragged", False, 1, True)
    sharer = cvr.Context(0, "regenerationSK")
    scalar = cvr.Context(0, "regenerationSK")
    try:
        sharer.share_medium(owner)
        geometry = SMALL_TILES[1]
        view(sharer, "oblique", geometry)
        md = float(sharer.medium_info().max_density_eff)
        assert_image(sharer.preview(), host_image("ragged", False, 1, "oblique", geometry, "headlight", md), "shared")
        # a medium classified on the device under a crop and a clip plane: the host statement on
        # clip_host of classify_host's arrays
        rng = np.random.default_rng(9)
        field = rng.integers(0, 256, (11, 13, 19), dtype=np.uint8)
        table = np.zeros((16, 4), F)
        table[:, :3] = 0.2 + 0.8 * rng.random((16, 3), dtype=F)
        table[4:, 3] = np.linspace(0.05, 1.0, 12, dtype=F)
        lo, hi, planes = (2, 1, 0), (17, 12, 10), [(1.0, 0.5, -0.25, -4.0)]
        scalar.set_clip(lo, hi, planes)
        scalar.set_medium_scalar(torch.from_numpy(field).cuda(), table, lo=0.0, hi=255.0, scale=SCALE, max_density=1.0)
        d, a = cvr.classify_host(field, table, 0.0, 255.0)
        keep, d, a = cvr.clip_host((19, 13, 11), lo, hi, planes, d, a)
        assert 0.2 < keep.mean() < 0.9
        view(scalar, "oblique", geometry)
        m, keep_alive = cvr.medium_from_arrays(d, a, scale=SCALE, max_density=float(scalar.medium_info().max_density_eff))
        cam = params.camera("oblique", geometry[0])
        for desc in ("headlight", "directional"):
            want = cvr.preview_host(m, cam.inv_view, cam.r2v, *geometry, 0, make_desc(cvr, desc))
            got = scalar.preview(make_desc(cvr, desc))
            assert_image(got, want, f"classified, clipped medium: {desc}")
            assert (got[..., 3] > 0.5).any()
    finally:
        scalar.close()
        sharer.close()
        owner.close()


# --------------------------------------------------------------------- CLI --
def test_cli_preview(cvr, tmp_path):
    out = str(tmp_path / "p.hdr")
    r = run_cli("-i", "0", "--preview", out, "--pfm")
    assert r.returncode == 0, r.stderr
    assert "rendering time" not in r.stdout  # no render
    scene = cvr.Scene.synthetic("bucky")
    ctx = bucky_ctx(cvr, scene)
    try:
        want = ctx.preview()
        lit = ctx.preview(cvr.PreviewDesc(cvr.FeaturesDesc(0.5), light=(1.0, 2.0, 0.5), ambient=0.2, diffuse=0.6, specular=0.4,
                                          shininess_log2=3, knee=0.1, background=(0.5, 0.25, 0.125)))
        flat = ctx.preview(cvr.PreviewDesc(flags=cvr.PREVIEW_UNSHADED))
    finally:
        ctx.close()
    assert (want[..., 3] > 0.5).any() and os.path.getsize(out) > 0
    assert np.array_equal(bits(read_pfm(out + ".pfm")), bits(want[..., :3]))
    other = str(tmp_path / "q.hdr")
    r = run_cli("-i", "0", "--preview", other, "--pfm", "--feature-step", "0.5", "--preview-light", "1", "2", "0.5",
                "--preview-shading", "0.2", "0.6", "0.4", "3", "--preview-knee", "0.1", "--preview-background", "0.5", "0.25",
                "0.125")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(bits(read_pfm(other + ".pfm")), bits(lit[..., :3]))
    third = str(tmp_path / "u.hdr")
    r = run_cli("-i", "2", "--preview", third, "--pfm", "--preview-unshaded", "-o", str(tmp_path / "render"))
    assert r.returncode == 0, r.stderr
    assert "rendering time" in r.stdout and os.path.getsize(str(tmp_path / "render.hdr")) > 0
    assert np.array_equal(bits(read_pfm(third + ".pfm")), bits(flat[..., :3]))
    r = run_cli("-i", "0", "--preview", out, "--number-of-tiles", "2", "2")
    assert r.returncode == 2 and "--preview renders one tile on one device" in r.stderr
    r = run_cli("-i", "0", "--preview", out, "--preview-shading", "0.3", "0.7", "0.2", "11")
    assert r.returncode == 1 and "shininess" in r.stderr
