"""The light volume and the shadowed preview on the GPU.  k_light_volume runs light_node and
k_preview_shadowed runs preview_shadowed_pixel (csrc/cvr_shadow.h), the definitions the two host
statements run on the CPU: every comparison here is of bits (uint32 views), never within a tolerance.

Media, storages, cameras and tiles are those of tests/test_gpu_features.py: blob16 (cells and bounds;
cells off; bounds off) and the ragged 24x17x19 grid dense and as a sparse upload (empty mask on, off,
without cells), each in CVR_FORMAT_F32 and CVR_FORMAT_F16 (the host then reads the cvr_half_round-ed
arrays and the majorant cvr_medium_info reports).  Light grids: 13x11x9 (ragged against the kernel's
4x4x4 node blocks and its 16x4x4 workgroups), 1x1x1, and 70x9x5, which takes 5 x 3 x 2 workgroups
(the launch has no grid cap to cross).  All storages of one medium are compared with the same host
result: neither pass depends on the storage."""
import ctypes as C
import os
from functools import lru_cache

import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import params
from test_denoise_cpu import bits
from test_gpu_denoise import read_pfm
from test_gpu_features import BIG_TILE, SCALE, SMALL_TILES, arrays, bucky_ctx, make_ctx, run_cli, storages, view

pytestmark = pytest.mark.gpu

STATE, INVALID = -3, -1
F = np.float32
LIGHT = (0.3, 1.0, -0.4)
GRIDS = [(13, 11, 9), (1, 1, 1), (70, 9, 5)]
MARCH = (1.0, 1.0 / 256.0, 4096)
# name -> PreviewDesc keywords (flags 0: the directional light; the light itself is the volume's)
DESCS = {
    "shaded": dict(flags=0, specular=0.3, shininess_log2=3, background=(0.25, 0.5, 0.125)),
    "unshaded": dict(flags=1),
}


def make_desc(cvr, name, march=MARCH):
    return cvr.PreviewDesc(cvr.FeaturesDesc(*march), **DESCS[name])


def host_medium(cvr, name, fmt, max_density=1.0):
    d, a = arrays(name, False, fmt)
    return cvr.medium_from_arrays(d, a, scale=SCALE, max_density=max_density)


@lru_cache(maxsize=None)
def host_volume(name, fmt, res, light=LIGHT, march=MARCH):
    import cudavolumerenderer_amd as cvr
    m, keep = host_medium(cvr, name, fmt)
    S = cvr.light_volume_host(m, cvr.LightVolumeDesc(res, light, cvr.FeaturesDesc(*march)))
    S.setflags(write=False)
    return S


@lru_cache(maxsize=None)
def host_image(name, fmt, camera, geometry, desc, shadow, max_density=1.0, res=GRIDS[0], light=LIGHT):
    import cudavolumerenderer_amd as cvr
    full, tile, off = geometry
    m, keep = host_medium(cvr, name, fmt, max_density)
    cam = params.camera(camera, full)
    img = cvr.preview_shadowed_host(m, cam.inv_view, cam.r2v, full, cvr.LightVolumeDesc(res, light), host_volume(name, fmt, res, light),
                                    tile, off, 0, make_desc(cvr, desc), shadow)
    img.setflags(write=False)
    return img


def assert_image(got, want, what):
    assert np.array_equal(bits(got[..., 3]), bits(want[..., 3])), what + ": alpha"
    assert np.array_equal(bits(got), bits(want)), what + ": rgb"


# ------------------------------------------------ device == host, bit for bit --
@pytest.mark.parametrize("storage", range(7))
@pytest.mark.parametrize("fmt", [0, 1], ids=["f32", "f16"])
def test_light_volume_equals_host(cvr, storage, fmt):
    name, sparse, opts = storages(cvr)[storage]
    ctx = make_ctx(cvr, name, False, fmt, sparse, opts)
    try:
        dark = 0
        for res in GRIDS:
            for light in (LIGHT, (0.0, 0.0, 1.0)):
                used = ctx.build_light_volume(light, res)
                assert tuple(used.res) == res
                got = ctx.light_volume()
                assert got.shape == res[::-1]
                assert np.array_equal(bits(got), bits(host_volume(name, fmt, res, light))), f"{res} {light}"
                dark += int((got < 0.5).sum())
        assert dark > 500
        info = ctx.light_volume_info().as_dict()
        assert info["valid"] and info["res"] == GRIDS[-1] and info["bytes"] == 70 * 9 * 5 * 4 and info["light"] == (0.0, 0.0, 1.0)
        # another march: a half step, no early stop
        march = (0.5, 0.0, 4096)
        ctx.build_light_volume(LIGHT, GRIDS[0], cvr.FeaturesDesc(*march))
        assert np.array_equal(bits(ctx.light_volume()), bits(host_volume(name, fmt, GRIDS[0], LIGHT, march)))
    finally:
        ctx.close()


@pytest.mark.parametrize("storage", range(7))
@pytest.mark.parametrize("fmt", [0, 1], ids=["f32", "f16"])
def test_preview_shadowed_equals_host(cvr, storage, fmt):
    name, sparse, opts = storages(cvr)[storage]
    ctx = make_ctx(cvr, name, False, fmt, sparse, opts)
    try:
        md = float(ctx.medium_info().max_density_eff)
        ctx.build_light_volume(LIGHT, GRIDS[0])
        lit = 0
        for desc in DESCS:
            for shadow in (0.5, 1.0):
                for camera in ("oblique", "inside"):
                    for geometry in SMALL_TILES:
                        view(ctx, camera, geometry)
                        got = ctx.preview_shadowed(make_desc(cvr, desc), shadow)
                        assert_image(got, host_image(name, fmt, camera, geometry, desc, shadow, md), f"{desc} {shadow} {camera} {geometry[1]}")
                        lit += int((got[..., 3] > 0).sum())
        for desc, shadow in (("shaded", 0.5), ("unshaded", 1.0)):
            view(ctx, "oblique", BIG_TILE)
            got = ctx.preview_shadowed(make_desc(cvr, desc), shadow)
            assert_image(got, host_image(name, fmt, "oblique", BIG_TILE, desc, shadow, md), f"{desc} {shadow} oblique 256x256")
            assert (got[..., 3] > 0.5).any() and (got[..., 3] == 0).any()
        assert lit > 3000
    finally:
        ctx.close()


# ----------------------------------------------------------- entry points ----
def test_destinations_and_refusals(cvr):
    ctx = make_ctx(cvr, "ragged", False, 0, True)
    try:
        geometry = SMALL_TILES[1]
        view(ctx, "oblique", geometry)
        w, h = geometry[1]
        t = torch.full((h, w, 4), float("nan"), device="cuda")
        with pytest.raises(cvr.CvrError) as e:  # no volume yet
            ctx.preview_shadowed()
        assert e.value.code == STATE and "light volume" in str(e.value)
        with pytest.raises(cvr.CvrError) as e:
            ctx.light_volume()
        assert e.value.code == STATE and not ctx.light_volume_info().valid
        ctx.build_light_volume(LIGHT, GRIDS[0])
        for desc, shadow in (("shaded", 0.5), ("unshaded", 1.0)):
            want = host_image("ragged", 0, "oblique", geometry, desc, shadow)
            t.fill_(float("nan"))
            torch.cuda.synchronize()  # the context runs on its own stream
            ctx.preview_shadowed_buffers(t, make_desc(cvr, desc), shadow)
            ctx.synchronize()
            assert_image(t.cpu().numpy(), want, f"buffers {desc}")
            assert_image(ctx.preview_shadowed(make_desc(cvr, desc), shadow), want, f"pageable {desc}")
            with cvr.PinnedImage(w, h) as pin:
                pin.array[:] = np.nan
                assert_image(np.array(ctx.preview_shadowed(make_desc(cvr, desc), shadow, host_ptr=pin), copy=True), want, f"pinned {desc}")
        lib = cvr.load()
        d = make_desc(cvr, "shaded")
        out = np.zeros((h, w, 4), F)
        assert lib.cvr_preview_shadowed(ctx._h, C.byref(d), C.c_float(0.5), C.c_void_p(out.ctypes.data), out.size - 1) == INVALID
        assert lib.cvr_preview_shadowed(ctx._h, None, C.c_float(0.5), C.c_void_p(out.ctypes.data), out.size) == INVALID
        with pytest.raises(cvr.CvrError) as e:
            ctx.preview_shadowed_buffers(t.data_ptr() + 4)
        assert e.value.code == INVALID and "aligned" in str(e.value)
        with pytest.raises(cvr.CvrError) as e:
            ctx.preview_shadowed(cvr.PreviewDesc())  # the default descriptor is the headlight's
        assert e.value.code == INVALID and "HEADLIGHT" in str(e.value)
        for shadow in (-0.01, 1.01, float("nan")):
            with pytest.raises(cvr.CvrError) as e:
                ctx.preview_shadowed(shadow=shadow)
            assert e.value.code == INVALID and "shadow" in str(e.value)
        for kw in (dict(res=(0, 1, 1)), dict(res=(1025, 1, 1)), dict(res=(1024, 1024, 129)), dict(light=(0, 0, 0)),
                   dict(march=cvr.FeaturesDesc(9.0))):
            with pytest.raises(cvr.CvrError) as e:
                ctx.build_light_volume(kw.get("light", LIGHT), kw.get("res", GRIDS[0]), kw.get("march"))
            assert e.value.code == INVALID, kw
        # a refused build leaves the volume as it was
        assert_image(ctx.preview_shadowed(make_desc(cvr, "shaded"), 0.5), host_image("ragged", 0, "oblique", geometry, "shaded", 0.5), "after refusals")
        ctx.clear_light_volume()
        assert not ctx.light_volume_info().valid and ctx.light_volume_info().bytes == 0
        with pytest.raises(cvr.CvrError) as e:
            ctx.preview_shadowed()
        assert e.value.code == STATE
        # the default grid: half the medium's res, rounded up
        used = ctx.build_light_volume(LIGHT)
        assert tuple(used.res) == (12, 9, 10) and ctx.light_volume().shape == (10, 9, 12)
    finally:
        ctx.close()
    empty = cvr.Context(0, "regenerationSK")
    try:
        with pytest.raises(cvr.CvrError) as e:
            empty.build_light_volume(LIGHT, GRIDS[0])
        assert e.value.code == STATE and "medium" in str(e.value)
    finally:
        empty.close()


def test_shadow_zero_is_the_preview(cvr):
    ctx = make_ctx(cvr, "blob16")
    try:
        ctx.build_light_volume(LIGHT, GRIDS[0])
        for geometry in (SMALL_TILES[1], BIG_TILE):
            view(ctx, "oblique", geometry)
            for kw in (dict(specular=0.3, background=(0.25, 0.5, 0.125)), dict(flags=1)):
                want = ctx.preview(cvr.PreviewDesc(light=LIGHT, **dict(dict(flags=0), **kw)))
                got = ctx.preview_shadowed(cvr.PreviewDesc(light=(9.0, 9.0, 9.0), **dict(dict(flags=0), **kw)), 0.0)
                assert np.array_equal(bits(got), bits(want)), (geometry[1], kw)
                assert (got[..., 3] > 0).sum() > 500
                dark = ctx.preview_shadowed(cvr.PreviewDesc(**dict(dict(flags=0), **kw)), 1.0)
                assert np.array_equal(bits(dark[..., 3]), bits(want[..., 3])) and (dark[..., :3] <= want[..., :3]).all()
                assert (dark[..., :3] < want[..., :3]).any()
    finally:
        ctx.close()


# ------------------------------------------------- whose volume, and how long --
def test_volume_is_per_context(cvr):
    owner = make_ctx(cvr, "ragged", False, 1, True)
    sharer = cvr.Context(0, "regenerationSK")
    try:
        owner.build_light_volume(LIGHT, GRIDS[0])
        mine = owner.light_volume()
        sharer.share_medium(owner)
        assert not sharer.light_volume_info().valid
        geometry = SMALL_TILES[1]
        view(sharer, "oblique", geometry)
        with pytest.raises(cvr.CvrError) as e:
            sharer.preview_shadowed()
        assert e.value.code == STATE
        other = (0.0, 0.0, 1.0)
        sharer.build_light_volume(other, GRIDS[2])
        assert np.array_equal(bits(sharer.light_volume()), bits(host_volume("ragged", 1, GRIDS[2], other)))
        md = float(sharer.medium_info().max_density_eff)
        assert_image(sharer.preview_shadowed(make_desc(cvr, "shaded"), 0.5),
                     host_image("ragged", 1, "oblique", geometry, "shaded", 0.5, md, GRIDS[2], other), "the sharer's volume")
        # the owner's volume is untouched
        assert owner.light_volume_info().as_dict()["res"] == GRIDS[0]
        assert np.array_equal(bits(owner.light_volume()), bits(mine)) and np.array_equal(bits(mine), bits(host_volume("ragged", 1, GRIDS[0])))
        view(owner, "oblique", geometry)
        assert_image(owner.preview_shadowed(make_desc(cvr, "shaded"), 0.5), host_image("ragged", 1, "oblique", geometry, "shaded", 0.5, md), "the owner's volume")
    finally:
        sharer.close()
        owner.close()


def test_volume_is_dropped_with_the_medium(cvr):
    other = make_ctx(cvr, "blob16")
    ctx = make_ctx(cvr, "blob16")
    try:
        view(ctx, "oblique", SMALL_TILES[1])
        d, a = arrays("blob16", False, 0)
        m, keep = cvr.medium_from_arrays(d, a, scale=SCALE, max_density=1.0)

        def stale():
            with pytest.raises(cvr.CvrError) as e:
                ctx.preview_shadowed()
            assert e.value.code == STATE, str(e.value)
            return str(e.value)

        def rebuilt():
            ctx.build_light_volume(LIGHT, GRIDS[0])
            assert (ctx.preview_shadowed()[..., 3] > 0).any()

        rebuilt()
        ctx.set_medium(m)
        assert "no light volume" in stale() and not ctx.light_volume_info().valid
        rebuilt()
        dd, da = torch.tensor(d).cuda(), torch.tensor(a).cuda()
        ctx.set_medium_device(dd, da, scale=SCALE, max_density=1.0)
        stale()
        rebuilt()
        ctx.set_medium_device(dd, da, scale=SCALE, max_density=1.0, sparse=True)
        stale()
        rebuilt()
        ctx.share_medium(other)
        stale()
        rebuilt()
        # a volume built under another CVR_OPT_WORLD_TO_AABB is stale, and good again when the option is back
        ctx.set_option(cvr.OPT_WORLD_TO_AABB, 1)
        assert "stale" in stale() and ctx.light_volume_info().valid
        ctx.set_option(cvr.OPT_WORLD_TO_AABB, 0)
        assert (ctx.preview_shadowed()[..., 3] > 0).any()
    finally:
        ctx.close()
        other.close()


def test_device_classified_clipped_medium(cvr):
    scalar = cvr.Context(0, "regenerationSK")
    try:
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
        geometry = SMALL_TILES[1]
        view(scalar, "oblique", geometry)
        m, keep_alive = cvr.medium_from_arrays(d, a, scale=SCALE, max_density=float(scalar.medium_info().max_density_eff))
        cam = params.camera("oblique", geometry[0])
        vd = scalar.build_light_volume(LIGHT)
        assert tuple(vd.res) == (10, 7, 6)
        S = cvr.light_volume_host(m, vd)
        assert np.array_equal(bits(scalar.light_volume()), bits(S)) and (S < 0.5).any() and (S == 1).any()
        for desc, shadow in (("shaded", 0.7), ("unshaded", 1.0)):
            want = cvr.preview_shadowed_host(m, cam.inv_view, cam.r2v, geometry[0], vd, S, geometry[1], geometry[2], 0,
                                             make_desc(cvr, desc), shadow)
            got = scalar.preview_shadowed(make_desc(cvr, desc), shadow)
            assert_image(got, want, f"classified, clipped medium: {desc}")
            assert (got[..., 3] > 0.5).any()
    finally:
        scalar.close()


def test_build_inside_an_adaptive_session(cvr):
    W = H = 32
    geometry = ((W, H), (W, H), (0, 0))
    results = []
    for with_shadows in (False, True):
        ctx = make_ctx(cvr, "blob16")
        try:
            view(ctx, "oblique", geometry)
            ctx.set_seed(3)
            ctx.init()
            with ctx.adaptive(cvr.AdaptiveDesc(2, 6, 1, -1.0, 0.01)) as a:  # one sample per launch: reproducible sums
                while not a.step().done:
                    if with_shadows:
                        ctx.build_light_volume(LIGHT, GRIDS[0])
                        assert np.array_equal(bits(ctx.light_volume()), bits(host_volume("blob16", 0, GRIDS[0])))
                        assert_image(ctx.preview_shadowed(make_desc(cvr, "shaded"), 0.5),
                                     host_image("blob16", 0, "oblique", geometry, "shaded", 0.5), "inside the session")
                img = a.image()
                s1, s2 = ctx.copy_moments()
            results.append((img, s1, s2))
        finally:
            ctx.close()
    for x, y in zip(*results):
        assert np.array_equal(bits(x), bits(y))


# --------------------------------------------------------------------- CLI --
def test_cli_preview_shadows(cvr, tmp_path):
    out = str(tmp_path / "s.hdr")
    r = run_cli("-i", "0", "--preview", out, "--pfm", "--preview-light", "1", "2", "0.5", "--preview-shadows", "0.7")
    assert r.returncode == 0, r.stderr
    assert "rendering time" not in r.stdout  # no render
    scene = cvr.Scene.synthetic("bucky")
    ctx = bucky_ctx(cvr, scene)
    try:
        light = (1.0, 2.0, 0.5)
        ctx.build_light_volume(light)
        want = ctx.preview_shadowed(cvr.PreviewDesc(light=light), 0.7)
        plain = ctx.preview(cvr.PreviewDesc(light=light))
        ctx.build_light_volume(light, (9, 7, 5), cvr.FeaturesDesc(0.5))
        other = ctx.preview_shadowed(cvr.PreviewDesc(light=light, flags=cvr.PREVIEW_UNSHADED), 1.0)
    finally:
        ctx.close()
    assert (want[..., 3] > 0.5).any() and (want[..., :3] < plain[..., :3]).any()
    assert np.array_equal(bits(read_pfm(out + ".pfm")), bits(want[..., :3]))
    second = str(tmp_path / "t.hdr")
    r = run_cli("-i", "0", "--preview", second, "--pfm", "--preview-light", "1", "2", "0.5", "--preview-shadows", "1",
                "--preview-shadow-res", "9", "7", "5", "--preview-shadow-step", "0.5", "--preview-unshaded")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(bits(read_pfm(second + ".pfm")), bits(other[..., :3]))
    # usage errors: shadows need the preview and its directional light
    r = run_cli("-i", "0", "--preview", out, "--preview-shadows", "0.7")
    assert r.returncode == 2 and "--preview-light" in r.stderr
    r = run_cli("-i", "1", "--preview-light", "1", "2", "0.5", "--preview-shadows", "0.7")
    assert r.returncode == 2 and "--preview FILE" in r.stderr
    r = run_cli("-i", "0", "--preview", out, "--preview-light", "1", "2", "0.5", "--preview-shadow-res", "8", "8", "8")
    assert r.returncode == 2 and "--preview-shadows" in r.stderr
    r = run_cli("-i", "0", "--preview", out, "--preview-light", "1", "2", "0.5", "--preview-shadows", "1.5")
    assert r.returncode == 1 and "shadow" in r.stderr
