"""The primary-ray feature pass and the feature-guided filter on the GPU.  k_features runs
feature_pixel (csrc/cvr_features.h), the definition cvr_features_host runs on the CPU, and the
guided passes run the per-pixel function cvr_denoise_guided_host runs: every comparison here is of
bits (uint32 views), never within a tolerance.

Tiles: 13x7 and 40x24 at offset (8, 8) of a 64x48 image (ragged against the wave's 8x8 block and
the workgroup's 16x16) for every camera, one 256x256 tile (256 workgroups) for "oblique".
Media, each in CVR_FORMAT_F32 and CVR_FORMAT_F16 (the host then reads the cvr_half_round-ed arrays),
with a varied and a uniform albedo: blob16 dense (cells and bounds; cells off; bounds off; uniform
albedo loaded), and a ragged 24x17x19 grid whose leaves are partly empty, dense and as a sparse
upload with CVR_OPT_EMPTY_MASK 1 and 0 (and without cells).  All storages of one medium are compared
with the same host result: the pass does not depend on the storage."""
import os
import subprocess
from functools import lru_cache

import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import devmed
import media
import params
from test_denoise_cpu import bits, plant_invalid, random_sums, two_count_map
from test_gpu_denoise import read_pfm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cudavolumerenderer_amd", "cvr")
STATE, INVALID = -3, -1
F = np.float32
SCALE = 40.0
CAMERAS = ["oblique", "inside"] + params.PENCILS
# (full resolution, tile, offset)
SMALL_TILES = [((64, 48), (13, 7), (8, 8)), ((64, 48), (40, 24), (8, 8))]
BIG_TILE = ((256, 256), (256, 256), (0, 0))


# ------------------------------------------------------------------ media --
@lru_cache(maxsize=None)
def arrays(name, uniform, fmt):
    """(density (z, y, x), albedo (z, y, x, 4)) as format `fmt` stores them."""
    import cudavolumerenderer_amd as cvr
    if name == "blob16":
        d, a = params.blob16()
        if uniform:
            a = np.ones_like(a)
            a[..., :3] = (0.8, 0.6, 0.3)
    else:  # ragged: 24 x 17 x 19 voxels = 3 x 3 x 3 leaves, 11 of them empty, the others partly
        rng = np.random.default_rng(5)
        d = rng.random((19, 17, 24), dtype=F)
        d[rng.random(d.shape) < 0.5] = 0.0
        d[:8, :, 16:] = 0.0
        d[8:16, 8:16, 8:16] = 0.0
        d[16:, :8, :] = 0.0
        d[:, 16:, :8] = 0.0
        a = np.ones(d.shape + (4,), F)
        a[..., :3] = (0.7, 0.55, 0.33)
        if not uniform:
            a[..., :3] = np.where((d > 0)[..., None], 0.2 + 0.8 * rng.random(d.shape + (3,), dtype=F), a[..., :3])
        a[0, 0, 0, :3] = (0.7, 0.55, 0.33)  # the background of the leaf rule
        d[0, 0, 0] = 0.0
    d, a = np.ascontiguousarray(d, F), np.ascontiguousarray(a, F)
    if fmt:
        d, a = cvr.half_round(d), cvr.half_round(a)
    for x in (d, a):
        x.setflags(write=False)
    return d, a


@lru_cache(maxsize=None)
def host_planes(name, uniform, fmt, camera, geometry, desc=(1.0, 1.0 / 256.0, 4096)):
    import cudavolumerenderer_amd as cvr
    d, a = arrays(name, uniform, fmt)
    full, tile, off = geometry
    m, keep = cvr.medium_from_arrays(d, a, scale=SCALE, max_density=1.0)
    cam = params.camera(camera, full)
    return cvr.features_host(m, cam.inv_view, cam.r2v, full, tile, off, 0, cvr.FeaturesDesc(*desc))


def make_ctx(cvr, name, uniform=False, fmt=0, sparse=False, opts=()):
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
    for k, v in opts:
        ctx.set_option(k, v)
    d, a = arrays(name, uniform, 0)  # the context rounds by itself
    if sparse:
        sp = devmed.leaf_rule(d, a)
        assert (sp.table == devmed.NO_LEAF).sum() >= 8 and (sp.leaf_albedo is None) == uniform
        desc, keep = media.sparse_desc(cvr, sp.res, sp.table, sp.leaf_density, sp.leaf_albedo, sp.albedo_bg, 1.0)
        desc.scale = SCALE
        ctx.set_medium_sparse(desc)
    else:
        m, keep = cvr.medium_from_arrays(d, a, scale=SCALE, max_density=1.0)
        ctx.set_medium(m)
    return ctx


def view(ctx, camera, geometry):
    full, tile, off = geometry
    cam = params.camera(camera, full)
    ctx.set_camera(cam.inv_view, cam.r2v, full)
    ctx.set_resolution(*tile)
    ctx.set_offset(*off)


def assert_planes(got, want, what):
    assert np.array_equal(bits(got[0]), bits(want[0])), what + ": feat_rgba"
    assert np.array_equal(bits(got[1]), bits(want[1])), what + ": feat_depth"


# ------------------------------------------------ device == host, bit for bit --
def storages(cvr):
    return [
        ("blob16", False, ()),
        ("blob16", False, ((cvr.OPT_CELLS, 0),)),
        ("blob16", False, ((cvr.OPT_BOUNDS, 0),)),
        ("ragged", False, ()),
        ("ragged", True, ()),
        ("ragged", True, ((cvr.OPT_EMPTY_MASK, 0),)),
        ("ragged", True, ((cvr.OPT_CELLS, 0),)),
    ]


@pytest.mark.parametrize("storage", range(7))
@pytest.mark.parametrize("uniform", [False, True], ids=["varied", "uniform"])
@pytest.mark.parametrize("fmt", [0, 1], ids=["f32", "f16"])
def test_device_equals_host(cvr, storage, uniform, fmt):
    name, sparse, opts = storages(cvr)[storage]
    ctx = make_ctx(cvr, name, uniform, fmt, sparse, opts)
    try:
        lay = ctx.medium_layout().as_dict()
        assert lay["sparse"] == int(sparse) and (sparse or lay["albedo_uniform"] == int(uniform))
        lit = 0
        for camera in CAMERAS:
            for geometry in SMALL_TILES:
                view(ctx, camera, geometry)
                got = ctx.features()
                assert_planes(got, host_planes(name, uniform, fmt, camera, geometry), f"{camera} {geometry[1]}")
                lit += int((got[0][..., 3] > 0).sum())
        assert lit > 1000
        view(ctx, "oblique", BIG_TILE)
        got = ctx.features()
        assert_planes(got, host_planes(name, uniform, fmt, "oblique", BIG_TILE), "oblique 256x256")
        assert (got[0][..., 3] > 0.5).any() and (got[0][..., 3] == 0).any()
    finally:
        ctx.close()


def test_uniform_albedo_loaded_or_constant(cvr):
    """CVR_OPT_UNIFORM_ALBEDO 0 loads the uniform grid, 1 reads the constant: the same bits."""
    ctx = make_ctx(cvr, "blob16", True, 0, False, ((cvr.OPT_UNIFORM_ALBEDO, 0),))
    try:
        assert ctx.medium_layout().albedo_uniform == 0
        view(ctx, "oblique", SMALL_TILES[1])
        assert_planes(ctx.features(), host_planes("blob16", True, 0, "oblique", SMALL_TILES[1]), "loaded")
    finally:
        ctx.close()


def test_descriptor_and_buffers(cvr):
    """Other descriptors, the device-buffer entry point (torch tensors, depth optional) and pinned memory."""
    ctx = make_ctx(cvr, "ragged", False, 0, True)
    try:
        geometry = SMALL_TILES[1]
        view(ctx, "oblique", geometry)
        w, h = geometry[1]
        for desc in ((0.125, 0.0, 16), (0.5, 0.25, 4096), (8.0, 1.0 / 256.0, 3)):
            want = host_planes("ragged", False, 0, "oblique", geometry, desc)
            assert_planes(ctx.features(cvr.FeaturesDesc(*desc)), want, str(desc))
            rgba = torch.full((h, w, 4), float("nan"), device="cuda")
            depth = torch.full((h, w), float("nan"), device="cuda")
            only = torch.full((h, w, 4), float("nan"), device="cuda")
            torch.cuda.synchronize()  # the context runs on its own stream
            ctx.features_buffers(rgba, depth, cvr.FeaturesDesc(*desc))
            ctx.features_buffers(only, None, cvr.FeaturesDesc(*desc))
            ctx.synchronize()
            assert_planes((rgba.cpu().numpy(), depth.cpu().numpy()), want, f"buffers {desc}")
            assert np.array_equal(bits(only.cpu().numpy()), bits(want[0]))
        lib = cvr.load()
        import ctypes as C
        with cvr.PinnedImage(w, h) as pin:
            pin.array[:] = np.nan
            depth = np.zeros((h, w), F)
            d = cvr.FeaturesDesc()
            assert lib.cvr_features(ctx._h, C.byref(d), pin.ptr, C.c_void_p(depth.ctypes.data), pin.floats) == 0
            assert_planes((np.array(pin.array, copy=True).reshape(h, w, 4), depth),
                          host_planes("ragged", False, 0, "oblique", geometry), "pinned")
            assert lib.cvr_features(ctx._h, C.byref(d), pin.ptr, None, pin.floats - 1) == INVALID
            assert lib.cvr_features(ctx._h, C.byref(cvr.FeaturesDesc(9.0)), pin.ptr, None, pin.floats) == INVALID
            assert lib.cvr_features(ctx._h, None, pin.ptr, None, pin.floats) == INVALID
        t = torch.zeros((h, w, 4), device="cuda")
        with pytest.raises(cvr.CvrError) as e:
            ctx.features_buffers(t.data_ptr() + 4)
        assert e.value.code == INVALID and "aligned" in str(e.value)
        with pytest.raises(cvr.CvrError) as e:
            ctx.features_buffers(t, None, cvr.FeaturesDesc(1.0, 1.0))
        assert e.value.code == INVALID
    finally:
        ctx.close()
    empty = cvr.Context(0, "regenerationSK")
    try:
        with pytest.raises(cvr.CvrError) as e:
            empty.features()
        assert e.value.code == STATE and "medium" in str(e.value)
    finally:
        empty.close()


def test_shared_and_scalar_media(cvr):
    owner = make_ctx(cvr, "ragged", False, 1, True)
    sharer = cvr.Context(0, "regenerationSK")
    scalar = cvr.Context(0, "regenerationSK")
    try:
        sharer.share_medium(owner)
        view(sharer, "oblique", SMALL_TILES[1])
        assert_planes(sharer.features(), host_planes("ragged", False, 1, "oblique", SMALL_TILES[1]), "shared")
        # a medium classified on the device: the host statement on cvr_classify_host's arrays
        rng = np.random.default_rng(9)
        field = rng.integers(0, 256, (11, 13, 19), dtype=np.uint8)
        table = np.zeros((16, 4), F)
        table[:, :3] = 0.2 + 0.8 * rng.random((16, 3), dtype=F)
        table[4:, 3] = np.linspace(0.05, 1.0, 12, dtype=F)
        scalar.set_medium_scalar(torch.from_numpy(field).cuda(), table, lo=0.0, hi=255.0, scale=SCALE, max_density=1.0)
        d, a = cvr.classify_host(field, table, 0.0, 255.0)
        geometry = SMALL_TILES[1]
        view(scalar, "oblique", geometry)
        m, keep = cvr.medium_from_arrays(d, a, scale=SCALE, max_density=1.0)
        cam = params.camera("oblique", geometry[0])
        want = cvr.features_host(m, cam.inv_view, cam.r2v, *geometry)
        got = scalar.features()
        assert_planes(got, want, "scalar medium")
        assert (got[0][..., 3] > 0.5).any()
    finally:
        scalar.close()
        sharer.close()
        owner.close()


# ------------------------------------------------------ the context is read --
def test_context_is_untouched(cvr, oracle_mod):
    W = H = 32
    d, a = arrays("blob16", False, 0)
    ctx = make_ctx(cvr, "blob16")
    try:
        view(ctx, "oblique", ((W, H), (W, H), (0, 0)))
        ctx.set_seed(params.SEED)
        ctx.set_iterations(4)
        ctx.set_option(cvr.OPT_MOMENTS, 1)
        ctx.init()
        ctx.clear_output()
        ctx.launch_render()
        ctx.synchronize()
        s1, s2 = ctx.copy_moments()
        seed, st = ctx.get_seed(), ctx.stats().as_dict()
        planes = ctx.features()
        assert_planes(planes, host_planes("blob16", False, 0, "oblique", ((W, H), (W, H), (0, 0))), "after a render")
        a1, a2 = ctx.copy_moments()
        assert np.array_equal(bits(a1), bits(s1)) and np.array_equal(bits(a2), bits(s2))
        assert ctx.get_seed() == seed and ctx.stats().as_dict() == st
        assert st["paths"] == W * H * 4
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
    want = host_planes("blob16", False, 0, "oblique", geometry)
    results = []
    for with_features in (False, True):
        ctx = make_ctx(cvr, "blob16")
        try:
            view(ctx, "oblique", geometry)
            ctx.set_seed(3)
            ctx.init()
            with ctx.adaptive(cvr.AdaptiveDesc(2, 6, 1, -1.0, 0.01)) as a:  # one sample per launch: reproducible sums
                while not a.step().done:
                    if with_features:
                        assert_planes(ctx.features(), want, "inside the session")
                img = a.image()
                s1, s2 = ctx.copy_moments()
                _, smp = a.maps()
                if with_features:
                    guided = a.denoised_guided()
                    f4, fz = ctx.features()
                    assert np.array_equal(bits(guided),
                                          bits(cvr.denoise_guided_host(s1, s2, f4, fz, block_samples=smp)[0]))
                    assert not np.array_equal(bits(guided), bits(a.denoised()))
            results.append((img, s1, s2))
        finally:
            ctx.close()
    for x, y in zip(*results):
        assert np.array_equal(bits(x), bits(y))


# ------------------------------------------------------- the guided filter --
def device_guided(ctx, s1, s2, f4, fz, n, counts, desc, want_var=True):
    h, w = s1.shape[:2]
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (s1, s2, f4, fz)]
    dc = None if counts is None else torch.from_numpy(counts.astype(np.int32)).cuda()
    out = torch.full((h, w, 4), float("nan"), device="cuda")
    var = torch.full((h, w), float("nan"), device="cuda") if want_var else None
    torch.cuda.synchronize()
    ctx.denoise_guided_buffers(t[0], t[1], t[2], t[3], w, h, out, n_samples=n, block_samples=dc, desc=desc, out_var=var)
    ctx.synchronize()
    return out.cpu().numpy(), None if var is None else var.cpu().numpy()


def planes_for(h, w, seed):
    rng = np.random.default_rng(seed)
    f4 = rng.random((h, w, 4), dtype=F) * F(0.05)
    f4[:, w // 2:, :3] += F(0.6)
    f4[h // 2:, :, 3] += F(0.5)
    fz = np.ascontiguousarray(np.linspace(0, 1, w, dtype=F)[None, :] * np.ones((h, 1), F), F)
    return f4, fz


@pytest.mark.parametrize("h,w,use_map", [(7, 13, False), (24, 40, True), (72, 96, False)])
def test_guided_buffers_equal_host(cvr, h, w, use_map):
    ctx = cvr.Context(0, "regenerationSK")
    try:
        counts = two_count_map(h, w) if use_map else None
        s1, s2 = random_sums(h, w, counts if use_map else 8, 300 + w)
        if use_map:
            s1, s2, counts, _ = plant_invalid(s1, s2, counts)
        else:
            s1[h // 2, w // 3, 2] = np.nan
            s2[1, w - 1, 0] = np.inf
        n = None if use_map else 8
        f4, fz = planes_for(h, w, w)
        for passes in range(1, 7):
            desc = cvr.DenoiseGuidedDesc(cvr.DenoiseDesc(passes))
            want, wvar = cvr.denoise_guided_host(s1, s2, f4, fz, n, counts, desc)
            got, gvar = device_guided(ctx, s1, s2, f4, fz, n, counts, desc)
            assert np.array_equal(bits(got), bits(want)), passes
            assert np.array_equal(bits(gvar), bits(wvar)), passes
            off = cvr.DenoiseGuidedDesc(cvr.DenoiseDesc(passes), 0.0, -1.0, 0.0)
            got, gvar = device_guided(ctx, s1, s2, f4, fz, n, counts, off)
            d1, d2 = torch.from_numpy(s1).cuda(), torch.from_numpy(s2).cuda()
            dc = None if counts is None else torch.from_numpy(counts.astype(np.int32)).cuda()
            plain = torch.full((h, w, 4), float("nan"), device="cuda")
            torch.cuda.synchronize()
            ctx.denoise_buffers(d1, d2, w, h, plain, n_samples=n, block_samples=dc, desc=cvr.DenoiseDesc(passes))
            ctx.synchronize()
            assert np.array_equal(bits(got), bits(plain.cpu().numpy())), passes  # all sigmas off: cvr_denoise's bits
        one = cvr.DenoiseGuidedDesc(cvr.DenoiseDesc(3, 2.0, 0.05), 0.1, 0.0, 0.05)
        got, _ = device_guided(ctx, s1, s2, f4, fz, n, counts, one, want_var=False)
        assert np.array_equal(bits(got), bits(cvr.denoise_guided_host(s1, s2, f4, fz, n, counts, one)[0]))
        t = torch.zeros((8, 8, 4), device="cuda")
        z = torch.zeros((8, 8), device="cuda")
        for kw in (dict(desc=cvr.DenoiseGuidedDesc(None, float("nan"))), dict(desc=cvr.DenoiseGuidedDesc(cvr.DenoiseDesc(0))),
                   dict(n_samples=1), dict(feat_rgba=t.data_ptr() + 4)):
            args = dict(sum_rgba=t, m2_rgba=t, feat_rgba=t, feat_depth=z, width=8, height=8, out_rgba=t, n_samples=8)
            args.update(kw)
            with pytest.raises(cvr.CvrError) as e:
                ctx.denoise_guided_buffers(**args)
            assert e.value.code == INVALID, kw
    finally:
        ctx.close()


def test_context_denoise_guided_equals_host(cvr):
    W = H = 64
    geometry = ((W, H), (W, H), (0, 0))
    ctx = make_ctx(cvr, "blob16")
    try:
        view(ctx, "oblique", geometry)
        ctx.set_seed(7)
        ctx.set_iterations(8)
        ctx.set_option(cvr.OPT_MOMENTS, 1)
        ctx.init()
        ctx.clear_output()
        ctx.launch_render()
        ctx.synchronize()
        s1, s2 = ctx.copy_moments()
        f4, fz = host_planes("blob16", False, 0, "oblique", geometry)
        for desc in (None, cvr.DenoiseGuidedDesc(cvr.DenoiseDesc(2, 1.0, 0.02), 0.1, 0.05, 0.0)):
            img = ctx.denoise_guided(desc, n_samples=8)
            assert np.array_equal(bits(img), bits(cvr.denoise_guided_host(s1, s2, f4, fz, 8, desc=desc)[0]))
        with cvr.PinnedImage(W, H) as pin:
            pin.array[:] = np.nan
            pinned = np.array(ctx.denoise_guided(n_samples=8, host_ptr=pin), copy=True).reshape(H, W, 4)
        assert np.array_equal(bits(pinned), bits(img if desc is None else ctx.denoise_guided(n_samples=8)))
        off = cvr.DenoiseGuidedDesc(None, 0.0, 0.0, 0.0)
        assert np.array_equal(bits(ctx.denoise_guided(off, n_samples=8)), bits(ctx.denoise(n_samples=8)))
        a1, a2 = ctx.copy_moments()  # only read
        assert np.array_equal(bits(a1), bits(s1)) and np.array_equal(bits(a2), bits(s2))
        with pytest.raises(cvr.CvrError) as e:
            ctx.denoise_guided(n_samples=8, features=cvr.FeaturesDesc(0.0))
        assert e.value.code == INVALID
        ctx.set_option(cvr.OPT_MOMENTS, 0)
        with pytest.raises(cvr.CvrError) as e:
            ctx.denoise_guided(n_samples=8)
        assert e.value.code == STATE
    finally:
        ctx.close()


# --------------------------------------------------------------------- CLI --
def run_cli(*args):
    return subprocess.run([CLI, "--interactive", "0", "--synthetic", "bucky", "-r", "64", "64", *args],
                          capture_output=True, text=True, timeout=120)


def bucky_ctx(cvr, scene):
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_medium(scene.medium)
    iv, r2v = scene.camera(64, 64)
    ctx.set_camera(iv, r2v, (64, 64))
    ctx.set_resolution(64, 64)
    ctx.set_offset(0, 0)
    ctx.set_seed(0)
    ctx.init()
    return ctx


def test_cli_features(cvr, tmp_path):
    out = str(tmp_path / "f")
    r = run_cli("-i", "2", "--features", "--pfm", "-o", out)
    assert r.returncode == 0, r.stderr
    scene = cvr.Scene.synthetic("bucky")
    ctx = bucky_ctx(cvr, scene)
    try:
        f4, fz = ctx.features()
    finally:
        ctx.close()
    assert (f4[..., 3] > 0.5).any()
    for suffix in ("_albedo", "_alpha", "_depth"):
        assert os.path.getsize(out + suffix + ".hdr") > 0, suffix
    assert np.array_equal(bits(read_pfm(out + "_albedo.pfm")), bits(f4[..., :3]))
    for name, plane in (("_alpha", f4[..., 3]), ("_depth", fz)):
        img = read_pfm(out + name + ".pfm")
        for c in range(3):
            assert np.array_equal(bits(img[..., c]), bits(plane)), name
    half = str(tmp_path / "h")
    r = run_cli("-i", "2", "--features", "--feature-step", "0.5", "--pfm", "-o", half)
    assert r.returncode == 0, r.stderr
    assert not np.array_equal(bits(read_pfm(half + "_alpha.pfm")), bits(read_pfm(out + "_alpha.pfm")))
    r = run_cli("-i", "2", "--features", "--number-of-tiles", "2", "2")
    assert r.returncode == 2 and "--features renders one tile on one device" in r.stderr


def test_cli_denoise_guided(cvr, tmp_path):
    """`cvr --denoise-guided` twice: identical files (the sample-by-sample session of --denoise), and
    the bits of a Python session stepped the same way."""
    outs = [str(tmp_path / n) for n in ("a", "b")]
    for out in outs:
        r = run_cli("-i", "8", "--denoise-guided", "--pfm", "-o", out)
        assert r.returncode == 0, r.stderr
    for suffix in (".pfm", "_denoised.pfm", "_denoised.hdr"):
        assert open(outs[0] + suffix, "rb").read() == open(outs[1] + suffix, "rb").read(), suffix
    scene = cvr.Scene.synthetic("bucky")
    ctx = bucky_ctx(cvr, scene)
    try:
        with ctx.adaptive(cvr.AdaptiveDesc(2, 8, 1, -1.0, 0.01)) as a:
            while not a.step().done:
                pass
            want, plain, image = a.denoised_guided(), a.denoised(), a.image()
    finally:
        ctx.close()
    assert np.array_equal(bits(read_pfm(outs[0] + ".pfm")), bits(image[..., :3]))
    assert np.array_equal(bits(read_pfm(outs[0] + "_denoised.pfm")), bits(want[..., :3]))
    assert not np.array_equal(bits(want), bits(plain))
    other = str(tmp_path / "c")
    r = run_cli("-i", "8", "--denoise-guided", "--guide-sigma", "0", "0", "0", "--pfm", "-o", other)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(bits(read_pfm(other + "_denoised.pfm")), bits(plain[..., :3]))  # all terms off: --denoise
    r = run_cli("-i", "8", "--denoise-guided", "--denoise")
    assert r.returncode == 2 and "excludes --denoise" in r.stderr
    r = run_cli("-i", "8", "--denoise-guided", "--number-of-tiles", "2", "2")
    assert r.returncode == 2 and "--denoise-guided renders one tile on one device" in r.stderr
