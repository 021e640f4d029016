"""The field projections on the GPU.  k_project runs project_pixel (csrc/cvr_project.h), the
definition cvr_field_project_host runs on the CPU: every comparison here is of bits (uint32 views)
on the rgba, value and depth planes, never within a tolerance.

Fields, windows and levels are those of tests/test_project_cpu.py.  Tiles: one 72x40 image (45 wave
blocks, the last column and row of workgroups half empty) and the ragged 19x13 tile at offset (8, 8)
of 64x48.  Cameras: "oblique", "inside" and one that misses the box."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import params
from test_gpu_denoise import read_pfm
from test_gpu_features import make_ctx, run_cli
from test_project_cpu import BOX, MODES, TYPES, UNIT, bits, camera, field, span

pytestmark = pytest.mark.gpu

STATE, INVALID = -3, -1
F = np.float32
# (full resolution, tile, offset)
WIDE = ((72, 40), (72, 40), (0, 0))
RAGGED = ((64, 48), (19, 13), (8, 8))
LOOK = dict(background=(0.25, 0.5, 0.125), colour=(0.9, 0.6, 0.3))


def desc_for(cvr, a, mode, box=UNIT, **kw):
    lo, hi, iso = span(a) if a.dtype != np.float32 or np.isfinite(a).all() else (0.2, 0.8, 0.6)
    return cvr.ProjectDesc(mode, box[0], box[1], **dict(dict(lo=lo, hi=hi, iso=iso), **kw))


def view(ctx, cam, geometry):
    full, tile, off = geometry
    c = camera(cam, full)
    ctx.set_camera(c.inv_view, c.r2v, full)
    ctx.set_resolution(*tile)
    ctx.set_offset(*off)


def host(cvr, a, desc, cam, geometry):
    full, tile, off = geometry
    c = camera(cam, full)
    return cvr.field_project_host(a, c.inv_view, c.r2v, full, desc, tile, off)


def assert_planes(got, want, what):
    for name, g, w in zip(("rgba", "value", "depth"), got, want):
        assert np.array_equal(bits(g), bits(w)), f"{what}: {name}"


@pytest.fixture
def ctx(cvr):
    c = cvr.Context(0, "regenerationSK")  # no medium: the calls need none
    yield c
    c.close()


# ------------------------------------------------ device == host, bit for bit --
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", TYPES)
def test_device_equals_host(cvr, ctx, dtype, mode):
    a = field("ragged_" + dtype)
    t = torch.from_numpy(a.copy()).cuda()
    for cam, geometry, kw in (("oblique", WIDE, dict(LOOK)), ("oblique", RAGGED, dict(LOOK, box=BOX, step=0.5)),
                              ("inside", RAGGED, dict(LOOK, light=(0.3, 1.0, -0.4), refine=8)),
                              ("away", RAGGED, dict(LOOK, max_steps=5))):
        d = desc_for(cvr, a, mode, **kw)
        view(ctx, cam, geometry)
        got, want = ctx.field_project(t, d), host(cvr, a, d, cam, geometry)
        assert_planes(got, want, f"{dtype} {mode} {cam} {geometry[1]}")
        if cam == "oblique":
            assert (got[0][..., 3] == 1).sum() > 50
        elif cam == "away":
            assert (got[0][..., 3] == 0).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int16"])
def test_view_one_element_into_the_allocation(cvr, ctx, dtype, mode):
    a = field("ragged_" + dtype)
    raw = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
    buf = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device="cuda")
    buf[a.itemsize:a.itemsize + raw.numel()] = raw
    t = buf[a.itemsize:a.itemsize + raw.numel()].view(getattr(torch, dtype)).view(a.shape)
    assert t.data_ptr() == buf.data_ptr() + a.itemsize and t.data_ptr() % 16 == a.itemsize and t.is_contiguous()
    d = desc_for(cvr, a, mode, **LOOK)
    view(ctx, "oblique", RAGGED)
    assert_planes(ctx.field_project(t, d), host(cvr, a, d, "oblique", RAGGED), f"{dtype} {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["thin", "nan", "allnan"])
def test_small_and_nan_fields(cvr, ctx, name, mode):
    a = field(name)
    t = torch.from_numpy(a.copy()).cuda()
    d = desc_for(cvr, a, mode, **LOOK)
    for cam in ("oblique", "inside"):
        view(ctx, cam, RAGGED)
        got = ctx.field_project(t, d)
        assert_planes(got, host(cvr, a, d, cam, RAGGED), f"{name} {mode} {cam}")
        if name == "allnan":
            assert (got[0] == np.array([0.25, 0.5, 0.125, 0.0], F)).all() and not got[1].any() and not got[2].any()


# ------------------------------------------------ a voxel index past 2^31 ----
BIG = (2049, 1024, 1024)      # (z, y, x): 2^31 + 2^20 voxels, the last z layer past index 2^31
BIG_BLOCK = 32
# just outside the far corner, looking down -z through the block's 32 x 32 cells of the + z face:
# at the block's far side, 0.036 from the eye, the 30 degree view is 0.019 wide, inside the block's 0.031
BIG_EYE, BIG_AT, BIG_FOV = (0.488, 0.482, 0.52), (0.4853, 0.4853, 0.4922), 30.0


def big_block():
    return np.random.default_rng(17).integers(1, 256, (BIG_BLOCK,) * 3).astype(np.uint8)


def test_field_index_past_2_31(cvr, ctx):
    """A uint8 field of 1024 x 1024 x 2049 voxels, zero but for a 32^3 block of random values at the
    far corner, whose last z layer lies past voxel index 2^31: the host statement reads the same
    array through size_t.  The camera's rays enter through that layer."""
    block = big_block()
    t = torch.zeros(BIG, dtype=torch.uint8, device="cuda")
    t[-BIG_BLOCK:, -BIG_BLOCK:, -BIG_BLOCK:] = torch.from_numpy(block).cuda()
    a = np.zeros(BIG, np.uint8)   # (untouched pages are never read: the host statement reads only the taps)
    a[-BIG_BLOCK:, -BIG_BLOCK:, -BIG_BLOCK:] = block
    assert a.size == (1 << 31) + (1 << 20) and a.reshape(-1)[1 << 31:].any()
    full = (32, 32)
    c = params.look_at(BIG_EYE, BIG_AT, fov=BIG_FOV, full=full)
    ctx.set_camera(c.inv_view, c.r2v, full)
    ctx.set_resolution(*full)
    ctx.set_offset(0, 0)
    for mode in ("max", "mean", "iso"):
        d = cvr.ProjectDesc(mode, UNIT[0], UNIT[1], lo=0.0, hi=255.0, iso=128.0, refine=4, **LOOK)
        want = cvr.field_project_host(a, c.inv_view, c.r2v, full, d)
        share = float((want[1] != 0).mean())
        print(f"{mode}: {100 * share:.1f} % of the pixels have a value")
        assert share >= 0.95, mode
        assert_planes(ctx.field_project(t, d), want, f"2^31 + 2^20 voxels, {mode}")


def test_field_past_2_32_is_refused(cvr, ctx):
    """More than 2^32 - 1 voxels: refused before the field is read (a one-element dummy)."""
    one = torch.zeros(1, dtype=torch.uint8, device="cuda")
    ctx.set_resolution(8, 8)
    c = camera("oblique", (8, 8))
    ctx.set_camera(c.inv_view, c.r2v, (8, 8))
    rgba = torch.zeros((8, 8, 4), device="cuda")
    for res in ((65536, 65536, 1), (1024, 1024, 4096)):
        with pytest.raises(cvr.CvrError) as e:
            ctx.field_project_buffers(one.data_ptr(), rgba, None, None, cvr.ProjectDesc("max"), scalar_type=cvr.SCALAR_U8, res=res)
        assert e.value.code == INVALID and "more than 2^32 - 1" in str(e.value)
        with pytest.raises(cvr.CvrError) as e:
            ctx.field_project(one.data_ptr(), cvr.ProjectDesc("max"), scalar_type=cvr.SCALAR_U8, res=res)
        assert e.value.code == INVALID and "more than 2^32 - 1" in str(e.value)


# ----------------------------------------------------------- entry points ----
def test_destinations(cvr, ctx):
    lib = cvr.load()
    a = field("ragged_uint16")
    t = torch.from_numpy(a.copy()).cuda()
    view(ctx, "oblique", RAGGED)
    w, h = RAGGED[1]
    for mode in ("max", "iso"):
        d = desc_for(cvr, a, mode, **LOOK)
        want = host(cvr, a, d, "oblique", RAGGED)
        # device tensors, with and without the two planes
        rgba = torch.full((h, w, 4), float("nan"), device="cuda")
        value, depth = torch.full((h, w), float("nan"), device="cuda"), torch.full((h, w), float("nan"), device="cuda")
        torch.cuda.synchronize()  # the context runs on its own stream
        ctx.field_project_buffers(t, rgba, value, depth, d)
        ctx.synchronize()
        assert_planes((rgba.cpu().numpy(), value.cpu().numpy(), depth.cpu().numpy()), want, f"buffers {mode}")
        rgba.fill_(float("nan"))
        torch.cuda.synchronize()
        ctx.field_project_buffers(t, rgba, None, None, d)
        ctx.synchronize()
        assert np.array_equal(bits(rgba.cpu().numpy()), bits(want[0])), "buffers, rgba alone"
        # pageable host memory, all planes and rgba alone
        assert_planes(ctx.field_project(t, d), want, f"pageable {mode}")
        got = ctx.field_project(t, d, value=False, depth=False)
        assert got[1] is None and got[2] is None and np.array_equal(bits(got[0]), bits(want[0]))
        got = ctx.field_project(t, d, value=False)
        assert got[1] is None and np.array_equal(bits(got[2]), bits(want[2]))
        f = ctx._device_field("test", t, (1.0, 1.0, 1.0), None, None)[0]
        # pinned rgba, pageable value and depth: one plane stored by the kernel, two staged
        with cvr.PinnedImage(w, h) as pin:
            pin.array[:] = np.nan
            v, z = np.full((h, w), np.nan, F), np.full((h, w), np.nan, F)
            assert lib.cvr_field_project(ctx._h, C.byref(f), C.byref(d), pin.ptr, v.ctypes.data, z.ctypes.data, pin.floats) == 0
            assert_planes((np.array(pin.array, copy=True), v, z), want, f"pinned {mode}")
            assert lib.cvr_field_project(ctx._h, C.byref(f), C.byref(d), pin.ptr, None, None, pin.floats - 1) == INVALID
        # registered host memory, all three planes in one registration
        raw = np.full(w * h * 6 + 1024, np.nan, F)
        start = (-raw.ctypes.data // 4) % 1024  # a page-aligned window of the array
        reg = raw[start:start + w * h * 6]
        rt = torch.cuda.cudart()
        assert int(rt.cudaHostRegister(reg.ctypes.data, reg.nbytes, 0)) == 0
        try:
            base = reg.ctypes.data
            assert lib.cvr_field_project(ctx._h, C.byref(f), C.byref(d), base, base + w * h * 16, base + w * h * 20,
                                         w * h * 4) == 0
            got = (reg[:w * h * 4].reshape(h, w, 4), reg[w * h * 4:w * h * 5].reshape(h, w), reg[w * h * 5:].reshape(h, w))
            assert_planes(got, want, f"registered {mode}")
        finally:
            rt.cudaHostUnregister(reg.ctypes.data)
    # refusals of the device calls
    rgba = torch.zeros((h, w, 4), device="cuda")
    with pytest.raises(cvr.CvrError) as e:
        ctx.field_project_buffers(t, rgba.data_ptr() + 4, None, None, d)
    assert e.value.code == INVALID and "aligned" in str(e.value)
    with pytest.raises(cvr.CvrError) as e:
        ctx.field_project_buffers(t, np.zeros((h, w, 4), F).ctypes.data, None, None, d)
    assert e.value.code == INVALID and "device-accessible" in str(e.value)
    with pytest.raises(cvr.CvrError) as e:
        ctx.field_project_buffers(a.ctypes.data, rgba, None, None, d, scalar_type=cvr.SCALAR_U16, res=a.shape[::-1])
    assert e.value.code == INVALID and "device-accessible" in str(e.value)
    with pytest.raises(cvr.CvrError) as e:
        ctx.field_project(t, cvr.ProjectDesc("iso", refine=9))
    assert e.value.code == INVALID and "refine" in str(e.value)


def test_without_a_camera(cvr):
    a = field("ragged_uint8")
    t = torch.from_numpy(a.copy()).cuda()
    ctx = cvr.Context(0, "regenerationSK")
    try:
        ctx.set_resolution(8, 8)
        with pytest.raises(cvr.CvrError) as e:
            ctx.field_project(t, desc_for(cvr, a, "max"))
        assert e.value.code == STATE and "camera" in str(e.value)
        rgba = torch.zeros((8, 8, 4), device="cuda")
        with pytest.raises(cvr.CvrError) as e:
            ctx.field_project_buffers(t, rgba, None, None, desc_for(cvr, a, "iso"))
        assert e.value.code == STATE
    finally:
        ctx.close()


# ------------------------------------------------------ the context is read --
def test_context_is_untouched(cvr):
    W = H = 32
    geometry = ((W, H), (W, H), (0, 0))
    a = field("ragged_uint8")
    t = torch.from_numpy(a.copy()).cuda()
    d = desc_for(cvr, a, "iso", **LOOK)
    want = host(cvr, a, d, "oblique", geometry)
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
        seed, st, info = ctx.get_seed(), ctx.stats().as_dict(), bytes(ctx.medium_info())
        for mode in MODES:
            dm = desc_for(cvr, a, mode, **LOOK)
            assert_planes(ctx.field_project(t, dm), host(cvr, a, dm, "oblique", geometry), mode)
        a1, a2 = ctx.copy_moments()
        assert np.array_equal(bits(a1), bits(s1)) and np.array_equal(bits(a2), bits(s2))
        assert ctx.get_seed() == seed and ctx.stats().as_dict() == st and st["paths"] == W * H * 4
        assert bytes(ctx.medium_info()) == info
    finally:
        ctx.close()
    # inside an adaptive session: the session's result does not change
    results = []
    for with_projection in (False, True):
        ctx = make_ctx(cvr, "blob16")
        try:
            view(ctx, "oblique", geometry)
            ctx.set_seed(3)
            ctx.init()
            with ctx.adaptive(cvr.AdaptiveDesc(2, 6, 1, -1.0, 0.01)) as s:  # one sample per launch: reproducible sums
                while not s.step().done:
                    if with_projection:
                        assert_planes(ctx.field_project(t, d), want, "inside the session")
                img = s.image()
                m1, m2 = ctx.copy_moments()
            results.append((img, m1, m2))
        finally:
            ctx.close()
    for x, y in zip(*results):
        assert np.array_equal(bits(x), bits(y))


# --------------------------------------------------------------------- CLI --
def test_cli_project(cvr, tmp_path):
    scene = cvr.Scene.synthetic("bucky")
    raw = np.frombuffer(scene.raw_bytes, np.uint8).reshape(32, 32, 32).copy()
    md = scene.medium
    box = (tuple(md.box_min), tuple(md.box_max))
    t = torch.from_numpy(raw).cuda()
    ctx = cvr.Context(0, "regenerationSK")
    try:
        iv, r2v = scene.camera(64, 64)
        ctx.set_camera(iv, r2v, (64, 64))
        ctx.set_resolution(64, 64)
        top = float(raw.max())
        iso = ctx.field_project(t, cvr.ProjectDesc("iso", *box, iso=0.5 * top))[0]
        lit = ctx.field_project(t, cvr.ProjectDesc("iso", *box, iso=90.0, step=0.5, refine=2, light=(1.0, 2.0, 0.5), ambient=0.2,
                                                   diffuse=0.6, specular=0.4, shininess_log2=3, colour=(0.9, 0.6, 0.3),
                                                   background=(0.5, 0.25, 0.125)))[0]
        mip = ctx.field_project(t, cvr.ProjectDesc("max", *box, lo=0.0, hi=top))[0]
        mean = ctx.field_project(t, cvr.ProjectDesc("mean", *box, lo=10.0, hi=100.0))[0]
    finally:
        ctx.close()
    assert (iso[..., 3] == 1).sum() > 100 and (iso[..., 3] == 0).sum() > 100

    def cli(want, *args):
        out = str(tmp_path / "p.hdr")
        r = run_cli("-i", "0", "--pfm", *args[:1], args[1], out, *args[2:])
        assert r.returncode == 0, r.stderr
        assert "rendering time" not in r.stdout and "projection" in r.stdout  # no render
        assert os.path.getsize(out) > 0
        assert np.array_equal(bits(read_pfm(out + ".pfm")), bits(want[..., :3]))

    cli(iso, "--project", "iso")
    cli(lit, "--project", "iso", "--iso", "90", "--project-step", "0.5", "--project-refine", "2", "--preview-light", "1", "2",
        "0.5", "--preview-shading", "0.2", "0.6", "0.4", "3", "--project-colour", "0.9", "0.6", "0.3", "--preview-background",
        "0.5", "0.25", "0.125")
    cli(mip, "--project", "max")
    cli(mean, "--project", "mean", "--project-window", "10", "100")
    out = str(tmp_path / "q.hdr")
    r = run_cli("-i", "0", "--project", "iso", out, "--number-of-tiles", "2", "2")
    assert r.returncode == 2 and "--project renders one tile on one device" in r.stderr
    r = run_cli("-i", "0", "--project", "iso", out, "--project-refine", "9")
    assert r.returncode == 1 and "refine" in r.stderr
    r = run_cli("-i", "0", "--project", "median", out)
    assert r.returncode == 2 and "--project takes" in r.stderr
