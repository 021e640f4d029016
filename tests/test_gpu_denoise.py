"""The denoiser on the GPU: k_denoise_prepare / k_denoise_pass run the per-pixel functions that
cvr_denoise_host runs on the CPU (csrc/cvr_kernels.h), fp32 in the written order with no fused
multiply-add, so every comparison here is of bits (uint32 views), never within a tolerance.

Shapes: 8x8 (one partial tile, every pixel at a border), 72x40 and 40x72 (partial 32x8 tiles in
x; whole block maps), 70x37 (partial tiles on both axes, uniform N only), 64x64 for passes 1..6.
The sums are those of tests/test_denoise_cpu.py, planted invalid pixels included.

Two separate renders (the CLI's and a Python session's) are compared bit for bit too: `cvr
--denoise` adds at most two samples per pixel per launch, which makes its sums reproducible
(test_cli_denoised_equals_python_bits)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_distributed_cpu.py and bench.py do)

from parity_util import assert_pixels_close
from test_denoise_cpu import bits, plant_invalid, random_sums, two_count_map

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cudavolumerenderer_amd", "cvr")
W = H = 64
STATE, INVALID = -3, -1


@pytest.fixture(scope="module")
def bucky(cvr):
    return cvr.Scene.synthetic("bucky")


def make_ctx(cvr, scene, seed=7, camera=None):
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_medium(scene.medium)
    iv, r2v = camera if camera is not None else cvr.default_camera(W, H)
    ctx.set_camera(iv, r2v, (W, H))
    ctx.set_resolution(W, H)
    ctx.set_offset(0, 0)
    ctx.set_seed(seed)
    ctx.init()
    return ctx


# ------------------------------------------------ device == host, bit for bit --
def device_denoise(ctx, s1, s2, n, counts, desc, want_var=True):
    h, w = s1.shape[:2]
    d1, d2 = torch.from_numpy(s1).cuda(), torch.from_numpy(s2).cuda()
    dc = None if counts is None else torch.from_numpy(counts.astype(np.int32)).cuda()
    out = torch.full((h, w, 4), float("nan"), device="cuda")
    var = torch.full((h, w), float("nan"), device="cuda") if want_var else None
    torch.cuda.synchronize()  # the context runs on its own stream
    ctx.denoise_buffers(d1, d2, w, h, out, n_samples=n, block_samples=dc, desc=desc, out_var=var)
    ctx.synchronize()
    assert np.array_equal(bits(d1.cpu().numpy()), bits(s1)) and np.array_equal(bits(d2.cpu().numpy()), bits(s2))
    return out.cpu().numpy(), None if var is None else var.cpu().numpy()


BUFFER_CASES = [(8, 8, (5,)), (40, 72, (5,)), (72, 40, (3,)), (37, 70, (5,)), (64, 64, (1, 2, 3, 4, 5, 6))]


@pytest.mark.parametrize("h,w,passes", BUFFER_CASES)
def test_buffers_equal_host(cvr, h, w, passes):
    ctx = cvr.Context(0, "regenerationSK")
    try:
        s1, s2 = random_sums(h, w, 8, 100 + w)
        s1[h // 2, w // 3, 2] = np.nan  # invalid pixels in the uniform case too
        s2[1, w - 1, 0] = np.inf
        cases = [(s1, s2, 8, None)]
        if h % 8 == 0 and w % 8 == 0:
            counts = two_count_map(h, w)
            m1, m2 = random_sums(h, w, counts, 200 + w)
            if h >= 16:
                m1, m2, counts, _ = plant_invalid(m1, m2, counts)
            cases.append((m1, m2, None, counts))
        for a, b, n, counts in cases:
            for p in passes:
                desc = cvr.DenoiseDesc(p)
                want, wvar = cvr.denoise_host(a, b, n, counts, desc)
                got, gvar = device_denoise(ctx, a, b, n, counts, desc)
                what = f"{w}x{h} passes {p} {'map' if n is None else 'uniform'}"
                assert np.array_equal(bits(got), bits(want)), what
                assert np.array_equal(bits(gvar), bits(wvar)), what
        got, _ = device_denoise(ctx, s1, s2, 8, None, cvr.DenoiseDesc(2, 2.0, 0.05), want_var=False)
        assert np.array_equal(bits(got), bits(cvr.denoise_host(s1, s2, 8, None, cvr.DenoiseDesc(2, 2.0, 0.05))[0]))
    finally:
        ctx.close()


# ------------------------------------------------- the context's own buffers --
@pytest.fixture(scope="module")
def rendered(cvr, bucky):
    """A context holding 8 samples of bucky with moments, and its sums."""
    ctx = make_ctx(cvr, bucky)
    ctx.set_iterations(8)
    ctx.set_option(cvr.OPT_MOMENTS, 1)
    ctx.clear_output()
    ctx.launch_render()
    ctx.synchronize()
    s1, s2 = ctx.copy_moments()
    yield ctx, s1, s2
    ctx.close()


def test_context_denoise_equals_host(cvr, rendered):
    ctx, s1, s2 = rendered
    assert (s2[..., 3] > 1).any()
    img = ctx.denoise(n_samples=8)
    want, _ = cvr.denoise_host(s1, s2, 8)
    assert np.array_equal(bits(img), bits(want))
    assert np.isfinite(img).all() and img[..., :3].max() > 0
    a1, a2 = ctx.copy_moments()  # only read
    assert np.array_equal(bits(a1), bits(s1)) and np.array_equal(bits(a2), bits(s2))
    img2 = ctx.denoise(cvr.DenoiseDesc(2, 1.0, 0.02), n_samples=8)
    assert np.array_equal(bits(img2), bits(cvr.denoise_host(s1, s2, 8, desc=cvr.DenoiseDesc(2, 1.0, 0.02))[0]))
    assert not np.array_equal(bits(img2), bits(img))


def test_pinned_and_pageable_destinations_agree(cvr, rendered):
    ctx, s1, s2 = rendered
    with cvr.PinnedImage(W, H) as pin:
        pin.array[:] = np.nan
        got = np.array(ctx.denoise(n_samples=8, host_ptr=pin), copy=True)
    plain = ctx.denoise(n_samples=8)
    assert got.tobytes() == plain.tobytes()
    assert np.array_equal(bits(plain), bits(cvr.denoise_host(s1, s2, 8)[0]))


def test_adaptive_session_denoised(cvr, bucky):
    ctx = make_ctx(cvr, bucky)
    try:
        with ctx.adaptive(cvr.AdaptiveDesc(8, 32, 4, 0.1, 0.01)) as a:
            early = a.denoised()  # before the first pass no block has samples: nothing is valid
            assert (early == 0).all()
            while not a.step().done:
                pass
            img = a.denoised()
            with cvr.PinnedImage(W, H) as pin:
                pinned = np.array(a.denoised(host_ptr=pin), copy=True)
            s1, s2 = ctx.copy_moments()
            _, smp = a.maps()
            with pytest.raises(cvr.CvrError) as e:  # a count of the caller's inside a session
                ctx.denoise(n_samples=8)
            assert e.value.code == INVALID and "session" in str(e.value)
        assert len(np.unique(smp)) > 1
        want, _ = cvr.denoise_host(s1, s2, block_samples=smp)
        assert np.array_equal(bits(img), bits(want)) and np.array_equal(bits(pinned), bits(want))
        with pytest.raises(cvr.CvrError) as e:  # the session has ended and the moments are off again
            a.denoised()
        assert e.value.code == STATE
    finally:
        ctx.close()


def test_refusals(cvr, bucky, rendered):
    lib = cvr.load()
    ctx, _, _ = rendered
    desc = cvr.DenoiseDesc()
    img = np.zeros((H, W, 4), np.float32)
    ptr = C.c_void_p(img.ctypes.data)
    assert lib.cvr_denoise(ctx._h, C.byref(desc), 8, ptr, img.size) == 0
    assert lib.cvr_denoise(ctx._h, C.byref(desc), 8, ptr, img.size - 1) == INVALID  # a short host buffer
    assert lib.cvr_denoise(ctx._h, C.byref(desc), 0, ptr, img.size) == INVALID      # no count outside a session
    assert lib.cvr_denoise(ctx._h, C.byref(desc), 1, ptr, img.size) == INVALID
    assert lib.cvr_denoise(ctx._h, None, 8, ptr, img.size) == INVALID
    assert lib.cvr_denoise(ctx._h, C.byref(desc), 8, None, img.size) == INVALID
    assert lib.cvr_denoise(ctx._h, C.byref(cvr.DenoiseDesc(7)), 8, ptr, img.size) == INVALID
    assert lib.cvr_denoise(ctx._h, C.byref(cvr.DenoiseDesc(5, 4.0, 0.0)), 8, ptr, img.size) == INVALID
    plain = make_ctx(cvr, bucky)
    try:
        with pytest.raises(cvr.CvrError) as e:  # moments off
            plain.denoise(n_samples=8)
        assert e.value.code == STATE and "moments" in str(e.value)
        # cvr_denoise_buffers checks its arguments before anything is launched
        d = torch.zeros((16, 16, 4), device="cuda")
        torch.cuda.synchronize()
        for kw in (dict(n_samples=1), dict(n_samples=8, desc=cvr.DenoiseDesc(0)), dict(n_samples=8, width=0),
                   dict(block_samples=d, width=12)):
            args = dict(sum_rgba=d, m2_rgba=d, width=16, height=16, out_rgba=d)
            args.update(kw)
            with pytest.raises(cvr.CvrError) as e:
                plain.denoise_buffers(**args)
            assert e.value.code == INVALID, kw
        with pytest.raises(cvr.CvrError) as e:  # an unaligned rgba buffer
            plain.denoise_buffers(d.data_ptr() + 4, d, 8, 8, d, n_samples=8)
        assert e.value.code == INVALID and "aligned" in str(e.value)
    finally:
        plain.close()


# --------------------------------------------------------------------- CLI --
def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n"
        w, h = (int(v) for v in f.readline().split())
        assert float(f.readline()) < 0  # little-endian
        data = np.frombuffer(f.read(), "<f4").reshape(h, w, 3)
    return data[::-1]  # rows are stored bottom to top


@pytest.fixture(scope="module")
def cli_run(cvr, bucky, tmp_path_factory):
    """`cvr --synthetic bucky -r 64 64 -i 8 --denoise --pfm`, and the library's own run of the same
    render from Python (the CLI's seed 0 and scene camera): a session that never stops a block, two
    samples in its first pass and one in each later pass, as the CLI runs it.
    -> (CLI image, CLI denoised, Python image, Python denoised, one-launch Python image), rgb."""
    out = str(tmp_path_factory.mktemp("cli") / "x")
    r = subprocess.run([CLI, "--interactive", "0", "--synthetic", "bucky", "-r", "64", "64", "-i", "8", "--denoise",
                        "--pfm", "-o", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for suffix in (".hdr", ".pfm", "_denoised.hdr", "_denoised.pfm"):
        assert os.path.getsize(out + suffix) > 0, suffix
    ctx = make_ctx(cvr, bucky, seed=0, camera=bucky.camera(W, H))
    try:
        with ctx.adaptive(cvr.AdaptiveDesc(2, 8, 1, -1.0, 0.01)) as a:
            while not a.step().done:
                pass
            assert a.result.passes == 7
            want = a.denoised()
            plain = a.image()
        ctx.set_seed(0)
        with ctx.adaptive(cvr.AdaptiveDesc(8, 8, 8, -1.0, 0.01)) as a:
            assert a.step().done
            one_launch = a.image()
    finally:
        ctx.close()
    return (read_pfm(out + ".pfm"), read_pfm(out + "_denoised.pfm"), plain[..., :3], want[..., :3],
            one_launch[..., :3])


def test_cli_denoised_equals_python_bits(cli_run):
    """The CLI's <output>_denoised.pfm against the Python path's result for the same seed, bit for
    bit.  These are two separate renders, and a render that adds all 8 samples of a pixel in one
    launch is not reproducible in its last bit: the wave pool adds them with float atomics in
    arrival order (measured on such launches: 16 to 28 of the 4096 pixels of S1 differ by one ulp
    from run to run, which the filter carries into 586 to 1536 pixels of its output, <= 4.8e-7).
    So `cvr --denoise` renders two samples in its first launch and one in each later launch: a
    launch then adds two values onto zero or one value onto a sum, fp32 addition commutes, and
    launches on one stream are ordered, so every run leaves the same bits in both sums."""
    cli_img, cli_den, py_img, py_den, _ = cli_run
    for name, a, b in (("image", cli_img, py_img), ("denoised", cli_den, py_den)):
        differ = int((bits(a) != bits(b)).any(-1).sum())
        print(f"cli vs python, {name}: {differ} of {W * H} pixels differ in bits, "
              f"largest |difference| {np.abs(a.astype(np.float64) - b).max():.3g}")
    assert np.array_equal(bits(cli_img), bits(py_img))
    assert np.array_equal(bits(cli_den), bits(py_den))


def test_cli_denoise_outputs_and_refusals(cli_run):
    """The CLI's sample-by-sample session renders the paths of the one-launch render: the images
    agree up to the summation order of a pixel's 8 samples (the bound of parity_util).  The
    filtered image is finite and smoother than the image."""
    cli_img, cli_den, py_img, py_den, one_launch = cli_run
    assert_pixels_close(cli_img, one_launch, 8, "cli vs one-launch image")
    assert np.isfinite(cli_den).all() and cli_den.shape == (H, W, 3)

    def roughness(x):  # mean squared difference between horizontal neighbours
        return float(((x[:, 1:] - x[:, :-1]).astype(np.float64) ** 2).mean())

    assert roughness(cli_den) < roughness(cli_img)
    # refusals before anything renders
    r = subprocess.run([CLI, "--interactive", "0", "--synthetic", "bucky", "-r", "64", "-i", "8", "--denoise",
                        "--number-of-tiles", "2", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--denoise renders one tile on one device" in r.stderr
    r = subprocess.run([CLI, "--interactive", "0", "--synthetic", "bucky", "-r", "64", "-i", "1", "--denoise"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--iterations of at least 2" in r.stderr
