"""The half medium format (CVR_OPT_MEDIUM_FORMAT 1): density, density cells and
albedo stored as IEEE binary16 on the device.

A half converts to fp32 exactly and everything after the load is fp32, so a
format-1 render must be bit-identical per path to the fp32 render of the
rounded medium with the majorant max_density_eff = max(max_density,
f32(f16(max_density))).  Every check here is against oracle.Oracle built from
cvr.half_round()ed arrays and that majorant: per-path records (image id, flags,
T bits, segments; step / density / albedo counts through cvr_trace_paths), launch
counters, and pixels within the summation-order bound (parity_util).

Scenes are the smallest that take every path of the code: a dense 19x13x11 grid
(no multiple of the 4^3 brick, ~40 % zeros, planted fp16 subnormal / flush-to-
zero / tie values), the same with a uniform albedo, and a sparse 20x12x28 index
box with about half of its 8^3 leaves absent."""
import numpy as np
import pytest

from media import SCALE, dense_arrays, sparse_arrays, sparse_desc
from parity_util import (COUNTERS, NTHREADS, assert_counters_equal, assert_pixels_close, gpu_range_render,
                         oracle_image)

pytestmark = pytest.mark.gpu

TILE = (16, 16)
ITERS = 4  # 1024 paths


# ------------------------------------------------------------------ scenes --
def md_eff(cvr, md):
    h = float(cvr.half_round(np.array([md], np.float32))[0])
    return max(float(np.float32(md)), h)


def dense_ctx(cvr, d, a, md, kernel="regenerationSK", fmt=1, res=TILE, opts=()):
    ctx = cvr.Context(0, kernel)
    ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
    for k, v in opts:
        ctx.set_option(k, v)
    desc, keep = cvr.medium_from_arrays(d, a, scale=SCALE, max_density=md)
    ctx.set_medium(desc)
    iv, r2v = cvr.default_camera(*res)
    ctx.set_camera(iv, r2v, res)
    ctx.init()
    return ctx, iv, r2v


def dense_oracle(cvr, oracle_mod, d, a, md):
    """The fp32 oracle of the rounded medium with the effective majorant."""
    return oracle_mod.Oracle(cvr.half_round(d), cvr.half_round(a), scale=SCALE, max_density=md_eff(cvr, md))


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
    assert (c["flags"] & 1).any() and (c["flags"] == 0).any(), what  # escapes and roulette deaths
    assert (c["n_albedo"] > 0).any(), what                            # real collisions: the albedo is read


def check_launch(ctx, orc, iv, r2v, kid, what, tile=TILE, iters=ITERS, seed=3):
    """Records of the production launch, its counters and pixels, and cvr_trace_paths."""
    n = tile[0] * tile[1] * iters
    L = orc.launch(iv, r2v, tile, tile, (0, 0), kid, seed)
    c = orc.trace_paths(L, 0, n)
    ctx.set_resolution(*tile)
    ctx.set_offset(0, 0)
    ctx.set_iterations(iters)
    ctx.set_seed(seed)
    ctx.set_path_range(0, n)
    compare_records(ctx.trace_launch(n), c, what + ": trace_launch")
    compare_records(ctx.trace_paths(0, n), c, what + ": trace_paths", counts=True)
    acc, st = gpu_range_render(ctx, tile, (0, 0), iters, seed, 0, n)
    ref, rst = orc.render(L, 0, n, nthreads=NTHREADS)
    assert_counters_equal(st, rst, what)
    assert_pixels_close(acc[..., :3], ref[..., :3], iters, what)
    return c


# ------------------------------------------------------------------- tests --
@pytest.mark.parametrize("kernel", ["regenerationSK", "sortingSK"])
@pytest.mark.parametrize("md_case", ["max", "up", "down"])
def test_dense_records_and_counters(cvr, oracle_mod, kernel, md_case):
    d, a, md = dense_arrays(md_case)
    ctx, iv, r2v = dense_ctx(cvr, d, a, md, kernel)
    info = ctx.medium_info()
    assert info.format == cvr.FORMAT_F16 and info.max_density_eff == np.float32(md_eff(cvr, md))
    if md_case == "up":
        assert info.max_density_eff > np.float32(md)
    if md_case == "down":
        assert info.max_density_eff == np.float32(md)
    orc = dense_oracle(cvr, oracle_mod, d, a, md)
    check_launch(ctx, orc, iv, r2v, cvr.KERNELS.index(kernel), f"dense {kernel} {md_case}")
    ctx.close()


def test_dense_without_cells(cvr, oracle_mod):
    """CVR_OPT_CELLS 0: every evaluation is the 8-tap gather of the half grid (the generic instance)."""
    d, a, md = dense_arrays("max")
    ctx, iv, r2v = dense_ctx(cvr, d, a, md, opts=((cvr.OPT_CELLS, 0),))
    assert ctx.medium_info().cells_bytes == 0
    check_launch(ctx, dense_oracle(cvr, oracle_mod, d, a, md), iv, r2v, 2, "dense, no cells")
    ctx.close()


@pytest.mark.parametrize("kernel", ["regenerationSK", "sortingSK"])
def test_dense_uniform_albedo(cvr, oracle_mod, kernel):
    d, a, md = dense_arrays("max", uniform=True)
    r = cvr.half_round(np.array([0.9], np.float32))[0]
    assert r == np.float32(0.89990234375) and r != np.float32(0.9)  # a kernel that kept 0.9 fails below
    ctx, iv, r2v = dense_ctx(cvr, d, a, md, kernel)
    check_launch(ctx, dense_oracle(cvr, oracle_mod, d, a, md), iv, r2v, cvr.KERNELS.index(kernel),
                 f"uniform {kernel}")
    ctx.close()


@pytest.mark.parametrize("emask", [1, 0])
@pytest.mark.parametrize("with_albedo", [True, False])
def test_sparse_records_and_counters(cvr, oracle_mod, with_albedo, emask):
    res, table, dens, alb, bg, md = sparse_arrays(with_albedo)
    # a whole super-brick without a cell leaf (none of its 8 forward leaves exists)
    present = table != 0xFFFFFFFF
    pad = np.zeros(tuple(s + 1 for s in present.shape), bool)
    pad[:-1, :-1, :-1] = present
    has_cells = np.zeros_like(present)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                has_cells |= pad[dz:dz + present.shape[0], dy:dy + present.shape[1], dx:dx + present.shape[2]]
    assert (~has_cells).any() and 0.35 <= (~present).mean() <= 0.65
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_option(cvr.OPT_MEDIUM_FORMAT, cvr.FORMAT_F16)
    ctx.set_option(cvr.OPT_EMPTY_MASK, emask)
    desc, keep = sparse_desc(cvr, res, table, dens, alb, bg, md)
    ctx.set_medium_sparse(desc)
    tile = (32, 32)
    iv, r2v = cvr.default_camera(*tile)
    ctx.set_camera(iv, r2v, tile)
    ctx.init()
    orc = oracle_mod.Oracle.from_leaves(res, table, cvr.half_round(dens),
                                        None if alb is None else cvr.half_round(alb),
                                        tuple(float(v) for v in cvr.half_round(np.array(bg, np.float32))),
                                        scale=SCALE,
                                        max_density=md_eff(cvr, md))
    check_launch(ctx, orc, iv, r2v, 2, f"sparse albedo={with_albedo} emask={emask}", tile=tile, iters=2)
    ctx.close()


def test_pixels_frame_tiles_shards(cvr, oracle_mod):
    d, a, md = dense_arrays("max")
    W = H = 64
    iters = 2
    ctx, iv, r2v = dense_ctx(cvr, d, a, md, res=(W, H))
    orc = dense_oracle(cvr, oracle_mod, d, a, md)
    ref, rst = oracle_image(orc, iv, r2v, W, H, (1, 1), iters, 2)
    pin = cvr.PinnedImage(W, H)
    try:
        # cvr_render_frame: the in-launch output instance stores the blocks
        ctx.set_resolution(W, H)
        ctx.set_iterations(iters)
        ctx.set_seed(0)
        pin.array[:] = np.nan
        _, st = ctx.render_frame(pin, 1)
        assert ctx.frame_flush_info() == ((W // 8) * (H // 8), 0)
        assert_counters_equal(st, rst, "render_frame")
        assert_pixels_close(pin.array[..., :3].copy(), ref[..., :3], iters, "render_frame")
        # 2x2 tiles
        ctx.set_seed(0)
        img, st = ctx.render_image(W, H, (2, 2), iters)
        tref, trst = oracle_image(orc, iv, r2v, W, H, (2, 2), iters, 2)
        assert_counters_equal(st, trst, "2x2 tiles")
        assert_pixels_close(img[..., :3], tref[..., :3], iters, "2x2 tiles")
        # the sum of 2 block shards (pixel-disjoint), through cvr_render_share_to_host
        pin.array[:] = np.nan
        total = dict.fromkeys(COUNTERS, 0)
        for k in range(2):
            ctx.set_block_shard(k, 2)
            ctx.set_seed(0)
            s = ctx.render_share_to_host(pin.ptr.value, pin.floats, W, H, (1, 1), iters)
            for key in COUNTERS:
                total[key] += getattr(s, key)
        ctx.set_block_shard(0, 1)
        assert total == {k: rst[k] for k in COUNTERS}
        assert_pixels_close(pin.array[..., :3].copy(), ref[..., :3], iters, "2 block shards")
    finally:
        pin.close()
        ctx.close()


@pytest.mark.parametrize("kernel", ["naiveMK", "naiveSK"])
def test_naive_kernels(cvr, oracle_mod, kernel):
    d, a, md = dense_arrays("max")
    W = H = 64
    iters = 2
    ctx, iv, r2v = dense_ctx(cvr, d, a, md, kernel, res=(W, H))
    img, st = ctx.render_image(W, H, (1, 1), iters)
    ref, rst = oracle_image(dense_oracle(cvr, oracle_mod, d, a, md), iv, r2v, W, H, (1, 1), iters,
                            cvr.KERNELS.index(kernel))
    assert_counters_equal(st, rst, kernel)
    assert_pixels_close(img[..., :3], ref[..., :3], iters, kernel)
    ctx.close()


def _records(ctx, n, seed=3):
    ctx.set_resolution(*TILE)
    ctx.set_offset(0, 0)
    ctx.set_iterations(ITERS)
    ctx.set_seed(seed)
    ctx.set_path_range(0, n)
    return ctx.trace_launch(n)


def test_option_takes_effect_and_switches_back(cvr, oracle_mod):
    d, a, md = dense_arrays("max")
    n = TILE[0] * TILE[1] * ITERS
    iv, r2v = cvr.default_camera(*TILE)
    L = oracle_mod.Oracle.launch(iv, r2v, TILE, TILE, (0, 0), 2, 3)
    o_round = dense_oracle(cvr, oracle_mod, d, a, md).trace_paths(L, 0, n)
    o_plain = oracle_mod.Oracle(d, a, scale=SCALE, max_density=md).trace_paths(L, 0, n)
    differ = (o_round["T"].view(np.uint32) != o_plain["T"].view(np.uint32)).any(axis=1)
    assert differ.any(), "the seed does not tell the rounded medium from the unrounded one"

    ctx, _, _ = dense_ctx(cvr, d, a, md, fmt=1)
    g1 = _records(ctx, n)
    compare_records(g1, o_round, "format 1")
    ref0, _, _ = dense_ctx(cvr, d, a, md, fmt=0)
    g0 = _records(ref0, n)
    compare_records(g0, o_plain, "format 0")
    assert (g1["T"].view(np.uint32) != g0["T"].view(np.uint32)).any(), "format 1 rendered the unrounded grid"
    # back to format 0 on the same context: the option applies at the next set_medium
    ctx.set_option(cvr.OPT_MEDIUM_FORMAT, cvr.FORMAT_F32)
    assert ctx.medium_info().format == cvr.FORMAT_F16
    desc, keep = cvr.medium_from_arrays(d, a, scale=SCALE, max_density=md)
    ctx.set_medium(desc)
    assert ctx.medium_info().format == cvr.FORMAT_F32
    back = _records(ctx, n)
    assert back.tobytes() == g0.tobytes()
    ctx.close()
    ref0.close()


def test_medium_info_bytes_and_shared_medium(cvr, oracle_mod):
    d, a, md = dense_arrays("max")
    n = d.size
    infos = {}
    for fmt in (0, 1):
        ctx, _, _ = dense_ctx(cvr, d, a, md, fmt=fmt)
        infos[fmt] = ctx.medium_info().as_dict()
        ctx.close()
    assert infos[0]["density_bytes"] == 4 * n and infos[0]["cells_bytes"] == 32 * n and infos[0]["albedo_bytes"] == 16 * n
    for k in ("density_bytes", "cells_bytes", "albedo_bytes"):
        assert 2 * infos[1][k] == infos[0][k], k
    assert infos[1]["bounds_bytes"] == infos[0]["bounds_bytes"] > 0
    for i in infos.values():
        assert i["total_bytes"] == i["density_bytes"] + i["cells_bytes"] + i["albedo_bytes"] + i["bounds_bytes"]

    res, table, dens, alb, bg, smd = sparse_arrays(True)
    sinfo = {}
    for fmt in (0, 1):
        ctx = cvr.Context(0, "regenerationSK")
        ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
        desc, keep = sparse_desc(cvr, res, table, dens, alb, bg, smd)
        ctx.set_medium_sparse(desc)
        sinfo[fmt] = ctx.medium_info().as_dict()
        ctx.close()
    assert sinfo[0]["density_bytes"] == 4 * dens.size and sinfo[0]["albedo_bytes"] == 16 * dens.size
    assert sinfo[0]["cells_bytes"] % (512 * 32) == 0 and sinfo[0]["cells_bytes"] > 0
    for k in ("density_bytes", "cells_bytes", "albedo_bytes"):
        assert 2 * sinfo[1][k] == sinfo[0][k], k
    assert sinfo[1]["bounds_bytes"] == sinfo[0]["bounds_bytes"] > 0

    # no medium: CVR_ERR_STATE; a shared medium reports and renders the source's format
    empty = cvr.Context(0, "regenerationSK")
    with pytest.raises(cvr.CvrError) as e:
        empty.medium_info()
    assert e.value.code == -3
    src, iv, r2v = dense_ctx(cvr, d, a, md, fmt=1)
    empty.set_option(cvr.OPT_MEDIUM_FORMAT, cvr.FORMAT_F32)
    empty.share_medium(src)
    assert empty.medium_info().as_dict() == src.medium_info().as_dict()
    empty.set_camera(iv, r2v, TILE)
    empty.init()
    count = TILE[0] * TILE[1] * ITERS
    L = oracle_mod.Oracle.launch(iv, r2v, TILE, TILE, (0, 0), 2, 3)
    compare_records(_records(empty, count), dense_oracle(cvr, oracle_mod, d, a, md).trace_paths(L, 0, count),
                    "shared medium")
    empty.close()
    src.close()


def _launch_code(ctx):
    ctx.set_resolution(*TILE)
    ctx.set_iterations(1)
    ctx.set_path_range(0, TILE[0] * TILE[1])
    with pytest.raises(Exception) as e:
        ctx.launch_render()
    return e.value.code


def test_refusals(cvr):
    d, a, md = dense_arrays("max")
    iv, r2v = cvr.default_camera(*TILE)
    # a finite value that rounds to inf: CVR_ERR_INVALID naming it, and no medium afterwards
    ctx, _, _ = dense_ctx(cvr, d, a, md)
    bad = d.copy()
    bad[2, 3, 4] = 70000.0
    desc, keep = cvr.medium_from_arrays(bad, a, scale=SCALE, max_density=md)
    with pytest.raises(cvr.CvrError) as e:
        ctx.set_medium(desc)
    assert e.value.code == -1 and "70000" in str(e.value)
    assert _launch_code(ctx) == -3
    bada = a.copy()
    bada[1, 1, 1, 2] = -65520.0
    desc, keep = cvr.medium_from_arrays(d, bada, scale=SCALE, max_density=md)
    with pytest.raises(cvr.CvrError) as e:
        ctx.set_medium(desc)
    assert e.value.code == -1 and "albedo" in str(e.value)
    # inf itself passes, as format 0 passes it
    infd = d.copy()
    infd[0, 0, 0] = np.inf
    desc, keep = cvr.medium_from_arrays(infd, a, scale=SCALE, max_density=md)
    ctx.set_medium(desc)
    with pytest.raises(cvr.CvrError) as e:
        ctx.set_option(cvr.OPT_MEDIUM_FORMAT, 2)
    assert e.value.code == -1
    ctx.close()
    # the combinations format 1 does not run: CVR_ERR_UNSUPPORTED from the launch
    for kernel, opt, val in (("regenerationSK", cvr.OPT_COUNT_WORDS, 1), ("regenerationSK", cvr.OPT_SCHEDULER, 0),
                             ("regenerationSK", cvr.OPT_SCHEDULER, 1), ("regenerationSK", cvr.OPT_SCHEDULER, 2),
                             ("naiveSK", cvr.OPT_SCHEDULER, 4), ("regenerationSK", cvr.OPT_RNG_BINDING, 1),
                             ("regenerationSK", cvr.OPT_WAVES, 4), ("naiveMK", cvr.OPT_MK_COMPACTION, 1)):
        ctx, _, _ = dense_ctx(cvr, d, a, md, kernel, opts=((opt, val),))
        assert _launch_code(ctx) == -5, (kernel, opt, val)
        ctx.close()


def test_cli_medium_format_half(cvr, tmp_path):
    """`cvr --medium-format half`: the summary names the format and the halved bytes, and the
    image is the library's format-1 render of the same scene."""
    import os
    import re
    import subprocess
    from test_cli_devices import CLI, read_pfm
    W = H = 64
    iters = 2
    outs = {}
    for fmt in ("float", "half"):
        out = str(tmp_path / fmt)
        r = subprocess.run([CLI, "--interactive", "0", "--synthetic", "bucky", "-r", str(W), str(H), "-i", str(iters),
                            "--medium-format", fmt, "--pfm", "-o", out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.search(r"medium on device\s*: (\w+), (\d+) bytes \(density (\d+), cells (\d+), albedo (\d+), bounds (\d+)\)",
                      r.stdout)
        assert m and m.group(1) == fmt, r.stdout
        outs[fmt] = ([int(v) for v in m.groups()[1:]], read_pfm(out + ".pfm"))
    (tf, df, cf, af, bf), _ = outs["float"]
    (th, dh, ch, ah, bh), img = outs["half"]
    assert (2 * dh, 2 * ch, 2 * ah, bh) == (df, cf, af, bf) and th == dh + ch + ah + bh
    scene = cvr.Scene.synthetic("bucky")
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_option(cvr.OPT_MEDIUM_FORMAT, cvr.FORMAT_F16)
    ctx.set_medium(scene.medium)
    iv, r2v = cvr.default_camera(W, H)
    ctx.set_camera(iv, r2v, (W, H))
    ctx.init()
    ref, _ = ctx.render_image(W, H, (1, 1), iters)
    ctx.close()
    assert_pixels_close(img, ref[..., :3], iters, "cli half")
    assert os.path.getsize(str(tmp_path / "half") + ".pfm") > 0
