"""Crop box and clip planes of the device builds (cvr_set_clip) against cvr_set_medium_device on
clipped arrays.

Each case builds two contexts.  A sets the clip and calls the device build under test on the
unclipped source (two arrays, a scalar field, or a scalar field with a 2-D table).  B sets no clip
and calls set_medium_device on the arrays that tests/clip_ref.py (the numpy restatement of the
statement, checked on the CPU in tests/test_clip_cpu.py) makes of the source's arrays, which for
the classified sources are cvr_classify_host's / cvr_classify_gradient_host's output.  The two must
be in one state: cvr_medium_info, cvr_medium_layout, every stored array byte for byte
(cvr_debug_copy_medium), the 4096 records of the production launch and its counters; A's records
are also compared with the oracle over the dense clipped arrays, and A's count of kept voxels
with the mask's.  B runs kernels that a context without a clip runs, so A's clipped instances are
judged against the unclipped ones."""
from functools import lru_cache

import numpy as np
import pytest
import torch  # (imported before libcvr is loaded, as tests/test_gpu_denoise.py does)

import build_scale as bs
import clip_ref as cr
import devmed
import gradient_ref as gr
import media
import transfer_ref as tr
from parity_util import assert_pixels_close
from test_cli_devices import run_cli
from test_gpu_build_scale import offset_tensor
from test_gpu_device_medium import (DEV, INVALID, STATE, UNSUPPORTED, assert_same_state, new_ctx, ready, records,
                                    refusal, tensors)

pytestmark = pytest.mark.gpu

NX, NY, NZ = cr.RES
SHAPE = (NZ, NY, NX)
CONST = (0.9, 0.55, 0.3, 0.75)
SOURCES = ("arrays", "const_albedo", "scalar_u8_offset", "scalar_f32", "gradient_u16", "gradient_f32")


# ----------------------------------------------------------------- sources --
@lru_cache(maxsize=None)
def field(dtype):
    """A smooth ramp under noise, so that the classification and the gradient both vary."""
    rng = np.random.default_rng(223)
    z, y, x = np.meshgrid(*(np.arange(v) for v in SHAPE), indexing="ij", sparse=True)
    if dtype == "float32":
        s = (0.9 * np.sin(0.21 * x + 0.13 * y) * np.cos(0.17 * z) + 0.1 * rng.random(SHAPE)).astype(np.float32)
        s[0, 0, 0] = np.float32(-0.2)
        return s
    top = np.iinfo(dtype).max
    s = ((x * 37 + y * 101 + z * 53) * (top // 255) % (top + 1)).astype(dtype)
    noisy = rng.random(SHAPE) < 0.3
    s[noisy] = rng.integers(0, top + 1, int(noisy.sum())).astype(dtype)
    return s


@lru_cache(maxsize=None)
def source(name):
    """(kind, case or arrays) of a source; the classified ones as tr.Case / gr.Case."""
    if name in ("arrays", "const_albedo"):
        d, a = cr.arrays()
        if name == "const_albedo":
            a = np.empty(SHAPE + (4,), np.float32)
            a[:] = np.array(CONST, np.float32)
        return d, a
    if name.startswith("scalar"):
        s = field("uint8" if "u8" in name else "float32")
        lo, hi = (20.0, 230.0) if s.dtype == np.uint8 else (-0.5, 0.7)
        return tr.Case(s, tr.table7(), lo, hi, False, False, *tr.UNIT, media.SCALE, False)
    s = field("uint16" if "u16" in name else "float32")
    lo, hi, ghi = (1000.0, 60000.0, 30000.0) if s.dtype == np.uint16 else (-0.5, 0.7, 0.4)
    return gr.Case(s, gr.table2d(), lo, hi, 0.0, ghi, (1.0, 0.5, 2.0), *tr.UNIT, media.SCALE, False)


@lru_cache(maxsize=None)
def unclipped(cvr, name):
    """(density, albedo) of the source before the clip: the arrays, or the host statement's output."""
    c = source(name)
    if isinstance(c, tuple) and not hasattr(c, "scalar"):
        return c
    if isinstance(c, gr.Case):
        return cvr.classify_gradient_host(c.scalar, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)[:2]
    return cvr.classify_host(c.scalar, c.table, c.lo, c.hi, ceil=c.ceil, density_u=c.density_u)


@lru_cache(maxsize=None)
def clipped(cvr, name, region_name):
    """(keep, density, albedo) by tests/clip_ref.py; read-only, shared by the cases."""
    d, a = unclipped(cvr, name)
    keep, dc, ac = cr.clip(d, a, cr.GPU_REGIONS[region_name])
    for v in (keep, dc, ac):
        v.setflags(write=False)
    return keep, dc, ac


@lru_cache(maxsize=None)
def oracle_ref(cvr, name, region_name, fmt):
    _, d, a = clipped(cvr, name, region_name)
    return devmed.oracle_records(d, a, float(d.max()), fmt)


def set_clip(ctx, region):
    ctx.set_clip(region.lo, region.hi, region.planes)


def build(cvr, ctx, name, sparse, arrays=None, max_density=None):
    """The device call of source `name` on ctx: on the source itself, or (arrays given: context B)
    set_medium_device on those arrays."""
    c = source(name)
    common = dict(sparse=sparse, scale=media.SCALE, max_density=max_density)
    if arrays is not None or not hasattr(c, "scalar"):
        d, a = arrays if arrays is not None else c
        if name == "const_albedo":
            td, = tensors(d)
            ctx.set_medium_device(td, None, const_albedo=CONST, **common)
        else:
            td, ta = tensors(d, a)
            ctx.set_medium_device(td, ta, **common)
        return ctx
    t = offset_tensor(c.scalar) if "offset" in name else torch.from_numpy(np.ascontiguousarray(c.scalar)).to(DEV)
    if isinstance(c, gr.Case):
        ctx.set_medium_gradient(t, c.table, lo=c.lo, hi=c.hi, glo=c.glo, ghi=c.ghi, spacing=c.spacing, **common)
    else:
        ctx.set_medium_scalar(t, c.table, lo=c.lo, hi=c.hi, **common)
    return ctx


def stored_arrays(cvr, ctx):
    return {k: ctx.debug_medium_array(k) for k in cvr.MEDIUM_ARRAYS}


def assert_same_arrays(cvr, b, a, what):
    """Every CVR_MEDIUM_* array of the two contexts, byte for byte."""
    hb, ha = stored_arrays(cvr, b), stored_arrays(cvr, a)
    for k in cvr.MEDIUM_ARRAYS:
        assert (ha[k] is None) == (hb[k] is None), f"{what}: array {k} exists in one context only"
        if ha[k] is None:
            continue
        assert ha[k].dtype == hb[k].dtype and ha[k].shape == hb[k].shape, f"{what}: array {k}"
        if ha[k].tobytes() != hb[k].tobytes():
            bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[ha[k].dtype.itemsize]
            mism = np.nonzero(ha[k].view(bits) != hb[k].view(bits))[0]
            raise AssertionError(f"{what}: {k}: {mism.size} of {ha[k].size} entries differ between the clipped build "
                                 f"and the build on clipped arrays, first at {mism[:4]}, last at {mism[-1]}")
    return ha


def assert_clip_info(ctx, region, keep, what):
    info, kept = ctx.medium_clip_info()
    assert kept == int(keep.sum()), f"{what}: {kept} kept voxels counted on the device, the mask holds {int(keep.sum())}"
    assert info["lo"] == tuple(region.lo or (0, 0, 0)) and info["hi"] == tuple(region.hi or (0xFFFFFFFF,) * 3), what
    assert info["planes"] == [tuple(np.float32(v) for v in p) for p in region.planes], what


def close(*ctxs):
    for c in ctxs:
        c.close()


def pair(cvr, name, region_name, sparse, fmt, ref=None):
    region = cr.GPU_REGIONS[region_name]
    keep, d, a = clipped(cvr, name, region_name)
    what = f"{name} {region_name} {'sparse' if sparse else 'dense'} format {fmt}"
    ctx_a = new_ctx(cvr, fmt)
    set_clip(ctx_a, region)
    ready(cvr, build(cvr, ctx_a, name, sparse))
    ctx_b = ready(cvr, build(cvr, new_ctx(cvr, fmt), name, sparse, arrays=(d, a)))
    lay = assert_same_state(ctx_b, ctx_a, what, ref)
    assert lay["sparse"] == int(sparse), what
    got = assert_same_arrays(cvr, ctx_b, ctx_a, what)
    assert_clip_info(ctx_a, region, keep, what)
    assert ctx_b.medium_clip_info()[1] == keep.size, what       # a medium built without a clip keeps every voxel
    return ctx_a, ctx_b, lay, got


# ------------------------------------------------------------------ matrix --
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("region_name", sorted(cr.GPU_REGIONS))
@pytest.mark.parametrize("name", SOURCES)
def test_clipped_build_equals_the_build_on_clipped_arrays(cvr, oracle_mod, name, region_name, sparse, fmt):
    # (an all-clipped grid has a majorant of 0, which the oracle's free-flight sampling cannot take)
    ref = oracle_ref(cvr, name, region_name, fmt) if region_name != "all_clipped" else None
    a, b, lay, got = pair(cvr, name, region_name, sparse, fmt, ref)
    keep, d, _ = clipped(cvr, name, region_name)
    assert a.medium_info().max_density_eff == b.medium_info().max_density_eff   # CVR_DEVMED_MAX_DENSITY, clipped values
    if region_name == "all_clipped":
        assert not keep.any() and a.medium_info().max_density_eff == 0.0
        if sparse:
            assert lay["n_leaves"] == 0
    else:
        assert 0 < keep.sum() < keep.size
    close(a, b)


def test_the_sources_are_what_the_matrix_says(cvr):
    """The u8 field starts one element into its allocation, and the classified sources vary."""
    t = offset_tensor(source("scalar_u8_offset").scalar)
    assert t.data_ptr() % 16 == 1
    for name in SOURCES[2:]:
        d, a = unclipped(cvr, name)
        assert len(np.unique(d)) > 16 and len(np.unique(a[..., 0])) > 16, name


# ---------------------------------------------------------------- gradient --
@pytest.mark.parametrize("name", ["gradient_u16", "gradient_f32"])
def test_a_kept_voxel_beside_the_cut_keeps_the_uncut_fields_gradient(cvr, name):
    """The stencil of a kept voxel reads its clipped neighbours from the field: the stored density
    beside the cut is the unclipped build's, not that of a field with a hole."""
    region = cr.GPU_REGIONS["crop_slab"]
    keep = clipped(cvr, name, "crop_slab")[0]
    a = new_ctx(cvr)
    set_clip(a, region)
    build(cvr, a, name, False)
    u = build(cvr, new_ctx(cvr), name, False)
    da, du = (c.debug_medium_array("density").reshape(SHAPE) for c in (a, u))
    cut = np.zeros(SHAPE, bool)                       # kept voxels with a clipped 6-neighbour
    for axis in range(3):
        for shift in (1, -1):
            nb = np.roll(keep, shift, axis)
            edge = [slice(None)] * 3
            edge[axis] = 0 if shift == 1 else -1
            nb[tuple(edge)] = True                    # (no neighbour past the grid)
            cut |= keep & ~nb
    assert cut.sum() > 100, "no kept voxel lies beside the cut"
    assert da[cut].tobytes() == du[cut].tobytes()
    assert da[keep].tobytes() == du[keep].tobytes() and not da[~keep].view(np.uint32).any()
    # the case tells the two apart: classifying the cut field instead gives other densities there
    c = source(name)
    holed = c.scalar.copy()
    holed[~keep] = 0
    dh = cvr.classify_gradient_host(holed, c.table, c.lo, c.hi, c.glo, c.ghi, c.spacing)[0]
    assert (dh[cut] != du[cut]).any()
    close(a, u)


# ------------------------------------------------------------------ leaves --
@pytest.mark.parametrize("fmt", [0, 1])
def test_a_crop_sheds_the_leaves_it_empties(cvr, fmt):
    region = cr.GPU_REGIONS["crop"]
    keep, d, a = clipped(cvr, "arrays", "crop")
    ctx = new_ctx(cvr, fmt)
    set_clip(ctx, region)
    build(cvr, ctx, "arrays", True)
    full = build(cvr, new_ctx(cvr, fmt), "arrays", True)
    sp = devmed.leaf_rule(d, a)
    n = int((sp.table != devmed.NO_LEAF).sum())
    assert ctx.medium_layout().n_leaves == n < full.medium_layout().n_leaves
    table = ctx.debug_medium_array("leaf_table")
    assert np.array_equal(table != devmed.NO_LEAF, (sp.table != devmed.NO_LEAF).reshape(-1))
    assert np.array_equal(table, sp.table.reshape(-1))
    # the leaves outside the crop box are the ones that went: 3..29 x 9..16 x 2..20 in voxels
    lz, ly, lx = np.nonzero(sp.table != devmed.NO_LEAF)
    assert lx.min() == 0 and lx.max() == 3 and ly.min() == 1 and ly.max() == 2 and lz.min() == 0 and lz.max() == 2
    assert ctx.medium_info().total_bytes < full.medium_info().total_bytes
    close(ctx, full)


# ------------------------------------------------------------ second trips --
def scaled_region(shape):
    """The crop-plus-slab clip over a (z, y, x) grid of any size: a crop off the leaf grid with hi
    past the grid in z, and a slab of two oblique planes that keeps about half of it."""
    nz, ny, nx = shape
    s = float(nx + ny)
    return cr.Region((3, 9, 2), (nx - 7, ny - 12, nz + 19), ((1.0, 1.0, 0.25, -0.3 * s), (-1.0, -1.0, -0.25, 0.8 * s + 0.5)))


@lru_cache(maxsize=2)
def big_case(cvr, name):
    """(unclipped density and albedo, region, keep, clipped density and albedo) of a tests/build_scale.py medium."""
    if name == "dense_2m":
        d, a = bs.dense_base()[:2]
    elif name == "sparse_4m":
        d, a = bs.sparse_arrays()[:2]
    else:
        d, a = bs.host_classified(cvr, name)
    region = scaled_region(d.shape)
    keep, dc, ac = cr.clip(d, a, region)
    return region, keep, dc, ac


def big_build(cvr, ctx, name, sparse, arrays=None):
    if arrays is not None or name in ("dense_2m", "sparse_4m"):
        d, a = arrays if arrays is not None else (bs.dense_base()[:2] if name == "dense_2m" else bs.sparse_arrays()[:2])
        td, ta = tensors(d, a)
        ctx.set_medium_device(td, ta, sparse=sparse, scale=media.SCALE, max_density=None)
        return ctx
    c = bs.case(name)
    t = offset_tensor(c.scalar) if name in bs.HEAD else torch.from_numpy(np.ascontiguousarray(c.scalar)).to(DEV)
    common = dict(lo=c.lo, hi=c.hi, sparse=sparse, box_min=c.box_min, box_max=c.box_max, scale=c.scale, max_density=None)
    if bs.is_gradient(name):
        ctx.set_medium_gradient(t, c.table, glo=c.glo, ghi=c.ghi, spacing=c.spacing, **common)
    else:
        ctx.set_medium_scalar(t, c.table, ceil=c.ceil, density_u=c.density_u, **common)
    return ctx


@pytest.mark.parametrize("name,sparse,fmt", [("dense_2m", False, 0), ("dense_2m", False, 1), ("scalar_u8_8m", False, 1),
                                             ("gradient_u16_4m", False, 0), ("sparse_4m", True, 0),
                                             ("sparse_4m", True, 1)])
def test_second_trips_of_the_clipped_instances(cvr, name, sparse, fmt):
    """tests/build_scale.py's media, each the smallest that makes one build kernel loop over its
    capped grid: the clipped instances carry the same loops (the 2.1 M-voxel arrays: k_arrays_clip;
    scalar_u8_8m one element into its allocation: k_classified_clip's 16-byte body;
    gradient_u16_4m: k_gradient_clip; sparse_4m: k_leaf_flags and k_gather_leaves with xc = 1)."""
    region, keep, dc, ac = big_case(cvr, name)
    what = f"{name} format {fmt}"
    a = new_ctx(cvr, fmt)
    set_clip(a, region)
    ready(cvr, big_build(cvr, a, name, sparse))
    b = ready(cvr, big_build(cvr, new_ctx(cvr, fmt), name, sparse, arrays=(dc, ac)))
    assert_same_state(b, a, what)
    assert_same_arrays(cvr, b, a, what)
    assert_clip_info(a, region, keep, what)
    assert 0.05 < keep.mean() < 0.95
    close(a, b)


# ---------------------------------------------------------------- overflow --
def overflow_field():
    """cr.arrays' density with two values that round to infinity in binary16, both outside the crop."""
    d, a = (v.copy() for v in cr.arrays())
    d[1, 3, 5] = np.float32(70000.0)     # z = 1 < lo[2]: clipped by the crop
    d[10, 20, 8] = np.float32(-1e6)      # y = 20 >= hi[1]
    return d, a


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_format_1_overflow_is_judged_on_the_clipped_values(cvr, sparse):
    region = cr.GPU_REGIONS["crop"]
    d, a = overflow_field()
    keep, dc, ac = cr.clip(d, a, region)
    assert not keep[1, 3, 5] and not keep[10, 20, 8] and np.isfinite(cvr.half_round(dc)).all()
    ctx = new_ctx(cvr, 1)
    set_clip(ctx, region)
    ready(cvr, build(cvr, ctx, "arrays", sparse, arrays=(d, a)))          # builds: the overflowing voxels are clipped
    ref = ready(cvr, build(cvr, new_ctx(cvr, 1), "arrays", sparse, arrays=(dc, ac)))
    assert_same_state(ref, ctx, "overflow clipped away")
    assert_same_arrays(cvr, ref, ctx, "overflow clipped away")
    # one of them kept: the refusal of the host call on the clipped arrays, code, message and index
    d[10, 12, 8] = np.float32(-1e6)
    keep, dc, ac = cr.clip(d, a, region)
    assert keep[10, 12, 8]
    host = new_ctx(cvr, 1)
    if sparse:
        sp = devmed.leaf_rule(dc, ac)
        desc, alive = media.sparse_desc(cvr, sp.res, sp.table, sp.leaf_density, sp.leaf_albedo, sp.albedo_bg, 1.0)
        want = refusal(cvr, lambda: host.set_medium_sparse(desc))
    else:
        desc, alive = cvr.medium_from_arrays(dc, ac, (-0.5,) * 3, (0.5,) * 3, media.SCALE, 1.0)
        want = refusal(cvr, lambda: host.set_medium(desc))
    got = refusal(cvr, lambda: build(cvr, ctx, "arrays", sparse, arrays=(d, a), max_density=1.0))
    assert got == want and got[0] == INVALID and "value -1e+06 at index" in got[1], (got, want)
    if not sparse:
        assert f"at index {(10 * NY + 12) * NX + 8} " in got[1]
    close(ctx, ref, host)


# ------------------------------------------------------------------- state --
def test_set_clip_refusals_and_round_trip(cvr):
    ctx = new_ctx(cvr)
    assert ctx.clip is None
    region = cr.GPU_REGIONS["crop_slab"]
    set_clip(ctx, region)
    got = ctx.clip
    assert got["lo"] == region.lo and got["hi"] == region.hi
    assert got["planes"] == [tuple(np.float32(v) for v in p) for p in region.planes]
    for bad, words in ((dict(planes=[(1, 0, 0, 0)] * 9), "clip planes"), (dict(lo=(5, 0, 0), hi=(4, 9, 9)), "crop lo"),
                       (dict(planes=[(1, 0, float("nan"), 0)]), "not finite"), (dict(planes=[(0, 0, 0, 1)]), "zero normal")):
        code, text = refusal(cvr, lambda: ctx.set_clip(**bad))
        assert code == INVALID and words in text, (bad, text)
    assert ctx.clip == got                                   # a refused call leaves the clip as it was
    import ctypes as C
    lib = cvr.load()
    assert lib.cvr_set_clip(ctx._h, None) == INVALID
    d = cvr.ClipDesc()
    d.hi[:] = (9, 9, 9)
    d.flags = 1
    assert lib.cvr_set_clip(ctx._h, C.byref(d)) == INVALID
    ctx.clear_clip()
    assert ctx.clip is None
    code, _ = refusal(cvr, ctx.medium_clip_info)
    assert code == STATE                                      # no medium
    ctx.close()


def test_clear_clip_restores_the_unclipped_build(cvr):
    d, a = unclipped(cvr, "arrays")
    plain = ready(cvr, build(cvr, new_ctx(cvr), "arrays", False))
    ctx = new_ctx(cvr)
    set_clip(ctx, cr.GPU_REGIONS["oblique"])
    ready(cvr, build(cvr, ctx, "arrays", False))
    assert records(ctx).tobytes() != records(plain).tobytes()
    # the clip is taken at the build: setting another one does not touch the medium in use
    before = records(ctx)
    set_clip(ctx, cr.GPU_REGIONS["crop"])
    assert records(ctx).tobytes() == before.tobytes() and ctx.medium_clip_info()[0]["lo"] == (0, 0, 0)
    ctx.clear_clip()
    build(cvr, ctx, "arrays", False)
    assert_same_state(plain, ctx, "after clear_clip")
    assert_same_arrays(cvr, plain, ctx, "after clear_clip")
    assert ctx.medium_clip_info() == ({"lo": (0, 0, 0), "hi": (0xFFFFFFFF,) * 3, "planes": []}, d.size)
    close(plain, ctx)


def test_host_uploads_refuse_while_a_clip_is_set_and_keep_the_medium(cvr):
    keep = clipped(cvr, "arrays", "crop")[0]
    ctx = new_ctx(cvr)
    set_clip(ctx, cr.GPU_REGIONS["crop"])
    ready(cvr, build(cvr, ctx, "arrays", False))
    before = records(ctx)
    m = media.random40()
    desc, alive = cvr.medium_from_arrays(m.density, m.albedo, m.box_min, m.box_max, m.scale, m.max_density)
    code, text = refusal(cvr, lambda: ctx.set_medium(desc))
    assert code == UNSUPPORTED and "clip" in text
    sp = media.sparse_small()
    sdesc, alive2 = media.sparse_desc(cvr, sp.res, sp.table, sp.leaf_density, sp.leaf_albedo, sp.albedo_bg, sp.max_density)
    code, text = refusal(cvr, lambda: ctx.set_medium_sparse(sdesc))
    assert code == UNSUPPORTED and "clip" in text
    assert records(ctx).tobytes() == before.tobytes()
    # a shared medium carries what the source built
    other = new_ctx(cvr)
    other.share_medium(ctx)
    assert other.medium_clip_info() == ctx.medium_clip_info() and other.medium_clip_info()[1] == int(keep.sum())
    assert records(ready(cvr, other)).tobytes() == before.tobytes()
    # without a clip the host upload is what it was
    ctx.clear_clip()
    ctx.set_medium(desc)
    assert ctx.medium_clip_info()[1] == m.density.size
    close(other, ctx)


def test_set_clip_is_refused_inside_an_adaptive_session(cvr):
    ctx = ready(cvr, build(cvr, new_ctx(cvr), "arrays", False))
    before = records(ctx)
    with ctx.adaptive(cvr.AdaptiveDesc(8, 16, 4, -1.0, 0.01)):
        code, text = refusal(cvr, lambda: set_clip(ctx, cr.GPU_REGIONS["crop"]))
        assert code == STATE and "adaptive session" in text and "cvr_set_clip" in text
        code, text = refusal(cvr, ctx.clear_clip)
        assert code == STATE and "cvr_clear_clip" in text
    assert ctx.clip is None and records(ctx).tobytes() == before.tobytes()
    ctx.close()


# --------------------------------------------------------------------- CLI --
def test_cli_crop_and_clip_plane(cvr, tmp_path):
    """cvr --synthetic bucky --transfer2d ... --crop ... --clip-plane ... writes the image of a Python
    session set up the same way (the comparison of test_cli_transfer2d)."""
    W, H, iters = 64, 64, 2
    table = gr.table2d()
    m, n = table.shape[:2]
    glo, ghi, spacing = 2.0, 90.0, (1.0, 2.0, 0.5)
    crop, plane = (2, 0, 3, 29, 32, 40), (0.5, 1.0, -0.25, -11.5)
    path = tmp_path / "tf2d.txt"
    path.write_text(f"# n m\n{n} {m}\n" + "".join("%.9g %.9g %.9g %.9g\n" % tuple(row) for row in table.reshape(-1, 4)))
    common = ("--synthetic", "bucky", "--transfer2d", str(path), "--gradient-range", str(glo), str(ghi), "--voxel-spacing",
              *(str(v) for v in spacing), "-r", str(W), str(H), "-i", str(iters))
    img, out = run_cli(tmp_path, "clip", *common, "--crop", *(str(v) for v in crop), "--clip-plane",
                       *(str(v) for v in plane), "--field-stats")
    uncut, _ = run_cli(tmp_path, "uncut", *common)
    scene = cvr.Scene.synthetic("bucky")
    raw = np.frombuffer(scene.raw_bytes, np.uint8).reshape(32, 32, 32)
    md = scene.medium
    iv, r2v = scene.camera(W, H)
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_clip(crop[:3], crop[3:], [plane])
    ctx.set_medium_gradient(torch.from_numpy(raw.copy()).to(DEV), table, lo=0.0, hi=float(raw.max()), glo=glo, ghi=ghi,
                            spacing=spacing, box_min=tuple(md.box_min), box_max=tuple(md.box_max), scale=md.scale,
                            g=md.g, roughness=tuple(md.roughness), eta=md.eta)
    ctx.set_camera(iv, r2v, (W, H))
    ctx.init()
    py, _ = ctx.render_image(W, H, (1, 1), iters)
    kept = ctx.medium_clip_info()[1]
    assert kept == int(cr.keep_mask((32, 32, 32), crop[:3], crop[3:], [plane]).sum()) and 0 < kept < raw.size
    scene.close()
    ctx.close()
    assert py[..., :3].max() > 0
    assert_pixels_close(img, py[..., :3], iters, "cvr --crop --clip-plane against set_clip + set_medium_gradient")
    assert img.tobytes() != uncut.tobytes()
    assert f"kept voxels {kept} of {raw.size}" in out, out
    assert out.count("kept voxels") == 1                     # from the render's own build, once
    # --iterations 0: the field's numbers alone, the medium built once for the count, no image
    import subprocess
    from test_cli_devices import CLI
    r = subprocess.run([CLI, "--interactive", "0", "-o", str(tmp_path / "none"), *common[:-2], "-i", "0", "--crop",
                        *(str(v) for v in crop), "--clip-plane", *(str(v) for v in plane), "--field-stats"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"kept voxels {kept} of {raw.size}" in r.stdout, r.stdout + r.stderr
    assert not (tmp_path / "none.pfm").exists()
