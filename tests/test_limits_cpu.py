"""The inputs of tests/test_gpu_limits.py are sharp, and the host pins of the index arithmetic (no GPU).

A case at a limit of the 24-bit multiplies proves something only if the walk really forms the large
products there: the oracle's evaluation log (Oracle.trace_evals) of every medium case is restated in
plain integer numpy (tests/limits.py) and must hold at least limits.MIN_SHARP in-grid evaluations
with a non-zero test value whose brick or cell index has a term that a narrower multiply would
change.  The whole trace of a case stays under limits.MAX_EVALS evaluations, so that the GPU tests
take seconds.

Host pins: fastdiv's constants and formula against integer division (cvr_debug_fastdiv, host form),
and the sign extension of seed + path id (Q3) that limits.SEED_SIGN takes in mid-launch."""
import ctypes as C

import numpy as np
import pytest

import limits
from test_oracle_cpu import curand_init_state


@pytest.fixture(scope="module")
def traces(oracle_mod):
    """name -> (case, records, evals), traced once."""
    cache = {}

    def get(name):
        if name not in cache:
            case = limits.MEDIA[name]()
            orc = limits.make_oracle(oracle_mod, case)
            recs, evals = orc.trace_evals(limits.make_launch(oracle_mod, case), 0, limits.N_PATHS)
            cache[name] = (case, recs, evals)
        return cache[name]

    return get


def _sharp(case, evals):
    ok, x1, y1, z1 = limits.in_grid(case, evals)
    return ok & (evals["test_value"] != 0), x1, y1, z1


@pytest.mark.parametrize("name", list(limits.MEDIA))
def test_trace_is_small(traces, name):
    case, recs, evals = traces(name)
    print(f"{name}: {len(evals)} evaluations, {(evals['test_value'] != 0).sum()} non-zero, "
          f"{(recs['n_density'] > 0).mean():.2f} of the paths evaluate, {(recs['flags'] & 1).mean():.2f} escape")
    assert len(evals) < limits.MAX_EVALS
    # every path walks the medium, and both outcomes occur
    assert (recs["n_density"] > 0).mean() > 0.75
    assert 0.1 < (recs["flags"] & 1).mean() < 0.9


@pytest.mark.parametrize("name", [k for k in limits.SPARSE if k.startswith("sparse_xy_limit")])
def test_sparse_brick_terms(traces, name):
    """by * bnx >= 2^23 (a 23-bit multiply would wrap) and bz * (bnx bny) >= 2^24 - 4096 (the
    precomputed product just below the guard's 2^24)."""
    case, _, evals = traces(name)
    nz, x1, y1, z1 = _sharp(case, evals)
    zt, yt = limits.brick_terms(case, x1, y1, z1)
    rx, ry, _ = limits.res_of(case)
    s = limits.brick_shift(case)
    bnx, bny = rx >> s, ry >> s
    # one more column of leaves (8 >> s bricks) would reach 2^24
    assert bnx * bny < (1 << 24) <= (bnx + (8 >> s)) * bny and bny & (bny - 1) == 0
    assert (nz & (yt >= 1 << 23)).sum() >= limits.MIN_SHARP
    assert (nz & (zt >= (1 << 24) - 4096)).sum() >= limits.MIN_SHARP
    # the leaf-table index (texel_density: ((z >> 3) lny + (y >> 3)) lnx + (x >> 3)) reaches its end
    lz, ly, lx = case.medium.table.shape
    li = ((z1 >> 3) * ly + (y1 >> 3)) * lx + (x1 >> 3)
    assert (nz & (li >= lz * ly * lx - 64 * lx)).sum() >= limits.MIN_SHARP


@pytest.mark.parametrize("name,term", [("dense_xy_limit", 1), ("dense_yz_limit", 0)])
def test_dense_cell_terms(traces, name, term):
    """y1 * rx (x/y case) or z1 * (rx ry) (y/z case) >= 2^23 in the cell index, with the guarded
    product rx ry or ry rz = 2^24 - 4096; the 8-tap gather (cells off) reads up to the last voxel."""
    case, _, evals = traces(name)
    nz, x1, y1, z1 = _sharp(case, evals)
    rx, ry, rz = limits.res_of(case)
    assert (rx * ry if term else ry * rz) == (1 << 24) - 4096
    t = limits.cell_terms(case, x1, y1, z1)[term]
    assert (nz & (t >= 1 << 23)).sum() >= limits.MIN_SHARP
    last = ((z1 + 1) * ry + (y1 + 1)) * rx + x1 + 1   # the gather's far tap
    assert (nz & (last >= rx * ry * rz - 64 * rx * (1 if term else ry))).sum() >= limits.MIN_SHARP
    if term:  # both z layers weigh in: 0 < fz
        assert (nz & (evals["cz"] > 0) & (evals["cz"] < 1)).sum() >= limits.MIN_SHARP


def test_long_x_exceeds_2_24(traces):
    case, _, evals = traces("sparse_long_x")
    nz, x1, _, _ = _sharp(case, evals)
    assert limits.res_of(case)[0] > 1 << 24
    assert (nz & (evals["cx"] >= np.float32(1 << 24))).sum() >= limits.MIN_SHARP
    # coordinates there have no fraction bits, and odd cells cannot be addressed at all
    assert (np.modf(evals["cx"][nz & (x1 >= 1 << 24)])[0] == 0).all()


def test_long_z_multiplicands(traces):
    """The z multiplicands of the brick-word and leaf indices need all 24 bits."""
    case, _, evals = traces("sparse_long_z")
    nz, _, _, z1 = _sharp(case, evals)
    assert limits.res_of(case)[2] == 1 << 27 and limits.brick_shift(case) == 3
    assert (nz & ((z1 >> 3) >= 1 << 23)).sum() >= limits.MIN_SHARP
    assert (z1 >> 3).max() >= (1 << 24) - 64


@pytest.mark.parametrize("name,shape", [("sparse_thin_mask", (8, 11, 0, 0)), ("sparse_xy_limit", (10, 5, 5, 0)),
                                        ("sparse_long_x", (14, 11, 0, 0)), ("sparse_long_z", (16, 0, 0, 11))])
def test_mask_values_visited(traces, name, shape):
    """The empty-region mask of an extreme-aspect leaf table: axes without mask bits, and evaluations
    in super-bricks of both mask values."""
    case, _, evals = traces(name)
    es, lx, ly, lz, bits = limits.emask_model(case)
    assert (es, lx, ly, lz) == shape
    ok, x1, y1, z1 = limits.in_grid(case, evals)
    sb = limits.super_brick(case, x1, y1, z1)[ok]
    assert sb.max() < limits.EMASK_BITS
    is_set = np.isin(sb, sorted(bits))
    assert is_set.sum() >= limits.MIN_SHARP and (~is_set).sum() >= limits.MIN_SHARP
    # a clear super-brick holds no density
    assert (evals["test_value"][ok][~is_set] == 0).all()


def test_media_are_half_exact(cvr, traces):
    """Format 1 renders these media unchanged (densities k / 1024, albedo of few bits), so one oracle
    serves both formats."""
    for name in limits.DENSE + ["sparse_xy_limit"]:
        m = traces(name)[0].medium
        d = m.density if name in limits.DENSE else m.leaf_density
        block = d[d != 0]
        assert (cvr.half_round(block) == block).all()
        assert cvr.half_round(np.array(limits.ALBEDO_BG, np.float32)).tolist() == list(limits.ALBEDO_BG)
        if name not in limits.DENSE:
            assert (cvr.half_round(m.leaf_albedo[:64]) == m.leaf_albedo[:64]).all()


# ------------------------------------------------------------------- seeds ----
def _xorwow_first(state):
    """The first output of the XORWOW state (curand_kernel.h curand(): five words and the Weyl d)."""
    M = 0xFFFFFFFF
    v, d = list(state[:5]), state[5]
    t = v[0] ^ (v[0] >> 2)
    v4 = (v[4] ^ ((v[4] << 4) & M)) ^ (t ^ ((t << 1) & M))
    return (v4 + ((d + 362437) & M)) & M


def test_seed_sign_extension_is_visible(oracle_mod):
    """limits.SEED_SIGN: from id 256 on, seed + id read as int32 is negative and Rng(int) sign-extends
    it (Q3): the state is that of the 64-bit seed reduced by 2^32, not of the unsigned sum, and the
    first draw differs for at least 99 % of those paths."""
    differ = 0
    ids = range(256, limits.N_PATHS)
    for i in ids:
        u = (limits.SEED_SIGN + i) & 0xFFFFFFFF
        assert u >= 1 << 31
        signed = [int(v) for v in oracle_mod.rng_state(u - (1 << 32))]
        assert signed == curand_init_state(u - (1 << 32))
        unsigned = curand_init_state(u)
        assert signed != unsigned
        differ += _xorwow_first(signed) != _xorwow_first(unsigned)
    assert differ >= 0.99 * len(ids)
    # below id 256 the two readings agree
    u = limits.SEED_SIGN + 255
    assert [int(v) for v in oracle_mod.rng_state(u)] == curand_init_state(u)
    # the oracle's first draw is the model's
    got, _ = oracle_mod.rng_stream((limits.SEED_SIGN + 256) - (1 << 32), 1)
    assert int(got[0]) == _xorwow_first(curand_init_state((limits.SEED_SIGN + 256) - (1 << 32)))


# ----------------------------------------------------------------- fastdiv ----
def debug_fastdiv(cvr, d, u, on_device):
    fn = cvr.load().cvr_debug_fastdiv
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    u = np.ascontiguousarray(u, np.uint32)
    q = np.full(u.shape, 0xDEADBEEF, np.uint32)
    rc = fn(d, u.ctypes.data, q.ctypes.data, u.size, on_device)
    assert rc == 0, cvr.load().cvr_last_error(None)
    return q


def check_fastdiv(cvr, on_device):
    divisors = limits.fastdiv_divisors()
    assert len(divisors) > 280 and divisors[0] == 1 and divisors[-1] == (1 << 32) - 1
    for d in divisors:
        u = limits.fastdiv_dividends(d)
        q = debug_fastdiv(cvr, d, u, on_device)
        bad = np.nonzero(q != u // np.uint32(d))[0]
        assert bad.size == 0, f"d = {d}: u = {u[bad[:4]]} gives {q[bad[:4]]}"


def test_fastdiv_host(cvr):
    """make_fastdiv's constants with the three-line formula of cvr_walk.h fastdiv, on the host."""
    check_fastdiv(cvr, 0)
    assert cvr.load().cvr_debug_fastdiv(0, None, None, 0, 0) == -1  # d = 0: CVR_ERR_INVALID


def test_launch_constants():
    """The launches sit where DESIGN.md §5 (Range limits) says they do."""
    assert limits.WIDE_TILE[0] * limits.WIDE_TILE[1] == 1 << 24
    assert limits.TALL_TILE[0] * limits.TALL_TILE[1] == 16_777_152 <= 1 << 24
    assert limits.TOP_N == 4_294_967_232 <= 0xFFFFFFFF < limits.TOP_N + 192
    for first, count in limits.TOP_RANGES.values():
        assert first + count <= limits.TOP_N
    assert 64 * 64 * limits.MAX_SAMPLES == 1 << 32   # unit_to_path's rem << 6 stays below 2^32
    assert (limits.SEED_SIGN + 256) == 1 << 31 and (limits.SEED_WRAP + 256) == 1 << 32
