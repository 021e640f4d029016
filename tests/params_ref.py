"""What the parameter-space GPU tests share (tests/test_gpu_params.py, tests/test_gpu_limits.py,
tests/test_gpu_wpool_matrix.py): the oracle's records of a case turned into what a render of them must
give, the comparisons with a render, and the sparse upload of the cases' medium.  Nothing here touches
a GPU; the library is used for its host functions only."""
import numpy as np

import media
import params
from parity_util import COUNTERS, assert_counters_equal, assert_sums_close


class Ref:
    """The oracle's records of one case and kernel id, and what a render of them must give: the
    counters, and per pixel the sums of T and fl32(T T) over its escapes, added sample by sample in
    fp32, with the escape count."""

    def __init__(self, recs, case, samples=params.SAMPLES):
        self.recs = recs
        px = case.tile[0] * case.tile[1]
        self.s1 = np.zeros((px, 3), np.float32)
        self.s2 = np.zeros((px, 3), np.float32)
        self.cnt = np.zeros(px, np.int64)
        for s in range(samples):
            r = recs[s * px:(s + 1) * px]
            esc = (r["flags"] & 1) != 0
            ids = r["image_id"][esc]
            assert len(np.unique(ids)) == len(ids)
            T = r["T"][esc].astype(np.float32)
            self.s1[ids] += T
            self.s2[ids] += T * T
            self.cnt[ids] += 1
        self.counters = dict(paths=len(recs), segments=int(recs["n_segments"].sum()),
                             steps=int(recs["n_steps"].sum()), density=int(recs["n_density"].sum()),
                             albedo=int(recs["n_albedo"].sum()), escaped=int(((recs["flags"] & 1) != 0).sum()),
                             truncated=int(((recs["flags"] & 2) != 0).sum()))
        assert set(self.counters) == set(COUNTERS)


class Refs:
    def __init__(self, oracle_mod):
        self.oracle_mod = oracle_mod
        self.blob = params.blob16()
        self.cache = {}

    def get(self, name, kid, half=None):
        """half: None, or (cvr, max_density_eff) for the oracle of the half-rounded arrays."""
        key = (name, kid, None if half is None else half[1])
        if key not in self.cache:
            case = params.CASES[name]
            if half is None:
                orc = params.make_oracle(self.oracle_mod, case, *self.blob)
            else:
                cvr, md_eff = half
                orc = params.make_oracle(self.oracle_mod, case, cvr.half_round(self.blob[0]),
                                         cvr.half_round(self.blob[1]), md_eff)
            L = params.make_launch(self.oracle_mod, case, kid)
            self.cache[key] = Ref(orc.trace_paths(L, 0, params.n_paths(case)), case)
        return self.cache[key]


def blob_leaves(blob):
    """(leaf table (2, 2, 2), leaf density (8, 512), leaf albedo (8, 512, 4)) of a 16^3 medium."""
    density, albedo = blob
    table = np.arange(8, dtype=np.uint32).reshape(2, 2, 2)
    dens = np.zeros((8, 512), np.float32)
    alb = np.zeros((8, 512, 4), np.float32)
    for lz in range(2):
        for ly in range(2):
            for lx in range(2):
                sl = (slice(8 * lz, 8 * lz + 8), slice(8 * ly, 8 * ly + 8), slice(8 * lx, 8 * lx + 8))
                dens[table[lz, ly, lx]] = density[sl].reshape(512)
                alb[table[lz, ly, lx]] = albedo[sl].reshape(512, 4)
    return table, dens, alb


def sparse_blob(cvr, blob, p):
    """blob16 (or arrays of its shape) as 2x2x2 leaves of 8^3 (tests/media.sparse_desc) with the case's
    box and BSDF."""
    table, dens, alb = blob_leaves(blob)
    s, keep = media.sparse_desc(cvr, (16, 16, 16), table, dens, alb, (0.0, 0.0, 0.0, 1.0), params.MAX_DENSITY)
    s.box_min[:] = p["box_min"]
    s.box_max[:] = p["box_max"]
    s.scale = params.SCALE
    s.g = p["g"]
    s.roughness[:] = p["roughness"]
    s.eta = p["eta"]
    return s, keep


def assert_records_equal(g, c, fields, what):
    assert len(g) == len(c)
    for f in fields:
        mism = np.nonzero(g[f] != c[f])[0]
        assert mism.size == 0, f"{what}: {f} differs for {mism.size} paths, first {mism[:5]}"
    mism = np.nonzero((g["T"].view(np.uint32) != c["T"].view(np.uint32)).any(axis=1))[0]
    assert mism.size == 0, (f"{what}: T bits differ for {mism.size} paths, first {mism[:5]}: gpu "
                            f"{g['T'][mism[:2]]} cpu {c['T'][mism[:2]]}")


def assert_frame(out, st, ref, what, scale=1.0, exact_w=True):
    px = len(ref.cnt)
    out = out.reshape(px, 4)
    assert_counters_equal(st, ref.counters, what)
    assert_sums_close(out[:, :3], ref.s1 / np.float32(scale), ref.cnt, what)  # scale: a power of two
    if exact_w:
        assert (out[:, 3] == (ref.cnt > 0)).all(), f"{what}: w channel"
    else:
        assert ((out[:, 3] != 0) == (ref.cnt > 0)).all(), f"{what}: w channel"
