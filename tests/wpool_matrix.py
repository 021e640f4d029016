"""One entry per wave-pool kernel instance the library ships (kWpoolTable, csrc/cvr_wpool.hip): the
instance and a configuration that reaches it.  Plain Python, no GPU.

tests/test_wpool_matrix_cpu.py holds the entries against the table itself (cvr_debug_wpool_rows) and
against the selection rule's output; tests/test_gpu_wpool_matrix.py runs every entry against the oracle
and asks the library which instance ran (cvr_debug_last_wpool).

An instance is (eps, waves, med, record, flush) as include/cvr.h states it (CVR_HAS_WPOOL_DEBUG); med is a
layout (0 any dense medium, 1 sparse, 2 dense with cells and bounds, 3 the same with a uniform albedo)
plus 4 naiveMK's walk, 8 word counts, 16 the half format, 32 second moments, 64 an environment map.  The
tuples below are written out by hand: nothing here is computed from the selection rule.

An entry's configuration:
  kernel   regenerationSK (scatter -eps off), naiveSK (on) or naiveMK (its own walk, -eps on);
  medium   the 16^3 blob of tests/params.py as "f32", "half" (CVR_FORMAT_F16: the oracle sees the
           cvr_half_round-ed arrays), "uniform" (one rgb everywhere) or "uniform_half";
  sparse   uploaded as 2x2x2 leaves (the same values: the dense reference holds);
  opts     options set before the medium, by name;
  entry    "launch" cvr_launch_render, "trace" cvr_trace_launch, "frame" cvr_render_frame into a pinned
           image, "env" cvr_launch_render with an environment map set.
"""
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import params
from params_ref import Ref
from parity_util import NTHREADS

Entry = namedtuple("Entry", "name instance kernel medium sparse opts entry")

KERNEL_IDS = {"naiveSK": 0, "naiveMK": 1, "regenerationSK": 2}
CASES = ("box_all", "inside_all")
# launch 1: one sample per pixel of a 128x128 image (16384 paths); launch 2: the case as it stands (32x32 x 4)
ONE_TILE, ONE_SAMPLES = (128, 128), 1
# CVR_OPT_GRID, in waves: few waves carry the launch, so every lane regenerates.  cvr_render_frame
# takes the in-launch output only above 32 waves.
GRID, GRID_FRAME = 8, 64
MIN_PATHS_PER_WAVE = 256  # launch 1: four paths per lane
UNIFORM_RGB = (0.8, 0.65, 0.9)

DENSE, SPARSE = False, True
NONE = ()
CELLS0 = (("OPT_CELLS", 0),)
BOUNDS0 = (("OPT_BOUNDS", 0),)
HALF = (("OPT_MEDIUM_FORMAT", 1),)
MOMENTS = (("OPT_MOMENTS", 1),)
COUNT = (("OPT_COUNT_WORDS", 1),)


def WAVES(n):
    return (("OPT_WAVES", n),)


R, N, MK = "regenerationSK", "naiveSK", "naiveMK"
E = Entry
ENTRIES = [
    # ---- 5 waves per SIMD: every layout, fp32 and half, plain and with the in-launch output
    E("dense", (0, 5, 0, 0, 0), R, "f32", DENSE, CELLS0, "launch"),
    E("dense-eps", (1, 5, 0, 0, 0), N, "f32", DENSE, BOUNDS0, "launch"),
    E("dense-frame", (0, 5, 0, 0, 1), R, "f32", DENSE, BOUNDS0, "frame"),
    E("dense-eps-frame", (1, 5, 0, 0, 1), N, "f32", DENSE, CELLS0, "frame"),
    E("sparse", (0, 5, 1, 0, 0), R, "f32", SPARSE, NONE, "launch"),
    E("sparse-eps", (1, 5, 1, 0, 0), N, "f32", SPARSE, NONE, "launch"),
    E("sparse-frame", (0, 5, 1, 0, 1), R, "f32", SPARSE, NONE, "frame"),
    E("sparse-eps-frame", (1, 5, 1, 0, 1), N, "f32", SPARSE, NONE, "frame"),
    E("full", (0, 5, 2, 0, 0), R, "f32", DENSE, NONE, "launch"),
    E("full-eps", (1, 5, 2, 0, 0), N, "f32", DENSE, NONE, "launch"),
    E("full-frame", (0, 5, 2, 0, 1), R, "f32", DENSE, NONE, "frame"),
    E("full-eps-frame", (1, 5, 2, 0, 1), N, "f32", DENSE, NONE, "frame"),
    E("uniform", (0, 5, 3, 0, 0), R, "uniform", DENSE, NONE, "launch"),
    E("uniform-eps", (1, 5, 3, 0, 0), N, "uniform", DENSE, NONE, "launch"),
    E("uniform-frame", (0, 5, 3, 0, 1), R, "uniform", DENSE, NONE, "frame"),
    E("uniform-eps-frame", (1, 5, 3, 0, 1), N, "uniform", DENSE, NONE, "frame"),
    E("sparse-half", (0, 5, 17, 0, 0), R, "half", SPARSE, HALF, "launch"),
    E("sparse-half-eps", (1, 5, 17, 0, 0), N, "half", SPARSE, HALF, "launch"),
    E("sparse-half-frame", (0, 5, 17, 0, 1), R, "half", SPARSE, HALF, "frame"),
    E("sparse-half-eps-frame", (1, 5, 17, 0, 1), N, "half", SPARSE, HALF, "frame"),
    E("full-half", (0, 5, 18, 0, 0), R, "half", DENSE, HALF, "launch"),
    E("full-half-eps", (1, 5, 18, 0, 0), N, "half", DENSE, HALF, "launch"),
    E("full-half-frame", (0, 5, 18, 0, 1), R, "half", DENSE, HALF, "frame"),
    E("full-half-eps-frame", (1, 5, 18, 0, 1), N, "half", DENSE, HALF, "frame"),
    E("uniform-half", (0, 5, 19, 0, 0), R, "uniform_half", DENSE, HALF, "launch"),
    E("uniform-half-eps", (1, 5, 19, 0, 0), N, "uniform_half", DENSE, HALF, "launch"),
    E("uniform-half-frame", (0, 5, 19, 0, 1), R, "uniform_half", DENSE, HALF, "frame"),
    E("uniform-half-eps-frame", (1, 5, 19, 0, 1), N, "uniform_half", DENSE, HALF, "frame"),
    # ---- the other budgets: the generic layouts (a full dense medium degrades to the generic one; a
    # sparse medium's other budgets all run its 4-wave instance)
    E("waves3", (0, 3, 0, 0, 0), R, "f32", DENSE, WAVES(3), "launch"),
    E("waves3-eps", (1, 3, 0, 0, 0), N, "f32", DENSE, WAVES(3) + CELLS0, "launch"),
    E("waves4", (0, 4, 0, 0, 0), R, "f32", DENSE, WAVES(4) + BOUNDS0, "launch"),
    E("waves4-eps", (1, 4, 0, 0, 0), N, "f32", DENSE, WAVES(4), "launch"),
    E("waves6", (0, 6, 0, 0, 0), R, "uniform", DENSE, WAVES(6), "launch"),
    E("waves6-eps", (1, 6, 0, 0, 0), N, "f32", DENSE, WAVES(6), "launch"),
    E("sparse-waves4", (0, 4, 1, 0, 0), R, "f32", SPARSE, WAVES(4), "launch"),
    E("sparse-waves4-eps", (1, 4, 1, 0, 0), N, "f32", SPARSE, WAVES(6), "launch"),
    # ---- records (cvr_trace_launch)
    E("dense-trace", (0, 5, 0, 1, 0), R, "f32", DENSE, NONE, "trace"),
    E("dense-eps-trace", (1, 5, 0, 1, 0), N, "f32", DENSE, NONE, "trace"),
    E("sparse-trace", (0, 5, 1, 1, 0), R, "f32", SPARSE, NONE, "trace"),
    E("sparse-eps-trace", (1, 5, 1, 1, 0), N, "f32", SPARSE, NONE, "trace"),
    E("sparse-half-trace", (0, 5, 17, 1, 0), R, "half", SPARSE, HALF, "trace"),
    E("sparse-half-eps-trace", (1, 5, 17, 1, 0), N, "half", SPARSE, HALF, "trace"),
    E("sparse-waves4-trace", (0, 4, 1, 1, 0), R, "f32", SPARSE, WAVES(4), "trace"),
    E("sparse-waves4-eps-trace", (1, 4, 1, 1, 0), N, "f32", SPARSE, WAVES(4), "trace"),
    # ---- second moments, word counts
    E("dense-moments", (0, 5, 32, 0, 0), R, "f32", DENSE, MOMENTS, "launch"),
    E("dense-eps-moments", (1, 5, 32, 0, 0), N, "f32", DENSE, MOMENTS, "launch"),
    E("sparse-moments", (0, 5, 33, 0, 0), R, "f32", SPARSE, MOMENTS, "launch"),
    E("sparse-eps-moments", (1, 5, 33, 0, 0), N, "f32", SPARSE, MOMENTS, "launch"),
    E("sparse-count", (0, 5, 9, 0, 0), R, "f32", SPARSE, COUNT, "launch"),
    E("sparse-eps-count", (1, 5, 9, 0, 0), N, "f32", SPARSE, COUNT, "launch"),
    # ---- an environment map: the generic layouts, without and with the second moments
    E("dense-env", (0, 5, 64, 0, 0), R, "f32", DENSE, NONE, "env"),
    E("dense-eps-env", (1, 5, 64, 0, 0), N, "f32", DENSE, NONE, "env"),
    E("sparse-env", (0, 5, 65, 0, 0), R, "f32", SPARSE, NONE, "env"),
    E("sparse-eps-env", (1, 5, 65, 0, 0), N, "f32", SPARSE, NONE, "env"),
    E("sparse-half-env", (0, 5, 81, 0, 0), R, "half", SPARSE, HALF, "env"),
    E("sparse-half-eps-env", (1, 5, 81, 0, 0), N, "half", SPARSE, HALF, "env"),
    E("dense-env-moments", (0, 5, 96, 0, 0), R, "f32", DENSE, MOMENTS, "env"),
    E("dense-eps-env-moments", (1, 5, 96, 0, 0), N, "f32", DENSE, MOMENTS, "env"),
    E("sparse-env-moments", (0, 5, 97, 0, 0), R, "f32", SPARSE, MOMENTS, "env"),
    E("sparse-eps-env-moments", (1, 5, 97, 0, 0), N, "f32", SPARSE, MOMENTS, "env"),
    # ---- naiveMK's walk (scatter -eps always)
    E("mk-dense", (1, 5, 4, 0, 0), MK, "f32", DENSE, CELLS0, "launch"),
    E("mk-sparse", (1, 5, 5, 0, 0), MK, "f32", SPARSE, NONE, "launch"),
    E("mk-full", (1, 5, 6, 0, 0), MK, "f32", DENSE, NONE, "launch"),
    E("mk-uniform", (1, 5, 7, 0, 0), MK, "uniform", DENSE, NONE, "launch"),
    E("mk-sparse-half", (1, 5, 21, 0, 0), MK, "half", SPARSE, HALF, "launch"),
    E("mk-full-half", (1, 5, 22, 0, 0), MK, "half", DENSE, HALF, "launch"),
    E("mk-uniform-half", (1, 5, 23, 0, 0), MK, "uniform_half", DENSE, HALF, "launch"),
]
del E
BY_NAME = {e.name: e for e in ENTRIES}


def opt(entry, name):
    """The value the entry sets for option `name`, or None."""
    return dict(entry.opts).get(name)


def grid_of(entry):
    return GRID_FRAME if entry.entry == "frame" else GRID


def md_eff(half_round, md=params.MAX_DENSITY):
    """CVR_FORMAT_F16's majorant: max(max_density, f32(f16(max_density)))."""
    return max(float(np.float32(md)), float(half_round(np.array([md], np.float32))[0]))


def medium_arrays(variant, half_round):
    """(density, albedo, max_density) the oracle walks for a medium variant; half_round: cvr.half_round."""
    density, albedo = params.blob16()
    if variant.startswith("uniform"):
        albedo[..., :3] = UNIFORM_RGB
    if variant.endswith("half"):
        return half_round(density), half_round(albedo), md_eff(half_round)
    assert variant in ("f32", "uniform"), variant
    return density, albedo, params.MAX_DENSITY


def upload_arrays(variant):
    """(density, albedo) as uploaded: the library rounds a CVR_FORMAT_F16 medium itself."""
    density, albedo = params.blob16()
    if variant.startswith("uniform"):
        albedo[..., :3] = UNIFORM_RGB
    return density, albedo


def launch_case(case_name, which):
    """(case, samples) of launch "one" or "acc"."""
    case = params.CASES[case_name]
    return (params.at_tile(case, ONE_TILE), ONE_SAMPLES) if which == "one" else (case, params.SAMPLES)


def _trace(orc, L, n):
    step = (n + NTHREADS - 1) // NTHREADS
    with ThreadPoolExecutor(NTHREADS) as ex:
        parts = list(ex.map(lambda a: orc.trace_paths(L, a, min(step, n - a)), range(0, n, step)))
    return np.concatenate(parts)


def check_guards(ref, samples, what):
    """A reference that cannot let a wrong kernel pass: escapes and roulette deaths both occur, and in an
    accumulating launch some pixel receives more than one contribution."""
    esc = float(((ref.recs["flags"] & 1) != 0).mean())
    assert 0.2 <= esc <= 1.0, f"{what}: {esc:.3f} of the paths escape"
    assert (ref.recs["flags"] == 0).any(), f"{what}: no path dies by roulette"
    if samples > 1:
        assert ref.cnt.max() > 1, f"{what}: no pixel gets more than one contribution"
    else:
        assert ref.cnt.max() == 1, what


class Refs:
    """The oracle's records per (case, kernel id, medium variant, launch), traced once and kept."""

    def __init__(self, oracle_mod, half_round):
        self.oracle_mod = oracle_mod
        self.half_round = half_round
        self.cache = {}
        self.evals_cache = {}

    def _oracle(self, case, variant):
        density, albedo, md = medium_arrays(variant, self.half_round)
        return params.make_oracle(self.oracle_mod, case, density, albedo, md)

    def get(self, case_name, kernel, variant, which):
        key = (case_name, kernel, variant, which)
        if key not in self.cache:
            case, samples = launch_case(case_name, which)
            L = params.make_launch(self.oracle_mod, case, KERNEL_IDS[kernel])
            ref = Ref(_trace(self._oracle(case, variant), L, params.n_paths(case, samples)), case, samples)
            ref.recs.flags.writeable = False
            check_guards(ref, samples, " ".join(key))
            self.cache[key] = ref
        return self.cache[key]

    def evals(self, case_name, kernel, variant):
        """Launch 1's evaluation log (Oracle.trace_evals), for the word-count bounds."""
        key = (case_name, kernel, variant)
        if key not in self.evals_cache:
            case, samples = launch_case(case_name, "one")
            L = params.make_launch(self.oracle_mod, case, KERNEL_IDS[kernel])
            recs, evals = self._oracle(case, variant).trace_evals(L, 0, params.n_paths(case, samples))
            assert recs.tobytes() == self.get(case_name, kernel, variant, "one").recs.tobytes()
            self.evals_cache[key] = evals
        return self.evals_cache[key]
