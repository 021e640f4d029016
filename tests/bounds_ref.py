"""What the oracle and the bound model (tests/bounds_model.py) say about one launch of the
brick-bound media (tests/media.py): a tile of 32x32 pixels x 8 iterations = 8192 paths from
cvr.default_camera, seed 3.  Computed once per (medium, format, Q4 setting, kernel id) and shared
by tests/test_bounds_model.py (CPU) and tests/test_gpu_bounds_model.py; nothing here touches a GPU
(default_camera and half_round are host functions of the library)."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import bounds_model as bm
import media
import oracle
from parity_util import NTHREADS

TILE = (32, 32)
ITERS = 8
N = TILE[0] * TILE[1] * ITERS
SEED = 3
QUARTERS = [(q * N // 4, (q + 1) * N // 4) for q in range(4)]

# records / evals: Oracle.trace_evals of path ids [0, N); stats: the oracle's seven counters
Ref = namedtuple("Ref", "records evals stats res")


def _cvr():
    import cudavolumerenderer_amd as cvr
    cvr.load()
    return cvr


# (full image resolution, offset of the 32x32 tile in it) per medium.  sparse_es4 is seen through
# the centre tile of a 256x256 image: its 8192 paths cross 2x2 columns of super-bricks, so that one
# super-brick holds more evaluations than the slack of the brick-word bounds.
VIEWS = {"sparse_es4": ((256, 256), (112, 112))}


def view(name):
    return VIEWS.get(name, (TILE, (0, 0)))


@lru_cache(maxsize=None)
def camera(full=TILE):
    return _cvr().default_camera(*full)


def md_eff(md):
    """Format 1's majorant: max(max_density, f32(f16(max_density)))."""
    return max(float(np.float32(md)), float(_cvr().half_round(np.array([md], np.float32))[0]))


@lru_cache(maxsize=None)
def medium(name, fmt=0):
    """The medium as the library stores it: format 1 is the half-rounded arrays with md_eff."""
    m = (media.DENSE_MEDIA.get(name) or media.SPARSE_MEDIA[name])()
    if not fmt:
        return m
    hr = _cvr().half_round
    if isinstance(m, media.Dense):
        return m._replace(density=hr(m.density), albedo=hr(m.albedo), max_density=md_eff(m.max_density))
    return m._replace(leaf_density=hr(m.leaf_density), leaf_albedo=hr(m.leaf_albedo),
                      albedo_bg=tuple(float(v) for v in hr(np.array(m.albedo_bg, np.float32))),
                      max_density=md_eff(m.max_density))


def res_of(m):
    return m.density.shape[::-1] if isinstance(m, media.Dense) else tuple(m.res)


def make_oracle(m):
    if isinstance(m, media.Dense):
        return oracle.Oracle(m.density, m.albedo, m.box_min, m.box_max, m.scale, m.max_density)
    return oracle.Oracle.from_leaves(m.res, m.table, m.leaf_density, m.leaf_albedo, m.albedo_bg, scale=media.SCALE,
                                     max_density=m.max_density)


@lru_cache(maxsize=None)
def reference(name, fmt=0, q4=0, kernel=2, n=N):
    m = medium(name, fmt)
    orc = make_oracle(m)
    full, offset = view(name)
    iv, r2v = camera(full)
    L = orc.launch(iv, r2v, full, TILE, offset, kernel, SEED, world_to_aabb=q4)
    records, evals = orc.trace_evals(L, 0, n)
    _, st = orc.render(L, 0, n, nthreads=NTHREADS)
    return Ref(records, evals, st.as_dict(), res_of(m))


@lru_cache(maxsize=None)
def codes(name, fmt, bounds_opt, short_window=False):
    """(code table, brick shift) the library builds for CVR_OPT_BOUNDS bounds_opt (None: not set);
    (None, None): the bounds are off (every point reads 255)."""
    m = medium(name, fmt)
    if isinstance(m, media.Dense):
        bshift = 2 if bounds_opt is None else bounds_opt
        if bshift == 0:
            return None, None
        return bm.dense_codes(m.density, m.max_density, bshift, short_window), bshift
    bshift = bm.sparse_bshift(bounds_opt)
    if bshift is None:
        return None, None
    return bm.sparse_codes(m.res, m.table, m.leaf_density, m.max_density, bshift, short_window), bshift


def expected(name, fmt=0, q4=0, kernel=2, bounds_opt=None):
    """(fetches of the whole launch, fetches of the four quarter ranges)."""
    ref = reference(name, fmt, q4, kernel)
    table, bshift = codes(name, fmt, bounds_opt)
    return (bm.expected_fetches(ref.evals, ref.res, table, bshift),
            bm.expected_fetches(ref.evals, ref.res, table, bshift, QUARTERS))
