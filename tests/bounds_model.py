"""A plain restatement of the brick bounds: the bound table,
the sparse brick codes and empty-region mask, and what they decide per density
evaluation.  numpy and exact rational arithmetic only; nothing here calls the
library.  Together with the oracle's evaluation log (Oracle.trace_evals) it says
what cvr_stats.fetches must be and where cvr_stats.words must lie.

Conventions: grids are (z, y, x) arrays, `res` is (nx, ny, nz), a brick has
B = 2^bshift cells per axis, code tables are (bz, by, bx) arrays of ints.

Codes.  bound_value(c) is the float with bits (c << 19) + (112 << 23).  Brick b of
an axis holds the cells [bB, bB+B-1], which interpolate the voxels
[bB, min(bB+B, res-1)] (the texel clamp).  mx is the maximum of 0 and those
voxels; the code is 255 if one of them is NaN or +inf or mx > max_density, else the
smallest c with bound_value(c) * max_density >= mx * (1 + 2^-16), capped at 255.
The comparison is made in fractions.Fraction; code_margin() is the relative
distance of a brick from the nearest threshold, so that a test can require that
no other correct arithmetic (the library works in doubles) may disagree.

Sparse media.  The codes are those of the densified grid at the library's brick
shift (sparse_bshift).  A leaf has a cell leaf iff it or one of its 7 forward
neighbours exists; a brick in a leaf without one has code 0.  The mask has one
bit per super-brick of 2^es cells per axis, es the smallest value >= 3 whose
super-brick grid, each axis padded to a power of two, fits 2048 bits; a bit is set
iff a leaf of the super-brick has a cell leaf.

Per evaluation (a row of the oracle's log: grid coordinate, test draw, test
value).  in-grid <=> 0 <= c < res on all three axes.  An in-grid point reads the
code of the brick of its cell floor(c), an off-grid point reads 255 (the sentinel).
fetch <=> not (bound_value(code) < xi_test).  cvr_stats.fetches is the number of
fetches; with the bounds off every code is 255 and it equals the evaluations.

Brick words (cvr_stats.words, the sparse counting launch).  The wave pool loads
the word of both tentative points of a lookahead pair before it tests either
(cvr_wpool.hip, the track loop), so points it then drops are counted and there is
no exact model, only bounds:
    W_lo = evaluated points that are in-grid and whose mask bit is set (mask off,
           or bounds off: every in-grid evaluated point),
    W_hi = W_lo + 2 S + F,
S the segments that ran Woodcock tracking, F the model's fetches.  From the code:
a word is loaded only for the two points of a pair, and every evaluated point is a
point of the pair that evaluates it, hence W_lo.  Points loaded and not evaluated
in that pair are: both points of a pair whose first point lies past max_t (2), the
second point of a pair whose second point lies past max_t (1) -- a segment ends
past max_t at most once -- and the second point of a pair whose first point needs
its cell (the sparse kernel parks the lane and drops the second point, which the
next pair draws again: 1 per fetch; a real collision is such a fetch).  So the
extra loads are at most 2 per segment that ended past max_t plus 1 per fetch,
which is at most 2 S + F.  S = (steps - density evaluations) + real collisions:
a tracked segment ends either past max_t (a step without an evaluation) or with an
accepted evaluation (not (test value < test draw)).
"""
from fractions import Fraction

import numpy as np

NO_LEAF = 0xFFFFFFFF
EMASK_BITS = 2048
MARGIN = Fraction(1, 1 << 40)


def bound_value(c):
    """The float32 with bits (c << 19) + (112 << 23) (scalar or array of codes)."""
    bits = (np.asarray(c, np.uint32) << np.uint32(19)) + np.uint32(112 << 23)
    return bits.view(np.float32)


BOUND_VALUES = bound_value(np.arange(256))
_BV = [Fraction(float(v)) for v in BOUND_VALUES]
_UP = 1 + Fraction(1, 1 << 16)


def code_of_max(mx, max_density, bad=False):
    """The code of a brick whose largest voxel is mx (float32); `bad`: a NaN or +inf voxel."""
    mx = np.float32(mx)
    if bad or np.isnan(mx) or np.isinf(mx):
        return 255
    md = Fraction(float(np.float32(max_density)))
    m = Fraction(float(mx))
    if not (md > 0 and m <= md):
        return 255
    target = m * _UP
    lo, hi = 0, 255  # the smallest c in [0, 255] with _BV[c] * md >= target, else 255
    while lo < hi:
        mid = (lo + hi) // 2
        if _BV[mid] * md >= target:
            hi = mid
        else:
            lo = mid + 1
    return lo


def code_margin(mx, max_density):
    """Relative distance of mx (1 + 2^-16) from the nearest threshold bound_value(c) * max_density
    that could change its code (None: no threshold matters, mx is 0 or the code is 255 by rule)."""
    m = Fraction(float(np.float32(mx)))
    md = Fraction(float(np.float32(max_density)))
    if m <= 0 or m > md:
        return None
    c = code_of_max(mx, max_density)
    target = m * _UP
    near = [abs(_BV[k] * md / target - 1) for k in (c - 1, c) if 0 <= k < 255]
    return min(near) if near else None


def _window_reduce(a, axis, B, short, op):
    n = a.shape[axis]
    out = []
    for b in range(-(-n // B)):
        hi = min(b * B + (B - 1 if short else B), n - 1)
        out.append(op.reduce(np.take(a, np.arange(b * B, hi + 1), axis=axis), axis=axis))
    return np.stack(out, axis=axis)


def brick_maxima(D, bshift, short_window=False):
    """(mx, bad) per brick: the maximum of 0 and the voxels [bB, min(bB+B, res-1)] of each axis (NaN
    ignored), and whether one of them is NaN or +inf.  short_window: the wrong window [bB, bB+B-1],
    for tests that must tell the two apart."""
    D = np.asarray(D, np.float32)
    B = 1 << bshift
    mx = np.fmax(D, np.float32(0))
    bad = np.isnan(D) | (D == np.inf)
    for axis in range(3):
        mx = _window_reduce(mx, axis, B, short_window, np.fmax)
        bad = _window_reduce(bad, axis, B, short_window, np.logical_or)
    return mx, bad


def dense_codes(D, max_density, bshift, short_window=False, margin=True):
    """Code table (bz, by, bx) of the grid D.  margin: assert that no brick lies within 2^-40
    relative of a threshold."""
    mx, bad = brick_maxima(D, bshift, short_window)
    codes = np.full(mx.shape, 255, np.int64)
    ok = ~bad
    for v in np.unique(mx[ok]):
        codes[ok & (mx == v)] = code_of_max(v, max_density)
        if margin:
            g = code_margin(v, max_density)
            assert g is None or g > MARGIN, f"brick maximum {v!r} lies on a code threshold"
    return codes


# ------------------------------------------------------------------ sparse ---
def sparse_bshift(bounds_opt):
    """The brick shift of a sparse medium for CVR_OPT_BOUNDS `bounds_opt` (None: not set);
    None: unbounded (every code 255, no mask)."""
    if bounds_opt is None:
        return 3
    if bounds_opt == 0:
        return None
    return min(bounds_opt, 3)


def densify(res, table, leaf_density):
    """The (nz, ny, nx) grid a leaf table stands for (absent leaves: 0)."""
    nx, ny, nz = res
    lz, ly, lx = table.shape
    full = np.zeros((lz * 8, ly * 8, lx * 8), np.float32)
    ld = np.asarray(leaf_density, np.float32).reshape(-1, 8, 8, 8)
    for z, y, x in zip(*np.nonzero(table != NO_LEAF)):
        full[8 * z:8 * z + 8, 8 * y:8 * y + 8, 8 * x:8 * x + 8] = ld[table[z, y, x]]
    return full[:nz, :ny, :nx].copy()


def cell_leaves(table):
    """Per leaf: it or one of its 7 forward neighbours exists."""
    occ = table != NO_LEAF
    lz, ly, lx = occ.shape
    cell = occ.copy()
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cell[:lz - dz, :ly - dy, :lx - dx] |= occ[dz:, dy:, dx:]
    return cell


def sparse_codes(res, table, leaf_density, max_density, bshift, short_window=False, margin=True):
    """Code table of a sparse medium at brick shift bshift (1..3)."""
    assert 1 <= bshift <= 3
    codes = dense_codes(densify(res, table, leaf_density), max_density, bshift, short_window, margin)
    per_leaf = 8 >> bshift
    cell = cell_leaves(table)
    for axis in range(3):
        cell = np.repeat(cell, per_leaf, axis=axis)
    bz, by, bx = codes.shape
    codes[~cell[:bz, :by, :bx]] = 0
    return codes


def mask_shift(leaf_dims):
    """es: the smallest value >= 3 whose super-brick grid (2^(es-3) leaves per axis), each axis padded
    to a power of two, has at most 2048 super-bricks.  leaf_dims in any axis order."""
    es = 3
    while True:
        n = 1
        for d in leaf_dims:
            sb = -(-int(d) // (1 << (es - 3)))
            n *= 1 << (sb - 1).bit_length()
        if n <= EMASK_BITS:
            return es
        es += 1


def sparse_mask(table):
    """(es, mask): mask[sz, sy, sx] is set iff a leaf of that super-brick has a cell leaf."""
    es = mask_shift(table.shape)
    k = 1 << (es - 3)
    cell = cell_leaves(table)
    sz, sy, sx = (-(-n // k) for n in cell.shape)
    pad = np.zeros((sz * k, sy * k, sx * k), bool)
    pad[:cell.shape[0], :cell.shape[1], :cell.shape[2]] = cell
    return es, pad.reshape(sz, k, sy, k, sx, k).any(axis=(1, 3, 5))


# ---------------------------------------------------------- per evaluation ---
def in_grid(evals, res):
    ok = np.ones(len(evals), bool)
    for f, n in zip(("cx", "cy", "cz"), res):
        c = evals[f]
        ok &= (c >= 0) & (c < np.float32(n))  # NaN: off the grid
    return ok


def cell_index(evals, res):
    """(inside, x1, y1, z1): floor of the coordinate (0 where the point is off the grid)."""
    inside = in_grid(evals, res)
    idx = [np.where(inside, np.floor(np.where(inside, evals[f], 0)), 0).astype(np.int64) for f in ("cx", "cy", "cz")]
    return (inside, *idx)


def eval_codes(evals, res, codes, bshift):
    """The code every evaluation reads: its brick's, 255 off the grid; codes None: the bounds are off."""
    if codes is None:
        return np.full(len(evals), 255, np.int64)
    inside, x1, y1, z1 = cell_index(evals, res)
    return np.where(inside, codes[z1 >> bshift, y1 >> bshift, x1 >> bshift], 255)


def fetch_flags(evals, res, codes, bshift):
    return ~(bound_value(eval_codes(evals, res, codes, bshift)) < evals["xi_test"])


def expected_fetches(evals, res, codes, bshift, ranges=None):
    """cvr_stats.fetches of the launch that made `evals`; ranges: [(first, end), ...] of path ids ->
    a list with one count per range."""
    f = fetch_flags(evals, res, codes, bshift)
    if ranges is None:
        return int(f.sum())
    pid = evals["path_id"]
    return [int(f[(pid >= a) & (pid < b)].sum()) for a, b in ranges]


def real_collisions(evals):
    return ~(evals["test_value"] < evals["xi_test"])


def unsound(evals, res, codes, bshift):
    """In-grid evaluations whose test value exceeds their brick's bound (the proof says: none)."""
    inside = in_grid(evals, res)
    return inside & ~(evals["test_value"] <= bound_value(eval_codes(evals, res, codes, bshift)))


def word_bounds(evals, records, res, fetches, mask=None, es=None):
    """(W_lo, W_hi, S) of a sparse counting launch (module docstring).  mask None: every bit set."""
    inside, x1, y1, z1 = cell_index(evals, res)
    loaded = inside if mask is None else inside & mask[z1 >> es, y1 >> es, x1 >> es]
    w_lo = int(loaded.sum())
    segs = int(records["n_steps"].sum()) - int(records["n_density"].sum()) + int(real_collisions(evals).sum())
    return w_lo, w_lo + 2 * segs + fetches, segs
