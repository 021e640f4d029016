"""The brick-bound model (tests/bounds_model.py) and the oracle's evaluation log, on the CPU.

Known answers of the table and the code rule; the soundness of the bound proof
over every logged evaluation of every test medium, brick size and storage format; the log
itself against oracle_trace_paths; and the conditions that make the GPU tests of
tests/test_gpu_bounds_model.py sharp, evaluated from the oracle and the model alone.

Measured with cvr.default_camera(32, 32), 8192 paths, seed 3, format 0 (bounds_ref; the prototype's
hand-written camera gave other figures):
  staircase     477 849 evaluations, 46 588 off the grid (all at negative coordinates), 96 612 in a
                last cell layer; 54 distinct codes at B = 4 (75 at B = 2); the model expects 107 115
                fetches at B = 4, and 104 596 / 109 871 with every code one lower / higher; of the 240
                single changes (brick with code < 255, +-1) 11 leave the count unchanged (4.6 %).
                The box is stretched to (-0.5..0.59, 0.60, 0.64): under the default worldToAABB (Q4)
                a unit box maps to [0, res - 1] and never enters the one-cell-thick last bricks.
  spikes        332 094 evaluations; the model with the short window [bB, bB+B-1] bounds out 191 real
                collisions (and expects 37 774 fetches instead of 169 156 at B = 4).
  random40      61 698 evaluations, 60 836 fetches at B = 4 (6 distinct codes).
  offgrid       Q4 default: 20 880 evaluations, 5 821 off the grid (none negative: the camera enters
                at the far z face), 7 633 in a last cell layer; CVR_OPT_WORLD_TO_AABB 1: 18 904, none off.
  sparse_small  386 778 evaluations, es 3, 16 of 24 mask bits set; 239 280 fetches at the default 8^3
                bricks; W_lo 240 602, W_hi 509 944.
  sparse_es4    (the centre 32x32 tile of cvr.default_camera(256, 256)) 786 200 evaluations, es 4, 29
                of 288 super-bricks set; 38 196 fetches at 8^3 bricks; W_lo 422 206, W_hi 480 606 <
                786 200 in-grid evaluations; forcing the bit of the clear super-brick (z, y, x) =
                (3, 3, 4) or (3, 4, 4) adds 68 718 / 61 822 words, more than the slack of 58 400.
No evaluation of any medium, brick size or format violates the proof."""
from fractions import Fraction

import numpy as np
import pytest

import bounds_model as bm
import bounds_ref as br
import media

DENSE = ["staircase", "spikes", "random40", "offgrid"]
SPARSE = ["sparse_small", "sparse_es4"]


# ---------------------------------------------------------- known answers ---
def test_bound_value_table():
    assert bm.bound_value(0) == np.float32(2.0 ** -15)
    assert bm.bound_value(240) == np.float32(1.0)
    assert bm.bound_value(255) == np.float32(1.9375)
    assert bm.bound_value(16 * 9 + 6) == np.float32(2.0 ** -6 * (1 + 6 / 16))
    assert (np.diff(bm.BOUND_VALUES.astype(np.float64)) > 0).all()
    assert bm.BOUND_VALUES.dtype == np.float32 and len(bm.BOUND_VALUES) == 256


def test_code_rule_known_answers():
    assert bm.code_of_max(0.0, 1.0) == 0
    for md in (1.0, 0.37, 3.0):
        assert bm.code_of_max(np.float32(md), np.float32(md)) == 241
    for c in (0, 1, 17, 150, 209, 239, 240):
        v = bm.bound_value(c)
        assert bm.code_of_max(v, 1.0) == c + 1
        # the largest mx that still gets c lies just below bound_value(c) / (1 + 2^-16)
        below = np.float32(float(v) / (1 + 2.0 ** -16))
        while Fraction(float(below)) * (1 + Fraction(1, 65536)) > Fraction(float(v)):
            below = np.nextafter(below, np.float32(0), dtype=np.float32)
        assert bm.code_of_max(below, 1.0) == c
        assert bm.code_of_max(np.nextafter(below, np.float32(4), dtype=np.float32), 1.0) == c + 1
    assert bm.code_of_max(np.float32(2.0 ** -20), 1.0) == 0          # below bound_value(0)
    assert bm.code_of_max(np.nextafter(np.float32(1), np.float32(2)), 1.0) == 255   # above the majorant
    assert bm.code_of_max(np.float32(0.5), 1.0, bad=True) == 255
    assert bm.code_of_max(np.float32(np.nan), 1.0) == 255 and bm.code_of_max(np.float32(np.inf), 1.0) == 255


def test_dense_codes_window_nan_inf_and_ragged_edge():
    d = np.zeros((5, 6, 9), np.float32)  # (nz, ny, nx); B = 4: 3 x 2 x 2 bricks, all axes ragged
    d[0, 0, 4] = 0.5       # voxel x = 4: the +1 voxel of brick x 0, the first of brick x 1
    d[4, 5, 8] = 0.25      # the far corner: brick (2, 1, 1) alone
    codes = bm.dense_codes(d, 1.0, 2)
    assert codes.shape == (2, 2, 3)
    half, quarter = bm.code_of_max(0.5, 1.0), bm.code_of_max(0.25, 1.0)
    assert (half, quarter) == (16 * 14 + 1, 16 * 13 + 1)
    assert codes[0, 0, 0] == half and codes[0, 0, 1] == half and codes[0, 0, 2] == 0
    assert codes[1, 1, 2] == quarter and codes[1, 1, 1] == quarter  # x = 8 is brick 1's +1 voxel too
    assert codes[0, 1, 0] == 0
    short = bm.dense_codes(d, 1.0, 2, short_window=True)
    assert short[0, 0, 0] == 0 and short[0, 0, 1] == half
    for bad in (np.nan, np.inf):
        e = d.copy()
        e[2, 2, 2] = bad
        c = bm.dense_codes(e, 1.0, 2)
        assert c[0, 0, 0] == 255 and c[0, 0, 1] == half and c[1, 1, 2] == quarter
    e = d.copy()
    e[0, 0, 0] = 1.5  # above the majorant
    assert bm.dense_codes(e, 1.0, 2)[0, 0, 0] == 255
    with pytest.raises(AssertionError):  # a maximum within 2^-40 of a threshold is refused
        on = np.zeros((2, 2, 2), np.float32)
        on[0, 0, 0] = 1.0
        bm.dense_codes(on, float(np.float32(1 + 2.0 ** -16)), 1)


def test_sparse_rules():
    assert [bm.sparse_bshift(o) for o in (None, 0, 1, 2, 3, 5)] == [3, None, 1, 2, 3, 3]
    assert bm.mask_shift((4, 2, 3)) == 3 and bm.mask_shift((8, 16, 17)) == 4
    assert bm.mask_shift((16, 16, 8)) == 3 and bm.mask_shift((256, 128, 256)) == 7  # the C5 cloud: 128^3 cells
    small, es4 = br.medium("sparse_small"), br.medium("sparse_es4")
    es, mask = bm.sparse_mask(small.table)
    assert es == 3 and mask.shape == small.table.shape and 0 < mask.sum() < mask.size
    assert np.array_equal(mask, bm.cell_leaves(small.table))
    es, mask = bm.sparse_mask(es4.table)
    assert es == 4 and mask.shape == (4, 8, 9) and 0 < mask.sum() < mask.size
    sb = {(x >> 1, y >> 1, z >> 1) for x, y, z in media.ES4_LEAVES}
    assert len(sb) < len(media.ES4_LEAVES)                 # two leaves share a super-brick
    assert any(x == 16 for x, _, _ in media.ES4_LEAVES)    # the ragged last leaf column
    assert mask[2, 4, 8] and not mask[0, 0, 0]
    # a brick of a leaf without a cell leaf has code 0; with one, the densified grid's code
    for m in (small, es4):
        for bshift in (1, 2, 3):
            codes = bm.sparse_codes(m.res, m.table, m.leaf_density, m.max_density, bshift)
            dense = bm.dense_codes(bm.densify(m.res, m.table, m.leaf_density), m.max_density, bshift)
            cell = bm.cell_leaves(m.table)
            per = 8 >> bshift
            for axis in range(3):
                cell = np.repeat(cell, per, axis=axis)
            cell = cell[:codes.shape[0], :codes.shape[1], :codes.shape[2]]
            assert (codes[~cell] == 0).all() and np.array_equal(codes[cell], dense[cell])
            assert (dense[~cell] == 0).all()  # (their voxels are all 0: the rule changes nothing here)


# ------------------------------------------------------ the evaluation log ---
@pytest.mark.parametrize("name,kernel", [("staircase", 2), ("staircase", 0), ("staircase", 1), ("offgrid", 2),
                                         ("sparse_small", 2)])
def test_eval_log_matches_trace_paths(name, kernel):
    ref = br.reference(name, 0, 0, kernel)
    m = br.medium(name)
    orc = br.make_oracle(m)
    full, offset = br.view(name)
    iv, r2v = br.camera(full)
    L = orc.launch(iv, r2v, full, br.TILE, offset, kernel, br.SEED)
    plain = orc.trace_paths(L, 0, br.N)
    assert plain.tobytes() == ref.records.tobytes()
    ev = ref.evals
    assert len(ev) == int(plain["n_density"].sum()) == ref.stats["density"] > 0
    assert (np.diff(ev["path_id"].astype(np.int64)) >= 0).all()  # walk order: path after path
    assert np.array_equal(np.bincount(ev["path_id"], minlength=br.N), plain["n_density"])
    assert ((ev["xi_test"] > 0) & (ev["xi_test"] <= 1)).all()
    # accepted evaluations: every scatter is one (a collision at t == max_t is one without a scatter)
    real = np.bincount(ev["path_id"], weights=bm.real_collisions(ev), minlength=br.N)
    assert (real >= plain["n_albedo"]).all() and real.sum() - plain["n_albedo"].sum() <= 2
    # the log is off again: the same calls give the same answers
    assert orc.trace_paths(L, 0, 64).tobytes() == plain[:64].tobytes()
    # the logged test value is the oracle's density at the logged coordinate (first 200 in-grid rows)
    if name != "sparse_small" and kernel == 2:
        res = ref.res
        inside = np.nonzero(bm.in_grid(ev, res))[0][:200]
        inv = np.float32(1) / (np.float32(m.scale) * np.float32(m.max_density))
        for i in inside:
            p = np.array([ev["cx"][i] / np.float32(res[0] - 1), ev["cy"][i] / np.float32(res[1] - 1),
                          ev["cz"][i] / np.float32(res[2] - 1)], np.float32)
            if not all(np.float32(p[k] * np.float32(res[k] - 1)) == ev[f][i] for k, f in enumerate(("cx", "cy", "cz"))):
                continue  # the division did not invert the product exactly
            tv = np.float32(np.float32(np.float32(m.scale) * np.float32(orc.density_at(p))) * inv)
            assert tv == ev["test_value"][i], i


# ------------------------------------------------- soundness of the proof ---
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("name", DENSE + SPARSE)
def test_bound_proof_holds_for_every_evaluation(name, fmt):
    """test value <= bound_value(code) for every in-grid evaluation, every brick size."""
    q4s = (0, 1) if name == "offgrid" else (0,)
    for q4 in q4s:
        ref = br.reference(name, fmt, q4)
        assert bm.in_grid(ref.evals, ref.res).sum() > 10000
        for opt in ((1, 2, 3) if name in SPARSE else (1, 2, 3, 4, 5)):
            table, bshift = br.codes(name, fmt, opt)
            bad = bm.unsound(ref.evals, ref.res, table, bshift)
            assert not bad.any(), f"{name} format {fmt} q4 {q4} B 2^{bshift}: {bad.sum()} unsound, first {np.nonzero(bad)[0][:5]}"
            # and a real collision is never bounded out
            assert (bm.fetch_flags(ref.evals, ref.res, table, bshift) | ~bm.real_collisions(ref.evals)).all()


def test_format_1_changes_the_tables():
    """The half-rounded media are other media: the format-1 cases check other walks, and on the
    sparse medium other codes (the staircase peaks are halves, or round to them)."""
    for name in ("staircase", "spikes", "sparse_small"):
        assert br.reference(name, 1).records.tobytes() != br.reference(name, 0).records.tobytes()
    assert (br.codes("sparse_small", 0, 1)[0] != br.codes("sparse_small", 1, 1)[0]).any()


# --------------------------------------------- conditions on the test inputs ---
def test_staircase_single_code_changes_show():
    ref = br.reference("staircase")
    table, bshift = br.codes("staircase", 0, 2)
    assert table.shape == (4, 5, 6) and len(np.unique(table)) >= 50
    base = bm.expected_fetches(ref.evals, ref.res, table, bshift)
    lower = bm.expected_fetches(ref.evals, ref.res, np.maximum(table - 1, 0), bshift)
    higher = bm.expected_fetches(ref.evals, ref.res, np.minimum(table + 1, 255), bshift)
    assert lower < base < higher
    total = unchanged = 0
    inside, x1, y1, z1 = bm.cell_index(ref.evals, ref.res)
    for idx in np.ndindex(table.shape):
        if table[idx] >= 255:
            continue
        # a brick's code decides only the evaluations in the brick: the model on those alone
        own = ref.evals[inside & (z1 >> bshift == idx[0]) & (y1 >> bshift == idx[1]) & (x1 >> bshift == idx[2])]
        for step in (-1, 1):
            t = table.copy()
            t[idx] = min(max(t[idx] + step, 0), 255)
            total += 1
            unchanged += bm.expected_fetches(own, ref.res, t, bshift) == bm.expected_fetches(own, ref.res, table, bshift)
    print(f"staircase: {base} fetches ({lower} / {higher} with every code -1 / +1), "
          f"{unchanged} of {total} single changes unchanged")
    assert total == 240 and unchanged <= 0.10 * total
    # every axis' one-cell-thick last brick is visited, and so are negative coordinates
    ev = ref.evals
    for f, n in zip(("cx", "cy", "cz"), ref.res):
        assert (bm.in_grid(ev, ref.res) & (ev[f] >= n - 1)).sum() > 1000
    assert ((ev["cx"] < 0) | (ev["cy"] < 0) | (ev["cz"] < 0)).sum() > 1000


def test_spikes_short_window_bounds_out_real_collisions():
    ref = br.reference("spikes")
    table, bshift = br.codes("spikes", 0, 2)
    short, _ = br.codes("spikes", 0, 2, True)
    assert (short <= table).all() and (short < table).any()
    lost = bm.real_collisions(ref.evals) & ~bm.fetch_flags(ref.evals, ref.res, short, bshift)
    print(f"spikes: the short window bounds out {lost.sum()} real collisions")
    assert lost.sum() >= 1
    assert bm.expected_fetches(ref.evals, ref.res, short, bshift) < bm.expected_fetches(ref.evals, ref.res, table, bshift)
    d = br.medium("spikes").density
    for x, y, z in media.SPIKES:
        assert d[z, y, x] == 1.0


def test_offgrid_leaves_the_grid_only_under_q4():
    ref = br.reference("offgrid")
    ev, res = ref.evals, ref.res
    off = ~bm.in_grid(ev, res)
    last = bm.in_grid(ev, res) & ((ev["cx"] >= res[0] - 1) | (ev["cy"] >= res[1] - 1) | (ev["cz"] >= res[2] - 1))
    print(f"offgrid: {len(ev)} evaluations, {off.sum()} off the grid, {last.sum()} in a last cell layer")
    assert off.sum() > 1000 and last.sum() > 1000
    fixed = br.reference("offgrid", 0, 1)
    assert bm.in_grid(fixed.evals, res).all()
    assert bm.expected_fetches(ev, res, None, None) == len(ev)  # bounds off: every evaluation fetches


def test_sparse_word_bounds_tell_a_full_mask():
    """sparse_es4: with the mask on, W_hi lies below the in-grid evaluations, so a mask with every bit
    set (every in-grid point loads its word) cannot pass; sparse_small has clear super-bricks too."""
    for name in SPARSE:
        m = br.medium(name)
        ref = br.reference(name)
        es, mask = bm.sparse_mask(m.table)
        for opt in (None, 1, 2):
            table, bshift = br.codes(name, 0, opt)
            f = bm.expected_fetches(ref.evals, ref.res, table, bshift)
            lo, hi, segs = bm.word_bounds(ref.evals, ref.records, ref.res, f, mask, es)
            lo_all, hi_all, _ = bm.word_bounds(ref.evals, ref.records, ref.res, f)
            inside = int(bm.in_grid(ref.evals, ref.res).sum())
            print(f"{name} bounds {opt}: fetches {f}, segments {segs}, W_lo {lo}, W_hi {hi}, in-grid {inside}")
            assert 0 < lo < lo_all == inside and hi < hi_all
            if name == "sparse_es4":
                assert hi < inside
                # one clear bit forced to 1 adds its super-brick's evaluations to W_lo: it shows
                # where those exceed the slack of the bounds
                _, x1, y1, z1 = bm.cell_index(ref.evals, ref.res)
                per_sb = np.zeros(mask.shape, np.int64)
                np.add.at(per_sb, (z1 >> es, y1 >> es, x1 >> es), 1)
                shown = [tuple(int(i) for i in idx) for idx in zip(*np.nonzero(~mask & (per_sb > hi - lo)))]
                print(f"sparse_es4 bounds {opt}: a forced bit shows in super-bricks (z, y, x) {shown}")
                assert len(shown) >= 2 and (3, 3, 4) in shown
