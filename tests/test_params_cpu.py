"""The parameter cases of tests/params.py on the CPU: pins of the oracle branches they reach, the
sharpness of every case and what each case covers.  No GPU; tests/test_gpu_params.py compares the
kernels with the oracle on the same cases.

a. Pins.  The fp32 oracle against fp64 numpy restatements of the reference's formulas (HG.h:46-63,
   GGX.h:13-38, :85-181, :213-326, CVRMath.h:58-91), written from the reference, on grids of a few
   thousand points.  Each test's docstring carries the largest error measured and asserts 4x that.
b. Sharpness.  Every case is traced (4 samples, seed 7, kernel ids 0 and 2) next to the parameter sets
   a plausible kernel bug would effectively render; at least 1 % of the paths must differ in flags,
   segment count or T bits.  A mutant that leaves a case's parameters unchanged does not apply to it
   (g := 0 at g = 0, the roughness mutants at ax == ay, R^T for the symmetric R of front and the
   pencils, the other world_to_aabb for the unit box, where both compute the same).
   Measured fractions of differing paths, kernel id 0 (id 2 within 0.3 points of it):
     default          eta:=1/eta 61.5 %
     g_pos            g:=0 36.9 %, g:=-g 38.2 %, eta:=1/eta 61.5 %
     g_neg            g:=0 13.4 %, g:=-g 14.7 %, eta:=1/eta 22.6 %, R^T 25.7 %
     aniso_a          ay:=ax 22.1 %, ax:=ay 23.3 %, swap 22.5 %, eta:=1/eta 23.2 %, R^T 26.6 %
     aniso_b          ay:=ax 63.5 %, ax:=ay 58.5 %, swap 63.5 %, eta:=1/eta 62.7 %
     eta_one          eta:=default 21.4 %, R^T 24.9 %
     eta_lt1          eta:=default 34.9 %, eta:=1/eta 32.0 %, R^T 6.1 %
     eta_big          eta:=default 63.3 %, eta:=1/eta 60.4 %
     inside           eta:=1/eta 5.1 %, R^T 95.5 %
     inside_all       ay:=ax 24.3 %, ax:=ay 24.3 %, swap 24.8 %, g:=0 74.4 %, g:=-g 75.1 %,
                      eta:=default 22.6 %, eta:=1/eta 23.1 %, R^T 98.6 %
     box_all          ay:=ax 17.1 %, ax:=ay 17.1 %, swap 17.2 %, g:=0 11.1 %, g:=-g 11.4 %,
                      eta:=1/eta 17.8 %, R^T 20.7 %, world_to_aabb 1 12.5 %
     box_all_w2a      ay:=ax 14.5 %, ax:=ay 14.6 %, swap 14.7 %, g:=0 9.0 %, g:=-g 9.3 %,
                      eta:=1/eta 15.8 %, R^T 18.6 %, world_to_aabb 0 12.5 %
     oblique_offset   eta:=1/eta 32.8 %, R^T 34.5 %, offset (0, 0) 82.8 %, r2v[1]:=r2v[0] 42.9 %
     pencil_in, pencil_negzero   eta:=1/eta 99.9 %;   pencil_x_inside   eta:=1/eta 2.8 %
   Two cameras are not the first ones tried: with the inside camera at (0.1, -0.05, 0.2) looking at
   (0.5, 0.4, -0.3) 8 % of the paths reached a boundary and eta:=1/eta changed 0.5 % of them
   (inside_all: 3.2 to 3.7 % for the roughness and eta mutants), and pencil_x_inside from (0, 0.1, 0.2)
   gave 0.3 %; both eyes were moved towards the box's faces (tests/params.py), the 1 % stayed.
   The four all-miss pencil cameras: every path of the case is a one-segment miss, and with the eye
   moved 1e-3 into the slab on the axes where it lies on a box plane (pencil_out: to x = 0.5 - 1e-3)
   every path hits.  One ulp into the slab does the same for pencil_face, pencil_edge and
   pencil_in_plane.
c. Coverage.  inside, inside_all and pencil_x_inside: every camera ray starts inside the box
   (oracle.aabb on oracle.camera_ray).  eta_lt1: 92.8 % of the paths that hit the box reflect at
   entry and leave (two segments, no Woodcock step), 0.1 % at eta = 1 (corner grazes).
   pencil_negzero: 1024 of 4096 rays have d.x = -0 and 1024 have d.y = -0, pencil_in none.  g_neg: the
   mean of cos(theta) over HG samples at g = -0.4 is +0.400, the reference's 2 |g| divisor mirrors a
   negative g."""
import numpy as np
import pytest

import params

TWOPI = float(np.float32(6.2831853071795864769))
PI = float(np.float32(3.14159265358979323846))
EPS = float(np.float32(0.00001))


def f32(x):
    return np.asarray(x, np.float32)


def unit_grid(n):
    """n points of (0, 1): the cell centres."""
    return f32((np.arange(n) + 0.5) / n)


def hemisphere(n_theta, n_phi, lo=0.02, hi=0.98):
    """Unit vectors (fp32 components) with theta over (lo, hi) * pi / 2 and phi over the circle,
    offset so that no component is 0."""
    th = (lo + (hi - lo) * (np.arange(n_theta) + 0.5) / n_theta) * np.pi / 2
    ph = 2 * np.pi * (np.arange(n_phi) + 0.37) / n_phi
    th, ph = np.meshgrid(th, ph, indexing="ij")
    v = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1).reshape(-1, 3)
    return f32(v)


# ------------------------------------------------- the reference's formulas in fp64 --
def ref_hg(v, g, e1, e2):
    """ImportanceSampleHG, HG.h:46-63 (generateLocalBasis :11-17, sphericalDirection :19-24)."""
    v = np.asarray(v, np.float64)
    g, e1, e2 = float(g), float(e1), float(e2)
    if abs(g) > EPS:
        sq = (1 - g * g) / (1 - g + 2 * g * e1)
        c = (1 + g * g - sq * sq) / (2 * abs(g))
    else:
        c = 1 - 2 * e1
    s = np.sqrt(max(0.0, 1 - c * c))
    phi = TWOPI * e2
    inv = 1 / np.sqrt(v[0] * v[0] + v[2] * v[2])
    v1 = np.array([v[2] * inv, 0.0, -v[0] * inv])
    v2 = np.cross(v, v1)
    return s * np.cos(phi) * v1 + s * np.sin(phi) * v2 + c * v


def ref_fresnel(eta, c):
    """fresnelDielectric, GGX.h:13-38 -> (F, ndotwt, ndotwt_sqr)."""
    eta, c = float(eta), float(c)
    if eta == 1:
        return 0.0, -c, 1.0
    scale = 1 / eta if c > 0 else eta
    t2 = 1 - (1 - c * c) * scale * scale
    if t2 <= 0:
        return 1.0, 0.0, t2
    a, b = abs(c), np.sqrt(t2)
    rs = (a - eta * b) / (a + eta * b)
    rp = (eta * a - b) / (eta * a + b)
    return 0.5 * (rs * rs + rp * rp), (-b if c > 0 else b), t2


def ref_project_roughness(v, ax, ay):
    """projectRoughness, GGX.h:213-225."""
    inv = 1 / (1 - v[2] * v[2])
    if ax == ay or inv <= 0:
        return ax
    return np.sqrt(v[0] * v[0] * inv * ax * ax + v[1] * v[1] * inv * ay * ay)


def ref_g1(ax, ay, v, m):
    """GGX_G1, GGX.h:227-255."""
    v = np.asarray(v, np.float64)
    m = np.asarray(m, np.float64)
    ax, ay = float(ax), float(ay)
    if np.dot(v, m) * v[2] <= 0:
        return 0.0
    t = 1 - v[2] * v[2]
    if t <= 0:
        return 0.0
    tan = abs(np.sqrt(t) / v[2])
    if tan == 0:
        return 1.0
    root = ref_project_roughness(v, ax, ay) * tan
    return 2 / (1 + np.sqrt(1 + root * root))


def ref_visible11(theta, sx, sy):
    """sampleVisible11, GGX.h:85-144 -> (slope x, slope y, |A|)."""
    phi = 2 * PI * sy
    if theta < 1e-4:
        r = np.sqrt(max(0.0, sx / (1 - sx)))
        return r * np.cos(phi), r * np.sin(phi), 0.0
    tan = np.tan(theta)
    a = 1 / tan
    a = 1 + 1 / (a * a)
    G1 = 2 / (1 + np.sqrt(a))
    A = 2 * sx / G1 - 1
    if abs(A) == 1:
        A -= np.copysign(1.0, A) * EPS
    tmp = 1 / (A * A - 1)
    B = tan
    D = np.sqrt(max(0.0, B * B * tmp * tmp - (A * A - B * B) * tmp))
    s1, s2 = B * tmp - D, B * tmp + D
    slx = s1 if (A < 0 or s2 > 1 / tan) else s2
    if sy > 0.5:
        S, sy = 1.0, 2 * (sy - 0.5)
    else:
        S, sy = -1.0, 2 * (0.5 - sy)
    c = [float(np.float32(k)) for k in (0.365728915865723, 0.790235037209296, 0.424965825137544,
                                        0.000152998850436920, 0.169507819808272, 0.397203533833404,
                                        0.232500544458471, 0.539825872510702)]
    z = ((sy * (sy * (sy * -c[0] + c[1]) - c[2]) + c[3])
         / (sy * (sy * (sy * (sy * c[4] - c[5]) - c[6]) + 1) - c[7]))
    return slx, S * z * np.sqrt(1 + slx * slx), abs(A)


def ref_vndf(wi, ax, ay, sx, sy):
    """mitsuba_GGX_sampleVNDF, GGX.h:146-181 -> (normal, stretched wi.z, theta, |A|)."""
    wi = np.asarray(wi, np.float64)
    ax, ay, sx, sy = float(ax), float(ay), float(sx), float(sy)
    w = np.array([ax * wi[0], ay * wi[1], wi[2]])
    w /= np.linalg.norm(w)
    theta = phi = 0.0
    if w[2] < float(np.float32(0.999999)):
        theta = np.arccos(w[2])
        phi = np.arctan2(w[1], w[0])
    sp, cp = np.sin(phi), np.cos(phi)
    slx, sly, A = ref_visible11(theta, sx, sy)
    rx = (cp * slx - sp * sly) * ax
    ry = (sp * slx + cp * sly) * ay
    n = 1 / np.sqrt(rx * rx + ry * ry + 1)
    return np.array([-rx * n, -ry * n, n]), w[2], theta, A


def ref_ggx_sample(rough, eta, wi, s):
    """GGX_sample, GGX.h:265-326 (reflect :40-43, refract :45-50) with the three draws s
    -> (ok, wo, weight, margins: the distances to the thresholds the fp32 code may take otherwise)."""
    wi = np.asarray(wi, np.float64)
    eta = float(eta)
    sign = wi[2] / abs(wi[2])
    wh, wz, theta, A = ref_vndf(sign * wi, rough[0], rough[1], s[0], s[1])
    c = float(np.dot(wh, wi))
    F, t, t2 = ref_fresnel(eta, c)
    # (the stretched wi.z decides between theta = 0 and theta >= 1.4e-3: 1e-5 of room is enough there)
    margins = [100 * abs(wz - 0.999999), abs(A - 1), abs(t2) if eta != 1 else 1.0,
               abs(float(s[2]) - F) if 0 < F < 1 else 1.0]
    if float(s[2]) <= F:
        wo = 2 * c * wh - wi
        if wi[2] * wo[2] <= 0:
            return False, wo, 0.0, margins
    else:
        if t == 0:
            return False, None, 0.0, margins
        e = 1 / eta if t < 0 else eta
        wo = wh * (c * e + t) - wi * e
        if wi[2] * wo[2] >= 0:
            return False, wo, 0.0, margins
    margins.append(abs(wi[2] * wo[2]))
    return True, wo, ref_g1(rough[0], rough[1], wo, wh), margins


def ref_frame(n):
    """Frame from its z axis, CVRMath.h:58-91: rows x, y, z."""
    z = np.asarray(n, np.float64)
    z = z / np.linalg.norm(z)
    tx = np.array([0.0, 1.0, 0.0]) if abs(z[0]) > float(np.float32(0.99)) else np.array([1.0, 0.0, 0.0])
    y = np.cross(z, tx)
    y /= np.linalg.norm(y)
    return np.stack([np.cross(y, z), y, z])


def all_roughness():
    pairs = set(params.ROUGHNESS) | {(b, a) for a, b in params.ROUGHNESS}
    return sorted((float(np.float32(a)), float(np.float32(b))) for a, b in pairs)


# --------------------------------------------------------------------- a. the pins --
def test_pin_hg(oracle_mod):
    """hg_sample against HG.h:46-63 at g in {-0.9, -0.4, 0.3, 0.6, 0.95}: 16 x 16 (e1, e2), 8 directions,
    10 240 points, none skipped.  Largest component error measured 1.81e-6 (at g = 0.95, where
    cos(theta) is near 1 and sin(theta) = sqrt(1 - cos^2) amplifies its rounding); bound 4x = 7.3e-6
    < 1e-4.  The reference's 2|g| divisor makes g < 0 the sample of -g at 1 - e1 (asserted on the fp64
    side); a 2g divisor would negate cos(theta)."""
    vs = hemisphere(2, 2, 0.2, 0.8)
    vs = np.concatenate([vs, vs * f32([1, -1, -1])])
    vs = f32(vs / np.linalg.norm(vs.astype(np.float64), axis=1)[:, None])
    assert len(vs) == 8 and (np.abs(vs[:, [0, 2]]).max(axis=1) > 0.1).all()  # none parallel to y
    worst = 0.0
    mirror = 0.0
    for g in f32([-0.9, -0.4, 0.3, 0.6, 0.95]):
        for v in vs:
            for e1 in unit_grid(16):
                for e2 in unit_grid(16):
                    got = oracle_mod.hg(v, g, e1, e2).astype(np.float64)
                    want = ref_hg(v, g, e1, e2)
                    worst = max(worst, np.abs(got - want).max())
                    if g < 0:  # e1 -> 1 - e1 in f32 moves the sample by some 1e-7
                        mirror = max(mirror, np.abs(want - ref_hg(v, -g, 1 - e1, e2)).max())
    print(f"hg: worst component error {worst:.3g}")
    assert worst <= 4 * 1.81e-6 < 1e-4
    assert mirror < 1e-6


def test_pin_fresnel(oracle_mod):
    """fresnel_dielectric against GGX.h:13-38 at eta in {1, f32(1/1.5), 1.33, 1.5}, 2001 cosines over
    [-1, 1], 8 004 points, 2 150 of them totally reflected (on entry for eta < 1, on exit for eta > 1);
    skipped: |ndotwt^2| < 1e-3 (1 point).  Largest relative error of F measured 3.54e-6, largest absolute
    error of ndotwt 6.4e-7; bounds 4x = 1.4e-5 and 2.6e-6, both < 1e-4.  eta == 1 is exact (F = 0,
    ndotwt = -ndotwi); total internal reflection returns exactly (1, 0)."""
    cs = f32(np.linspace(-1, 1, 2001))
    worst_f = worst_t = 0.0
    skipped = total = tir = 0
    for eta in (1.0, float(np.float32(1 / 1.5)), float(np.float32(1.33)), 1.5):
        for c in cs:
            F, t = oracle_mod.fresnel(eta, c)
            rF, rt, t2 = ref_fresnel(eta, c)
            total += 1
            if eta == 1.0:
                assert F == 0.0 and t == -float(c)
                continue
            if abs(t2) < 1e-3:
                skipped += 1
                continue
            if t2 <= 0:
                tir += 1
                assert (F, t) == (1.0, 0.0)
                continue
            worst_f = max(worst_f, abs(F - rF) / rF)
            worst_t = max(worst_t, abs(t - rt))
    print(f"fresnel: worst rel F {worst_f:.3g}, abs ndotwt {worst_t:.3g}, skipped {skipped}/{total}, TIR {tir}")
    assert tir > 500 and skipped < 0.02 * total
    assert worst_f <= 4 * 3.54e-6 < 1e-4
    assert worst_t <= 4 * 6.4e-7 < 1e-4


def test_pin_g1_and_projected_roughness(oracle_mod):
    """ggx_g1 (and through it project_roughness) against GGX.h:213-255: the roughness pairs of the
    cases and their swaps (10 pairs), v over 20 x 24 directions of each hemisphere with the facet
    normal (0, 0, 1), 9 600 points, none skipped.  Largest relative error measured 1.23e-7; bound 4x
    = 4.9e-7 < 1e-4.  Swapping ax and ay, or ax for both, moves the fp64 G1 of every anisotropic pair by
    more than 1e-2 somewhere on the grid (asserted): no room for either under the bound."""
    up = hemisphere(20, 24)
    worst = 0.0
    for ax, ay in all_roughness():
        swap = one = 0.0
        for sgn in (1.0, -1.0):
            m = f32([0, 0, 1])  # the facet normal lies in the upper hemisphere for either side
            for v in up * f32([1, 1, sgn]):
                got = oracle_mod.ggx_g1(ax, ay, v, m)
                want = ref_g1(ax, ay, v, m)
                assert want > 0
                worst = max(worst, abs(got - want) / want)
                swap = max(swap, abs(want - ref_g1(ay, ax, v, m)))
                one = max(one, abs(want - ref_g1(ax, ax, v, m)))
        if ax != ay:
            assert swap > 1e-2 and one > 1e-2, (ax, ay, swap, one)
        # wrong side of the facet: exactly 0
        assert oracle_mod.ggx_g1(ax, ay, up[5], f32([0, 0, -1])) == 0.0
        # v = n: 1 - v.z^2 <= 0 returns 0 before the "perpendicular incidence" branch can return 1
        assert oracle_mod.ggx_g1(ax, ay, f32([0, 0, 1]), f32([0, 0, 1])) == ref_g1(ax, ay, [0, 0, 1], [0, 0, 1]) == 0.0
    print(f"g1: worst relative error {worst:.3g}")
    assert worst <= 4 * 1.23e-7 < 1e-4


def _vndf_points():
    wis = hemisphere(6, 8, 0.0, 0.95)
    ss = unit_grid(6)
    for ax, ay in all_roughness():
        for wi in wis:
            for sx in ss:
                for sy in ss:
                    yield ax, ay, wi, sx, sy


def test_pin_vndf(oracle_mod):
    """ggx_sample_vndf against GGX.h:85-181: the 10 roughness pairs, 6 x 8 incoming directions, 6 x 6
    samples, 17 280 points; skipped: stretched wi.z within 1e-5 of 0.999999 (it decides between theta = 0
    and theta >= 1.4e-3, so theta is never near 1e-4; the small roughnesses put many directions within
    1e-3 of it) or |A| within 1e-3 of 1: none on this grid.  Largest component error measured 3.44e-6;
    bound 4x = 1.4e-5 < 1e-4.  (Near A = 0, which this grid does not hit, D is the root of a cancelling
    difference and errors reach 5e-5.)  ax used for both axes moves the normal by more than 1e-2
    (asserted)."""
    worst = 0.0
    skipped = total = 0
    one = 0.0
    for ax, ay, wi, sx, sy in _vndf_points():
        total += 1
        want, wz, theta, A = ref_vndf(wi, ax, ay, sx, sy)
        if abs(wz - 0.999999) < 1e-5 or abs(A - 1) < 1e-3:  # (theta is 0 or above 1.4e-3, never near 1e-4)
            skipped += 1
            continue
        got = oracle_mod.ggx_vndf(wi, ax, ay, sx, sy).astype(np.float64)
        worst = max(worst, np.abs(got - want).max())
        if ax != ay:
            one = max(one, np.abs(want - ref_vndf(wi, ax, ax, sx, sy)[0]).max())
    print(f"vndf: worst component error {worst:.3g}, skipped {skipped}/{total}")
    assert skipped < 0.02 * total
    assert one > 1e-2
    assert worst <= 4 * 3.44e-6 < 1e-4


def test_pin_ggx_sample(oracle_mod):
    """ggx_sample against GGX.h:265-326 with the oracle's own three draws (rng_stream): roughness and
    eta of every case, 24 incoming directions of each hemisphere, 8 seeds, 3 072 points; skipped within
    1e-3 of a threshold (those of the VNDF, ndotwt^2 near 0, the Fresnel draw near F, wi.z wo.z near 0):
    6 points (0.2 %).  The ok flags are equal everywhere else.  This is a composition, and worse
    conditioned than its parts: sampleVisible11's D is the root of a cancelling difference near A = 0
    (VNDF errors up to 5e-5 there on a 12 x 12 sample grid), and a refraction multiplies the error of
    wh . wi by eta^2 cos / |ndotwt| (up to 7 on this grid).  Largest error of a wo component measured
    1.2e-4, of the weight 1.31e-4 absolute; bounds 4x, capped at 1e-3 (a swapped roughness, the
    wrong side's eta or a missing |.| move both by 1e-2 or more).  Reflections and refractions occur on
    both sides of the surface for eta < 1 and eta > 1."""
    sets = sorted({(tuple(float(np.float32(r)) for r in params.medium_params(c)["roughness"]),
                    float(np.float32(params.medium_params(c)["eta"]))) for c in params.CASES.values()})
    up = hemisphere(4, 6, 0.05, 0.95)
    worst_wo = worst_w = 0.0
    skipped = total = 0
    kinds = set()
    for rough, eta in sets:
        for sgn in (1.0, -1.0):
            for i, wi in enumerate(up * f32([1, 1, sgn])):
                for seed in range(8):
                    sd = 1000 * i + seed
                    total += 1
                    _, s = oracle_mod.rng_stream(sd, 3)
                    rok, rwo, rw, margins = ref_ggx_sample(rough, eta, wi, s)
                    if min(margins) < 1e-3:
                        skipped += 1
                        continue
                    ok, wo, w = oracle_mod.ggx_sample(rough, eta, wi, sd)
                    assert ok == rok, (rough, eta, wi, sd)
                    if not ok:
                        assert w == 0.0
                        continue
                    kinds.add((sgn, "reflect" if wi[2] * rwo[2] > 0 else "refract", eta < 1))
                    worst_wo = max(worst_wo, np.abs(wo.astype(np.float64) - rwo).max())
                    worst_w = max(worst_w, abs(float(w) - rw))
    print(f"ggx_sample: worst wo {worst_wo:.3g}, weight {worst_w:.3g}, skipped {skipped}/{total}")
    assert len(kinds) == 8, kinds
    assert skipped < 0.02 * total
    assert worst_wo <= 4 * 1.2e-4 < 1e-3
    assert worst_w <= 4 * 1.31e-4 < 1e-3


def test_pin_frame(oracle_mod):
    """frame_from_z against CVRMath.h:58-91: the six box normals (exact) and 96 directions of both
    hemispheres, the |z.x| > 0.99 helper-axis switch among them.  Largest component error measured
    1.67e-7; bound 4x = 6.7e-7."""
    for n in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]):
        got = oracle_mod.frame(f32(n)).astype(np.float64)
        assert np.array_equal(got, ref_frame(n)), n
    vs = hemisphere(6, 8)
    vs = np.concatenate([vs, -vs, f32([[0.995, 0.06, 0.08], [-0.999, 0.03, -0.03], [0.98, 0.1, 0.17]])])
    worst = 0.0
    switched = 0
    for v in vs:
        nv = np.linalg.norm(v.astype(np.float64))
        if abs(abs(v[0] / nv) - 0.99) < 1e-3:
            continue
        switched += abs(v[0] / nv) > 0.99
        worst = max(worst, np.abs(oracle_mod.frame(v).astype(np.float64) - ref_frame(v)).max())
    print(f"frame: worst component error {worst:.3g}")
    assert switched >= 2
    assert worst <= 4 * 1.67e-7


# ------------------------------------------------------------------ b. sharpness --
def _trace(oracle_mod, case, kid, blob, cam=None, w2a=None, launch=None, **override):
    orc = params.make_oracle(oracle_mod, case, *blob, **override)
    L = launch if launch is not None else params.make_launch(oracle_mod, case, kid, cam, w2a)
    return orc.trace_paths(L, 0, params.n_paths(case))


def _differ(a, b):
    return ((a["flags"] != b["flags"]) | (a["n_segments"] != b["n_segments"])
            | (a["T"].view(np.uint32) != b["T"].view(np.uint32)).any(axis=1)).mean()


def _transposed(cam):
    M = cam.inv_view.reshape(3, 4).copy()
    M[:, :3] = M[:, :3].T.copy()
    return params.Camera(M.ravel(), cam.r2v)


def mutants(name):
    """(label, kwargs of _trace) of every mutant that changes the case's parameters."""
    case = params.CASES[name]
    p = params.medium_params(case)
    ax, ay = p["roughness"]
    out = []
    if ax != ay:
        out += [("ay:=ax", dict(roughness=(ax, ax))), ("ax:=ay", dict(roughness=(ay, ay))),
                ("swap", dict(roughness=(ay, ax)))]
    if p["g"] != 0:
        out += [("g:=0", dict(g=0.0)), ("g:=-g", dict(g=-p["g"]))]
    if p["eta"] != params.DEFAULT_ETA:
        out.append(("eta:=default", dict(eta=params.DEFAULT_ETA)))
    if p["eta"] != 1.0:
        out.append(("eta:=1/eta", dict(eta=float(np.float32(1) / np.float32(p["eta"])))))
    cam = params.camera(case.camera, case.full)
    t = _transposed(cam)
    if not np.array_equal(t.inv_view, cam.inv_view):
        out.append(("R^T", dict(cam=t)))
    if tuple(p["box_min"]) != params.DEFAULTS["box_min"]:
        out.append((f"world_to_aabb {1 - case.w2a}", dict(w2a=1 - case.w2a)))
    if case.offset != (0, 0):
        out.append(("offset (0, 0)", dict(launch="no_offset")))
        out.append(("r2v[1]:=r2v[0]", dict(cam=params.Camera(cam.inv_view, f32([cam.r2v[0], cam.r2v[0]])))))
    return out


@pytest.fixture(scope="module")
def blob():
    return params.blob16()


@pytest.mark.parametrize("name", [n for n in params.CASES if n not in params.ALL_MISS])
def test_case_is_sharp(oracle_mod, blob, name):
    case = params.CASES[name]
    ms = mutants(name)
    assert ms, name
    report = []
    for kid in (0, 2):
        base = _trace(oracle_mod, case, kid, blob)
        assert not np.isnan(base["T"]).any() and not (base["flags"] & 2).any()
        for label, kw in ms:
            kw = dict(kw)
            if kw.get("launch") == "no_offset":
                cam = params.camera(case.camera, case.full)
                kw["launch"] = oracle_mod.Oracle.launch(cam.inv_view, cam.r2v, case.full, case.tile, (0, 0), kid,
                                                        params.SEED, world_to_aabb=case.w2a)
            frac = _differ(base, _trace(oracle_mod, case, kid, blob, **kw))
            report.append(f"{label} k{kid} {100 * frac:.1f} %")
            assert frac >= 0.01, f"{name}: mutant {label} (kernel id {kid}) changes only {frac:.4f} of the paths"
    print(f"{name}: " + ", ".join(report))


def _moved_eye(name, step):
    """The pencil camera with its eye moved into the slab, by `step` (None: one ulp), on every axis
    where it lies on a box plane; pencil_out (on none): to 0.5 - step in x."""
    cam = params.camera(name)
    M = cam.inv_view.reshape(3, 4).copy()
    moved = 0
    for ax in range(3):
        e = M[ax, 3]
        if abs(e) == np.float32(0.5) and M[ax, 2] == 0:
            M[ax, 3] = np.nextafter(e, np.float32(0)) if step is None else e - np.sign(e) * np.float32(step)
            moved += 1
    if name == "pencil_out" and step is not None:
        M[0, 3] = np.float32(0.5) - np.float32(step)
        moved += 1
    return params.Camera(M.ravel(), cam.r2v) if moved else None


@pytest.mark.parametrize("name", params.ALL_MISS)
def test_all_miss_cameras_decide_hit_or_miss(oracle_mod, blob, name):
    """The case is the hit/miss decision: every path a one-segment miss with T = 1, and every path a
    hit once the eye is 1e-3 (and, on a plane, one ulp) inside the slab."""
    case = params.CASES[name]
    for kid in (0, 2):
        base = _trace(oracle_mod, case, kid, blob)
        assert (base["n_segments"] == 1).all() and (base["flags"] == 1).all() and (base["T"] == 1).all()
        for step in (1e-3, None):
            cam = _moved_eye(name, step)
            if cam is None:
                assert name == "pencil_out" and step is None
                continue
            hit = _trace(oracle_mod, case, kid, blob, cam=cam)
            # (a hit may end at its first segment, at the roulette after the boundary event: flags 0)
            assert ((hit["n_segments"] > 1) | (hit["flags"] == 0)).all(), (name, step)
            assert (hit["n_segments"] > 1).mean() > 0.9
            assert _differ(base, hit) == 1.0


# ------------------------------------------------------------------- c. coverage --
def _rays(oracle_mod, case):
    L = params.make_launch(oracle_mod, case, 0)
    return [oracle_mod.camera_ray(L, i) for i in range(params.n_paths(case))]


@pytest.mark.parametrize("name", ["inside", "inside_all", "pencil_x_inside"])
def test_inside_cases_start_inside(oracle_mod, blob, name):
    case = params.CASES[name]
    orc = params.make_oracle(oracle_mod, case, *blob)
    p = params.medium_params(case)
    for o, d in _rays(oracle_mod, case):
        assert (o > f32(p["box_min"])).all() and (o < f32(p["box_max"])).all()
        hit, out = orc.aabb(o, d)
        assert hit and out[4] == 1.0 and out[0] > 0  # leaving through the far plane: no entry event
    recs = _trace(oracle_mod, case, 2, blob)
    assert (recs["n_steps"] > 0).all()  # every path tracks from its first segment


def test_eta_lt1_reflects_at_entry(oracle_mod, blob):
    """eta < 1: total internal reflection on entry for cos < 0.745.  A path that hits the box and ends
    as two segments without a Woodcock step was turned back at the boundary."""
    def frac(name):
        r = _trace(oracle_mod, params.CASES[name], 2, blob)
        hits = r["n_segments"] > 1
        return (((r["n_segments"] == 2) & (r["n_steps"] == 0) & (r["flags"] == 1))[hits]).mean()
    lt1, default = frac("eta_lt1"), frac("eta_one")
    print(f"reflect at entry: eta_lt1 {lt1:.3f}, eta_one {default:.3f}")
    assert lt1 > 0.5 and default < 0.01
    F, t = oracle_mod.fresnel(params.CASES["eta_lt1"].params["eta"], 0.7)
    assert (F, t) == (1.0, 0.0)


def test_pencil_zero_signs(oracle_mod):
    """pencil_in's zero direction components are +0 for every path; pencil_negzero has -0 ones."""
    d_in = np.array([d for _, d in _rays(oracle_mod, params.CASES["pencil_in"])])
    d_nz = np.array([d for _, d in _rays(oracle_mod, params.CASES["pencil_negzero"])])
    for d in (d_in, d_nz):
        assert (d[:, :2] == 0).all() and (d[:, 2] == -1).all()
    assert not np.signbit(d_in[:, :2]).any()
    nx, ny = np.signbit(d_nz[:, 0]).sum(), np.signbit(d_nz[:, 1]).sum()
    print(f"pencil_negzero: d.x = -0 for {nx}, d.y = -0 for {ny} of {len(d_nz)}")
    assert nx > 100 and ny > 100


def test_negative_g_scatters_as_abs_g(oracle_mod):
    """HG.h:51 divides by 2 |g|: for g < 0 the sampled cos(theta) is that of |g| (the mean over e1 of
    the Henyey-Greenstein cosine is g; here it is +0.4 at g = -0.4)."""
    v = f32([0.6, 0.0, 0.8])
    for g, want in ((-0.4, 0.4), (0.4, 0.4), (-0.9, 0.9)):
        cos = [float(np.dot(oracle_mod.hg(v, g, e1, e2).astype(np.float64), v.astype(np.float64)))
               for e1 in unit_grid(64) for e2 in unit_grid(4)]
        mean = np.mean(cos)
        print(f"g = {g}: mean cos(theta) {mean:.4f}")
        assert abs(mean - want) < 5e-3
