"""The primary-ray feature pass restated in numpy from the text of include/cvr.h (CVR_HAS_FEATURES),
independently of csrc/cvr_features.h: fp32 arrays over all pixels at once, one operation per numpy
call in the written order, so every intermediate is rounded as the text says.  numpy has no fused
multiply-add; fma() below builds the correctly rounded one from fp64 operations (exact product,
error-free sum, round to odd, one final rounding), so the restatement can state every operation of
the text and is compared bit for bit.

features(...) -> (feat_rgba (h, w, 4), feat_depth (h, w)).  density_at: an optional function taking
the (n, 3) fp32 density coordinates c = p - shift and returning n densities, used instead of the
restatement's own trilinear (the tie to oracle.density_at).

features_fetch(res, density, albedo, ...) is the same march over two fetch functions
density(x, y, z) -> (n,) and albedo(x, y, z) -> (n, 3) of clamped integer voxel indices (int64
arrays), for media that cannot be held as a dense array: features() is features_fetch over
array_fetch, and leaf_fetch reads a sparse medium's leaf table and pools.  taps: an optional list
that receives, per density sample of the march, the (n, 3) int32 integer corners (x1, y1, z1) of
the sampled points before the texel clamp."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

F = np.float32
NO_LEAF = 0xFFFFFFFF
_ERR = dict(invalid="ignore", divide="ignore", over="ignore", under="ignore")


def fma(a, b, c):
    """fp32 fma(a, b, c), correctly rounded.  a * b is exact in fp64 (48 bits); x + c is computed
    with its exact error (TwoSum), the fp64 sum is moved to the neighbour with an odd last bit when
    it was inexact (round to odd), and rounding that to fp32 rounds the exact value once."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    with np.errstate(**_ERR):
        x = a.astype(np.float64) * b.astype(np.float64)
        y = c.astype(np.float64)
        s = x + y
        bb = s - x
        err = (x - (s - bb)) + (y - bb)
        odd = np.nonzero(err != 0)  # few: a lerp's two terms are of like size
        if odd[0].size:
            so, eo = s[odd], err[odd]
            fix = np.isfinite(so) & np.isfinite(eo) & ((so.view(np.int64) & 1) == 0)
            s[odd] = np.where(fix, np.nextafter(so, np.where(eo > 0, np.inf, -np.inf)), so)
        return s.astype(F)


def minnum(a, b):
    """det_fminf: a NaN first operand gives the second, a NaN second the first; else the smaller."""
    with np.errstate(**_ERR):
        return np.where(a != a, b, np.where(b < a, b, a)).astype(F)


def maxnum(a, b):
    with np.errstate(**_ERR):
        return np.where(a != a, b, np.where(b > a, b, a)).astype(F)


def floor_i32(x):
    """(int)floor(x), saturating, NaN -> INT_MIN."""
    with np.errstate(**_ERR):
        f = minnum(maxnum(np.floor(x).astype(F), F(-2147483648.0)), F(2147483520.0))
    return f.astype(np.int64)


def texel(i, res):
    """The clamp of the reference's point-sampled texture: the int index goes through uint32."""
    u = i & 0xFFFFFFFF
    return np.where(u < res - 1, u, res - 1)


def lerp(a, b, f, fi):
    return fma(b, f, (a * fi).astype(F))


def trilinear(fetch, cx, cy, cz, res, taps=None):
    """fetch(x, y, z) -> (n,) or (n, k) values; coordinates (n,) fp32; res (rx, ry, rz); taps: a
    list that receives the (n, 3) int32 lower corners."""
    x1, y1, z1 = floor_i32(cx), floor_i32(cy), floor_i32(cz)
    if taps is not None:
        taps.append(np.stack([x1, y1, z1], axis=1).astype(np.int32))
    with np.errstate(**_ERR):
        fx, fy, fz = cx - x1.astype(F), cy - y1.astype(F), cz - z1.astype(F)
        _fx, _fy, _fz = F(1) - fx, F(1) - fy, F(1) - fz
    xa, xb = texel(x1, res[0]), texel(x1 + 1, res[0])
    ya, yb = texel(y1, res[1]), texel(y1 + 1, res[1])
    za, zb = texel(z1, res[2]), texel(z1 + 1, res[2])
    d000, d001, d010, d011 = fetch(xa, ya, za), fetch(xb, ya, za), fetch(xa, yb, za), fetch(xb, yb, za)
    d100, d101, d110, d111 = fetch(xa, ya, zb), fetch(xb, ya, zb), fetch(xa, yb, zb), fetch(xb, yb, zb)
    if d000.ndim == 2:
        fx, fy, fz, _fx, _fy, _fz = (v[:, None] for v in (fx, fy, fz, _fx, _fy, _fz))
    with np.errstate(**_ERR):
        a = lerp(lerp(d000, d001, fx, _fx), lerp(d010, d011, fx, _fx), fy, _fy)
        b = lerp(lerp(d100, d101, fx, _fx), lerp(d110, d111, fx, _fx), fy, _fy)
        return lerp(a, b, fz, _fz)


def rays(inv_view, r2v, full, tile, offset):
    """Pixel-centre rays of the tile, row-major: o (3,), d (n, 3)."""
    M = np.asarray(inv_view, F).reshape(3, 4)
    w, h = tile
    ix, iy = np.meshgrid(np.arange(w), np.arange(h))
    px = ix.ravel().astype(F) + F(offset[0])
    py = iy.ravel().astype(F) + F(offset[1])
    rx = F(r2v[0]) * (((px + F(0.5)) * F(2)) / F(full[0]) - F(1))
    ry = F(r2v[1]) * (((py + F(0.5)) * F(2)) / F(full[1]) - F(1))
    inv = F(1) / np.sqrt((rx * rx + ry * ry) + F(1) * F(1))
    v = np.stack([rx * inv, ry * inv, F(1) * inv], -1)
    o = np.array([F(0) * M[a, 0] + F(0) * M[a, 1] + F(0) * M[a, 2] + F(1) * M[a, 3] for a in range(3)], F)
    d = np.stack([(v[:, 0] * M[a, 0] + v[:, 1] * M[a, 1]) + v[:, 2] * M[a, 2] for a in range(3)], -1)
    return o, d.astype(F)


def chord(o, d, bmin, bmax):
    """-> (has (n,) bool, t0, t1)."""
    with np.errstate(**_ERR):
        i = F(1) / d
        tbot = i * (bmin - o)
        ttop = i * (bmax - o)
        lo, hi = minnum(ttop, tbot), maxnum(ttop, tbot)
        enter = maxnum(maxnum(lo[:, 0], lo[:, 1]), maxnum(lo[:, 0], lo[:, 2]))
        t1 = minnum(minnum(hi[:, 0], hi[:, 1]), minnum(hi[:, 0], hi[:, 2]))
        t0 = np.where(enter > 0, enter, F(0)).astype(F)
        return (t1 > enter) & (t1 > t0), t0, t1


def array_fetch(density, albedo):
    """(res, density fetch, albedo fetch) over a dense medium's arrays (z, y, x) and (z, y, x, 4)."""
    density = np.asarray(density, F)
    albedo = np.asarray(albedo, F)
    return density.shape[::-1], (lambda x, y, z: density[z, y, x]), (lambda x, y, z: albedo[z, y, x, :3])


def leaf_fetch(res, table, leaf_density, leaf_albedo, albedo_bg):
    """(density fetch, albedo fetch) over a sparse medium (cvr_sparse_medium_desc: table (lz, ly, lx)
    of pool slots or NO_LEAF, pools (n, 512) and (n, 512, 4) or None, a voxel of leaf (x >> 3, y >> 3,
    z >> 3) at (z & 7) 64 + (y & 7) 8 + (x & 7)): where the table holds NO_LEAF the density is 0 and
    the albedo the background, which it is everywhere without an albedo pool."""
    table = np.asarray(table)
    bg = np.asarray(albedo_bg, F)[:3]
    assert table.shape == tuple((r + 7) // 8 for r in res[::-1])

    def at(x, y, z):
        slot = table[z >> 3, y >> 3, x >> 3]
        have = slot != NO_LEAF
        return slot[have].astype(np.int64), (((z & 7) << 6) | ((y & 7) << 3) | (x & 7))[have], have

    def density(x, y, z):
        slot, local, have = at(x, y, z)
        out = np.zeros(x.shape, F)
        out[have] = leaf_density[slot, local]
        return out

    def albedo(x, y, z):
        out = np.empty(x.shape + (3,), F)
        out[:] = bg
        if leaf_albedo is not None:
            slot, local, have = at(x, y, z)
            out[have] = leaf_albedo[slot, local, :3]
        return out

    return density, albedo


def leaf_support(table):
    """The cells (lo (3), hi (3), inclusive, x y z) outside of which a leaf table's density is +0:
    the bounding box of its leaves."""
    z, y, x = np.nonzero(np.asarray(table) != NO_LEAF)
    lo = np.array([x.min(), y.min(), z.min()], np.int64) * 8
    hi = np.array([x.max(), y.max(), z.max()], np.int64) * 8 + 7
    return lo, hi


def support_skip(support, res, shift, g):
    """-> skip(p): for points p (n, 3), six conditions (n, 6) of which any one says that the point
    needs no density sample, because all 8 taps lie outside `support` (leaf_support's box), where
    the density is +0: the sample's s is 0 and the march passes it by.  Per axis: the coordinate c
    lies below the box, or above it.  Judged on the grid coordinate in fp64 with a margin m of
    8 cells + 2^-19 max(|c|, g): the fp32 point and coordinate are sums and differences of numbers
    below 2, each rounded to 2^-24, times g, so within 2^-22 g of the exact ray's.  Never for a
    coordinate within m of 0 or below it (a negative index clamps to the last voxel, quirk Q5), and
    above the box only where its top is not the grid's last voxel (indices past the grid clamp to
    it).  c - m and c + m grow with c, so along a ray each condition holds on one interval: one
    that holds at both ends of a stretch holds throughout."""
    lo, hi = (np.asarray(v, np.float64) for v in support)
    shift64, g64 = np.asarray(shift, np.float64), np.asarray(g, np.float64)
    open_top = hi < np.array(res, np.float64) - 1

    def skip(p):
        c = (p.astype(np.float64) - shift64) * g64
        m = 8 + np.maximum(np.abs(c), g64) * 2.0 ** -19
        below = (c > m) & (c < lo - 1 - m)
        above = open_top & (c > hi + 1 + m)
        return np.concatenate([below, above], axis=1)

    return skip


def _in_chunks(fn, arrays, log, chunk=1 << 14):
    """fn(*arrays, log) over rows in chunks on a few threads (the rows are independent; numpy releases
    the interpreter lock): the same values and log rows in the same order."""
    n = arrays[0].shape[0]
    if n <= chunk:
        return fn(*arrays, log)

    def one(i):
        part = []
        return fn(*(a[i:i + chunk] for a in arrays), part), part

    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        parts = list(pool.map(one, range(0, n, chunk)))
    log.extend(np.concatenate(rows) for rows in zip(*(part for _, part in parts)))
    return np.concatenate([v for v, _ in parts])


def march(o, d, n, t0, t1, delta, scale, t_stop, density, payload, n_acc, skip=None, taps=None, block=128):
    """The march's loop over all pixels, `block` steps at a time.  What a sample adds does not depend
    on the ray's state, so a block's samples are evaluated at once: density(p, log) -> rho (m,) for
    points p (m, 3), and for those with s = (scale rho) delta > 0, payload(k, t, p, log) -> (m, n_acc)
    for pixel indices k, distances t and points p.  Then the pixels take their samples in step order:
    w = T a, acc += w payload, W += w, T = T - w, the march of a pixel ending with T < t_stop.
    log: a list the two append (n, 3) tap arrays to, one row per point.  Samples that skip(p) names
    are passed by.  taps receives the logged rows of the samples the march really takes (none after
    a pixel's end).  -> (acc (n_px, n_acc), W, T)."""
    n_px = d.shape[0]
    T = np.ones(n_px, F)
    acc = np.zeros((n_px, n_acc), F)
    W = np.zeros(n_px, F)
    alive = n > 0
    n_max = int(n.max(initial=0))
    for i0 in range(0, n_max, block):
        ka = np.nonzero(alive)[0]
        if not ka.size:
            break
        steps = np.arange(i0, min(i0 + block, n_max))
        with np.errstate(**_ERR):
            t = t0[ka, None] + (steps[None, :].astype(F) + F(0.5)) * delta
            valid = (steps[None, :] < n[ka, None]) & (t < t1[ka, None])
        last = ka[~valid[:, -1]]  # t does not decrease: every later sample of these is dropped too
        if skip is not None:  # pixels that pass the whole block by: one condition at both of its ends
            ends = [(o + t[:, j][:, None] * d[ka]).astype(F) for j in (0, -1)]
            valid[(skip(ends[0]) & skip(ends[1])).any(axis=1)] = False
        pi, si = np.nonzero(valid)
        k, tk, si = ka[pi], t[pi, si], steps[si]
        p = (o + tk[:, None] * d[k]).astype(F)
        if skip is not None:
            keep = ~skip(p).any(axis=1)
            k, tk, si, p = k[keep], tk[keep], si[keep], p[keep]
        if not k.size:
            alive[last] = False
            continue
        log_d, log_p = [], []
        rho = _in_chunks(density, (p,), log_d)
        with np.errstate(**_ERR):
            s = (scale * rho) * delta
            hit = s > 0
        kh, sh, th, sih = k[hit], s[hit], tk[hit], si[hit]
        end = np.full(n_px, n_max, np.int64)  # the step with which a pixel's march ends
        if kh.size:
            a = sh / (F(1) + sh)
            pay = _in_chunks(payload, (kh, th, p[hit]), log_p)
            order = np.argsort(sih, kind="stable")
            cuts = np.nonzero(np.diff(sih[order]))[0] + 1
            for sel in np.split(order, cuts):
                sel = sel[alive[kh[sel]]]
                kk = kh[sel]
                w = T[kk] * a[sel]
                acc[kk] += w[:, None] * pay[sel]
                W[kk] += w
                T[kk] = T[kk] - w
                done = kk[T[kk] < t_stop]
                alive[done] = False
                end[done] = sih[sel[0]] if sel.size else 0
        alive[last] = False
        if taps is not None:
            taps.extend(rows[si <= end[k]] for rows in log_d)
            taps.extend(rows[sih <= end[kh]] for rows in log_p)
    return acc, W, T


def features(density, albedo, box_min, box_max, scale, inv_view, r2v, full, tile, offset=(0, 0), w2a=0, step=1.0,
             t_stop=1.0 / 256.0, max_steps=4096, density_at=None, taps=None):
    """The march over a dense medium's arrays: features_fetch over array_fetch."""
    res, dens, alb = array_fetch(density, albedo)
    return features_fetch(res, dens, alb, box_min, box_max, scale, inv_view, r2v, full, tile, offset, w2a, step, t_stop,
                          max_steps, density_at, taps)


def features_fetch(res, density, albedo, box_min, box_max, scale, inv_view, r2v, full, tile, offset=(0, 0), w2a=0,
                   step=1.0, t_stop=1.0 / 256.0, max_steps=4096, density_at=None, taps=None, support=None, sums=None):
    """support: leaf_support's box, outside of which density() is +0 (support_skip).  sums: a dict
    that receives the march's per-pixel sums A (n, 3) = sum of w c, W, the final T and `has` (a
    chord): the unshaded preview composites exactly these (preview_ref.unshaded_from)."""
    res = tuple(int(r) for r in res)
    fres = np.array(res, F)
    bmin, bmax = np.asarray(box_min, F), np.asarray(box_max, F)
    e = bmax - bmin
    ag = np.array([r - 1 for r in res], F)
    shift, g = (bmin, ag / e) if w2a else (bmin / e, ag)
    cell = e / fres
    delta = F(step) * minnum(minnum(cell[0], cell[1]), cell[2])
    diag = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    scale, t_stop = F(scale), F(t_stop)

    o, d = rays(inv_view, r2v, full, tile, offset)
    n_px = d.shape[0]
    has, t0, t1 = chord(o, d, bmin, bmax)
    with np.errstate(**_ERR):
        q = np.ceil((t1 - t0) / delta).astype(F)
        n = np.where(q < F(max_steps), np.where(q > 0, q, 0), max_steps)
    n = np.where(has, n, 0).astype(np.int64)

    def rho_at(p, log):
        c = p - shift
        if density_at is not None:
            return np.asarray(density_at(c), F)
        cg = fma(c, g, F(0))
        return trilinear(density, cg[:, 0], cg[:, 1], cg[:, 2], res, log)

    def colour_and_t(k, t, p, log):
        ca = ((p - bmin) / e) * ag
        col = trilinear(albedo, ca[:, 0], ca[:, 1], ca[:, 2], res)
        return np.concatenate([col, t[:, None]], axis=1).astype(F)

    skip = None if support is None else support_skip(support, res, shift, g)
    acc, W, T = march(o, d, n, t0, t1, delta, scale, t_stop, rho_at, colour_and_t, 4, skip, taps)
    A, Z = acc[:, :3], acc[:, 3]
    if sums is not None:
        sums.update(A=A.copy(), W=W.copy(), T=T, has=has, tile=tuple(tile))
    rgba = np.zeros((n_px, 4), F)
    depth = np.zeros(n_px, F)
    nz = W != 0
    rgba[nz, :3] = A[nz] / W[nz, None]
    rgba[nz, 3] = W[nz]
    depth[nz] = (Z[nz] / W[nz]) / diag
    return rgba.reshape(tile[1], tile[0], 4), depth.reshape(tile[1], tile[0])
