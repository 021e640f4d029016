"""The primary-ray feature pass restated in numpy from the text of include/cvr.h (CVR_HAS_FEATURES),
independently of csrc/cvr_features.h: fp32 arrays over all pixels at once, one operation per numpy
call in the written order, so every intermediate is rounded as the text says.  numpy has no fused
multiply-add; fma() below builds the correctly rounded one from fp64 operations (exact product,
error-free sum, round to odd, one final rounding), so the restatement can state every operation of
the text and is compared bit for bit.

features(...) -> (feat_rgba (h, w, 4), feat_depth (h, w)).  density_at: an optional function taking
the (n, 3) fp32 density coordinates c = p - shift and returning n densities, used instead of the
restatement's own trilinear (the tie to oracle.density_at)."""
import numpy as np

F = np.float32
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
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
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


def trilinear(fetch, cx, cy, cz, res):
    """fetch(x, y, z) -> (n,) or (n, k) values; coordinates (n,) fp32; res (rx, ry, rz)."""
    x1, y1, z1 = floor_i32(cx), floor_i32(cy), floor_i32(cz)
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


def features(density, albedo, box_min, box_max, scale, inv_view, r2v, full, tile, offset=(0, 0), w2a=0, step=1.0,
             t_stop=1.0 / 256.0, max_steps=4096, density_at=None):
    density = np.asarray(density, F)
    albedo = np.asarray(albedo, F)
    res = density.shape[::-1]
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

    T = np.ones(n_px, F)
    A = np.zeros((n_px, 3), F)
    Z = np.zeros(n_px, F)
    W = np.zeros(n_px, F)
    live = n > 0
    for i in range(int(n.max(initial=0))):
        live &= i < n
        t = t0 + (F(i) + F(0.5)) * delta
        with np.errstate(**_ERR):
            live &= t < t1
        if not live.any():
            break
        k = np.nonzero(live)[0]
        tk = t[k]
        p = (o + tk[:, None] * d[k]).astype(F)
        c = p - shift
        if density_at is None:
            cg = fma(c, g, F(0))
            rho = trilinear(lambda x, y, z: density[z, y, x], cg[:, 0], cg[:, 1], cg[:, 2], res)
        else:
            rho = np.asarray(density_at(c), F)
        with np.errstate(**_ERR):
            s = (scale * rho) * delta
            hit = s > 0
        kh, sh, th = k[hit], s[hit], tk[hit]
        if kh.size:
            a = sh / (F(1) + sh)
            w = T[kh] * a
            ca = ((p[hit] - bmin) / e) * ag
            col = trilinear(lambda x, y, z: albedo[z, y, x, :3], ca[:, 0], ca[:, 1], ca[:, 2], res)
            A[kh] += w[:, None] * col
            Z[kh] += w * th
            W[kh] += w
            T[kh] = T[kh] - w
            live[kh[T[kh] < t_stop]] = False
    rgba = np.zeros((n_px, 4), F)
    depth = np.zeros(n_px, F)
    nz = W != 0
    rgba[nz, :3] = A[nz] / W[nz, None]
    rgba[nz, 3] = W[nz]
    depth[nz] = (Z[nz] / W[nz]) / diag
    return rgba.reshape(tile[1], tile[0], 4), depth.reshape(tile[1], tile[0])
