"""The light volume and the shadowed preview restated in numpy from the text of include/cvr.h
(CVR_HAS_SHADOWS), independently of csrc/cvr_shadow.h: fp32 arrays over all nodes or pixels at once,
one operation per numpy call in the written order, so every intermediate is rounded as the text
says.  The ray, the chord, the trilinear and the exact fused multiply-add are features_ref's, the
dot product preview_ref's.

light_volume(...) -> S (z, y, x);  lookup(S, p, ...) -> (n,);  preview_shadowed(...) -> rgba (h, w, 4)."""
import numpy as np

from features_ref import chord, floor_i32, fma, lerp, minnum, rays, trilinear
from preview_ref import dot3

F = np.float32
_ERR = dict(invalid="ignore", divide="ignore", over="ignore", under="ignore")
UNSHADED = 1


def normalise(light):
    l = np.asarray(light, F)
    return (l / np.sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2])).astype(F)


def _medium(density, box_min, box_max, w2a, step):
    res = density.shape[::-1]
    bmin, bmax = np.asarray(box_min, F), np.asarray(box_max, F)
    e = bmax - bmin
    ag = np.array([r - 1 for r in res], F)
    shift, g = (bmin, ag / e) if w2a else (bmin / e, ag)
    h = (e / np.array(res, F)).astype(F)
    delta = F(step) * minnum(minnum(h[0], h[1]), h[2])

    def rho_at(p):
        cg = fma((p - shift).astype(F), g, F(0))
        return trilinear(lambda x, y, z: density[z, y, x], cg[:, 0], cg[:, 1], cg[:, 2], res)

    return res, bmin, bmax, e, ag, h, delta, rho_at


def light_volume(density, box_min, box_max, scale, sres, light, w2a=0, step=1.0, t_stop=1.0 / 256.0, max_steps=4096):
    density = np.asarray(density, F)
    res, bmin, bmax, e, ag, h, delta, rho_at = _medium(density, box_min, box_max, w2a, step)
    scale, t_stop = F(scale), F(t_stop)
    L = normalise(light)
    sx, sy, sz = (int(v) for v in sres)
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    idx = np.stack([i.ravel(), j.ravel(), k.ravel()], -1).astype(F)
    cell = (e / np.array([sx, sy, sz], F)).astype(F)
    p0 = (bmin + (idx + F(0.5)) * cell).astype(F)
    has, _, t1 = chord(p0, L, bmin, bmax)
    with np.errstate(**_ERR):
        q = np.ceil(t1 / delta).astype(F)
        n = np.where(q < F(max_steps), np.where(q > 0, q, 0), max_steps)
    n = np.where(has, n, 0).astype(np.int64)
    T = np.ones(p0.shape[0], F)
    live = n > 0
    for s_i in range(int(n.max(initial=0))):
        live &= s_i < n
        t = (F(s_i) + F(0.5)) * delta
        with np.errstate(**_ERR):
            live &= t < t1
        if not live.any():
            break
        kk = np.nonzero(live)[0]
        p = (p0[kk] + (t * L)[None, :]).astype(F)
        rho = rho_at(p)
        with np.errstate(**_ERR):
            s = (scale * rho) * delta
            hit = s > 0
        kh, sh = kk[hit], s[hit]
        if kh.size:
            T[kh] = T[kh] - T[kh] * (sh / (F(1) + sh))
            live[kh[T[kh] < t_stop]] = False
    return T.reshape(sz, sy, sx)


def lookup(S, p, bmin, e):
    """The volume's trilinear value at the world points p (n, 3)."""
    S = np.asarray(S, F)
    sres = S.shape[::-1]
    u = (((p - bmin) / e) * np.array(sres, F) - F(0.5)).astype(F)
    i1 = [floor_i32(u[:, a]) for a in range(3)]
    f = [(u[:, a] - i1[a].astype(F)).astype(F) for a in range(3)]
    fi = [(F(1) - v).astype(F) for v in f]
    lo = [np.clip(i1[a], 0, sres[a] - 1) for a in range(3)]
    hi = [np.clip(i1[a] + 1, 0, sres[a] - 1) for a in range(3)]
    (xa, ya, za), (xb, yb, zb) = lo, hi
    a = lerp(lerp(S[za, ya, xa], S[za, ya, xb], f[0], fi[0]), lerp(S[za, yb, xa], S[za, yb, xb], f[0], fi[0]), f[1], fi[1])
    b = lerp(lerp(S[zb, ya, xa], S[zb, ya, xb], f[0], fi[0]), lerp(S[zb, yb, xa], S[zb, yb, xb], f[0], fi[0]), f[1], fi[1])
    return lerp(a, b, f[2], fi[2])


def preview_shadowed(density, albedo, box_min, box_max, scale, max_density, inv_view, r2v, full, tile, volume, vol_light,
                     shadow, offset=(0, 0), w2a=0, step=1.0, t_stop=1.0 / 256.0, max_steps=4096, ambient=0.3, diffuse=0.7,
                     specular=0.2, shininess_log2=4, knee=0.05, background=(0, 0, 0), flags=0):
    density = np.asarray(density, F)
    albedo = np.asarray(albedo, F)
    res, bmin, bmax, e, ag, h, delta, rho_at = _medium(density, box_min, box_max, w2a, step)
    hmin = minnum(minnum(h[0], h[1]), h[2])
    scale, t_stop, shadow = F(scale), F(t_stop), F(shadow)
    ambient, diffuse, specular = F(ambient), F(diffuse), F(specular)
    knee_abs = F(knee) * (F(max_density) / hmin)
    bg = np.asarray(background, F)
    shaded = not flags & UNSHADED
    L_fixed = normalise(vol_light)

    o, d = rays(inv_view, r2v, full, tile, offset)
    n_px = d.shape[0]
    has, t0, t1 = chord(o, d, bmin, bmax)
    with np.errstate(**_ERR):
        q = np.ceil((t1 - t0) / delta).astype(F)
        n = np.where(q < F(max_steps), np.where(q > 0, q, 0), max_steps)
    n = np.where(has, n, 0).astype(np.int64)

    T = np.ones(n_px, F)
    Cc = np.zeros((n_px, 3), F)
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
        p = (o + t[k][:, None] * d[k]).astype(F)
        rho = rho_at(p)
        with np.errstate(**_ERR):
            s = (scale * rho) * delta
            hit = s > 0
        kh, sh, ph = k[hit], s[hit], p[hit]
        if not kh.size:
            continue
        a = sh / (F(1) + sh)
        w = T[kh] * a
        ca = ((ph - bmin) / e) * ag
        c = trilinear(lambda x, y, z: albedo[z, y, x, :3], ca[:, 0], ca[:, 1], ca[:, 2], res).astype(F)
        V = (F(1) - shadow * (F(1) - lookup(volume, ph, bmin, e))).astype(F)
        em = (V[:, None] * c).astype(F)
        if shaded:
            G = np.zeros_like(ph)
            for ax in range(3):
                up, dn = ph.copy(), ph.copy()
                up[:, ax] = ph[:, ax] + h[ax]
                dn[:, ax] = ph[:, ax] - h[ax]
                G[:, ax] = (rho_at(up) - rho_at(dn)) / h[ax]
            with np.errstate(**_ERR):
                m = np.sqrt(dot3(G, G)).astype(F)
                lit = m > 0
            if lit.any():
                Gl, ml, cl, Vl = G[lit], m[lit], c[lit], V[lit]
                nrm = (Gl / ml[:, None]).astype(F)
                view = (-d[kh][lit]).astype(F)
                Ld = np.broadcast_to(L_fixed, view.shape)
                nl = -dot3(nrm, Ld)
                nl = np.where(nl > 0, nl, F(0)).astype(F)
                sp = np.zeros_like(nl)
                if specular > 0:
                    H = (Ld + view).astype(F)
                    with np.errstate(**_ERR):
                        hh = np.sqrt(dot3(H, H)).astype(F)
                        nh = -dot3(nrm, H) / hh
                    nh = np.where(nh > 0, nh, F(0)).astype(F)
                    for _ in range(int(shininess_log2)):
                        nh = nh * nh
                    sp = np.where(hh > 0, nh, F(0)).astype(F)
                f = ambient + (diffuse * nl) * Vl
                litc = f[:, None] * cl + ((specular * sp) * Vl)[:, None]
                qq = ml / (ml + knee_abs)
                em[lit] = (F(1) - qq)[:, None] * (Vl[:, None] * cl) + qq[:, None] * litc
        Cc[kh] += w[:, None] * em
        W[kh] += w
        T[kh] = T[kh] - w
        live[kh[T[kh] < t_stop]] = False
    rgba = np.zeros((n_px, 4), F)
    rgba[:, :3] = Cc + T[:, None] * bg
    rgba[:, 3] = W
    rgba[~has, :3] = bg
    rgba[~has, 3] = 0
    return rgba.reshape(tile[1], tile[0], 4)
