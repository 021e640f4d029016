"""The field projections restated in numpy from the text of include/cvr.h (CVR_HAS_FIELD_PROJECT),
independently of csrc/cvr_project.h: fp32 arrays over all pixels at once, one operation per numpy
call in the written order, so every intermediate is rounded as the text says.  The ray, the chord,
the trilinear and the exact fused multiply-add are features_ref's (the restatement of
CVR_HAS_FEATURES, which the text refers to for them).

project(field (z, y, x), mode, ...) -> (rgba (h, w, 4), value (h, w), depth (h, w))."""
import numpy as np

from features_ref import chord, minnum, rays, trilinear

F = np.float32
_ERR = dict(invalid="ignore", divide="ignore", over="ignore", under="ignore")
MAX, MIN, MEAN, ISO = 0, 1, 2, 3
HEADLIGHT = 1


def dot3(a, b):
    """(a_x b_x + a_y b_y) + a_z b_z over the last axis."""
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


def project(field, mode, box_min, box_max, inv_view, r2v, full, tile, offset=(0, 0), step=1.0, max_steps=4096, lo=0.0,
            hi=1.0, iso=0.5, refine=4, light=(0, 0, 0), ambient=0.3, diffuse=0.7, specular=0.2, shininess_log2=4,
            colour=(1, 1, 1), background=(0, 0, 0), flags=HEADLIGHT):
    field = np.asarray(field)
    res = field.shape[::-1]
    fres = np.array(res, F)
    bmin, bmax = np.asarray(box_min, F), np.asarray(box_max, F)
    e = bmax - bmin
    ag = np.array([r - 1 for r in res], F)
    h = (e / fres).astype(F)
    delta = F(step) * minnum(minnum(h[0], h[1]), h[2])
    diag = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    lo, hi, iso = F(lo), F(hi), F(iso)
    ambient, diffuse, specular = F(ambient), F(diffuse), F(specular)
    colour, bg = np.asarray(colour, F), np.asarray(background, F)

    def S(p):
        with np.errstate(**_ERR):
            c = (((p - bmin) / e) * ag).astype(F)
            return trilinear(lambda x, y, z: field[z, y, x].astype(F), c[:, 0], c[:, 1], c[:, 2], res)

    def at(o, t, d):
        with np.errstate(**_ERR):
            return (o + t[:, None] * d).astype(F)

    o, d = rays(inv_view, r2v, full, tile, offset)
    n_px = d.shape[0]
    has, t0, t1 = chord(o, d, bmin, bmax)
    with np.errstate(**_ERR):
        q = np.ceil((t1 - t0) / delta).astype(F)
        n = np.where(q < F(max_steps), np.where(q > 0, q, 0), max_steps)
    n = np.where(has, n, 0).astype(np.int64)

    V = np.zeros(n_px, F)       # the running extremum or sum
    tz = np.zeros(n_px, F)
    cnt = np.zeros(n_px, np.int64)
    hit = np.zeros(n_px, bool)  # ISO
    hit_i = np.zeros(n_px, np.int64)
    ta, tb = np.zeros(n_px, F), np.zeros(n_px, F)
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
        v = S(at(o, tk, d[k]))
        with np.errstate(**_ERR):
            if mode == ISO:
                inside = v >= iso
                kh = k[inside]
                hit[kh], hit_i[kh], tb[kh] = True, i, tk[inside]
                if i > 0:
                    ta[kh] = (t0 + (F(i - 1) + F(0.5)) * delta)[kh]
                live[kh] = False
                continue
            ok = v == v
            k, v, tk = k[ok], v[ok], tk[ok]
            if mode == MEAN:
                V[k] = V[k] + v
            else:
                better = (cnt[k] == 0) | ((v > V[k]) if mode == MAX else (v < V[k]))
                V[k[better]], tz[k[better]] = v[better], tk[better]
            cnt[k] += 1

    rgba = np.zeros((n_px, 4), F)
    rgba[:, :3] = bg
    value, depth = np.zeros(n_px, F), np.zeros(n_px, F)
    if mode != ISO:
        k = np.nonzero(cnt > 0)[0]
        with np.errstate(**_ERR):
            val = (V[k] / cnt[k].astype(F)).astype(F) if mode == MEAN else V[k]
            t = (val - lo) / (hi - lo)
            u = np.where(t > 0, t, F(0)).astype(F)
            u = np.where(u < 1, u, F(1)).astype(F)
            rgba[k, :3] = u[:, None] * colour
            rgba[k, 3] = 1
            value[k], depth[k] = val, tz[k] / diag
        shape = (tile[1], tile[0])
        return rgba.reshape(shape + (4,)), value.reshape(shape), depth.reshape(shape)

    k = np.nonzero(hit)[0]
    if k.size:
        dk = d[k]
        a, b = ta[k].copy(), tb[k].copy()
        bisect = hit_i[k] > 0
        for _ in range(int(refine)):
            with np.errstate(**_ERR):
                tm = (a + F(0.5) * (b - a)).astype(F)
                inside = S(at(o, tm, dk)) >= iso
            b = np.where(bisect & inside, tm, b).astype(F)
            a = np.where(bisect & ~inside, tm, a).astype(F)
        p = at(o, b, dk)
        val = S(p)
        G = np.zeros_like(p)
        for ax in range(3):
            up, dn = p.copy(), p.copy()
            up[:, ax] = p[:, ax] + h[ax]
            dn[:, ax] = p[:, ax] - h[ax]
            with np.errstate(**_ERR):
                G[:, ax] = (S(up) - S(dn)) / h[ax]
        with np.errstate(**_ERR):
            m = np.sqrt(dot3(G, G)).astype(F)
            lit = m > 0
        rgb = np.broadcast_to(colour, p.shape).copy()
        if lit.any():
            with np.errstate(**_ERR):
                nrm = (G[lit] / m[lit][:, None]).astype(F)
                Vv = (-dk[lit]).astype(F)
                if flags & HEADLIGHT:
                    L = Vv
                else:
                    l = np.asarray(light, F)
                    L = np.broadcast_to((l / np.sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2])).astype(F), Vv.shape)
                nl = -dot3(nrm, L)
                nl = np.where(nl > 0, nl, F(0)).astype(F)
                sp = np.zeros_like(nl)
                if specular > 0:
                    H = (L + Vv).astype(F)
                    hh = np.sqrt(dot3(H, H)).astype(F)
                    nh = -dot3(nrm, H) / hh
                    nh = np.where(nh > 0, nh, F(0)).astype(F)
                    for _ in range(int(shininess_log2)):
                        nh = nh * nh
                    sp = np.where(hh > 0, nh, F(0)).astype(F)
                f = ambient + diffuse * nl
                rgb[lit] = f[:, None] * colour + (specular * sp)[:, None]
        rgba[k, :3] = rgb
        rgba[k, 3] = 1
        value[k] = val
        with np.errstate(**_ERR):
            depth[k] = b / diag
    shape = (tile[1], tile[0])
    return rgba.reshape(shape + (4,)), value.reshape(shape), depth.reshape(shape)
