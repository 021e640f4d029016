"""The shaded preview pass restated in numpy from the text of include/cvr.h (CVR_HAS_PREVIEW),
independently of csrc/cvr_preview.h: fp32 arrays over all pixels at once, one operation per numpy
call in the written order, so every intermediate is rounded as the text says.  The ray, the chord,
the trilinear and the exact fused multiply-add are features_ref's (the restatement of
CVR_HAS_FEATURES, which the text refers to for them).

preview(...) -> rgba (h, w, 4)."""
import numpy as np

from features_ref import chord, fma, maxnum, minnum, rays, trilinear  # noqa: F401

F = np.float32
_ERR = dict(invalid="ignore", divide="ignore", over="ignore", under="ignore")
UNSHADED, HEADLIGHT = 1, 2


def dot3(a, b):
    """(a_x b_x + a_y b_y) + a_z b_z over the last axis."""
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


def preview(density, albedo, box_min, box_max, scale, max_density, inv_view, r2v, full, tile, offset=(0, 0), w2a=0,
            step=1.0, t_stop=1.0 / 256.0, max_steps=4096, light=(0, 0, 0), ambient=0.3, diffuse=0.7, specular=0.2,
            shininess_log2=4, knee=0.05, background=(0, 0, 0), flags=HEADLIGHT):
    density = np.asarray(density, F)
    albedo = np.asarray(albedo, F)
    res = density.shape[::-1]
    fres = np.array(res, F)
    bmin, bmax = np.asarray(box_min, F), np.asarray(box_max, F)
    e = bmax - bmin
    ag = np.array([r - 1 for r in res], F)
    shift, g = (bmin, ag / e) if w2a else (bmin / e, ag)
    h = (e / fres).astype(F)
    hmin = minnum(minnum(h[0], h[1]), h[2])
    delta = F(step) * hmin
    scale, t_stop = F(scale), F(t_stop)
    ambient, diffuse, specular = F(ambient), F(diffuse), F(specular)
    knee_abs = F(knee) * (F(max_density) / hmin)
    bg = np.asarray(background, F)
    shaded = not flags & UNSHADED
    headlight = bool(flags & HEADLIGHT)
    if shaded and not headlight:
        l = np.asarray(light, F)
        L_fixed = (l / np.sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2])).astype(F)

    def rho_at(p):
        cg = fma((p - shift).astype(F), g, F(0))
        return trilinear(lambda x, y, z: density[z, y, x], cg[:, 0], cg[:, 1], cg[:, 2], res)

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
        em = c.copy()
        if shaded:
            G = np.zeros_like(ph)
            for ax in range(3):
                hi, lo = ph.copy(), ph.copy()
                hi[:, ax] = ph[:, ax] + h[ax]
                lo[:, ax] = ph[:, ax] - h[ax]
                G[:, ax] = (rho_at(hi) - rho_at(lo)) / h[ax]
            with np.errstate(**_ERR):
                m = np.sqrt(dot3(G, G)).astype(F)
                lit = m > 0
            if lit.any():
                Gl, ml, cl = G[lit], m[lit], c[lit]
                nrm = (Gl / ml[:, None]).astype(F)
                V = (-d[kh][lit]).astype(F)
                L = V if headlight else np.broadcast_to(L_fixed, V.shape)
                nl = -dot3(nrm, L)
                nl = np.where(nl > 0, nl, F(0)).astype(F)
                sp = np.zeros_like(nl)
                if specular > 0:
                    H = (L + V).astype(F)
                    with np.errstate(**_ERR):
                        hh = np.sqrt(dot3(H, H)).astype(F)
                        nh = -dot3(nrm, H) / hh
                    nh = np.where(nh > 0, nh, F(0)).astype(F)
                    for _ in range(int(shininess_log2)):
                        nh = nh * nh
                    sp = np.where(hh > 0, nh, F(0)).astype(F)
                f = ambient + diffuse * nl
                litc = f[:, None] * cl + (specular * sp)[:, None]
                qq = ml / (ml + knee_abs)
                em[lit] = (F(1) - qq)[:, None] * cl + qq[:, None] * litc
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
