"""The shaded preview pass restated in numpy from the text of include/cvr.h (CVR_HAS_PREVIEW),
independently of csrc/cvr_preview.h: fp32 arrays over all pixels at once, one operation per numpy
call in the written order, so every intermediate is rounded as the text says.  The ray, the chord,
the trilinear and the exact fused multiply-add are features_ref's (the restatement of
CVR_HAS_FEATURES, which the text refers to for them).

preview(...) -> rgba (h, w, 4).  preview_fetch(res, density, albedo, ...) is the same march over two
fetch functions and an optional tap log (features_ref.features_fetch's); preview() is preview_fetch
over features_ref.array_fetch."""
import numpy as np

from features_ref import array_fetch, chord, fma, march, maxnum, minnum, rays, support_skip, trilinear  # noqa: F401

F = np.float32
_ERR = dict(invalid="ignore", divide="ignore", over="ignore", under="ignore")
UNSHADED, HEADLIGHT = 1, 2


def dot3(a, b):
    """(a_x b_x + a_y b_y) + a_z b_z over the last axis."""
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


def preview(density, albedo, box_min, box_max, scale, max_density, inv_view, r2v, full, tile, offset=(0, 0), w2a=0,
            step=1.0, t_stop=1.0 / 256.0, max_steps=4096, light=(0, 0, 0), ambient=0.3, diffuse=0.7, specular=0.2,
            shininess_log2=4, knee=0.05, background=(0, 0, 0), flags=HEADLIGHT, taps=None):
    """The march over a dense medium's arrays: preview_fetch over array_fetch."""
    res, dens, alb = array_fetch(density, albedo)
    return preview_fetch(res, dens, alb, box_min, box_max, scale, max_density, inv_view, r2v, full, tile, offset, w2a, step,
                         t_stop, max_steps, light, ambient, diffuse, specular, shininess_log2, knee, background, flags, taps)


def preview_fetch(res, density, albedo, box_min, box_max, scale, max_density, inv_view, r2v, full, tile, offset=(0, 0),
                  w2a=0, step=1.0, t_stop=1.0 / 256.0, max_steps=4096, light=(0, 0, 0), ambient=0.3, diffuse=0.7,
                  specular=0.2, shininess_log2=4, knee=0.05, background=(0, 0, 0), flags=HEADLIGHT, taps=None, support=None):
    res = tuple(int(r) for r in res)
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

    def rho_at(p, log):
        cg = fma((p - shift).astype(F), g, F(0))
        return trilinear(density, cg[:, 0], cg[:, 1], cg[:, 2], res, log)

    o, d = rays(inv_view, r2v, full, tile, offset)
    n_px = d.shape[0]
    has, t0, t1 = chord(o, d, bmin, bmax)
    with np.errstate(**_ERR):
        q = np.ceil((t1 - t0) / delta).astype(F)
        n = np.where(q < F(max_steps), np.where(q > 0, q, 0), max_steps)
    n = np.where(has, n, 0).astype(np.int64)

    def emission(kh, th, ph, log):
        ca = ((ph - bmin) / e) * ag
        c = trilinear(albedo, ca[:, 0], ca[:, 1], ca[:, 2], res).astype(F)
        em = c.copy()
        if shaded:
            G = np.zeros_like(ph)
            for ax in range(3):
                hi, lo = ph.copy(), ph.copy()
                hi[:, ax] = ph[:, ax] + h[ax]
                lo[:, ax] = ph[:, ax] - h[ax]
                G[:, ax] = (rho_at(hi, log) - rho_at(lo, log)) / h[ax]
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
        return em

    skip = None if support is None else support_skip(support, res, shift, g)
    Cc, W, T = march(o, d, n, t0, t1, delta, scale, t_stop, rho_at, emission, 3, skip, taps)
    rgba = np.zeros((n_px, 4), F)
    rgba[:, :3] = Cc + T[:, None] * bg
    rgba[:, 3] = W
    rgba[~has, :3] = bg
    rgba[~has, 3] = 0
    return rgba.reshape(tile[1], tile[0], 4)


def unshaded_from(sums, background=(0, 0, 0)):
    """The unshaded preview of the march whose sums features_ref.features_fetch left in `sums`: an
    unshaded sample's emission is its albedo c, so the preview's C is the feature pass's A, sample
    for sample in the same order, and rgba = (A + T background, W), the background alone without a
    chord."""
    bg = np.asarray(background, F)
    rgba = np.zeros(sums["W"].shape + (4,), F)
    rgba[:, :3] = sums["A"] + sums["T"][:, None] * bg
    rgba[:, 3] = sums["W"]
    rgba[~sums["has"], :3] = bg
    rgba[~sums["has"], 3] = 0
    w, h = sums["tile"]
    return rgba.reshape(h, w, 4)
