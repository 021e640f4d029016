#!/usr/bin/env python3
"""A/B of classifying a scalar volume by value and gradient magnitude: inside the build kernels
(cvr_set_medium_gradient) against torch ops followed by cvr_set_medium_device, and against the 1-D
cvr_set_medium_scalar on the same tensor.

  python tools/gradient_medium_ab.py [--reps 5] [--case manix|cloud] [--cloud 512 256 512] [--out FILE.md]
  python tools/gradient_medium_ab.py --case manix --once u16|f32     (for a rocprofv3 --pmc run)

One process.  Per row the three routes alternate, one unrecorded round first, then `reps` recorded
rounds; the time is the wall clock around the synchronous calls, median (min-max).

  (a)  set_medium_gradient from a resident scalar tensor (u16 and f32) and a 64 x 16 table;
  (b)  the same gradient and bilinear classification written in torch ops on the device (density
       and albedo tensors are made on every call, as an edit of the table needs), then
       set_medium_device: the only route without this call;
  (c)  set_medium_scalar on the same tensor with a 64-entry 1-D table: no stencil, the floor that
       shows what the stencil adds.

  manix  the C2 medium's grid (the manix proxy at its default size), dense, formats 0 and 1.
  cloud  the cloud proxy at --cloud voxels, densified, sparse=True, formats 0 and 1.

Peak device memory of (a) and (b): torch.cuda.mem_get_info before the first call on a fresh
context with torch's cache emptied, and after it (torch's cache then holds what (b)'s
intermediates took at their peak; the library's own temporaries are freed before it returns).
A context with CVR_OPT_TIMING 1 repeats (a) and (c) for the device time per kernel group.  Before
a row is written, (a)'s context must agree with one built by set_medium_device on
classify_gradient_host's arrays in cvr_medium_info, cvr_medium_layout and the records of 4096
paths.

--once: one format-0 call of (a) and one of (c) on the field, nothing else, so that a counter run
(rocprofv3 --pmc FETCH_SIZE, no tracing; FETCH_SIZE and WRITE_SIZE do not fit one pass) lists each
build kernel once."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch  # (before libcvr is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cudavolumerenderer_amd as cvr  # noqa: E402
from device_medium_ab import DEV, GROUPS, assert_same, densify, med, wall  # noqa: E402
from scalar_medium_ab import CHUNK, as_float, first_call_bytes, group_ms, new_ctx  # noqa: E402

N, M = 64, 16
SPACING = (1.0, 1.0, 1.0)


def make_tables(uniform_colour):
    """The (M, N, 4) table, entry (0, 0) of density 0, and its row 0 as the 1-D table of (c)."""
    rng = np.random.default_rng(61)
    t = np.ones((M, N, 4), np.float32)
    if not uniform_colour:
        t[..., :3] = 0.2 + 0.8 * rng.random((M, N, 3), dtype=np.float32)
    ramp = np.linspace(0.0, 1.0, N, dtype=np.float32)
    t[..., 3] = np.minimum(ramp[None, :] + np.linspace(0.0, 0.5, M, dtype=np.float32)[:, None], 1.0)
    return t, np.ascontiguousarray(t[0])


def torch_gradient_classify(s, table, lo, hi, glo, ghi):
    """The statement of cvr.h in torch ops, whole-grid tensors: (density (z, y, x), albedo (z, y, x, 4))."""
    m, n = table.shape[:2]
    S = as_float(s)

    def diff(axis):
        size = S.shape[axis]
        idx = torch.arange(size, device=S.device)
        cm, cp = (idx - 1).clamp(min=0), (idx + 1).clamp(max=size - 1)
        k = torch.where(cp - cm == 2, 0.5, 1.0).to(torch.float32)
        shape = [1, 1, 1]
        shape[axis] = size
        return (S.index_select(axis, cp) - S.index_select(axis, cm)) * k.reshape(shape)

    gx, gy, gz = diff(2), diff(1), diff(0)
    mag = torch.sqrt((gx * gx + gy * gy) + gz * gz)
    del gx, gy, gz
    u = ((S - lo) / (hi - lo)).clamp(0.0, 1.0).reshape(-1)
    v = ((mag - glo) / (ghi - glo)).clamp(0.0, 1.0).reshape(-1)
    del mag
    flat = table.reshape(m * n, 4)
    density = torch.empty(u.shape, dtype=torch.float32, device=s.device)
    albedo = torch.empty(u.shape + (4,), dtype=torch.float32, device=s.device)
    for k in range(0, u.numel(), CHUNK):
        xt, yt = u[k:k + CHUNK] * float(n - 1), v[k:k + CHUNK] * float(m - 1)
        i, j = xt.floor().clamp(max=n - 2).long(), yt.floor().clamp(max=m - 2).long()
        f, h = (xt - i.to(torch.float32)).unsqueeze(-1), (yt - j.to(torch.float32)).unsqueeze(-1)
        at = j * n + i
        P, Q, R, W = flat[at], flat[at + 1], flat[at + n], flat[at + n + 1]
        a = P + f * (Q - P)
        b = R + f * (W - R)
        e = a + h * (b - a)
        density[k:k + CHUNK] = e[:, 3]
        e[:, 3] = 1.0
        albedo[k:k + CHUNK] = e
    return density.reshape(s.shape), albedo.reshape(s.shape + (4,))


def run_case(title, scalar_f32, kw, uniform_colour, reps, out, once=None):
    """scalar_f32: the field in [0, 1] as a numpy (z, y, x) float array; zeros stay code 0."""
    table, row = make_tables(uniform_colour)
    n = scalar_f32.size
    fields = {"u16": (np.ceil(scalar_f32.astype(np.float64) * 65535).astype(np.uint16), 0.0, 65535.0),
              "f32": (scalar_f32, 0.0, 1.0)}
    ttab = torch.from_numpy(table).to(DEV)
    out += [f"## {title}: {n} voxels, {N} x {M} table", "",
            "| scalar | format | (a) set_medium_gradient, ms | (b) torch ops + set_medium_device, ms | (c) "
            "set_medium_scalar (1-D), ms | (b) / (a) | (a) / (c) | (a) first-call bytes | (b) first-call bytes |",
            "|---|---|---|---|---|---|---|---|---|"]
    groups = []
    for name, (host, lo, hi) in fields.items():
        if once and name != once:
            continue
        glo, ghi = 0.0, 0.05 * (hi - lo)
        ts = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
        torch.cuda.synchronize()

        def call_a(ctx):
            ctx.set_medium_gradient(ts, table, lo=lo, hi=hi, glo=glo, ghi=ghi, spacing=SPACING, **kw)

        def call_b(ctx):
            bd, ba = torch_gradient_classify(ts, ttab, lo, hi, glo, ghi)
            ctx.set_medium_device(bd, ba, **kw)

        def call_c(ctx):
            ctx.set_medium_scalar(ts, row, lo=lo, hi=hi, **kw)

        if once:
            ctx = new_ctx(0)
            call_a(ctx)
            call_c(ctx)
            ctx.close()
            print(f"{title} {name}: one call of (a), one of (c); field {host.nbytes} bytes", flush=True)
            return
        # (a) against set_medium_device on the host statement's arrays, once per field and format
        d, a, _ = cvr.classify_gradient_host(host, table, lo, hi, glo, ghi, SPACING)
        td, ta = torch.from_numpy(d).to(DEV), torch.from_numpy(a).to(DEV)
        del d, a
        for fmt in (0, 1):
            ref, ca = new_ctx(fmt), new_ctx(fmt)
            ref.set_medium_device(td, ta, **kw)
            call_a(ca)
            assert_same(ref, ca, f"{title} {name} format {fmt}")
            ref.close(), ca.close()
        del td, ta
        torch.cuda.empty_cache()
        for fmt in (0, 1):
            ca, cb, cc = new_ctx(fmt), new_ctx(fmt), new_ctx(fmt)
            ta_, tb_, tc_ = [], [], []
            for i in range(reps + 1):
                x, y, z = wall(lambda: call_a(ca)), wall(lambda: call_b(cb)), wall(lambda: call_c(cc))
                if i:
                    ta_.append(x), tb_.append(y), tc_.append(z)
            for c in (ca, cb, cc):
                c.close()
            ma, mb = first_call_bytes(fmt, call_a), first_call_bytes(fmt, call_b)
            sa, sb, sc = (statistics.median(v) for v in (ta_, tb_, tc_))
            out.append(f"| {name} | {fmt} | {med(ta_)} | {med(tb_)} | {med(tc_)} | {sb / sa:.2f}x | {sa / sc:.2f}x | "
                       f"{ma / 1e6:.0f} MB | {mb / 1e6:.0f} MB |")
            groups.append((name, fmt, group_ms(fmt, call_a, reps), group_ms(fmt, call_c, reps)))
            print(f"{title} {name} format {fmt}: done", file=sys.stderr, flush=True)
        del ts
        torch.cuda.empty_cache()
    out += ["", "Device time per group (CVR_OPT_TIMING 1, HIP events, median ms), (a) / (c):", "",
            "| scalar | format | " + " | ".join(GROUPS) + " |", "|---|---|" + "---|" * 6]
    for name, fmt, ga, gc in groups:
        out.append(f"| {name} | {fmt} | " + " | ".join(f"{ga[k]:.3f} / {gc[k]:.3f}" for k in range(6)) + " |")
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=("manix", "cloud"), default="manix")
    ap.add_argument("--cloud", type=int, nargs=3, default=(512, 256, 512))
    ap.add_argument("--once", choices=("u16", "f32"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = ["# Classifying a scalar volume by value and gradient magnitude: in the build kernels against torch ops", "",
           f"`python tools/gradient_medium_ab.py --reps {a.reps} --case {a.case}`: one process, the three routes "
           f"alternating, one unrecorded round, then {a.reps}; wall time around the synchronous calls in ms, median "
           "(min-max).  (a)'s context agrees with one built by set_medium_device on classify_gradient_host's arrays in "
           "cvr_medium_info, cvr_medium_layout and the records of 4096 paths (asserted before the rows are written).", ""]
    if a.case == "manix":
        scene = cvr.Scene.synthetic("manix")
        m = scene.medium
        d = np.ascontiguousarray(scene.density, np.float32)
        kw = dict(box_min=tuple(m.box_min), box_max=tuple(m.box_max), scale=m.scale, g=m.g, roughness=tuple(m.roughness),
                  eta=m.eta)
        nx, ny, nz = scene.dims
        run_case(f"manix proxy grid (C2), {nx}x{ny}x{nz}, dense", d / d.max(), kw, False, a.reps, out, a.once)
    else:
        scene = cvr.Scene.synthetic("cloud", 0, tuple(a.cloud))
        sm = scene.sparse_medium
        D, _, _ = densify(scene)
        kw = dict(sparse=True, box_min=tuple(sm.box_min), box_max=tuple(sm.box_max), scale=sm.scale, g=sm.g,
                  roughness=tuple(sm.roughness), eta=sm.eta)
        nx, ny, nz = scene.dims
        run_case(f"cloud proxy, {nx}x{ny}x{nz}, densified, sparse=True, one colour", D / D.max(), kw, True, a.reps, out,
                 a.once)
    if a.once:
        return 0
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
