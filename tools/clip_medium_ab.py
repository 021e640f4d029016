#!/usr/bin/env python3
"""A/B of the clip region of the device builds (cvr_set_clip) on the 2-D classification route:
what the test costs when it keeps everything, what a cut saves, and the cut done in torch ops.

  python tools/clip_medium_ab.py [--reps 5] [--case manix|cloud] [--cloud 512 256 512] [--out FILE.md]
  python tools/clip_medium_ab.py --case manix --once none|all|crop|plane   (for a rocprofv3 --pmc run)

One process.  Per format the routes alternate, one unrecorded round first, then `reps` recorded
rounds: the wall clock around the synchronous call, median (min-max), and the device time of the
call's kernels by HIP events (CVR_OPT_TIMING 1: the sum of cvr_debug_device_medium_ms' six groups,
median of `reps` calls on a context of its own).  The field is u16, the table 64 x 16.

  (p)  set_medium_gradient with no clip set: the kernels of the parent commit (the unclipped
       instances are its instruction streams, tools/isa_same.py), and by the alternation the
       run-to-run spread that (a) is held against;
  (a)  the same call under a clip that keeps everything (the whole grid as crop box and one
       plane no voxel fails): the cost of the test itself;
  (b)  under a crop to the lower half in z, and under an oblique plane through the grid's centre;
  (c)  the only route before: the classification in torch ops, the cut as a multiplication by a
       mask tensor (and the albedo set to voxel 0's), then set_medium_device; with its peak device
       memory beside (b)'s (torch.cuda.mem_get_info around a fresh context's first call);
  (d)  the stored bytes (cvr_medium_info.total_bytes) of each.

--case manix adds the arrays' route: set_medium_device on C2's own density and albedo tensors,
(p), (a) and the half crop, where the clipped passes (one voxel per lane) stand in for the
16-byte scans and the copy or conversion.

Before a number is written, (a)'s context must equal (p)'s, and each of (b)'s must equal one built
by set_medium_device on cvr_clip_host's output of classify_gradient_host's arrays, in
cvr_medium_info, cvr_medium_layout, the records of 4096 paths and every stored array
(device_medium_ab.assert_same); the kept count must be the mask's.

--once: one format-0 call of one route on the field, nothing else, so that a counter run
(rocprofv3 --pmc FETCH_SIZE, no tracing) lists each build kernel once."""
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
from device_medium_ab import DEV, assert_same, densify, med, wall  # noqa: E402
from gradient_medium_ab import SPACING, make_tables, torch_gradient_classify  # noqa: E402
from scalar_medium_ab import first_call_bytes, group_ms, new_ctx  # noqa: E402

ROUTES = ("none", "all", "crop", "plane")


def regions(shape):
    """The clips by route for a (z, y, x) grid: lo, hi, planes."""
    nz, ny, nx = shape
    centre = 0.5 * ((nx - 1) + (ny - 1) + (nz - 1))
    return {"all": ((0, 0, 0), (nx, ny, nz), [(0.0, 0.0, 1.0, 1.0)]),
            "crop": ((0, 0, 0), (nx, ny, nz // 2), []),
            "plane": (None, None, [(1.0, 1.0, 1.0, -centre)])}


def torch_clip(d, a, region):
    """The cut in torch ops on classified tensors: the mask of the region, density times the mask,
    the albedo of a clipped voxel replaced by voxel 0's."""
    lo, hi, planes = region
    nz, ny, nx = d.shape
    z, y, x = (torch.arange(n, device=d.device).reshape(s) for n, s in ((nz, (-1, 1, 1)), (ny, (1, -1, 1)), (nx, (1, 1, -1))))
    keep = torch.ones(d.shape, dtype=torch.bool, device=d.device)
    if lo is not None:
        keep &= (x >= lo[0]) & (x < hi[0]) & (y >= lo[1]) & (y < hi[1]) & (z >= lo[2]) & (z < hi[2])
    for A, B, C, D in planes:
        keep &= ((A * x.float() + B * y.float()) + C * z.float()) + D >= 0
    a0 = a[0, 0, 0].clone()
    return d * keep, torch.where(keep.unsqueeze(-1), a, a0)


def run_case(title, scalar_f32, kw, uniform_colour, reps, out, once=None):
    table, _ = make_tables(uniform_colour)
    host = np.ceil(scalar_f32.astype(np.float64) * 65535).astype(np.uint16)
    lo, hi, glo, ghi = 0.0, 65535.0, 0.0, 0.05 * 65535.0
    shape = host.shape
    nz, ny, nx = shape
    reg = regions(shape)
    ts = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
    ttab = torch.from_numpy(table).to(DEV)
    torch.cuda.synchronize()

    def build(ctx, route):
        if route == "none":
            ctx.clear_clip()
        else:
            ctx.set_clip(*reg[route])
        ctx.set_medium_gradient(ts, table, lo=lo, hi=hi, glo=glo, ghi=ghi, spacing=SPACING, **kw)

    def build_torch(ctx, route):
        d, a = torch_gradient_classify(ts, ttab, lo, hi, glo, ghi)
        d, a = torch_clip(d, a, reg[route])
        ctx.set_medium_device(d, a, **kw)

    if once:
        ctx = new_ctx(0)
        build(ctx, once)
        ctx.close()
        print(f"{title}: one call of route {once}; field {host.nbytes} bytes", flush=True)
        return
    # equality first: (a) against (p); (b) against set_medium_device on the host statements' arrays
    d0, a0, _ = cvr.classify_gradient_host(host, table, lo, hi, glo, ghi, SPACING)
    kept = {}
    for fmt in (0, 1):
        plain, ca = new_ctx(fmt), new_ctx(fmt)
        build(plain, "none")
        build(ca, "all")
        assert_same(plain, ca, f"{title} format {fmt}: keep-everything clip against no clip")
        assert ca.medium_clip_info()[1] == host.size
        plain.close(), ca.close()
        for route in ("crop", "plane"):
            keep, dc, ac = cvr.clip_host((nx, ny, nz), *reg[route], density=d0, albedo=a0)
            ref, cb = new_ctx(fmt), new_ctx(fmt)
            td, ta = torch.from_numpy(dc).to(DEV), torch.from_numpy(ac).to(DEV)
            ref.set_medium_device(td, ta, **kw)
            build(cb, route)
            assert_same(ref, cb, f"{title} format {fmt}: {route} against clip_host's arrays")
            kept[route] = cb.medium_clip_info()[1]
            assert kept[route] == int(keep.sum())
            ref.close(), cb.close()
            del td, ta
    del d0, a0
    torch.cuda.empty_cache()
    out += [f"## {title}: {host.size} voxels u16 ({host.nbytes / 1e6:.0f} MB), 64 x 16 table", "",
            f"Kept voxels: crop {kept['crop']} ({kept['crop'] / host.size:.3f}), plane {kept['plane']} "
            f"({kept['plane'] / host.size:.3f}).", "",
            "| format | route | wall ms, median (min-max) | device ms (HIP events) | device ms / (p) | stored bytes | "
            "first-call bytes |", "|---|---|---|---|---|---|---|"]
    for fmt in (0, 1):
        names = [("(p) no clip", "none", build), ("(a) keeps everything", "all", build), ("(b) half crop", "crop", build),
                 ("(b) oblique plane", "plane", build), ("(c) torch ops, half crop", "crop", build_torch),
                 ("(c) torch ops, oblique plane", "plane", build_torch)]
        ctxs = [new_ctx(fmt) for _ in names]
        times = [[] for _ in names]
        for i in range(reps + 1):
            for k, (_, route, fn) in enumerate(names):
                t = wall(lambda: fn(ctxs[k], route))
                if i:
                    times[k].append(t)
        stored = [c.medium_info().total_bytes for c in ctxs]
        for c in ctxs:
            c.close()
        base = None
        for k, (label, route, fn) in enumerate(names):
            dev = sum(group_ms(fmt, lambda c: fn(c, route), reps)) if fn is build else None
            base = dev if base is None else base
            first = first_call_bytes(fmt, lambda c: fn(c, route))
            out.append(f"| {fmt} | {label} | {med(times[k])} | " + (f"{dev:.3f} | {dev / base:.2f}x" if dev is not None
                                                                  else "- | -")
                       + f" | {stored[k] / 1e6:.1f} MB | {first / 1e6:.0f} MB |")
        spread = max(times[0]) - min(times[0])
        out.append(f"| {fmt} | (p)'s own spread, max - min of its {reps} calls | {spread:.2f} | | | | |")
        print(f"{title} format {fmt}: done", file=sys.stderr, flush=True)
    out.append("")


def run_arrays(title, d, a, kw, reps, out):
    """The arrays' route, dense: set_medium_device on resident density and albedo tensors with no
    clip (16-byte scans, the copy or k_to_half), under the keep-everything clip and under the half
    crop (k_arrays_clip: one voxel per lane)."""
    nz, ny, nx = d.shape
    reg = regions(d.shape)
    td, ta = torch.from_numpy(np.ascontiguousarray(d)).to(DEV), torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    torch.cuda.synchronize()

    def build(ctx, route):
        if route == "none":
            ctx.clear_clip()
        else:
            ctx.set_clip(*reg[route])
        ctx.set_medium_device(td, ta, **kw)

    for fmt in (0, 1):
        plain, ca, ref, cb = (new_ctx(fmt) for _ in range(4))
        build(plain, "none"), build(ca, "all"), build(cb, "crop")
        assert_same(plain, ca, f"{title} format {fmt}: keep-everything clip against no clip")
        keep, dc, ac = cvr.clip_host((nx, ny, nz), *reg["crop"], density=d, albedo=a)
        rd, ra = torch.from_numpy(dc).to(DEV), torch.from_numpy(ac).to(DEV)
        ref.set_medium_device(rd, ra, **kw)
        assert_same(ref, cb, f"{title} format {fmt}: crop against clip_host's arrays")
        assert cb.medium_clip_info()[1] == int(keep.sum())
        for c in (plain, ca, ref, cb):
            c.close()
        del rd, ra
    out += [f"## {title}: set_medium_device on density and albedo tensors ({d.nbytes / 1e6:.0f} + {a.nbytes / 1e6:.0f} MB)", "",
            "| format | route | wall ms, median (min-max) | device ms (HIP events) | device ms / (p) |", "|---|---|---|---|---|"]
    for fmt in (0, 1):
        names = [("(p) no clip", "none"), ("(a) keeps everything", "all"), ("(b) half crop", "crop")]
        ctxs = [new_ctx(fmt) for _ in names]
        times = [[] for _ in names]
        for i in range(reps + 1):
            for k, (_, route) in enumerate(names):
                t = wall(lambda: build(ctxs[k], route))
                if i:
                    times[k].append(t)
        for c in ctxs:
            c.close()
        base = None
        for k, (label, route) in enumerate(names):
            dev = sum(group_ms(fmt, lambda c: build(c, route), reps))
            base = dev if base is None else base
            out.append(f"| {fmt} | {label} | {med(times[k])} | {dev:.3f} | {dev / base:.2f}x |")
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=("manix", "cloud"), default="manix")
    ap.add_argument("--cloud", type=int, nargs=3, default=(512, 256, 512))
    ap.add_argument("--once", choices=ROUTES, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = ["# Clip region of the device builds: the cost of the test, what a cut saves, the cut in torch ops", "",
           f"`python tools/clip_medium_ab.py --reps {a.reps} --case {a.case}`: one process, the routes alternating, one "
           f"unrecorded round, then {a.reps}.  Every clipped context equals its reference in cvr_medium_info, "
           "cvr_medium_layout, the records of 4096 paths and every stored array (asserted before the rows are written).", ""]
    if a.case == "manix":
        scene = cvr.Scene.synthetic("manix")
        m = scene.medium
        d = np.ascontiguousarray(scene.density, np.float32)
        kw = dict(box_min=tuple(m.box_min), box_max=tuple(m.box_max), scale=m.scale, g=m.g, roughness=tuple(m.roughness),
                  eta=m.eta)
        nx, ny, nz = scene.dims
        run_case(f"manix proxy grid (C2), {nx}x{ny}x{nz}, dense", d / d.max(), kw, False, a.reps, out, a.once)
        if not a.once:
            run_arrays(f"manix proxy (C2's medium), {nx}x{ny}x{nz}, dense, the arrays' route", d,
                       np.ascontiguousarray(scene.albedo, np.float32), dict(kw, max_density=m.max_density), a.reps, out)
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
