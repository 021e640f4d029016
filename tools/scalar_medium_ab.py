#!/usr/bin/env python3
"""A/B of classifying a scalar volume: inside the build kernels (cvr_set_medium_scalar) against
torch ops followed by cvr_set_medium_device, and against cvr_set_medium_device alone.

  python tools/scalar_medium_ab.py [--reps 5] [--case manix|cloud] [--cloud 512 256 512] [--out FILE.md]

One process.  Per row the three routes alternate, one unrecorded round first, then `reps` recorded
rounds; the time is the wall clock around the synchronous calls, median (min-max).

  (a)  set_medium_scalar from a resident scalar tensor (u16 and f32) and a 256-entry table;
  (b)  the same classification written in torch ops on the device (density and albedo tensors
       are made on every call, as an edit of the table needs), then set_medium_device;
  (c)  set_medium_device alone from resident, ready classified tensors (classify_host's).

  manix  the C2 medium's grid (the manix proxy at its default size), dense, formats 0 and 1.
  cloud  the cloud proxy at --cloud voxels, densified, sparse=True, formats 0 and 1.

Peak device memory of (a) and (b): torch.cuda.mem_get_info before the first call on a fresh
context with torch's cache emptied, and after it (torch's cache then holds what (b)'s
intermediates took at their peak; the library's own temporaries are freed before it returns).
A context with CVR_OPT_TIMING 1 repeats (a) and (c) for the device time per kernel group.  Before
a row is written, (a)'s and (c)'s contexts must agree in cvr_medium_info, cvr_medium_layout and
the records of 4096 paths."""
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

N_TABLE = 256


def make_table(uniform_colour):
    rng = np.random.default_rng(61)
    t = np.ones((N_TABLE, 4), np.float32)
    if not uniform_colour:
        t[:, :3] = 0.2 + 0.8 * rng.random((N_TABLE, 3), dtype=np.float32)
    t[:, 3] = np.linspace(0.0, 1.0, N_TABLE, dtype=np.float32)   # entry 0: density 0
    return t


def as_float(s):
    if s.dtype == torch.uint16:  # (through int32: conversions of uint16 are not everywhere in torch)
        return (s.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float32)
    return s.to(torch.float32)


CHUNK = 1 << 24  # voxels per round of torch ops: torch's gather kernels refuse 2^26 rows in one launch here


def torch_classify(s, table, lo, hi):
    """The linear rule of cvr.h in torch ops: (density (z, y, x), albedo (z, y, x, 4)) tensors."""
    n = table.shape[0]
    flat = s.reshape(-1)
    density = torch.empty(flat.shape, dtype=torch.float32, device=s.device)
    albedo = torch.empty(flat.shape + (4,), dtype=torch.float32, device=s.device)
    for k in range(0, flat.numel(), CHUNK):
        u = ((as_float(flat[k:k + CHUNK]) - lo) / (hi - lo)).clamp(0.0, 1.0)
        x = u * float(n - 1)
        i = x.floor().clamp(max=n - 2).long()
        f = (x - i.to(torch.float32)).unsqueeze(-1)
        a, b = table[i], table[i + 1]
        e = a + f * (b - a)
        density[k:k + CHUNK] = e[:, 3]
        e[:, 3] = 1.0
        albedo[k:k + CHUNK] = e
    return density.reshape(s.shape), albedo.reshape(s.shape + (4,))


def new_ctx(fmt, timing=0):
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
    ctx.set_option(cvr.OPT_TIMING, timing)
    return ctx


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def first_call_bytes(fmt, call):
    """Device bytes a fresh context's first call takes and holds on return (torch's cache included)."""
    torch.cuda.empty_cache()
    ctx = new_ctx(fmt)
    before = free_bytes()
    call(ctx)
    after = free_bytes()
    ctx.close()
    torch.cuda.empty_cache()
    return before - after


def group_ms(fmt, call, reps):
    ctx = new_ctx(fmt, 1)
    rows = []
    for i in range(reps + 1):
        call(ctx)
        if i:
            rows.append(ctx.device_medium_ms())
    ctx.close()
    return [statistics.median(r[k] for r in rows) for k in range(6)]


def run_case(title, scalar_f32, kw, uniform_colour, reps, out):
    """scalar_f32: the field in [0, 1] as a numpy (z, y, x) float array; zeros stay code 0."""
    table = make_table(uniform_colour)
    n = scalar_f32.size
    fields = {"u16": (np.ceil(scalar_f32.astype(np.float64) * 65535).astype(np.uint16), 0.0, 65535.0),
              "f32": (scalar_f32, 0.0, 1.0)}
    ttab = torch.from_numpy(table).to(DEV)
    out += [f"## {title}: {n} voxels, {N_TABLE}-entry table, linear", "",
            "| scalar | format | (a) set_medium_scalar, ms | (b) torch ops + set_medium_device, ms | (c) set_medium_device "
            "alone, ms | (b) / (a) | (a) / (c) | (a) first-call bytes | (b) first-call bytes |", "|---|---|---|---|---|---|---|---|---|"]
    groups = []
    for name, (host, lo, hi) in fields.items():
        ts = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
        d, a = cvr.classify_host(host, table, lo, hi)
        td, ta = torch.from_numpy(d).to(DEV), torch.from_numpy(a).to(DEV)
        del d, a
        torch.cuda.synchronize()

        def call_a(ctx):
            ctx.set_medium_scalar(ts, table, lo=lo, hi=hi, **kw)

        def call_b(ctx):
            bd, ba = torch_classify(ts, ttab, lo, hi)
            ctx.set_medium_device(bd, ba, **kw)

        def call_c(ctx):
            ctx.set_medium_device(td, ta, **kw)

        for fmt in (0, 1):
            ca, cb, cc = new_ctx(fmt), new_ctx(fmt), new_ctx(fmt)
            ta_, tb_, tc_ = [], [], []
            for i in range(reps + 1):
                x, y, z = wall(lambda: call_a(ca)), wall(lambda: call_b(cb)), wall(lambda: call_c(cc))
                if i:
                    ta_.append(x), tb_.append(y), tc_.append(z)
            assert_same(cc, ca, f"{title} {name} format {fmt}")
            for c in (ca, cb, cc):
                c.close()
            ma, mb = first_call_bytes(fmt, call_a), first_call_bytes(fmt, call_b)
            sa, sb, sc = (statistics.median(v) for v in (ta_, tb_, tc_))
            out.append(f"| {name} | {fmt} | {med(ta_)} | {med(tb_)} | {med(tc_)} | {sb / sa:.2f}x | {sa / sc:.2f}x | "
                       f"{ma / 1e6:.0f} MB | {mb / 1e6:.0f} MB |")
            groups.append((name, fmt, group_ms(fmt, call_a, reps), group_ms(fmt, call_c, reps)))
            print(f"{title} {name} format {fmt}: done", file=sys.stderr, flush=True)
        del ts, td, ta
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = ["# Classifying a scalar volume: in the build kernels against torch ops", "",
           f"`python tools/scalar_medium_ab.py --reps {a.reps} --case {a.case}`: one process, the three routes "
           f"alternating, one unrecorded round, then {a.reps}; wall time around the synchronous calls in ms, median "
           "(min-max).  (a)'s and (c)'s contexts agree in cvr_medium_info, cvr_medium_layout and the records of 4096 "
           "paths (asserted before the row is written).", ""]
    if a.case == "manix":
        scene = cvr.Scene.synthetic("manix")
        m = scene.medium
        d = np.ascontiguousarray(scene.density, np.float32)
        kw = dict(box_min=tuple(m.box_min), box_max=tuple(m.box_max), scale=m.scale, g=m.g, roughness=tuple(m.roughness),
                  eta=m.eta)
        nx, ny, nz = scene.dims
        run_case(f"manix proxy grid (C2), {nx}x{ny}x{nz}, dense", d / d.max(), kw, False, a.reps, out)
    else:
        scene = cvr.Scene.synthetic("cloud", 0, tuple(a.cloud))
        sm = scene.sparse_medium
        D, _, _ = densify(scene)
        kw = dict(sparse=True, box_min=tuple(sm.box_min), box_max=tuple(sm.box_max), scale=sm.scale, g=sm.g,
                  roughness=tuple(sm.roughness), eta=sm.eta)
        nx, ny, nz = scene.dims
        run_case(f"cloud proxy, {nx}x{ny}x{nz}, densified, sparse=True, one colour", D / D.max(), kw, True, a.reps, out)
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
