#!/usr/bin/env python3
"""A/B of classifying a scalar volume through one table row per label: inside the build kernels
(cvr_set_medium_labeled) against cvr_set_medium_scalar on the same field, the floor without labels,
and against the only route before, the row gather and interpolation in torch ops followed by
cvr_set_medium_device.

  python tools/labeled_medium_ab.py [--reps 5] [--case manix|cloud] [--cloud 512 256 512]
                                    [--labels blocks|random] [--out FILE.md]
  python tools/labeled_medium_ab.py --case manix --once labeled|scalar     (for a rocprofv3 --pmc run)

One process.  Per row the three routes alternate, one unrecorded round first, then `reps` recorded
rounds: the wall clock around the synchronous calls, median (min-max), and the device time, the sum
of the build's kernel groups from HIP events (CVR_OPT_TIMING 1, cvr_debug_device_medium_ms), median.

  (L)  set_medium_labeled from resident u16 scalar and u8 label tensors and an 8 x 256 table;
  (a)  set_medium_scalar on the same scalar tensor with row 1 of the table;
  (b)  the labelled classification in torch ops on the device (the row gather, the interpolation;
       density and albedo tensors are made on every call), then set_medium_device.

  manix  the C2 medium's grid (the manix proxy at its default size), dense, formats 0 and 1.
  cloud  the cloud proxy at --cloud voxels, densified, sparse=True, formats 0 and 1.

labels: "blocks" gives 32^3-voxel segments of labels 1..7 over the non-zero voxels and 0 elsewhere
(a segmentation: a wave sees one label); "random" draws every voxel's label on its own.

Before a row is written, (L)'s context must equal a context given classify_labels_host's arrays
through set_medium_device in cvr_medium_info, cvr_medium_layout, the records of 4096 paths and
every stored array byte for byte, and its label counts must be the host statement's.  The process's
device memory after the first call on a fresh context is reported for (L), (a) and (b).  CVR_LIB
names another build of the library (a byte of labels per lane; the counters compiled out, with
--no-counts).

--once: one format-0 call of one route on the fields, nothing else, so that a counter run
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
from device_medium_ab import DEV, GROUPS, assert_same, densify, med, wall  # noqa: E402
from scalar_medium_ab import as_float, first_call_bytes, group_ms, new_ctx  # noqa: E402

N_TABLE, ROWS = 256, 8
CHUNK = 1 << 24  # voxels per round of torch ops


def make_table(one_colour):
    rng = np.random.default_rng(67)
    t = np.ones((ROWS, N_TABLE, 4), np.float32)
    if not one_colour:
        t[..., :3] = 0.2 + 0.8 * rng.random((ROWS, N_TABLE, 3), dtype=np.float32)
    ramp = np.linspace(0.0, 1.0, N_TABLE, dtype=np.float32)           # entry 0 of every row: density 0
    t[..., 3] = ramp[None, :] * (0.3 + 0.1 * np.arange(ROWS, dtype=np.float32))[:, None]
    return t


def make_labels(scalar, kind):
    nz, ny, nx = scalar.shape
    if kind == "random":
        return np.random.default_rng(71).integers(0, ROWS, scalar.shape).astype(np.uint8)
    z, y, x = np.meshgrid(np.arange(nz) >> 5, np.arange(ny) >> 5, np.arange(nx) >> 5, indexing="ij", sparse=True)
    lab = (1 + (x + y + z) % (ROWS - 1)).astype(np.uint8)
    return np.where(scalar != 0, lab, 0).astype(np.uint8)


def torch_classify(s, lab, table, lo, hi):
    """The labelled linear rule of cvr.h in torch ops: (density (z, y, x), albedo (z, y, x, 4))."""
    m, n = table.shape[:2]
    flat_t = table.reshape(m * n, 4)
    flat, flab = s.reshape(-1), lab.reshape(-1)
    density = torch.empty(flat.shape, dtype=torch.float32, device=s.device)
    albedo = torch.empty(flat.shape + (4,), dtype=torch.float32, device=s.device)
    for k in range(0, flat.numel(), CHUNK):
        u = ((as_float(flat[k:k + CHUNK]) - lo) / (hi - lo)).clamp(0.0, 1.0)
        x = u * float(n - 1)
        i = x.floor().clamp(max=n - 2).long()
        f = (x - i.to(torch.float32)).unsqueeze(-1)
        row = flab[k:k + CHUNK].long()
        at = torch.where(row < m, row, torch.zeros_like(row)) * n + i
        a, b = flat_t[at], flat_t[at + 1]
        e = a + f * (b - a)
        density[k:k + CHUNK] = e[:, 3]
        e[:, 3] = 1.0
        albedo[k:k + CHUNK] = e
    return density.reshape(s.shape), albedo.reshape(s.shape + (4,))


def run_case(title, scalar_f32, kw, one_colour, label_kind, reps, out, once=None, check_counts=True):
    table = make_table(one_colour)
    host = np.ceil(scalar_f32.astype(np.float64) * 65535).astype(np.uint16)
    lab = make_labels(host, label_kind)
    lo, hi = 0.0, 65535.0
    n = host.size
    ts, tl = torch.from_numpy(host).to(DEV), torch.from_numpy(lab).to(DEV)
    if once:
        ctx = new_ctx(0)
        if once == "labeled":
            ctx.set_medium_labeled(ts, tl, table, lo=lo, hi=hi, **kw)
        else:
            ctx.set_medium_scalar(ts, table[1], lo=lo, hi=hi, **kw)
        ctx.close()
        print(f"{title}: one call of route {once}; field {host.nbytes} bytes, labels {lab.nbytes} bytes", flush=True)
        return
    ttab = torch.from_numpy(table).to(DEV)
    d, a, counts = cvr.classify_labels_host(host, lab, table, lo, hi)
    td, ta = torch.from_numpy(d).to(DEV), torch.from_numpy(a).to(DEV)
    del d, a
    torch.cuda.synchronize()

    def call_l(ctx):
        ctx.set_medium_labeled(ts, tl, table, lo=lo, hi=hi, **kw)

    def call_a(ctx):
        ctx.set_medium_scalar(ts, table[1], lo=lo, hi=hi, **kw)

    def call_b(ctx):
        bd, ba = torch_classify(ts, tl, ttab, lo, hi)
        ctx.set_medium_device(bd, ba, **kw)

    out += [f"## {title}: {n} voxels, u16 field + u8 labels ({label_kind}), {ROWS} x {N_TABLE} table, linear", "",
            "| format | (L) set_medium_labeled, ms | (a) set_medium_scalar, ms | (b) torch ops + set_medium_device, ms | "
            "(L) / (a) | (b) / (L) | device ms (L) | device ms (a) | first-call bytes (L) | (a) | (b) |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    groups = []
    for fmt in (0, 1):
        cl, ca, cb, cc = new_ctx(fmt), new_ctx(fmt), new_ctx(fmt), new_ctx(fmt)
        tl_, ta_, tb_ = [], [], []
        for i in range(reps + 1):
            x, y, z = wall(lambda: call_l(cl)), wall(lambda: call_a(ca)), wall(lambda: call_b(cb))
            if i:
                tl_.append(x), ta_.append(y), tb_.append(z)
        cc.set_medium_device(td, ta, **kw)
        assert_same(cc, cl, f"{title} format {fmt}")
        m, got = cl.medium_label_info()
        assert m == ROWS and (not check_counts or (got == counts).all()), f"{title} format {fmt}: label counts"
        for c in (cl, ca, cb, cc):
            c.close()
        ml, ma, mb = (first_call_bytes(fmt, c) for c in (call_l, call_a, call_b))
        gl, ga = group_ms(fmt, call_l, reps), group_ms(fmt, call_a, reps)
        sl, sa, sb = (statistics.median(v) for v in (tl_, ta_, tb_))
        out.append(f"| {fmt} | {med(tl_)} | {med(ta_)} | {med(tb_)} | {sl / sa:.2f}x | {sb / sl:.2f}x | {sum(gl):.3f} | "
                   f"{sum(ga):.3f} | {ml / 1e6:.0f} MB | {ma / 1e6:.0f} MB | {mb / 1e6:.0f} MB |")
        groups.append((fmt, gl, ga))
        print(f"{title} format {fmt}: done", file=sys.stderr, flush=True)
    out += ["", "Device time per group (CVR_OPT_TIMING 1, HIP events, median ms), (L) / (a):", "",
            "| format | " + " | ".join(GROUPS) + " |", "|---|" + "---|" * 6]
    for fmt, gl, ga in groups:
        out.append(f"| {fmt} | " + " | ".join(f"{gl[k]:.3f} / {ga[k]:.3f}" for k in range(6)) + " |")
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=("manix", "cloud"), default="manix")
    ap.add_argument("--cloud", type=int, nargs=3, default=(512, 256, 512))
    ap.add_argument("--labels", choices=("blocks", "random"), default="blocks")
    ap.add_argument("--once", choices=("labeled", "scalar"), default=None)
    ap.add_argument("--no-counts", action="store_true", help="a library built with -DCVR_LABEL_COUNTS=0: its counts are not checked")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = ["# Classifying a scalar volume through one table row per label", "",
           f"`python tools/labeled_medium_ab.py --reps {a.reps} --case {a.case} --labels {a.labels}`, library "
           f"`{os.path.relpath(cvr._lib.LIB_PATH, ROOT)}`: one process, the three routes alternating, one unrecorded round, "
           f"then {a.reps}; wall time around the synchronous calls in ms, median (min-max); device ms: the sum of the "
           "build's kernel groups.  (L)'s context equals set_medium_device on classify_labels_host's arrays in "
           "cvr_medium_info, cvr_medium_layout, the records of 4096 paths and every stored array, and its label counts are "
           "the host statement's (asserted before the row is written).", ""]
    if a.case == "manix":
        scene = cvr.Scene.synthetic("manix")
        m = scene.medium
        d = np.ascontiguousarray(scene.density, np.float32)
        kw = dict(box_min=tuple(m.box_min), box_max=tuple(m.box_max), scale=m.scale, g=m.g, roughness=tuple(m.roughness),
                  eta=m.eta)
        nx, ny, nz = scene.dims
        run_case(f"manix proxy grid (C2), {nx}x{ny}x{nz}, dense", d / d.max(), kw, False, a.labels, a.reps, out, a.once, not a.no_counts)
    else:
        scene = cvr.Scene.synthetic("cloud", 0, tuple(a.cloud))
        sm = scene.sparse_medium
        D, _, _ = densify(scene)
        kw = dict(sparse=True, box_min=tuple(sm.box_min), box_max=tuple(sm.box_max), scale=sm.scale, g=sm.g,
                  roughness=tuple(sm.roughness), eta=sm.eta)
        nx, ny, nz = scene.dims
        run_case(f"cloud proxy, {nx}x{ny}x{nz}, densified, sparse=True, one colour", D / D.max(), kw, True, a.labels,
                 a.reps, out, a.once, not a.no_counts)
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
