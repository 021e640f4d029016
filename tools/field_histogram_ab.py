#!/usr/bin/env python3
"""A/B of the value-gradient histogram and the statistics of a scalar field in device memory:
cvr_field_histogram / cvr_field_stats against torch ops and torch.bincount, and against the
stencil walk without bins.

  python tools/field_histogram_ab.py [--reps 5] [--case manix|random|cloud] [--cloud 512 256 512]
                                     [--routes ab|a] [--out FILE.md]
  python tools/field_histogram_ab.py --case manix --once u16|f32     (for a rocprofv3 --pmc run)

One process.  Per row the routes alternate, one unrecorded round first, then `reps` recorded
rounds.  Wall time is the clock around the synchronous calls; device time is between two HIP
events on the stream the context is given (torch's current one), around the asynchronous
cvr_field_histogram_buffers for (a).  Median (min-max), ms.

  (a)  Context.field_histogram (and field_stats) on a resident tensor;
  (b)  the only route before: the gradient magnitude and both coordinates in torch ops (whole-grid
       tensors), the bin rule, then torch.bincount;
  (c)  the floor: the device time of set_medium_gradient's scan pass on the same tensor
       (k_gradient<T, false>, the same walk without bins; CVR_OPT_TIMING's first group).

  manix   the C2 medium's grid (the manix proxy at its default size) as u16 and f32: mostly empty,
          so most voxels fall into one bin (the contended case);
  random  a uniform random u16 field of the same shape (the uncontended case);
  cloud   the cloud proxy at --cloud voxels, densified, as u16.

The value range is the type's (u16: 0..65535, f32: 0..1), the gradient range 0..gmax of (a)'s
field_stats.  Before a field's first number is printed, (a)'s counts must equal (b)'s for every bin
shape, and cvr_field_histogram_host's for the largest; (a)'s statistics must equal
cvr_field_stats_host's bits.  --routes a skips (b) (and its assertion), for a library built with
-DCVR_FIELD_MERGE=0 loaded through CVR_LIB.

--once: one field_stats and one field_histogram of 64 x 64, of 256 x 256 and of 256 x 1 bins (the
last reads the field once, no stencil: the calibration), nothing else, so that a counter run
(rocprofv3 --pmc FETCH_SIZE, no tracing) lists each kernel once."""
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
from device_medium_ab import DEV, densify, med, wall  # noqa: E402
from scalar_medium_ab import as_float, free_bytes, group_ms  # noqa: E402

BINS = [(64, 64), (128, 128), (129, 128), (256, 256), (256, 1), (65536, 1)]


def torch_magnitude(S):
    """The gradient statement of cvr.h in torch ops, spacing 1, on the float field S (z, y, x)."""
    def diff(axis):
        size = S.shape[axis]
        idx = torch.arange(size, device=S.device)
        cm, cp = (idx - 1).clamp(min=0), (idx + 1).clamp(max=size - 1)
        k = torch.where(cp - cm == 2, 0.5, 1.0).to(torch.float32)
        shape = [1, 1, 1]
        shape[axis] = size
        return (S.index_select(axis, cp) - S.index_select(axis, cm)) * k.reshape(shape)

    gx, gy, gz = diff(2), diff(1), diff(0)
    return torch.sqrt((gx * gx + gy * gy) + gz * gz)


def torch_bins(c, lo, hi, k):
    """The bin of every element of c over [lo, hi] on k nodes (a true division: by a tensor)."""
    den = torch.tensor(np.float32(hi) - np.float32(lo), dtype=torch.float32, device=c.device)
    x = ((c - lo) / den).clamp(0.0, 1.0) * float(k - 1)
    i0 = x.floor().clamp(max=k - 1)
    return (i0 + (x - i0 >= 0.5)).clamp(max=k - 1).long()


def torch_histogram(s, n, m, lo, hi, glo, ghi):
    S = as_float(s)
    at = torch_bins(S, lo, hi, n).reshape(-1)
    if m > 1:
        at = torch_bins(torch_magnitude(S), glo, ghi, m).reshape(-1) * n + at
    return torch.bincount(at, minlength=n * m).reshape(m, n)


def event_ms(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def first_call_bytes(call):
    """Device bytes the call takes at its peak and holds on return (torch's cache included)."""
    torch.cuda.empty_cache()
    before = free_bytes()
    call()
    after = free_bytes()
    torch.cuda.empty_cache()
    return before - after


def run_field(title, name, host, lo, hi, reps, routes, out, once):
    ts = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
    torch.cuda.synchronize()
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    if once:
        st = ctx.field_stats(ts)
        for n, m in ((64, 64), (256, 256), (256, 1)):
            ctx.field_histogram(ts, n, m, lo=lo, hi=hi, glo=0.0, ghi=float(st.gmax))
        print(f"{title} {name}: one field_stats, one histogram of 64 x 64, of 256 x 256 and of 256 x 1; field "
              f"{host.nbytes} bytes", flush=True)
        ctx.close()
        return
    st = ctx.field_stats(ts)
    want = cvr.field_stats_host(host)
    assert [np.float32(v).view(np.uint32) for v in st[:3]] == [np.float32(v).view(np.uint32) for v in want[:3]] and \
        st[3:] == want[3:], (st, want)
    glo, ghi = 0.0, float(st.gmax)
    outs = {b: torch.empty(b[0] * b[1], dtype=torch.int32, device=DEV) for b in BINS}

    def call_a(n, m):
        return ctx.field_histogram(ts, n, m, lo=lo, hi=hi, glo=glo, ghi=ghi)

    def call_a_async(n, m):
        ctx.field_histogram(ts, n, m, lo=lo, hi=hi, glo=glo, ghi=ghi, out=outs[(n, m)])

    def call_b(n, m):
        h = torch_histogram(ts, n, m, lo, hi, glo, ghi)
        torch.cuda.synchronize()
        return h

    # the routes agree, before any number
    for n, m in BINS:
        got = call_a(n, m)
        assert int(got.sum(dtype=np.uint64)) == host.size
        if "b" in routes:
            ref = call_b(n, m).cpu().numpy()
            bad = int((got.astype(np.int64) != ref).sum())
            assert bad == 0, f"{title} {name} {n} x {m}: {bad} bins differ between (a) and (b)"
    n, m = 256, 256
    assert np.array_equal(call_a(n, m), cvr.field_histogram_host(host, n, m, lo=lo, hi=hi, glo=glo, ghi=ghi))
    torch.cuda.empty_cache()
    # (c): the scan pass of set_medium_gradient with a 64 x 16 table on the same tensor
    table = np.ones((16, 64, 4), np.float32)
    table[..., 3] = np.linspace(0.0, 1.0, 64, dtype=np.float32)[None, :]
    floor = group_ms(0, lambda c: c.set_medium_gradient(ts, table, lo=lo, hi=hi, glo=glo, ghi=ghi), reps)[0]
    stats_ms = [event_ms(lambda: ctx.field_stats(ts)) for _ in range(reps + 1)][1:]
    largest = max(int(np.max(call_a(n, m))) for n, m in ((64, 64),))
    out += [f"## {title}, {name}: {host.size} voxels, {host.nbytes / 1e6:.0f} MB; gmax {ghi:.6g}; the fullest of 64 x 64 "
            f"bins holds {100.0 * largest / host.size:.1f} % of the voxels", "",
            f"(c) the walk without bins (set_medium_gradient's scan pass): {floor:.3f} ms device time.  field_stats "
            f"(synchronous, with its allocation and copies): {med(stats_ms)} ms.", "",
            "| bins | (a) wall, ms | (a) device, ms | (b) wall, ms | (b) device, ms | (b) / (a) wall | (a) device / (c) | "
            "(a) first-call bytes | (b) first-call bytes |", "|---|---|---|---|---|---|---|---|---|"]
    for n, m in BINS:
        wa, da, wb, db = [], [], [], []
        for i in range(reps + 1):
            x = wall(lambda: call_a(n, m))
            y = event_ms(lambda: call_a_async(n, m))
            z = w = float("nan")
            if "b" in routes:
                z = wall(lambda: call_b(n, m))
                w = event_ms(lambda: torch_histogram(ts, n, m, lo, hi, glo, ghi))
            if i:
                wa.append(x), da.append(y), wb.append(z), db.append(w)
        ma = first_call_bytes(lambda: call_a(n, m))
        sa, sd = statistics.median(wa), statistics.median(da)
        row = f"| {n} x {m} | {med(wa)} | {med(da)} | "
        if "b" in routes:
            mb = first_call_bytes(lambda: call_b(n, m))
            row += f"{med(wb)} | {med(db)} | {statistics.median(wb) / sa:.1f}x | "
        else:
            mb = 0
            row += "- | - | - | "
        row += f"{sd / floor:.2f}x | " if m > 1 else "- | "
        out.append(row + f"{ma / 1e6:.1f} MB | {mb / 1e6:.0f} MB |")
        print(f"{title} {name} {n} x {m}: done", file=sys.stderr, flush=True)
    out.append("")
    ctx.close()
    del ts, outs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=("manix", "random", "cloud"), default="manix")
    ap.add_argument("--cloud", type=int, nargs=3, default=(512, 256, 512))
    ap.add_argument("--routes", choices=("ab", "a"), default="ab")
    ap.add_argument("--once", choices=("u16", "f32"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = ["# Histogram and statistics of a scalar field on the device: the field kernels against torch ops", "",
           f"`python tools/field_histogram_ab.py --reps {a.reps} --case {a.case} --routes {a.routes}` with the library "
           f"`{os.path.relpath(cvr.LIB_PATH, ROOT)}`: one process, the routes alternating, one unrecorded round, then "
           f"{a.reps}; ms, median (min-max).  The routes' counts are equal (asserted before a field's rows are written).",
           ""]
    u16 = lambda d: np.ceil(d.astype(np.float64) * 65535).astype(np.uint16)  # noqa: E731  (zeros stay code 0)
    if a.case == "cloud":
        scene = cvr.Scene.synthetic("cloud", 0, tuple(a.cloud))
        D, _, _ = densify(scene)
        nx, ny, nz = scene.dims
        fields = [(f"cloud proxy, {nx}x{ny}x{nz}, densified", "u16", u16(D / D.max()), 0.0, 65535.0)]
    else:
        scene = cvr.Scene.synthetic("manix")
        d = np.ascontiguousarray(scene.density, np.float32)
        nx, ny, nz = scene.dims
        if a.case == "manix":
            d = d / d.max()
            title = f"manix proxy grid (C2), {nx}x{ny}x{nz}"
            fields = [(title, "u16", u16(d), 0.0, 65535.0), (title, "f32", d, 0.0, 1.0)]
        else:
            r = np.random.default_rng(107).integers(0, 65536, d.shape).astype(np.uint16)
            fields = [(f"uniform random field, {nx}x{ny}x{nz}", "u16", r, 0.0, 65535.0)]
    for title, name, host, lo, hi in fields:
        if a.once and name != a.once:
            continue
        run_field(title, name, host, lo, hi, a.reps, a.routes, out, a.once)
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
