#!/usr/bin/env python3
"""Device times of the kernels that run the stencil walk (gradient_walk, csrc/cvr_gradient.h) and of
the 1-D histogram, each with its spread, on the C2 medium's grid as u16 and f32.

  [CVR_LIB=OTHER/libcvr.so] python tools/stencil_spread.py OUT.json [--reps 30]

One process, one library.  Per measurement one unrecorded call, then `reps` recorded ones; median
(min-max) in ms, printed and written to OUT.json as [median, min, max].  set_medium_gradient's
kernel groups come from CVR_OPT_TIMING 1 (k_gradient<T, false> is the density scan group,
k_gradient<T, true> the copy / convert / gather group; the cells + bounds + brick words group runs
no walk and shows the noise), field_stats and field_histogram lie between two events on the
context's stream.  gradient_medium_ab.py and field_histogram_ab.py print the groups' medians only;
this gives a comparison of two libraries the spread it needs (profiles/stencil/README.md)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cudavolumerenderer_amd as cvr  # noqa: E402
from device_medium_ab import DEV  # noqa: E402
from field_histogram_ab import event_ms  # noqa: E402
from gradient_medium_ab import make_tables  # noqa: E402
from scalar_medium_ab import new_ctx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--reps", type=int, default=30)
ARGS = ap.parse_args()
REPS = ARGS.reps
scene = cvr.Scene.synthetic("manix")
m = scene.medium
d = np.ascontiguousarray(scene.density, np.float32)
d = d / d.max()
kw = dict(box_min=tuple(m.box_min), box_max=tuple(m.box_max), scale=m.scale, g=m.g, roughness=tuple(m.roughness), eta=m.eta)
table, _ = make_tables(False)
fields = {"u16": (np.ceil(d.astype(np.float64) * 65535).astype(np.uint16), 0.0, 65535.0), "f32": (d, 0.0, 1.0)}
res = {}


def put(key, v):
    res[key] = [statistics.median(v), min(v), max(v)]
    print(f"{key}: {res[key][0]:.4f} ({res[key][1]:.4f}-{res[key][2]:.4f})", flush=True)


for name, (host, lo, hi) in fields.items():
    ts = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
    torch.cuda.synchronize()
    for fmt in (0, 1):
        ctx = new_ctx(fmt, 1)
        rows = []
        for i in range(REPS + 1):
            ctx.set_medium_gradient(ts, table, lo=lo, hi=hi, glo=0.0, ghi=0.05 * (hi - lo), spacing=(1.0, 1.0, 1.0), **kw)
            if i:
                rows.append(ctx.device_medium_ms())
        ctx.close()
        put(f"{name} fmt {fmt} k_gradient<T, false> (density scan group)", [r[0] for r in rows])
        put(f"{name} fmt {fmt} k_gradient<T, true> (copy / convert / gather group)", [r[4] for r in rows])
        put(f"{name} fmt {fmt} cells + bounds + brick words (kernels not touched)", [r[5] for r in rows])
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    st = ctx.field_stats(ts)
    put(f"{name} field_stats (events round the synchronous call)", [event_ms(lambda: ctx.field_stats(ts)) for _ in range(REPS + 1)][1:])
    for n, mm in ((64, 64), (256, 256), (256, 1), (65536, 1)):
        out = torch.empty(n * mm, dtype=torch.int32, device=DEV)
        f = lambda: ctx.field_histogram(ts, n, mm, lo=lo, hi=hi, glo=0.0, ghi=float(st.gmax), out=out)  # noqa: E731
        put(f"{name} field_histogram {n} x {mm} (events)", [event_ms(f) for _ in range(REPS + 1)][1:])
    ctx.close()
    del ts
with open(ARGS.out, "w") as fo:
    json.dump(res, fo, indent=1)
