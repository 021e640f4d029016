#!/usr/bin/env python3
"""Run the denoiser's kernels at a frame size, for a profiler or a host clock (needs a GPU).

  python tools/denoise_probe.py [--size 1024] [--passes 5] [--warmup 5] [--reps 50] [--map]

Random sums of 8 samples per pixel (T in [0, 1.5), 20 % zeros) are made on the device with
torch; cvr_denoise_buffers then runs warmup + reps times on them.  Prints the mean wall time of
one call (prepare + passes, host clock around a stream synchronise) as a JSON line.  Kernel
times per pass: run it under `rocprofv3 --kernel-trace --stats -d DIR -- python
tools/denoise_probe.py ...` (the kernels are k_denoise_prepare, k_denoise_pass<false> and
k_denoise_pass<true>; pass k of every call is the (k + 1)-th pass kernel after a prepare), then
`python tools/denoise_probe.py --summarise DIR/..._kernel_trace.csv [WARMUP_CALLS]` for the
time per pass.
--check compares one call with cvr_denoise_host bit for bit (sizes up to 1024)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cudavolumerenderer_amd as cvr  # noqa: E402


def summarise(trace_csv, skip_calls):
    """Mean and median kernel time per position in a call (prepare, pass 0, 1, ...) from a
    rocprofv3 kernel-trace CSV, the first skip_calls calls (warm-up) left out."""
    import csv

    rows = [r for r in csv.DictReader(open(trace_csv)) if "k_denoise" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = []
    for r in rows:
        if "k_denoise_prepare" in r["Kernel_Name"]:
            calls.append([])
        if calls:
            calls[-1].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)  # us
    calls = [c for c in calls[skip_calls:] if len(c) == len(calls[-1])]
    t = np.array(calls)
    names = ["prepare"] + [f"pass {k}" for k in range(t.shape[1] - 1)]
    out = {"calls": len(calls), "mean_us": dict(zip(names, np.round(t.mean(0), 2).tolist())),
           "median_us": dict(zip(names, np.round(np.median(t, 0), 2).tolist())),
           "total_mean_us": round(float(t.sum(1).mean()), 2), "total_median_us": round(float(np.median(t.sum(1))), 2)}
    print(json.dumps(out))
    return 0


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "--summarise":
        return summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 0)
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--map", action="store_true", help="per-block sample counts (8 and 20) instead of a uniform 8")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    n, N = a.size, 8
    g = torch.Generator(device="cuda").manual_seed(1)
    s1 = torch.zeros((n, n, 4), device="cuda")
    s2 = torch.zeros((n, n, 4), device="cuda")
    for _ in range(N):
        T = torch.rand((n, n, 4), device="cuda", generator=g) * 1.5
        T = T * (torch.rand((n, n, 1), device="cuda", generator=g) < 0.8)
        s1 += T
        s2 += T * T
    counts = None
    if a.map:
        counts = torch.full((n // 8, n // 8), 8, dtype=torch.int32, device="cuda")
        counts[:, n // 16:] = 20
    out = torch.empty((n, n, 4), device="cuda")
    var = torch.empty((n, n), device="cuda")
    torch.cuda.synchronize()
    ctx = cvr.Context(0, "regenerationSK")
    desc = cvr.DenoiseDesc(a.passes)

    def call():
        ctx.denoise_buffers(s1, s2, n, n, out, n_samples=None if a.map else N, block_samples=counts, desc=desc,
                            out_var=var)

    for _ in range(a.warmup):
        call()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        call()
    ctx.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / max(a.reps, 1)
    res = {"size": n, "passes": a.passes, "map": a.map, "reps": a.reps, "call_ms": round(ms, 4)}
    if a.check:
        want, wvar = cvr.denoise_host(s1.cpu().numpy(), s2.cpu().numpy(), None if a.map else N,
                                      None if counts is None else counts.cpu().numpy(), desc)
        res["bits_equal"] = bool(np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)) and
                                 np.array_equal(var.cpu().numpy().view(np.uint32), wvar.view(np.uint32)))
    ctx.close()
    print(json.dumps(res))
    return 0 if res.get("bits_equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())
