#!/usr/bin/env python3
"""A/B of the medium storage formats (CVR_OPT_MEDIUM_FORMAT 0 fp32 / 1 half) on the
benchmark configurations C2 (manix 1024^2, 20 it), C3 (hetvol 1024^2, 20 it) and C5
(cloud 4096^2, 20 it).

  python tools/medium_format_ab.py [--configs C2 C3 C5] [--launches 10] [--warmup 3] [--out FILE.md]

Per configuration one child process (its own time limit; the first failure stops the
run) sets the medium once per format in two contexts, then alternates format-0 and
format-1 launches of the whole render (regenerationSK, the wave pool, every knob at its
default): `warmup` unrecorded pairs, then `launches` recorded pairs.  Reported: median
and min-max of cvr_stats.kernel_ms per format, the launch counters (which differ
between the formats: format 1 renders the rounded medium), and cvr_medium_info's device
bytes.  Prints a markdown report (also written to --out).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {  # name: (synthetic scene, resolution, iterations, child time limit in seconds)
    "C2": ("manix", 1024, 20, 240),
    "C3": ("hetvol", 1024, 20, 180),
    "C5": ("cloud", 4096, 20, 900),
}


def child(name, launches, warmup):
    import cudavolumerenderer_amd as cvr
    scene_name, res, iters, _ = CONFIGS[name]
    scene = cvr.Scene.synthetic(scene_name)
    iv, r2v = cvr.default_camera(res, res)
    ctxs, info = {}, {}
    for fmt in (cvr.FORMAT_F32, cvr.FORMAT_F16):
        c = cvr.Context(0, "regenerationSK")
        c.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
        if scene.is_sparse:
            c.set_medium_sparse(scene.sparse_medium)
        else:
            c.set_medium(scene.medium)
        c.set_camera(iv, r2v, (res, res))
        c.init()
        c.set_resolution(res, res)
        c.set_iterations(iters)
        ctxs[fmt] = c
        info[fmt] = c.medium_info().as_dict()
    ms = {0: [], 1: []}
    stats = {}
    for i in range(warmup + launches):
        for fmt in (0, 1):
            c = ctxs[fmt]
            c.set_seed(0)
            c.clear_output()
            c.launch_render()
            st = c.stats()  # synchronises
            if i >= warmup:
                ms[fmt].append(st.kernel_ms)
            stats[fmt] = {k: getattr(st, k) for k in ("paths", "segments", "steps", "density", "albedo", "fetches")}
    print("AB_RESULT " + json.dumps({"config": name, "scene": scene_name, "res": res, "iters": iters, "ms": ms,
                                     "info": info, "stats": stats}), flush=True)


def fmt_ms(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f}-{max(v):.3f})"


def report(results, launches, warmup):
    out = ["# Medium storage format A/B: fp32 (format 0) vs half (format 1)", "",
           f"`python tools/medium_format_ab.py`: per configuration one process, the medium set once per format, "
           f"{warmup} warm-up pairs, then {launches} alternating format-0 / format-1 launches of the whole render "
           "(regenerationSK, wave pool, defaults).  `kernel_ms` is cvr_stats.kernel_ms (HIP events around the "
           "launch): median (min-max).", "",
           "| Config | format 0 kernel_ms | format 1 kernel_ms | format 1 / format 0 (medians) |", "|---|---|---|---|"]
    for r in results:
        m0, m1 = r["ms"]["0"], r["ms"]["1"]
        ratio = statistics.median(m1) / statistics.median(m0)
        out.append(f"| {r['config']} ({r['scene']} {r['res']}^2, {r['iters']} it) | {fmt_ms(m0)} | {fmt_ms(m1)} | "
                   f"{ratio:.4f} ({(ratio - 1) * 100:+.2f} %) |")
    out += ["", "Device bytes (cvr_medium_info):", "",
            "| Config | format | density | cells | albedo | bounds / words | total | max_density_eff |",
            "|---|---|---|---|---|---|---|---|"]
    for r in results:
        for f in ("0", "1"):
            i = r["info"][f]
            out.append(f"| {r['config']} | {f} | {i['density_bytes']} | {i['cells_bytes']} | {i['albedo_bytes']} | "
                       f"{i['bounds_bytes']} | {i['total_bytes']} | {i['max_density_eff']:.9g} |")
    out += ["", "Launch counters (format 1 renders the rounded medium, so they differ slightly):", "",
            "| Config | format | paths | segments | Woodcock steps | cell fetches | albedo lookups |",
            "|---|---|---|---|---|---|---|"]
    for r in results:
        for f in ("0", "1"):
            s = r["stats"][f]
            out.append(f"| {r['config']} | {f} | {s['paths']} | {s['segments']} | {s['steps']} | {s['fetches']} | "
                       f"{s['albedo']} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["C2", "C3", "C5"], choices=sorted(CONFIGS))
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)  # the child of one configuration
    a = ap.parse_args()
    if a.launches < 10 or a.warmup < 3:
        ap.error("at least 10 launches after 3 warm-ups")
    if a.one:
        child(a.one, a.launches, a.warmup)
        return 0
    results = []
    for name in a.configs:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--launches", str(a.launches), "--warmup",
               str(a.warmup)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=CONFIGS[name][3])
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {CONFIGS[name][3]} s; stopping", file=sys.stderr)
            return 1
        line = [l for l in p.stdout.splitlines() if l.startswith("AB_RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{name}: failed (exit {p.returncode}); stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}",
                  file=sys.stderr)
            return 1
        results.append(json.loads(line[-1][len("AB_RESULT "):]))
        print(f"{name}: done", file=sys.stderr, flush=True)
    text = report(results, a.launches, a.warmup)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
