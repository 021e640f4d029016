#!/usr/bin/env python3
"""Cost and gain of adaptive sampling on the benchmark configurations C2 (manix 1024^2,
20 it) and C5 (cloud 4096^2, 20 it).

  python tools/adaptive_ab.py [--configs C2 C5] [--launches 10] [--warmup 3] [--out FILE.md]

Per configuration one child process (its own time limit; the first failure stops the run),
regenerationSK on the wave pool with every knob at its default, two contexts on one medium:

 (a) the moments instance against the plain instance: alternating launches of the whole
     render with CVR_OPT_MOMENTS 0 (the instance cvr_launch_render picks by default) and 1,
     `warmup` unrecorded pairs, then `launches` recorded ones; cvr_stats.kernel_ms.
 (b) the adaptive render against the uniform one: the noise target is the worst finite
     8x8-block error (cvr_block_error, floor 0.01) that the uniform 20-iteration render
     reaches, so both end with the same worst block; min 8, 4 per pass, at most 20
     samples.  Alternating cvr_render_frame (moments off, into a pinned image: the
     in-launch output) and cvr_render_adaptive (into a pinned image) calls, wall clock
     around each call; also the paths traced and the passes.

Medians (min-max) are printed as a markdown report (also written to --out).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {  # name: (synthetic scene, resolution, iterations, child time limit in seconds)
    "C2": ("manix", 1024, 20, 240),
    "C5": ("cloud", 4096, 20, 900),
}
FLOOR, MIN_IT, PASS_IT = 0.01, 8, 4


def block_errors(s1, s2, n, floor):
    """cvr_block_error for every 8x8 block of (h, w, 4) sums, vectorised in fp64."""
    import numpy as np
    h, w = s1.shape[:2]
    a = s1[..., :3].astype(np.float64)
    b = s2[..., :3].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = a / n
        v = np.maximum(0.0, b / n - m * m) / (n - 1.0)
        den = m.sum(-1) + np.float64(np.float32(floor))
        e = np.sqrt(v.sum(-1)) / den
    e = np.where(den == 0.0, 0.0, e)
    e = np.where(np.isfinite(a).all(-1) & np.isfinite(b).all(-1) & ~np.isnan(e), e, np.inf)
    return e.reshape(h // 8, 8, w // 8, 8).mean(axis=(1, 3))


def child(name, launches, warmup):
    import numpy as np
    import cudavolumerenderer_amd as cvr
    scene_name, res, iters, _ = CONFIGS[name]
    scene = cvr.Scene.synthetic(scene_name)
    iv, r2v = cvr.default_camera(res, res)
    ctxs = []
    for k in range(2):
        c = cvr.Context(0, "regenerationSK")
        if k:
            c.share_medium(ctxs[0])
        elif scene.is_sparse:
            c.set_medium_sparse(scene.sparse_medium)
        else:
            c.set_medium(scene.medium)
        c.set_camera(iv, r2v, (res, res))
        c.init()
        c.set_resolution(res, res)
        c.set_iterations(iters)
        ctxs.append(c)
    plain, mom = ctxs
    mom.set_option(cvr.OPT_MOMENTS, 1)
    # (a) kernel time, alternating
    ms = {"plain": [], "moments": []}
    for i in range(warmup + launches):
        for key, c in (("plain", plain), ("moments", mom)):
            c.set_seed(0)
            c.clear_output()
            c.launch_render()
            st = c.stats()  # synchronises
            if i >= warmup:
                ms[key].append(st.kernel_ms)
    # the uniform render's worst block (the moments context holds the 20-iteration sums of seed 0)
    s1, s2 = mom.copy_moments()
    e = block_errors(s1, s2, iters, FLOOR)
    finite = np.isfinite(e)
    target = float(e[finite].max())
    quiet = float((e[finite] <= 0.25 * target).mean())
    mom.set_option(cvr.OPT_MOMENTS, 0)
    # (b) wall time, alternating
    desc = cvr.AdaptiveDesc(MIN_IT, iters, PASS_IT, target, FLOOR)
    wall = {"uniform": [], "adaptive": []}
    pin_u, pin_a = cvr.PinnedImage(res, res), cvr.PinnedImage(res, res)
    info = {}
    for i in range(warmup + launches):
        plain.set_seed(0)
        t0 = time.perf_counter()
        plain.render_frame(pin_u, 1, stats=False)
        t1 = time.perf_counter()
        mom.set_seed(0)
        t2 = time.perf_counter()
        _, r, err, smp = mom.render_adaptive(desc, pin_a)
        t3 = time.perf_counter()
        if i >= warmup:
            wall["uniform"].append((t1 - t0) * 1e3)
            wall["adaptive"].append((t3 - t2) * 1e3)
        info = {"passes": r.passes, "paths": r.paths, "max_error": r.max_error, "mean_error": r.mean_error,
                "kernel_ms": mom.adaptive_stats.kernel_ms,
                "samples": {int(k): int((smp == k).sum()) for k in np.unique(smp)}}
    flushed = plain.frame_flush_info()[0]
    pin_u.close()
    pin_a.close()
    print("AB_RESULT " + json.dumps({"config": name, "scene": scene_name, "res": res, "iters": iters, "ms": ms,
                                     "wall": wall, "target": target, "nonfinite_blocks": int((~finite).sum()),
                                     "blocks": int(e.size), "quiet_share": quiet, "adaptive": info,
                                     "uniform_paths": res * res * iters, "flushed_blocks": flushed}), flush=True)


def fmt_ms(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f}-{max(v):.3f})"


def report(results, launches, warmup):
    out = ["# Adaptive sampling: the cost of the moments and the gain of the adaptive render", "",
           f"`python tools/adaptive_ab.py`: per configuration one process, two contexts on one medium, {warmup} "
           f"warm-up pairs, then {launches} recorded alternating pairs; median (min-max), regenerationSK, wave "
           "pool, defaults.", "",
           "## (a) The moments instance against the plain one (cvr_stats.kernel_ms of the whole launch)", "",
           "| Config | plain kernel_ms | moments kernel_ms | moments / plain (medians) |", "|---|---|---|---|"]
    for r in results:
        p, m = r["ms"]["plain"], r["ms"]["moments"]
        ratio = statistics.median(m) / statistics.median(p)
        out.append(f"| {r['config']} ({r['scene']} {r['res']}^2, {r['iters']} it) | {fmt_ms(p)} | {fmt_ms(m)} | "
                   f"{ratio:.4f} ({(ratio - 1) * 100:+.2f} %) |")
    out += ["", "## (b) cvr_render_adaptive against the uniform cvr_render_frame (wall clock per call, ms)", "",
            f"Target: the worst finite block error of the uniform render; min {MIN_IT}, {PASS_IT} per pass, the "
            "uniform iteration count as the cap; floor 0.01.", "",
            "| Config | target | uniform wall | adaptive wall | adaptive / uniform | paths traced (share of uniform) "
            "| passes | blocks by final samples | summed launch kernel_ms |", "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        u, a, ad = r["wall"]["uniform"], r["wall"]["adaptive"], r["adaptive"]
        ratio = statistics.median(a) / statistics.median(u)
        out.append(f"| {r['config']} | {r['target']:.5g} | {fmt_ms(u)} | {fmt_ms(a)} | {ratio:.4f} "
                   f"({(ratio - 1) * 100:+.2f} %) | {ad['paths']} ({100.0 * ad['paths'] / r['uniform_paths']:.1f} %) | "
                   f"{ad['passes']} | {ad['samples']} | {ad['kernel_ms']:.3f} |")
    out += [""]
    for r in results:
        out.append(f"- {r['config']}: {r['blocks']} blocks, {r['nonfinite_blocks']} with a non-finite error (NaN pixels: "
                   f"never converge, left out of the target); {100.0 * r['quiet_share']:.1f} % of the blocks are at or "
                   f"below a quarter of the target after the uniform render; the uniform call stored "
                   f"{r['flushed_blocks']} blocks inside its launch.")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["C2", "C5"], choices=sorted(CONFIGS))
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
