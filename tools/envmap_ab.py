#!/usr/bin/env python3
"""What an environment map costs: the measurements of profiles/envmap/README.md.

  python tools/envmap_ab.py [--parent-lib build/variants/parent/libcvr.so] [--configs C2 C5]
                            [--launches 5] [--warmup 2] [--out profiles/envmap/README.md]

 (a) with --parent-lib (the library of the commit before the environment instances): the
     benchmark's C2 line (bench.py --gpus 1 --steps 20 --warmup 5) for that library, this build
     and that library again, one process each, and tools/isa_same.py over the two libraries;
 (b) per configuration (C2: manix 1024^2, 20 it; C5: cloud 4096^2, 20 it) one child process,
     regenerationSK on the wave pool with every knob at its default: alternating launches of
     the whole render without an environment and with a 2048x1024 map, `warmup` unrecorded
     pairs, then `launches` recorded ones; cvr_stats.kernel_ms.  With a map the launch runs
     the generic-layout environment instance, so the difference includes what records and
     moments also pay for that layout;
 (c) cvr_set_environment of a 4096x2048 map from a host array and from a resident torch
     tensor, wall clock per call (the call is synchronous);
 (d) per environment instance the registers and scratch the compiler reports (no GPU:
     -Rpass-analysis=kernel-resource-usage on csrc/cvr_wpool.hip with the Makefile's flags).

Every child runs under its own time limit and the first failure stops the run.  Medians
(min-max) are printed as a markdown report (also written to --out).
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {  # name: (synthetic scene, resolution, iterations, child time limit in seconds)
    "C2": ("manix", 1024, 20, 240),
    "C5": ("cloud", 4096, 20, 600),
}
MED_NAMES = {64: "kMedDense + kMedEnv", 65: "kMedSparse + kMedEnv", 81: "kMedSparse + kMedHalf + kMedEnv",
             96: "kMedDense + kMedEnv + kMedMoments", 97: "kMedSparse + kMedEnv + kMedMoments"}


def sky(w, h):
    """A smooth sky with a bright sun: (h, w, 3) float32."""
    import numpy as np
    yy, xx = np.mgrid[0:h, 0:w]
    v = (yy + 0.5) / h
    img = np.empty((h, w, 3), np.float32)
    img[..., 0] = 0.3 + 0.5 * v
    img[..., 1] = 0.5 + 0.3 * v
    img[..., 2] = 1.0 - 0.4 * v
    d2 = ((xx - 0.7 * w) / (0.01 * w)) ** 2 + ((yy - 0.3 * h) / (0.02 * h)) ** 2
    img += (50.0 * np.exp(-d2))[..., None].astype(np.float32)
    return img


def child(name, launches, warmup):
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
    plain, env = ctxs
    env.set_environment(sky(2048, 1024))
    ms = {"plain": [], "env": []}
    for i in range(warmup + launches):
        for key, c in (("plain", plain), ("env", env)):
            c.set_seed(0)
            c.clear_output()
            c.launch_render()
            st = c.stats()  # synchronises
            if i >= warmup:
                ms[key].append(st.kernel_ms)
    print("AB_RESULT " + json.dumps({"config": name, "scene": scene_name, "res": res, "iters": iters, "ms": ms}),
          flush=True)


def child_upload(launches, warmup):
    import torch
    import cudavolumerenderer_amd as cvr
    img = sky(4096, 2048)
    t = torch.from_numpy(img).to("cuda:0")
    torch.cuda.synchronize()
    c = cvr.Context(0, "regenerationSK")
    wall = {"host": [], "device": []}
    for i in range(warmup + launches):
        for key, src in (("host", img), ("device", t)):
            t0 = time.perf_counter()
            c.set_environment(src)
            t1 = time.perf_counter()
            if i >= warmup:
                wall[key].append((t1 - t0) * 1e3)
    info = c.environment_info()
    print("AB_RESULT " + json.dumps({"wall": wall, "bytes": info.bytes, "w": info.width, "h": info.height}), flush=True)


def run_child(args, limit, env=None):
    """The AB_RESULT of a child of this script, or None (with the reason on stderr)."""
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env)
    except subprocess.TimeoutExpired:
        print(f"{args}: no result within {limit} s; stopping", file=sys.stderr)
        return None
    line = [l for l in p.stdout.splitlines() if l.startswith("AB_RESULT ")]
    if p.returncode != 0 or not line:
        print(f"{args}: failed (exit {p.returncode}); stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
        return None
    return json.loads(line[-1][len("AB_RESULT "):])


def bench_line(lib):
    """bench.py's JSON result line for C2 with the library `lib` (None: the in-tree one)."""
    env = dict(os.environ)
    if lib:
        env["CVR_LIB"] = os.path.abspath(lib)
    else:
        env.pop("CVR_LIB", None)
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                           capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print("bench.py: no result within 300 s; stopping", file=sys.stderr)
        return None
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not lines:
        print(f"bench.py failed (exit {p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
        return None
    return json.loads(lines[-1])


def resources():
    """(scatter eps, med, VGPRs, SGPRs, scratch bytes per lane, occupancy) of every environment instance."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS := (.*?)(?<!\\)$", mk, flags=re.M | re.S).group(1).replace("\\\n", " ")
    flags = flags.replace("$(ARCH)", "gfx950").replace("$(CSRC)", "cudavolumerenderer_amd/csrc").split()
    flags += re.search(r"^HIPFLAGS_cvr_wpool := (.*)$", mk, flags=re.M).group(1).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                          "cudavolumerenderer_amd/csrc/cvr_wpool.hip", "-o", os.devnull],
                       capture_output=True, text=True, cwd=ROOT)
    out = []
    for blk in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:]:
        m = re.match(r"\S*k_wpoolILb(\d)ELi(\d)ELi(\d+)ELb(\d)ELb(\d)", blk)
        if not m or not int(m.group(3)) & 64:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))  # noqa: E731
        out.append((int(m.group(1)), int(m.group(3)), get("VGPRs"), get("SGPRs"), get(r"ScratchSize \[bytes/lane\]"),
                    get(r"Occupancy \[waves/SIMD\]")))
    return sorted(out, key=lambda r: (r[1], r[0]))


def fmt_ms(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f}-{max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--configs", nargs="*", default=["C2", "C5"], choices=sorted(CONFIGS))
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-resources", action="store_true", help="skip (d): no compiler on this machine")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)  # the child of one configuration
    a = ap.parse_args()
    if a.one == "upload":
        child_upload(a.launches, a.warmup)
        return 0
    if a.one:
        child(a.one, a.launches, a.warmup)
        return 0
    out = ["# Environment-map lighting: what the map costs", "",
           "`python tools/envmap_ab.py --parent-lib build/variants/parent/libcvr.so`; regenerationSK, wave pool, "
           "every knob at its default; median (min-max).", ""]
    if a.parent_lib:
        same = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_same.py"), a.parent_lib,
                               os.path.join(ROOT, "cudavolumerenderer_amd", "libcvr.so")], capture_output=True, text=True)
        out += ["## The benchmarked instances against the parent's library", "",
                f"`tools/isa_same.py`: {same.stdout.strip().splitlines()[-1] if same.stdout.strip() else 'failed'} "
                f"(exit {same.returncode}).", "",
                "C2 bench line (`bench.py --gpus 1 --steps 20 --warmup 5`), one process each, in this order:", "",
                "| library | result line |", "|---|---|"]
        for label, lib in (("parent", a.parent_lib), ("this build", None), ("parent again", a.parent_lib)):
            r = bench_line(lib)
            if r is None:
                return 1
            out.append(f"| {label} | `{json.dumps(r)}` |")
            print(f"bench {label}: done", file=sys.stderr, flush=True)
        out.append("")
    results = []
    for name in a.configs:
        r = run_child(["--one", name, "--launches", str(a.launches), "--warmup", str(a.warmup)], CONFIGS[name][3])
        if r is None:
            return 1
        results.append(r)
        print(f"{name}: done", file=sys.stderr, flush=True)
    if results:
        out += ["## Kernel time with a 2048x1024 map against no environment (cvr_stats.kernel_ms)", "",
                f"{a.warmup} warm-up pairs, then {a.launches} recorded alternating pairs, two contexts on one medium.", "",
                "| Config | no environment | 2048x1024 map | map / none (medians) |", "|---|---|---|---|"]
        for r in results:
            p, e = r["ms"]["plain"], r["ms"]["env"]
            ratio = statistics.median(e) / statistics.median(p)
            out.append(f"| {r['config']} ({r['scene']} {r['res']}^2, {r['iters']} it) | {fmt_ms(p)} | {fmt_ms(e)} | "
                       f"{ratio:.4f} ({(ratio - 1) * 100:+.2f} %) |")
        out.append("")
    up = run_child(["--one", "upload", "--launches", str(a.launches), "--warmup", str(a.warmup)], 240)
    if up is None:
        return 1
    out += [f"## cvr_set_environment of a {up['w']}x{up['h']} map ({up['bytes'] / 2 ** 20:.0f} MiB stored), wall clock per call (ms)",
            "", "| from a host array (3 channels) | from a resident tensor (3 channels) |", "|---|---|",
            f"| {fmt_ms(up['wall']['host'])} | {fmt_ms(up['wall']['device'])} |", ""]
    if not a.no_resources:
        out += ["## Registers and scratch of the environment instances", "",
                "| instance (5 waves per SIMD, no records, no in-launch output) | scatter -eps | VGPRs | SGPRs | scratch bytes per lane | waves per SIMD |",
                "|---|---|---|---|---|---|"]
        for eps, med, vg, sg, sc, occ in resources():
            out.append(f"| {MED_NAMES.get(med, med)} | {'yes' if eps else 'no'} | {vg} | {sg} | {sc} | {occ} |")
        out.append("")
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
