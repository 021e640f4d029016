#!/usr/bin/env python3
"""What the primary-ray feature pass costs, in units of render samples, and the guided filter
against the colour-only one.

  python tools/features_probe.py [--reps 9] [--skip manix|cloud] [--out FILE.md]

One process.  Per scene (the C2 medium, the manix proxy, at 1024^2; the cloud proxy, sparse, at
2048^2; default camera, default cvr_features_desc):
  features   cvr_features_buffers into device tensors, a stream synchronise before and after each
             call, the wall clock around it; calls alternate with the render launches below, one
             unrecorded round first, median (min-max) of `reps`
  sample     cvr_stats.kernel_ms of a 20-sample launch of the same view, divided by 20: the
             render kernel's device time per sample per pixel of the image
  ratio      features / sample: "the guides cost k samples"
and at 1024^2 on the C2 medium, 8 samples with moments: cvr_denoise_buffers against
cvr_denoise_guided_buffers (default descriptors, the feature planes already computed), the same
way.  Before any number is reported the device planes of a 64x64 view must equal
cvr_features_host's bits (dense scene only: the cloud has no dense host arrays)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch  # (before libcvr is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cudavolumerenderer_amd as cvr  # noqa: E402


def med(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f}-{max(v):.3f})"


def timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def probe(name, side, reps, lines):
    scene = cvr.Scene.synthetic(name)
    ctx = cvr.Context(0, "regenerationSK")
    if scene.is_sparse:
        ctx.set_medium_sparse(scene.sparse_medium)
    else:
        ctx.set_medium(scene.medium)
        iv, r2v = cvr.default_camera(64, 64)
        ctx.set_camera(iv, r2v, (64, 64))
        ctx.set_resolution(64, 64)
        got = ctx.features()
        want = cvr.features_host(scene.medium, iv, r2v, (64, 64))
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    iv, r2v = cvr.default_camera(side, side)
    ctx.set_camera(iv, r2v, (side, side))
    ctx.set_resolution(side, side)
    ctx.set_offset(0, 0)
    ctx.set_iterations(20)
    ctx.init()
    rgba = torch.zeros((side, side, 4), device="cuda")
    depth = torch.zeros((side, side), device="cuda")
    torch.cuda.synchronize()
    feat, sample = [], []
    for r in range(reps + 1):
        t = timed(ctx, lambda: ctx.features_buffers(rgba, depth))
        ctx.clear_output()
        ctx.launch_render()
        ctx.synchronize()
        k = ctx.stats().kernel_ms / 20.0
        ctx.reset()
        if r:
            feat.append(t)
            sample.append(k)
    alpha = rgba[..., 3]
    lines.append(f"| {name} {scene.dims} at {side}^2 | {med(feat)} | {med(sample)} | "
                 f"{statistics.median(feat) / statistics.median(sample):.2f} | "
                 f"{float((alpha > 0).float().mean()):.3f} | {float(alpha.mean()):.3f} |")
    if scene.is_sparse:
        ctx.close()
        return
    # the filters, on 8 samples of this view
    ctx.set_iterations(8)
    ctx.set_option(cvr.OPT_MOMENTS, 1)
    ctx.clear_output()
    ctx.launch_render()
    ctx.synchronize()
    s1, s2 = (torch.from_numpy(a).cuda() for a in ctx.copy_moments())
    out = torch.zeros((side, side, 4), device="cuda")
    torch.cuda.synchronize()
    plain, guided = [], []
    for r in range(reps + 1):
        a = timed(ctx, lambda: ctx.denoise_buffers(s1, s2, side, side, out, n_samples=8))
        b = timed(ctx, lambda: ctx.denoise_guided_buffers(s1, s2, rgba, depth, side, side, out, n_samples=8))
        if r:
            plain.append(a)
            guided.append(b)
    lines.append("")
    lines.append(f"filter at {side}^2, 5 passes, ms: colour-only {med(plain)}, guided {med(guided)}, "
                 f"ratio {statistics.median(guided) / statistics.median(plain):.2f}")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip", choices=["manix", "cloud"])
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = ["| scene | features ms | render ms per sample | features / sample | pixels with a chord's opacity | mean opacity |",
             "|---|---|---|---|---|---|"]
    tail = []
    if args.skip != "manix":
        probe("manix", 1024, args.reps, lines)
        tail = lines[-2:]
        del lines[-2:]
    if args.skip != "cloud":
        probe("cloud", 2048, args.reps, lines)
    text = "\n".join(lines + tail) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
