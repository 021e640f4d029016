#!/usr/bin/env python3
"""What the shaded preview pass costs against the feature pass it marches like.

  python tools/preview_probe.py [--reps 5] [--skip manix|cloud] [--features-only] [--out FILE.md]

One process.  Before any number is reported the device image of a 40x24 tile at offset (8, 8) of a
64x48 view of the C2 medium must equal cvr_preview_host's bits, shaded and unshaded.  Then, per
scene (the C2 medium, the manix proxy, at 1024^2; the cloud proxy, sparse, at 2048^2; default
camera, default descriptors, one march descriptor for all three kernels):
  features   cvr_features_buffers (k_features)
  unshaded   cvr_preview_buffers with CVR_PREVIEW_UNSHADED (k_preview<false>)
  shaded     cvr_preview_buffers with the default descriptor (k_preview<true>)
Device time between two HIP events on the context's stream around each call; the three calls
alternate, one unrecorded round first; median (min-max) of `reps`, in ms.
--features-only times k_features alone: the yardstick on a library that has no preview pass
(CVR_LIB names the library of another commit)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch  # (before libcvr is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cudavolumerenderer_amd as cvr  # noqa: E402


def med(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f}-{max(v):.3f})"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_equals_host():
    scene = cvr.Scene.synthetic("manix")
    ctx = cvr.Context(0, "regenerationSK")
    try:
        ctx.set_medium(scene.medium)
        iv, r2v = cvr.default_camera(64, 48)
        ctx.set_camera(iv, r2v, (64, 48))
        ctx.set_resolution(40, 24)
        ctx.set_offset(8, 8)
        md = scene.medium  # (a float medium: the majorant in use is the scene's)
        for desc in (cvr.PreviewDesc(), cvr.PreviewDesc(flags=cvr.PREVIEW_UNSHADED)):
            got = ctx.preview(desc)
            want = cvr.preview_host(md, iv, r2v, (64, 48), (40, 24), (8, 8), 0, desc)
            assert np.array_equal(bits(got), bits(want)), "the device image differs from cvr_preview_host"
            assert (got[..., 3] > 0).any()
    finally:
        ctx.close()


def probe(name, side, reps, features_only, lines):
    scene = cvr.Scene.synthetic(name)
    ctx = cvr.Context(0, "regenerationSK")
    if scene.is_sparse:
        ctx.set_medium_sparse(scene.sparse_medium)
    else:
        ctx.set_medium(scene.medium)
    iv, r2v = cvr.default_camera(side, side)
    ctx.set_camera(iv, r2v, (side, side))
    ctx.set_resolution(side, side)
    ctx.set_offset(0, 0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    rgba = torch.zeros((side, side, 4), device="cuda")
    depth = torch.zeros((side, side), device="cuda")
    torch.cuda.synchronize()
    calls = {"features": lambda: ctx.features_buffers(rgba, depth)}
    if not features_only:
        flat, lit = cvr.PreviewDesc(flags=cvr.PREVIEW_UNSHADED), cvr.PreviewDesc()
        calls["unshaded"] = lambda: ctx.preview_buffers(rgba, flat)
        calls["shaded"] = lambda: ctx.preview_buffers(rgba, lit)
    ms = {k: [] for k in calls}
    for r in range(reps + 1):
        for k, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            if r:
                ms[k].append(a.elapsed_time(b))
    row = f"| {name} {scene.dims} at {side}^2 | {med(ms['features'])} |"
    if not features_only:
        f, u, s = (statistics.median(ms[k]) for k in ("features", "unshaded", "shaded"))
        row += f" {med(ms['unshaded'])} | {med(ms['shaded'])} | {u / f:.2f} | {s / u:.2f} |"
    lines.append(row)
    ctx.set_stream(None)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", choices=["manix", "cloud"])
    ap.add_argument("--features-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.features_only:
        lines = ["| scene | features ms |", "|---|---|"]
    else:
        check_equals_host()
        lines = ["| scene | features ms | unshaded ms | shaded ms | unshaded / features | shaded / unshaded |", "|---|---|---|---|---|---|"]
    if args.skip != "manix":
        probe("manix", 1024, args.reps, args.features_only, lines)
    if args.skip != "cloud":
        probe("cloud", 2048, args.reps, args.features_only, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
