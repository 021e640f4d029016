#!/usr/bin/env python3
"""What the light volume costs to build and what its lookup adds to the preview.

  python tools/shadow_probe.py [--reps 5] [--skip manix|cloud] [--build-only] [--out FILE.md]

One process.  Before any number is reported a 13x11x9 light volume of the C2 medium must equal
cvr_light_volume_host's bits, and the shadowed image of a 40x24 tile at offset (8, 8) of a 64x48 view
cvr_preview_shadowed_host's, shaded and unshaded.  Then, default march descriptors throughout:
  build      cvr_build_light_volume (k_light_volume) for the light (0.3, 1.0, -0.4): the C2 medium
             (manix proxy) with 128x115x128 and 256x230x256 nodes, the cloud proxy (sparse) with its
             default grid; and, next to each, cvr_features_buffers (k_features) at the scene's
             resolution, the march the build repeats per node
  preview    cvr_preview_buffers against cvr_preview_shadowed_buffers (shadow 0.7, the scene's
             default grid), shaded with the same directional light and unshaded: the C2 medium at
             1024^2, the cloud proxy at 2048^2
Device time between two HIP events on the context's stream around each call; the calls alternate,
one unrecorded round first; median (min-max) of `reps`, in ms.
--build-only times the builds alone: the other lane mapping (`make variant NAME=shadowrows
DEFS=-DCVR_SHADOW_ROWS=1`, CVR_LIB names its library)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch  # (before libcvr is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cudavolumerenderer_amd as cvr  # noqa: E402

LIGHT = (0.3, 1.0, -0.4)


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
        vd = ctx.build_light_volume(LIGHT, (13, 11, 9))
        S = cvr.light_volume_host(scene.medium, vd)
        assert np.array_equal(bits(ctx.light_volume()), bits(S)), "the device volume differs from cvr_light_volume_host"
        assert (S < 0.5).any()
        for desc in (cvr.PreviewDesc(flags=0), cvr.PreviewDesc(flags=cvr.PREVIEW_UNSHADED)):
            got = ctx.preview_shadowed(desc, 0.7)
            want = cvr.preview_shadowed_host(scene.medium, iv, r2v, (64, 48), vd, S, (40, 24), (8, 8), 0, desc, 0.7)
            assert np.array_equal(bits(got), bits(want)), "the device image differs from cvr_preview_shadowed_host"
            assert (got[..., 3] > 0).any()
    finally:
        ctx.close()


def timed(stream, calls, reps):
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
    return ms


def probe(name, side, grids, reps, build_only, build_lines, preview_lines):
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
    for res in grids:
        calls[res] = lambda res=res: ctx.build_light_volume(LIGHT, res)
    ms = timed(stream, calls, reps)
    f = statistics.median(ms["features"])
    for res in grids:
        used = tuple(ctx.build_light_volume(LIGHT, res).res)
        nodes = used[0] * used[1] * used[2]
        b = statistics.median(ms[res])
        build_lines.append(f"| {name} {scene.dims} | {used[0]}x{used[1]}x{used[2]} | {med(ms[res])} | {b * 1e6 / nodes:.2f} | "
                           f"{med(ms['features'])} | {f * 1e6 / (side * side):.2f} |")
    if not build_only:
        ctx.build_light_volume(LIGHT)
        lit, flat = cvr.PreviewDesc(light=LIGHT), cvr.PreviewDesc(flags=cvr.PREVIEW_UNSHADED)
        ms = timed(stream, {
            "shaded": lambda: ctx.preview_buffers(rgba, lit),
            "shaded+s": lambda: ctx.preview_shadowed_buffers(rgba, lit, 0.7),
            "unshaded": lambda: ctx.preview_buffers(rgba, flat),
            "unshaded+s": lambda: ctx.preview_shadowed_buffers(rgba, flat, 0.7),
        }, reps)
        m = {k: statistics.median(v) for k, v in ms.items()}
        preview_lines.append(f"| {name} {scene.dims} at {side}^2 | {med(ms['shaded'])} | {med(ms['shaded+s'])} | "
                             f"{m['shaded+s'] / m['shaded']:.2f} | {med(ms['unshaded'])} | {med(ms['unshaded+s'])} | "
                             f"{m['unshaded+s'] / m['unshaded']:.2f} |")
    ctx.set_stream(None)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", choices=["manix", "cloud"])
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    check_equals_host()
    build_lines = ["| scene | light grid | build ms | ns per node | features ms | ns per pixel |", "|---|---|---|---|---|---|"]
    preview_lines = ["| scene | shaded ms | shaded, shadowed ms | ratio | unshaded ms | unshaded, shadowed ms | ratio |",
                     "|---|---|---|---|---|---|---|"]
    if args.skip != "manix":
        probe("manix", 1024, [(128, 115, 128), (256, 230, 256)], args.reps, args.build_only, build_lines, preview_lines)
    if args.skip != "cloud":
        probe("cloud", 2048, [None], args.reps, args.build_only, build_lines, preview_lines)
    text = "\n".join(build_lines) + "\n"
    if not args.build_only:
        text += "\n" + "\n".join(preview_lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
