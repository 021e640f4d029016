#!/usr/bin/env python3
"""What the field projections cost, against the preview pass that marches like them and against
the torch ops that were the only route to a MIP of a resident tensor before.

  python tools/project_probe.py [--reps 5] [--skip c2|cloud] [--no-torch] [--counters] [--out FILE.md]

One process.  Before any number is reported, per field, the device planes of a 64x64 tile in the
middle of the view must equal cvr_field_project_host's bits in every mode.  Fields (procedural: a
product of sines under a radial window, so rays see a full range of values): C2's grid 256x230x256
as uint16 and float32 at 1024^2, the cloud proxy's 512x256x512 as uint8 at 2048^2; the unit box, the
default camera, the default descriptor (step 1, refine 4, the headlight).
  max, min, mean, iso   cvr_field_project_buffers, all three planes (k_project)
  preview               (a) cvr_preview_buffers, CVR_PREVIEW_UNSHADED, t_stop 0, of the medium
                        cvr_set_medium_scalar builds from the same field through a grey ramp: the
                        same march with a density and an albedo lookup per step
Device time between two HIP events on the context's stream around each call; the calls alternate,
one unrecorded round first; median (min-max) of `reps`, in ms.
  torch                 (b) the MIP by torch ops on the resident tensor: per step one grid_sample
                        (align_corners, the node-centred coordinate of the pass) of all rays and a
                        running maximum under the chord's mask; wall time of one run after a warm-up
                        of 8 steps, and the peak of torch's allocated memory above the field itself
--counters: nothing but one k_project launch per mode and field (for a counter run, which must
collect nothing else: rocprofv3 --pmc FETCH_SIZE -- python tools/project_probe.py --counters)."""
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

MODES = ("max", "min", "mean", "iso")
FIELDS = {"c2_u16": ((256, 230, 256), np.uint16, 1024), "c2_f32": ((256, 230, 256), np.float32, 1024),
          "cloud_u8": ((512, 256, 512), np.uint8, 2048)}


def med(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f}-{max(v):.3f})"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_field(dims, dtype):
    """(z, y, x): 0.5 + 0.5 sin sin sin under a radial window, scaled to the type's range."""
    nx, ny, nz = dims
    x = np.linspace(-1, 1, nx, dtype=np.float32)[None, None, :]
    y = np.linspace(-1, 1, ny, dtype=np.float32)[None, :, None]
    z = np.linspace(-1, 1, nz, dtype=np.float32)[:, None, None]
    v = (0.5 + 0.5 * np.sin(7 * x) * np.sin(5 * y + 1) * np.sin(6 * z + 2)) * np.clip(1.2 - (x * x + y * y + z * z), 0, 1)
    top = 1.0 if dtype == np.float32 else float(np.iinfo(dtype).max)
    return np.ascontiguousarray((v * np.float32(top)).astype(dtype)), top


def descs(top):
    return {m: cvr.ProjectDesc(m, lo=0.0, hi=top, iso=0.4 * top) for m in MODES}


def check_equals_host(ctx, a, t, top, side):
    iv, r2v = cvr.default_camera(side, side)
    off = (side // 2 - 32, side // 2 - 32)
    ctx.set_resolution(64, 64)
    ctx.set_offset(*off)
    for mode, d in descs(top).items():
        got = ctx.field_project(t, d)
        want = cvr.field_project_host(a, iv, r2v, (side, side), d, (64, 64), off)
        for g, w, name in zip(got, want, ("rgba", "value", "depth")):
            assert np.array_equal(bits(g), bits(w)), f"{mode}: the device {name} plane differs from cvr_field_project_host"
        assert (got[0][..., 3] == 1).any()
    ctx.set_resolution(side, side)
    ctx.set_offset(0, 0)


def torch_mip(t, iv, r2v, side, steps=None):
    """The MIP of tensor t (z, y, x) in the unit box by torch ops -> (value (side, side), steps)."""
    dev = t.device
    M = torch.tensor(np.asarray(iv, np.float32).reshape(3, 4), device=dev)
    px = torch.arange(side, device=dev, dtype=torch.float32) + 0.5
    rx = float(r2v[0]) * (px * 2 / side - 1)
    ry = float(r2v[1]) * (px * 2 / side - 1)
    v = torch.stack([rx[None, :].expand(side, side), ry[:, None].expand(side, side), torch.ones((side, side), device=dev)], -1)
    v = v / v.norm(dim=-1, keepdim=True)
    d = v @ M[:, :3].T
    o = M[:, 3]
    inv = 1.0 / d
    ta, tb = (-0.5 - o) * inv, (0.5 - o) * inv
    t0 = torch.minimum(ta, tb).amax(-1).clamp_min(0)
    t1 = torch.maximum(ta, tb).amin(-1)
    nz, ny, nx = t.shape
    delta = min(1.0 / nx, 1.0 / ny, 1.0 / nz)
    n = int(np.ceil(np.sqrt(3.0) / delta)) if steps is None else steps
    # grid_sample takes floats: four bytes per voxel of temporary (uint16 goes through int32 first)
    wide = (t.view(torch.int16).to(torch.int32) & 0xFFFF) if t.dtype == torch.uint16 else t
    vol = wide.to(torch.float32)[None, None]
    del wide
    best = torch.full((side, side), -float("inf"), device=dev)
    for i in range(n):
        ti = t0 + (i + 0.5) * delta
        p = o + ti[..., None] * d
        s = torch.nn.functional.grid_sample(vol, (p * 2)[None, None], mode="bilinear", padding_mode="border",
                                            align_corners=True)[0, 0, 0]
        best = torch.where(ti < t1, torch.maximum(best, s), best)
    return best, n


def probe(name, reps, with_torch, counters, lines):
    dims, dtype, side = FIELDS[name]
    a, top = make_field(dims, dtype)
    t = torch.from_numpy(a).cuda()
    ctx = cvr.Context(0, "regenerationSK")
    iv, r2v = cvr.default_camera(side, side)
    ctx.set_camera(iv, r2v, (side, side))
    ctx.set_resolution(side, side)
    ctx.set_offset(0, 0)
    rgba = torch.zeros((side, side, 4), device="cuda")
    value, depth = torch.zeros((side, side), device="cuda"), torch.zeros((side, side), device="cuda")
    torch.cuda.synchronize()
    ds = descs(top)
    if counters:
        for m in MODES:
            ctx.field_project_buffers(t, rgba, value, depth, ds[m])
            ctx.synchronize()
        ctx.close()
        return
    check_equals_host(ctx, a, t, top, side)
    ramp = np.zeros((256, 4), np.float32)
    ramp[:, :3] = 0.8
    ramp[:, 3] = np.linspace(0.0, 1.0, 256, dtype=np.float32)
    try:
        ctx.set_medium_scalar(t, ramp, lo=0.0, hi=top, scale=40.0, max_density=1.0)
        have_medium = True
    except cvr.CvrError as e:  # (a grid the dense build refuses: the projections still run)
        print(f"{name}: no medium for the preview column: {e}")
        have_medium = False
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    flat = cvr.PreviewDesc(cvr.FeaturesDesc(1.0, 0.0, 4096), flags=cvr.PREVIEW_UNSHADED)
    calls = {m: (lambda m=m: ctx.field_project_buffers(t, rgba, value, depth, ds[m])) for m in MODES}
    if have_medium:
        calls["preview"] = lambda: ctx.preview_buffers(rgba, flat)
    ms = {k: [] for k in calls}
    for r in range(reps + 1):
        for k, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            if r:
                ms[k].append(e0.elapsed_time(e1))
    ctx.set_stream(None)
    ctx.close()
    row = f"| {name} {dims[0]}x{dims[1]}x{dims[2]} at {side}^2 | " + " | ".join(med(ms[k]) for k in MODES)
    if have_medium:
        row += f" | {med(ms['preview'])} | {statistics.median(ms['max']) / statistics.median(ms['preview']):.2f} |"
    else:
        row += " | n/a | n/a |"
    if with_torch:
        torch_mip(t, iv, r2v, side, steps=8)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        w0 = time.perf_counter()
        best, n = torch_mip(t, iv, r2v, side)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - w0) * 1e3
        peak = torch.cuda.max_memory_allocated() - base
        row += f" {wall:.0f} ({n} steps) | {peak / 2 ** 20:.0f} MiB ({peak / a.nbytes:.1f} fields) | {wall / statistics.median(ms['max']):.0f} |"
    lines.append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", choices=["c2", "cloud"])
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--counters", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    head = "| field | max ms | min ms | mean ms | iso ms | preview ms | max / preview |"
    rule = "|---|---|---|---|---|---|---|"
    if not args.no_torch:
        head += " torch MIP wall ms | torch peak memory | torch / max |"
        rule += "---|---|---|"
    lines = [head, rule]
    for name in FIELDS:
        if args.skip and name.startswith(args.skip):
            continue
        probe(name, args.reps, not args.no_torch, args.counters, lines)
    if args.counters:
        return
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
