#!/usr/bin/env python3
"""A/B of medium setup from host memory and from device memory (cvr_set_medium_device).

  python tools/device_medium_ab.py [--reps 5] [--cloud 512 256 512] [--skip manix|cloud] [--out FILE.md]

One process.  Per case the two paths alternate, one unrecorded pair first, then `reps` recorded
pairs; the time is the wall clock around the synchronous call, median (min-max).

  manix  the C2 medium (the manix proxy at its default size), formats 0 and 1:
         cvr_set_medium from host arrays against cvr_set_medium_device from resident tensors.
  cloud  the cloud proxy at --cloud voxels: cvr_scene_sparse_medium + cvr_set_medium_sparse on the
         scene's leaves against cvr_set_medium_device with CVR_DEVMED_SPARSE on the densified
         tensors.  The scene is generated as leaves, so the host side does not pay the
         dense -> leaves pass a host-resident dense volume would need first.

A third context with CVR_OPT_TIMING 1 repeats the device call for the per-kernel device times
(HIP events; timing adds synchronisations, so it is kept out of the wall-time pairs) and their
bytes over time.  Before any number is reported the two contexts of a case must agree in
cvr_medium_info, cvr_medium_layout and the records of 4096 paths."""
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

DEV = "cuda:0"
GROUPS = ("density scan", "albedo scan", "leaf flags", "scans + scatters", "copy / convert / gather",
          "cells + bounds + brick words")


def med(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f}-{max(v):.2f})"


def wall(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def records(ctx):
    tile = (32, 32)
    iv, r2v = cvr.default_camera(*tile)
    ctx.set_camera(iv, r2v, tile)
    ctx.init()
    ctx.set_resolution(*tile)
    ctx.set_iterations(4)
    ctx.set_seed(3)
    ctx.set_path_range(0, 4096)
    return ctx.trace_launch(4096)


def assert_same(host, dev, what):
    assert dev.medium_info().as_dict() == host.medium_info().as_dict(), what
    assert dev.medium_layout().as_dict() == host.medium_layout().as_dict(), what
    assert records(dev).tobytes() == records(host).tobytes(), what
    # the whole stored medium, read back (cvr_debug_copy_medium): the paths touch a sliver of it
    for name in cvr.MEDIUM_ARRAYS:
        h, d = host.debug_medium_array(name), dev.debug_medium_array(name)
        assert (h is None) == (d is None) and (h is None or h.tobytes() == d.tobytes()), f"{what}: stored {name}"


def alternate(host_call, dev_call, reps):
    th, td = [], []
    for i in range(reps + 1):
        a, b = wall(host_call), wall(dev_call)
        if i:
            th.append(a)
            td.append(b)
    return th, td


def kernel_times(fmt, dev_call_on, reps):
    """Median device ms per group of a context with CVR_OPT_TIMING 1."""
    ctx = cvr.Context(0, "regenerationSK")
    ctx.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
    ctx.set_option(cvr.OPT_TIMING, 1)
    rows = []
    for i in range(reps + 1):
        dev_call_on(ctx)
        if i:
            rows.append(ctx.device_medium_ms())
    ctx.close()
    return [statistics.median(r[k] for r in rows) for k in range(6)]


def rate(nbytes, ms):
    return f"{nbytes / 1e6:.0f} MB, {nbytes / ms / 1e9:.2f} TB/s" if ms > 0 else "-"


def manix(reps, out):
    scene = cvr.Scene.synthetic("manix")
    nx, ny, nz = scene.dims
    n = nx * ny * nz
    m = scene.medium
    kw = dict(box_min=tuple(m.box_min), box_max=tuple(m.box_max), scale=m.scale, max_density=m.max_density, g=m.g,
              roughness=tuple(m.roughness), eta=m.eta)
    td = torch.from_numpy(np.ascontiguousarray(scene.density)).to(DEV)
    ta = torch.from_numpy(np.ascontiguousarray(scene.albedo)).to(DEV)
    torch.cuda.synchronize()
    out += [f"## manix proxy (C2's medium), {nx}x{ny}x{nz} = {n} voxels: {4 * n / 1e6:.0f} MB density, "
            f"{16 * n / 1e6:.0f} MB albedo", "",
            "| format | cvr_set_medium (host arrays), ms | cvr_set_medium_device (resident tensors), ms | host / device |",
            "|---|---|---|---|"]
    kern = {}
    for fmt in (0, 1):
        host, dev = cvr.Context(0, "regenerationSK"), cvr.Context(0, "regenerationSK")
        for c in (host, dev):
            c.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
        th, tdv = alternate(lambda: host.set_medium(m), lambda: dev.set_medium_device(td, ta, **kw), reps)
        assert_same(host, dev, f"manix format {fmt}")
        out.append(f"| {fmt} | {med(th)} | {med(tdv)} | {statistics.median(th) / statistics.median(tdv):.1f}x |")
        host.close()
        dev.close()
        kern[fmt] = kernel_times(fmt, lambda c: c.set_medium_device(td, ta, **kw), reps)
    dB = {0: 4, 1: 2}
    out += ["", "Device time per group (CVR_OPT_TIMING 1, HIP events, median), with the bytes each reads and writes:", "",
            "| format | " + " | ".join(GROUPS) + " |", "|---|" + "---|" * 6]
    for fmt in (0, 1):
        k = kern[fmt]
        nbytes = [4 * n, 16 * n, 0, 0, (4 + 16) * n + (dB[fmt] + 4 * dB[fmt]) * n, 0]
        cols = [f"{k[i]:.3f} ms" + (f" ({rate(nbytes[i], k[i])})" if nbytes[i] and k[i] > 0 else "") for i in range(6)]
        out.append(f"| {fmt} | " + " | ".join(cols) + " |")
    out.append("")


def densify(scene):
    table, dens, alb, bg = scene.leaves()
    nx, ny, nz = scene.dims
    lz, ly, lx = table.shape
    D = np.zeros((lz * 8, ly * 8, lx * 8), np.float32)
    A = None
    if alb is not None:
        A = np.empty((lz * 8, ly * 8, lx * 8, 4), np.float32)
        A[:] = np.asarray(bg, np.float32)
    dens = dens.reshape(-1, 8, 8, 8)
    for z, y, x in zip(*np.nonzero(table != 0xFFFFFFFF)):
        s = table[z, y, x]
        D[z * 8:z * 8 + 8, y * 8:y * 8 + 8, x * 8:x * 8 + 8] = dens[s]
        if A is not None:
            A[z * 8:z * 8 + 8, y * 8:y * 8 + 8, x * 8:x * 8 + 8] = alb.reshape(-1, 8, 8, 8, 4)[s]
    D = np.ascontiguousarray(D[:nz, :ny, :nx])
    return D, (None if A is None else np.ascontiguousarray(A[:nz, :ny, :nx])), tuple(float(v) for v in bg)


def cloud(dims, reps, out):
    scene = cvr.Scene.synthetic("cloud", 0, dims)
    assert scene.is_sparse
    nx, ny, nz = scene.dims
    n = nx * ny * nz
    D, A, bg = densify(scene)
    # the rule's background is voxel (0,0,0)'s albedo; the scene's is its own
    const = None if A is not None else bg
    if A is not None:
        assert tuple(float(v) for v in A[0, 0, 0]) == bg, "voxel (0,0,0) does not hold the scene's background"
    sm = scene.sparse_medium
    kw = dict(sparse=True, box_min=tuple(sm.box_min), box_max=tuple(sm.box_max), scale=sm.scale,
              max_density=sm.max_density, g=sm.g, roughness=tuple(sm.roughness), eta=sm.eta, const_albedo=const)
    td = torch.from_numpy(D).to(DEV)
    ta = None if A is None else torch.from_numpy(A).to(DEV)
    torch.cuda.synchronize()
    lib = cvr.load()
    from cudavolumerenderer_amd._lib import SparseMediumDesc
    import ctypes as C

    def host_call(ctx):
        d = SparseMediumDesc()
        assert lib.cvr_scene_sparse_medium(scene._h, C.byref(d)) == 0
        ctx.set_medium_sparse(d)

    n_leaves = int(sm.n_leaves)
    np_ = n_leaves * 512
    out += [f"## cloud proxy, {nx}x{ny}x{nz} = {n} voxels, {n_leaves} of {(nx + 7) // 8 * ((ny + 7) // 8) * ((nz + 7) // 8)} "
            f"leaves stored; albedo: {'per voxel' if A is not None else 'constant (CVR_DEVMED_CONST_ALBEDO)'}", "",
            "| format | cvr_scene_sparse_medium + cvr_set_medium_sparse (host leaves), ms | cvr_set_medium_device, SPARSE "
            "(resident dense tensor), ms | host / device |", "|---|---|---|---|"]
    kern = {}
    for fmt in (0, 1):
        host, dev = cvr.Context(0, "regenerationSK"), cvr.Context(0, "regenerationSK")
        for c in (host, dev):
            c.set_option(cvr.OPT_MEDIUM_FORMAT, fmt)
        th, tdv = alternate(lambda: host_call(host), lambda: dev.set_medium_device(td, ta, **kw), reps)
        assert_same(host, dev, f"cloud format {fmt}")
        out.append(f"| {fmt} | {med(th)} | {med(tdv)} | {statistics.median(th) / statistics.median(tdv):.1f}x |")
        host.close()
        dev.close()
        kern[fmt] = kernel_times(fmt, lambda c: c.set_medium_device(td, ta, **kw), reps)
    out += ["", "Device time per group (CVR_OPT_TIMING 1, HIP events, median), with the bytes each reads and writes:", "",
            "| format | " + " | ".join(GROUPS) + " |", "|---|" + "---|" * 6]
    va = 16 if A is not None else 0
    for fmt in (0, 1):
        k = kern[fmt]
        dB = 4 if fmt == 0 else 2
        nbytes = [4 * n, va * n, (4 + va) * n, 0, np_ * (4 + va) + np_ * (dB + (4 * dB if va else 0)), 0]
        cols = [f"{k[i]:.3f} ms" + (f" ({rate(nbytes[i], k[i])})" if nbytes[i] and k[i] > 0 else "") for i in range(6)]
        out.append(f"| {fmt} | " + " | ".join(cols) + " |")
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cloud", type=int, nargs=3, default=(512, 256, 512))
    ap.add_argument("--skip", choices=("manix", "cloud"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = ["# Medium setup: host arrays against device tensors", "",
           f"`python tools/device_medium_ab.py --reps {a.reps} --cloud {' '.join(str(v) for v in a.cloud)}`: one "
           f"process, the two paths alternating, one unrecorded pair, then {a.reps}; wall time around the "
           "synchronous call in ms, median (min-max).  The two contexts of each row agree in cvr_medium_info, "
           "cvr_medium_layout and the records of 4096 paths (asserted before the row is written).", ""]
    if a.skip != "manix":
        manix(a.reps, out)
        print("manix: done", file=sys.stderr, flush=True)
    if a.skip != "cloud":
        cloud(tuple(a.cloud), a.reps, out)
        print("cloud: done", file=sys.stderr, flush=True)
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
