#!/usr/bin/env python3
"""Event batches and regeneration of k_wpool launches, from the CVR_WPOOL_REGENSTAT diagnostic
build (never the shipped library):
  make variant NAME=rstat DEFS=-DCVR_WPOOL_REGENSTAT=1
  make variant NAME=rstat0 DEFS="-DCVR_WPOOL_REGENSTAT=1 -DCVR_WPOOL_REGEN_PHASE=0"   (in-batch regeneration)
  CVR_LIB=build/variants/rstat/libcvr.so python3 tools/regen_stats.py [--scene manix]
Per launch: batches, their boundary / collision / new parts, regeneration runs and their
width, camera paths that missed the box, free slots at the event trigger."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cudavolumerenderer_amd as cvr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="manix")
ap.add_argument("--res", type=int, default=1024)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=2)
a = ap.parse_args()
lib = cvr.load()
lib.cvr_debug_regenstats.argtypes = [C.c_void_p, C.c_int]
scene = cvr.Scene.synthetic(a.scene)
W = H = a.res
iv, r2v = cvr.default_camera(W, H)
c = cvr.Context(0, "regenerationSK")
if scene.is_sparse:
    c.set_medium_sparse(scene.sparse_medium)
else:
    c.set_medium(scene.medium)
c.set_camera(iv, r2v, (W, H))
c.set_option(cvr.OPT_INFLIGHT, 1)
c.init()
c.set_resolution(W, H)
c.set_iterations(a.iters)
buf = (C.c_uint64 * 16)()
for rep in range(a.reps):
    lib.cvr_debug_regenstats(buf, 1)
    c.clear_output()
    c.launch_render()
    st = c.stats()
    n = lib.cvr_debug_regenstats(buf, 1)
    assert n > 0
    r = [int(buf[i]) for i in range(n)]
    batches, runs = r[0], max(r[1], 1)
    out = {
        "scene": a.scene, "rep": rep, "kernel_ms": round(st.kernel_ms, 4), "paths": st.paths, "segments": st.segments,
        "escaped": st.escaped, "batches": batches, "regen_runs": r[1], "phases": r[10],
        "mean_tb": round(r[2] / batches, 2), "mean_tc": round(r[3] / batches, 2),
        "mean_tn_or_accepted_per_batch": round(r[4] / batches, 2),
        "new_or_accepted_per_regen_run": round(r[4] / runs, 2), "camera_misses": r[5],
        "misses_per_batch": round(r[5] / batches, 2), "mean_n_ln_at_trigger": round(r[6] / max(r[7], 1), 2),
        "batches_before_exhaustion": r[7], "mean_burst_width": round(r[8] / runs, 2), "units_taken_back": r[9],
    }
    print(json.dumps(out), flush=True)
c.close()
