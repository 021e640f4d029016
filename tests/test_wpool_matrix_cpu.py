"""The wave-pool instance matrix (tests/wpool_matrix.py) against the library's table and the selection
rule.  No GPU.

  * the declared instances are exactly the rows cvr_debug_wpool_rows returns: a row added to the table
    without an entry fails here, and so does an entry for a row that no longer ships;
  * every declared tuple, and the tuple the rule gives for the entry's own configuration, comes out of
    build/wpool_select or build/wpool_select_env (the programs tests/test_wpool_select.py and
    tests/test_wpool_select_env.py pin), so the hand-written literals are the rule's;
  * the oracle's references satisfy the guards the GPU module relies on;
  * cvr_debug_last_wpool before any launch.
"""
import ctypes as C
import os
import subprocess

import pytest

import params
import wpool_matrix as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = "scatter_eps waves sparse full uniform half naive_mk count_words moments record flush env".split()


def selection():
    """{request tuple (FIELDS order): instance tuple or None} over both halves of the request space."""
    out = {}
    for prog, env in (("wpool_select", 0), ("wpool_select_env", 1)):
        path = os.path.join(ROOT, "build", prog)
        assert os.path.exists(path), f"build/{prog} missing: run make"
        r = subprocess.run([path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        for line in r.stdout.splitlines():
            req, inst = line.split(" : ")
            q = tuple(int(v) for v in req.split())
            q = q if len(q) == len(FIELDS) else q + (env,)
            assert len(q) == len(FIELDS) and q[-1] == env
            out[q] = None if inst == "-" else tuple(int(v) for v in inst.split())
    assert len(out) == 4096
    return out


def request_of(e):
    """What the entry's configuration asks of the kernel, field by field as cvr_launch.cpp's wpool_request
    reads a context: the library's defaults are cells and bounds on, uniform-albedo detection on."""
    dense_full = not e.sparse and wm.opt(e, "OPT_CELLS") != 0 and wm.opt(e, "OPT_BOUNDS") != 0
    q = dict(scatter_eps=int(e.kernel != "regenerationSK"), waves=wm.opt(e, "OPT_WAVES") or 5, sparse=int(e.sparse),
             full=int(dense_full), uniform=int(e.medium.startswith("uniform") and not e.sparse),
             half=int(wm.opt(e, "OPT_MEDIUM_FORMAT") == 1), naive_mk=int(e.kernel == "naiveMK"),
             count_words=int(wm.opt(e, "OPT_COUNT_WORDS") == 1), moments=int(wm.opt(e, "OPT_MOMENTS") == 1),
             record=int(e.entry == "trace"), flush=int(e.entry == "frame"), env=int(e.entry == "env"))
    return tuple(q[f] for f in FIELDS)


def test_entries_are_exactly_the_shipped_rows(cvr):
    rows = cvr.wpool_rows()
    assert len(set(rows)) == len(rows), "the library's table repeats a row"
    declared = [e.instance for e in wm.ENTRIES]
    assert len(set(declared)) == len(declared), "two entries declare the same instance"
    assert len({e.name for e in wm.ENTRIES}) == len(wm.ENTRIES)
    missing = sorted(set(rows) - set(declared))
    gone = sorted(set(declared) - set(rows))
    assert not missing, f"shipped instances without a matrix entry: {missing}"
    assert not gone, f"matrix entries for instances that do not ship: {gone}"
    assert len(rows) == len(declared)


def test_declared_tuples_are_the_selection_rules():
    sel = selection()
    plain = {k for q, k in sel.items() if k is not None and not q[-1]}
    env = {k for q, k in sel.items() if k is not None and q[-1]}
    for e in wm.ENTRIES:
        assert e.instance in (env if e.entry == "env" else plain), f"{e.name}: {e.instance} is selected by no request"
        q = request_of(e)
        assert q in sel, (e.name, q)
        assert sel[q] == e.instance, f"{e.name}: its configuration {dict(zip(FIELDS, q))} selects {sel[q]}"
        assert e.medium.endswith("half") == (wm.opt(e, "OPT_MEDIUM_FORMAT") == 1), e.name
        assert wm.opt(e, "OPT_GRID") is None, e.name  # the GPU module sets it


@pytest.mark.parametrize("case_name", wm.CASES)
def test_references_guard_against_a_vacuous_pass(cvr, oracle_mod, case_name):
    """Between 20 % and 100 % of the paths escape, some die by roulette, launch 1 gives a pixel at most
    one contribution and launch 2 gives some pixel several (wpool_matrix.check_guards, asserted whenever
    a reference is made): here for every kernel id on the fp32 medium, under the oracle alone."""
    refs = wm.Refs(oracle_mod, cvr.half_round)
    for kernel in wm.KERNEL_IDS:
        one = refs.get(case_name, kernel, "f32", "one")
        acc = refs.get(case_name, kernel, "f32", "acc")
        assert len(one.recs) == 128 * 128 and len(acc.recs) == params.n_paths(params.CASES[case_name])
        assert one.counters["paths"] // wm.GRID >= wm.MIN_PATHS_PER_WAVE
        assert one.counters["paths"] // wm.GRID_FRAME >= wm.MIN_PATHS_PER_WAVE


def test_last_wpool_before_any_launch(cvr):
    lib = cvr.load()
    inst, grid = (C.c_int32 * 5)(), C.c_uint32(0)
    assert lib.cvr_debug_last_wpool(None, inst, C.byref(grid)) == -1  # CVR_ERR_INVALID: no context
    n = C.c_uint32(0)
    assert lib.cvr_debug_wpool_rows(None, 4, C.byref(n)) == -1  # a capacity without rows
    assert lib.cvr_debug_wpool_rows(None, 0, None) == -1
    if not os.path.exists("/dev/kfd"):
        return  # no device, no context: tests/test_gpu_wpool_matrix.py asserts the same on every fresh context
    ctx = cvr.Context(0, "regenerationSK")
    try:
        with pytest.raises(cvr.CvrError) as e:
            ctx.last_wpool()
        assert e.value.code == -3  # CVR_ERR_STATE
    finally:
        ctx.close()
