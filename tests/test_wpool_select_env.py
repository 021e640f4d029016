"""The wave pool's instance selection with an environment map set (csrc/cvr_wpool_select.h).

build/wpool_select_env (tests/cpp/wpool_select_env.cpp, plain g++, built by `make`) prints what
wpool_select returns for every request of the environment half of the space: the 2048 requests of
tests/test_wpool_select.py with `env` set.  Each line is checked against the rule include/cvr.h
states, restated here: which requests are refused, and what an accepted one runs."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "wpool_select_env")
K_DENSE, K_SPARSE, K_HALF, K_MOMENTS, K_ENV = 0, 1, 16, 32, 64
FIELDS = "scatter_eps waves sparse full uniform half naive_mk count_words moments record flush env".split()


def lines():
    assert os.path.exists(BIN), "build/wpool_select_env missing: run make"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        req, inst = line.split(" : ")
        q = dict(zip(FIELDS, (int(v) for v in req.split())))
        out.append((q, None if inst == "-" else tuple(int(v) for v in inst.split())))
    return out


def refusal(q):
    """The listed obstacle a request with an environment meets, or None."""
    if q["naive_mk"]:
        return "kernel id naiveMK"
    if q["waves"] != 5:
        return "CVR_OPT_WAVES other than 5"
    if q["count_words"]:
        return "CVR_OPT_COUNT_WORDS 1"
    if q["record"]:
        return "cvr_trace_launch"
    if q["flush"]:
        return "cvr_render_frame's in-launch output (never requested: the call copies instead)"
    if q["moments"] and q["sparse"] and q["half"]:
        return "second moments on a sparse half medium"
    return None


def test_environment_half_of_the_space():
    got = lines()
    assert len(got) == 2048
    seen = set()
    for q, inst in got:
        assert q["env"] == 1
        why = refusal(q)
        if inst is None:
            assert why is not None, f"refused without a listed reason: {q}"
            continue
        assert why is None, f"accepted in spite of {why}: {q}"
        eps, waves, med, record, flush = inst
        assert med & K_ENV and waves == 5 and not record and not flush, (q, inst)
        assert eps == q["scatter_eps"]
        # the generic layout of the medium's kind: cells, bounds and a uniform albedo are read at run time
        assert med & 3 == (K_SPARSE if q["sparse"] else K_DENSE), (q, inst)
        want = (med & 3) | K_ENV | (K_MOMENTS if q["moments"] else 0) | (K_HALF if q["sparse"] and q["half"] else 0)
        assert med == want, (q, inst)
        seen.add(inst)
    # five media (dense, sparse, sparse half, dense + moments, sparse + moments) x two scatter modes
    assert len(seen) == 10, sorted(seen)
    assert {m for _, _, m, _, _ in seen} == {64, 65, 81, 96, 97}


def test_plain_half_is_untouched_by_the_new_field():
    """The first 2048 requests have the feature off: build/wpool_select's lines (pinned by
    tests/test_wpool_select.py) and this program's differ in the env column and the selection only."""
    plain = subprocess.run([os.path.join(ROOT, "build", "wpool_select")], capture_output=True, text=True, timeout=60)
    assert plain.returncode == 0
    p = plain.stdout.splitlines()
    e = lines()
    assert len(p) == len(e) == 2048
    for a, (q, _) in zip(p, e):
        assert a.split(" : ")[0].split() == [str(q[k]) for k in FIELDS[:-1]]
