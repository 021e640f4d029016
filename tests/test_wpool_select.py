"""The wave pool's instance selection (csrc/cvr_wpool_select.h), pinned request by request.

build/wpool_select (tests/cpp/wpool_select.cpp, plain g++, built by `make`) prints the instance
wpool_select returns for every request of the space: 2 scatter modes x 4 budgets x 4 layouts
x 2^6 features = 2048 lines.  tests/golden/wpool_instances.txt holds the same lines as recorded
from the commit before the selection function existed: that commit's launch_wpool, compiled
unedited into a host program whose hipLaunchKernel was a macro that kept the kernel address,
called once per request with dummy pointers for the medium's and the launch's arrays, the
addresses resolved to k_wpool<...> names with nm -C.  Every request of the space can be put
through that launch_wpool, so none is left out.

A wrong pick renders the same image more slowly, so no parity test sees it: this one does.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "wpool_select")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wpool_instances.txt")


def test_selection_matches_the_recorded_instances():
    assert os.path.exists(BIN), "build/wpool_select missing: run make"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert len(want) == 2048 and len(got) == 2048
    wrong = [f"{g!r} (recorded: {w!r})" for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} requests select another instance, the first: " + "; ".join(wrong[:5])
    instances = {line.split(" : ")[1] for line in got} - {"-"}
    assert len(instances) == 57
