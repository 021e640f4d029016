"""The regeneration burst's bookkeeping (csrc/cvr_regen_plan.h), on the host.

k_wpool's regeneration phase makes camera paths in bursts across the wave and leaves the
arithmetic of a burst (its width, the hits that get a slot, the units it commits and where
the cursor goes) to plain constexpr functions.  build/regen_plan (tests/cpp/regen_plan.cpp,
plain g++, built by `make`) compares them with a unit-by-unit model: every (free, remaining,
hit mask) whose burst is at most 8 wide, random 64-wide masks, and chained bursts over chunked
streams, where every unit must be committed exactly once and a committed hit always has a
slot.  The header's own static_assert sweep runs when this program (and the kernel) compiles."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "regen_plan")


def test_burst_plan_matches_the_unit_by_unit_model():
    assert os.path.exists(BIN), "build/regen_plan missing: run make"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("regen_plan ok: "), r.stdout
    assert int(r.stdout.split()[2]) > 200000
