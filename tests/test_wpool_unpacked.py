"""No packed fp32 arithmetic in the wave-pool kernels of the built library.

A wave64 fp32 op issues at the SIMD's whole fp32 rate on gfx950, so a
v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 does two ops' work in no less than
two ops' time, and assembling its register pairs costs moves, SALU and SGPR
spills on top (profiles/round7/README.md).  cvr_wpool.hip is
therefore compiled with SLP vectorisation off and trilerp_cell is written with
plain lerps.  A flag or compiler change that brings the packing back would
render the same bits more slowly, and no parity test would notice: this one
reads the library's gfx950 code object (tools/isa_same.py's disassembly) and
fails on the first packed fp32 op in any k_wpool instance."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_same  # noqa: E402

import test_gpu_unpacked as gpu_cases  # noqa: E402

LIB = os.path.join(ROOT, "cudavolumerenderer_amd", "libcvr.so")
PACKED = ("v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32")
LLVM_TOOLS = ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")


def test_no_packed_fp32_in_any_wave_pool_instance(tmp_path):
    if not os.path.exists(LIB):
        pytest.skip("libcvr.so is not built")
    if not all(os.access(os.path.join(isa_same.LLVM, t), os.X_OK) for t in LLVM_TOOLS):
        pytest.skip("the LLVM tools are absent")
    found = isa_same.kernels(LIB, str(tmp_path), re.compile(r"k_wpool<"))
    assert len(found) >= 57, f"only {len(found)} k_wpool instances in the library"
    packed = {name: [i for i in body if i.split()[0].startswith(PACKED)] for name, body in found.items()}
    bad = {name: ins for name, ins in packed.items() if ins}
    assert not bad, "packed fp32 ops in " + "; ".join(f"{n}: {len(i)} (first: {i[0]})" for n, i in sorted(bad.items()))
    # the disassembly is of real kernels: every instance has its VALU code and ends its program
    for name, body in found.items():
        assert sum(i.startswith("v_") for i in body) > 1000 and any(i.startswith("s_endpgm") for i in body), name


@pytest.mark.parametrize("name", gpu_cases.CASES)
def test_gpu_cases_reach_the_trilinear_code(cvr, oracle_mod, name):
    """tests/test_gpu_unpacked.py's media on the CPU: the oracle's walk of each case has real
    collisions (a collision is accepted against an interpolated density, so its cell was
    fetched), escapes and roulette deaths.  On the GPU each case asserts the same of its own
    counters (stats.fetches > 0, stats.albedo > 0)."""
    _, _, _, rec, _, stats = gpu_cases.reference(cvr, oracle_mod, name)
    gpu_cases.assert_reaches_the_trilinear_code(rec, stats, name)
    print(f"{name}: oracle density {stats['density']} albedo {stats['albedo']} escaped {stats['escaped']}")
