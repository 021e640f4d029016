#!/usr/bin/env python3
"""Compare the instruction streams of kernels in two builds (needs no GPU).

  python tools/isa_same.py OLD.o NEW.o [--match REGEX]

OLD.o / NEW.o: host objects of one .hip file from two builds (build/obj/cvr_wpool.o),
or shared libraries.  The gfx950 code object of each is unbundled and disassembled;
every kernel whose demangled name matches REGEX (default: the k_wpool instances
bench.py times: 5 waves per SIMD, kMedDenseFull / kMedDenseFullUniform / kMedSparse,
no records) is reduced to its instructions: addresses and encodings are dropped,
and branch targets are kept as offsets from the kernel's own start.  Prints one
line per kernel and exits 1 if any differs or is missing.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
# k_wpool<E, 5, kMed, false, kFlush> with kMed 2 (DenseFull), 3 (DenseFullUniform), 1 (Sparse)
DEFAULT = r"k_wpool<(true|false), 5, [123], false, (true|false)>"


BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path, tmp):
    """The gfx950 code objects of an object (one) or a shared library (one per .hip file)."""
    # objects and shared libraries carry their offload bundles in the .hip_fatbin section, a library
    # one bundle per linked object, each at its own alignment
    fat = os.path.join(tmp, os.path.basename(path) + ".fatbin")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, fat])
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), data)] or [0]
    outs = []
    for i, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
        part, out = f"{fat}.{i}", os.path.join(tmp, f"{os.path.basename(path)}.{i}.co")
        with open(part, "wb") as f:
            f.write(data[a:b])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={out}"])
        if os.path.getsize(out):
            outs.append(out)
    return outs


def kernels(path, tmp, pattern):
    txt = "\n".join(subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--demangle", "--no-show-raw-insn",
                                             "--no-leading-addr", co], text=True) for co in code_objects(path, tmp))
    res, name, body = {}, None, []

    def keep():
        # "..." is objdump's mark for zero bytes it skipped.  As a kernel's last line it is the fill up to
        # the next kernel's alignment, which every kernel but the section's last has: no instruction, and
        # it moves with the order the kernels are emitted in.  Anywhere else it stays and is compared.
        if name is not None:
            res[name] = body[:-1] if body and body[-1] == "..." else body

    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.*)>:$", line)
        if m:
            keep()
            name, body = m.group(1), []
            if not pattern.search(name):
                name = None
            continue
        if re.search(r":\s+file format \S+$", line):  # the next code object's header ends the last kernel
            keep()
            name = None
        if name is None or not line.strip():
            continue
        ins = line.split("//")[0].strip()  # drop the address / encoding comment
        if ins:
            body.append(ins)
    keep()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--match", default=DEFAULT)
    ap.add_argument("--show", type=int, default=20, help="diff lines to print per differing kernel")
    a = ap.parse_args()
    pat = re.compile(a.match)
    with tempfile.TemporaryDirectory() as tmp:
        os.mkdir(os.path.join(tmp, "a"))
        os.mkdir(os.path.join(tmp, "b"))
        old = kernels(a.old, os.path.join(tmp, "a"), pat)
        new = kernels(a.new, os.path.join(tmp, "b"), pat)
    bad = 0
    for name in sorted(old):
        if name not in new:
            print(f"MISSING  {name}")
            bad += 1
        elif old[name] != new[name]:
            print(f"DIFFERS  {name}: {len(old[name])} -> {len(new[name])} instructions")
            for l in list(difflib.unified_diff(old[name], new[name], lineterm="", n=0))[: a.show]:
                print("    " + l)
            bad += 1
        else:
            print(f"same     {name}: {len(old[name])} instructions")
    print(f"{len(old)} kernels compared, {bad} differ")
    return 1 if bad or not old else 0


if __name__ == "__main__":
    sys.exit(main())
