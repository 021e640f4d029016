#!/usr/bin/env python3
"""Issue-cost census of one kernel of a device assembly: per section and per source function,
the VALU instructions by count and by issue weight (needs no GPU).

  make census-asm                                   # build/census/cvr_wpool.s, with .loc lines
  python3 tools/isa_census.py build/census/cvr_wpool.s [--kernel REGEX] [--top N] [--title TEXT]

The assembly is `hipcc ... -gline-tables-only --cuda-device-only -S` of a .hip file (line tables
change no instruction).  The kernel is the one whose demangled name matches REGEX (default: the
instance bench.py's C2 runs).  Its instructions are split into three sections by the priority
switches of the wave pool: prologue (up to the first `s_setprio 1`), track loop (from there to the
first `s_setprio 0`), event batch (everything after), in the order the assembly lays them out.
Every instruction is attributed to the source function that holds the line of the last `.loc`
before it: for inlined code that is the innermost callee, found by a brace scan of the source
file the `.loc` names.  Output: markdown.

Weights, in plain wave64 fp32 ops (MI355X_MICROARCH.md, "Per-instruction cycle constants"):
  1  a plain VALU op: `v_fma_f32` (wave64) issues in 2 cycles on the 32-wide SIMD, which is the whole
     vector peak of 64 FLOP/clk/SIMD.
  2  v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32: two ops' work at that same peak, so no less than two
     ops' time.  This is a floor: the row "price of one filler beside MFMAs" measured one v_pk_fma_f32
     at +22 cycles over two v_fma_f32 and two v_pk_add_f32 at +26, in the setting it was taken in.
  4  v_rcp_* / v_rsq_* / v_sqrt_*: the transcendental unit runs at a quarter of the fp32 rate; the
     row "vector-instruction ISSUE cost" (one wave alone) measured 8 cycles against 4 for v_fma_f32,
     so the true weight lies between 2 and 4.
SQ_INSTS_VALU and the count column count every one of these once.
"""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
C2 = r"k_wpool<false, 5, 2, false, false>"
PACKED = ("v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32")
WEIGHTS = ((PACKED, 2), (("v_rcp_", "v_rsq_", "v_sqrt_"), 4))
SECTIONS = ("prologue", "track loop", "event batch")
NOT_A_FUNCTION = {"if", "for", "while", "switch", "return", "sizeof", "catch", "static_assert", "decltype",
                  "alignas", "__attribute__", "__launch_bounds__", "defined"}


def weight(op):
    for prefixes, w in WEIGHTS:
        if op.startswith(prefixes):
            return w
    return 1


def demangle(names):
    """{mangled: demangled} through llvm-cxxfilt or c++filt (the names as they are where neither exists)."""
    tool = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, out.stdout.splitlines()))


# ------------------------------------------------------- source functions ---
def _blank(text):
    """The text with comments, string and character literals and preprocessor lines blanked (newlines kept)."""
    def sub(m):
        return re.sub(r"[^\n]", " ", m.group(0))
    text = re.sub(r"//[^\n]*|/\*.*?\*/|\"(?:\\.|[^\"\\\n])*\"|'(?:\\.|[^'\\\n])*'", sub, text, flags=re.S)
    return re.sub(r"^[ \t]*#(?:[^\n\\]|\\\n|\\.)*", sub, text, flags=re.M)


def function_spans(path):
    """[(first line, last line, name)] of the function bodies of a C++ source, outermost functions
    only (a lambda or a local struct belongs to the function around it); namespaces, extern "C"
    blocks and struct / class bodies are looked into."""
    try:
        text = _blank(open(path, errors="replace").read())
    except OSError:
        return []
    spans, stack, decl, line, head_line, in_fn = [], [], [], 1, 1, 0
    for tok in re.finditer(r"[{};]|\n|[^{};\n]+", text):
        t = tok.group(0)
        if t == "\n":
            line += 1
        elif in_fn:  # inside a function body: only count braces
            if t == "{":
                in_fn += 1
            elif t == "}":
                in_fn -= 1
                if not in_fn:
                    spans[-1][1] = line
        elif t == "{":
            head = " ".join(decl)
            decl = []
            flat = head  # every parenthesised group, nested ones included, as one mark: f(g(x)) h(y) -> f@ h@
            while re.search(r"\([^()]*\)", flat):
                flat = re.sub(r"\([^()]*\)", "@", flat)
            calls = [n for n in re.findall(r"(~?\w+)\s*(?:<[^<>@]*>)?\s*@", flat) if n not in NOT_A_FUNCTION]
            if calls and not head.rstrip().endswith("="):
                spans.append([head_line, line, calls[0]])
                in_fn = 1
            else:  # a namespace, an extern "C" block, a struct body or an initialiser
                stack.append(t)
        elif t == "}":
            if stack:
                stack.pop()
            decl = []
        elif t == ";":
            decl = []
        elif t.strip():
            if not decl:
                head_line = line
            decl.append(t.strip())
    return [tuple(s) for s in spans]


class Sources:
    def __init__(self):
        self.spans = {}

    def function(self, path, line):
        if path not in self.spans:
            self.spans[path] = function_spans(path)
        for a, b, name in self.spans[path]:
            if a <= line <= b:
                return name
        return f"({os.path.basename(path)})"


# ------------------------------------------------------------- assembly ---
def kernel_body(lines, pattern):
    """(demangled name, the lines of the first kernel whose demangled name matches)."""
    starts = [(i, m.group(1)) for i, l in enumerate(lines) if (m := re.match(r"^(_Z\w+):\s*(;.*)?$", l))]
    names = demangle(sorted({n for _, n in starts}))
    for i, n in starts:
        if pattern.search(names[n]):
            end = next(j for j in range(i, len(lines)) if lines[j].lstrip().startswith("s_endpgm"))
            while not lines[end].lstrip().startswith((".Lfunc_end", ".section", ".size")) and end + 1 < len(lines):
                end += 1  # blocks laid out after the first s_endpgm belong to the kernel too
            return names[n], lines[i:end]
    sys.exit(f"no kernel matches {pattern.pattern}")


def file_table(lines):
    """({file number: path}, the directory of the compilation)."""
    files, compile_dir = {}, ""
    for l in lines:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            n, a, b = m.groups()
            files[int(n)] = os.path.normpath(os.path.join(a, b) if b else a)
            if int(n) == 0 and b:
                compile_dir = a
    return files, compile_dir


def census(lines, pattern, root):
    files, compile_dir = file_table(lines)
    name, body = kernel_body(lines, pattern)
    src = Sources()
    rows = collections.defaultdict(lambda: collections.Counter())  # (section, function) -> counters
    section, fn = 0, "(no line)"
    for l in body:
        t = l.split(";")[0].split()
        if not t:
            continue
        if t[0] == ".loc":
            # file 0 is the compiled file under the directory it was compiled in; the project's other
            # files are relative to that directory.  Both are looked up under `root`.
            path = files.get(int(t[1]), "?")
            if os.path.isabs(path) and 0 in files and path == files[0]:
                path = os.path.relpath(path, compile_dir)
            path = path if os.path.isabs(path) else os.path.join(root, path)
            fn = src.function(path, int(t[2])) if int(t[2]) else "(no line)"
            continue
        op = t[0]
        if op.startswith(".") or op.endswith(":"):
            continue
        if op == "s_setprio":
            if section == 0 and t[1] == "1":
                section = 1
            elif section == 1 and t[1] == "0":
                section = 2
        c = rows[(SECTIONS[section], fn)]
        if op.startswith("v_"):
            c["valu"] += 1
            c["weighted"] += weight(op)
            c["packed"] += op.startswith(PACKED)
            c["moves"] += op.startswith(("v_mov_b32", "v_pk_mov", "v_mov_b64", "v_accvgpr"))
            c["lanes"] += op.startswith(("v_readlane", "v_writelane", "v_readfirstlane"))
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            c["vmem"] += 1
    return name, rows


COLS = ("valu", "weighted", "packed", "moves", "lanes", "salu", "lds", "vmem")
HEAD = ("VALU", "weighted", "packed fp32", "moves", "lane r/w", "SALU", "LDS", "VMEM")


def report(name, rows, top, title):
    out = [f"# {title}", "", f"Kernel: `{name}`.  Weights: packed fp32 2, `v_rcp` / `v_rsq` / `v_sqrt` 4, every other "
           "VALU instruction 1 (`tools/isa_census.py`).  `moves`: `v_mov_b32`, `v_pk_mov_b32`, AGPR copies; "
           "`lane r/w`: `v_readlane`, `v_writelane`, `v_readfirstlane` (SGPR spill traffic among them); "
           "both are part of `VALU`.", "", "## Sections", "",
           "| section | " + " | ".join(HEAD) + " |", "|---|" + "---:|" * len(COLS)]
    total = collections.Counter()
    for s in SECTIONS:
        c = collections.Counter()
        for (sec, _), v in rows.items():
            if sec == s:
                c.update(v)
        total.update(c)
        out.append(f"| {s} | " + " | ".join(str(c[k]) for k in COLS) + " |")
    out.append("| whole kernel | " + " | ".join(str(total[k]) for k in COLS) + " |")
    for s in SECTIONS:
        fns = sorted(((v, fn) for (sec, fn), v in rows.items() if sec == s and v["valu"]),
                     key=lambda r: (-r[0]["weighted"], r[1]))
        out += ["", f"## {s}: VALU by source function", "",
                "| function | VALU | weighted | packed fp32 | moves | lane r/w |", "|---|---:|---:|---:|---:|---:|"]
        for v, fn in fns[:top]:
            out.append(f"| `{fn}` | {v['valu']} | {v['weighted']} | {v['packed']} | {v['moves']} | {v['lanes']} |")
        rest = collections.Counter()
        for v, _ in fns[top:]:
            rest.update(v)
        if rest:
            out.append(f"| {len(fns) - top} others | {rest['valu']} | {rest['weighted']} | {rest['packed']} | "
                       f"{rest['moves']} | {rest['lanes']} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default=C2, help="regex on the demangled kernel name")
    ap.add_argument("--top", type=int, default=40, help="functions listed per section")
    ap.add_argument("--title", default="Issue-cost census")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."),
                    help="directory relative .file paths start from")
    a = ap.parse_args()
    lines = open(a.asm).read().split("\n")
    name, rows = census(lines, re.compile(a.kernel), a.root)
    sys.stdout.write(report(name, rows, a.top, a.title))


if __name__ == "__main__":
    main()
