#!/usr/bin/env python3
"""Device assembly of two csrc directories, kernel by kernel (CPU only; hipcc cross-compiles).

    python tools/kernel_isa_diff.py PARENT_CSRC CHILD_CSRC [--flags "-DOMDS_TIMELINE"] [--files mlp_kernels tail_kernel]
                                    [--alias "k_old<int>=k_new<int, bool>"]

Every kernel translation unit of each side (a .hip file with a __global__) is compiled with the Makefile's CXXFLAGS plus
--cuda-device-only -S into a scratch directory, the assembly is cut per kernel symbol, and each kernel is reported as
"identical" or with instruction count, resource figures and spill counts of both sides.  Kernels are matched by name over all the
translation units of a side, so one that moved to another file is compared with itself; --alias pairs one that was renamed with
its former name.  It diffs and counts; it looks for no instruction.  Exit status 1 when a kernel differs or exists on one side only.
"""
import argparse
import concurrent.futures
import pathlib
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
FIGURES = ["NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy"]


def cxxflags(csrc):
    """CXXFLAGS of csrc/Makefile; include/ is this checkout's (a scratch copy of csrc has none beside it)."""
    line = next(l for l in (csrc / "Makefile").read_text().splitlines() if l.startswith("CXXFLAGS :="))
    return line.split(":=", 1)[1].replace("$(ARCH)", "gfx950").replace("$(ROOT)", str(ROOT)).split()


def compile_asm(job):
    src, out, flags = job
    subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-Wno-unused-command-line-argument", "--cuda-device-only", "-S", str(src), "-o", str(out)], check=True)
    return out


def kernels(asm):
    """{kernel name: (normalised body lines, figures)} of one assembly file."""
    text = asm.read_text()
    found = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M):
        start = text.index(f"\n{sym}:")
        end = text.index("; Occupancy:", start)
        chunk = text[start:text.index("\n", end)]
        body = []
        for line in chunk.splitlines():
            line = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI)\d+", r".\1", line.split(";")[0].rstrip())   # labels carry the function's index
            line = line.replace(sym, "KERNEL")
            if line.strip():
                body.append(line)
        figs = {k: int(re.search(rf"^; {k}: (\d+)", chunk, re.M).group(1)) for k in FIGURES}
        code = body[:next(i for i, l in enumerate(body) if l.startswith("\t.section"))]
        figs["instructions"] = sum(1 for l in code if re.match(r"\t[a-z]", l))
        meta = text[text.index(f".name:           {sym}\n"):]           # the kernel's entry of amdhsa.kernels: its spill counts
        for k in ("sgpr_spill_count", "vgpr_spill_count"):
            figs[k] = int(re.search(rf"\.{k}:\s+(\d+)", meta[:meta.index(".wavefront_size:")] if ".wavefront_size:" in meta else meta).group(1))
        found[demangle(sym)] = (body, figs)
    return found


def demangle(sym):
    """k_exact<0, 1> for _Z7k_exactILi0ELi1EEv...; an enumerator prints as its value, so a kernel keeps its name when an int parameter
    becomes an enum; "> >" prints as ">>" (c++filt writes either, by how the template's parameters are declared).  Without c++filt the
    symbol itself."""
    if not shutil.which("c++filt"):
        return sym
    name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "")
    name = re.sub(r"\(\w+\)(?=-?\d)", "", name).split("(")[0].removeprefix("void ")
    while "> >" in name:
        name = name.replace("> >", ">>")
    return name


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("parent", type=pathlib.Path)
    ap.add_argument("child", type=pathlib.Path)
    ap.add_argument("--flags", default="", help="extra compiler flags for both sides (a diagnostic build's defines)")
    ap.add_argument("--files", nargs="*", help="translation units by stem (default: every .hip with a __global__)")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--scratch", help="keep the assembly in this directory instead of a temporary one")
    ap.add_argument("--alias", action="append", default=[], metavar="OLD=NEW",
                    help="pair the parent's kernel OLD with the child's NEW (demangled names): a kernel that was renamed")
    a = ap.parse_args()
    alias = dict(pair.split("=", 1) for pair in a.alias)
    with tempfile.TemporaryDirectory() as tmp:
        if a.scratch:
            tmp = a.scratch
            pathlib.Path(tmp).mkdir(parents=True, exist_ok=True)
        jobs = []
        for side, csrc in (("parent", a.parent), ("child", a.child)):
            units = sorted(p for p in csrc.glob("*.hip") if "__global__" in p.read_text() and (not a.files or p.stem in a.files))
            jobs += [(p, pathlib.Path(tmp) / f"{side}_{p.stem}.s", cxxflags(csrc) + a.flags.split()) for p in units]
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
            list(pool.map(compile_asm, jobs))
        old, new, where = {}, {}, {}
        for _, out, _ in jobs:
            side, stem = out.stem.split("_", 1)
            for sym, entry in kernels(out).items():
                if side == "parent":
                    sym = alias.get(sym, sym)
                (old if side == "parent" else new)[sym] = entry
                where.setdefault(sym, {})[side] = stem
        same = [s for s in old if s in new and old[s][0] == new[s][0]]
        print(f"== {len(same)} of {len(old)} kernels identical ({len(new)} on the child's side)")
        for sym in sorted(set(old) | set(new)):
            moved = len(set(where[sym].values())) > 1
            if sym in same:
                if moved:
                    print(f"  {sym}: identical, {where[sym]['parent']} -> {where[sym]['child']}")
                continue
            print(f"  {sym}" + (f" ({where[sym]['parent']} -> {where[sym]['child']})" if moved else ""))
            for side, table in (("parent", old), ("child", new)):
                print(f"    {side:6s} " + ("absent" if sym not in table else "  ".join(f"{k} {v}" for k, v in table[sym][1].items())))
        return 1 if len(same) < len(set(old) | set(new)) else 0


if __name__ == "__main__":
    sys.exit(main())
