"""Compare the gfx950 device code of two builds of the library, kernel by kernel.  No GPU needed.
usage: python scripts/isa_compare.py PARENT.so BRANCH.so [--label NAME] [--show KERNEL_SUBSTRING]

For each library the gfx950 code object is taken out of the fat binary and disassembled; every kernel's instruction
stream is compared after masking only what moves when code around it moves: instruction addresses, branch-target
labels and the literal of an s_add_u32 / s_addc_u32 that follows s_getpc_b64 (PC-relative data offsets).
One line per kernel: name, instructions parent / branch, `identical` or the number of differing lines; then the
kernel descriptors' resource columns (VGPR, AGPR, SGPR, scratch, LDS, spills) wherever they differ, or a line saying
that none does.  --show prints the unified diff of the kernels whose demangled name contains the substring."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def code_object(lib, tmp):
    fat = os.path.join(tmp, "fatbin")
    co = os.path.join(tmp, "gfx950.co")
    run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "unused.so"))
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co)
    return co


def demangle(names):
    out = run("c++filt", input="\n".join(names)).split("\n")
    return {n: re.sub(r"ilqr::", "", d) for n, d in zip(names, out)}


def kernels(co):
    """{symbol: [normalised instruction lines]} of the kernels (the symbols that have a descriptor) and their resources."""
    notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    res = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        block = ".agpr_count:" + block
        g = lambda k: int((re.search(r"\." + k + r":\s+(\d+)", block) or [0, 0])[1])
        name = re.search(r"\.name:\s+(\S+)", block)[1]
        res[name] = dict(VGPR=g("vgpr_count"), AGPR=g("agpr_count"), SGPR=g("sgpr_count"), scratch=g("private_segment_fixed_size"),
                         LDS=g("group_segment_fixed_size"), vspill=g("vgpr_spill_count"), sspill=g("sgpr_spill_count"))
    dis = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co)
    code, cur, after_getpc = {}, None, 0
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = code.setdefault(m[1], []) if m[1] in res else None
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = re.sub(r"\s*//.*$", "", line).strip()   # the address (and raw words) after the instruction
        ins = re.sub(r"\s*<[^>]*>", "", ins)            # branch-target labels (the operand, a distance inside the kernel, stays)
        if after_getpc and re.match(r"s_addc?_u32 ", ins):
            ins = re.sub(r"(0x[0-9a-f]+|\d+)$", "<pcrel>", ins)
        after_getpc = 3 if ins.startswith("s_getpc_b64") else max(0, after_getpc - 1)
        cur.append(ins)
    for body in code.values():  # the padding behind s_endpgm
        while body and body[-1] in ("s_nop 0", "s_code_end"):
            body.pop()
    return code, res


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--label", help="what to call the pair in the report (default: the branch library's file name)")
    ap.add_argument("--show", metavar="SUBSTRING", help="print the diff of the differing kernels whose demangled name contains this")
    a = ap.parse_args()
    parent, branch, label, show = a.parent, a.branch, a.label, a.show
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        (ca, ra), (cb, rb) = kernels(code_object(parent, ta)), kernels(code_object(branch, tb))
    dem = demangle(sorted(set(ca) | set(cb)))
    print("== %s: %d kernels parent, %d branch" % (label or os.path.basename(branch), len(ca), len(cb)))
    n_diff = 0
    for sym in sorted(dem, key=lambda s: dem[s]):
        a, b = ca.get(sym), cb.get(sym)
        if a is None or b is None:
            verdict = "only in " + ("branch" if a is None else "parent")
            n_diff += 1
        elif a == b:
            verdict = "identical"
        else:
            d = [l for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
            verdict = "%d differing lines" % len(d)
            n_diff += 1
            if show is not None and show in dem[sym]:
                print("\n".join(difflib.unified_diff(a, b, "parent", "branch", lineterm="", n=3)))
        print("%-150s %6d %6d  %s" % (dem[sym][:150], len(a or ()), len(b or ()), verdict))
    print("-- %d of %d kernels differ in their instructions" % (n_diff, len(dem)))
    cols = ("VGPR", "AGPR", "SGPR", "scratch", "LDS", "vspill", "sspill")
    moved = [s for s in sorted(dem, key=lambda s: dem[s]) if ra.get(s) != rb.get(s)]
    for s in moved:
        for who, r in (("parent", ra.get(s)), ("branch", rb.get(s))):
            print("%-6s %-120s %s" % (who, dem[s][:120], " ".join("%s %d" % (c, r[c]) for c in cols) if r else "-"))
    print("-- kernel descriptors (%s): %s" % (", ".join(cols), "%d kernels differ" % len(moved) if moved else "equal for every kernel"))
    return 1 if n_diff or moved else 0


if __name__ == "__main__":
    sys.exit(main())
