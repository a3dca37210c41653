#!/usr/bin/env python3
"""Generated code of one HIP source, a git revision against the working tree, kernel by kernel (CPU only: hipcc cross-compiles,
no GPU is opened).

    python tools/kernel_isa_diff.py REV FILE [--show N] [--define NAME[=VALUE] ...]

REV's vit-ssl_amd/csrc, include, include_ext and include_addons are materialised in a temporary directory; both sides of FILE (a name under
csrc/) are compiled with __graft_entry__.FLAGS plus the file's PER_FILE_FLAGS and `--cuda-device-only -S`; the assembly is
split per kernel symbol; comments, .loc / .file / .cfi / .p2align lines and the function ordinal of .LBB labels are dropped.
Per kernel: `same` (identical line for line) or the number of differing lines, `sorted` (the sorted instruction lists are
equal: the same instructions, operands and registers in another order), and VGPR / AGPR / SGPR / scratch bytes / spill counts
/ static LDS / kernel-argument bytes / occupancy of both sides.  The tool compares text and counts lines; it knows nothing
about particular instructions.  Exit status 0 when every kernel is identical, 1 otherwise."""
import argparse
import difflib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREES = ("vit-ssl_amd/csrc", "include", "include_ext", "include_addons")
META_KEYS = (("VGPR", "vgpr_count"), ("AGPR", "agpr_count"), ("SGPR", "sgpr_count"), ("scratch", "private_segment_fixed_size"),
             ("vspill", "vgpr_spill_count"), ("sspill", "sgpr_spill_count"), ("LDS", "group_segment_fixed_size"),
             ("kernarg", "kernarg_segment_size"))
DROPPED = re.compile(r"\.(loc|file|cfi_\w+|p2align)\b")
LBB = re.compile(r"\.LBB\d+_")


def split_kernels(asm):
    """{kernel symbol: the lines from its label to the end of its code (the next .section, where its kernel descriptor starts,
    or its .Lfunc_end label)} for every symbol that has an .amdhsa_kernel block."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, name = {}, None
    for line in asm.splitlines():
        s = line.split(";", 1)[0].strip()
        if name is None:
            if s.endswith(":") and s[:-1] in kernels:
                name = s[:-1]
                out[name] = []
        elif s.startswith(".Lfunc_end") or s.startswith(".section"):
            name = None
        else:
            out[name].append(line)
    return out


def normalise(lines):
    """Comments, blank lines, debug / alignment directives and the function ordinal of .LBB labels removed."""
    out = []
    for line in lines:
        s = line.split(";", 1)[0].strip()
        if not s or DROPPED.match(s):
            continue
        out.append(LBB.sub(".LBB_", " ".join(s.split())))
    return out


def instructions(lines):
    """The normalised lines that are neither labels nor directives."""
    return [s for s in lines if not s.endswith(":") and not s.startswith(".")]


def metadata(asm):
    """{kernel symbol: {column: value}} from the code-object metadata and the compiler's `; Occupancy:` remark."""
    out = {}
    for block in re.split(r"^  - (?=\.)", asm, flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
        if not name:
            continue
        row = {}
        for col, key in META_KEYS:
            m = re.search(r"^\s*\." + key + r":\s+(\d+)", block, re.M)
            row[col] = int(m.group(1)) if m else -1
        out[name.group(1)] = row
    for name, occ in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+).*?^; Occupancy:\s+(\d+)", asm, re.M | re.S):
        out.setdefault(name, {})["occ"] = int(occ)
    return out


def compare(parent, branch):
    """(differing lines, sorted instruction lists equal) of two normalised kernels."""
    if parent == branch:
        return 0, True
    sm = difflib.SequenceMatcher(None, parent, branch, autojunk=False)
    differing = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")
    return differing, sorted(instructions(parent)) == sorted(instructions(branch))


def demangle(names):
    for tool in ("c++filt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"):
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
        except OSError:
            continue
        if r.returncode == 0:
            short = [re.sub(r"\(anonymous namespace\)::", "", d) for d in r.stdout.splitlines()]
            return [re.sub(r"^void |\(.*$", "", d) for d in short]
    return names


def materialise(rev, into):
    tar = subprocess.run(["git", "-C", ROOT, "archive", "--format=tar", rev, "--"] + [t for t in TREES if tree_exists(rev, t)],
                         capture_output=True, check=True).stdout
    tarfile.open(fileobj=io.BytesIO(tar)).extractall(into)
    return os.path.join(into, "vit-ssl_amd", "csrc")


def tree_exists(rev, path):
    return subprocess.run(["git", "-C", ROOT, "cat-file", "-e", f"{rev}:{path}"], capture_output=True).returncode == 0


def assemble(csrc, name, out, defines):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    cmd = [ge.HIPCC] + ge.FLAGS + ge.PER_FILE_FLAGS.get(name, []) + ["-D" + d for d in defines] + [
        "--cuda-device-only", "-S", "-x", "hip", os.path.join(csrc, name), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"hipcc failed for {os.path.join(csrc, name)}:\n{r.stderr[-4000:]}")
    with open(out) as f:
        return f.read()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev")
    ap.add_argument("file", help="source under vit-ssl_amd/csrc, e.g. gemm_nt.hip")
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N lines of each differing kernel's diff")
    ap.add_argument("--define", action="append", default=[], metavar="NAME[=VALUE]", help="extra -D for both sides")
    a = ap.parse_args()
    name = os.path.basename(a.file)
    with tempfile.TemporaryDirectory() as tmp:
        old = materialise(a.rev, tmp)
        with ThreadPoolExecutor(2) as ex:
            fp = ex.submit(assemble, old, name, os.path.join(tmp, "parent.s"), a.define)
            fb = ex.submit(assemble, os.path.join(ROOT, "vit-ssl_amd", "csrc"), name, os.path.join(tmp, "branch.s"), a.define)
            asm = {"parent": fp.result(), "branch": fb.result()}
    code = {side: {k: normalise(v) for k, v in split_kernels(t).items()} for side, t in asm.items()}
    meta = {side: metadata(t) for side, t in asm.items()}
    syms = sorted(set(code["parent"]) | set(code["branch"]))
    cols = [c for c, _ in META_KEYS] + ["occ"]
    print(f"{name}: {a.rev} (parent) against the working tree (branch)")
    print(f"{'kernel':60s} {'same':>5s} {'sorted':>6s} {'side':7s} {'instr':>6s} " + " ".join(f"{c:>7s}" for c in cols))
    same = reordered = 0
    for sym, dn in zip(syms, demangle(syms)):
        p, b = code["parent"].get(sym), code["branch"].get(sym)
        if p is None or b is None:
            print(f"{dn[:60]:60s} only in {'branch' if p is None else 'parent'}")
            continue
        n, srt = compare(p, b)
        same += n == 0
        reordered += n != 0 and srt and meta["parent"].get(sym) == meta["branch"].get(sym)
        for side, lines in (("parent", p), ("branch", b)):
            m = meta[side].get(sym, {})
            print(f"{dn[:60]:60s} {'yes' if n == 0 else n:>5} {'yes' if srt else 'NO':>6s} {side:7s} {len(instructions(lines)):6d} " +
                  " ".join(f"{m.get(c, -1):7d}" for c in cols))
        if n and a.show:
            print("\n".join(list(difflib.unified_diff(p, b, "parent", "branch", lineterm="", n=1))[:a.show]))
    print(f"{same} of {len(syms)} kernels identical, {reordered} reordered only (same sorted instructions and metadata); "
          f"parent has {len(code['parent'])} kernels, branch {len(code['branch'])}")
    return 0 if same == len(syms) else 1


if __name__ == "__main__":
    sys.exit(main())
