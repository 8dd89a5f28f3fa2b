"""Instruction-level diff of every kernel of liblfmcmc.so between a git revision (default: the parent, HEAD~1 - or HEAD when
the working tree has changes of its own) and the working tree.  Both are compiled here (hipcc --cuda-device-only -S, the
build's flags); no GPU needed.
    python tools/isa_diff.py [--base REV] [--allow PREFIX ...] [--show N]
Per kernel: identical, identical but for removed kernel-argument warm-up loads (lf_math.h: warm_kernarg's ladder, an
`s_load_dword` of the kernarg segment pointer), or changed.  Exit status 1 when a kernel outside the --allow prefixes
(default: the one-launch lf_free<ST, false, true>) changed, appeared or disappeared."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lumfuncmcmc_amd import build  # noqa: E402

ALLOW = ["_ZN2lf7lf_freeILi2ELb0ELb1EEE", "_ZN2lf7lf_freeILi4ELb0ELb1EEE", "_ZN2lf7lf_freeILi8ELb0ELb1EEE"]


def device_asm(src_root):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "lf.s")
        src = os.path.join(src_root, "lumfuncmcmc_amd", "csrc", "lfmcmc.hip")
        subprocess.run([build.hipcc()] + build.CXXFLAGS + ["--cuda-device-only", "-S", "-o", out, src], check=True,
                       cwd=os.path.dirname(src))
        return open(out).read()


def kernels(text):
    """{mangled name: [normalised instruction lines]} - comments, directives and labels dropped, basic-block labels
    renumbered per kernel (their numbers carry the function's index in the module), inline-asm offsets evaluated"""
    out = {}
    for m in re.finditer(r"^(_ZN2lf\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M):
        ins = []
        for line in m.group(2).split("\n"):
            line = line.split(";")[0].strip()
            if not line or line.startswith((".", "//")) or line.endswith(":"):
                continue
            line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
            line = re.sub(r"\s+", " ", line)
            mm = re.match(r"(s_load_dword \w+, s\[\d+:\d+\]), (0x[0-9a-f]+) \+ (0x[0-9a-f]+)$", line)
            if mm:
                line = "%s, 0x%x" % (mm.group(1), int(mm.group(2), 16) + int(mm.group(3), 16))
            ins.append(line)
        out[m.group(1)] = ins
    return out


def warm_load(line):
    return re.match(r"s_load_dword s\d+, s\[\d+:\d+\], 0x[0-9a-f]+$", line) is not None


def compare(a, b):
    """'identical', ('loads removed', n) or ('changed', diff lines)"""
    if a == b:
        return "identical", []
    sm = difflib.SequenceMatcher(a=a, b=b, autojunk=False)
    removed, other = [], []
    for op, i1, i2, j1, j2 in sm.get_opcodes():
        if op == "equal":
            continue
        if op == "delete" and all(warm_load(l) for l in a[i1:i2]):
            removed += a[i1:i2]
            continue
        other += ["- " + l for l in a[i1:i2]] + ["+ " + l for l in b[j1:j2]]
    if other:
        return "changed", other
    return "loads removed", removed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default=None, help="git revision to compare against (default: HEAD~1 if the tree is clean, else HEAD)")
    ap.add_argument("--allow", nargs="*", default=ALLOW, help="kernel name prefixes that may change")
    ap.add_argument("--show", type=int, default=8, help="diff lines shown per changed kernel")
    a = ap.parse_args()
    base = a.base
    if base is None:
        dirty = subprocess.run(["git", "status", "--porcelain", "--untracked-files=no"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
        base = "HEAD" if dirty else "HEAD~1"
    with tempfile.TemporaryDirectory() as d:
        tar = os.path.join(d, "base.tar")
        subprocess.run(["git", "archive", "-o", tar, base, "lumfuncmcmc_amd/csrc", "include"], cwd=ROOT, check=True)
        with tarfile.open(tar) as t:
            t.extractall(d)
        old = kernels(device_asm(d))
    new = kernels(device_asm(ROOT))
    bad = 0
    allowed = lambda n: any(n.startswith(p) for p in a.allow)      # noqa: E731
    counts = {}
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            tag = "only in the working tree" if name in new else "only in " + base
            print("%-26s %s%s" % (tag, name, "  (allowed)" if allowed(name) else ""))
            bad += not allowed(name)
            continue
        kind, lines = compare(old[name], new[name])
        counts[kind] = counts.get(kind, 0) + 1
        if kind == "identical":
            continue
        if kind == "loads removed":
            print("%-26s %s: %s" % ("warm-up loads removed", name, ", ".join(l.split(", ")[-1] for l in lines)))
            continue
        print("%-26s %s: %d lines%s" % ("CHANGED", name, len(lines), "  (allowed)" if allowed(name) else ""))
        for l in lines[:a.show]:
            print("    " + l)
        bad += not allowed(name)
    print("base %s: %d kernels; working tree: %d; %s; %d disallowed change(s)"
          % (base, len(old), len(new), ", ".join("%d %s" % (v, k) for k, v in sorted(counts.items())), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
