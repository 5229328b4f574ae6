#!/usr/bin/env python3
"""Are the kernels of two `hipcc -S --cuda-device-only` outputs the same instruction for instruction?
    python tools/isa_compare.py before.s after.s [--rename OLD=NEW ...]
Compares, per kernel symbol, the instruction lines between the label and the kernel's .Lfunc_end (comments, directives and
basic-block labels' numbering and the operand order of commutative scalar and/or/xor aside).  Used when source is refactored without an intended change of the code (round 4:
the resolved A/B switches of csrc/photo_train.hip).  Each kernel's .amdhsa_kernel ... .end_amdhsa_kernel block (register counts,
LDS size, wave limits) must be equal too: DESC marks a kernel whose instructions agree and whose descriptor does not.
--rename OLD=NEW (repeatable): a type was renamed.  The kernels are then matched by their DEMANGLED names (c++filt; a renamed
namespace shifts the substitution indices of a mangled name, so text replacement there does not do), OLD replaced by NEW in the
first file's: --rename mdx::nhwc::bf16=mdx::bf16 --rename mdx::bf16n=mdx::bf16 (round 7: one bf16 storage type)."""
import argparse
import re
import subprocess
import sys


def kernels(path):
    """{kernel symbol: (instruction lines, lines of its .amdhsa_kernel block)}"""
    out, desc, name, body, dname = {}, {}, None, [], None
    for ln in open(path):
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", ln)
        if m:
            dname = m.group(1)
            desc[dname] = []
            continue
        if dname is not None:
            if ln.strip() == ".end_amdhsa_kernel":
                dname = None
            else:
                desc[dname].append(ln.split(";")[0].strip())
            continue
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if ln.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            t = ln.split(";")[0].strip()
            if not t or t.startswith("."):
                t = re.sub(r"^\.LBB\d+_(\d+):", r"L\1:", t) if t.startswith(".LBB") else ""
                if not t:
                    continue
            t = re.sub(r"\.LBB\d+_(\d+)", r"L\1", t)
            m2 = re.match(r"^(s_(?:and|or|xor)_b(?:32|64)) (\S+), (\S+), (\S+)$", t)
            if m2:                                   # commutative scalar ops: operand order is not a difference
                x, y = sorted([m2.group(3), m2.group(4)])
                t = "%s %s %s, %s" % (m2.group(1), m2.group(2), x, y)
            body.append(t)
    return {k: (v, desc.get(k)) for k, v in out.items()}


def by_demangled_name(ks, renames):
    names = sorted(ks)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for k, d in zip(names, plain):
        for old, new in renames:
            d = d.replace(old, new)
        assert d not in out, "two kernels named %s" % d
        out[d] = ks[k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("first")
    ap.add_argument("second")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    a, b = kernels(args.first), kernels(args.second)
    if args.rename:
        a, b = by_demangled_name(a, [r.split("=", 1) for r in args.rename]), by_demangled_name(b, [])
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print("ONLY IN %s  %s" % ("first" if k in a else "second", k))
            bad += 1
            continue
        word = "DIFF" if a[k][0] != b[k][0] else ("same" if a[k][1] == b[k][1] and a[k][1] is not None else "DESC")
        bad += word != "same"
        print("%s %-78s %6d %6d instructions" % (word, k[:78], len(a[k][0]), len(b[k][0])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
