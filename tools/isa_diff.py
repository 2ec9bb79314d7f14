#!/usr/bin/env python3
"""Compare the kernels of two AMDGPU assembly files, or of two directories of
.s files (each directory one pool: a kernel may move between files), kernel
by kernel.

    tools/isa_diff.py OLD NEW [--names table.json]

Each file is split per kernel (`.amdhsa_kernel NAME`: the code from `NAME:` to
its `.Lfunc_end`, and the `.amdhsa_*` descriptor block).  Comments and
directives are dropped, mangled symbols become `SYM` and `.LBB<f>_<n>` labels
are renumbered in order of appearance, so a kernel that only changed its name
or its place in the file compares equal.  The JSON table maps an old kernel
name to its new one; a kernel it does not list keeps its name.

Per kernel one line: `identical` (same instructions in the same order, same
descriptor), `renamed-registers` (the same multiset of mnemonics and the same
descriptor: the code was scheduled or allocated differently) or `different`.
Exit status 1 if any kernel is `different` or has no partner.
"""
import argparse
import collections
import json
import os
import re
import sys

_LABEL = re.compile(r"\.LBB\d+_\d+")
_SYMBOL = re.compile(r"\b_Z\w+")


def kernels(text):
    """{kernel name: (normalised instruction lines, descriptor lines)}"""
    lines = text.splitlines()
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        code, labels = [], {}
        for l in lines[start + 1:]:
            l = l.split(";")[0].strip()
            if l.startswith(".Lfunc_end"):
                break
            if not l or (l.startswith(".") and not _LABEL.match(l)):
                continue
            l = _LABEL.sub(lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), l)
            code.append(" ".join(_SYMBOL.sub("SYM", l).split()))
        d0 = next(i for i, l in enumerate(lines) if l.split() == [".amdhsa_kernel", name])
        d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        out[name] = (code, [" ".join(l.split(";")[0].split()) for l in lines[d0 + 1:d1]])
    return out


def verdict(old, new):
    if old == new:
        return "identical"
    ops = lambda code: collections.Counter(l.split()[0] for l in code if not l.endswith(":"))
    if old[1] == new[1] and ops(old[0]) == ops(new[0]):
        return "renamed-registers"
    return "different"


def compare(old_text, new_text, names, out=sys.stdout):
    """Prints one line per kernel; returns the verdicts, one per kernel."""
    old, new = kernels(old_text), kernels(new_text)
    got, seen = [], set()
    for name, k in old.items():
        to = names.get(name, name)
        seen.add(to)
        got.append(verdict(k, new[to]) if to in new else "unmatched (old)")
        print("%-18s %s%s" % (got[-1], name, "" if to == name else " -> " + to), file=out)
    for name in new:
        if name not in seen:
            got.append("unmatched (new)")
            print("%-18s %s" % (got[-1], name), file=out)
    return got


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--names", help="JSON object: old kernel name -> new kernel name")
    args = ap.parse_args()
    names = json.load(open(args.names)) if args.names else {}

    def read(path):  # a directory: its .s files as one pool (a kernel may change files)
        files = [os.path.join(path, f) for f in sorted(os.listdir(path)) if f.endswith(".s")] \
            if os.path.isdir(path) else [path]
        return "\n".join(open(f).read() for f in files)

    got = compare(read(args.old), read(args.new), names)
    bad = sum(v not in ("identical", "renamed-registers") for v in got)
    print("%d kernels: %d identical, %d renamed-registers, %d different or unmatched" %
          (len(got), got.count("identical"), got.count("renamed-registers"), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
