#!/usr/bin/env python3
"""Which sg:: functions differ between two device assemblies of engine.hip?

    hipcc --offload-arch=gfx950 --cuda-device-only -O3 -std=c++17 -ffp-contract=off -S engine.hip -o X.s   (twice)
    python tools/kernel_asm_diff.py parent.s new.s [-v]

A function's body is its instruction lines: comments and directives dropped, .LBB<n>_<m> / .Ltmp<n> labels renumbered relative
to the function, so a function that merely moved in the file compares equal.  Prints one line per function that differs, was
added or was removed (-v: the first differing lines); exit status 1 if there is any."""
import re
import sys


def functions(path):
    out, name, body, labels = {}, None, [], {}

    def rel(m):
        return labels.setdefault(m.group(0), "L%d" % len(labels))

    for line in open(path):
        m = re.match(r"^(_ZN2sg\w+):", line)
        if m:
            name, body, labels = m.group(1), [], {}
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name], name = body, None
            continue
        s = line.split(";", 1)[0].strip()
        if not s or (s.startswith(".") and not s.endswith(":")):
            continue
        body.append(re.sub(r"\.LBB\d+_\d+|\.Ltmp\d+", rel, s))
    return out


def main():
    verbose = "-v" in sys.argv
    a, b = [functions(p) for p in sys.argv[1:] if p != "-v"]
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("%s  %s" % ("added  " if name in b else "removed", name))
        elif a[name] != b[name]:
            print("differs  %s  (%d -> %d instructions)" % (name, len(a[name]), len(b[name])))
            if verbose:
                at = next((i for i, (x, y) in enumerate(zip(a[name], b[name])) if x != y), min(len(a[name]), len(b[name])))
                for x, y in list(zip(a[name], b[name]))[at:at + 8]:
                    print("    %-60s | %s" % (x, y))
        else:
            continue
        bad += 1
    print("%d of %d sg:: functions differ" % (bad, len(set(a) | set(b))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
