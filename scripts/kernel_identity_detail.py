#!/usr/bin/env python3
"""What exactly differs where scripts/kernel_identity.py reports a finding: the same extraction from the same two object
directories, then per matched kernel the note fields that changed, every changed instruction (before -> after) of a kernel
that kept its instruction count, and instructions / VGPRs / SGPRs / scratch / LDS before -> after of one that did not.
usage: scripts/kernel_identity_detail.py [--rename REGEX=REPL]... BEFORE/_obj AFTER/_obj"""
import argparse
import collections
import difflib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_identity as K  # noqa: E402

RES = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def main(before_dir, after_dir, renames):
    (b, _), (a, _) = K.kernels_of(before_dir), K.kernels_of(after_dir)
    names = sorted(set(b) | set(a))
    short = dict(zip(names, K.run("c++filt", input="\n".join(names)).splitlines()))

    def name_of(s, rename):
        n = short[s].replace("void ", "")
        for pattern, repl in (renames if rename else ()):
            n = re.sub(pattern, repl, n)
        return n

    b = {name_of(s, True): v for s, v in b.items()}
    a = {name_of(s, False): v for s, v in a.items()}
    notes, pairs, resized = collections.Counter(), collections.defaultdict(list), []
    for s in sorted(set(a) & set(b)):
        (_, tb, mb), (_, ta, ma) = b[s], a[s]
        for k in sorted(set(mb) | set(ma)):
            if k != "symbol" and mb.get(k) != ma.get(k):
                notes[f"{k} {mb.get(k)} -> {ma.get(k)}"] += 1
        if len(tb) != len(ta):
            row = lambda m, t: (len(t),) + tuple(int(m[f]) for f in RES)
            resized.append((s.split("(")[0], row(mb, tb), row(ma, ta)))
        elif tb != ta:
            for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, tb, ta, autojunk=False).get_opcodes():
                if tag != "equal":
                    pairs[s.split("(")[0]].append(f"{' ; '.join(tb[i1:i2])}  ->  {' ; '.join(ta[j1:j2])}")
    print("note fields that changed (field before -> after: kernels):")
    for k, n in sorted(notes.items()):
        print(f"  {k}: {n}")
    print("kernels with the same instruction count: every changed instruction")
    for s, ps in sorted(pairs.items()):
        print(f"  {s}: {len(ps)}")
        for p in ps:
            print(f"    {p}")
    print("kernels with another instruction count: (instructions, VGPRs, SGPRs, scratch, LDS) before -> after")
    for s, x, y in resized:
        print(f"  {s}: {x} -> {y}{'   RISES' if any(q > p for p, q in zip(x, y)) else ''}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("before")
    ap.add_argument("after")
    args = ap.parse_args()
    main(args.before, args.after, [r.split("=", 1) for r in args.rename])
