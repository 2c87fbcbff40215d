#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds the same?  Takes the code objects out of every *.o of two lib.build() object
directories and compares, kernel symbol by kernel symbol, the instruction text (addresses, encodings and label names
dropped) and the scalar fields of the code-object notes (VGPR / SGPR / AGPR counts, scratch, LDS, max_flat_workgroup_size,
kernarg size, spill counts).  Prints one line per kernel that changed its object file or differs, one line per object
whose kernels all stayed and are identical, and exits 1 on any lost, new, duplicated or differing kernel.
Kernels are matched by demangled name.  --rename REGEX=REPL (repeatable) rewrites the BEFORE names first, for a kernel that
lost a template argument; a renamed kernel is compared without the .symbol note field, which carries the name.
--lost-ok REGEX (repeatable): a BEFORE kernel without a partner whose name matches is printed as retired, not as a finding.
usage: scripts/kernel_identity.py [--rename REGEX=REPL]... [--lost-ok REGEX]... BEFORE/_obj AFTER/_obj"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
          "max_flat_workgroup_size")


def run(*cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def kernels_of(objdir):
    """{symbol: (object name, [instruction text], {note field: value})}, and the symbols seen in more than one object"""
    found, dup = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(objdir, "*.o"))):
            name = os.path.basename(obj)
            local = os.path.join(tmp, name)
            os.symlink(os.path.abspath(obj), local)
            run(os.path.join(LLVM, "llvm-objdump"), "--offloading", name, cwd=tmp)   # writes NAME.<n>.<target> beside it
            for co in glob.glob(local + ".*gfx950"):
                notes = {}
                for entry in re.split(r"^  - (?=\.)", run(os.path.join(LLVM, "llvm-readelf"), "--notes", co), flags=re.M)[1:]:
                    scalars = dict(re.findall(r"^    \.(\w+): +(\S+)$", "    " + entry, flags=re.M))
                    if "name" in scalars:
                        notes[scalars.pop("name")] = scalars
                # a function ends where its symbol does: the alignment padding behind it belongs to no kernel
                end = {}
                for line in run(os.path.join(LLVM, "llvm-readelf"), "-s", "--wide", co).splitlines():
                    f = line.split()
                    if len(f) == 8 and f[3] == "FUNC":
                        end[f[7]] = int(f[1], 16) + int(f[2], 0)
                text, cur = {}, None
                for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", co).splitlines():
                    m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
                    if m:
                        cur, stop = text.setdefault(m[1], []), end.get(m[1], 0)
                        continue
                    m = re.match(r"\t(.+?)\s*// ([0-9A-F]+):", line)
                    if m and cur is not None and int(m[2], 16) < stop:
                        cur.append(" ".join(m[1].split()))
                for sym, meta in notes.items():
                    insns = text.get(sym, [])
                    if sym in found:
                        dup.append(sym)
                    found[sym] = (name, insns, meta)
    return found, dup


def main(before_dir, after_dir, renames=(), lost_ok=()):
    (before, dup_b), (after, dup_a) = kernels_of(before_dir), kernels_of(after_dir)
    names = sorted(set(before) | set(after))
    short = dict(zip(names, run("c++filt", input="\n".join(names)).splitlines()))
    bad, stayed, retired, renamed = 0, {}, 0, set()
    for s in dup_b + dup_a:
        bad += 1
        print(f"DUPLICATED across objects ({'before' if s in dup_b else 'after'}): {short[s]}")

    def new_name(name):
        for pattern, repl in renames:
            name = re.sub(pattern, repl, name)
        return name

    n_before = len(before)
    before = {new_name(short[s]): v for s, v in before.items()}
    after = {short[s]: v for s, v in after.items()}
    if len(before) != n_before:
        bad += 1
        print(f"--rename maps {n_before - len(before)} BEFORE kernels onto the name of another one")
    for s in sorted(set(before) | set(after)):
        if s not in before or s not in after:
            if s in before and any(re.search(p, s) for p in lost_ok):
                retired += 1
                print(f"retired: {s}")
                continue
            bad += 1
            print(f"{'NEW' if s not in before else 'LOST'}: {s}")
            continue
        (ob, tb, mb), (oa, ta, ma) = before[s], after[s]
        if mb.get("symbol") != ma.get("symbol"):        # only a renamed kernel: the field carries the mangled name
            mb, ma = ({k: v for k, v in m.items() if k != "symbol"} for m in (mb, ma))
            renamed.add(s)
        same_text, same_meta = tb == ta and len(tb) > 0, mb == ma and len(mb) > 0
        if ob == oa and same_text and same_meta:
            stayed[oa] = stayed.get(oa, 0) + 1
            continue
        verdict = "identical" if same_text and same_meta else "DIFFERS:" + " text" * (not same_text) + " notes" * (not same_meta)
        bad += verdict != "identical"
        res = " ".join(f"{mb.get(f, '?')}/{ma.get(f, '?')}" for f in FIELDS)
        print(f"{s.replace('void ', '')}{' (renamed)' * (s in renamed)}\n    {ob} -> {oa}  insns {len(tb)}/{len(ta)}  {res}  {verdict}")
        if not same_text:
            for i, (x, y) in enumerate(zip(tb, ta)):
                if x != y:
                    print(f"    first difference at instruction {i}: {x!r} / {y!r}")
                    break
    for o in sorted(stayed):
        print(f"{o}: {stayed[o]} kernels stayed, text and notes identical")
    print(f"{len(before)} kernels before, {len(after)} after, {retired} retired, {len(renamed)} renamed, {bad} findings")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("--lost-ok", action="append", default=[], metavar="REGEX")
    ap.add_argument("before")
    ap.add_argument("after")
    args = ap.parse_args()
    sys.exit(main(args.before, args.after, [r.split("=", 1) for r in args.rename], args.lost_ok))
