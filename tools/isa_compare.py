#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two builds, kernel by kernel.

    hipcc $(CXXFLAGS) --cuda-device-only -S x.hip -o OLD_DIR/x.s      (same for NEW_DIR, same flags)
    tools/isa_compare.py OLD_DIR NEW_DIR [--md]

Reads every *.s in both folders and prints one row per kernel symbol: the resources from the code-object metadata
(VGPRs, AGPRs, SGPRs, scratch, LDS, workgroup size, spills) and a per-mnemonic histogram of the instruction stream.
A refactor that must not change what a kernel costs is held to (exit status 1 otherwise):
  * the same kernel symbols;
  * equal .vgpr_count, .agpr_count, scratch size, LDS size and maximal workgroup size;
  * VGPR / SGPR spill counts not above OLD's;
  * equal counts of every buffer_* / global_* / flat_* / scratch_*, ds_*, v_mfma_*, v_exp_* / v_rcp_* mnemonic, of
    s_barrier, and of every distinct `s_waitcnt` operand.
Every other mnemonic whose count differs, and whether the instruction streams are identical, is reported but not held
to anything: timing decides about those."""
import argparse
import collections
import glob
import os
import re
import sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
        ".max_flat_workgroup_size", ".vgpr_spill_count", ".sgpr_spill_count")
EQUAL = (".vgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
         ".max_flat_workgroup_size")
NOT_ABOVE = (".vgpr_spill_count", ".sgpr_spill_count")
GATED = re.compile(r"^(buffer_|global_|flat_|scratch_|ds_|v_mfma_|v_exp_|v_rcp_|s_barrier$|s_waitcnt )")


def parse(path):
    """{symbol: {"meta": {...}, "hist": Counter, "stream": [instruction lines]}} of one .s file"""
    lines = open(path).read().split("\n")
    kernels = {}
    # instruction streams: `sym:` after `.type sym,@function` up to `.Lfunc_end`
    funcs = set(m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", l) for l in lines) if m)
    cur = None
    for l in lines:
        m = re.match(r"^(\S+):", l)
        if m and m.group(1) in funcs:
            cur = kernels.setdefault(m.group(1), {"meta": {}, "hist": collections.Counter(), "stream": []})
            continue
        if l.startswith(".Lfunc_end"):
            cur = None
        if cur is None or not l.startswith("\t") or l[1:2] in (".", ";", ""):
            continue
        ins = re.sub(r"\s+", " ", l.split(";")[0].strip())
        if not ins:
            continue
        mn = ins.split(" ")[0]
        cur["hist"][ins if mn == "s_waitcnt" else mn] += 1
        cur["stream"].append(ins)
    # metadata: the amdhsa.kernels YAML list, one `- .agpr_count:` ... block per kernel
    block = None
    blocks = []
    for l in lines:
        if re.match(r"^  - \.", l):
            block = {}
            blocks.append(block)
            l = "    " + l[4:]
        elif not l.startswith("    "):
            block = None
        if block is not None:
            m = re.match(r"^    (\.\w+):\s*(\S+)\s*$", l)
            if m:
                block[m.group(1)] = m.group(2)
    for b in blocks:
        name = b.get(".name")
        if name in kernels and ".vgpr_count" in b:
            kernels[name]["meta"] = {k: int(b.get(k, 0)) for k in META}
    return {k: v for k, v in kernels.items() if v["meta"]}


def load(folder):
    out = {}
    for path in sorted(glob.glob(os.path.join(folder, "*.s"))):
        for sym, k in parse(path).items():
            out[(os.path.basename(path), sym)] = k
    return out


def short(sym):
    """lstm_static4_kernel<256,12,16,...> from the mangled name: template arguments that are plain integers / bools"""
    m = re.match(r"_ZN\d+\w+?\d+(lstm\w+?)I(.*?)EEv", sym)
    if not m:
        return sym
    args = re.findall(r"L[ib](\d+)E", m.group(2))
    return "%s<%s>" % (m.group(1), ",".join(args))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_dir")
    ap.add_argument("new_dir")
    ap.add_argument("--md", action="store_true", help="print the table as markdown")
    a = ap.parse_args()
    old, new = load(a.old_dir), load(a.new_dir)
    bad = 0
    rows = []
    for key in sorted(set(old) | set(new)):
        if key not in old or key not in new:
            rows.append((key[0], short(key[1]), "only in " + ("OLD" if key in old else "NEW"), "", "", "", "", "FAIL", "", ""))
            bad += 1
            continue
        o, n = old[key], new[key]
        fails = []
        for k in EQUAL:
            if o["meta"][k] != n["meta"][k]:
                fails.append("%s %d->%d" % (k, o["meta"][k], n["meta"][k]))
        for k in NOT_ABOVE:
            if n["meta"][k] > o["meta"][k]:
                fails.append("%s %d->%d" % (k, o["meta"][k], n["meta"][k]))
        other = []
        for mn in sorted(set(o["hist"]) | set(n["hist"])):
            if o["hist"][mn] != n["hist"][mn]:
                d = "%s %d->%d" % (mn, o["hist"][mn], n["hist"][mn])
                (fails if GATED.match(mn) else other).append(d)
        bad += 1 if fails else 0

        def pair(k):
            return "%d" % o["meta"][k] if o["meta"][k] == n["meta"][k] else "%d->%d" % (o["meta"][k], n["meta"][k])
        rows.append((key[0], short(key[1]), pair(".vgpr_count"), pair(".agpr_count"), pair(".sgpr_count"),
                     "%s/%s" % (pair(".private_segment_fixed_size"), pair(".group_segment_fixed_size")),
                     "%s/%s" % (pair(".vgpr_spill_count"), pair(".sgpr_spill_count")),
                     "FAIL: " + "; ".join(fails) if fails else "ok", "; ".join(other) if other else "-",
                     "yes" if o["stream"] == n["stream"] else "no (%d instr.)" % len(n["stream"])))
    head = ("file", "kernel", "VGPR", "AGPR", "SGPR", "scratch/LDS", "spills v/s", "held-to counts", "other mnemonics",
            "same stream")
    if a.md:
        print("| " + " | ".join(head) + " |")
        print("|" + "---|" * len(head))
        for r in rows:
            print("| " + " | ".join(r) + " |")
    else:
        for r in [head] + rows:
            print("\t".join(r))
    print("%d kernel symbols, %d outside the conditions" % (len(rows), bad), file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
