#!/usr/bin/env python
"""Per-kernel comparison of two sets of gfx950 assembly files (hipcc --offload-arch=gfx950 --cuda-device-only -S).

    python tools/kernel_isa_diff.py --before old/parc_kin.s --after new/parc_kin.s new/parc_motion.s ... [--json out.json]

Each side is split at the function labels of its kernels; comments and directives are dropped, local label numbers (.LBB<n>_, .Ltmp<n>,
.LJTI<n>_) are normalised.  Per kernel name it reports the instruction counts, whether the two instruction streams are equal and whether
the .amdhsa_ resource lines (registers, accum offset, private and group segment) are equal.  A kernel that is missing on one side or
appears more than once on a side is a difference.  A kernel whose streams differ while its resource lines, its instruction count and the
multiset of its opcodes (the first token of each instruction) are equal - only register names or the order of instructions and operands
can then differ - is listed as "same-ops".  It compares and prints; it knows nothing about any instruction.
Exit status 0 when every kernel is equal, 2 when the rest are all same-ops, 1 otherwise."""
import argparse
import json
import re
import sys

LOCAL = re.compile(r"\.(LBB|Ltmp|LJTI|Lfunc_end|Lfunc_begin)\d+")
RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels_of(path):
    """{kernel name: [(instruction lines, resource lines)]} of one assembly file."""
    lines = open(path).read().split("\n")
    names = {m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m}
    body, res, cur = {}, {}, None
    for ln in lines:
        s = ln.split(";")[0].strip()
        m = re.match(r"(\S+):$", s)
        if m and not s.startswith("."):
            cur = m.group(1) if m.group(1) in names else None
            if cur:
                body.setdefault(cur, []).append([])
            continue
        if s.startswith(".end_amdhsa_kernel"):
            cur = None
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            cur = ("res", m.group(1))
            res.setdefault(m.group(1), []).append([])
            continue
        if isinstance(cur, tuple):
            if any(s.startswith(".amdhsa_" + r) for r in RESOURCES):
                res[cur[1]][-1].append(s)
        elif cur and s and (not s.startswith(".") or re.match(r"\.L\w+:$", s)):
            body[cur][-1].append(LOCAL.sub(lambda g: "." + g.group(1), " ".join(s.split())))
    return {k: list(zip(body.get(k, []), res.get(k, []))) for k in names}


def collect(paths):
    out = {}
    for p in paths:
        for k, v in kernels_of(p).items():
            out.setdefault(k, []).extend((p, b, r) for b, r in v)
    return out


def count(stream):
    return sum(not ln.endswith(":") for ln in stream)        # the local labels stay in the stream but are no instructions


def opcodes(stream):
    return sorted(ln.split()[0] for ln in stream if not ln.endswith(":"))       # the multiset of first tokens; equal lengths follow


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--before", nargs="+", required=True)
    ap.add_argument("--after", nargs="+", required=True)
    ap.add_argument("--json", help="also write the per-kernel table here")
    a = ap.parse_args()
    old, new = collect(a.before), collect(a.after)
    rows, ok, same_ops = [], True, 0
    for k in sorted(set(old) | set(new)):
        o, n = old.get(k, []), new.get(k, [])
        row = {"kernel": k, "before": [count(b) for _, b, _ in o], "after": [count(b) for _, b, _ in n], "after_file": [p.split("/")[-1] for p, _, _ in n]}
        row["once"] = len(o) == 1 and len(n) == 1
        row["stream_equal"] = row["once"] and o[0][1] == n[0][1]
        row["resources_equal"] = row["once"] and o[0][2] == n[0][2] and len(o[0][2]) == len(RESOURCES)
        row["opcodes_equal"] = row["once"] and opcodes(o[0][1]) == opcodes(n[0][1])
        row["verdict"] = "DIFFERS" if not row["resources_equal"] else "equal" if row["stream_equal"] else "same-ops" if row["opcodes_equal"] else "DIFFERS"
        ok &= row["verdict"] == "equal"
        same_ops += row["verdict"] == "same-ops"
        rows.append(row)
        print("{:8s} {:>6s} {:>6s}  {}  {}".format(row["verdict"],
              ",".join(map(str, row["before"])) or "-", ",".join(map(str, row["after"])) or "-", ",".join(row["after_file"]) or "-", k))
    differs = sum(r["verdict"] == "DIFFERS" for r in rows)
    print("{} kernels, {}".format(len(rows), "all equal" if ok else "{} same-ops, {} DIFFER".format(same_ops, differs)))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"kernels": rows, "all_equal": ok, "same_ops": same_ops, "differ": differs}, f, indent=1)
    return 0 if ok else 2 if not differs else 1


if __name__ == "__main__":
    sys.exit(main())
