"""Static branch census of one solve kernel by source site.

Compile the TU with line tables into a build directory (never the shipped library):
    tools/asm_stats.sh -gline-tables-only        -> build/asm/k_solve_rw.s
    python tools/branch_census.py [kernel-substring] [build/asm/<tu>.s] [top]
Every instruction belongs to the source line of the last .loc before it (the innermost inlined
frame).  Branch sites are s_cbranch_* and s_branch; s_and_saveexec / s_or_saveexec are counted
beside them (a divergent `if` is one saveexec plus one s_cbranch_execz).  A helper-wave kernel
holds both waves' code: an instruction counts towards the helper when the last solve_block.h
line seen before it lies in the helper's loop (the lines between `if (wave == 1)` and its
`return`), so the solving path is everything else.  Prints one JSON object."""
import collections
import json
import re
import sys

name = sys.argv[1] if len(sys.argv) > 1 else "mbik_solve_kernel_helpILi103"
path = sys.argv[2] if len(sys.argv) > 2 else "build/asm/k_solve_rw.s"
top = int(sys.argv[3]) if len(sys.argv) > 3 else 40
s = open(path).read().split("\n")
files = {}
for l in s:
    m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
    if m:
        files[int(m.group(1))] = (m.group(3) or m.group(2)).rsplit("/", 1)[-1]
start = next(i for i, l in enumerate(s) if name in l and l.startswith("_Z") and l.split(";")[0].rstrip().endswith(":"))
end = next(i for i in range(start, len(s)) if s[i].startswith(".Lfunc_end"))


def helper_range():
    src = open("many_bone_ik_amd/csrc/solve_block.h").read().split("\n")
    a = next(i for i, l in enumerate(src) if "if (wave == 1)" in l) + 1
    b = next(i for i in range(a, len(src)) if src[i].strip() == "return;") + 1
    return a, b


h0, h1 = helper_range()
site = ("?", 0)
in_helper = False
tot = collections.Counter()
by_site = collections.defaultdict(collections.Counter)
for l in s[start:end]:
    t = l.strip()
    m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
    if m:
        site = (files.get(int(m.group(1)), m.group(1)), int(m.group(2)))
        if site[0] == "solve_block.h":
            in_helper = h0 <= site[1] <= h1
        continue
    if not t or t.startswith((".", ";")) or t.endswith(":") or ":" in t.split()[0]:
        continue
    op = t.split()[0]
    kind = ("branch" if op.startswith(("s_cbranch", "s_branch")) else "saveexec" if "saveexec" in op else
            "waitcnt" if op == "s_waitcnt" else "nop" if op == "s_nop" else "valu" if op.startswith("v_") else
            "salu" if op.startswith("s_") else "mem")
    part = "helper" if in_helper else "solver"
    tot[part + "_" + kind] += 1
    tot[part + "_insts"] += 1
    if op == "s_cbranch_execz":
        tot[part + "_cbranch_execz"] += 1
    if kind in ("branch", "saveexec") and not in_helper:
        by_site["%s:%d" % site][kind] += 1
rank = sorted(by_site.items(), key=lambda kv: -kv[1]["branch"])
print(json.dumps({"kernel": name, "static": dict(sorted(tot.items())),
                  "solver_sites_ranked": [{"site": k, "branches": v["branch"], "saveexec": v["saveexec"]} for k, v in rank[:top]],
                  "solver_sites": len(rank)}, indent=1))
