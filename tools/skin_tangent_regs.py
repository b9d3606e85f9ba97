#!/usr/bin/env python3
"""Registers and instruction counts of the skinning kernels from their gfx950 assembly (tools/asm_stats.sh), no GPU involved:

    ASM_TUS='k_skin k_skin_list' ASM_OUT=build/asm tools/asm_stats.sh
    git archive <parent> many_bone_ik_amd/csrc include | tar -x -C DIR
    ASM_TUS='k_skin k_skin_list' ASM_CSRC=DIR/many_bone_ik_amd/csrc ASM_OUT=DIR/asm tools/asm_stats.sh
    tools/skin_tangent_regs.py DIR/asm build/asm

writes profiles/skin_tangent_regs.json: the 24 kernels of the positions and normals tiers, parent against new -- VGPRs, SGPRs,
scratch, spills and the number of instructions must be equal -- and the 12 kernels of the tangent tier.
An instruction is a line of a kernel's body that is neither a label, a directive nor a comment.
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def pretty(mangled):
    m = re.search(r"\d+(mbik_skin_[a-z_]+)I((?:L[ib]n?\d+E)+)E", mangled)
    args = ", ".join(("-" if neg else "") + v for _, neg, v in re.findall(r"L([ib])(n?)(\d+)E", m.group(2)))
    return f"{m.group(1)}<{args}>"


def kernels(asm_dir):
    out = {}
    for tu in ("k_skin", "k_skin_list"):
        txt = open(os.path.join(asm_dir, tu + ".s")).read()
        meta = txt[txt.index("amdhsa.kernels:"):]
        for blk in meta.split("\n  - ")[1:]:
            f = dict(re.findall(r"\.(\w+):\s+(\S+)", blk))
            name = f.get("name", "")
            if "mbik_skin_" not in name:
                continue
            body = txt[txt.index("\n" + name + ":"):]
            body = body[:body.index("s_endpgm")]
            lines = [l.strip() for l in body.split("\n")[2:]]
            count = sum(1 for l in lines if l and not l.startswith((".", ";")) and not l.split(";")[0].strip().endswith(":")) + 1
            rec = {k: int(f[k]) for k in KEYS}
            rec["instructions"] = count
            rec["waves_per_simd"] = min(8, 512 // ((rec["vgpr_count"] + 7) // 8 * 8))
            out[pretty(name)] = rec
    return out


def main():
    parent, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    rows = [{"kernel": k, "parent": parent[k], "new": new[k], "equal": parent[k] == new[k]} for k in sorted(parent)]
    added = [{"kernel": k, **new[k]} for k in sorted(new) if k not in parent]
    doc = {
        "what": "the 24 skinning kernels of the positions and normals tiers (k_skin.hip, k_skin_list.hip) before and after the tangent "
                "tier was added to skin_dev.h's block body, and the tier's 12 kernels; cross-compiled for gfx950 with the library's flags",
        "recipe": "tools/skin_tangent_regs.py PARENT_ASM NEW_ASM (see its head)",
        "waves_per_simd": "min(8, floor(512 / round_up(vgpr_count, 8)))",
        "conditions": "every existing kernel: registers, scratch, spills and instruction count equal to the parent's; every new kernel: "
                      "no scratch, no spills",
        "existing_equal": all(r["equal"] for r in rows) and len(rows) == 24,
        "new_without_scratch_or_spills": len(added) == 12 and all(
            a["private_segment_fixed_size"] == 0 and a["vgpr_spill_count"] == 0 and a["sgpr_spill_count"] == 0 for a in added),
        "existing": rows,
        "tangent_tier": added,
    }
    path = os.path.join(ROOT, "profiles", "skin_tangent_regs.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(path, "existing_equal:", doc["existing_equal"], "new clean:", doc["new_without_scratch_or_spills"])
    return 0 if doc["existing_equal"] and doc["new_without_scratch_or_spills"] else 1


if __name__ == "__main__":
    sys.exit(main())
