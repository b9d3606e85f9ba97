#!/bin/bash
# Device assembly of the solve and the skinning kernel TUs plus per-kernel register / scratch usage:
#   tools/asm_stats.sh [extra hipcc flags]      -> build/asm/<tu>.s
# ASM_CSRC=dir: the csrc of another revision, inside a tree that also holds include/ (plan.h reads ../../include/mbik.h),
#   e.g. git archive <parent> many_bone_ik_amd/csrc include | tar -x -C DIR, then ASM_CSRC=DIR/many_bone_ik_amd/csrc;
# ASM_TUS="k_skin k_skin_list": some of the units only; ASM_OUT=dir: where the assembly goes; ASM_JSON=file: the printed records, {kernel: counts}.
set -e
cd "$(dirname "$0")/.."
export ASM_CSRC="${ASM_CSRC:-many_bone_ik_amd/csrc}" ASM_OUT="${ASM_OUT:-build/asm}"
export ASM_TUS="${ASM_TUS:-k_solve_w1 k_solve_w2 k_solve_rw k_cmode k_skin k_skin_list}"
mkdir -p "$ASM_OUT"
pids=()
for tu in $ASM_TUS; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -Wno-unused-result -Wno-unused-command-line-argument \
    --cuda-device-only -S "$@" "$ASM_CSRC/$tu.hip" -o "$ASM_OUT/$tu.s" &
  pids+=($!)
done
for pid in "${pids[@]}"; do wait "$pid"; done   # (set -e: a unit that does not compile ends the script, its errors shown)
python3 - <<'PY'
import json, os, re
out = {}
for tu in os.environ["ASM_TUS"].split():
  txt = open(f"{os.environ['ASM_OUT']}/{tu}.s").read()
  meta = txt[txt.index("amdhsa.kernels:"):]
  for blk in meta.split("\n  - ")[1:]:
    f = dict(re.findall(r"\.(\w+):\s+(\S+)", blk))
    n = f.get("name", "?")
    if any(k in n for k in ("solve_kernel", "group_kernel", "cmode_kernel", "mbik_skin_")):
        if "mbik_skin_" in n:  # (template arguments tell the instantiations apart)
            m = re.search(r"\d+(mbik_skin_[a-z_]+)I((?:L[ib]n?\d+E)+)E", n)
            args = ", ".join(("-" if neg else "") + v for _, neg, v in re.findall(r"L([ib])(n?)(\d+)E", m.group(2)))
            n = f"{m.group(1)}<{args}>"
        else:
            n = n.replace("_ZN12_GLOBAL__N_1", "")[:40]
        out[n] = {k: int(f[k]) if f.get(k, "").isdigit() else f.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
        print(n, out[n])
if os.environ.get("ASM_JSON"):
    json.dump(out, open(os.environ["ASM_JSON"], "w"), indent=1)
PY
