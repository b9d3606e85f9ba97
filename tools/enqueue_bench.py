"""Host-side cost of a solve call: back-to-back mbik_solve enqueues of a tiny batch (C1 x 8
skeletons), no synchronisation inside the loop and one at the end.  Every call runs the layout
decision (ensure_schedule, resolve_launch).

    [MBIK_LIB_OVERRIDE=other/libmbik.so] python tools/enqueue_bench.py [CALLS [REPEATS]]

Two plans: the rig's own iteration count, whose kernel (~0.4 ms) is longer than the call, so the
loop's total is device time; and one iteration per frame, a launch cheap enough for the host to be
the bound.  Per plan and repeat two figures, microseconds per call: `enqueue` up to the loop's
return (the host's share, as long as the runtime's queue takes the launches without blocking) and
`total` including the final synchronisation.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from many_bone_ik_amd import _lib  # noqa: E402
from many_bone_ik_amd import workloads as W  # noqa: E402
from many_bone_ik_amd.solver import Plan  # noqa: E402


def main(calls=2000, repeats=4):
    dev = torch.device("cuda", 0)
    wl = W.generate(1, 8)
    pi = torch.from_numpy(wl.pose).to(dev)
    tg = torch.from_numpy(wl.targets).to(dev)
    po = torch.empty_like(pi)
    out = {"lib": os.path.basename(_lib.LIB_PATH), "calls": calls}
    for name, kw in (("full", {}), ("one_iteration", {"iterations": 1})):
        plan = Plan.from_workload(wl, **kw)
        solve = plan._L.mbik_solve
        args = (plan.h, 0, 8, C.c_void_p(pi.data_ptr()), C.c_void_p(tg.data_ptr()), C.c_void_p(po.data_ptr()), None)
        for _ in range(200):
            solve(*args)
        torch.cuda.synchronize()
        enqueue, total = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(calls):
                solve(*args)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            enqueue.append(round((t1 - t0) / calls * 1e6, 3))
            total.append(round((t2 - t0) / calls * 1e6, 3))
        out[name] = {"enqueue_us": enqueue, "total_us": total}
        plan.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
