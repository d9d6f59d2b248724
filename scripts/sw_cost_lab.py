"""What having stateless-worker types set costs a batch that holds no such message (config 2's shape: 1M registered
long-key grains, 64M uniform messages, stages 1-4).  Routes the same device batch `reps` times with the types unset
(k_route, the 8-B probe table) and `reps` times with one type set (k_route_sw: the type test per message, and local
owners probe the 32-B table).  Prints event-timed step times; run it under `rocprofv3 --kernel-trace --stats` for the
two kernels' own times.  Lab script, not a test.

usage: python scripts/sw_cost_lab.py [n_msgs] [reps]
"""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from orleans_amd import _lib as L  # noqa: E402
from orleans_amd import workloads as W  # noqa: E402
from orleans_amd.engine import GrainDirectoryEngine  # noqa: E402

SW_TCD = (L.CAT_GRAIN << 56) | 0x5157


def main(n_msgs=64 << 20, reps=5):
    n_grains = 1_000_000
    cl = W.default_cluster()
    eng = GrainDirectoryEngine(n_act=n_grains, dir_capacity=n_grains, max_batch=n_msgs, device=0)
    W.setup_engine(eng, cl)
    keys, uni, owner, reg = W.grain_population(cl, n_grains)
    W.register_population(eng, keys, owner, reg)
    torch.cuda.set_stream(torch.cuda.Stream())
    st = torch.cuda.current_stream().cuda_stream
    m = W.device_messages(torch, cl, n_grains, n_msgs, W.SEED_C2)
    route, act, order = (torch.empty(n_msgs, dtype=torch.int32, device="cuda") for _ in range(3))
    offs = torch.empty(n_grains + 2, dtype=torch.int32, device="cuda")
    outs = {}
    for label, types in (("types unset", []), ("one type set", [SW_TCD])):
        eng.set_stateless_types(types, [1] * len(types))
        ts = []
        for i in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.address_messages_device(m, n_msgs, route, act, order, offs, stream=st)
            b.record()
            b.synchronize()
            if i:
                ts.append(a.elapsed_time(b))
        outs[label] = (route.clone(), act.clone(), order.clone(), offs.clone())
        print(f"{label}: step {np.median(ts):.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}); probe form "
              f"{eng.query(L.Q_PROBE_FORM)}", flush=True)
    same = all(torch.equal(x, y) for x, y in zip(outs["types unset"], outs["one type set"]))
    print("outputs identical:", same, flush=True)
    eng.close()


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:]))
