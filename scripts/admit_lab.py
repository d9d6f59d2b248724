"""What admission costs beside the stage 4 it follows, at config 2's shape: 1M activations, 64M messages per batch,
handles uniform or Zipf(1.1), 10 % responses, 20 % read-only requests, every activation VALID and idle at the start.
Times the wall clock of one orl_admit_device plus one stream synchronise, and in the same run of one orl_bucket_device
over the same handles: median, min and max of `reps` calls after `warm` warm-up calls, limits off and hard = 64.  The
state table is put back before every admission call (outside the timing).

    python scripts/admit_lab.py [reps] [warm] [log2 n] [log2 n_act]

Run it under `rocprofv3 --kernel-trace --stats` (small reps) for the kernels' own times.  Lab script, not a test."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from orleans_amd import _lib as L  # noqa: E402
from orleans_amd import workloads as W  # noqa: E402
from orleans_amd.engine import GrainDirectoryEngine  # noqa: E402


def timed(stream, reps, warm, call, before=None):
    ms = []
    for r in range(reps + warm):
        if before:
            before()
        stream.synchronize()
        t0 = time.perf_counter()
        call()
        stream.synchronize()
        if r >= warm:
            ms.append((time.perf_counter() - t0) * 1e3)
    return np.median(ms), min(ms), max(ms)


def main(reps=20, warm=3, log_n=26, log_act=20):
    n, n_act = 1 << log_n, 1 << log_act
    dev = torch.device("cuda", 0)
    eng = GrainDirectoryEngine(n_act=n_act, dir_capacity=16, max_batch=n, device=0)
    W.setup_engine(eng, W.default_cluster())
    torch.cuda.set_stream(torch.cuda.Stream())
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(16)
    u = torch.rand(n, device=dev, generator=g)
    mflags = (torch.where(u < 0.1, L.MF_RESPONSE, L.MF_REQUEST)
              | torch.where(torch.rand(n, device=dev, generator=g) < 0.2, L.MF_READ_ONLY, 0)).to(torch.uint8)
    state0 = np.zeros(n_act, L.ACT_STATE_DTYPE)
    state0["state"] = L.ACT_VALID
    d_state0 = torch.from_numpy(state0.view(np.uint8)).to(dev)
    d_state = d_state0.clone()
    order = torch.empty(n, dtype=torch.int32, device=dev)
    off = torch.empty(n_act + 2, dtype=torch.int32, device=dev)
    disp = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    cdf = torch.from_numpy(W.zipf_cdf(n_act, 1.1)).to(dev)
    print(f"admit_lab: n = {n}, n_act = {n_act}, reps = {reps}, warm = {warm}; ms: median min max", flush=True)
    for name in ("uniform", "zipf1.1"):
        if name == "uniform":
            act = torch.randint(0, n_act, (n,), device=dev, generator=g, dtype=torch.int32)
        else:
            act = torch.searchsorted(cdf, torch.rand(n, device=dev, generator=g, dtype=cdf.dtype)).clamp_(max=n_act - 1).to(torch.int32)
        stream.synchronize()
        b = timed(stream, reps, warm, lambda: eng.bucket_device(act, n, order, off, stream=sp))
        top = int(torch.bincount(act.long(), minlength=n_act).max())
        print(f"{name:8s} orl_bucket_device                 {b[0]:8.3f} {b[1]:8.3f} {b[2]:8.3f}   largest bucket {top}", flush=True)
        for hard in (0, 64):
            a = timed(stream, reps, warm,
                      lambda: eng.admit_device(act, mflags, n, order, off, d_state, disp, hard, 0, counts, stream=sp),
                      before=lambda: d_state.copy_(d_state0))
            c = counts.cpu().numpy()
            print(f"{name:8s} orl_admit_device hard = {hard:<3d}        {a[0]:8.3f} {a[1]:8.3f} {a[2]:8.3f}   "
                  f"{a[0] / b[0]:.2f} x stage 4; run {c[L.ADM_RUN]} enqueue {c[L.ADM_ENQUEUE]} response {c[L.ADM_RESPONSE]} "
                  f"overloaded {c[L.ADM_OVERLOADED]}", flush=True)
            assert int(c.sum()) == n
    eng.close()


if __name__ == "__main__":
    main(*(int(x) for x in sys.argv[1:]))
