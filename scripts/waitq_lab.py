"""What the waiting queues cost beside the admission and the stage 4 they follow, at config 2's shape: 1M activations, 64M
messages per batch, handles uniform or Zipf(1.1), 10 % responses, 20 % read-only requests, every activation VALID and
idle at the start, hard = 0.  Times the wall clock of one call plus one stream synchronise: orl_bucket_device and
orl_admit_device over the batch (for scale), orl_waitq_append_device behind that admission, then orl_bucket_device and
orl_complete_device over a completion list that finishes every running request (one record per ORL_ADM_RUN message).
Median, min and max of `reps` calls after `warm` warm-up calls.  Before every timed append the queue is a new, empty one;
before every timed complete it is a new one with that append redone and the table is the one admission left (all outside
the timing).

    python scripts/waitq_lab.py [reps] [warm] [log2 n] [log2 n_act]

Run it under `rocprofv3 --kernel-trace --stats` (small reps) for the kernels' own times.  Lab script, not a test."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from orleans_amd import _lib as L  # noqa: E402
from orleans_amd import workloads as W  # noqa: E402
from orleans_amd.engine import GrainDirectoryEngine  # noqa: E402


def timed(stream, reps, warm, call, before=None, after=None):
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
        if after:
            after()
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
    tok = torch.arange(n, dtype=torch.int32, device=dev)
    state0 = np.zeros(n_act, L.ACT_STATE_DTYPE)
    state0["state"] = L.ACT_VALID
    d_state0 = torch.from_numpy(state0.view(np.uint8)).to(dev)
    d_state = d_state0.clone()
    order = torch.empty(n, dtype=torch.int32, device=dev)
    off = torch.empty(n_act + 2, dtype=torch.int32, device=dev)
    coff = torch.empty(n_act + 2, dtype=torch.int32, device=dev)
    disp = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    cdf = torch.from_numpy(W.zipf_cdf(n_act, 1.1)).to(dev)
    print(f"waitq_lab: n = {n}, n_act = {n_act}, reps = {reps}, warm = {warm}; ms: median min max", flush=True)
    for name in ("uniform", "zipf1.1"):
        if name == "uniform":
            act = torch.randint(0, n_act, (n,), device=dev, generator=g, dtype=torch.int32)
        else:
            act = torch.searchsorted(cdf, torch.rand(n, device=dev, generator=g, dtype=cdf.dtype)).clamp_(max=n_act - 1).to(torch.int32)
        stream.synchronize()
        b = timed(stream, reps, warm, lambda: eng.bucket_device(act, n, order, off, stream=sp))
        print(f"{name:8s} orl_bucket_device (batch)         {b[0]:8.3f} {b[1]:8.3f} {b[2]:8.3f}", flush=True)
        a = timed(stream, reps, warm,
                  lambda: eng.admit_device(act, mflags, n, order, off, d_state, disp, 0, 0, counts, stream=sp),
                  before=lambda: d_state.copy_(d_state0))
        c = counts.cpu().numpy()
        print(f"{name:8s} orl_admit_device                  {a[0]:8.3f} {a[1]:8.3f} {a[2]:8.3f}   "
              f"run {c[L.ADM_RUN]} enqueue {c[L.ADM_ENQUEUE]} response {c[L.ADM_RESPONSE]}", flush=True)
        d_state_adm = d_state.clone()
        ran = disp == L.ADM_RUN
        cact, ctok = act[ran].contiguous(), tok[ran].contiguous()
        m = int(cact.numel())
        corder = torch.empty(m, dtype=torch.int32, device=dev)
        box = {}

        def fresh(appended):
            box["q"] = eng.waitq_create(n)
            torch.cuda.synchronize()  # a build before DESIGN §19 returned with its fills still running on the null stream
            if appended:
                eng.waitq_append_device(box["q"], tok, mflags, n, order, off, disp, stream=sp)
                d_state.copy_(d_state_adm)

        def drop():
            eng.waitq_destroy(box.pop("q"))

        stream.synchronize()
        p = timed(stream, reps, warm, lambda: eng.waitq_append_device(box["q"], tok, mflags, n, order, off, disp, stream=sp),
                  before=lambda: fresh(False), after=drop)
        print(f"{name:8s} orl_waitq_append_device           {p[0]:8.3f} {p[1]:8.3f} {p[2]:8.3f}   "
              f"{p[0] / a[0]:.2f} x admission, {p[0] / b[0]:.2f} x stage 4", flush=True)
        cb = timed(stream, reps, warm, lambda: eng.bucket_device(cact, m, corder, coff, stream=sp))
        print(f"{name:8s} orl_bucket_device (completions)   {cb[0]:8.3f} {cb[1]:8.3f} {cb[2]:8.3f}   m = {m}", flush=True)
        k = timed(stream, reps, warm,
                  lambda: eng.complete_device(box["q"], cact, ctok, m, corder, coff, d_state, counts, stream=sp),
                  before=lambda: fresh(True), after=drop)
        c = counts.cpu().numpy()
        print(f"{name:8s} orl_complete_device               {k[0]:8.3f} {k[1]:8.3f} {k[2]:8.3f}   "
              f"{k[0] / a[0]:.2f} x admission, {k[0] / b[0]:.2f} x stage 4; completions {c[L.CMP_COMPLETIONS]} "
              f"underflows {c[L.CMP_UNDERFLOWS]} run {c[L.CMP_RUN]} still waiting {c[L.CMP_WAITING]}", flush=True)
        assert int(c[L.CMP_COMPLETIONS]) == m and int(c[L.CMP_UNDERFLOWS]) == 0
    eng.close()


if __name__ == "__main__":
    main(*(int(x) for x in sys.argv[1:]))
