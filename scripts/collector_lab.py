"""What the activation collector's calls cost, at 1M and 16M activations.  Times the wall clock of one call plus one stream
synchronise; median, min and max of `reps` calls after `warm` warm-up calls, the state restored before each (outside the
timing).  Each scan is set beside a plain streamed read (torch's sum) of the same ticket[] array measured in the same run:
the pattern floor of 8 B x n_act.  The touch, over a batch of 2^log_n messages with uniform handles, is set beside
orl_admit_device over the same batch; orl_collect_on_complete_device gets one record per ORL_ADM_RUN message.

Start state: every activation VALID and idle, age limit 2 quanta, ticketed for the second quantum, idle for 3 quanta
except where noted.  The scans:
  nothing due      ScanStale one quantum in: no ticket is below next_ticket (the pure stream over ticket[])
  all due, 1/16    ScanStale three quanta in: every ticket is due; 15 of 16 activations became idle late, so they are
                   rescheduled (ticket rewritten) and 1 of 16 is condemned
  all due, all     the same with every activation stale: all condemned
  ScanAll 1/16     ScanAll over the same state as "all due, 1/16"

    python scripts/collector_lab.py [reps] [warm] [log2 n]

Lab script, not a test."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from orleans_amd import _lib as L  # noqa: E402
from orleans_amd import workloads as W  # noqa: E402
from orleans_amd.engine import GrainDirectoryEngine  # noqa: E402

SEC = L.TICKS_PER_SECOND
QT = 60 * SEC
T0 = 630_000_000 * SEC


class DevArray:
    """A device pointer as something torch.as_tensor can wrap without a copy."""

    def __init__(self, p, count, typestr):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (int(p), False), "version": 2}


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


def row(name, r, extra=""):
    print(f"  {name:44s} {r[0]:8.3f} {r[1]:8.3f} {r[2]:8.3f}   {extra}", flush=True)


def run(eng, n_act, n, reps, warm, stream, dev):
    sp = stream.cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(18)
    state0 = np.zeros(n_act, L.ACT_STATE_DTYPE)
    state0["state"] = L.ACT_VALID
    d_state0 = torch.from_numpy(state0.view(np.uint8)).to(dev)
    d_state = d_state0.clone()
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    ticket0 = torch.full((n_act,), T0 + 2 * QT, dtype=torch.int64, device=dev)
    age0 = torch.full((n_act,), 2 * QT, dtype=torch.int64, device=dev)
    idle_all = torch.full((n_act,), T0 - 3 * QT, dtype=torch.int64, device=dev)
    idle_16 = torch.where(torch.arange(n_act, device=dev) % 16 == 0, T0 - 3 * QT, T0 + 2 * QT)
    box = {}

    def fresh(idle):
        box["col"] = col = eng.collector_create(QT, T0)
        torch.cuda.synchronize()  # a build before DESIGN §19 returned with its zero-fill still running on the null stream
        v = eng.collector_view(col)
        for p, src in ((v.d_ticket, ticket0), (v.d_age_limit, age0), (v.d_became_idle, idle)):
            eng.copy_on_device(p, src, 8 * n_act, stream=sp)
        d_state.copy_(d_state0)
        box["view"] = v
        try:
            box["ticket"] = torch.as_tensor(DevArray(v.d_ticket, n_act, "<i8"), device=dev)
        except Exception as e:  # no zero-copy wrap in this torch: read an array of the same size and say so
            print(f"  (ticket[] not wrapped: {type(e).__name__}; the read below is of a torch array of the same size)", flush=True)
            box["ticket"] = ticket0

    def drop():
        box.pop("ticket", None)
        eng.collector_destroy(box.pop("col"))

    print(f"n_act = {n_act}: ticket[] is {8 * n_act / 2**20:.0f} MiB", flush=True)
    fresh(idle_all)
    tk = box["ticket"]
    stream.synchronize()
    assert int(tk[0]) == T0 + 2 * QT
    fl = timed(stream, reps, warm, lambda: tk.sum())
    row("streamed read of ticket[] (torch sum)", fl, f"{8 * n_act / fl[0] / 1e6:.0f} GB/s")
    drop()

    def scan(name, idle, now, all_age=None, expect=None):
        call = ((lambda: eng.collect_scan_all_device(box["col"], d_state, all_age, now, counts, stream=sp)) if all_age
                else (lambda: eng.collect_scan_stale_device(box["col"], d_state, now, counts, stream=sp)))
        r = timed(stream, reps, warm, call, before=lambda: fresh(idle), after=drop)
        c = counts.cpu().numpy()
        row(name, r, f"{r[0] / fl[0]:.2f} x the read; candidates {c[L.SCAN_CANDIDATES]} condemned {c[L.SCAN_CONDEMNED]}")
        assert expect is None or int(c[L.SCAN_CONDEMNED]) == expect, (c, expect)

    scan("ScanStale, nothing due", idle_all, T0 + QT, expect=0)
    scan("ScanStale, all due, 1/16 condemned", idle_16, T0 + 3 * QT, expect=(n_act + 15) // 16)
    scan("ScanStale, all due, all condemned", idle_all, T0 + 3 * QT, expect=n_act)
    scan("ScanAll(2 quanta), 1/16 condemned", idle_16, T0 + 3 * QT, all_age=2 * QT, expect=(n_act + 15) // 16)

    # touch and on-complete behind an admitted batch of n messages
    act = torch.randint(0, n_act, (n,), device=dev, generator=g, dtype=torch.int32)
    u = torch.rand(n, device=dev, generator=g)
    mflags = (torch.where(u < 0.1, L.MF_RESPONSE, L.MF_REQUEST)
              | torch.where(torch.rand(n, device=dev, generator=g) < 0.2, L.MF_READ_ONLY, 0)).to(torch.uint8)
    del u
    order = torch.empty(n, dtype=torch.int32, device=dev)
    off = torch.empty(n_act + 2, dtype=torch.int32, device=dev)
    disp = torch.empty(n, dtype=torch.uint8, device=dev)
    stream.synchronize()
    eng.bucket_device(act, n, order, off, stream=sp)
    a = timed(stream, reps, warm, lambda: eng.admit_device(act, mflags, n, order, off, d_state, disp, 0, 0, counts, stream=sp),
              before=lambda: d_state.copy_(d_state0))
    row(f"orl_admit_device, {n} messages", a)
    d_state_adm = d_state.clone()

    def fresh_adm():
        fresh(idle_all)
        d_state.copy_(d_state_adm)

    now = T0 + QT + 7
    t = timed(stream, reps, warm, lambda: eng.collect_touch_device(box["col"], act, disp, n, d_state, now, 0, 0, counts, stream=sp),
              before=fresh_adm, after=drop)
    c = counts.cpu().numpy()
    row(f"orl_collect_touch_device, {n} messages", t,
        f"{t[0] / a[0]:.2f} x admission; touched {c[L.COL_TOUCHED]} moved {c[L.COL_MOVED]}")
    ran = disp == L.ADM_RUN
    cact = act[ran].contiguous()
    ctok = torch.arange(int(cact.numel()), dtype=torch.int32, device=dev)
    m = int(cact.numel())
    k = timed(stream, reps, warm, lambda: eng.collect_on_complete_device(box["col"], cact, ctok, m, d_state, now, counts, stream=sp),
              before=fresh_adm, after=drop)
    c = counts.cpu().numpy()
    row(f"orl_collect_on_complete_device, {m} records", k,
        f"{k[0] / a[0]:.2f} x admission; became idle {c[L.COL_BECAME_IDLE]} moved {c[L.COL_MOVED]}")


def main(reps=20, warm=3, log_n=26):
    n = 1 << log_n
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream())
    stream = torch.cuda.current_stream()
    print(f"collector_lab: reps = {reps}, warm = {warm}, batch = {n} messages; ms: median min max", flush=True)
    for log_act in (20, 24):
        eng = GrainDirectoryEngine(n_act=1 << log_act, dir_capacity=16, max_batch=n, device=0)
        W.setup_engine(eng, W.default_cluster())
        run(eng, 1 << log_act, n, reps, warm, stream, dev)
        eng.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(*(int(x) for x in sys.argv[1:]))
