"""What one maintainer sweep costs at the reference's operating point: an adaptive cache of 1M entries (GlobalConfiguration's
default CacheSize), full; about half of the entries expired, about half of those accessed since — so a sweep keeps ~500k
entries, removes ~250k and lists ~250k for refresh (AdaptiveDirectoryCacheMaintainer.cs:54-143).  A sweep changes the table,
so every repetition rebuilds the same state first (configure, fill, one route batch over the accessed quarter); only
orl_cache_maintain_device plus one stream synchronise is timed.

The comparison is the floor of ANY host-side maintainer on the same machine: it has to read the table (slots of 32 B)
and the stamps (8 B per slot) before it can decide anything, so the device-to-host copy of those bytes into pinned memory
is timed too, same repetitions.  Nothing else is measured here.
    python scripts/cache_maintain_lab.py [reps] [warm]
Lab script, not a test."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from orleans_amd import _lib as L  # noqa: E402
from orleans_amd import workloads as W  # noqa: E402
from orleans_amd.engine import GrainDirectoryEngine  # noqa: E402

CAP, NB = 1_000_000, 1 << 18
T0 = 638_000_000_000_000_000
INITIAL, MAX_TTL, GROWTH = 30 * L.TICKS_PER_SECOND, 240 * L.TICKS_PER_SECOND, 2.0
SLOT_BYTES_READ = 32 + 8 + 8 + 8 + 8  # pass 1 per FULL slot: the slot, last_refreshed, ttl, generation, seen


def summary(ts):
    ts = np.array(ts)
    return (f"median {np.median(ts):.3f} ms (min {ts.min():.3f}, max {ts.max():.3f}, p25 {np.percentile(ts, 25):.3f}, "
            f"p75 {np.percentile(ts, 75):.3f})")


def main(reps=20, warm=3):
    cl = W.default_cluster()
    n_grains = int(CAP / 0.70)
    keys, _, owner, _ = W.grain_population(cl, n_grains)
    remote = np.nonzero(~np.isin(owner, [0, 1]))[0][:CAP]
    assert len(remote) == CAP
    n_act = 1 << 20
    eng = GrainDirectoryEngine(n_act=n_act, dir_capacity=1024, max_batch=NB, device=0)
    eng.set_silos(8, local=[1, 1, 0, 0, 0, 0, 0, 0])
    for s in range(8):
        eng.add_server(s, int(cl.hashes[s]))
    torch.cuda.set_stream(torch.cuda.Stream())
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    rng = np.random.default_rng(3)
    old, young = remote[: CAP // 2], remote[CAP // 2:]           # expired at the sweep / not yet
    hot = old[: CAP // 4]                                         # the expired entries that were accessed
    assert len(hot) <= NB
    d_keys = torch.from_numpy(np.ascontiguousarray(keys[remote]).view(np.uint8)).cuda()
    d_acts = torch.from_numpy((remote % n_act).astype(np.uint32).view(np.int32)).cuda()
    d_silos = torch.from_numpy(rng.integers(2, 8, CAP).astype(np.uint8)).cuda()
    d_etags = torch.from_numpy(rng.integers(0, 1 << 20, CAP).astype(np.int32)).cuda()
    msgs = W.uniform_messages(cl, n_grains, len(hot), seed=5)
    msgs["n1"] = hot.astype(np.uint64)
    d_msgs = torch.from_numpy(msgs.view(np.uint8)).cuda()
    d_route = torch.empty(len(hot), dtype=torch.int32, device="cuda")
    d_act = torch.empty(len(hot), dtype=torch.int32, device="cuda")
    slots = 1 << int(2 * CAP - 1).bit_length()
    table = torch.zeros(slots * 40, dtype=torch.uint8, device="cuda")  # stands for the table + stamps a host maintainer reads
    pinned = torch.empty(slots * 40, dtype=torch.uint8).pin_memory()
    now = T0 + INITIAL + 10

    def build_state():
        eng.cache_config_adaptive(CAP, INITIAL, MAX_TTL, GROWTH)
        for lo in range(0, CAP, NB):
            hi = min(lo + NB, CAP)
            # the first half at T0 (expired at `now`), the second at T0 + 20 ticks (not expired)
            for a, b, t in ((lo, min(hi, CAP // 2), T0), (max(lo, CAP // 2), hi, T0 + 20)):
                if a < b:
                    eng.cache_add_or_update_versioned_device(d_keys[a * 24:], d_acts[a:], d_silos[a:], d_etags[a:], b - a, t, stream=st)
        eng.address_messages_device(d_msgs, len(hot), d_route, d_act, stream=st, opts=L.OPT_NO_BUCKETS)
        stream.synchronize()

    sweeps, copies, counts = [], [], None
    for i in range(warm + reps):
        build_state()
        t0 = time.perf_counter()
        sw = eng.cache_maintain_device(0, now, stream=st)
        stream.synchronize()
        t_sweep = (time.perf_counter() - t0) * 1e3
        counts = eng._from_device(sw.d_counts, 5, np.uint64).tolist()
        stream.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(table, non_blocking=True)
        stream.synchronize()
        t_copy = (time.perf_counter() - t0) * 1e3
        if i >= warm:
            sweeps.append(t_sweep)
            copies.append(t_copy)
    assert counts[0] == 0 and counts[4] == 0 and sum(counts) == CAP, counts
    print(f"sweep of {CAP} entries in {slots} slots; {{self-owned, kept, expired, to refresh, owner null}} = {counts}", flush=True)
    print(f"orl_cache_maintain_device + stream synchronise: {summary(sweeps)}; {reps} sweeps after {warm} warm-up", flush=True)
    med = float(np.median(sweeps)) * 1e-3
    print(f"  pass 1 reads {SLOT_BYTES_READ} B per entry and 32 B per other slot: "
          f"{(CAP * SLOT_BYTES_READ + (slots - CAP) * 32) / med / 1e9:.1f} GB/s over the whole call "
          f"({slots * SLOT_BYTES_READ / med / 1e9:.1f} GB/s counting {SLOT_BYTES_READ} B for every slot)", flush=True)
    print(f"device-to-host copy of {slots * 40 / 1e6:.0f} MB (slots x (32 B + 8 B stamp)) into pinned memory + synchronise, "
          f"the floor of a host-side maintainer: {summary(copies)}", flush=True)
    print("count after the last sweep:", eng.cache_count(), flush=True)
    eng.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 20, int(a[1]) if len(a) > 1 else 3)
