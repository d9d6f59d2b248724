"""What one directory-cache add costs at the reference's operating point: a cache of 1M entries (GlobalConfiguration's
default CacheSize), full, taking batches of 64k adds of which half are new keys and half update present ones — every
LRU.Add runs AdjustSize at capacity (LRU.cs:104-116,188-205).  Times the wall clock of one
orl_cache_add_or_update_device including a stream synchronise (so a build that works on the host and a build that only
enqueues are charged the same way): median and spread of `reps` adds after `warm` warm-up adds.

Uses only calls older builds have too (the stats call is guarded), so the same script measures any build:
    python scripts/cache_evict_lab.py [reps] [warm] [mode]          (LAB_LIB=path/to/liborleans_route.so: another build)
mode: "device" (default) or "host" (ORL_CACHE_EVICT_HOST, where the build has it).  Run it under
`rocprofv3 --kernel-trace --stats` for the kernels' own times.  Lab script, not a test."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from orleans_amd import _lib as L  # noqa: E402

if os.environ.get("LAB_LIB"):  # A/B only: another build of the same library, which may lack the newer exports
    L.LIB_PATH = os.path.abspath(os.environ["LAB_LIB"])
    _probe = C.CDLL(L.LIB_PATH, mode=C.RTLD_GLOBAL)
    for _name in [s for s in L._SIGS if not hasattr(_probe, s)]:
        del L._SIGS[_name]

from orleans_amd import workloads as W  # noqa: E402
from orleans_amd.engine import GrainDirectoryEngine  # noqa: E402

CAP, NB = 1_000_000, 1 << 16


def main(reps=20, warm=3, mode="device"):
    cl = W.default_cluster()
    n_new = (reps + warm) * (NB // 2)
    n_grains = int((CAP + n_new) / 0.78) + 100_000
    keys, _, owner, _ = W.grain_population(cl, n_grains)
    remote = np.nonzero(~np.isin(owner, [0, 1]))[0]
    assert len(remote) >= CAP + n_new, (len(remote), CAP + n_new)
    n_act = 1 << 20
    eng = GrainDirectoryEngine(n_act=n_act, dir_capacity=1024, max_batch=NB, device=0)
    eng.set_silos(8, local=[1, 1, 0, 0, 0, 0, 0, 0])
    for s in range(8):
        eng.add_server(s, int(cl.hashes[s]))
    eng.cache_config(CAP)
    if hasattr(eng, "cache_evict_mode") and "orl_cache_evict_mode" in L._SIGS:
        eng.cache_evict_mode(L.CACHE_EVICT_HOST if mode == "host" else L.CACHE_EVICT_DEVICE)
    elif mode != "host":
        print("this build has no eviction mode: it runs its only path", flush=True)
    torch.cuda.set_stream(torch.cuda.Stream())
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(3)

    def add(pick):
        d_k = torch.from_numpy(np.ascontiguousarray(keys[pick]).view(np.uint8)).cuda()
        d_a = torch.from_numpy((pick % n_act).astype(np.uint32).view(np.int32)).cuda()
        d_s = torch.from_numpy(rng.integers(2, 8, len(pick)).astype(np.uint8)).cuda()
        stream.synchronize()
        t0 = time.perf_counter()
        eng.cache_add_or_update_device(d_k, d_a, d_s, len(pick), stream=stream.cuda_stream)
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3

    fill = [add(remote[lo: lo + NB]) for lo in range(0, CAP, NB)]
    assert eng.cache_count() == CAP
    print(f"fill: {len(fill)} adds of {NB}, median {np.median(fill):.3f} ms each", flush=True)
    ts, nxt = [], CAP
    recent = remote[CAP - 100_000: CAP]  # far from the LRU end for the whole run: these stay present
    for i in range(warm + reps):
        pick = np.concatenate([remote[nxt: nxt + NB // 2], rng.choice(recent, NB // 2, replace=False)])
        nxt += NB // 2
        rng.shuffle(pick)
        t = add(pick)
        if i >= warm:
            ts.append(t)
    ts = np.array(ts)
    assert eng.cache_count() <= CAP
    line = (f"at-capacity add of {NB} (half new, half present) into {CAP} entries, mode {mode}: median {np.median(ts):.3f} ms "
            f"(min {ts.min():.3f}, max {ts.max():.3f}, p25 {np.percentile(ts, 25):.3f}, p75 {np.percentile(ts, 75):.3f}; "
            f"{reps} adds after {warm} warm-up)")
    print(line, flush=True)
    if hasattr(eng, "cache_stats") and "orl_cache_stats" in L._SIGS:
        print("stats:", eng.cache_stats(), flush=True)
    print("count:", eng.cache_count(), flush=True)
    eng.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 20, int(a[1]) if len(a) > 1 else 3, a[2] if len(a) > 2 else "device")
