"""What applying a refresh response costs at the reference's operating point: an adaptive cache of 1M entries
(GlobalConfiguration's default CacheSize), full, and an owner's answer over cached grains with the mix and order of
scripts/lookup_many_lab.py — half unchanged, a quarter updated, a quarter absent, in random order
(AdaptiveDirectoryCacheMaintainer.cs:167-207).  An apply changes the table, so every repetition rebuilds the same state
first (configure, fill); only the apply plus one stream synchronise is timed.  Four measurements:
  1. orl_cache_apply_refresh_device at 8,192 entries;
  2. the host composition it replaces on the same 8,192-entry response: the device-to-host copy of the kinds, the split
     into maximal runs of one kind, and one of the three existing calls per run (pointer offsets into the same arrays);
     at 250,000 entries only the number of runs is printed;
  3. the new call over a 250,000-entry response in max_batch pieces (engine.cache_apply_refresh);
  4. the same response with every UPDATED turned into UNCHANGED: no ADD, the data-parallel path.
    python scripts/cache_refresh_apply_lab.py [reps] [warm] [max_batch] [nohost]
`nohost` leaves measurement 2 out (for a kernel trace of the new call alone).  Lab script, not a test."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from orleans_amd import _lib as L  # noqa: E402
from orleans_amd import workloads as W  # noqa: E402
from orleans_amd.engine import GrainDirectoryEngine  # noqa: E402

CAP = 1_000_000
SMALL, LARGE = 8192, 250_000
T0 = 638_000_000_000_000_000
INITIAL, MAX_TTL, GROWTH = 30 * L.TICKS_PER_SECOND, 240 * L.TICKS_PER_SECOND, 2.0


def summary(ts):
    ts = np.array(ts)
    return f"median {np.median(ts):.3f} ms (min {ts.min():.3f}, max {ts.max():.3f})"


def main(reps=20, warm=3, nb=1 << 16, host=True):
    cl = W.default_cluster()
    n_grains = int(CAP / 0.70)
    keys, _, owner, _ = W.grain_population(cl, n_grains)
    remote = np.nonzero(~np.isin(owner, [0, 1]))[0][:CAP]
    assert len(remote) == CAP
    n_act = 1 << 20
    eng = GrainDirectoryEngine(n_act=n_act, dir_capacity=1024, max_batch=nb, device=0)
    eng.set_silos(8, local=[1, 1, 0, 0, 0, 0, 0, 0])
    for s in range(8):
        eng.add_server(s, int(cl.hashes[s]))
    torch.cuda.set_stream(torch.cuda.Stream())
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    rng = np.random.default_rng(3)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()
    d_keys, d_acts = up(keys[remote]), up((remote % n_act).astype(np.uint32))
    d_silos, d_etags = up(rng.integers(2, 8, CAP).astype(np.uint8)), up(rng.integers(0, 1 << 20, CAP).astype(np.int32))

    def build_state():
        eng.cache_config_adaptive(CAP, INITIAL, MAX_TTL, GROWTH)
        for lo in range(0, CAP, nb):
            eng.cache_add_or_update_versioned_device(d_keys[lo * 24:], d_acts[lo * 4:], d_silos[lo:], d_etags[lo * 4:],
                                                     min(nb, CAP - lo), T0, stream=st)
        stream.synchronize()

    # the response: LARGE distinct cached grains in random order; its first SMALL entries are the small response
    pick = rng.permutation(CAP)[:LARGE]
    kind = rng.choice(np.array([L.LUM_UNCHANGED, L.LUM_UNCHANGED, L.LUM_UPDATED, L.LUM_ABSENT], np.uint8), LARGE)
    r_keys, r_kind = up(keys[remote[pick]]), up(kind)
    r_kind_noadd = up(np.where(kind == L.LUM_UPDATED, L.LUM_UNCHANGED, kind).astype(np.uint8))
    r_etags, r_acts = up(rng.integers(0, 1 << 20, LARGE).astype(np.int32)), up(rng.integers(0, n_act, LARGE).astype(np.uint32))
    r_silos = up(rng.integers(2, 8, LARGE).astype(np.uint8))
    d_removed = torch.zeros(LARGE, dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros(4 * (LARGE // nb + 1), dtype=torch.int64, device="cuda")
    now = T0 + INITIAL + 10
    kp, ep, ap, sp, rp = (x.data_ptr() for x in (r_keys, r_etags, r_acts, r_silos, d_removed))

    def new_call(n, d_kind):
        return eng.cache_apply_refresh(r_keys, d_kind, r_etags, r_acts, r_silos, n, now, None, d_counts, stream=st)

    def host_composition(n):
        k = r_kind[:n].cpu().numpy()                          # the copy of the kinds (synchronises the stream)
        cut = np.flatnonzero(np.diff(k)) + 1
        starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [n]])
        for a, b in zip(starts.tolist(), ends.tolist()):
            if k[a] == L.LUM_UPDATED:
                eng.cache_add_or_update_versioned_device(kp + a * 24, ap + a * 4, sp + a, ep + a * 4, b - a, now, stream=st)
            elif k[a] == L.LUM_UNCHANGED:
                eng.cache_mark_fresh_device(kp + a * 24, b - a, now, stream=st)
            else:
                eng.cache_remove_device(kp + a * 24, b - a, rp + a, stream=st)
        return len(starts)

    def measure(label, fn):
        ts, extra = [], None
        for i in range(warm + reps):
            build_state()
            t0 = time.perf_counter()
            extra = fn()
            stream.synchronize()
            t = (time.perf_counter() - t0) * 1e3
            if i >= warm:
                ts.append(t)
        stats = eng.cache_stats()                             # raises if a kernel raised the cache's error word
        print(f"{label}: {summary(ts)}; {reps} timed after {warm} warm-up; calls / runs = {extra}; "
              f"entries after = {stats['entries']}, evictions = {stats['evictions']}, rebuilds = {stats['rebuilds']}", flush=True)
        return float(np.median(ts)), stats["entries"]

    print(f"cache of {CAP} entries, full; max_batch {nb}; response mix over {LARGE}: "
          f"{dict(zip(*np.unique(kind, return_counts=True)))} (0 unchanged, 1 absent, 2 updated)", flush=True)
    t1, e1 = measure(f"1. orl_cache_apply_refresh_device, {SMALL} entries", lambda: new_call(SMALL, r_kind))
    if host:
        t2, e2 = measure(f"2. host composition (copy of the kinds, run split, one existing call per run), {SMALL} entries",
                         lambda: host_composition(SMALL))
        assert e1 == e2, (e1, e2)
        print(f"   new call / host composition at {SMALL} entries: {t1 / t2:.4f} ({t2 / t1:.1f}x)", flush=True)
    k = kind
    print(f"   runs at {LARGE} entries (not timed): {int((np.diff(k) != 0).sum()) + 1}", flush=True)
    measure(f"3. engine.cache_apply_refresh, {LARGE} entries in pieces of {nb}", lambda: new_call(LARGE, r_kind))
    measure(f"4. the same without an ADD (UPDATED read as UNCHANGED), {LARGE} entries", lambda: new_call(LARGE, r_kind_noadd))
    eng.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 20, int(a[1]) if len(a) > 1 else 3, int(a[2]) if len(a) > 2 else 1 << 16, "nohost" not in a[3:])
