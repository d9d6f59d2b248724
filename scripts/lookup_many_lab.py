"""What one LookUpMany costs the directory owner at the refresh loop's operating point: a versioned
partition of 1M entries in 2^21 slots and one requester's sweep list of 250,000 (grain, etag) pairs — half of them
unchanged, a quarter updated (the entry carries another tag), a quarter absent.

Timed: orl_dir_lookup_many_device plus one stream synchronise.  The comparison is the owner's host alternative,
orl_dir_lookup_many_host on the same requests in the same run: once with a current mirror, and once after a device
registration batch, when it first has to download the table and the tags (the case on a live directory, whose
registrations run on the device).  There is no earlier device path to compare with.
    python scripts/lookup_many_lab.py [reps] [warm]
Lab script, not a test."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from orleans_amd import _lib as L  # noqa: E402
from orleans_amd import workloads as W  # noqa: E402
from orleans_amd.engine import GrainDirectoryEngine, grain_keys_from_longs  # noqa: E402

ENTRIES, REQUESTS, NB = 1 << 20, 250_000, 1 << 18


def summary(ts):
    ts = np.array(ts)
    return f"median {np.median(ts):.3f} ms (min {ts.min():.3f}, max {ts.max():.3f})"


def main(reps=20, warm=3):
    cl = W.default_cluster()
    n_act = 1 << 20
    eng = GrainDirectoryEngine(n_act=n_act, dir_capacity=ENTRIES, max_batch=NB, device=0)
    eng.set_silos(8)
    for s in range(8):
        eng.add_server(s, int(cl.hashes[s]))
    eng.enable_directory_versions()
    torch.cuda.set_stream(torch.cuda.Stream())
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    rng = np.random.default_rng(13)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()  # noqa: E731
    keys = grain_keys_from_longs(cl.type_code, np.arange(ENTRIES + REQUESTS, dtype=np.int64))
    tags = rng.integers(0, 1 << 31, ENTRIES).astype(np.int32)
    acts = (np.arange(ENTRIES) % n_act).astype(np.uint32)
    silos = rng.integers(0, 8, ENTRIES).astype(np.uint8)
    d_status = torch.empty(NB, dtype=torch.uint8, device="cuda")
    for lo in range(0, ENTRIES - 1024, NB):  # the last 1024 entries are the registration batch of the stale-mirror case
        hi = min(lo + NB, ENTRIES - 1024)
        eng.register_single_activation_versioned_device(dev(keys[lo:hi]), dev(acts[lo:hi]), dev(silos[lo:hi]), dev(tags[lo:hi]),
                                                        hi - lo, d_status, stream=st)
    stream.synchronize()
    assert eng.directory_count() == ENTRIES - 1024
    # the request list: present keys with their tag, present keys with another tag, keys the partition never held
    n_same, n_upd = REQUESTS // 2, REQUESTS // 4
    pick = rng.permutation(ENTRIES - 1024)[: n_same + n_upd]
    rk = np.concatenate([keys[pick], keys[ENTRIES: ENTRIES + REQUESTS - n_same - n_upd]])
    re = np.concatenate([tags[pick[:n_same]], tags[pick[n_same:]] ^ 1, np.zeros(REQUESTS - n_same - n_upd, np.int32)])
    order = rng.permutation(REQUESTS)
    rk, re = np.ascontiguousarray(rk[order]), np.ascontiguousarray(re[order])
    d_rk, d_re = dev(rk), dev(re)
    d_kind = torch.empty(REQUESTS, dtype=torch.uint8, device="cuda")
    d_etag = torch.empty(REQUESTS, dtype=torch.int32, device="cuda")
    d_act = torch.empty(REQUESTS, dtype=torch.int32, device="cuda")
    d_silo = torch.empty(REQUESTS, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(5, dtype=torch.int64, device="cuda")
    ts = []
    for i in range(warm + reps):
        stream.synchronize()
        t0 = time.perf_counter()
        eng.lookup_many_device(d_rk, d_re, REQUESTS, d_kind, d_etag, d_act, d_silo, d_cnt, stream=st)
        stream.synchronize()
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    counts = d_cnt.cpu().numpy().tolist()
    assert counts == [n_same, REQUESTS - n_same - n_upd, n_upd, 0, 0], counts
    print(f"{REQUESTS} requests against {ENTRIES - 1024} entries in {2 * ENTRIES} slots; "
          f"{{unchanged, absent, updated, updated-empty, unsupported}} = {counts}", flush=True)
    print(f"orl_dir_lookup_many_device + stream synchronise: {summary(ts)}; {reps} runs after {warm} warm-up", flush=True)
    med = float(np.median(ts)) * 1e-3
    print(f"  {REQUESTS / med / 1e6:.1f} M requests/s", flush=True)
    # the host form on the same requests: a current mirror (the first call downloads it: not timed), then a stale one
    kind = eng.lookup_many(rk, re)[0]
    np.testing.assert_array_equal(kind, d_kind.cpu().numpy())
    hs = []
    for _ in range(3):
        t0 = time.perf_counter()
        eng.lookup_many(rk, re)
        hs.append((time.perf_counter() - t0) * 1e3)
    print(f"orl_dir_lookup_many_host, mirror current: {summary(hs)}; 3 runs", flush=True)
    lo = ENTRIES - 1024
    eng.register_single_activation_versioned_device(dev(keys[lo:ENTRIES]), dev(acts[lo:]), dev(silos[lo:]), dev(tags[lo:]), 1024,
                                                    d_status, stream=st)
    stream.synchronize()
    t0 = time.perf_counter()
    eng.lookup_many(rk, re)
    print(f"orl_dir_lookup_many_host after a device registration batch of 1024 (downloads {2 * ENTRIES * 36 / 1e6:.0f} MB of "
          f"slots and tags, recounts): {(time.perf_counter() - t0) * 1e3:.3f} ms; 1 run", flush=True)
    eng.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 20, int(a[1]) if len(a) > 1 else 3)
