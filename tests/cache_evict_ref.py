"""The directory cache's batch eviction algorithm restated in Python (what orleans_amd/csrc/cache_evict.hip computes), with
coverage counters, and the scenario the GPU tests replay.

The reference is sequential: LRU.Add runs AdjustSize before every add (src/Orleans/Utils/LRU.cs:104-116,188-205, used by
AdaptiveGrainDirectoryCache.cs:97-133).  BatchLRU.add_batch computes the same result for a whole batch as one
preparation (candidates, the eviction queue with its nxt / prevpos links), one serial pass over sequential arrays and
one apply.  tests/test_cache_evict_ref.py pins it against oracle/pyref.LRUCache; the GPU tests use its counters as
conditions on their input (that the scenario really holds self-evictions, skips, evicted batch entries ...)."""
from __future__ import annotations

import numpy as np

INF = float("inf")
SCENARIO_GRAINS = 5000  # 4046 of them remote: one route batch of max_batch = 4096 messages looks every one up
SCENARIO_BATCH = 4096
SCENARIO_SEED = 5       # chosen on the CPU (tests/test_cache_evict_ref.py::test_scenario_holds_its_cases)


class BatchLRU:
    """Cache of `cap` entries: key -> [value, stamp].  Stamps are the device's: entry / message i of a batch stamps
    G + i + 1 and G advances by the batch size (only their order matters)."""

    def __init__(self, cap: int):
        self.cap = cap
        self.G = 0
        self.d = {}
        self.counters = dict(evictions=0, self_evictions=0, skips=0, batch_entry_evictions=0, below_cap_evicting_batches=0)
        self.pointer_left_candidates = False  # the 2 * n_valid bound, checked on every batch

    # -- lookups and removals, as the route kernels and orl_cache_remove_device do them
    def lookup_batch(self, keys, n_total=None):
        """keys: (message index, key) pairs of the messages that look the cache up; n_total: the batch size."""
        keys = list(keys)
        for i, k in keys:
            if k in self.d:
                self.d[k][1] = max(self.d[k][1], self.G + i + 1)
        self.G += len(keys) if n_total is None else n_total

    def remove(self, key) -> bool:
        return self.d.pop(key, None) is not None

    def order(self):
        """Keys from least to most recently used."""
        return [k for k, _ in sorted(self.d.items(), key=lambda kv: kv[1][1])]

    def items(self):
        return {k: v[0] for k, v in self.d.items()}

    # -- the batch add
    def add_batch(self, entries):
        """entries: (key, value, valid) in batch order.  Exactly LRU.Add per valid entry, in order."""
        n = len(entries)
        valid = [bool(e[2]) for e in entries]
        n_valid = sum(valid)
        old = sorted(self.d.items(), key=lambda kv: kv[1][1])      # FULL slots, ascending stamps
        K = min(len(old), 2 * n_valid)
        cand = [k for k, _ in old[:K]]
        cand_pos = {k: q for q, k in enumerate(cand)}
        # nxt of every queue element: the first later valid batch entry with the same key
        nxt = [INF] * (K + n)
        prevpos = [None] * n
        last_occ = {}                                              # key -> queue position of its latest occurrence
        for i, (k, _, ok) in enumerate(entries):
            if not ok:
                continue
            if k in last_occ:
                prevpos[i] = last_occ[k]
                nxt[last_occ[k]] = i
            elif k in cand_pos:
                prevpos[i] = cand_pos[k]
                nxt[cand_pos[k]] = i
            elif k in self.d:
                prevpos[i] = INF                                   # present, and never a victim: always present
            last_occ[k] = K + i
        # the serial pass
        c, p = len(self.d), 0
        started_below = c < self.cap
        evicted = [False] * (K + n)
        ev0 = self.counters["evictions"]
        for i in range(n):
            if not valid[i]:
                continue
            while c >= self.cap:
                while p < K + n and ((p >= K and not valid[p - K]) or nxt[p] < i):
                    if not (p >= K and not valid[p - K]):
                        self.counters["skips"] += 1
                    p += 1
                assert p < K + i, "nothing left to evict"
                if p >= K and K < len(old):
                    self.pointer_left_candidates = True
                evicted[p] = True
                self.counters["evictions"] += 1
                self.counters["self_evictions"] += nxt[p] == i
                self.counters["batch_entry_evictions"] += p >= K
                p += 1
                c -= 1
            present = prevpos[i] is not None and prevpos[i] >= p
            if not present:
                c += 1
        if started_below and self.counters["evictions"] > ev0:
            self.counters["below_cap_evicting_batches"] += 1
        # apply: a key's fate is that of its last incarnation
        for q in range(K):
            if evicted[q]:
                del self.d[cand[q]]
        for i, (k, v, ok) in enumerate(entries):
            if not ok or nxt[K + i] != INF:
                continue
            if evicted[K + i]:
                self.d.pop(k, None)                                # the old slot of a key whose last occurrence went
            else:
                self.d[k] = [v, self.G + i + 1]
        self.G += n
        assert len(self.d) == c, (len(self.d), c)


# ---- the scenario of tests/test_gpu_cache_evict.py ------------------------------------------------------------------

class Scenario:
    """Feeds one operation sequence to pyref.LRUCache (the oracle), to BatchLRU (the coverage counters) and, when given,
    to a backend (the device).  All randomness comes from `seed`; the picks depend on the oracle's state only."""

    def __init__(self, cap, keys_t, remote, valid_of, seed, lru, backend=None):
        """keys_t[g]: grain g's key tuple; remote: the grains the cache may hold; valid_of(act, silo): the device's
        validity predicate; lru: a pyref.LRUCache (or a subclass) of the same capacity."""
        self.cap, self.kt, self.remote, self.valid_of, self.backend = cap, keys_t, np.asarray(remote), valid_of, backend
        self.lru = lru
        self.ref = BatchLRU(cap)
        self.rng = np.random.default_rng(seed)
        self.route_seed = 0

    # picks
    def present(self):
        return np.array([g for g in self.remote.tolist() if self.kt[g] in self.lru.d], np.int64)

    def absent(self, n):
        a = np.array([g for g in self.remote.tolist() if self.kt[g] not in self.lru.d], np.int64)
        return self.rng.choice(a, n, replace=False)

    def lru_first(self, n):
        p = self.present().tolist()
        return np.array(sorted(p, key=lambda g: self.lru.d[self.kt[g]][1])[:n], np.int64)

    # operations
    def add(self, pick, acts=None, silos=None, all_valid=False):
        """Handles in [50000, 70000): those >= n_act = 60000 are kept only off the local silos, so about one entry in
        eight is invalid; all_valid keeps them below n_act."""
        pick = np.asarray(pick, np.int64)
        n = len(pick)
        if acts is None:
            acts = (50_000 + self.rng.integers(0, 10_000 if all_valid else 20_000, n)).astype(np.uint32)
        if silos is None:
            silos = self.rng.integers(0, 8, n).astype(np.uint8)
        ent = [(self.kt[g], (int(a), int(s)), self.valid_of(int(a), int(s))) for g, a, s in zip(pick.tolist(), acts, silos)]
        if self.backend:
            self.backend.add(pick, np.asarray(acts, np.uint32), np.asarray(silos, np.uint8))
        for k, v, ok in ent:
            if ok:
                self.lru.add(k, v)
        self.ref.add_batch(ent)
        self.check()

    def remove(self, pick):
        if self.backend:
            self.backend.remove(np.asarray(pick, np.int64))
        for g in np.asarray(pick).tolist():
            self.lru.remove(self.kt[g])
            self.ref.remove(self.kt[g])
        self.check()

    def route(self, msgs_of):
        """One route batch that looks up every remote grain at least once (so every kept and every evicted key shows)."""
        self.route_seed += 1
        looked = msgs_of(self.route_seed, self.lru, self.backend)   # [(message index, key)] of the cache lookups, n
        self.ref.lookup_batch(looked[0], looked[1])
        self.check()

    def check(self):
        assert self.ref.items() == self.lru.items()
        assert self.ref.order() == [k for k, _ in sorted(self.lru.d.items(), key=lambda kv: kv[1][1])]
        assert not self.ref.pointer_left_candidates
        if self.backend:
            self.backend.check_count(len(self.lru.d))


def run_scenario(sc: Scenario, msgs_of, big=4096):
    """The steps of the capacity-257 test, in order.  Returns nothing: sc.lru / sc.ref / the backend hold the results."""
    cap, rng = sc.cap, sc.rng
    sc.add(sc.absent(200))                                              # fits
    if sc.backend:
        sc.backend.after_fitting_add()
    sc.route(msgs_of)
    sc.add(sc.absent(150))                                              # eviction starts mid-batch, K = entries
    sc.route(msgs_of)
    sc.add(sc.absent(64))                                               # at capacity: K = 128 < entries
    sc.route(msgs_of)
    p = sc.present()
    rnd = rng.choice(p, 40)
    # the least recently used keys (each update at capacity frees the very key it updates), random present keys, 10 repeated
    sc.add(np.concatenate([sc.lru_first(40), rnd, rnd[:10]]), all_valid=True)
    sc.route(msgs_of)
    pick = np.concatenate([sc.absent(40), rng.choice(sc.present(), 40)])
    rng.shuffle(pick)
    acts = (50_000 + rng.integers(0, 20_000, len(pick))).astype(np.uint32)
    silos = rng.integers(0, 8, len(pick)).astype(np.uint8)
    bad = rng.random(len(pick)) < 0.2                                   # ~20 % invalid entries interleaved
    acts[bad & (np.arange(len(pick)) % 2 == 0)] = 0xFFFFFFFF           # ORL_NO_ACT
    silos[bad & (np.arange(len(pick)) % 2 == 1)] = 200                  # an unknown silo
    sc.add(pick, acts, silos)
    sc.route(msgs_of)
    sc.remove(rng.choice(sc.present(), 50, replace=False))
    sc.route(msgs_of)
    sc.add(sc.absent(30))
    sc.route(msgs_of)
    # below capacity: the 40 least recently used keys updated first, then 60 new keys whose evictions skip those 40
    sc.add(np.concatenate([sc.lru_first(40), sc.absent(60)]), all_valid=True)
    sc.route(msgs_of)
    sc.add(sc.absent(cap + 70), all_valid=True)                         # one batch larger than the cache: 70 of its own go
    sc.route(msgs_of)
    third = rng.choice(sc.remote, (2 * cap) // 3 + 1, replace=False)
    pick = np.concatenate([third, third, third])                        # ~2 * capacity entries, every key three times
    rng.shuffle(pick)
    sc.add(pick)
    sc.route(msgs_of)
    for j in range(20):                                                 # n = 1: the LRU-first present key / a new key
        sc.add(sc.lru_first(1) if j % 2 == 0 else sc.absent(1), all_valid=True)
    sc.route(msgs_of)
    sc.add(np.zeros(0, np.int64))                                       # n = 0
    sc.route(msgs_of)
    for j in range(30):
        sc.add(sc.absent(64))
        if j % 10 == 9:
            sc.route(msgs_of)


class World:
    """The cluster of the directory-cache tests (8 silos, two of them local, one not functional), its CPU oracle and a
    grain population; route batches that look every grain up at least once."""

    def __init__(self, n_grains, n_act=60_000, running=None):
        """running (optional): LocalGrainDirectory.Running per silo (tests/hop1_ref.py stops one local silo); all by default."""
        from oracle import cpu_ref
        from orleans_amd import workloads as W
        self.W = W
        self.cl = W.default_cluster()
        self.local = [1, 1, 0, 0, 0, 0, 0, 0]
        self.functional = [1, 1, 1, 1, 1, 1, 0, 1]
        self.running = [1] * 8 if running is None else list(running)
        self.n_grains, self.n_act = n_grains, n_act
        self.o = cpu_ref.Oracle(8, running=self.running, functional=self.functional, local=self.local)
        for s in range(8):
            self.o.add_server(s, int(self.cl.hashes[s]))
        self.keys, _, self.owner, _ = W.grain_population(self.cl, n_grains)
        self.mine = np.nonzero(np.isin(self.owner, [0, 1]))[0]
        self.o.register(self.keys[self.mine], self.mine.astype(np.uint32), self.owner[self.mine])
        self.remote = np.nonzero(~np.isin(self.owner, [0, 1]))[0]
        self.kt = [(int(a), int(b), int(c)) for a, b, c in zip(self.keys["tcd"], self.keys["n0"], self.keys["n1"])]

    def valid_of(self, act, silo):
        """What the device keeps (k_cache_probe)."""
        return silo < 8 and (act < self.n_act or (act != 0xFFFFFFFF and not self.local[silo]))

    def messages(self, seed, n_msgs):
        """n_msgs messages: every remote grain once, the rest uniform over all grains, in a random order."""
        assert len(self.remote) <= n_msgs
        m = self.W.uniform_messages(self.cl, self.n_grains, n_msgs, seed=seed)
        rng = np.random.default_rng(1000 + seed)
        t = m["n1"].astype(np.uint64)
        t[: len(self.remote)] = self.remote.astype(np.uint64)
        rng.shuffle(t)
        m["n1"] = t
        return m

    def msgs_of(self, n_msgs):
        from oracle import pyref as P

        def f(seed, lru, backend):
            msgs = self.messages(seed, n_msgs)
            kt = list(zip(msgs["tcd"].tolist(), msgs["n0"].tolist(), msgs["n1"].tolist()))
            r0, a0 = self.o.route(msgs)
            r_ref, a_ref = P.apply_directory_cache_lru(r0.tolist(), a0.tolist(), msgs["sending_silo"].tolist(), kt, lru,
                                                       self.functional)
            if backend:
                backend.route(msgs, np.array(r_ref, np.uint32), np.array(a_ref, np.uint32))
            looked = [(i, kt[i]) for i in np.nonzero(((r0 >> 16) & 0xFF) == P.ST_REMOTE_OWNER)[0].tolist()]
            return looked, len(msgs)

        return f
