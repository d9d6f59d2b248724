"""orl_cache_apply_refresh_device's algorithm restated in Python over plain dictionaries (what the k_ra_* kernels of
orleans_amd/csrc/cache_evict.hip compute), with coverage counters; the reference loop it must equal; and the responses
the GPU tests replay (test infrastructure, like cache_evict_ref.py).

The reference is sequential: ProcessCacheRefreshResponse (AdaptiveDirectoryCacheMaintainer.cs:167-207) walks the owner's
answer and, per entry, runs AddOrUpdate (LRU.Add: AdjustSize first), Remove or MarkAsFresh.  RefreshLRU.apply computes
the same result for the whole response as one preparation (candidates, the eviction queue with nxt / prevpos), one serial
pass over sequential arrays and one apply.  tests/test_refresh_apply_ref.py pins it against
adaptive_cache_ref.AdaptiveCache; the GPU tests use the counters as conditions on their input."""
from __future__ import annotations

import numpy as np

import adaptive_cache_ref as A

IGNORE, ADD, REMOVE, FRESH = 0, 1, 2, 3
LUM_UNCHANGED, LUM_ABSENT, LUM_UPDATED, LUM_UPDATED_EMPTY, LUM_UNSUPPORTED = 0, 1, 2, 3, 4  # include/orleans_route.h
OP_OF_KIND = {LUM_UPDATED: ADD, LUM_ABSENT: REMOVE, LUM_UNSUPPORTED: REMOVE, LUM_UPDATED_EMPTY: REMOVE, LUM_UNCHANGED: FRESH}
WINDOW = 2048  # kChunk of cache_evict.hip: queue / batch elements the serial pass stages at a time
INF = float("inf")
ALWAYS = "always"

COUNTERS = ("evictions", "self_evictions", "skips_add", "skips_remove", "skips_fresh", "evicted_add_elements",
            "evicted_fresh_elements", "fresh_gone_by_add", "remove_gone_by_add", "window_refills")


def operations(response, valid_of):
    """response: (key, kind, etag, act, silo) per entry, kind a LUM_* value or anything else.  Returns the operation of
    every entry as the call defines it: an unknown kind, an ADD that fails the validity predicate and every later
    occurrence of a key that an earlier entry operates on are IGNORE."""
    ops, seen = [], set()
    for key, kind, _etag, act, silo in response:
        op = OP_OF_KIND.get(kind, IGNORE)
        if op == ADD and not valid_of(act, silo):
            op = IGNORE
        if op != IGNORE and key in seen:
            op = IGNORE
        if op != IGNORE:
            seen.add(key)
        ops.append(op)
    return ops


def sequential_apply(cache: A.AdaptiveCache, response, valid_of, now):
    """The reference's loop (:167-207) over the entries that take a step.  Returns (present, counts): present[i] = the
    operation found its key at its turn (an ADD after its AdjustSize); counts = [ADDs, REMOVEs, FRESHes, ignored]."""
    ops = operations(response, valid_of)
    present, cnt = [], [0, 0, 0, 0]
    lru = cache.lru
    for (key, _kind, etag, act, silo), op in zip(response, ops):
        if op == IGNORE:
            present.append(False)
            cnt[3] += 1
            continue
        if op == ADD:                                 # :181-186
            while len(lru.d) >= lru.max:              # LRU.Add's AdjustSize (LRU.cs:188-205), so that `present` can be read
                lru.gen_free += 1
                victim = lru.by_gen.pop(lru.gen_free, None)
                if victim is not None:
                    del lru.d[victim]
                    lru.victims += 1
            present.append(key in lru.d)
            cache.add_or_update(key, (act, silo), etag, now)
        elif op == REMOVE:                            # :187-194
            present.append(cache.remove(key))
        else:                                         # :195-204
            present.append(cache.mark_as_fresh(key, now))
        cnt[op - 1] += 1
    return present, cnt


class RefreshLRU:
    """Cache of `cap` entries: key -> [value, etag, timer, last_refreshed, accessed, stamp].  Stamps are the device's:
    entry i of a call stamps G + i + 1 and G advances by n (only their order matters)."""

    def __init__(self, cap, initial=A.DEFAULT_INITIAL, max_timer=A.DEFAULT_MAX, growth=A.DEFAULT_GROWTH, window=WINDOW):
        self.cap, self.initial, self.max_timer, self.growth, self.window = cap, initial, max_timer, growth, window
        self.G = 0
        self.d = {}
        self.counters = dict.fromkeys(COUNTERS, 0)
        self.pointer_left_candidates = False  # the n_add + n_ops bound, checked on every call

    def order(self):
        """Keys from least to most recently used."""
        return [k for k, _ in sorted(self.d.items(), key=lambda kv: kv[1][5])]

    def apply(self, response, valid_of, now):
        """Returns (present, counts) like sequential_apply."""
        C = self.counters
        n = len(response)
        op = operations(response, valid_of)
        n_add, n_ops = op.count(ADD), n - op.count(IGNORE)
        # -- preparation
        old = sorted(self.d.items(), key=lambda kv: kv[1][5])       # FULL slots, ascending stamps
        K = min(len(old), n_add + n_ops) if n_add else 0
        cand = [k for k, _ in old[:K]]
        cand_pos = {k: q for q, k in enumerate(cand)}
        nxt = [INF] * (K + n)                                        # batch elements: keys are distinct, never touched again
        prevpos = [None] * n
        for i, (k, *_rest) in enumerate(response):
            if op[i] == IGNORE:
                continue
            if k in cand_pos:
                prevpos[i] = cand_pos[k]
                nxt[cand_pos[k]] = i
            elif k in self.d:
                prevpos[i] = ALWAYS
        # -- the serial pass, in the kernel's rounds: a queue window from the pointer and a batch window from the entry
        c, p, i = len(self.d), 0, 0
        live = [False] * n
        evicted = [False] * (K + n)
        present = [False] * n
        Q = K + n
        rounds, max_rounds = 0, (Q + n) // self.window + 4
        while i < n and n_add:
            assert rounds < max_rounds, "the round bound ran out"
            rounds += 1
            q0, b0 = p, i
            refill = False
            while i < n and i - b0 < self.window and not refill:
                if op[i] == IGNORE:
                    i += 1
                    continue
                if op[i] == ADD:
                    while c >= self.cap and not refill:              # AdjustSize
                        while p - q0 < self.window and p < Q and ((p >= K and not live[p - K]) or nxt[p] < i):
                            if p < K:
                                C[("skips_add", "skips_remove", "skips_fresh")[op[nxt[p]] - 1]] += 1
                            p += 1
                        assert p < Q and not (p >= K and p - K >= i), "nothing left to evict"
                        if p >= K and K < len(old):
                            self.pointer_left_candidates = True
                        if p - q0 >= self.window:
                            refill = True                            # refill the queue window, resume at this entry
                            C["window_refills"] += 1
                            break
                        evicted[p] = True
                        C["evictions"] += 1
                        C["self_evictions"] += nxt[p] == i
                        if p >= K:
                            C["evicted_add_elements" if op[p - K] == ADD else "evicted_fresh_elements"] += 1
                        p += 1
                        c -= 1
                    if refill:
                        break
                pp = prevpos[i]
                present[i] = pp is not None and (pp == ALWAYS or pp >= p)
                if pp is not None and not present[i]:
                    if op[i] == FRESH:
                        C["fresh_gone_by_add"] += 1
                    elif op[i] == REMOVE:
                        C["remove_gone_by_add"] += 1
                if op[i] == ADD:
                    live[i] = True
                    c += not present[i]
                elif op[i] == REMOVE:
                    c -= present[i]
                else:
                    live[i] = present[i]
                i += 1
        if not n_add:                                                # nothing can be evicted: the apply alone
            for j in range(n):
                present[j] = op[j] != IGNORE and prevpos[j] is not None
            c -= sum(present[j] for j in range(n) if op[j] == REMOVE)
        # -- apply
        for q in range(K):
            if evicted[q]:
                del self.d[cand[q]]
        for j, (k, _kind, etag, act, silo) in enumerate(response):
            stamp = self.G + j + 1
            if op[j] == ADD:
                if evicted[K + j]:
                    self.d.pop(k, None)                              # the old slot, if the update left it FULL
                else:
                    self.d[k] = [(act, silo), etag, self.initial, now, False, stamp]
            elif op[j] == REMOVE:
                self.d.pop(k, None)
            elif op[j] == FRESH and present[j]:
                if evicted[K + j]:
                    del self.d[k]
                else:
                    e = self.d[k]
                    e[2] = min(self.max_timer, A.multiply(e[2], self.growth))
                    e[3] = now
                    e[5] = stamp
        self.G += n
        assert len(self.d) == c, (len(self.d), c)
        return present, [op.count(ADD), op.count(REMOVE), op.count(FRESH), op.count(IGNORE)]


def same_state(ref: RefreshLRU, cache: A.AdaptiveCache):
    """Keys, LRU order and every field of every entry."""
    assert ref.order() == cache.lru_order()
    for k, e in ref.d.items():
        m = cache.entry(k)
        assert (e[0], e[1], e[2], e[3], e[4]) == (m.value, m.etag, m.expiration_timer, m.last_refreshed, m.num_accesses > 0), k


# ---- the responses of tests/test_gpu_cache_apply_refresh.py ----------------------------------------------------------

KIND_PATTERN = (0, 0, 2, 1, 2, 2, 0, 1, 1, 2, 0)  # test_gpu_cache_adaptive.test_scenario_capacity_257's: 0 add, 1 remove, 2 fresh


def interleaved_response(keys, etag_of, rng, extras=True):
    """keys in request order → (key, kind, etag, act, silo) with the three kinds interleaved by KIND_PATTERN; with
    `extras`, also UPDATED_EMPTY, UNSUPPORTED, an unknown kind, two invalid ADDs and one repeated key."""
    resp = []
    for j, k in enumerate(keys):
        kind = KIND_PATTERN[j % 11]
        if kind == 0:
            resp.append((k, LUM_UPDATED, int(rng.integers(-5, 1 << 20)), int(50_000 + rng.integers(0, 10_000)), int(rng.integers(0, 8))))
        elif kind == 1:
            resp.append((k, LUM_ABSENT, A.NO_ETAG, 0xFFFFFFFF, 0xFF))
        else:
            resp.append((k, LUM_UNCHANGED, etag_of(k), 0xFFFFFFFF, 0xFF))
    if extras and len(resp) >= 40:
        def as_kind(j, kind, act=0xFFFFFFFF, silo=0xFF):
            resp[j] = (resp[j][0], kind, resp[j][2], act, silo)
        as_kind(5, LUM_UPDATED_EMPTY)
        as_kind(9, LUM_UNSUPPORTED)
        as_kind(12, 9)                                   # an unknown kind
        as_kind(17, LUM_UPDATED, 0xFFFFFFFF, 3)          # ORL_NO_ACT
        as_kind(22, LUM_UPDATED, 51_000, 200)            # an unknown silo
        resp[30] = (resp[3][0],) + resp[30][1:]          # entry 3's key again: ignored
    return resp


def mixed_response(keys, etag_of, rng, p_add=0.25, p_remove=0.25):
    """The mix of scripts/lookup_many_lab.py by default: half unchanged, a quarter updated, a quarter absent, in random
    order."""
    resp = []
    for k in keys:
        u = rng.random()
        if u < p_add:
            resp.append((k, LUM_UPDATED, int(rng.integers(0, 1 << 30)), int(50_000 + rng.integers(0, 10_000)), int(rng.integers(0, 8))))
        elif u < p_add + p_remove:
            resp.append((k, LUM_ABSENT, A.NO_ETAG, 0xFFFFFFFF, 0xFF))
        else:
            resp.append((k, LUM_UNCHANGED, etag_of(k), 0xFFFFFFFF, 0xFF))
    return resp


def response_arrays(resp, key_dtype):
    """The five device input arrays of a response, as numpy."""
    n = len(resp)
    keys = np.zeros(n, key_dtype)
    for j, name in enumerate(key_dtype.names[:3]):
        keys[name] = np.array([t[0][j] for t in resp], np.uint64) if n else np.zeros(0, np.uint64)
    return (keys, np.array([t[1] for t in resp], np.uint8), np.array([t[2] for t in resp], np.int32),
            np.array([t[3] for t in resp], np.uint32), np.array([t[4] for t in resp], np.uint8))


# ---- the scenarios, written against a pair (model [+ device]) so that the CPU tests can check what they reach --------

T0 = 638_000_000_000_000_000
INITIAL, MAX_TTL, GROWTH = 10_000_001, 60_000_000, 1.5  # tests/test_gpu_cache_adaptive.py's: every second growth truncates


def load_from(ref: RefreshLRU, cache: A.AdaptiveCache):
    """ref takes the model's state (after adds, route batches and sweeps, which only the model and the device follow)."""
    ref.d = {k: [v[0].value, v[0].etag, v[0].expiration_timer, v[0].last_refreshed, v[0].num_accesses > 0, v[1]]
             for k, v in cache.lru.d.items()}
    ref.G = cache.lru.next_gen


class HostPair:
    """The model's half of tests/test_gpu_cache_adaptive.Pair, with the same operations: what a scenario does to the
    model when no device is there."""

    def __init__(self, w, cap, max_batch=4096, seed=1):
        from oracle import pyref as P
        self.P, self.w, self.cap = P, w, cap
        self.m = A.AdaptiveCache(cap, INITIAL, MAX_TTL, GROWTH)
        self.rng = np.random.default_rng(seed)
        self.n_msgs, self.route_seed = max_batch, 0
        self._own = None

    @property
    def own(self):
        if self._own is None:
            from test_gpu_cache_adaptive import Owners
            self._own = Owners(self.w)
        return self._own

    def close(self):
        pass

    def present(self, remote_only=True):
        pool = self.w.remote if remote_only else np.arange(self.w.n_grains)
        return np.array([g for g in pool.tolist() if self.w.kt[g] in self.m.lru.d], np.int64)

    def absent(self, n):
        a = np.array([g for g in self.w.remote.tolist() if self.w.kt[g] not in self.m.lru.d], np.int64)
        return self.rng.choice(a, n, replace=False)

    def add(self, pick, now, etags, acts, silos):
        for g, a, s, e in zip(np.asarray(pick).tolist(), acts.tolist(), silos.tolist(), etags.tolist()):
            if self.w.valid_of(a, s):
                self.m.add_or_update(self.w.kt[g], (a, s), e, now)

    def route(self, msgs):
        kt = list(zip(msgs["tcd"].tolist(), msgs["n0"].tolist(), msgs["n1"].tolist()))
        r0, a0 = self.w.o.route(msgs)
        self.P.apply_directory_cache_lru(r0.tolist(), a0.tolist(), msgs["sending_silo"].tolist(), kt, self.m, self.w.functional)

    def check(self, route=False):
        if route:
            self.route_seed += 1
            self.route(self.w.messages(self.route_seed, self.n_msgs))

    def sweep(self, now):
        fetch, cnt = A.maintainer_run(self.m, list(self.m.lru.d), self.own.owner_of, self.own.is_local, now)
        keys = [k for o in sorted(fetch) for k in fetch[o]]
        A.build_grain_and_etag_list(self.m, keys)
        return keys, cnt, None


class Applier:
    """Applies responses to a pair: the model by the reference loop, a RefreshLRU (reloaded from the model before each
    response) by the batch algorithm — the two must agree — and the device, when the pair has one, by the new call."""

    def __init__(self, p):
        self.p = p
        self.ref = RefreshLRU(p.cap, INITIAL, MAX_TTL, GROWTH)

    def apply(self, resp, now, **how):
        p = self.p
        load_from(self.ref, p.m)
        present, cnt = sequential_apply(p.m, resp, p.w.valid_of, now)
        present2, cnt2 = [], [0, 0, 0, 0]
        step = p.n_msgs if how.get("chunked") else max(len(resp), 1)  # the engine helper cuts at max_batch
        for at in range(0, max(len(resp), 1), step):
            pr, cn = self.ref.apply(resp[at:at + step], p.w.valid_of, now)
            present2 += pr
            cnt2 = [x + y for x, y in zip(cnt2, cn)]
        assert present2 == present and cnt2 == cnt
        same_state(self.ref, p.m)
        assert not self.ref.pointer_left_candidates
        if hasattr(p, "apply_refresh"):
            p.apply_refresh(resp, now, present, cnt, **how)
        return present, cnt


def explicit_add(p, pick, now):
    """A versioned add of valid entries; every random draw is made here, so a device pair and a host pair draw alike."""
    pick = np.asarray(pick, np.int64)
    n = len(pick)
    acts = (50_000 + p.rng.integers(0, 10_000, n)).astype(np.uint32)
    silos = p.rng.integers(0, 8, n).astype(np.uint8)
    etags = p.rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    p.add(pick, now, etags, acts, silos)


def etag_of(p):
    return lambda k: p.m.entry(k).etag if p.m.entry(k) is not None else 7


def keys_of(p, grains):
    return [p.w.kt[g] for g in np.asarray(grains).tolist()]


def lru_first(p, n):
    return p.m.lru_order()[:n]


def fill(p, now):
    explicit_add(p, p.absent(p.cap - len(p.m)), now)
    assert len(p.m) == p.cap


def scenario_257(p, ap):
    """Capacity 257, full: a sweep's emitted list plus two grains the cache does not hold, answered with the kinds
    interleaved and the extras; then an add at capacity, whose victims show the LRU order.  Returns the response."""
    w, rng = p.w, p.rng
    fill(p, T0)
    sub = rng.choice(p.present(), 120, replace=False)
    m = w.W.uniform_messages(w.cl, w.n_grains, 512, seed=3)
    m["n1"] = np.resize(np.asarray(sub, np.uint64), 512)
    p.route(m)                                           # 120 entries accessed
    emitted, cnt, _ = p.sweep(T0 + INITIAL)              # the unaccessed go, the accessed are listed
    assert cnt[3] == 120 and cnt[2] > 100, cnt
    p.check(route=True)                                  # every entry looked up: the LRU order no longer depends on the sweep's
    fill(p, T0 + INITIAL + 1)
    t1 = T0 + INITIAL + 5
    resp = interleaved_response(sorted(emitted) + keys_of(p, p.absent(2)), etag_of(p), rng)
    ap.apply(resp, t1)
    fill(p, t1 + 1)                                      # no lookup in between: the order the response left decides below
    victims = p.m.lru.victims
    explicit_add(p, p.absent(60), t1 + 2)                # at capacity: 60 victims, least recently used first
    assert p.m.lru.victims == victims + 60
    p.check(route=True)
    return resp


def scenario_tiny(p, ap):
    """Capacities 1 and 2: ADD then FRESH then ADD, and a REMOVE of the only entry."""
    w = p.w
    a, b, c = keys_of(p, w.remote[:3])
    upd = lambda k, e: (k, LUM_UPDATED, e, 50_001, 4)
    now = T0
    ap.apply([upd(a, 1), (a, LUM_UNCHANGED, 1, 0xFFFFFFFF, 0xFF)], now)          # the repeated key: ignored
    ap.apply([(a, LUM_UNCHANGED, 1, 0xFFFFFFFF, 0xFF), upd(b, 2)], now + 1)      # FRESH, then an ADD at capacity (cap 1)
    ap.apply([upd(a, 3), (b, LUM_UNCHANGED, 2, 0xFFFFFFFF, 0xFF), upd(c, 4)], now + 2)
    ap.apply([upd(c, 5)], now + 3)                                               # an update at capacity frees its own key
    for k in list(p.m.lru.d)[1:]:
        ap.apply([(k, LUM_ABSENT, -1, 0xFFFFFFFF, 0xFF)], now + 4)
    assert len(p.m) == 1
    only = next(iter(p.m.lru.d))
    ap.apply([(only, LUM_ABSENT, -1, 0xFFFFFFFF, 0xFF), (b, LUM_ABSENT, -1, 0xFFFFFFFF, 0xFF)], now + 5)
    assert len(p.m) == 0
    ap.apply([upd(a, 6), upd(b, 7), upd(c, 8), (a, LUM_UNCHANGED, 6, 0xFFFFFFFF, 0xFF)], now + 6)
    p.check(route=True)


SIZES = (0, 1, 63, 64, 65, 257)


def scenario_sizes(p, ap):
    """Responses of n = 0, 1, 63, 64, 65 and 257 entries on a full cache: present keys from the LRU end and absent keys."""
    now = T0
    fill(p, now)
    for n in SIZES:
        now += 3
        keys = lru_first(p, (2 * n) // 3) + keys_of(p, p.absent(n - (2 * n) // 3))
        order = p.rng.permutation(n)
        resp = mixed_response([keys[j] for j in order], etag_of(p), p.rng, 0.4, 0.2)
        ap.apply(resp, now)
    p.check(route=True)
    explicit_add(p, p.absent(40), now + 1)
    p.check(route=True)


def scenario_no_add(p, ap):
    """A response without an ADD on a full cache: nothing is evicted."""
    fill(p, T0)
    keys = lru_first(p, 150) + keys_of(p, p.absent(20))
    resp = mixed_response([keys[j] for j in p.rng.permutation(len(keys))], etag_of(p), p.rng, 0.0, 0.4)
    victims = p.m.lru.victims
    ap.apply(resp, T0 + 9, no_add=True)
    assert p.m.lru.victims == victims
    explicit_add(p, p.absent(5), T0 + 10)
    p.check(route=True)


BIG_CAP, BIG_BATCH, BIG_N = 3000, 4096, 4096
BIG_WORLD = 8000  # grains: a 6000-entry response of distinct keys


def big_response(p, n, p_add=0.5, p_remove=0.03, head=60, calm=2400):
    """n distinct keys.  First `head` removals of the most recently used keys, so that the count stays below the capacity
    — no eviction, the pointer rests — while the cached keys follow, least recently used first, for `calm` entries; from
    there on absent keys are dealt in at random places, and half of them close the response: the first eviction has
    more than a window of superseded candidates to pass, and the last ones find the candidates used up."""
    order = p.m.lru_order()
    lru = order[:min(len(order) - head, (n * 3) // 4 - head)]
    rest = [k for k in p.w.kt if k not in p.m.lru.d]
    rest = [rest[j] for j in p.rng.permutation(len(rest))[:n - head - len(lru)]]
    tail = len(rest) // 2
    where = (calm + p.rng.choice(n - tail - calm, len(rest) - tail, replace=False)).tolist() + list(range(n - tail, n))
    keys, a, b = [], iter(lru), iter(rest)
    at = set(where)
    for j in range(head, n):
        keys.append(next(b) if j in at else next(a))
    resp = [(k, LUM_ABSENT, A.NO_ETAG, 0xFFFFFFFF, 0xFF) for k in order[len(order) - head:]]
    resp += mixed_response(keys, etag_of(p), p.rng, p_add, p_remove)
    assert len({t[0] for t in resp}) == n == len(resp)
    return resp


def scenario_window(p, ap):
    """Capacity 3000, a 4096-entry response, about half ADDs over LRU-first keys: every cached entry is a candidate, the
    queue is longer than one window, the pointer crosses a refill and goes on into the batch elements."""
    explicit_add(p, p.w.remote[:BIG_CAP], T0)
    assert len(p.m) == BIG_CAP
    ap.apply(big_response(p, BIG_N), T0 + 5)
    explicit_add(p, p.absent(100), T0 + 6)
    p.check()


def scenario_compaction(p, ap):
    """Thirty applies at capacity: new keys keep arriving, so tombstones pile up until the load bound forces the compaction
    between the tombstoning and the inserts."""
    now = T0
    fill(p, now)
    for j in range(30):
        now += 2
        keys = keys_of(p, p.absent(64)) + keys_of(p, p.rng.choice(p.present(), 24, replace=False))
        resp = mixed_response([keys[i] for i in p.rng.permutation(len(keys))], etag_of(p), p.rng, 0.8, 0.1)
        ap.apply(resp, now, light=j % 10 != 9)
    p.check(route=True)


def scenario_chunks(p, ap):
    """A 6000-entry response through max_batch 4096."""
    explicit_add(p, p.w.remote[:BIG_CAP], T0)
    ap.apply(big_response(p, 6000, 0.3, 0.3), T0 + 5, chunked=True)
    explicit_add(p, p.absent(100), T0 + 6)
    p.check()
