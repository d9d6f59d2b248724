"""GPU tests of the adaptive directory cache (orleans_amd/csrc/cache_adaptive.hip and the adaptive state the update,
eviction and rebuild kernels carry): every step of a scenario is applied to the device and to the reference restated in
tests/adaptive_cache_ref.py, then the cached count and a stamp-free peek of EVERY grain of the world (act, silo, etag,
timer, refresh time, access mark) must be equal, and — where the next step does not need entries left unaccessed, since
the batch is itself an access of every entry — one route batch that looks every remote grain up is compared word / handle
/ order / offsets with pyref.apply_directory_cache_lru.  All integer work: exact equality."""
import os
import re

import numpy as np
import pytest

import adaptive_cache_ref as A
import cache_evict_ref as R
from oracle import pyref as P
from orleans_amd import _lib as L
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
T0 = 638_000_000_000_000_000
INITIAL, MAX_TTL, GROWTH = 10_000_001, 60_000_000, 1.5  # an odd tick count: every second growth step truncates
ETAG_EDGES = np.array([0, -1, -(1 << 31), (1 << 31) - 1], np.int32)


def sweep_tile() -> int:
    """The sweep kernels' tile, from the kernel source's constant."""
    text = open(os.path.join(ROOT, "orleans_amd", "csrc", "cache_adaptive.h")).read()
    return int(re.search(r"constexpr uint32_t kSweepTile = (\d+);", text).group(1))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def world():
    return R.World(R.SCENARIO_GRAINS)


class Owners:
    """CalculateTargetSilo for sender `me` over a pyref ring (the model's injected owner function), per grain index."""

    def __init__(self, w, me=0):
        self.w, self.me = w, me
        self.ring = P.Ring()
        for s in range(8):
            self.ring.add_server(s, int(w.cl.hashes[s]))
        self.view = P.SiloView(running=[True] * 8, functional=w.functional, local=w.local)
        self.g_of = {k: g for g, k in enumerate(w.kt)}
        self.refresh()

    def refresh(self):
        self.own = {}
        for g, k in enumerate(self.w.kt):
            s, _ = P.calculate_target_silo(self.ring, P.Key(*k), P.jenkins_u64(*k), self.me, self.view, True)
            self.own[k] = None if s == P.NULL_SILO else s

    def owner_of(self, key):
        return self.own[key]

    def is_local(self, silo):
        return bool(self.w.local[silo])


class Pair:
    """One engine and one model fed the same operations."""

    def __init__(self, t, w, cap, max_batch=R.SCENARIO_BATCH, adaptive=True, seed=1):
        self.t, self.w, self.cap, self.adaptive = t, w, cap, adaptive
        self.eng = GrainDirectoryEngine(n_act=w.n_act, dir_capacity=w.n_grains, max_batch=max_batch, device=0)
        self.eng.set_silos(8, functional=w.functional, local=w.local)
        for s in range(8):
            self.eng.add_server(s, int(w.cl.hashes[s]))
        self.eng.register_single_activation(w.keys[w.mine], w.mine.astype(np.uint32), w.owner[w.mine])
        if adaptive:
            self.eng.cache_config_adaptive(cap, INITIAL, MAX_TTL, GROWTH)
        else:
            self.eng.cache_config(cap)
        self.st = t.cuda.current_stream().cuda_stream
        self.m = A.AdaptiveCache(cap, INITIAL, MAX_TTL, GROWTH)
        self.own = Owners(w)
        self.rng = np.random.default_rng(seed)
        self.n_msgs = max_batch                            # one route batch looks every remote grain up
        self.route_seed = 0
        self.all_keys = self.dev(w.keys)

    def close(self):
        self.eng.close()

    def dev(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()

    def out(self, n, dtype):
        return self.t.zeros(max(n, 1) * np.dtype(dtype).itemsize, dtype=self.t.uint8, device="cuda")

    def host(self, d, n, dtype):
        return d.cpu().numpy().view(dtype)[:n]

    # -- picks (from the model's state only)
    def present(self, remote_only=True):
        pool = self.w.remote if remote_only else np.arange(self.w.n_grains)
        return np.array([g for g in pool.tolist() if self.w.kt[g] in self.m.lru.d], np.int64)

    def absent(self, n):
        a = np.array([g for g in self.w.remote.tolist() if self.w.kt[g] not in self.m.lru.d], np.int64)
        return self.rng.choice(a, n, replace=False)

    # -- operations
    def add(self, pick, now, etags=None, acts=None, silos=None, all_valid=True):
        pick = np.asarray(pick, np.int64)
        n = len(pick)
        if acts is None:
            acts = (50_000 + self.rng.integers(0, 10_000 if all_valid else 20_000, n)).astype(np.uint32)
        if silos is None:
            silos = self.rng.integers(0, 8, n).astype(np.uint8)
        if etags is None:
            etags = self.rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
        if self.adaptive:
            self.eng.cache_add_or_update_versioned_device(self.dev(self.w.keys[pick]), self.dev(acts), self.dev(silos),
                                                          self.dev(etags), n, now, stream=self.st)
        else:
            self.eng.cache_add_or_update_device(self.dev(self.w.keys[pick]), self.dev(acts), self.dev(silos), n, stream=self.st)
        for g, a, s, e in zip(pick.tolist(), acts.tolist(), silos.tolist(), etags.tolist()):
            if self.w.valid_of(a, s):
                self.m.add_or_update(self.w.kt[g], (a, s), e, now)

    def remove(self, pick):
        pick = np.asarray(pick, np.int64)
        self.eng.cache_remove_device(self.dev(self.w.keys[pick]), len(pick), self.out(len(pick), np.uint8), stream=self.st)
        for g in pick.tolist():
            self.m.remove(self.w.kt[g])

    def mark_fresh(self, pick, now):
        pick = np.asarray(pick, np.int64)
        d_found = self.out(len(pick), np.uint8)
        self.eng.cache_mark_fresh_device(self.dev(self.w.keys[pick]), len(pick), now, d_found, stream=self.st)
        ref = [self.m.mark_as_fresh(self.w.kt[g], now) for g in pick.tolist()]
        np.testing.assert_array_equal(self.host(d_found, len(pick), np.uint8), np.array(ref, np.uint8), err_msg="found")

    def route(self, msgs):
        """A route batch on both sides (LookUp per message with a remote owner): words, handles, order, offsets."""
        self.t.cuda.synchronize()
        kt = list(zip(msgs["tcd"].tolist(), msgs["n0"].tolist(), msgs["n1"].tolist()))
        r0, a0 = self.w.o.route(msgs)
        r_ref, a_ref = P.apply_directory_cache_lru(r0.tolist(), a0.tolist(), msgs["sending_silo"].tolist(), kt, self.m,
                                                   self.w.functional)
        res = self.eng.address_messages(msgs)
        np.testing.assert_array_equal(res.route, np.array(r_ref, np.uint32), err_msg="route words")
        np.testing.assert_array_equal(res.act, np.array(a_ref, np.uint32), err_msg="handles")
        o_ref, f_ref = self.w.o.bucket(np.array(a_ref, np.uint32), self.w.n_act)
        np.testing.assert_array_equal(res.order, o_ref)
        np.testing.assert_array_equal(res.offsets, f_ref)

    def sweep(self, now, me=0):
        """The device's sweep against the model's: counts, per-owner lists as sets with their etags, consistent offsets;
        then the device's emitted order replayed into the model (BuildGrainAndETagList's Gets), which must reproduce the
        device's (grain, etag) sequence.  Returns the emitted keys in output order and the counts."""
        res = self.eng.cache_maintain(me, now, stream=self.st)
        etag_before = {k: v[0].etag for k, v in self.m.lru.d.items()}
        fetch, cnt = A.maintainer_run(self.m, list(self.m.lru.d), self.own.owner_of, self.own.is_local, now)
        c = res["counts"]
        assert [c["self_owned"], c["kept"], c["expired"], c["refresh"], c["owner_null"]] == cnt, (c, cnt)
        off = res["owner_offsets"].astype(np.int64)
        assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == cnt[3] == len(res["keys"]), off
        keys = [(int(a), int(b), int(d)) for a, b, d in zip(res["keys"]["tcd"], res["keys"]["n0"], res["keys"]["n1"])]
        etags = res["etags"].tolist()
        for o in range(8):
            got = set(zip(keys[off[o]:off[o + 1]], etags[off[o]:off[o + 1]]))
            assert len(got) == off[o + 1] - off[o], "a grain listed twice"
            assert got == {(k, etag_before[k]) for k in fetch.get(o, [])}, f"owner {o}'s refresh list"
        for o in range(8):  # ascending owners, output order inside each: the order of the device's Gets
            lst = A.build_grain_and_etag_list(self.m, keys[off[o]:off[o + 1]])
            assert lst == list(zip(keys[off[o]:off[o + 1]], etags[off[o]:off[o + 1]]))
        return keys, cnt, off

    # -- comparisons
    def check(self, route=False):
        self.t.cuda.synchronize()
        assert self.eng.cache_count() == len(self.m), (self.eng.cache_count(), len(self.m))
        n = self.w.n_grains
        d_act, d_silo = self.out(n, np.uint32), self.out(n, np.uint8)
        if self.adaptive:
            d_etag, d_ttl, d_lr, d_acc = self.out(n, np.int32), self.out(n, np.int64), self.out(n, np.int64), self.out(n, np.uint8)
            self.eng.cache_peek_device(self.all_keys, n, d_act, d_silo, d_etag, d_ttl, d_lr, d_acc, stream=self.st)
        else:
            self.eng.cache_peek_device(self.all_keys, n, d_act, d_silo, stream=self.st)
        self.t.cuda.synchronize()
        act, silo = self.host(d_act, n, np.uint32), self.host(d_silo, n, np.uint8)
        r_act, r_silo = np.full(n, L.NO_ACT, np.uint32), np.full(n, L.NULL_SILO, np.uint8)
        r_etag, r_ttl, r_lr, r_acc = np.full(n, L.CACHE_NO_ETAG, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.uint8)
        for k, v in self.m.lru.d.items():
            g, e = self.own.g_of[k], v[0]
            r_act[g], r_silo[g], r_etag[g], r_ttl[g], r_lr[g], r_acc[g] = (e.value[0], e.value[1], e.etag, e.expiration_timer,
                                                                           e.last_refreshed, e.num_accesses > 0)
        np.testing.assert_array_equal(act, r_act, err_msg="peek: act")
        np.testing.assert_array_equal(silo, r_silo, err_msg="peek: silo")
        if self.adaptive:
            np.testing.assert_array_equal(self.host(d_etag, n, np.int32), r_etag, err_msg="peek: etag")
            np.testing.assert_array_equal(self.host(d_ttl, n, np.int64), r_ttl, err_msg="peek: ttl")
            np.testing.assert_array_equal(self.host(d_lr, n, np.int64), r_lr, err_msg="peek: last_refreshed")
            np.testing.assert_array_equal(self.host(d_acc, n, np.uint8), r_acc, err_msg="peek: accessed")
        if route:
            self.route_seed += 1
            self.route(self.w.messages(self.route_seed, self.n_msgs))

    def accessed(self):
        return {k for k, v in self.m.lru.d.items() if v[0].num_accesses > 0}

    def stats_clean(self):
        st = self.eng.cache_stats()  # raises if a kernel raised the cache's error word
        assert st["host_fallbacks"] == 0 and st["entries"] == len(self.m), st
        return st


def subset_messages(w, grains, n_msgs, seed):
    m = w.W.uniform_messages(w.cl, w.n_grains, n_msgs, seed=seed)
    m["n1"] = np.resize(np.asarray(grains, np.uint64), n_msgs)
    return m


def test_scenario_capacity_257(torch, world):
    w = world
    p = Pair(torch, w, 257)
    rng = p.rng
    # versioned adds at t0: remote grains, self-owned grains (owner's partition local), invalid entries, edge etags
    pick = np.concatenate([rng.choice(w.remote, 180, replace=False), rng.choice(w.mine, 12, replace=False)])
    rng.shuffle(pick)
    n = len(pick)
    acts = (50_000 + rng.integers(0, 20_000, n)).astype(np.uint32)
    silos = rng.integers(0, 8, n).astype(np.uint8)
    acts[5], silos[9] = 0xFFFFFFFF, 200  # ORL_NO_ACT, an unknown silo
    etags = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    valid = np.array([w.valid_of(int(a), int(s)) for a, s in zip(acts, silos)])
    etags[np.nonzero(valid)[0][:4]] = ETAG_EDGES
    p.add(pick, T0, etags, acts, silos)
    self_owned = [k for k in p.m.lru.d if p.own.is_local(p.own.owner_of(k))]
    assert 0 < (~valid).sum() < 60 and len(self_owned) >= 5 and len(p.m) < n
    assert {int(e) for e in ETAG_EDGES} <= {v[0].etag for v in p.m.lru.d.values()}
    p.check()
    assert not p.accessed()
    # a route batch over a subset: exactly those keys are accessed
    sub = rng.choice(p.present(), 70, replace=False)
    p.route(subset_messages(w, sub, 512, seed=3))
    assert p.accessed() == {w.kt[g] for g in sub.tolist()}
    p.check()
    # one tick before the boundary nothing expires; the self-owned entries go
    _, cnt, _ = p.sweep(T0 + INITIAL - 1)
    assert cnt[0] == len(self_owned) and cnt[2] == 0 and cnt[3] == 0 and cnt[1] == len(p.m), cnt
    p.check()
    # at the boundary everything is expired: the unaccessed go, the accessed are listed and their mark is reset
    emitted, cnt, off = p.sweep(T0 + INITIAL)
    assert cnt[2] > 50 and cnt[3] == 70 and cnt[1] == 0 and (np.diff(off) > 0).sum() >= 4, cnt
    assert not p.accessed()
    p.check(route=True)
    # a refresh response with the three kinds interleaved (and two grains the cache does not hold), issued as runs
    t1 = T0 + INITIAL + 5
    resp = []
    for j, k in enumerate(emitted + [w.kt[g] for g in p.absent(2).tolist()]):
        kind = (0, 0, 2, 1, 2, 2, 0, 1, 1, 2, 0)[j % 11]
        if kind == 0:
            resp.append((k, int(rng.integers(-5, 1 << 20)), (int(50_000 + rng.integers(0, 10_000)), int(rng.integers(0, 8)))))
        else:
            resp.append((k, A.NO_ETAG if kind == 1 else p.m.entry(k).etag if p.m.entry(k) else 7, None))
    runs = A.response_runs(resp)
    assert {kind for kind, _ in runs} == {"add", "remove", "fresh"} and len(runs) > 20
    for kind, items in runs:
        g = np.array([p.own.g_of[t[0]] for t in items], np.int64)
        if kind == "add":
            p.add(g, t1, np.array([t[1] for t in items], np.int32), np.array([t[2][0] for t in items], np.uint32),
                  np.array([t[2][1] for t in items], np.uint8))
        elif kind == "remove":
            p.remove(g)
        else:
            p.mark_fresh(g, t1)
    p.check(route=True)
    # growth 1.5 from an odd tick count until the timer saturates at the maximum
    fresh = rng.choice(p.present(), 40, replace=False)
    ttls = []
    for j in range(7):
        p.mark_fresh(fresh, t1 + 10 + j)
        p.check(route=j == 6)
        ttls.append(p.m.entry(w.kt[int(fresh[0])]).expiration_timer)
    assert ttls[-2:] == [MAX_TTL, MAX_TTL] and any(t % 2 for t in ttls) and len(set(ttls)) >= 4, ttls
    # at-capacity adds after a sweep: the entries the sweep listed were restamped (Get) and outlive older-looking ones
    p.add(p.absent(p.cap - len(p.m)), t1 + 20)
    assert len(p.m) == p.cap
    p.check(route=True)                                  # every entry looked up: accessed, stamps in message order
    young = rng.choice(p.present(), 100, replace=False)
    p.mark_fresh(young, t1 + 30)                         # not expired at the sweep below; most recently used before it
    before = p.m.lru_order()
    t2 = t1 + 20 + INITIAL
    emitted, cnt, _ = p.sweep(t2)
    assert cnt[3] > 100 and cnt[1] >= 100 and cnt[2] == 0, cnt
    p.check()
    victims0 = p.m.lru.victims
    present0 = set(p.m.lru.d)
    p.add(p.absent(60), t2 + 1)
    evicted = present0 - set(p.m.lru.d)
    assert p.m.lru.victims - victims0 == 60 == len(evicted)
    assert not (evicted & set(emitted))                  # the listed entries were most recently used
    assert min(before.index(k) for k in emitted) < max(before.index(k) for k in evicted)  # ... though not before the sweep
    p.check(route=True)
    st = p.stats_clean()
    assert st["evict_batches"] >= 1
    p.close()


def test_state_survives_eviction_and_compaction(torch, world):
    w = world
    p = Pair(torch, w, 257, seed=2)
    now = T0
    p.add(p.absent(257), now)
    for j in range(40):
        now += 3
        kept = p.rng.choice(p.present(), 30, replace=False)
        p.mark_fresh(kept, now)                          # timers other than the initial one, on the most recently used
        pick = np.concatenate([p.absent(48), p.rng.choice(p.present(), 16, replace=False)])
        p.rng.shuffle(pick)
        p.add(pick, now + 1, all_valid=False)
        if j % 8 == 7:
            p.check()
        st = p.eng.cache_stats()
        if st["rebuilds"] >= 1 and st["evict_batches"] >= 1 and j >= 8:
            break
    assert st["rebuilds"] >= 1 and st["evict_batches"] >= 1, st
    assert p.m.lru.victims > 0
    assert sum(v[0].expiration_timer != INITIAL for v in p.m.lru.d.values()) >= 1
    p.check(route=True)
    p.stats_clean()
    p.close()


def test_table_of_several_sweep_tiles(torch):
    tile = sweep_tile()
    cap = 2 * tile + 1                                   # next_pow2(2 * cap) = 8 tiles of slots
    w = R.World(3 * cap, n_act=60_000)
    p = Pair(torch, w, cap, max_batch=1 << 14, seed=3)
    slots = 1 << int(2 * cap - 1).bit_length()
    assert slots >= 4 * tile and len(w.remote) <= p.n_msgs
    mine = p.rng.choice(w.mine, 40, replace=False)
    p.add(np.concatenate([p.rng.choice(w.remote, cap - 300, replace=False), mine]), T0)
    owners = {p.own.owner_of(k) for k in p.m.lru.d}
    assert owners == set(range(8))                       # all 8 owners present
    p.check()
    emitted, cnt, off = p.sweep(T0 + 1)                  # nothing expired: no entry is listed, the self-owned go
    assert cnt[3] == 0 and cnt[0] == 40 and cnt[1] == len(p.m) and not emitted, cnt
    p.check(route=True)                                  # every entry accessed
    p.add(mine, T0 + 2)                                  # owners 0 and 1 are present again: their lists stay empty
    emitted, cnt, off = p.sweep(T0 + 2 + INITIAL)
    assert cnt[3] == len(p.m) == len(emitted) and cnt[1] == 0 and cnt[2] == 0 and cnt[0] == 40, cnt
    sizes = np.diff(off)
    assert (sizes[:2] == 0).all() and (sizes[2:] > 0).all() and sizes.max() > tile // 2, sizes
    p.check(route=True)
    p.stats_clean()
    p.close()


@pytest.mark.parametrize("cap", [1, 2])
def test_tiny_capacities(torch, world, cap):
    """Capacity 1 (2 slots) and 2 (4 slots): one partial tile."""
    w = world
    p = Pair(torch, w, cap, seed=10 + cap)
    few = w.remote[:6]
    now = T0
    for j in range(6):
        p.add(p.rng.choice(few, 4, replace=False), now)
        p.check()
        if j % 2:
            p.route(subset_messages(w, few[:3], 64, seed=j))
        p.mark_fresh(few[:4], now + 1)
        p.check()
        n_before = len(p.m)
        _, cnt, _ = p.sweep(now + 1 + (INITIAL if j < 3 else INITIAL + INITIAL // 2))
        assert sum(cnt) == n_before == cap
        p.check(route=True)
        now += 2 * INITIAL
    assert p.m.lru.victims >= 6
    p.stats_clean()
    p.close()


@pytest.mark.parametrize("adaptive", [True, False])
def test_adjust_local_cache(torch, world, adaptive):
    w = world
    p = Pair(torch, w, 257, adaptive=adaptive, seed=5)
    p.add(p.rng.choice(w.remote, 230, replace=False), T0)
    p.check()
    # a ring server whose range falls to a silo this context hosts
    removed = None
    for s in range(2, 8):
        ring = P.Ring(list(p.own.ring.entries))
        ring.remove_server(s)
        trial = Owners.__new__(Owners)
        trial.w, trial.me, trial.ring, trial.view = w, 0, ring, p.own.view
        trial.refresh()
        now_mine = [k for k in p.m.lru.d if trial.own[k] is not None and w.local[trial.own[k]]]
        if now_mine:
            removed = s
            break
    assert removed is not None
    on_removed = [k for k, v in p.m.lru.d.items() if v[0].value[1] == removed]
    assert len(now_mine) >= 5 and len(on_removed) >= 5 and len(set(now_mine) | set(on_removed)) < len(p.m) - 50
    p.eng.remove_server(removed)
    p.own.ring.remove_server(removed)
    p.own.refresh()
    d_cnt = p.out(1, np.uint64)
    p.eng.cache_adjust_for_removed_silo_device(0, removed, d_cnt, stream=p.st)
    n_ref = A.adjust_local_cache(p.m, removed, p.own.owner_of, p.own.is_local)
    p.check()
    assert int(p.host(d_cnt, 1, np.uint64)[0]) == n_ref == len(set(now_mine) | set(on_removed))
    p.stats_clean()
    p.close()


def test_plain_add_on_an_adaptive_cache(torch, world):
    """orl_cache_add_or_update_device on an adaptive cache: etag 0 and the last `now` the context was given."""
    w = world
    p = Pair(torch, w, 257, seed=7)
    p.add(p.absent(50), T0 + 7)
    p.mark_fresh(p.present()[:10], T0 + 9)               # the last now_ticks a call gave
    pick = np.concatenate([p.absent(30), p.present()[:20]])
    acts = (50_000 + p.rng.integers(0, 10_000, len(pick))).astype(np.uint32)
    silos = p.rng.integers(0, 8, len(pick)).astype(np.uint8)
    p.eng.cache_add_or_update_device(p.dev(w.keys[pick]), p.dev(acts), p.dev(silos), len(pick), stream=p.st)
    for g, a, s in zip(pick.tolist(), acts.tolist(), silos.tolist()):
        p.m.add_or_update(w.kt[g], (a, s), 0, T0 + 9)
    p.check(route=True)
    p.stats_clean()
    p.close()


def test_refusals(torch, world):
    w = world
    p = Pair(torch, w, 16, adaptive=False)
    e, st = p.eng, p.st
    k = p.dev(w.keys[w.remote[:4]])
    plain_calls = [lambda: e.cache_add_or_update_versioned_device(k, p.out(4, np.uint32), p.out(4, np.uint8), p.out(4, np.int32), 4, T0, stream=st),
                   lambda: e.cache_maintain_device(0, T0, stream=st),
                   lambda: e.cache_mark_fresh_device(k, 4, T0, stream=st),
                   lambda: e.cache_peek_device(k, 4, d_etag=p.out(4, np.int32), stream=st),
                   lambda: e.cache_peek_device(k, 4, d_accessed=p.out(4, np.uint8), stream=st)]
    for call in plain_calls:
        with pytest.raises(OrleansRouteError) as err:
            call()
        assert err.value.code == L.E_STATE
    e.cache_peek_device(k, 4, p.out(4, np.uint32), p.out(4, np.uint8), stream=st)  # act / silo: any cache
    e.cache_evict_mode(L.CACHE_EVICT_HOST)                                           # a plain cache takes the host mode
    bad = [(8, -1, 10, 2.0), (8, 11, 10, 2.0), (8, 0, (1 << 61) + 1, 1.0), (8, 1, 10, -0.5), (8, 1, 10, float("nan")),
           (8, 1, 10, float("inf")), (8, 1, 1 << 61, 4.0), (0, 1, 10, 2.0)]
    for args in bad:
        with pytest.raises(OrleansRouteError) as err:
            e.cache_config_adaptive(*args)
        assert err.value.code == L.E_INVALID, args
    for args in [(8, 0, 0, 0.0), (8, 1 << 61, 1 << 61, 3.9), (8, 5, 5, 1.0)]:
        e.cache_config_adaptive(*args)                    # the extremes that are allowed
    with pytest.raises(OrleansRouteError) as err:         # configuring reset the mode to DEVICE; HOST is refused now
        e.cache_evict_mode(L.CACHE_EVICT_HOST)
    assert err.value.code == L.E_STATE
    e.cache_evict_mode(L.CACHE_EVICT_DEVICE)
    with pytest.raises(OrleansRouteError) as err:
        e.cache_maintain_device(8, T0, stream=st)
    assert err.value.code == L.E_INVALID
    p.close()
