"""GPU tests of the directory cache's eviction on the device (orleans_amd/csrc/cache_evict.hip): an add that overflows
the capacity, a batch larger than the cache and a table full of tombstones are handled on the caller's stream, with the
results of the reference's sequential LRU (oracle/pyref.LRUCache: AdaptiveGrainDirectoryCache.cs:97-133, LRU.cs:104-116,
147-174,188-205) fed the same sequence.  After every step the cached count equals the oracle's and one route batch that
looks up every remote grain — so every kept and every evicted key is seen — is compared word / handle / order / offsets
with pyref.apply_directory_cache_lru.  All integer work: exact equality."""
import numpy as np
import pytest

import cache_evict_ref as R
from oracle import pyref as P
from orleans_amd import _lib as L
from orleans_amd.engine import GrainDirectoryEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def world():
    return R.World(R.SCENARIO_GRAINS)


class CountingLRU(P.LRUCache):
    """pyref.LRUCache that counts the entries AdjustSize frees."""

    def __init__(self, m):
        super().__init__(m)
        self.victims = 0

    def add(self, key, value):
        while len(self.d) >= self.max:  # AdjustSize (LRU.cs:188-205), as LRUCache.add runs it
            self.gen_free += 1
            victim = self.by_gen.pop(self.gen_free, None)
            if victim is not None:
                del self.d[victim]
                self.victims += 1
        super().add(key, value)  # Count < MaximumSize now: its own AdjustSize loop does not run


class Device:
    """The engine under test behind tests/cache_evict_ref.Scenario's backend interface."""

    def __init__(self, t, w, cap, max_batch, mode=L.CACHE_EVICT_DEVICE):
        self.t, self.w = t, w
        self.eng = GrainDirectoryEngine(n_act=w.n_act, dir_capacity=w.n_grains, max_batch=max_batch, device=0)
        self.eng.set_silos(8, functional=w.functional, local=w.local)
        for s in range(8):
            self.eng.add_server(s, int(w.cl.hashes[s]))
        self.eng.register_single_activation(w.keys[w.mine], w.mine.astype(np.uint32), w.owner[w.mine])
        self.eng.cache_config(cap)
        self.eng.cache_evict_mode(mode)
        self.st = t.cuda.current_stream().cuda_stream

    def dev(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()

    def add(self, pick, acts, silos):
        self.eng.cache_add_or_update_device(self.dev(self.w.keys[pick]), self.dev(acts), self.dev(silos), len(pick), stream=self.st)

    def remove(self, pick):
        d_rm = self.t.empty(max(len(pick), 1), dtype=self.t.uint8, device="cuda")
        self.eng.cache_remove_device(self.dev(self.w.keys[pick]), len(pick), d_rm, stream=self.st)

    def check_count(self, n):
        self.t.cuda.synchronize()
        assert self.eng.cache_count() == n, (self.eng.cache_count(), n)

    def after_fitting_add(self):
        assert self.eng.cache_stats()["evict_batches"] == 0

    def route(self, msgs, r_ref, a_ref):
        self.t.cuda.synchronize()
        res = self.eng.address_messages(msgs)
        np.testing.assert_array_equal(res.route, r_ref, err_msg="route words")
        np.testing.assert_array_equal(res.act, a_ref, err_msg="handles")
        o_ref, f_ref = self.w.o.bucket(a_ref, self.w.n_act)
        np.testing.assert_array_equal(res.order, o_ref)
        np.testing.assert_array_equal(res.offsets, f_ref)


def _scenario(torch, world, mode):
    cap = 257  # 1024 slots
    dev = Device(torch, world, cap, R.SCENARIO_BATCH, mode)
    lru = CountingLRU(cap)
    sc = R.Scenario(cap, world.kt, world.remote, world.valid_of, R.SCENARIO_SEED, lru, backend=dev)
    R.run_scenario(sc, world.msgs_of(R.SCENARIO_BATCH))
    # conditions on the input (the reference algorithm's own counters), not on the code under test
    c = sc.ref.counters
    assert c["self_evictions"] >= 20 and c["skips"] >= 20 and c["batch_entry_evictions"] >= 50, c
    assert c["below_cap_evicting_batches"] >= 1, c
    st = dev.eng.cache_stats()
    dev.eng.close()
    return st, lru


def test_scenario_capacity_257_on_the_device(torch, world):
    """Fitting adds, eviction that starts mid-batch (K = entries), adds at capacity (K = 2 n < entries: the radix select),
    updates of the least recently used and of random present keys with repeats, invalid entries interleaved, removals,
    a batch larger than the cache, every key three times, n = 1 and n = 0 adds, thirty adds at capacity (tombstones fill the
    table: compactions).  No add leaves the device."""
    st, lru = _scenario(torch, world, L.CACHE_EVICT_DEVICE)
    assert st["host_fallbacks"] == 0, st
    assert st["evictions"] == lru.victims, (st, lru.victims)
    assert st["rebuilds"] >= 2, st
    assert st["evict_batches"] > 30, st
    assert st["entries"] == len(lru.d)


def test_scenario_capacity_257_host_mode(torch, world):
    """The same scenario with ORL_CACHE_EVICT_HOST: the host LRU stays reachable and gives identical results."""
    st, lru = _scenario(torch, world, L.CACHE_EVICT_HOST)
    assert st["host_fallbacks"] > 0, st
    assert st["evict_batches"] == 0 and st["rebuilds"] == 0, st
    assert st["evictions"] == lru.victims, (st, lru.victims)


@pytest.mark.parametrize("cap", [1, 2])
def test_tiny_capacities(torch, world, cap):
    """Capacity 1 (2 slots) and 2 (4 slots): batches of 5 with repeats; every add evicts and compacts."""
    dev = Device(torch, world, cap, R.SCENARIO_BATCH)
    lru = CountingLRU(cap)
    sc = R.Scenario(cap, world.kt, world.remote, world.valid_of, 40 + cap, lru, backend=dev)
    msgs_of = world.msgs_of(R.SCENARIO_BATCH)
    few = world.remote[:6]
    for _ in range(10):
        sc.add(sc.rng.choice(few, 5))
        sc.route(msgs_of)
    st = dev.eng.cache_stats()
    dev.eng.close()
    assert st["host_fallbacks"] == 0 and st["evictions"] == lru.victims and lru.victims >= 10, (st, lru.victims)


def test_capacity_65536(torch):
    """A cache of 65,536 entries (131,072 slots), filled, then five at-capacity batches of 8192 (about 25 % present keys,
    about 5 % repeats), with route batches of ~200k messages that look every grain up: lookups restamp across many
    workgroups, so the select sees stamps above 2^17 and thresholds that span several digits."""
    t = torch
    cap, nb = 65_536, 8192
    w = R.World(160_000, n_act=200_000)
    n_msgs = 200_000
    dev = Device(t, w, cap, 1 << 18)
    lru = CountingLRU(cap)
    rng = np.random.default_rng(77)
    msgs_of = w.msgs_of(n_msgs)

    def add(pick):
        acts = (150_000 + rng.integers(0, 100_000, len(pick))).astype(np.uint32)  # some handles >= n_act: kept off local silos
        silos = rng.integers(0, 8, len(pick)).astype(np.uint8)
        dev.add(pick, acts, silos)
        for g, a, s in zip(pick.tolist(), acts.tolist(), silos.tolist()):
            if w.valid_of(a, s):
                lru.add(w.kt[g], (a, s))
        dev.check_count(len(lru.d))

    fill = rng.permutation(w.remote)[: 10 * nb]  # one entry in eight is invalid: ten batches fill the cache (the last evicts)
    for lo in range(0, len(fill), nb):
        add(fill[lo: lo + nb])
    assert len(lru.d) == cap
    msgs_of(1, lru, dev)
    for j in range(5):
        present = np.array([g for g in w.remote.tolist() if w.kt[g] in lru.d], np.int64)
        absent = np.array([g for g in w.remote.tolist() if w.kt[g] not in lru.d], np.int64)
        pick = np.concatenate([rng.choice(absent, nb - nb // 4, replace=False), rng.choice(present, nb // 4, replace=False)])
        rep = rng.integers(0, nb, nb // 20)
        pick[rep] = pick[rng.integers(0, nb, nb // 20)]
        rng.shuffle(pick)
        add(pick)
        if j in (1, 4):
            msgs_of(2 + j, lru, dev)
    st = dev.eng.cache_stats()
    dev.eng.close()
    assert st["host_fallbacks"] == 0 and st["evictions"] == lru.victims and st["evict_batches"] >= 5, (st, lru.victims)
