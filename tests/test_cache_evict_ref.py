"""CPU tests of the directory cache's device eviction: the batch algorithm (tests/cache_evict_ref.py, what
orleans_amd/csrc/cache_evict.hip computes) equals the reference's sequential LRU (oracle/pyref.LRUCache: LRU.cs:104-116,
147-174,188-205) in contents and LRU order; the capacity-257 scenario of the GPU tests holds the cases it is meant to
hold; the two new exports exist and a host-only context refuses them."""
import ctypes as C

import numpy as np
import pytest

import cache_evict_ref as R
from oracle import pyref as P
from orleans_amd import _lib as L
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError

SCENARIO_SEED = R.SCENARIO_SEED


def lru_order(lru):
    return [k for k, _ in sorted(lru.d.items(), key=lambda kv: kv[1][1])]


@pytest.mark.parametrize("cap", [1, 2, 3, 5, 17, 64])
def test_batch_algorithm_equals_sequential_lru(cap):
    """Random scenarios: batches of 0 .. 3 x capacity entries with duplicates and invalid entries, lookups and removals in
    between.  After every step contents and LRU order equal pyref.LRUCache; the eviction pointer never leaves the
    2 * n_valid candidates while more old entries exist."""
    evictions = 0
    for scen in range(60):
        rng = np.random.default_rng(1000 * cap + scen)
        universe = max(4, int(cap * rng.choice([1.5, 3, 6])))
        lru, ref = P.LRUCache(cap), R.BatchLRU(cap)
        for step in range(25):
            op = rng.random()
            if op < 0.6:
                n = int(rng.integers(0, 3 * cap + 1))
                ks = rng.integers(0, universe, n)
                if n and rng.random() < 0.5:  # more duplicates
                    ks[rng.integers(0, n, n // 2)] = ks[rng.integers(0, n, n // 2)]
                ok = rng.random(n) >= rng.choice([0.0, 0.2])
                ent = [((0, 0, int(k)), (int(rng.integers(0, 99)), 0), bool(v)) for k, v in zip(ks, ok)]
                for k, v, valid in ent:
                    if valid:
                        lru.add(k, v)
                ref.add_batch(ent)
            elif op < 0.85:
                ks = rng.integers(0, universe, int(rng.integers(0, 2 * cap + 2)))
                for k in ks:
                    lru.try_get((0, 0, int(k)))
                ref.lookup_batch([(i, (0, 0, int(k))) for i, k in enumerate(ks)])
            else:
                for k in rng.integers(0, universe, int(rng.integers(0, cap + 1))):
                    assert lru.remove((0, 0, int(k))) == ref.remove((0, 0, int(k)))
            assert ref.items() == lru.items(), (cap, scen, step)
            assert ref.order() == lru_order(lru), (cap, scen, step)
            assert not ref.pointer_left_candidates, (cap, scen, step)
        evictions += ref.counters["evictions"]
    assert evictions > 100 * min(cap, 8)


def test_scenario_holds_its_cases():
    """The GPU scenario on the CPU alone: BatchLRU == pyref.LRUCache after every step (Scenario.check), and the input
    holds what it is meant to exercise (conditions on the input, not on the code under test)."""
    w = R.World(R.SCENARIO_GRAINS)
    sc = R.Scenario(257, w.kt, w.remote, w.valid_of, SCENARIO_SEED, P.LRUCache(257))
    R.run_scenario(sc, w.msgs_of(R.SCENARIO_BATCH))
    c = sc.ref.counters
    assert c["self_evictions"] >= 20, c
    assert c["skips"] >= 20, c
    assert c["batch_entry_evictions"] >= 50, c
    assert c["below_cap_evicting_batches"] >= 1, c


def test_new_exports_refuse_a_host_only_context():
    lib = L.load()
    assert hasattr(lib, "orl_cache_stats") and hasattr(lib, "orl_cache_evict_mode")
    assert C.sizeof(L.orl_cache_stats) == 48
    eng = GrainDirectoryEngine(n_act=16, dir_capacity=16, device=-1)
    with pytest.raises(OrleansRouteError) as e:
        eng.cache_stats()
    assert e.value.code == L.E_STATE
    with pytest.raises(OrleansRouteError) as e:
        eng.cache_evict_mode(L.CACHE_EVICT_HOST)
    assert e.value.code == L.E_STATE
    eng.close()
