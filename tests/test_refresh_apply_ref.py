"""CPU tests of orl_cache_apply_refresh_device's algorithm (tests/refresh_apply_ref.RefreshLRU, the restatement of the
k_ra_* kernels): pinned against the reference's sequential loop over adaptive_cache_ref.AdaptiveCache on random responses
and on hand-derived cases; the scenarios of the GPU tests checked for the cases they must reach; the symbol's presence
and the refusals that need no device."""
import os
import re

import numpy as np
import pytest

import adaptive_cache_ref as A
import cache_evict_ref as E
import refresh_apply_ref as R
from orleans_amd import _lib as L
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NOA, NOS = 0xFFFFFFFF, 0xFF


def valid_of(act, silo):
    return silo < 8 and (act < 60_000 or (act != 0xFFFFFFFF and silo >= 2))


def upd(k, etag, act=50_001, silo=4):
    return (k, R.LUM_UPDATED, etag, act, silo)


def fresh(k, etag=0):
    return (k, R.LUM_UNCHANGED, etag, NOA, NOS)


def gone(k, kind=R.LUM_ABSENT):
    return (k, kind, -1, NOA, NOS)


class Both:
    """An AdaptiveCache under the reference loop and a RefreshLRU under the batch algorithm, fed the same responses."""

    def __init__(self, cap, window=R.WINDOW):
        self.m = A.AdaptiveCache(cap, R.INITIAL, R.MAX_TTL, R.GROWTH)
        self.ref = R.RefreshLRU(cap, R.INITIAL, R.MAX_TTL, R.GROWTH, window=window)

    def apply(self, resp, now):
        R.load_from(self.ref, self.m)
        present, cnt = R.sequential_apply(self.m, resp, valid_of, now)
        present2, cnt2 = self.ref.apply(resp, valid_of, now)
        assert present2 == present and cnt2 == cnt
        R.same_state(self.ref, self.m)
        assert not self.ref.pointer_left_candidates
        return present, cnt

    def look_up(self, keys):
        for k in keys:
            self.m.look_up(k)


@pytest.mark.parametrize("seed", range(60))
def test_random_responses_equal_the_sequential_loop(seed):
    """Capacities 1 to 64, n = 0 and responses larger than the cache, LRU-first picks, every kind mix, repeated keys,
    invalid ADDs and unknown kinds, lookups in between; a small window so that refills happen."""
    rng = np.random.default_rng(seed)
    cap = int(rng.integers(1, 65))
    universe = [(7, 0, g) for g in range(3 * cap + 8)]
    b = Both(cap, window=int(rng.choice([4, 16, R.WINDOW])))
    now = R.T0
    for _ in range(30):
        now += int(rng.integers(1, R.INITIAL))
        n = int(rng.choice([0, 1, 2, cap // 2, cap, cap + 3, 2 * cap + 5]))
        p_add, p_rem = rng.choice([0.0, 0.2, 0.5, 1.0]), rng.choice([0.0, 0.25, 0.5])
        if rng.random() < 0.5:
            first = b.m.lru_order()[:n]
            rest = [k for k in universe if k not in b.m.lru.d]
            keys = (first + [rest[j] for j in rng.permutation(len(rest))])[:n]
            if rng.random() < 0.5:
                keys = [keys[j] for j in rng.permutation(len(keys))]
        else:
            keys = [universe[j] for j in rng.integers(0, len(universe), n)]  # repeats
        resp = R.mixed_response(keys, lambda k: 3, rng, p_add, p_rem)
        for j in range(len(resp)):
            u = rng.random()
            if u < 0.03:
                resp[j] = (resp[j][0], 9, 1, 50_000, 3)                      # an unknown kind
            elif u < 0.06:
                resp[j] = upd(resp[j][0], 5, NOA, 3)                         # an invalid ADD
            elif u < 0.09:
                resp[j] = gone(resp[j][0], int(rng.choice([R.LUM_UNSUPPORTED, R.LUM_UPDATED_EMPTY])))
        b.apply(resp, now)
        if rng.random() < 0.5:
            b.look_up([universe[j] for j in rng.integers(0, len(universe), cap)])


def test_hand_derived_cases():
    a, b_, c, d = [(7, 0, g) for g in range(4)]
    t = R.T0
    x = Both(3)
    # ADD (:181-186): inserted with the etag, the initial timer, LastRefreshed = now, unaccessed
    assert x.apply([upd(a, 11), upd(b_, 12, 50_002, 5), upd(c, 13)], t) == ([False] * 3, [3, 0, 0, 0])
    e = x.ref.d[a]
    assert e[:5] == [(50_001, 4), 11, R.INITIAL, t, False] and x.ref.order() == [a, b_, c]
    # FRESH (:195-204): timer growth (truncated), LastRefreshed, most recently used, access mark as it was
    x.look_up([b_])
    assert x.apply([fresh(a, 11), fresh(b_, 12), fresh(d, 1)], t + 5) == ([True, True, False], [0, 0, 3, 0])
    assert x.ref.d[a][:5] == [(50_001, 4), 11, int(R.INITIAL * 1.5), t + 5, False]
    assert x.ref.d[b_][2:5] == [int(R.INITIAL * 1.5), t + 5, True] and x.ref.order() == [c, a, b_]
    # REMOVE (:187-194) for ABSENT, UNSUPPORTED and UPDATED_EMPTY; a key not held is not present
    assert x.apply([gone(c), gone(d, R.LUM_UNSUPPORTED), gone(a, R.LUM_UPDATED_EMPTY)], t + 6) == ([True, False, True], [0, 3, 0, 0])
    assert x.ref.order() == [b_]
    # ignored: an unknown kind, an invalid ADD (ORL_NO_ACT; a handle >= n_act on a local silo), a repeated key
    r = [(b_, 9, 1, 50_000, 3), upd(c, 1, NOA, 3), upd(d, 1, 60_001, 1), fresh(b_, 12), gone(b_)]
    assert x.apply(r, t + 7) == ([False, False, False, True, False], [0, 0, 1, 4])
    assert x.ref.order() == [b_]
    # the self-eviction: at capacity, an update of the least recently used key frees that key first, then inserts it anew
    x.apply([upd(a, 21), upd(c, 23)], t + 8)
    assert x.ref.order() == [b_, a, c]
    ev0 = x.ref.counters["self_evictions"]
    assert x.apply([upd(b_, 99)], t + 9) == ([False], [1, 0, 0, 0])
    assert x.ref.counters["self_evictions"] == ev0 + 1 and x.ref.order() == [a, c, b_]
    assert x.ref.d[b_][:5] == [(50_001, 4), 99, R.INITIAL, t + 9, False]
    # an ADD at capacity evicts the key a later FRESH and a later REMOVE of the same response then miss
    assert x.apply([upd(d, 31), fresh(a, 21), upd((7, 0, 9), 1), gone(c)], t + 10) == ([False] * 4, [2, 1, 1, 0])
    assert x.ref.counters["fresh_gone_by_add"] == 1 and x.ref.counters["remove_gone_by_add"] == 1
    assert x.ref.order() == [b_, d, (7, 0, 9)]


@pytest.fixture(scope="module")
def world():
    return E.World(E.SCENARIO_GRAINS)


@pytest.fixture(scope="module")
def big_world():
    return E.World(R.BIG_WORLD)


def test_gpu_scenarios_reach_their_cases(world, big_world):
    """The scenarios of tests/test_gpu_cache_apply_refresh.py on the model alone: together they make every counter
    non-zero, and the pointer never leaves the candidates (asserted after every response by the Applier)."""
    total = dict.fromkeys(R.COUNTERS, 0)

    def run(scn, w, cap, max_batch=4096, seed=1):
        p = R.HostPair(w, cap, max_batch, seed)
        ap = R.Applier(p)
        out = scn(p, ap)
        for k, v in ap.ref.counters.items():
            total[k] += v
        return ap, out

    ap, resp = run(R.scenario_257, world, 257)
    ops = R.operations(resp, world.valid_of)
    kinds = {t[1] for t in resp}
    assert {R.LUM_UPDATED, R.LUM_ABSENT, R.LUM_UNCHANGED, R.LUM_UPDATED_EMPTY, R.LUM_UNSUPPORTED, 9} <= kinds
    assert ops.count(R.IGNORE) == 4
    assert len(resp) == 122 and ap.ref.counters["evictions"] > 0
    for cap in (1, 2):
        ap, _ = run(R.scenario_tiny, world, cap, seed=10 + cap)
        assert ap.ref.counters["self_evictions"] > 0
    run(R.scenario_sizes, world, 257, seed=3)
    ap, _ = run(R.scenario_no_add, world, 257, seed=4)
    assert ap.ref.counters["evictions"] == 0
    ap, _ = run(R.scenario_window, big_world, R.BIG_CAP, R.BIG_BATCH, seed=5)
    c = ap.ref.counters
    assert c["window_refills"] > 0 and c["evicted_add_elements"] > 0 and c["evicted_fresh_elements"] > 0, c
    run(R.scenario_compaction, world, 257, seed=6)
    run(R.scenario_chunks, big_world, R.BIG_CAP, R.BIG_BATCH, seed=7)
    assert all(v > 0 for v in total.values()), total


def test_symbol_is_declared_mirrored_and_exported():
    text = open(os.path.join(ROOT, "include", "orleans_route.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+orl_cache_apply_refresh_device\s*\(", code)
    assert "orl_cache_apply_refresh_device" in L.EXPORTED
    assert hasattr(L.load(), "orl_cache_apply_refresh_device")
    assert L.load().orl_abi_version() == L.ABI_VERSION == 1


def test_host_only_context_refuses():
    e = GrainDirectoryEngine(n_act=16, dir_capacity=16, max_batch=64, device=-1)
    z = np.zeros(4, np.uint64)
    with pytest.raises(OrleansRouteError) as err:
        e.cache_apply_refresh_device(z, z, z, z, z, 0, R.T0)
    assert err.value.code == L.E_STATE
    with pytest.raises(OrleansRouteError) as err:
        e.cache_apply_refresh(z, z, z, z, z, 1, R.T0)
    assert err.value.code == L.E_STATE
    e.close()
