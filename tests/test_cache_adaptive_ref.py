"""CPU tests of the adaptive directory cache: the restatement of the reference (tests/adaptive_cache_ref.py) on
hand-derived cases, and the built library's new exports on a host-only context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adaptive_cache_ref as A
from orleans_amd import _lib as L
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
S = A.TICKS_PER_SECOND
T0 = 638_000_000_000_000_000  # a DateTime.UtcNow in 2022, in ticks

NEW_EXPORTS = ("orl_cache_config_adaptive", "orl_cache_add_or_update_versioned_device", "orl_cache_maintain_device",
               "orl_cache_mark_fresh_device", "orl_cache_adjust_for_removed_silo_device", "orl_cache_peek_device")


def test_default_ttl_doubles_to_the_maximum():
    """30 s → 60 → 120 → 240 → 240 s with the reference's defaults (GlobalConfiguration.cs:413-417)."""
    c = A.AdaptiveCache(4)
    c.add_or_update("g", (1, 2), 7, T0)
    seen = [c.entry("g").expiration_timer]
    for i in range(4):
        assert c.mark_as_fresh("g", T0 + i)
        seen.append(c.entry("g").expiration_timer)
    assert seen == [30 * S, 60 * S, 120 * S, 240 * S, 240 * S]
    assert c.entry("g").last_refreshed == T0 + 3 and c.entry("g").etag == 7


def test_multiply_truncates_toward_zero():
    assert A.multiply(3, 1.5) == 4                   # 4.5 → 4
    assert A.multiply(7, 1.5) == 10                  # 10.5 → 10
    assert A.multiply(5, 0.0) == 0
    assert A.multiply((1 << 53) + 1, 1.0) == 1 << 53  # (double)ticks rounds to nearest even first
    c = A.AdaptiveCache(4, initial=3, max_timer=100, growth=1.5)
    c.add_or_update("g", (1, 2), 0, T0)
    ttl = []
    for _ in range(10):
        c.mark_as_fresh("g", T0)
        ttl.append(c.entry("g").expiration_timer)
    assert ttl == [4, 6, 9, 13, 19, 28, 42, 63, 94, 100]


def test_expiry_is_at_the_boundary():
    """IsExpired is UtcNow >= LastRefreshed + ExpirationTimer: expired exactly at the boundary, not one tick earlier."""
    owner_of, is_local = (lambda g: 3), (lambda s: False)
    c = A.AdaptiveCache(4, initial=10 * S)
    c.add_or_update("g", (1, 2), 5, T0)
    fetch, cnt = A.maintainer_run(c, ["g"], owner_of, is_local, T0 + 10 * S - 1)
    assert (fetch, cnt) == ({}, [0, 1, 0, 0, 0]) and len(c) == 1
    fetch, cnt = A.maintainer_run(c, ["g"], owner_of, is_local, T0 + 10 * S)
    assert (fetch, cnt) == ({}, [0, 0, 1, 0, 0]) and len(c) == 0      # unaccessed: thrown away


def test_sweep_cases_and_access_reset():
    owner = {"self": 0, "null": None, "fresh": 3, "idle": 3, "hot": 4, "hot2": 3}
    c = A.AdaptiveCache(16, initial=10 * S)
    for g in ("self", "null", "idle", "hot", "hot2"):
        c.add_or_update(g, (1, 5), 11, T0)
    c.add_or_update("fresh", (1, 5), 12, T0 + 5 * S)
    assert c.look_up("hot") == ((1, 5), 11) and c.look_up("hot2") is not None and c.look_up("absent") is None
    order = ["hot2", "self", "null", "fresh", "idle", "hot"]
    fetch, cnt = A.maintainer_run(c, order, owner.get, lambda s: s == 0, T0 + 10 * S)
    assert fetch == {3: ["hot2"], 4: ["hot"]} and cnt == [1, 1, 1, 2, 1]
    assert sorted(k for k, _, _ in c.key_values()) == ["fresh", "hot", "hot2", "null"]
    assert c.entry("hot").num_accesses == 0 and c.entry("hot2").num_accesses == 0
    # the next sweep finds them expired and unaccessed: BuildGrainAndETagList's Get is no access
    assert A.build_grain_and_etag_list(c, fetch[3]) == [("hot2", 11)]
    assert A.build_grain_and_etag_list(c, fetch[4] + ["gone"]) == [("hot", 11)]
    assert c.entry("hot").num_accesses == 0
    _, cnt = A.maintainer_run(c, ["hot", "hot2"], owner.get, lambda s: s == 0, T0 + 10 * S)
    assert cnt == [0, 0, 2, 0, 0]


def test_add_or_update_resets_timer_and_accesses():
    c = A.AdaptiveCache(4)
    c.add_or_update("g", (1, 2), 1, T0)
    c.look_up("g")
    c.mark_as_fresh("g", T0 + 1)
    e = c.entry("g")
    assert (e.num_accesses, e.expiration_timer, e.last_refreshed) == (1, 60 * S, T0 + 1)
    c.add_or_update("g", (9, 3), 2, T0 + 2)
    e = c.entry("g")
    assert (e.value, e.etag, e.num_accesses, e.expiration_timer, e.last_refreshed) == ((9, 3), 2, 0, 30 * S, T0 + 2)


def test_mark_as_fresh_of_a_missing_key():
    c = A.AdaptiveCache(4)
    assert c.mark_as_fresh("g", T0) is False and len(c) == 0


def test_mark_as_fresh_and_get_move_lru_order_but_are_no_access():
    c = A.AdaptiveCache(3)
    for g in "abc":
        c.add_or_update(g, (1, 2), 0, T0)
    assert c.lru_order() == ["a", "b", "c"]
    c.mark_as_fresh("a", T0)
    assert c.lru_order() == ["b", "c", "a"]
    assert A.build_grain_and_etag_list(c, ["b"]) == [("b", 0)]
    assert c.lru_order() == ["c", "a", "b"]
    assert [c.entry(g).num_accesses for g in "abc"] == [0, 0, 0]
    c.look_up("c")
    assert c.lru_order() == ["a", "b", "c"] and c.entry("c").num_accesses == 1
    c.add_or_update("d", (1, 2), 0, T0)  # at capacity: the least recently used goes
    assert c.lru_order() == ["b", "c", "d"]


def test_update_at_full_capacity_may_evict_the_key_it_updates():
    """LRU.Add runs AdjustSize before the add (LRU.cs:111-116): at Count == MaximumSize the smallest generation goes, even
    when it is the key being updated — the key then re-enters as a new entry and the count stays."""
    c = A.AdaptiveCache(2)
    c.add_or_update("a", (1, 2), 1, T0)
    c.add_or_update("b", (1, 2), 1, T0)
    c.look_up("a")
    c.add_or_update("b", (7, 3), 2, T0 + 1)  # b is least recently used: evicted, then added
    assert c.lru.victims == 1 and c.lru_order() == ["a", "b"] and c.entry("b").etag == 2
    c.add_or_update("b", (8, 3), 3, T0 + 2)  # now a is least recently used: the update of b evicts a
    assert c.lru.victims == 2 and c.lru_order() == ["b"] and c.entry("b").value == (8, 3)


def test_process_cache_refresh_response_and_its_runs():
    c = A.AdaptiveCache(8, initial=10)
    for g in "abcd":
        c.add_or_update(g, (1, 2), 1, T0)
    resp = [("a", 4, (5, 6)), ("b", A.NO_ETAG, None), ("c", 1, None), ("d", 1, None), ("e", A.NO_ETAG, None), ("f", 2, (7, 7))]
    assert [(k, len(v)) for k, v in A.response_runs(resp)] == [("add", 1), ("remove", 1), ("fresh", 2), ("remove", 1), ("add", 1)]
    assert A.process_cache_refresh_response(c, resp, T0 + 3) == [2, 2, 2]
    assert sorted(k for k, _, _ in c.key_values()) == ["a", "c", "d", "f"]
    assert (c.entry("a").value, c.entry("a").etag, c.entry("a").last_refreshed) == ((5, 6), 4, T0 + 3)
    assert c.entry("c").expiration_timer == 20 and c.entry("c").last_refreshed == T0 + 3


def test_adjust_local_cache():
    owner = {"mine": 0, "dead": 4, "both": 0, "stay": 4, "null": None}
    c = A.AdaptiveCache(8)
    for g, silo in (("mine", 5), ("dead", 6), ("both", 6), ("stay", 5), ("null", 5)):
        c.add_or_update(g, (1, silo), 1, T0)
    assert A.adjust_local_cache(c, 6, owner.get, lambda s: s == 0) == 3
    assert sorted(k for k, _, _ in c.key_values()) == ["null", "stay"]


# ---- the built library ----------------------------------------------------------------------------------------------

def test_new_exports_exist():
    lib = L.load()
    for name in NEW_EXPORTS:
        assert name in L.EXPORTED and hasattr(lib, name), name


def test_no_etag_constant_matches_the_header():
    text = open(os.path.join(ROOT, "include", "orleans_route.h")).read()
    m = re.search(r"#define\s+ORL_CACHE_NO_ETAG\s+\((-?\d+)\)", text)
    assert m and int(m.group(1)) == L.CACHE_NO_ETAG == A.NO_ETAG


def test_host_only_ctx_refuses_the_adaptive_calls():
    eng = GrainDirectoryEngine(n_act=16, dir_capacity=16, device=-1)
    eng.set_silos(2)
    sweep = L.orl_cache_sweep()
    calls = [lambda: eng.cache_config_adaptive(8),
             lambda: eng.cache_add_or_update_versioned_device(None, None, None, None, 0, T0),
             lambda: eng.cache_maintain_device(0, T0),
             lambda: eng.cache_maintain(0, T0),
             lambda: eng.cache_mark_fresh_device(None, 0, T0),
             lambda: eng.cache_adjust_for_removed_silo_device(0, 1),
             lambda: eng.cache_peek_device(None, 0)]
    for call in calls:
        with pytest.raises(OrleansRouteError) as e:
            call()
        assert e.value.code == L.E_STATE
    assert sweep.d_keys is None and C.sizeof(L.orl_cache_sweep) == 32
    assert C.sizeof(L.orl_cache_stats) == 48  # the stats struct did not grow
    eng.close()
