"""GPU tests of orl_cache_apply_refresh_device (the k_ra_* kernels of orleans_amd/csrc/cache_evict.hip): a whole refresh
response applied in one device call.  The device and the model (adaptive_cache_ref.AdaptiveCache under the reference's
sequential loop, tests/refresh_apply_ref.sequential_apply) get the same steps; after every step the count, a stamp-free
peek of EVERY grain (act, silo, etag, timer, refresh time, access mark), d_present and d_counts must be equal, with zero
host fallbacks and a clean error word — the comparisons of tests/test_gpu_cache_adaptive.py, whose Pair this file extends.
The scenarios live in tests/refresh_apply_ref.py, where tests/test_refresh_apply_ref.py checks on the CPU which cases
they reach.  All integer work: exact equality."""
import numpy as np
import pytest

import adaptive_cache_ref as A
import cache_evict_ref as E
import refresh_apply_ref as R
import versioned_partition_ref as V
from oracle import pyref as P
from orleans_amd import _lib as L
from orleans_amd import workloads as W
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError, grain_keys_from_longs
from test_gpu_cache_adaptive import Pair

pytestmark = pytest.mark.gpu

T0, INITIAL, MAX_TTL, GROWTH = R.T0, R.INITIAL, R.MAX_TTL, R.GROWTH


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def world():
    return E.World(E.SCENARIO_GRAINS)


@pytest.fixture(scope="module")
def big_world():
    return E.World(R.BIG_WORLD)


class DevPair(Pair):
    """Pair plus the refresh apply.  runs = True composes a response on the host from maximal runs of one kind and the
    three existing calls (the documented alternative) instead."""

    def __init__(self, t, w, cap, max_batch=E.SCENARIO_BATCH, seed=1, runs=False):
        super().__init__(t, w, cap, max_batch=max_batch, seed=seed)
        self.runs = runs

    def apply_refresh(self, resp, now, present, cnt, no_add=False, light=False, chunked=False):
        """The model already took the response (present, cnt are its results)."""
        n = len(resp)
        keys, kind, etags, acts, silos = R.response_arrays(resp, L.KEY_DTYPE)
        st0 = self.eng.cache_stats() if no_add else None
        if self.runs:
            self.apply_as_runs(resp, keys, etags, acts, silos, now)
        else:
            pieces = max(1, -(-n // self.eng.max_batch)) if chunked else 1
            d_present = self.t.full((max(n, 1),), 0xEE, dtype=self.t.uint8, device="cuda")
            d_counts = self.t.full((4 * pieces,), -1, dtype=self.t.int64, device="cuda")
            d_in = [self.dev(a) for a in (keys, kind, etags, acts, silos)]
            call = self.eng.cache_apply_refresh if chunked else self.eng.cache_apply_refresh_device
            self.t.cuda.synchronize()                     # the buffers were filled on torch's stream, the call runs on the context's
            call(*d_in, n, now, d_present, d_counts, stream=self.st)
            self.t.cuda.synchronize()
            np.testing.assert_array_equal(d_present.cpu().numpy()[:n], np.array(present, np.uint8), err_msg="d_present")
            got = d_counts.cpu().numpy().reshape(pieces, 4)
            print(f"apply n={n} counts={got.sum(0).tolist()} model={cnt}")
            assert got.sum(0).tolist() == cnt, (got, cnt)
            if chunked:
                assert pieces > 1 and got.sum(1).tolist() == [min(self.eng.max_batch, n - j * self.eng.max_batch) for j in range(pieces)]
        if no_add:
            st1 = self.eng.cache_stats()
            assert st1["evictions"] == st0["evictions"] and st1["evict_batches"] - st0["evict_batches"] <= 1, (st0, st1)
        if not light:
            self.check()
            self.stats_clean()

    def apply_as_runs(self, resp, keys, etags, acts, silos, now):
        ops = R.operations(resp, self.w.valid_of)
        runs = []                                         # maximal runs of one operation over the entries that take a step
        for j, op in enumerate(ops):
            if op == R.IGNORE:
                continue
            if runs and runs[-1][0] == op:
                runs[-1][1].append(j)
            else:
                runs.append((op, [j]))
        hold = []                                         # the calls run on the context's stream: their buffers live until the sync
        for op, idx in runs:
            idx = np.array(idx, np.int64)
            bufs = [self.dev(keys[idx]), self.dev(acts[idx]), self.dev(silos[idx]), self.dev(etags[idx]), self.out(len(idx), np.uint8)]
            hold.append(bufs)
            if op == R.ADD:
                self.eng.cache_add_or_update_versioned_device(*bufs[:4], len(idx), now, stream=self.st)
            elif op == R.REMOVE:
                self.eng.cache_remove_device(bufs[0], len(idx), bufs[4], stream=self.st)
            else:
                self.eng.cache_mark_fresh_device(bufs[0], len(idx), now, stream=self.st)
        self.t.cuda.synchronize()


def run(p, scenario):
    ap = R.Applier(p)
    out = scenario(p, ap)
    st = p.stats_clean()
    return ap, out, st


def test_capacity_257_full_cache_new_call_and_runs(torch, world):
    """The sweep's list answered with the kinds interleaved plus the extras, once through the new call and once as runs of
    the three existing calls on a second engine: each engine equals its model after every step (route batches included),
    the two models end equal, and the add at capacity that follows shows the LRU order."""
    p = DevPair(torch, world, 257)
    ap, resp, st = run(p, R.scenario_257)
    assert ap.ref.counters["evictions"] > 0 and p.m.lru.victims >= 60 and st["evict_batches"] >= 2
    q = DevPair(torch, world, 257, runs=True)
    _, resp_q, _ = run(q, R.scenario_257)
    assert resp_q == resp
    assert p.m.lru_order() == q.m.lru_order()
    for k in p.m.lru.d:
        a, b = p.m.entry(k), q.m.entry(k)
        assert (a.value, a.etag, a.expiration_timer, a.last_refreshed, a.num_accesses) == (b.value, b.etag, b.expiration_timer, b.last_refreshed, b.num_accesses)
    p.close()
    q.close()


@pytest.mark.parametrize("cap", [1, 2])
def test_tiny_capacities(torch, world, cap):
    p = DevPair(torch, world, cap, seed=10 + cap)
    ap, _, _ = run(p, R.scenario_tiny)
    assert ap.ref.counters["self_evictions"] > 0
    p.close()


def test_response_sizes(torch, world):
    """n = 0, 1, 63, 64, 65 and 257."""
    p = DevPair(torch, world, 257, seed=3)
    run(p, R.scenario_sizes)
    p.close()


def test_no_add_on_a_full_cache(torch, world):
    p = DevPair(torch, world, 257, seed=4)
    ap, _, _ = run(p, R.scenario_no_add)
    assert ap.ref.counters["evictions"] == 0
    p.close()


def test_queue_longer_than_one_window(torch, big_world):
    """Capacity 3000, max_batch 4096, a 4096-entry response: the pointer crosses a window refill and enters the batch
    elements."""
    p = DevPair(torch, big_world, R.BIG_CAP, max_batch=R.BIG_BATCH, seed=5)
    ap, _, _ = run(p, R.scenario_window)
    c = ap.ref.counters
    assert c["window_refills"] > 0 and c["evicted_add_elements"] > 0 and c["evicted_fresh_elements"] > 0, c
    p.close()


def test_compaction_between_tombstoning_and_inserts(torch, world):
    p = DevPair(torch, world, 257, seed=6)
    _, _, st = run(p, R.scenario_compaction)
    assert st["rebuilds"] >= 1 and st["evict_batches"] >= 30, st
    p.close()


def test_engine_helper_chunks(torch, big_world):
    """A 6000-entry response through max_batch 4096."""
    p = DevPair(torch, big_world, R.BIG_CAP, max_batch=R.BIG_BATCH, seed=7)
    run(p, R.scenario_chunks)
    p.close()


def test_refresh_loop_end_to_end(torch):
    """Two contexts on one GPU, as tests/test_gpu_dir_versions.test_refresh_loop_end_to_end: A is silo 0 with an adaptive
    cache, B holds silo 1's versioned partition.  A's sweep list goes to B's lookup_many_device as the device pointers it
    is, and B's four output arrays go to A's orl_cache_apply_refresh_device as they are: no copy to the host in between."""
    import test_gpu_dir_versions as TV
    import dir_layout as D
    t = torch
    cluster = W.default_cluster(TV.N_SILOS)
    stream = t.cuda.Stream()                             # one stream of the caller's for both contexts' calls
    st_ = stream.cuda_stream
    assert st_ != 0
    keys_all = grain_keys_from_longs(cluster.type_code, np.arange(6000, dtype=np.int64))
    owner = cluster.owner_of(W.jenkins3_np(keys_all["tcd"], keys_all["n0"], keys_all["n1"]))
    keys = keys_all[owner == 1][:260]
    n = len(keys)
    assert n == 260
    kt = [(int(a), int(b), int(c)) for a, b, c in zip(keys["tcd"], keys["n0"], keys["n1"])]
    rng = np.random.default_rng(5)
    b = TV.Pair(t, cluster, 1024, local=[0, 1, 0, 0, 0, 0, 0, 0])
    acts = rng.integers(0, TV.N_ACT, n).astype(np.uint32)
    silos = rng.integers(0, TV.N_SILOS, n).astype(np.uint8)
    tags = rng.integers(0, 1 << 31, n).astype(np.int32)
    assert (b.register(keys, acts, silos, tags) == L.INS_INSERTED).all()
    a = GrainDirectoryEngine(n_act=TV.N_ACT, dir_capacity=64, max_batch=TV.MAX_BATCH, device=0)
    a_local = [1, 0, 0, 0, 0, 0, 0, 0]
    a.set_silos(TV.N_SILOS, local=a_local, seed=0)
    for s in range(TV.N_SILOS):
        a.add_server(s, int(cluster.hashes[s]))
    a.cache_config_adaptive(300, INITIAL, MAX_TTL, GROWTH)
    m = A.AdaptiveCache(300, INITIAL, MAX_TTL, GROWTH)
    filled = [b.dev(keys), b.dev(acts), b.dev(silos), b.dev(tags)]
    t.cuda.synchronize()
    a.cache_add_or_update_versioned_device(*filled, n, T0, stream=st_)
    t.cuda.synchronize()
    for k, ac, s, e in zip(kt, acts.tolist(), silos.tolist(), tags.tolist()):
        m.add_or_update(k, (ac, s), e, T0)
    msgs = D.messages(keys[rng.permutation(n)[:200]], 1)
    a.address_messages(msgs)
    for k in zip(msgs["tcd"].tolist(), msgs["n0"].tolist(), msgs["n1"].tolist()):
        assert m.look_up(k) is not None
    changed, removed = keys[:60], keys[60:100]
    b.unregister(np.concatenate([changed, removed]))
    b.register(changed, rng.integers(0, TV.N_ACT, 60).astype(np.uint32), rng.integers(0, TV.N_SILOS, 60).astype(np.uint8),
               rng.integers(0, 1 << 31, 60).astype(np.int32))
    b.set_functional([1, 1, 1, 1, 0, 1, 1, 1])
    # 1. the sweep; 2. the owner's lookup on the sweep's pointers; 3. the apply on the owner's pointers — one stream, no sync
    now, t1 = T0 + INITIAL, T0 + INITIAL + 7
    t.cuda.synchronize()
    sw = a.cache_maintain_device(0, now, stream=st_)
    n_req = 200                                           # every accessed entry is listed, and owner 1 holds them all
    d_kind, d_etag, d_act, d_silo = b.out(n_req, np.uint8), b.out(n_req, np.int32), b.out(n_req, np.uint32), b.out(n_req, np.uint8)
    d_present = t.full((n_req,), 0xEE, dtype=t.uint8, device="cuda")
    d_counts = t.full((4,), -1, dtype=t.int64, device="cuda")
    b.eng.lookup_many_device(int(sw.d_keys), int(sw.d_etags), n_req, d_kind, d_etag, d_act, d_silo, stream=st_)
    a.cache_apply_refresh_device(int(sw.d_keys), d_kind, d_etag, d_act, d_silo, n_req, t1, d_present, d_counts, stream=st_)
    t.cuda.synchronize()
    # the model: the same three steps, in the device's emitted order
    off = a._from_device(sw.d_owner_offsets, TV.N_SILOS + 1, np.uint32).astype(np.int64)
    assert int(off[1]) == 0 and int(off[2]) == n_req == int(off[-1])
    fetch, _ = A.maintainer_run(m, list(m.lru.d), lambda k: 1, lambda s: s == 0, now)
    req_k = a._from_device(sw.d_keys, n_req, L.KEY_DTYPE)
    req_e = a._from_device(sw.d_etags, n_req, np.int32)
    req_kt = [(int(x), int(y), int(z)) for x, y, z in zip(req_k["tcd"], req_k["n0"], req_k["n1"])]
    assert set(req_kt) == set(fetch[1])
    assert A.build_grain_and_etag_list(m, req_kt) == list(zip(req_kt, req_e.tolist()))
    answers = V.look_up_many(b.model.part, [(P.Key(*k), int(e)) for k, e in zip(req_kt, req_e)], b.model.view)
    kind = b.host(d_kind, n_req, np.uint8)
    assert list(zip(kind.tolist(), b.host(d_etag, n_req, np.int32).tolist(), b.host(d_act, n_req, np.uint32).tolist(),
                    b.host(d_silo, n_req, np.uint8).tolist())) == answers
    assert set(kind.tolist()) == {L.LUM_UNCHANGED, L.LUM_ABSENT, L.LUM_UPDATED, L.LUM_UPDATED_EMPTY}
    resp = [(k, kd, e, ac, s) for k, (kd, e, ac, s) in zip(req_kt, answers)]
    valid_of = lambda ac, s: s < TV.N_SILOS and (ac < TV.N_ACT or (ac != 0xFFFFFFFF and not a_local[s]))
    present, cnt = R.sequential_apply(m, resp, valid_of, t1)
    assert min(cnt[:3]) > 0 and cnt[3] == 0
    np.testing.assert_array_equal(d_present.cpu().numpy(), np.array(present, np.uint8), err_msg="d_present")
    assert d_counts.cpu().numpy().tolist() == cnt
    assert a.cache_count() == len(m) < 200
    d_pa, d_ps, d_pe, d_pt, d_pl, d_pc = (b.out(n, np.uint32), b.out(n, np.uint8), b.out(n, np.int32), b.out(n, np.int64),
                                          b.out(n, np.int64), b.out(n, np.uint8))
    a.cache_peek_device(b.dev(keys), n, d_pa, d_ps, d_pe, d_pt, d_pl, d_pc, stream=st_)
    t.cuda.synchronize()
    ref = np.zeros(n, [("a", np.uint32), ("s", np.uint8), ("e", np.int32), ("t", np.int64), ("l", np.int64), ("c", np.uint8)])
    ref["a"], ref["s"], ref["e"] = L.NO_ACT, L.NULL_SILO, L.CACHE_NO_ETAG
    for g, k in enumerate(kt):
        en = m.entry(k)
        if en is not None:
            ref[g] = (en.value[0], en.value[1], en.etag, en.expiration_timer, en.last_refreshed, en.num_accesses > 0)
    for d, col, dt in ((d_pa, "a", np.uint32), (d_ps, "s", np.uint8), (d_pe, "e", np.int32), (d_pt, "t", np.int64),
                       (d_pl, "l", np.int64), (d_pc, "c", np.uint8)):
        np.testing.assert_array_equal(b.host(d, n, dt), ref[col], err_msg=col)
    st = a.cache_stats()
    assert st["host_fallbacks"] == 0 and st["entries"] == len(m)
    a.close()
    b.close()


def test_refusals(torch, world):
    w = world
    p = Pair(torch, w, 16, adaptive=False)
    too_many = p.eng.max_batch + 1
    e, st = p.eng, p.st
    k = p.dev(w.keys[w.remote[:4]])
    u8, i32, u32 = p.out(too_many, np.uint8), p.out(too_many, np.int32), p.out(too_many, np.uint32)
    with pytest.raises(OrleansRouteError) as err:         # a plain cache
        e.cache_apply_refresh_device(k, u8, i32, u32, u8, 4, T0, stream=st)
    assert err.value.code == L.E_STATE
    e.cache_config_adaptive(16, INITIAL, MAX_TTL, GROWTH)
    big = p.out(too_many, L.KEY_DTYPE)
    with pytest.raises(OrleansRouteError) as err:         # n > max_batch
        e.cache_apply_refresh_device(big, u8, i32, u32, u8, too_many, T0, stream=st)
    assert err.value.code == L.E_CAPACITY
    args = [k, u8, i32, u32, u8]
    for j in range(5):                                    # each required pointer
        bad = list(args)
        bad[j] = None
        with pytest.raises(OrleansRouteError) as err:
            e.cache_apply_refresh_device(*bad, 4, T0, stream=st)
        assert err.value.code == L.E_INVALID, j
    d_counts = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e.cache_apply_refresh_device(None, None, None, None, None, 0, T0, None, d_counts, stream=st)  # n = 0: counts written
    torch.cuda.synchronize()
    assert d_counts.cpu().numpy().tolist() == [0, 0, 0, 0]
    e.cache_apply_refresh_device(*args, 4, T0, stream=st)  # the optional outputs left out
    assert e.cache_count() == 0 and e.cache_stats()["host_fallbacks"] == 0
    p.close()
