"""GPU tests of the node protocol's two cache-dependent device entry points called directly: orl_partition_cached_device
(hop 1 at the sender: k_part_lb / k_part_lb_sw with CACHE = true) and orl_route_received_device (the receiver: the route
kernels with CIN = true), against tests/hop1_ref.py — per-rank padded regions, act lanes, rewritten target silos, counts,
the status word, the partition's LRU stamps and access marks on the sender's cache, and every receiver verdict.  Sizes sit
on both sides of a wave's share (512), a partition tile (2048, five tiles + 1 for the look-back) and a route tile (4096).
All integer work: exact equality."""
import numpy as np
import pytest

import adaptive_cache_ref as A
import cache_evict_ref as CE
import hop1_ref as H
from oracle import pyref as P
from orleans_amd import _lib as L
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, H.CASE_N]
T0 = 638_000_000_000_000_000
INITIAL, MAX_TTL, GROWTH = 10_000_001, 60_000_000, 1.5
LANE_FILL, OUT_FILL = 0x5A5A5A5A, 0xEE


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def world():
    return H.stopping_world()


@pytest.fixture(autouse=True)
def one_stream(torch):
    """Every test runs on one stream of its own: torch's fills, copies and frees and the library's launches are ordered by
    it.  (The default stream's handle is NULL, which the ABI reads as "the context's own stream", a non-blocking one: a
    sentinel fill or a freed input could then race with the kernel.)"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        yield
    s.synchronize()


def ros_of(w, nranks):
    ros = w.cl.rank_of_silo(nranks) if nranks != 3 else np.array([s % 3 for s in range(8)], np.uint8)
    return ros, int(ros[0])  # my_rank: the rank of the local silo 0 (silo 1 is another rank's where the map says so)


def dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()


def engine_of(w, max_batch=1 << 14, register=True):
    eng = GrainDirectoryEngine(n_act=w.n_act, dir_capacity=w.n_grains, max_batch=max_batch, device=0)
    eng.set_silos(8, running=w.running, functional=w.functional, local=w.local)
    for s in range(8):
        eng.add_server(s, int(w.cl.hashes[s]))
    if register:
        eng.register_single_activation(w.keys[w.mine], w.mine.astype(np.uint32), w.owner[w.mine])
    return eng


def cache_fill(t, eng, case, st):
    eng.cache_add_or_update_device(dev(t, case.cache_keys), dev(t, case.cache_acts), dev(t, case.cache_silos),
                                   len(case.cache_keys), stream=st)


def random_batch(w, n, seed):
    """World.messages' kind of batch at any size: uniform targets (500 of them never registered), every silo sending, one
    message in 89 with a complete address."""
    m = w.W.uniform_messages(w.cl, w.n_grains + 500, n, seed=seed)
    m["flags"][::89] = L.HDR_ADDRESS_COMPLETE
    m["target_silo"][::89] = 3
    m["category"][::7] = 1
    return m


class Out:
    """The outputs of one partition call, prefilled with sentinels, and their comparison with a hop1_ref.Hop1."""

    def __init__(self, t, n, nranks, fmt):
        self.t, self.n, self.nranks, self.fmt, self.stride = t, n, nranks, fmt, n + 5
        self.d_out = t.full((nranks * self.stride, fmt), OUT_FILL, dtype=t.uint8, device="cuda")
        self.d_lane = t.full((nranks * self.stride,), LANE_FILL, dtype=t.int32, device="cuda")
        self.d_cnt = t.full((nranks,), -1, dtype=t.int64, device="cuda")
        self.d_st = t.full((1,), 0x7FFF, dtype=t.int32, device="cuda")

    def host(self):
        self.t.cuda.synchronize()
        return (self.d_out.cpu().numpy().reshape(-1).view(H.REC_DTYPE[self.fmt]), self.d_lane.cpu().numpy().view(np.uint32),
                self.d_cnt.cpu().numpy(), int(self.d_st.item()))

    def check(self, h, msg, lane_past_count=True):
        out, lane, cnt, st = self.host()
        np.testing.assert_array_equal(cnt, h.counts.astype(np.int64), err_msg=f"{msg}: counts")
        assert st == h.status, (msg, st, h.status)
        fill_rec = np.frombuffer(bytes([OUT_FILL]) * self.fmt, H.REC_DTYPE[self.fmt])[0]
        for r in range(self.nranks):
            lo, c = r * self.stride, int(h.counts[r])
            np.testing.assert_array_equal(out[lo:lo + c], h.regions[r], err_msg=f"{msg}: rank {r}'s records")
            np.testing.assert_array_equal(lane[lo:lo + c], h.lanes[r], err_msg=f"{msg}: rank {r}'s act lane")
            assert (out[lo + c:lo + self.stride] == fill_rec).all(), f"{msg}: records written past rank {r}'s count"
            if lane_past_count:
                assert (lane[lo + c:lo + self.stride] == LANE_FILL).all(), f"{msg}: lane written past rank {r}'s count"


def partition(t, eng, msgs, ros, nranks, my_rank, fmt, opts, st):
    o = Out(t, len(msgs), nranks, fmt)
    eng.partition_cached_device(dev(t, msgs), len(msgs), ros, nranks, my_rank, o.stride, o.d_out, fmt, o.d_lane, o.d_cnt,
                                o.d_st, stream=st, opts=opts)
    return o


@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", [8, 16, 32])
def test_partition_cached_vs_sender(torch, world, fmt, nranks):
    """Every size as consecutive launches on one context and one stream (the look-back's tickets and epochs run on):
    regions, lanes, counts, status, nothing past a count.  The constructed batch at five tiles + 1, random ones below."""
    t, w = torch, world
    st = t.cuda.current_stream().cuda_stream
    ros, me = ros_of(w, nranks)
    case = H.case_batch(w, ros, me, fmt=fmt)
    types = H.wire_types_of(w)
    eng = engine_of(w)
    eng.set_wire_types(types)
    eng.cache_config(4096)
    cache_fill(t, eng, case, st)
    lru = P.LRUCache(4096)
    for k, v in case.entries():
        lru.add(k, v)
    runs = []
    for n in SIZES:  # all launches first, compared afterwards: nothing but the stream orders them
        msgs, opts = (case.msgs, case.opts) if n == H.CASE_N else (random_batch(w, n, seed=n + nranks), 0)
        runs.append((n, msgs, opts, partition(t, eng, msgs, ros, nranks, me, fmt, opts, st)))
    addressed = 0
    for n, msgs, opts, o in runs:
        h = H.sender(w.o, lru, msgs, ros, nranks, me, fmt, opts, w.functional, types)
        o.check(h, f"fmt {fmt}, {nranks} ranks, n = {n}")
        addressed += int((h.lane != H.NO_ACT).sum())
    assert addressed > 3000  # a condition on the input: the random batches meet the cache too
    assert eng.cache_count() == len(lru.d) == len(case.cache_keys)
    assert eng.query(L.Q_PART_ERROR) == 0
    eng.close()


@pytest.mark.parametrize("fmt", [8, 16, 32])
def test_partition_cached_with_stateless_types(torch, world, fmt):
    """k_part_lb_sw<fmt, CACHE = true>: with stateless-worker types set and no such message the output is the plain form's;
    with a listed type present those messages stay in the self region, unaddressed and not looked up — although the cache
    holds their keys."""
    t, w = torch, world
    st = t.cuda.current_stream().cuda_stream
    ros, me = ros_of(w, 3)
    case = H.case_batch(w, ros, me, fmt=fmt)
    tcd2 = H.grain_tcd(w.cl) + 1  # a second grain class, the stateless-worker one
    types = H.wire_types_of(w) + [tcd2]
    eng = engine_of(w)
    eng.set_wire_types(types)
    eng.set_stateless_types([tcd2], [1])
    eng.cache_config(4096)
    cache_fill(t, eng, case, st)
    sw_grains = w.remote[:300]
    k2 = w.keys[sw_grains].copy()
    k2["tcd"] = tcd2
    a2, s2 = (50_000 + sw_grains).astype(np.uint32), np.full(len(sw_grains), 3, np.uint8)
    eng.cache_add_or_update_device(dev(t, k2), dev(t, a2), dev(t, s2), len(k2), stream=st)
    lru = P.LRUCache(4096)
    for k, v in case.entries() + [((tcd2, 0, int(g)), (50_000 + int(g), 3)) for g in sw_grains.tolist()]:
        lru.add(k, v)
    for n in (513, H.CASE_N):  # none of the listed type
        msgs, opts = (case.msgs, case.opts) if n == H.CASE_N else (random_batch(w, n, seed=n), 0)
        o = partition(t, eng, msgs, ros, 3, me, fmt, opts, st)
        o.check(H.sender(w.o, lru, msgs, ros, 3, me, fmt, opts, w.functional, types), f"SW types set, absent, n = {n}")
    msgs = random_batch(w, 2049, seed=9)
    listed = np.arange(2049) % 3 == 1
    msgs["tcd"][listed] = tcd2
    msgs["n1"][listed] = np.resize(sw_grains, int(listed.sum()))
    gen0 = lru.next_gen
    h = H.sender(w.o, lru, msgs, ros, 3, me, fmt, 0, w.functional, types, sw_types=[tcd2])
    still = listed & ((msgs["flags"] & L.HDR_ADDRESS_COMPLETE) == 0)
    assert (h.dest[still] == me).all() and (h.lane[still] == H.NO_ACT).all() and not set(np.nonzero(listed)[0]) & set(h.looked)
    h_plain = H.sender(w.o, dict(lru.items()), msgs, ros, 3, me, fmt, 0, w.functional, types)
    assert (h_plain.lane[still] != H.NO_ACT).sum() > 300  # as directory grains they would have been addressed
    assert lru.next_gen - gen0 == len(h.found)
    partition(t, eng, msgs, ros, 3, me, fmt, 0, st).check(h, "a listed type present")
    eng.close()


def test_partition_null_owner_stays_unlooked(torch):
    """S8 proper: the stopped sender alone on the ring has no owner (LocalGrainDirectory.cs:483-493); its messages stay in
    the self region and never reach the cache, the running silo's messages to the same cached grains are addressed."""
    t = torch
    st = t.cuda.current_stream().cuda_stream
    w, msgs, opts, ent = H.null_owner_case()
    eng = GrainDirectoryEngine(n_act=w.n_act, dir_capacity=1024, max_batch=1024, device=0)
    eng.set_silos(8, running=w.running, functional=w.functional, local=w.local)
    eng.add_server(0, int(w.cl.hashes[0]))
    eng.cache_config_adaptive(257, INITIAL, MAX_TTL, GROWTH)
    keys = np.zeros(len(ent), L.KEY_DTYPE)
    keys["tcd"], keys["n0"], keys["n1"] = [k[0] for k, _ in ent], [k[1] for k, _ in ent], [k[2] for k, _ in ent]
    eng.cache_add_or_update_versioned_device(dev(t, keys), dev(t, np.array([v[0] for _, v in ent], np.uint32)),
                                             dev(t, np.array([v[1] for _, v in ent], np.uint8)),
                                             dev(t, np.zeros(len(ent), np.int32)), len(ent), T0, stream=st)
    model = A.AdaptiveCache(257, INITIAL, MAX_TTL, GROWTH)
    for k, v in ent:
        model.add_or_update(k, v, 0, T0)
    for fmt in (16, 32):
        h = H.sender(w.o, model, msgs, w.ros, w.nranks, w.my_rank, fmt, opts, w.functional)
        partition(t, eng, msgs, w.ros, w.nranks, w.my_rank, fmt, opts, st).check(h, f"null owner, fmt {fmt}")
    ref_acc = np.array([model.entry(k).num_accesses > 0 for k, _ in ent], np.uint8)
    np.testing.assert_array_equal(ref_acc, np.arange(len(ent)) % 2)  # on the reference: the running silo's grains only
    _, acc = peek(t, eng, keys, st, adaptive=True)
    np.testing.assert_array_equal(acc, ref_acc, err_msg="access marks: a message without an owner looked the cache up")
    eng.close()


def peek(t, eng, keys, st, adaptive=False):
    n = len(keys)
    d_act = t.zeros(n, dtype=t.int32, device="cuda")
    d_acc = t.zeros(n, dtype=t.uint8, device="cuda")
    if adaptive:
        eng.cache_peek_device(dev(t, keys), n, d_act, d_accessed=d_acc, stream=st)
    else:
        eng.cache_peek_device(dev(t, keys), n, d_act, stream=st)
    t.cuda.synchronize()
    return d_act.cpu().numpy().view(np.uint32), d_acc.cpu().numpy()


def test_partition_stamps_decide_the_next_eviction(torch, world):
    """LRU mode, capacity 257: a fitting add, ONE partition over the constructed batch, an add that overflows.  The
    survivors are pyref.LRUCache's with sender's lookups — and not what they would be had the partition not stamped."""
    t, w = torch, world
    st = t.cuda.current_stream().cuda_stream
    ros, me = ros_of(w, 3)
    case = H.case_batch(w, ros, me, fmt=16, n_background=150)
    assert len(case.cache_keys) < 257
    eng = engine_of(w)
    eng.cache_config(257)
    cache_fill(t, eng, case, st)
    t.cuda.synchronize()
    assert eng.cache_stats()["evict_batches"] == 0 and eng.cache_count() == len(case.cache_keys)
    lru, unstamped = P.LRUCache(257), P.LRUCache(257)
    for k, v in case.entries():
        lru.add(k, v)
        unstamped.add(k, v)
    o = partition(t, eng, case.msgs, ros, 3, me, 16, case.opts, st)
    h = H.sender(w.o, lru, case.msgs, ros, 3, me, 16, case.opts, w.functional)
    o.check(h, "capacity 257")
    have = set(H.key_tuples(case.cache_keys))
    new = np.array([g for g in w.remote.tolist() if w.kt[g] not in have][:150], np.int64)
    acts, silos = (50_000 + new).astype(np.uint32), np.full(len(new), 3, np.uint8)
    eng.cache_add_or_update_device(dev(t, w.keys[new]), dev(t, acts), dev(t, silos), len(new), stream=st)
    for g in new.tolist():
        lru.add(w.kt[g], (50_000 + g, 3))
        unstamped.add(w.kt[g], (50_000 + g, 3))
    # on the reference alone: the partition's stamps change who survives (the cold and the never-looked-up entries go,
    # not the first added)
    assert set(lru.d) != set(unstamped.d) and len(set(unstamped.d) - set(lru.d)) >= 20
    all_keys = np.concatenate([case.cache_keys, w.keys[new]])
    act, _ = peek(t, eng, all_keys, st)
    kt = H.key_tuples(all_keys)
    assert {k for k, a in zip(kt, act.tolist()) if a != L.NO_ACT} == set(lru.d)
    np.testing.assert_array_equal(act, np.array([lru.d[k][0][0] if k in lru.d else L.NO_ACT for k in kt], np.uint32))
    stats = eng.cache_stats()
    assert eng.cache_count() == len(lru.d) and stats["host_fallbacks"] == 0 and stats["evict_batches"] >= 1
    eng.close()


def test_partition_marks_accessed_for_the_maintainer(torch, world):
    """Adaptive mode: after the partition the access mark is set for exactly the entries sender looked up (the hit on the
    non-functional silo included; the complete address, the system target, the KeyExt key excluded), and the maintainer at
    an expired `now` lists and removes what adaptive_cache_ref.maintainer_run does."""
    t, w = torch, world
    st = t.cuda.current_stream().cuda_stream
    ros, me = ros_of(w, 3)
    case = H.case_batch(w, ros, me, fmt=32)
    eng = engine_of(w)
    eng.cache_config_adaptive(4096, INITIAL, MAX_TTL, GROWTH)
    n_c = len(case.cache_keys)
    etags = np.arange(100, 100 + n_c, dtype=np.int32)
    eng.cache_add_or_update_versioned_device(dev(t, case.cache_keys), dev(t, case.cache_acts), dev(t, case.cache_silos),
                                             dev(t, etags), n_c, T0, stream=st)
    model = A.AdaptiveCache(4096, INITIAL, MAX_TTL, GROWTH)
    for (k, v), e in zip(case.entries(), etags.tolist()):
        model.add_or_update(k, v, e, T0)
    _, acc = peek(t, eng, case.cache_keys, st, adaptive=True)
    assert not acc.any()
    o = partition(t, eng, case.msgs, ros, 3, me, 32, case.opts, st)
    h = H.sender(w.o, model, case.msgs, ros, 3, me, 32, case.opts, w.functional)
    o.check(h, "adaptive cache")
    ck = H.key_tuples(case.cache_keys)
    kt = H.key_tuples(case.msgs)
    ref_acc = np.array([model.entry(k).num_accesses > 0 for k in ck], np.uint8)
    for c in ("S3", "S4", "S5", "S9", "HV"):  # on the reference: who is marked
        assert all(model.entry(kt[i]).num_accesses > 0 for i in case.at[c]), c
    for c in ("S6", "S7"):
        assert all(model.entry(kt[i]).num_accesses == 0 for i in case.at[c]), c
    # S8 on a ring of eight silos has an owner, the next silo: marked iff that one is remote (the null owner, which is
    # never looked up, needs the sender alone on the ring: test_partition_null_owner_stays_unlooked)
    assert all((model.entry(kt[i]).num_accesses > 0) == (not w.local[case.s8_owner]) for i in case.at["S8"])
    assert not ref_acc[case.cold].any() and 900 < ref_acc.sum() < n_c
    _, acc = peek(t, eng, case.cache_keys, st, adaptive=True)
    np.testing.assert_array_equal(acc, ref_acc, err_msg="access marks after the partition")
    # the maintainer, everything expired: the unaccessed go, the accessed are listed per owner
    ring = P.Ring()
    for s in range(8):
        ring.add_server(s, int(w.cl.hashes[s]))
    view = P.SiloView(running=[bool(x) for x in w.running], functional=w.functional, local=w.local)

    def owner_of(k):
        s, _ = P.calculate_target_silo(ring, P.Key(*k), P.jenkins_u64(*k), 0, view, True)
        return None if s == P.NULL_SILO else s

    now = T0 + INITIAL
    res = eng.cache_maintain(0, now, stream=st)
    etag_before = {k: v[0].etag for k, v in model.lru.d.items()}
    fetch, cnt = A.maintainer_run(model, list(model.lru.d), owner_of, lambda s: bool(w.local[s]), now)
    c = res["counts"]
    assert [c["self_owned"], c["kept"], c["expired"], c["refresh"], c["owner_null"]] == cnt, (c, cnt)
    assert cnt[0] >= 2 and cnt[1] == 0 and cnt[2] >= len(case.cold) and cnt[3] > 900, cnt  # conditions on the input
    off = res["owner_offsets"].astype(np.int64)
    keys = H.key_tuples(res["keys"])
    for s in range(8):
        got = set(zip(keys[off[s]:off[s + 1]], res["etags"][off[s]:off[s + 1]].tolist()))
        assert got == {(k, etag_before[k]) for k in fetch.get(s, [])}, f"owner {s}'s refresh list"
    act, acc = peek(t, eng, case.cache_keys, st, adaptive=True)
    assert {k for k, a in zip(ck, act.tolist()) if a != L.NO_ACT} == set(model.lru.d)
    assert not acc.any() and eng.cache_count() == len(model)
    eng.close()


def test_partition_cached_without_a_cache_is_the_plain_partition(torch, world):
    """No cache configured: records, counts and status equal partition_by_owner_padded / _compact / _narrow_device on the
    same batch, the lane is ORL_NO_ACT inside every count, ORL_PART_CACHED never set."""
    t, w = torch, world
    st = t.cuda.current_stream().cuda_stream
    ros, me = ros_of(w, 3)
    eng = engine_of(w)
    types = H.wire_types_of(w)
    eng.set_wire_types(types)
    for n in (1, 2049, H.CASE_N):
        msgs = random_batch(w, n, seed=70 + n)
        d_in = dev(t, msgs)
        for fmt in (8, 16, 32):
            o = partition(t, eng, msgs, ros, 3, me, fmt, 0, st)
            p = Out(t, n, 3, fmt)
            if fmt == 32:
                eng.partition_by_owner_padded_device(d_in, n, ros, 3, me, p.stride, p.d_out, p.d_cnt, stream=st)
                p.d_st.zero_()
            elif fmt == 16:
                eng.partition_compact_device(d_in, n, ros, 3, me, p.stride, p.d_out, p.d_cnt, p.d_st, stream=st)
            else:
                eng.partition_narrow_device(d_in, n, ros, 3, me, p.stride, p.d_out, p.d_cnt, p.d_st, stream=st)
            out, lane, cnt, status = o.host()
            out_p, _, cnt_p, status_p = p.host()
            np.testing.assert_array_equal(cnt, cnt_p)
            np.testing.assert_array_equal(out, out_p, err_msg=f"fmt {fmt}, n = {n}")  # the sentinels past the counts too
            assert status == status_p == 0
            for r in range(3):
                assert (lane[r * o.stride:r * o.stride + int(cnt[r])] == L.NO_ACT).all()
            o.check(H.sender(w.o, None, msgs, ros, 3, me, fmt, 0, w.functional, types), f"no cache, fmt {fmt}",
                    lane_past_count=False)
    eng.close()


def test_partition_cached_argument_edges(torch, world):
    t, w = torch, world
    st = t.cuda.current_stream().cuda_stream
    ros, me = ros_of(w, 2)
    case = H.case_batch(w, ros, me, fmt=16)
    eng = engine_of(w)
    eng.cache_config(4096)
    cache_fill(t, eng, case, st)
    n = 700
    msgs = random_batch(w, n, seed=3)
    d_in = dev(t, msgs)
    o = Out(t, n, 2, 32)

    def call(fmt=32, stride=o.stride, lane=o.d_lane, nn=n):
        eng.partition_cached_device(d_in, nn, ros, 2, me, stride, o.d_out, fmt, lane, o.d_cnt, o.d_st, stream=st)

    for bad in (0, 4, 12, 24, 64):
        with pytest.raises(OrleansRouteError):
            call(fmt=bad)
    with pytest.raises(OrleansRouteError):
        call(stride=n - 1)
    with pytest.raises(OrleansRouteError):
        call(lane=None)
    with pytest.raises(OrleansRouteError):  # the 8-B form needs the wire types
        call(fmt=8)
    call(lane=None, nn=0)  # nothing to write: no lane needed
    t.cuda.synchronize()
    assert (o.d_cnt.cpu().numpy() == 0).all()
    # a message without the 16-B / 8-B form: the status bits of the uncached forms, beside ORL_PART_CACHED
    types = H.wire_types_of(w)
    eng.set_wire_types(types)
    for field, val, want16, want8 in (("n1", 1 << 32, 0, 2), ("tcd", H.grain_tcd(w.cl) + 1, 0, 2), ("n0", 1, 1, 3),
                                      ("flags", L.HDR_HASH_VALID, 1, 3), ("tcd", (3 << 56) | 0x0000123412345678, 1, 3)):
        m2 = msgs.copy()
        m2[field][433] = val
        d2 = dev(t, m2)
        for fmt, want in ((16, want16), (8, want8)):
            o2, p2 = Out(t, n, 2, fmt), Out(t, n, 2, fmt)
            eng.partition_cached_device(d2, n, ros, 2, me, o2.stride, o2.d_out, fmt, o2.d_lane, o2.d_cnt, o2.d_st, stream=st)
            plain = eng.partition_compact_device if fmt == 16 else eng.partition_narrow_device
            plain(d2, n, ros, 2, me, p2.stride, p2.d_out, p2.d_cnt, p2.d_st, stream=st)
            t.cuda.synchronize()
            got, got_plain = int(o2.d_st.item()), int(p2.d_st.item())
            assert got_plain == want and got == (want | L.PART_CACHED), (field, fmt, got, got_plain)
            h = H.sender(w.o, dict(case.entries()), m2, ros, 2, me, fmt, 0, w.functional, types)
            assert h.status == got
    eng.close()


# ---- the receiver ---------------------------------------------------------------------------------------------------------

def receiving_engine(t, rw, st, cache=None, max_batch=1 << 14):
    """The receiving rank's context: registered while silo 5 is functional, which it then stops being."""
    w = rw.w
    eng = GrainDirectoryEngine(n_act=rw.n_act, dir_capacity=w.n_grains, max_batch=max_batch, device=0)
    eng.set_silos(8, functional=rw.functional_at_registration, local=rw.local)
    for s in range(8):
        eng.add_server(s, int(w.cl.hashes[s]))
    status, _, _ = eng.register_single_activation(w.keys[rw.held], rw.acts, rw.silos)
    assert (status == L.INS_INSERTED).all()
    eng.set_silos(8, functional=rw.functional, local=rw.local)
    eng.set_wire_types(H.wire_types_of(w))
    model = None
    if cache is not None:
        eng.cache_config_adaptive(4096, INITIAL, MAX_TTL, GROWTH)
        keys = np.zeros(len(cache), L.KEY_DTYPE)
        keys["tcd"], keys["n0"], keys["n1"] = [k[0] for k in cache], [k[1] for k in cache], [k[2] for k in cache]
        acts = np.array([v[0] for v in cache.values()], np.uint32)
        silos = np.array([v[1] for v in cache.values()], np.uint8)
        eng.cache_add_or_update_versioned_device(dev(t, keys), dev(t, acts), dev(t, silos),
                                                 dev(t, np.zeros(len(cache), np.int32)), len(cache), T0, stream=st)
        model = A.AdaptiveCache(4096, INITIAL, MAX_TTL, GROWTH)
        for k, v in cache.items():
            model.add_or_update(k, v, 0, T0)
    return eng, model


def received(t, eng, d_recs, fmt, n, d_lane, st):
    d_route = t.full((max(n, 1),), -1, dtype=t.int32, device="cuda")
    d_act = t.full((max(n, 1),), -2, dtype=t.int32, device="cuda")
    eng.route_received_device(d_recs, fmt, n, d_lane, d_route, d_act, stream=st)
    t.cuda.synchronize()
    return d_route.cpu().numpy().view(np.uint32)[:n], d_act.cpu().numpy().view(np.uint32)[:n]


@pytest.mark.parametrize("fmt", [8, 16, 32])
def test_route_received_vs_receiver(torch, fmt):
    """Every receiver verdict (hop1_ref.receiver_cases' classes R1-R7) on both sides of a route tile's edge; the receiver's
    own cache, holding other entries for the R7 grains, is neither used nor marked; once more with stateless-worker types
    set (the SW + CIN instance); lane-free input equals the plain route."""
    t = torch
    st = t.cuda.current_stream().cuda_stream
    rw = H.ReceivingWorld(CE.World(CE.SCENARIO_GRAINS))
    types = H.wire_types_of(rw.w)
    full = H.ROUTE_TILE + 1
    m, lane, cls, cache = H.receiver_cases(rw, full)
    assert len(cache) > 100
    eng, model = receiving_engine(t, rw, st, cache)
    recs, ok16, ok8 = H.encode(m, fmt, types)
    assert ok16.all() and ok8.all()
    ckeys = np.zeros(len(cache), L.KEY_DTYPE)
    ckeys["tcd"], ckeys["n0"], ckeys["n1"] = [k[0] for k in cache], [k[1] for k in cache], [k[2] for k in cache]
    for n in (1, 63, H.ROUTE_TILE - 1, H.ROUTE_TILE, full):  # prefixes: the classes cycle, the cache is the whole batch's
        r_ref, a_ref = H.receiver(rw.o, m[:n], lane[:n], rw.functional, cache=model)
        r, a = received(t, eng, dev(t, recs[:n]), fmt, n, dev(t, lane[:n]), st)
        np.testing.assert_array_equal(r, r_ref, err_msg=f"fmt {fmt}, n = {n}: route words")
        np.testing.assert_array_equal(a, a_ref, err_msg=f"fmt {fmt}, n = {n}: handles")
    for c in H.RECV_PATTERN:
        assert (cls == c).sum() > 300
    _, acc = peek(t, eng, ckeys, st, adaptive=True)
    assert not acc.any() and not any(v[0].num_accesses for v in model.lru.d.values())
    eng.set_stateless_types([H.grain_tcd(rw.w.cl) + 1], [1])
    r, a = received(t, eng, dev(t, recs), fmt, full, dev(t, lane), st)
    r_ref, a_ref = H.receiver(rw.o, m, lane, rw.functional, cache=model)
    np.testing.assert_array_equal(r, r_ref, err_msg="stateless-worker types set: route words")
    np.testing.assert_array_equal(a, a_ref, err_msg="stateless-worker types set: handles")
    eng.set_stateless_types([], [])
    # R1 only: the plain route of the same records
    m1, lane1, _, _ = H.receiver_cases(rw, full, seed=5, only_r1=True)
    assert (lane1 == H.NO_ACT).all()
    recs1, _, _ = H.encode(m1, fmt, types)
    d1 = dev(t, recs1)
    r, a = received(t, eng, d1, fmt, full, dev(t, lane1), st)
    d_route = t.empty(full, dtype=t.int32, device="cuda")
    d_act = t.empty(full, dtype=t.int32, device="cuda")
    plain = {8: eng.address_narrow_device, 16: eng.address_compact_device, 32: eng.address_messages_device}[fmt]
    plain(d1, full, d_route, d_act, stream=st, opts=L.OPT_NO_BUCKETS)
    t.cuda.synchronize()
    np.testing.assert_array_equal(r, d_route.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(a, d_act.cpu().numpy().view(np.uint32))
    r_ref, a_ref = H.receiver(rw.o, m1, lane1, rw.functional, cache=model)
    np.testing.assert_array_equal(r, r_ref)
    np.testing.assert_array_equal(a, a_ref)
    eng.close()


@pytest.mark.parametrize("fmt", [8, 16, 32])
def test_partitioned_regions_through_route_received(torch, world, fmt):
    """Hop 1 end to end on two contexts: the region and lane partition_cached_device wrote for rank 1, as they lie on the
    device, through route_received_device on a context holding rank 1's directory (where silo 5, which the sender's cache
    still points at, is no longer functional)."""
    t, w = torch, world
    st = t.cuda.current_stream().cuda_stream
    ros, me = ros_of(w, 2)
    case = H.case_batch(w, ros, me, fmt=fmt)
    types = H.wire_types_of(w)
    snd = engine_of(w)
    snd.set_wire_types(types)
    snd.cache_config(4096)
    cache_fill(t, snd, case, st)
    # true entries too: a third of rank 1's grains cached with their real handle and silo, so records get confirmed
    rw = H.ReceivingWorld(w, local=[int(r == 1) for r in ros])
    true_g = rw.held[::3]
    have = set(H.key_tuples(case.cache_keys))
    true_g = np.array([g for g in true_g.tolist() if w.kt[g] not in have], np.int64)
    sel = np.isin(rw.held, true_g)
    snd.cache_add_or_update_device(dev(t, w.keys[true_g]), dev(t, rw.acts[sel]), dev(t, rw.silos[sel]), len(true_g), stream=st)
    cache = dict(case.entries())
    for g, a, s in zip(true_g.tolist(), rw.acts[sel].tolist(), rw.silos[sel].tolist()):
        cache[w.kt[g]] = (a, s)
    o = partition(t, snd, case.msgs, ros, 2, me, fmt, case.opts, st)
    h = H.sender(w.o, cache, case.msgs, ros, 2, me, fmt, case.opts, w.functional, types)
    o.check(h, f"two contexts, fmt {fmt}")
    rcv, _ = receiving_engine(t, rw, st)
    c1 = int(h.counts[1])
    r, a = received(t, rcv, o.d_out[o.stride:o.stride + c1], fmt, c1, o.d_lane[o.stride:o.stride + c1], st)
    r_ref, a_ref = H.receiver(rw.o, h.headers_for(1), h.lanes[1], rw.functional)
    np.testing.assert_array_equal(r, r_ref, err_msg="route words")
    np.testing.assert_array_equal(a, a_ref, err_msg="handles")
    fl = r_ref >> 24
    kept = ((fl & L.RF_CACHED) != 0) & (H.status_of(r_ref) == L.ST_HIT)
    assert kept.sum() > 300 and ((fl & L.RF_CACHE_STALE) != 0).sum() > 50 and c1 > 2000  # conditions on the input
    snd.close()
    rcv.close()
