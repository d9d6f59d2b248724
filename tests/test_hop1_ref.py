"""tests/hop1_ref.py on the CPU: every class of the constructed batches occurs at its indices with the classification
intended (conditions on the reference alone, per class), and sender + receiver composed over the ranks of a small
node_replay.population reproduce node_replay.expected — the reference the node tests already trust."""
import numpy as np
import pytest

import cache_evict_ref as CE
import hop1_ref as H
import node_replay as R
from oracle import pyref as P
from orleans_amd import _lib as L

ROS3 = np.array([s % 3 for s in range(8)], np.uint8)
ROS8 = np.arange(8, dtype=np.uint8)


@pytest.fixture(scope="module")
def world():
    return H.stopping_world()


def filled(case, cap=4096):
    lru = P.LRUCache(cap)
    for k, v in case.entries():
        lru.add(k, v)
    return lru


@pytest.mark.parametrize("ros,nranks", [(ROS3, 3), (ROS8, 8)], ids=["3ranks", "8ranks"])
def test_case_batch_classes(world, ros, nranks):
    w = world
    case = H.case_batch(w, ros, 0, fmt=32)
    m, at = case.msgs, case.at
    assert len(m) == H.CASE_N == 5 * H.PART_TILE + 1
    for name, idx in at.items():  # the classes sit where CASE_AT says, and nowhere else
        assert (case.cls[idx] == name).all() and (case.cls == name).sum() == len(idx)
    lru = filled(case)
    gen0 = {k: v[1] for k, v in lru.d.items()}
    h = H.sender(w.o, lru, m, ros, nranks, 0, 32, case.opts, w.functional)
    r0, _ = w.o.route(m, case.opts)
    st, owner = H.status_of(r0), (r0 & 0xFF).astype(np.int64)
    looked, found = set(h.looked), set(h.found)
    kt = H.key_tuples(m)
    cached = dict(case.entries())
    unchanged = lambda i: h.hdr[i] == m[i]  # noqa: E731

    for i in at["S1"]:  # owner local: probed in the directory, never in the cache
        assert w.local[owner[i]] and st[i] in H.PROBED and i not in looked
        assert h.lane[i] == H.NO_ACT and h.dest[i] == ros[owner[i]] and unchanged(i)
    for i in at["S2"]:  # owner remote, cache miss
        assert st[i] == L.ST_REMOTE_OWNER and i in looked and i not in found and kt[i] not in cached
        assert h.lane[i] == H.NO_ACT and h.dest[i] == ros[owner[i]] and unchanged(i)
    for i in at["S3"]:  # a hit on a functional silo of a third rank
        act, silo = cached[kt[i]]
        assert i in found and w.functional[silo] and ros[silo] not in (0, ros[owner[i]])
        assert h.lane[i] == act and h.dest[i] == ros[silo] and h.hdr["target_silo"][i] == silo != m["target_silo"][i]
    for i in at["S4"]:  # a hit on one of my own silos: the self region, a handle of this rank
        act, silo = cached[kt[i]]
        assert i in found and w.local[silo] and ros[silo] == 0 and ros[owner[i]] != 0
        assert h.dest[i] == 0 and h.lane[i] == act < w.n_act and h.hdr["target_silo"][i] == silo
    for i in at["S5"]:  # a hit on the non-functional silo: the owner's rank, unaddressed, yet stamped
        act, silo = cached[kt[i]]
        assert i in found and not w.functional[silo]
        assert h.lane[i] == H.NO_ACT and h.dest[i] == ros[owner[i]] and unchanged(i)
        assert lru.d[kt[i]][1] > gen0[kt[i]]
    for i in at["S6"]:  # a cached grain with a complete address: untouched, not looked up
        assert kt[i] in cached and st[i] == L.ST_ADDRESS_COMPLETE and i not in looked
        assert h.dest[i] == 0 and h.lane[i] == H.NO_ACT and unchanged(i) and lru.d[kt[i]][1] == gen0[kt[i]]
    for j, i in enumerate(at["S7"]):  # a system target / a KeyExt-category key, both cached: decided before the probe
        assert kt[i] in cached and i not in looked and h.lane[i] == H.NO_ACT and unchanged(i)
        assert lru.d[kt[i]][1] == gen0[kt[i]]
        if j % 2 == 0:
            assert st[i] == L.ST_SYSTEM_TARGET and h.dest[i] == 0
        else:
            assert st[i] == L.ST_KEYEXT_UNRESOLVED and not w.local[owner[i]] and h.dest[i] == ros[owner[i]]
    # S8: the sender is not running and OPT_EXCLUDE_IF_STOPPING is set.  On a ring of eight the owner is then never null
    # (LocalGrainDirectory.cs:478-493): it moves off the sender, to s8_owner — null_owner_case has the null.
    r_plain, _ = w.o.route(m, 0)
    for i in at["S8"]:
        assert m["sending_silo"][i] == case.stopped and not w.running[case.stopped] and kt[i] in cached
        assert (r_plain[i] & 0xFF) == case.stopped and H.status_of(r_plain[i]) in H.PROBED  # without the option: its own
        assert owner[i] == case.s8_owner != case.stopped
        if w.local[case.s8_owner]:
            assert i not in looked and h.lane[i] == H.NO_ACT and h.dest[i] == ros[case.s8_owner]
        else:
            assert i in found and h.lane[i] == cached[kt[i]][0] and h.dest[i] == ros[cached[kt[i]][1]]
    s9 = at["S9"]  # one cached grain in every tile: its stamp is the last occurrence's
    assert len({kt[i] for i in s9}) == 1 and set(s9) <= found and s9[-1] == len(m) - 1 == h.looked[-1]
    assert sorted({i // H.PART_TILE for i in s9}) == list(range(6))
    assert lru.d[kt[s9[0]]][1] == lru.next_gen
    for i in at["HV"]:  # a precomputed hash, the right one: looked up like any other
        assert m["flags"][i] == L.HDR_HASH_VALID and m["aux"][i] == P.jenkins_u64(*kt[i])
        assert i in found and h.lane[i] == cached[kt[i]][0] and h.hdr["flags"][i] == L.HDR_HASH_VALID
    # the cold background entries are no message's target; the others are all found
    ck = H.key_tuples(case.cache_keys)
    hit_keys = {kt[i] for i in found}
    assert len(case.cold) >= 400 and not any(ck[j] in hit_keys for j in case.cold)
    assert all(lru.d[ck[j]][1] == gen0[ck[j]] for j in case.cold)
    assert h.status == L.PART_CACHED and int(h.counts.sum()) == len(m) and (h.counts > 0).all()
    for d in range(nranks):
        assert len(h.regions[d]) == len(h.lanes[d]) == h.counts[d]
        np.testing.assert_array_equal(h.regions[d], h.headers_for(d))
    # every message has the narrower forms, except the precomputed hashes
    for fmt in (16, 8):
        c2 = H.case_batch(w, ros, 0, fmt=fmt)
        assert "HV" not in c2.at
        h2 = H.sender(w.o, dict(c2.entries()), c2.msgs, ros, nranks, 0, fmt, c2.opts, w.functional, H.wire_types_of(w))
        assert h2.status == L.PART_CACHED and h2.regions[0].dtype == H.REC_DTYPE[fmt]
    h3 = H.sender(w.o, dict(case.entries()), m, ros, nranks, 0, 8, case.opts, w.functional, H.wire_types_of(w))
    assert h3.status == (L.PART_CACHED | 3)  # HASH_VALID has neither narrow form
    np.testing.assert_array_equal(h3.dest, h.dest)


def test_lookups_stamp_and_mark_both_cache_models(world):
    """sender leaves the same lookups on the LRU model and on the adaptive one (a stamp and NumAccesses)."""
    import adaptive_cache_ref as A
    w = world
    case = H.case_batch(w, ROS3, 0, fmt=16, n_background=150)
    ad = A.AdaptiveCache(4096)
    for k, v in case.entries():
        ad.add_or_update(k, v, 7, 1000)
    lru = filled(case)
    h1 = H.sender(w.o, lru, case.msgs, ROS3, 3, 0, 16, case.opts, w.functional)
    h2 = H.sender(w.o, ad, case.msgs, ROS3, 3, 0, 16, case.opts, w.functional)
    assert h1.found == h2.found and h1.looked == h2.looked
    kt = H.key_tuples(case.msgs)
    assert {k for k, v in ad.lru.d.items() if v[0].num_accesses > 0} == {kt[i] for i in h2.found}
    assert [k for k, _ in sorted(lru.d.items(), key=lambda kv: kv[1][1])] == ad.lru_order()
    for d in range(3):
        np.testing.assert_array_equal(h1.regions[d], h2.regions[d])
        np.testing.assert_array_equal(h1.lanes[d], h2.lanes[d])


def test_null_owner_case():
    w, m, opts, ent = H.null_owner_case()
    lru = P.LRUCache(256)
    for k, v in ent:
        lru.add(k, v)
    gen0 = lru.next_gen
    h = H.sender(w.o, lru, m, w.ros, w.nranks, w.my_rank, 32, opts, w.functional)
    r0, _ = w.o.route(m, opts)
    even, odd = np.arange(len(m)) % 2 == 0, np.arange(len(m)) % 2 == 1
    assert (H.status_of(r0[even]) == L.ST_OWNER_NULL).all() and ((r0[even] & 0xFF) == 0xFF).all()
    assert (h.dest[even] == w.my_rank).all() and (h.lane[even] == H.NO_ACT).all()
    assert set(h.looked) == set(h.found) == set(np.nonzero(odd)[0].tolist())
    assert (h.dest[odd] == w.ros[2]).all() and (h.lane[odd] == 50_000 + np.arange(len(m))[odd]).all()
    assert (h.hdr["target_silo"][odd] == 2).all() and lru.next_gen == gen0 + int(odd.sum())
    kt = H.key_tuples(m)
    assert all((lru.d[kt[i]][1] > gen0) == bool(i % 2) for i in range(len(m)))  # the even grains' entries: never stamped
    assert (H.status_of(w.o.route(m, 0)[0][even]) == L.ST_REMOTE_OWNER).all()  # without the option: silo 0's, looked up


@pytest.mark.parametrize("n", [63, H.ROUTE_TILE + 1])
def test_receiver_cases_classes(n):
    w = CE.World(CE.SCENARIO_GRAINS)
    rw = H.ReceivingWorld(w)
    m, lane, cls, cache = H.receiver_cases(rw, n)
    for c in H.RECV_PATTERN:
        assert (cls == c).sum() >= n // len(H.RECV_PATTERN)
    lru = P.LRUCache(4096)
    for k, v in cache.items():
        lru.add(k, v)
    gen0 = lru.next_gen
    r, a = H.receiver(rw.o, m, lane, rw.functional, cache=lru)
    r_own, a_own = rw.o.route(m)
    st, host, fl = H.status_of(r), (r >> 8) & 0xFF, r >> 24
    stale, cachedf = (fl & L.RF_CACHE_STALE) != 0, (fl & L.RF_CACHED) != 0
    ts = m["target_silo"]
    kt = H.key_tuples(m)
    sel = lambda c: cls == c  # noqa: E731
    s = sel("R1")
    assert (lane[s] == H.NO_ACT).all() and (r[s] == r_own[s]).all() and (a[s] == a_own[s]).all() and (st[s] == L.ST_HIT).all()
    s = sel("R1r")
    assert (lane[s] == H.NO_ACT).all() and (r[s] == r_own[s]).all() and (st[s] == L.ST_REMOTE_OWNER).all()
    s = sel("R2")
    assert (st[s] == L.ST_HIT).all() and cachedf[s].all() and not stale[s].any()
    assert (a[s] == lane[s]).all() and (host[s] == ts[s]).all() and (r[s] == (r_own[s] | (L.RF_CACHED << 24))).all()
    s = sel("R3")
    assert (st[s] == L.ST_HIT).all() and stale[s].all() and not cachedf[s].any()
    assert (a[s] == a_own[s]).all() and (a[s] != lane[s]).all() and (host[s] == ts[s]).all()
    s = sel("R4")
    assert (st[s] == L.ST_HIT).all() and stale[s].all() and not cachedf[s].any()
    assert (a[s] == lane[s]).all() and (host[s] != ts[s]).all() and np.asarray(rw.functional)[ts[s]].all()
    s = sel("R5")
    assert (st[s] == L.ST_NEW_PLACEMENT).all() and stale[s].all() and (a[s] == H.NO_ACT).all() and (lane[s] != H.NO_ACT).all()
    s = sel("R6")  # the directory holds that handle on that silo, which is not functional here
    held = dict(zip(rw.held.tolist(), zip(rw.acts.tolist(), rw.silos.tolist())))
    assert all(held[int(g)] == (int(l), int(t)) for g, l, t in zip(m["n1"][s], lane[s], ts[s]))
    assert not np.asarray(rw.functional)[ts[s]].any() and rw.functional_at_registration[5]
    assert (st[s] == L.ST_NEW_PLACEMENT).all() and stale[s].all() and (a[s] == H.NO_ACT).all()
    for c in ("R7", "R7x", "R7c"):  # not held: taken as addressed
        s = sel(c)
        assert (H.status_of(r_own[s]) == L.ST_REMOTE_OWNER).all()
        assert (st[s] == L.ST_HIT).all() and cachedf[s].all() and not stale[s].any()
        assert (a[s] == lane[s]).all() and (host[s] == ts[s]).all() and ((r[s] & 0xFF) == (r_own[s] & 0xFF)).all()
        assert (((fl[s] & L.RF_LOOPBACK) != 0) == (ts[s] == m["sending_silo"][s])).all()
    assert ((fl[sel("R7x")] & L.RF_LOOPBACK) != 0).all()
    s = sel("R7f")  # ... under the receiver's IsValidSilo: the FullLookup word, no handle
    assert not np.asarray(rw.functional)[ts[s]].any() and (r[s] == r_own[s]).all() and (a[s] == H.NO_ACT).all()
    assert (st[s] == L.ST_REMOTE_OWNER).all()
    # R7c: the receiver's own cache holds another entry for the grain: neither used nor stamped
    s = np.nonzero(sel("R7c"))[0]
    inc = [i for i in s.tolist() if kt[i] in cache]
    assert len(inc) >= len(s) // 2 >= 1
    assert all(cache[kt[i]] != (int(lane[i]), int(ts[i])) and a[i] == lane[i] for i in inc)
    assert lru.next_gen == gen0 and len(cache) >= 1


def test_receiver_refuses_a_lane_on_a_message_without_directory():
    w = CE.World(CE.SCENARIO_GRAINS)
    rw = H.ReceivingWorld(w)
    m, lane, _, _ = H.receiver_cases(rw, 4)
    m["flags"][1] = L.HDR_ADDRESS_COMPLETE
    with pytest.raises(ValueError):
        H.receiver(rw.o, m, lane, rw.functional)


def _caches(p, nranks, seed, skip=None):
    """As test_gpu_node._fill_caches, on the CPU: true entries for half the remote registered grains, stale ones for 5 %."""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(nranks):
        if r == skip:
            out.append({})
            continue
        remote = np.nonzero(p.reg & (p.ros[p.owner] != r))[0]
        pick = rng.choice(remote, len(remote) // 2, replace=False)
        stale = rng.choice(remote, len(remote) // 20, replace=False)
        c = {}
        for g in pick.tolist():
            c[(int(p.keys["tcd"][g]), int(p.keys["n0"][g]), int(p.keys["n1"][g]))] = (int(p.act[g]), int(p.host[g]))
        for g in stale.tolist():
            c[(int(p.keys["tcd"][g]), int(p.keys["n0"][g]), int(p.keys["n1"][g]))] = (int(rng.integers(0, p.n_act)),
                                                                                       int(rng.integers(0, 8)))
        out.append(c)
    return out


@pytest.mark.parametrize("nranks,chunks,skip", [(2, 2, None), (3, 1, 1)])
def test_sender_and_receiver_compose_to_node_replay(nranks, chunks, skip):
    ros = None if nranks != 3 else [s % 3 for s in range(8)]
    p = R.population(nranks, n_grains=4000, seed=5, host_mix=0.3, ros=ros)
    oracles = [R.rank_oracle(p, r) for r in range(nranks)]
    caches = _caches(p, nranks, 11 + nranks, skip)
    batches = [R.messages(p, r, 3000 - 170 * r, seed=40 + r, wide_at=(17 if r == 0 else None)) for r in range(nranks)]
    exp, forward = R.expected(oracles, p.ros, batches, chunks, p.n_act, caches=caches)
    owned, lanes = [[] for _ in range(nranks)], [[] for _ in range(nranks)]
    for c in range(chunks):
        for s in range(nranks):
            lo, hi = R.chunk_bounds(len(batches[s]), chunks, c)
            h = H.sender(oracles[s], caches[s], batches[s][lo:hi], p.ros, nranks, s, 32)
            for d in range(nranks):
                owned[d].append(h.regions[d])
                lanes[d].append(h.lanes[d])
    owned = [np.concatenate(x) for x in owned]
    routed = [H.receiver(oracles[d], owned[d], np.concatenate(lanes[d]), [1] * 8) for d in range(nranks)]
    n_cached = sum(int((((r >> 24) & L.RF_CACHED) != 0).sum()) for r, _ in routed)
    n_stale = sum(int((((r >> 24) & L.RF_CACHE_STALE) != 0).sum()) for r, _ in routed)
    assert n_cached > 500 and n_stale > 20 and forward  # conditions on the input: the caches addressed a real share
    # node_replay.expected returns the hosted sets, after its hop-2 step: the same step (its host_rank) over this result
    hostr = [R.host_rank(routed[d][0], p.ros, d) for d in range(nranks)]
    for hr in range(nranks):
        sel = [hostr[o] == hr for o in range(nranks)]
        np.testing.assert_array_equal(np.concatenate([owned[o][sel[o]] for o in range(nranks)]), exp[hr][4])
        np.testing.assert_array_equal(np.concatenate([routed[o][0][sel[o]] for o in range(nranks)]), exp[hr][0])
        np.testing.assert_array_equal(np.concatenate([routed[o][1][sel[o]] for o in range(nranks)]), exp[hr][1])
