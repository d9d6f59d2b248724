"""Stateless-worker grains on the CPU: the restatement (tests/stateless_ref.py) against hand-written cases, and the
library's host-side catalog (orl_sw_*, host-only contexts: device = -1) against the restatement's LocalCatalog.
Reference: StatelessWorkerDirector.cs:35-80, Catalog.cs:1156-1185 (paths relative to randa1/orleans)."""
import numpy as np
import pytest

import stateless_ref as S
from oracle import cpu_ref
from orleans_amd import _lib as L
from orleans_amd import workloads as W
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError, decode_route

T1 = (L.CAT_GRAIN << 56) | 0x101  # MaxLocal 1
T4 = (L.CAT_GRAIN << 56) | 0x104  # MaxLocal 4
TYPES = {T1: 1, T4: 4}
SW = L.RF_STATELESS | L.RF_LOOPBACK


def _key(tcd, n1, n0=0):
    k = np.zeros(1, L.KEY_DTYPE)
    k["tcd"], k["n0"], k["n1"] = tcd, n0, n1
    return k[0]


def _keys(tcd, n1s):
    k = np.zeros(len(n1s), L.KEY_DTYPE)
    k["tcd"], k["n1"] = tcd, np.asarray(n1s, np.uint64)
    return k


def _msg(tcd, n1, sender, flags=0, aux=0, target=0):
    m = np.zeros(1, L.MSG_DTYPE)
    m["tcd"], m["n1"], m["sending_silo"], m["category"] = tcd, n1, sender, 2
    m["flags"], m["aux"], m["target_silo"] = flags, aux, target
    return m


def _r1(ra):
    r, a = ra
    assert len(r) == 1 and len(a) == 1
    return int(r[0]), int(a[0])


def _oracle(n_silos=4, **kw):
    cl = W.default_cluster(n_silos)
    o = cpu_ref.Oracle(n_silos, **kw)
    for s in range(n_silos):
        o.add_server(s, int(cl.hashes[s]))
    return cl, o


# ---- the restatement, one hand-written case per row of the table ------------------------------------------------
def test_ref_rows_by_hand():
    cl, o = _oracle()
    cat = S.LocalCatalog(TYPES, n_act=100, n_silos=4)
    new = S.pack(0xFF, 2, L.ST_NEW_PLACEMENT, SW | L.RF_NEW_PLACEMENT)
    hit = S.pack(0xFF, 2, L.ST_HIT, SW)
    # absent (:46-47): placed on the sending silo, whatever the directory would say
    assert _r1(S.route(o, cat, TYPES, _msg(T4, 7, 2))) == (new, L.NO_ACT)
    # an entry on another silo only: still absent for sender 2
    assert cat.add(_key(T4, 7), 50, 1) == L.SW_ADDED
    assert _r1(S.route(o, cat, TYPES, _msg(T4, 7, 2))) == (new, L.NO_ACT)
    # idle (:51-58): the first idle one in list order, here at position 1
    for a in (10, 11, 12):
        assert cat.add(_key(T4, 7), a, 2) == L.SW_ADDED
    cat.set_busy(_key(T4, 7), 10, 2, True)
    assert _r1(S.route(o, cat, TYPES, _msg(T4, 7, 2))) == (hit, 11)
    # all busy, count < MaxLocal (:66): a new one
    cat.set_busy(_key(T4, 7), 11, 2, True)
    cat.set_busy(_key(T4, 7), 12, 2, True)
    assert _r1(S.route(o, cat, TYPES, _msg(T4, 7, 2))) == (new, L.NO_ACT)
    # all busy at MaxLocal, count > 1 (:60-64): list[h % count], h = aux with HASH_VALID
    assert cat.add(_key(T4, 7), 13, 2) == L.SW_ADDED
    cat.set_busy(_key(T4, 7), 13, 2, True)
    assert cat.add(_key(T4, 7), 14, 2) == L.SW_DUPLICATE  # Catalog.cs:1176-1180
    for aux in (0, 1, 6, 0xFFFFFFFF):
        assert _r1(S.route(o, cat, TYPES, _msg(T4, 7, 2, L.HDR_HASH_VALID, aux))) == (hit, [10, 11, 12, 13][aux % 4])
    h = int(W.jenkins3_np(*(np.array([v], np.uint64) for v in (T4, 0, 7)))[0])
    assert _r1(S.route(o, cat, TYPES, _msg(T4, 7, 2))) == (hit, [10, 11, 12, 13][h % 4])
    # all busy at MaxLocal, count == 1: local[0] whatever h
    assert cat.add(_key(T1, 9), 20, 2) == L.SW_ADDED
    cat.set_busy(_key(T1, 9), 20, 2, True)
    assert _r1(S.route(o, cat, TYPES, _msg(T1, 9, 2, L.HDR_HASH_VALID, 12345))) == (hit, 20)
    # a complete address passes through as the oracle has it; every other type too
    for m in (_msg(T4, 7, 2, L.HDR_ADDRESS_COMPLETE, target=3), _msg((L.CAT_GRAIN << 56) | 0x77, 7, 2)):
        r0, a0 = o.route(m)
        r1, a1 = S.route(o, cat, TYPES, m)
        assert (list(r0), list(a0)) == (list(r1), list(a1))
        assert not (decode_route(r1).flags[0] & L.RF_STATELESS)


def test_ref_ignores_ring_membership_and_policy():
    """No CalculateTargetSilo: an empty ring, a sender that is not running with EXCLUDE_IF_STOPPING, functional[] and the
    placement policy change nothing, and ORL_ST_OWNER_NULL never shows."""
    cat = S.LocalCatalog(TYPES, n_act=100, n_silos=4)
    cat.add(_key(T1, 1), 5, 3)
    m = np.concatenate([_msg(T1, 1, 3), _msg(T1, 2, 3)])
    want = None
    for kw, ring, opts in (({}, True, 0), ({"running": [1, 1, 1, 0], "functional": [1, 1, 1, 0]}, True, 1),
                           ({"running": [0, 0, 0, 0]}, False, 1), ({"policy": 1}, True, 0)):
        o = cpu_ref.Oracle(4, **kw)
        if ring:
            for s in range(4):
                o.add_server(s, int(W.default_cluster(4).hashes[s]))
        got = [[int(v) for v in x] for x in S.route(o, cat, TYPES, m, opts)]
        want = want or got
        assert got == want
    assert want == [[S.pack(0xFF, 3, L.ST_HIT, SW), S.pack(0xFF, 3, L.ST_NEW_PLACEMENT, SW | L.RF_NEW_PLACEMENT)],
                    [5, L.NO_ACT]]


# ---- the library's host-side catalog ------------------------------------------------------------------------------
def _engine(capacity=64, n_act=100, n_silos=4):
    eng = GrainDirectoryEngine(n_act=n_act, dir_capacity=16, device=-1)
    eng.set_silos(n_silos)
    eng.set_stateless_types(list(TYPES), list(TYPES.values()))
    eng.stateless_config(capacity)
    return eng


def _same(eng, cat, keys, silos):
    cnt, acts, busy = eng.stateless_lookup(keys, silos)
    for i in range(len(keys)):
        want = cat.lookup(keys[i], int(silos[i]))
        assert cnt[i] == len(want)
        assert list(acts[i][:cnt[i]]) == [a for a, _ in want]
        assert (acts[i][cnt[i]:] == L.NO_ACT).all()
        assert busy[i] == sum(1 << j for j, (_, b) in enumerate(want) if b)
    assert eng.stateless_count() == cat.count()


def test_host_catalog_vs_local_catalog():
    eng = _engine()
    cat = S.LocalCatalog(TYPES, 100, 4)
    rng = np.random.default_rng(5)
    keys = np.concatenate([_keys(T1, range(6)), _keys(T4, range(6))])
    grid_k = np.repeat(keys, 4)
    grid_s = np.tile(np.arange(4, dtype=np.uint8), len(keys))
    for step in range(40):
        n = 25
        k = keys[rng.integers(0, len(keys), n)]
        a = rng.integers(0, 12, n).astype(np.uint32)
        s = rng.integers(0, 4, n).astype(np.uint8)
        op = step % 4
        if op in (0, 1):
            got = eng.stateless_add(k, a, s)
            assert list(got) == [cat.add(k[i], int(a[i]), int(s[i])) for i in range(n)]
        elif op == 2:
            b = rng.integers(0, 2, n).astype(np.uint8)
            got = eng.stateless_set_busy(k, a, s, b)
            assert list(got) == [int(cat.set_busy(k[i], int(a[i]), int(s[i]), bool(b[i]))) for i in range(n)]
        else:
            got = eng.stateless_remove(k, a, s)
            assert list(got) == [int(cat.remove(k[i], int(a[i]), int(s[i]))) for i in range(n)]
        _same(eng, cat, grid_k, grid_s)
    eng.close()


def test_order_kept_after_removal_and_busy_bits_follow():
    eng = _engine()
    k = _keys(T4, [3] * 4)
    s = np.zeros(4, np.uint8)
    assert list(eng.stateless_add(k, [10, 11, 12, 13], s)) == [L.SW_ADDED] * 4
    assert list(eng.stateless_add(k[:1], [14], s[:1])) == [L.SW_DUPLICATE]      # the list is left unchanged
    assert list(eng.stateless_set_busy(k[:2], [11, 13], s[:2], [1, 1])) == [1, 1]
    assert list(eng.stateless_remove(k[:2], [10, 99], s[:2])) == [1, 0]
    cnt, acts, busy = eng.stateless_lookup(k[:1], s[:1])
    assert (cnt[0], list(acts[0][:3]), busy[0]) == (3, [11, 12, 13], 0b101)
    assert list(eng.stateless_add(k[:1], [15], s[:1])) == [L.SW_ADDED]          # appended at the end, idle
    cnt, acts, busy = eng.stateless_lookup(k[:1], s[:1])
    assert (cnt[0], list(acts[0][:4]), busy[0]) == (4, [11, 12, 13, 15], 0b0101)
    # an emptied list frees its entry
    assert list(eng.stateless_remove(k, [11, 12, 13, 15], s)) == [1] * 4
    assert eng.stateless_count() == 0 and eng.stateless_lookup(k[:1], s[:1])[0][0] == 0
    eng.close()


def test_validation_errors():
    eng = GrainDirectoryEngine(n_act=100, dir_capacity=16, device=-1)
    eng.set_silos(4)
    for types, maxl in (([(L.CAT_SYSTEM_GRAIN << 56) | 1], [1]),   # wrong category
                        ([T1, T1], [1, 2]),                         # duplicate
                        ([T1], [0]), ([T1], [9]),                   # MaxLocal outside 1..8
                        ([(L.CAT_GRAIN << 56) | i for i in range(9)], [1] * 9)):  # n > 8
        with pytest.raises(OrleansRouteError) as e:
            eng.set_stateless_types(types, maxl)
        assert e.value.code == L.E_INVALID
    eng.set_stateless_types([T1, T4], [1, 4])
    eng.stateless_config(8)
    k = np.concatenate([_keys((L.CAT_GRAIN << 56) | 0x77, [1]), _keys(T4, [1, 1, 1, 1])])
    st = eng.stateless_add(k, [1, 100, 2, 3, 3], [0, 0, 4, 0, 0])
    # type not listed, act >= n_act, silo out of range, added, the handle is already in that list
    assert list(st) == [L.SW_UNSUPPORTED, L.SW_UNSUPPORTED, L.SW_UNSUPPORTED, L.SW_ADDED, L.SW_UNSUPPORTED]
    # changing the types clears the catalog; n = 0 turns the feature off
    eng.set_stateless_types([T4], [2])
    assert eng.stateless_count() == 0
    eng.set_stateless_types([], [])
    assert list(eng.stateless_add(k[3:4], [3], [0])) == [L.SW_UNSUPPORTED]
    eng.close()


def test_capacity_and_tombstone_reuse():
    eng = _engine(capacity=8)  # 16 slots: at most 8 live entries
    k = _keys(T4, range(9))
    z = np.zeros(9, np.uint8)
    with pytest.raises(OrleansRouteError) as e:
        eng.stateless_add(k, np.arange(9), z)
    assert e.value.code == L.E_CAPACITY and eng.stateless_count() == 0  # before anything changed
    assert list(eng.stateless_add(k[:8], np.arange(8), z[:8])) == [L.SW_ADDED] * 8
    # a second activation of a present entry needs no slot; a ninth entry does
    assert list(eng.stateless_add(k[:1], [50], z[:1])) == [L.SW_ADDED]
    with pytest.raises(OrleansRouteError) as e:
        eng.stateless_add(k[8:], [8], z[8:])
    assert e.value.code == L.E_CAPACITY
    # remove + re-add cycles at 5 live entries: a re-add reuses a tombstone (three fit beside the live entries before the
    # table is rebuilt without them), chains never run out, and every lookup stays exact
    assert list(eng.stateless_remove(k[5:8], [5, 6, 7], z[5:8])) == [1, 1, 1]
    cat = {i: [i] for i in range(5)}
    cat[0].append(50)
    for rnd in range(40):
        i = rnd % 5
        assert list(eng.stateless_remove(np.repeat(k[i:i + 1], len(cat[i])), cat[i], np.zeros(len(cat[i]), np.uint8))) == \
            [1] * len(cat[i])
        assert eng.stateless_count() == 4
        kn = _keys(T4, [100 + rnd])
        assert list(eng.stateless_add(kn, [60 + (rnd % 30)], z[:1])) == [L.SW_ADDED]
        k[i] = kn[0]
        cat[i] = [60 + (rnd % 30)]
        cnt, acts, _ = eng.stateless_lookup(k[:5], z[:5])
        assert list(cnt) == [len(cat[j]) for j in range(5)]
        assert [list(acts[j][:cnt[j]]) for j in range(5)] == [cat[j] for j in range(5)]
        assert eng.stateless_lookup(k[5:8], z[5:8])[0].sum() == 0
    eng.close()


def test_entry_points_without_the_path_refuse():
    """Fan-out and KeyExt entries must not answer silently wrong while types are set (checked before any device work,
    so a host-only context shows it)."""
    eng = _engine()
    n_out_args = dict(d_pub_offsets=1, d_route=1, d_act=1, d_order=1, d_offsets=1)
    with pytest.raises(OrleansRouteError) as e:
        eng.fanout_device(1, 1, 1, 1, 1, T4, **n_out_args)
    assert e.value.code == L.E_INVALID and "stateless" in str(e.value)
    with pytest.raises(OrleansRouteError) as e:
        eng.fanout_keys_device(1, 1, 1, 1, 1, 1, **n_out_args)
    assert e.value.code == L.E_STATE and "stateless" in str(e.value)
    with pytest.raises(OrleansRouteError) as e:
        eng.fanout_mixed_device(1, 1, 1, 1, None, (L.CAT_GRAIN << 56) | 0x77, 1, 1, 1, **n_out_args)
    assert e.value.code == L.E_STATE and "stateless" in str(e.value)
    with pytest.raises(OrleansRouteError) as e:
        eng.address_keyext_device(1, 1, 1, 1, 1, 1, 1)
    assert e.value.code == L.E_STATE and "stateless" in str(e.value)
    # with the types unset the same calls get as far as the host-only check
    eng.set_stateless_types([], [])
    with pytest.raises(OrleansRouteError) as e:
        eng.fanout_keys_device(1, 1, 1, 1, 1, 1, **n_out_args)
    assert "stateless" not in str(e.value)
    eng.close()


def test_constants_match_header():
    import os
    import re
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "orleans_route.h")).read()
    d = dict(re.findall(r"#define (ORL_[A-Z_]+) (0x[0-9A-Fa-f]+|\d+)u", text))
    assert int(d["ORL_MAX_SW_TYPES"]) == L.MAX_SW_TYPES == 8
    assert int(d["ORL_SW_MAX_LOCAL"]) == L.SW_MAX_LOCAL == 8
    assert int(d["ORL_RF_STATELESS"], 16) == L.RF_STATELESS == 0x20
    assert (int(d["ORL_SW_ADDED"]), int(d["ORL_SW_DUPLICATE"]), int(d["ORL_SW_UNSUPPORTED"])) == (0, 1, 2)
    assert int(d["ORL_ABI_VERSION"]) == 1
