"""The directory's probe chains on small, crowded tables, on the device.

Every routed message ends in a linear-probe walk that is written out separately in route_msg, route_msg16, the three
branches of k_route (8-B, 16-B and 32-B slots), the U-wide fan-out kernel, find_or_claim, the KeyExt insert, the device
remove / split / merge kernels, k_probe_build and the host mirror.  The rest of the suite compares them with the oracle on
tables of thousands of slots at load <= 0.5, where a chain is one or two slots long and hardly ever crosses the table's
last slot.  Here the partition has 2, 8, 64 or 4096 slots and holds the key families of tests/dir_layout.py (every key
starting in the last slots, at one slot, or at the last slot of a 64-B line) at exactly half load, with tombstones inside
the chains.  The reference is the oracle's std::unordered_map partition (oracle/cpu_ref.cpp; pyref for the KeyExt table and
the merge), which knows nothing of slots; every comparison is exact.
"""
import numpy as np
import pytest

import dir_layout as D
from oracle import cpu_ref, pyref as P
from orleans_amd import _lib as L
from orleans_amd import workloads as W
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError, decode_route

pytestmark = pytest.mark.gpu

N_SILOS = 8
N_ACT = 1 << 14        # handles stay far below 2^24: the tables keep the 8-B probe form
MAX_BATCH = 1 << 15
CASES = [(s, n) for s in D.SIZES for n in D.family_names(s)]
IDS = [f"{s}-{n}" for s, n in CASES]
FORMS = (("default", {"ORL_NO_PROBE8": "0", "ORL_NO_PROBE16": "0"}, 8),
         ("no8", {"ORL_NO_PROBE8": "1", "ORL_NO_PROBE16": "0"}, 16),
         ("no16", {"ORL_NO_PROBE8": "0", "ORL_NO_PROBE16": "1"}, 32))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def cluster():
    return W.default_cluster(N_SILOS)


def _engine(cluster, slots, monkeypatch=None, env=None, n_silos=N_SILOS, local=None):
    """A context whose partition has exactly `slots` slots; the probe-form knobs are read at creation."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    eng = GrainDirectoryEngine(n_act=N_ACT, dir_capacity=slots // 2, max_batch=MAX_BATCH, device=0)
    eng.set_silos(n_silos, local=local, seed=0)
    for s in range(n_silos):
        eng.add_server(s, int(cluster.hashes[s]))
    return eng


def _oracle(cluster):
    o = cpu_ref.Oracle(N_SILOS, seed=0)
    for s in range(N_SILOS):
        o.add_server(s, int(cluster.hashes[s]))
    return o


def _both(eng, o, keys, acts, silos):
    """A host registration on the engine and the oracle: statuses and winners equal."""
    st, wa, ws = eng.register_single_activation(keys, acts, silos)
    st_o, wa_o, ws_o = o.register(keys, acts, silos)
    np.testing.assert_array_equal(st, st_o)
    np.testing.assert_array_equal(wa, wa_o)
    np.testing.assert_array_equal(ws, ws_o)
    return st


def _route_equal(eng, o, msgs):
    """address_messages == the oracle on route word, activation handle, order and offsets; returns the four arrays."""
    res = eng.address_messages(msgs)
    r, a = o.route(msgs)
    np.testing.assert_array_equal(res.route, r)
    np.testing.assert_array_equal(res.act, a)
    order, off = o.bucket(a, N_ACT)
    np.testing.assert_array_equal(res.offsets, off)
    np.testing.assert_array_equal(res.order, order)
    return res.route.copy(), res.act.copy(), res.order.copy(), res.offsets.copy()


def _batch(kinds, n, seed):
    """n messages drawn from the key lists of `kinds` (name -> keys), each kind at least once when n allows; returns the
    messages and, per message, the index of its kind."""
    rng = np.random.default_rng(seed)
    names = [k for k in kinds if len(kinds[k])]
    pool = np.concatenate([kinds[k] for k in names])
    label = np.concatenate([np.full(len(kinds[k]), i) for i, k in enumerate(names)])
    first = np.array([int(np.nonzero(label == i)[0][0]) for i in range(len(names))])
    pick = rng.integers(0, len(pool), n)
    if n >= len(names):
        pick[rng.permutation(n)[: len(names)]] = first
    msgs = D.messages(pool[pick], N_SILOS, seed)
    return msgs, label[pick], names


def _host_table(eng, o, f):
    """Steps of scenario a on one context: exact half load, then every other key unregistered (tombstones inside the
    chains).  Returns (live keys, removed keys)."""
    m = len(f.keys)
    st = _both(eng, o, f.keys, np.arange(m, dtype=np.uint32) + 100, (np.arange(m) % N_SILOS).astype(np.uint8))
    assert (st == L.INS_INSERTED).all()
    assert eng.directory_count() * 2 == f.slots == o.size() * 2
    gone = f.keys[::2]
    rm = eng.unregister(gone)
    np.testing.assert_array_equal(rm, o.unregister(gone))
    assert rm.all()
    return f.keys[1::2], gone


def _reregister_third(eng, o, f, gone):
    """A third of the removed keys again with new handles.  The host insert's documented rule, (count + tombstones + 1)
    * 2 > slots refuses, is evaluated from the counts; where it refuses, the partition is compacted first."""
    back = gone[::3]
    count, tombs = eng.directory_count(), len(gone)
    assert count == len(f.keys) - len(gone)
    if (count + tombs + 1) * 2 > f.slots:
        with pytest.raises(OrleansRouteError) as e:
            eng.register_single_activation(back[:1], np.array([1], np.uint32), np.zeros(1, np.uint8))
        assert e.value.code == L.E_CAPACITY
        eng.compact_directory()
        tombs = 0
        assert eng.directory_count() == o.size()
    assert (count + tombs + len(back)) * 2 <= f.slots
    st = _both(eng, o, back, np.arange(len(back), dtype=np.uint32) + 9000, ((np.arange(len(back)) + 5) % N_SILOS).astype(np.uint8))
    assert (st == L.INS_INSERTED).all()
    return back


@pytest.mark.parametrize("slots,name", CASES, ids=IDS)
def test_host_built_table_every_probe_form(torch, cluster, monkeypatch, slots, name):
    """Scenario a.  A host-built table at exactly half load, every other key unregistered, a third of those registered
    again with new handles (after the compaction the host insert's load rule asks for), routed with the default probe
    form (8-B), with ORL_NO_PROBE8=1 (16-B) and with ORL_NO_PROBE16=1 (32-B): hits, removed keys, ghosts of the same
    start slots and N1 + 2^32 aliases, in batches of 1 to 20 000 messages, before the re-registration (tombstones in the
    chains) and after it.  The three forms equal each other and the oracle; every kind of message occurs; HIT and
    NEW_PLACEMENT occur in the numbers the oracle gives, which are the numbers of messages to live and to absent keys."""
    f = D.family(name, slots, W.grain_tcd(cluster))
    f.check()
    outs = {}
    for form, env, width in FORMS:
        eng = _engine(cluster, slots, monkeypatch, env)
        o = _oracle(cluster)
        live, gone = _host_table(eng, o, f)
        for phase in ("tombstones", "reregistered"):
            if phase == "reregistered":
                back = _reregister_third(eng, o, f, gone)
                kinds = {"hit": live, "back": back, "removed": np.setdiff1d(gone, back), "ghost": f.ghosts, "alias": f.aliases}
            else:
                kinds = {"hit": live, "removed": gone, "ghost": f.ghosts, "alias": f.aliases}
            for n in (1, 63, 4097, 20_000):
                msgs, label, names = _batch(kinds, n, seed=slots * 31 + n)
                got = _route_equal(eng, o, msgs)
                key = (phase, n)
                if key in outs:
                    for x, y in zip(outs[key], got):
                        np.testing.assert_array_equal(x, y)
                outs[key] = got
                if n > 1:
                    assert set(label.tolist()) == set(range(len(names))), "a kind of message is missing from the batch"
                    present = np.isin(label, [names.index(k) for k in ("hit", "back") if k in names])
                    if len(live) == 0 and phase == "tombstones":
                        assert not present.any()  # 2 slots: the only key is the removed one
                    else:
                        assert present.any() and not present.all()
                    status = decode_route(got[0]).status
                    assert (status == L.ST_HIT).sum() == present.sum()
                    assert (status == L.ST_NEW_PLACEMENT).sum() == (~present).sum()
            # (a 2-slot table holds no live key in the first phase and comes out of an empty compaction in the second:
            # the host then has no type to build the 8-B form for, and the 16-B form serves)
            assert eng.query(L.Q_PROBE_FORM) == (16 if slots == 2 and width == 8 else width), (form, phase)
        eng.close()


def _csr(f, live, gone, seed):
    """A small follower graph over the family: 48 publishers whose followers are live keys, removed keys and ghosts (N1
    values), one publisher following every key of the family, a few following nobody."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([live["n1"], gone["n1"], f.ghosts["n1"]]).astype(np.uint32)
    lists = [np.concatenate([f.keys["n1"], f.ghosts["n1"]]).astype(np.uint32)]
    for p in range(47):
        deg = 0 if p % 11 == 0 else int(rng.integers(1, 40))
        lists.append(pool[rng.integers(0, len(pool), deg)])
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return off, np.concatenate(lists).astype(np.uint32)


@pytest.mark.parametrize("slots,name", CASES, ids=IDS)
def test_fanout_kernel_on_crowded_table(torch, cluster, monkeypatch, slots, name):
    """Scenario b.  The fan-out kernel (fanout_device) over the table of scenario a with its tombstones: followers are
    the family's live keys, removed keys and ghosts.  The kernel walks the 8-B table one message at a time and the 16-B
    table U messages at a time (ORL_FAN_U unset, "2", "4"), so every U runs on a context without the 8-B form
    (ORL_NO_PROBE8=1), which is the form ORL_FAN_PROBE16=1 selects: that knob is read once per process, so setting it
    here only takes effect when no fan-out ran before, and the test does not depend on it.  Expected: cpu_ref.fanout_expand
    plus the oracle's route and stable bucketing; the same expanded batch through address_messages must agree too."""
    t = torch
    tcd = W.grain_tcd(cluster)
    f = D.family(name, slots, tcd)
    f.check()
    dv = "cuda"
    configs = (("8-B, U=1", {"ORL_NO_PROBE8": "0"}, None),
               ("16-B, default U", {"ORL_NO_PROBE8": "1"}, None),
               ("16-B, U=2", {"ORL_NO_PROBE8": "1"}, "2"),
               ("16-B, U=4", {"ORL_NO_PROBE8": "1", "ORL_FAN_PROBE16": "1"}, "4"))
    for label, env, fan_u in configs:
        monkeypatch.setenv("ORL_NO_PROBE16", "0")
        if fan_u is None:
            monkeypatch.delenv("ORL_FAN_U", raising=False)
        else:
            monkeypatch.setenv("ORL_FAN_U", fan_u)
        eng = _engine(cluster, slots, monkeypatch, env)
        o = _oracle(cluster)
        live, gone = _host_table(eng, o, f)
        off, tgt = _csr(f, live, gone, seed=slots)
        rng = np.random.default_rng(slots + 1)
        pubs = np.concatenate([np.arange(len(off) - 1), rng.integers(0, len(off) - 1, 16)]).astype(np.uint32)
        psilo = rng.integers(0, N_SILOS, len(pubs)).astype(np.uint8)
        exp, poff_ref = cpu_ref.fanout_expand(off, tgt, pubs, psilo, tcd)
        total = len(exp)
        assert len(f.keys) + len(f.ghosts) < total <= MAX_BATCH
        poff = t.empty(len(pubs) + 1, dtype=t.int64, device=dv)
        outs = [t.empty(total, dtype=t.int32, device=dv) for _ in range(3)]
        of = t.empty(N_ACT + 2, dtype=t.int32, device=dv)
        got = eng.fanout_device(t.from_numpy(off.view(np.int64)).to(dv), t.from_numpy(tgt.view(np.int32)).to(dv),
                                t.from_numpy(pubs.view(np.int32)).to(dv), t.from_numpy(psilo).to(dv), len(pubs), tcd, poff,
                                *outs, of, stream=t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        assert got == total, label
        r, a, od, fo = (x.cpu().numpy().view(np.uint32) for x in outs + [of])
        np.testing.assert_array_equal(poff.cpu().numpy().view(np.uint64), poff_ref)
        ro, ao = o.route(exp)
        np.testing.assert_array_equal(r, ro, err_msg=label)
        np.testing.assert_array_equal(a, ao, err_msg=label)
        order, offsets = o.bucket(ao, N_ACT)
        np.testing.assert_array_equal(fo, offsets, err_msg=label)
        np.testing.assert_array_equal(od, order, err_msg=label)
        status = decode_route(ro).status
        n_live = int(np.isin(exp["n1"], live["n1"]).sum())
        assert (status == L.ST_HIT).sum() == n_live and (status == L.ST_NEW_PLACEMENT).sum() == total - n_live > 0
        assert n_live > 0 or len(live) == 0
        _route_equal(eng, o, exp)  # the route kernel on the same messages
        eng.close()


def _dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _fits(slots, count, tombs, n):
    """orl_dir_insert_single_device's documented rule: every message might insert; live entries stay <= 1/2 of the slots
    and entries + tombstones <= 7/8."""
    return (count + n) * 2 <= slots and (count + tombs + n) * 8 <= slots * 7


def _largest_fit(slots, count, tombs):
    n = 0
    while _fits(slots, count, tombs, n + 1):
        n += 1
    return n


@pytest.mark.parametrize("slots,name", CASES, ids=IDS)
def test_device_mutation_under_crowding(torch, cluster, monkeypatch, slots, name):
    """Scenario c.  register_single_activation_device and unregister_device on two contexts in lockstep (the
    device-rebuilt 16-B probe table, and ORL_NO_PROBE16=1: the 32-B table).  Every insert batch is the largest the
    documented fits() rule allows: a third of it one key under different handles, a third removed keys again, the rest
    keys that never were in the table (the family's first, then control keys of random start slots).  After every call
    statuses, winners and removed flags equal the oracle applying the batch one message at a time, the count equals the
    oracle's, and both contexts route a batch of live, removed, ghost and alias keys like the oracle.

    One key is registered from the host and routed first, so the context knows the type and rebuilds the 16-B table on
    the device afterwards.  Device batches then fill the table to exactly half load (no tombstones yet, so the rule is
    exact), and rounds follow: half of the live keys out, the largest batch in.  The test knows the entry count exactly
    (directory_count) but the tombstones only between bounds, because an insert takes a tombstone or an empty slot
    depending on the layout: t_hi counts every removal since the last compaction, t_lo subtracts every insert.  Batches
    are sized with t_hi, so they must be accepted.  Since the table was full, t_lo = slots / 2 - count, so once fewer
    than slots / 8 keys are live even t_lo tombstones make a batch that the half-load rule alone would take pass 7/8:
    that batch must be refused with E_CAPACITY and change nothing.  Then compact_directory(), one more device round,
    and a host registration that reads the device-built table back."""
    t = torch
    tcd = W.grain_tcd(cluster)
    f = D.family(name, slots, tcd)
    f.check()
    st_ = t.cuda.current_stream().cuda_stream
    engs = [_engine(cluster, slots, monkeypatch, {"ORL_NO_PROBE8": "0", "ORL_NO_PROBE16": "0"}),
            _engine(cluster, slots, monkeypatch, {"ORL_NO_PROBE8": "0", "ORL_NO_PROBE16": "1"})]
    o = _oracle(cluster)
    keys_of = lambda n1s: D._keys(tcd, np.array(n1s, np.uint64))  # noqa: E731
    fresh = [int(x) for x in np.concatenate([f.keys["n1"], D.control_keys(tcd, 8 * slots + 64)["n1"]])]  # never registered
    live, removed = [], []
    rng = np.random.default_rng(slots * 7 + len(name))
    next_act = [1]

    def insert(n1s, expect_refusal=False):
        n = len(n1s)
        keys = keys_of(n1s)
        acts = ((next_act[0] + np.arange(n)) % N_ACT).astype(np.uint32)
        next_act[0] += n
        silos = rng.integers(0, N_SILOS, n).astype(np.uint8)
        st_o = None
        for eng in engs:
            d_st = t.zeros(n, dtype=t.uint8, device="cuda")
            d_wa = t.zeros(n, dtype=t.int32, device="cuda")
            d_ws = t.zeros(n, dtype=t.uint8, device="cuda")
            if expect_refusal:
                with pytest.raises(OrleansRouteError) as e:
                    eng.register_single_activation_device(_dev(t, keys), _dev(t, acts), _dev(t, silos), n, d_st, d_wa, d_ws, stream=st_)
                assert e.value.code == L.E_CAPACITY
                continue
            eng.register_single_activation_device(_dev(t, keys), _dev(t, acts), _dev(t, silos), n, d_st, d_wa, d_ws, stream=st_)
            t.cuda.synchronize()
            if st_o is None:
                st_o, wa_o, ws_o = o.register(keys, acts, silos)
            np.testing.assert_array_equal(d_st.cpu().numpy(), st_o)
            np.testing.assert_array_equal(d_wa.cpu().numpy().view(np.uint32), wa_o)
            np.testing.assert_array_equal(d_ws.cpu().numpy(), ws_o)
        if expect_refusal:
            return 0
        new = list(dict.fromkeys(n1s))
        assert int((st_o == L.INS_INSERTED).sum()) == len(new)  # every key of a batch is absent before it
        live.extend(new)
        return len(new)

    def remove(n1s):
        keys = keys_of(n1s)
        rm_o = o.unregister(keys)
        for eng in engs:
            d_rm = t.zeros(len(keys), dtype=t.uint8, device="cuda")
            eng.unregister_device(_dev(t, keys), len(keys), d_rm, stream=st_)
            t.cuda.synchronize()
            np.testing.assert_array_equal(d_rm.cpu().numpy(), rm_o)
        return int(rm_o.sum())

    def batch_of(n):
        """n keys: a third one key under different handles, a third removed keys again, the rest never registered."""
        n_dup = n // 3
        n_re = min(n // 3, len(removed))
        n1s = [removed.pop(int(rng.integers(0, len(removed)))) for _ in range(n_re)]
        n1s += [fresh.pop(0) for _ in range(n - n_dup - n_re)]
        n1s += [n1s[0]] * n_dup
        return [n1s[i] for i in rng.permutation(n)]

    def routes(tag, device_built=False):
        kinds = {"hit": keys_of(live), "removed": keys_of(removed), "ghost": f.ghosts, "alias": f.aliases}
        for n in (1, 4097):
            msgs, _, _ = _batch(kinds, n, seed=slots + n)
            got = [_route_equal(eng, o, msgs) for eng in engs]
            for x, y in zip(*got):
                np.testing.assert_array_equal(x, y, err_msg=tag)
        if device_built:
            assert engs[0].query(L.Q_PROBE_FORM) == 17, tag
        assert engs[1].query(L.Q_PROBE_FORM) == 32
        for eng in engs:
            assert eng.directory_count() == o.size() == len(live), tag

    # the type list: one key from the host, routed through the host-built 8-B table
    seed_key = fresh.pop(0)
    for eng in engs:
        st = eng.register_single_activation(keys_of([seed_key]), np.zeros(1, np.uint32), np.zeros(1, np.uint8))[0]
        assert st[0] == L.INS_INSERTED
    o.register(keys_of([seed_key]), np.zeros(1, np.uint32), np.zeros(1, np.uint8))
    live.append(seed_key)
    routes("seed")
    assert engs[0].query(L.Q_PROBE_FORM) == 8
    # fill to exactly half load on the device: no tombstones yet, every batch is the largest that fits
    while len(live) * 2 < slots:
        n = _largest_fit(slots, len(live), 0)
        assert n == slots // 2 - len(live)
        insert(batch_of(n))
        routes("fill", device_built=True)
    assert len(live) * 2 == slots
    t_lo = t_hi = 0
    refused = False
    for rnd in range(64):
        count = len(live)
        if count:  # half of the live keys out (one of them twice, and a ghost that is not there), in one device batch
            out = [live.pop(int(rng.integers(0, len(live)))) for _ in range((count + 1) // 2)]
            assert remove(out + out[:1] + [int(f.ghosts["n1"][0])]) == len(out)
            removed += out
            t_lo, t_hi, count = t_lo + len(out), t_hi + len(out), count - len(out)
        assert t_lo == slots // 2 - count
        half = slots // 2 - count
        if _largest_fit(slots, count, t_lo) < half:
            # 7/8 binds even with the fewest tombstones the table can hold: one message more than that is refused,
            # though the half-load rule alone would take it
            n = _largest_fit(slots, count, t_lo) + 1
            assert (count + n) * 2 <= slots and not _fits(slots, count, t_lo, n)
            before = (list(removed), list(fresh))
            insert(batch_of(n), expect_refusal=True)
            removed[:], fresh[:] = before
            refused = True
            routes("after the refusal", device_built=slots > 2)
            for eng in engs:
                eng.compact_directory()
            routes("after the compaction")
            n = _largest_fit(slots, count, 0)  # the compacted table has no tombstones: the rule is exact again
            assert n == half > 0
            insert(batch_of(n))
            routes("after the last device round")
            # the mirror is re-read after device mutations: a host registration of a live key and, where the host rule
            # (count + tombstones + 1) * 2 <= slots allows one, of an absent key (no tombstones since the compaction)
            hk = [live[-1]] + ([removed[0]] if (len(live) + 1) * 2 <= slots and removed else [])
            ha = np.arange(len(hk), dtype=np.uint32) + 77
            hs = np.zeros(len(hk), np.uint8)
            st_o, wa_o, _ = o.register(keys_of(hk), ha, hs)
            for eng in engs:
                st_h, wa_h, _ = eng.register_single_activation(keys_of(hk), ha, hs)
                np.testing.assert_array_equal(st_h, st_o)
                np.testing.assert_array_equal(wa_h, wa_o)
            assert st_o[0] == L.INS_EXISTING
            if len(hk) > 1:
                assert st_o[1] == L.INS_INSERTED
                live.append(removed.pop(0))
            routes("after the host registration")
            break
        n = _largest_fit(slots, count, t_hi)
        if n:
            t_lo = max(0, t_lo - insert(batch_of(n)))
        routes(f"round {rnd}", device_built=slots > 2)
    assert refused, "no insert was refused for entries + tombstones passing 7/8"
    for eng in engs:
        eng.close()


@pytest.mark.parametrize("slots", [64, 4096])
@pytest.mark.parametrize("name", ["tail(4)", "random"])
def test_split_and_merge_on_crowded_table(torch, cluster, slots, name):
    """Scenario d.  A half-loaded table of silo 0 (the ring's only silo), then silo 1 joins with a hash that takes about
    half of the family: split_directory_device(remove=True) emits exactly the entries silo 1 now owns, in slot order,
    and tombstones them here across the wrap; the rest still routes like the oracle.  That copy is then merged
    (merge_directory_device) into a second table that is crowded with half of the same grains under other activations
    and with ghosts of the same start slots: statuses and dropped activations equal pyref.Partition.merge, and the whole
    table read back equals its partition."""
    t = torch
    tcd = W.grain_tcd(cluster)
    f = D.family(name, slots, tcd)
    f.check()
    m = len(f.keys)
    st_ = t.cuda.current_stream().cuda_stream
    h0 = int(cluster.hashes[0])
    kh = np.sort(W.jenkins3_np(f.keys["tcd"], f.keys["n0"], f.keys["n1"]).view(np.int32))
    msgs = D.messages(f.keys, 1)

    def oracle2(h1):
        o = cpu_ref.Oracle(2, seed=0)
        o.add_server(0, h0)
        o.add_server(1, h1)
        return o

    moved_by = {int(h): int((decode_route(oracle2(int(h)).route(msgs)[0]).owner == 1).sum()) for h in kh[:: max(1, m // 16)]
                if int(h) != h0}
    h1 = min(moved_by, key=lambda h: abs(moved_by[h] - m // 2))
    assert 4 <= moved_by[h1] <= m - 4, moved_by
    eng_a = GrainDirectoryEngine(n_act=N_ACT, dir_capacity=slots // 2, max_batch=MAX_BATCH, device=0)
    eng_a.set_silos(2, local=[1, 0], seed=0)
    eng_a.add_server(0, h0)
    acts = np.arange(m, dtype=np.uint32) + 10
    silos = np.zeros(m, np.uint8)
    st, _, _ = eng_a.register_single_activation(f.keys, acts, silos)
    assert (st == L.INS_INSERTED).all() and eng_a.directory_count() * 2 == slots
    eng_a.add_server(1, h1)
    o8 = oracle2(h1)
    moved = decode_route(o8.route(msgs)[0]).owner == 1
    assert moved.sum() == moved_by[h1]
    d_k = t.empty((m, 24), dtype=t.uint8, device="cuda")
    d_a = t.empty(m, dtype=t.int32, device="cuda")
    d_s = t.empty(m, dtype=t.uint8, device="cuda")
    d_n = t.zeros(1, dtype=t.int64, device="cuda")
    eng_a.split_directory_device(0, d_k, d_a, d_s, m, d_n, remove=True, stream=st_)
    t.cuda.synchronize()
    n_out = int(d_n.item())
    assert n_out == moved.sum()
    got_k = d_k[:n_out].cpu().numpy().reshape(-1).view(L.KEY_DTYPE)
    got_a = d_a[:n_out].cpu().numpy().view(np.uint32)
    assert sorted(got_a.tolist()) == sorted(acts[moved].tolist())
    np.testing.assert_array_equal(got_k, f.keys[got_a.astype(np.int64) - 10])
    assert (d_s[:n_out].cpu().numpy() == 0).all()
    assert eng_a.directory_count() == m - n_out
    a_h, s_h = eng_a.lookup_host(f.keys)
    np.testing.assert_array_equal(a_h, np.where(moved, L.NO_ACT, acts).astype(np.uint32))
    # silo 0's view: its own grains hit, the moved ones have a remote owner; ghosts of the same slots are placed
    local = [1, 0] + [0] * 254
    o_a = cpu_ref.Oracle(2, local=local, seed=0)
    o_a.add_server(0, h0)
    o_a.add_server(1, h1)
    o_a.register(f.keys[~moved], acts[~moved], silos[~moved])
    probe = D.messages(np.concatenate([f.keys, f.ghosts, f.aliases]), 1)
    res = eng_a.address_messages(probe)
    r_ref, a_ref = o_a.route(probe)
    np.testing.assert_array_equal(res.route, r_ref)
    np.testing.assert_array_equal(res.act, a_ref)
    assert (decode_route(r_ref).status == L.ST_HIT).sum() == m - n_out
    eng_a.close()
    # the copy merged into a second crowded table
    rng = np.random.default_rng(slots)
    ak = np.zeros(N_ACT, L.KEY_DTYPE)
    ak["tcd"] = rng.integers(0, 3, N_ACT).astype(np.uint64)
    ak["n0"] = rng.integers(0, 4, N_ACT).astype(np.uint64)
    ak["n1"] = rng.integers(0, 1 << 62, N_ACT, dtype=np.uint64)
    akey = lambda a: (int(ak["tcd"][a]), int(ak["n0"][a]), int(ak["n1"][a]))  # noqa: E731
    eng_b = _engine(cluster, slots)
    part = P.Partition()
    mk = f.keys[moved]
    pre = np.concatenate([mk[::2], f.ghosts])[: m - n_out]
    pre_a = rng.integers(0, N_ACT, len(pre)).astype(np.uint32)
    pre_a[0] = got_a[np.nonzero(got_k["n1"] == pre["n1"][0])[0][0]]  # the same activation on both sides
    pre_s = rng.integers(0, N_SILOS, len(pre)).astype(np.uint8)
    d_ak = _dev(t, ak)

    def merge(keys, acts_, silos_):
        n = len(keys)
        d_st = t.empty(n, dtype=t.uint8, device="cuda")
        d_da = t.empty(n, dtype=t.int32, device="cuda")
        d_ds = t.empty(n, dtype=t.uint8, device="cuda")
        eng_b.merge_directory_device(_dev(t, keys), _dev(t, acts_), _dev(t, silos_), n, d_ak, N_ACT, d_st, d_da, d_ds, stream=st_)
        t.cuda.synchronize()
        exp = part.merge([(P.Key(int(k["tcd"]), int(k["n0"]), int(k["n1"])), int(a), int(s)) for k, a, s in zip(keys, acts_, silos_)], akey)
        np.testing.assert_array_equal(d_st.cpu().numpy(), [e[0] for e in exp])
        np.testing.assert_array_equal(d_da.cpu().numpy().view(np.uint32), [e[1] for e in exp])
        np.testing.assert_array_equal(d_ds.cpu().numpy(), [e[2] for e in exp])
        return d_st.cpu().numpy()

    assert (merge(pre, pre_a, pre_s) == L.MERGE_INSERTED).all()
    st = merge(got_k, got_a, np.zeros(n_out, np.uint8))
    assert (st == L.MERGE_INSERTED).sum() >= n_out // 2 - len(f.ghosts) and (st == L.MERGE_SAME).sum() >= 1
    assert ((st == L.MERGE_KEPT) | (st == L.MERGE_REPLACED)).sum() >= 1
    everything = np.concatenate([f.keys, f.ghosts, f.aliases])
    a_h, s_h = eng_b.lookup_host(everything)
    for g, k in enumerate(everything):
        r = part.data.get((int(k["tcd"]), int(k["n0"]), int(k["n1"]), None))
        assert (int(a_h[g]), int(s_h[g])) == (r if r is not None else (L.NO_ACT, 0xFF)), g
    assert eng_b.directory_count() == len(part.data) <= slots // 2
    eng_b.close()


@pytest.mark.parametrize("name", D.keyext_family_names())
def test_keyext_table_clustered_extensions(torch, cluster, name):
    """Scenario e.  The KeyExt table at its initial size (1024 slots: orl_api.cpp ext_rebuild; see dir_layout) with the
    extensions "k%d" of one grain clustered by their KeyExt hash: a host registration of half the family, a device
    registration of all of it with duplicates in the batch (first writer wins), a host removal of every third key, a
    second device batch that registers the removed keys again among existing ones, and address_keyext_device over
    registered, removed and ghost extensions after every step — statuses, winners, lookups, the count and the routed
    batch (with its stable bucketing) equal pyref's restatement."""
    t = torch
    tcd = W.grain_tcd(cluster, L.CAT_KEYEXT_GRAIN)
    reg, ghosts, start = D.keyext_family(name, tcd)
    n1 = 7
    ring = P.Ring()
    for s in range(N_SILOS):
        ring.add_server(s, int(cluster.hashes[s]))
    view = P.SiloView(running=[True] * N_SILOS, functional=[True] * N_SILOS, local=[True] * N_SILOS)
    part = P.Partition()
    eng = _engine(cluster, 64)
    key = lambda x: P.Key(tcd, 0, n1, x)  # noqa: E731
    assert D.dir_slot_np(np.array([P.uniform_hash(key(reg[0]))], np.uint32), D.KEYEXT_SLOTS)[0] == start[0]
    karr = lambda exts: np.array([(tcd, 0, n1)] * len(exts), L.KEY_DTYPE)  # noqa: E731
    act_of = {x: 100 + i for i, x in enumerate(reg + ghosts)}

    def check(got, exp):
        st, wa, ws = got
        np.testing.assert_array_equal(st, np.array([e[0] for e in exp], np.uint8))
        np.testing.assert_array_equal(wa, np.array([e[1] for e in exp], np.uint32))
        np.testing.assert_array_equal(ws, np.array([e[2] for e in exp], np.uint8))

    def host_insert(exts, bump):
        acts = np.array([act_of[x] + bump for x in exts], np.uint32)
        silos = (acts % N_SILOS).astype(np.uint8)
        check(eng.register_keyext(karr(exts), exts, acts, silos),
              [P.register_keyext(ring, part, view, key(x), int(a), int(s)) for x, a, s in zip(exts, acts, silos)])

    def dev_insert(exts, bump):
        n = len(exts)
        acts = np.array([act_of[x] + bump + i for i, x in enumerate(exts)], np.uint32)
        silos = (acts % N_SILOS).astype(np.uint8)
        ref, blob = GrainDirectoryEngine.ext_blob(exts)
        d_st, d_wa, d_ws = (t.zeros(n, dtype=t.uint8, device="cuda"), t.zeros(n, dtype=t.int32, device="cuda"),
                            t.zeros(n, dtype=t.uint8, device="cuda"))
        eng.register_keyext_device(_dev(t, karr(exts)), _dev(t, ref), _dev(t, blob), len(blob), _dev(t, acts), _dev(t, silos), n,
                                   d_st, d_wa, d_ws, stream=t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        exp = [P.register_keyext(ring, part, view, key(x), int(a), int(s)) for x, a, s in zip(exts, acts, silos)]
        check((d_st.cpu().numpy(), d_wa.cpu().numpy().view(np.uint32), d_ws.cpu().numpy()), exp)
        return d_st.cpu().numpy()

    def route():
        exts = reg + ghosts + reg[::-1]
        n = len(exts)
        msgs = [P.Msg(key(x), i % N_SILOS) for i, x in enumerate(exts)]
        h = np.zeros(n, L.MSG_DTYPE)
        h["tcd"], h["n1"], h["category"], h["target_silo"] = tcd, n1, 2, 0xFF
        h["sending_silo"] = [m_.sending_silo for m_ in msgs]
        ref, blob = GrainDirectoryEngine.ext_blob(exts)
        outs = [t.empty(n, dtype=t.int32, device="cuda") for _ in range(3)] + [t.empty(N_ACT + 2, dtype=t.int32, device="cuda")]
        eng.address_keyext_device(t.from_numpy(h.view(np.int32).reshape(-1, 8)).cuda(), n, t.from_numpy(ref.view(np.int32)).cuda(),
                                  t.from_numpy(blob).cuda(), len(blob), *outs, stream=t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        er, ea = P.route_batch(msgs, ring, part, view, keyext_directory=True)
        er, ea = np.array(er, np.uint32), np.array(ea, np.uint32)
        np.testing.assert_array_equal(outs[0].cpu().numpy().view(np.uint32), er)
        np.testing.assert_array_equal(outs[1].cpu().numpy().view(np.uint32), ea)
        eo, ef = cpu_ref.Oracle(N_SILOS).bucket(ea, N_ACT)
        np.testing.assert_array_equal(outs[2].cpu().numpy().view(np.uint32), eo)
        np.testing.assert_array_equal(outs[3].cpu().numpy().view(np.uint32), ef)
        a_h, s_h = eng.lookup_keyext_host(karr(exts), exts)
        for i, x in enumerate(exts):
            r = part.data.get(P.Partition._k(key(x)))
            assert (a_h[i], s_h[i]) == ((r[0], r[1]) if r else (L.NO_ACT, 0xFF)), x
        assert eng.keyext_count() == len(part.data)
        status = (er >> 16) & 0xFF
        return int((status == L.ST_HIT).sum()), int((status == L.ST_NEW_PLACEMENT).sum())

    host_insert(reg[::2], 0)
    assert route() == (2 * len(reg[::2]), len(ghosts) + 2 * (len(reg) - len(reg[::2])))
    st = dev_insert(reg + reg[1::2][:5] + reg[:3], 1000)
    assert (st == L.INS_INSERTED).sum() == len(reg) - len(reg[::2]) and (st == L.INS_EXISTING).sum() == len(reg[::2]) + 8
    assert route() == (2 * len(reg), len(ghosts))
    gone = reg[::3]
    rm = eng.unregister_keyext(karr(gone + ghosts[:1]), gone + ghosts[:1])
    assert [bool(x) for x in rm] == [part.remove(key(x)) for x in gone + ghosts[:1]] == [True] * len(gone) + [False]
    assert route() == (2 * (len(reg) - len(gone)), len(ghosts) + 2 * len(gone))
    st = dev_insert(gone[::-1] + reg[:7] + gone[:2], 3000)
    assert (st == L.INS_INSERTED).sum() == len(gone)
    assert route() == (2 * len(reg), len(ghosts))
    eng.close()
