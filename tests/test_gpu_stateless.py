"""GPU parity of stateless-worker routing: the SW forms of k_route / k_part_lb and the busy-bit kernel, bit for bit
against tests/stateless_ref.py (StatelessWorkerDirector.cs:35-80 over the directory oracle).  All integer work: exact
equality, no tolerance."""
import numpy as np
import pytest

import node_replay as R
import stateless_ref as S
from oracle import cpu_ref
from orleans_amd import _lib as L
from orleans_amd import workloads as W
from orleans_amd.engine import GrainDirectoryEngine, decode_route
from orleans_amd.node import GrainNode, narrow_records_to_headers, wire_records_to_headers

pytestmark = pytest.mark.gpu

T1 = (L.CAT_GRAIN << 56) | 0x101  # MaxLocal 1
T4 = (L.CAT_GRAIN << 56) | 0x104  # MaxLocal 4
TYPES = {T1: 1, T4: 4}
N_SW = 300        # stateless-worker grains: n1 = 0..149 of each type
N_DIR = 20_000    # directory grains, as test_gpu_parity._random_setup builds them
SEED = 29         # chosen on the CPU so that the 8-silo batches of >= 4097 messages hold every case (_coverage)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def sw_keys():
    k = np.zeros(N_SW, L.KEY_DTYPE)
    k["tcd"] = np.where(np.arange(N_SW) < N_SW // 2, np.uint64(T1), np.uint64(T4))
    k["n1"] = np.arange(N_SW) % (N_SW // 2)
    return k


def fill_catalog(eng, cat, n_act, n_silos, seed, silos=None):
    """Entries of the N_SW grains on about half the silos each: 1..MaxLocal distinct handles, half of the lists all busy,
    the others with random busy bits — the same calls on the library (when given) and on the LocalCatalog."""
    rng = np.random.default_rng(seed)
    keys = sw_keys()
    silos = list(range(n_silos)) if silos is None else list(silos)
    ak, aa, asl, bk, ba, bs, bb = [], [], [], [], [], [], []
    for g in range(N_SW):
        maxl = TYPES[int(keys["tcd"][g])]
        for s in silos:
            if rng.random() < 0.5 and len(silos) > 1 and g != 0:  # grain 0 (the hot one) has an entry everywhere
                continue
            cnt = int(rng.integers(1, min(maxl, n_act) + 1))
            acts = rng.choice(n_act, cnt, replace=False)
            busy = np.ones(cnt, bool) if rng.random() < 0.5 else rng.random(cnt) < 0.5
            for a, b in zip(acts, busy):
                ak.append(g), aa.append(a), asl.append(s)
                if b:
                    bk.append(g), ba.append(a), bs.append(s), bb.append(1)
    ak, bk = np.array(ak, np.int64), np.array(bk, np.int64)
    aa, asl = np.array(aa, np.uint32), np.array(asl, np.uint8)
    ba, bs, bb = np.array(ba, np.uint32), np.array(bs, np.uint8), np.array(bb, np.uint8)
    for i in range(len(ak)):
        assert cat.add(keys[ak[i]], int(aa[i]), int(asl[i])) == L.SW_ADDED
    for i in range(len(bk)):
        assert cat.set_busy(keys[bk[i]], int(ba[i]), int(bs[i]), True)
    if eng is not None:
        assert (eng.stateless_add(keys[ak], aa, asl) == L.SW_ADDED).all()
        assert eng.stateless_set_busy(keys[bk], ba, bs, bb).all()
    return keys


def setup(n_act, n_silos, policy, running, device=0):
    """_random_setup's population (20 000 directory grains, 90 % registered) + the stateless-worker types and catalog;
    every fourth T4 grain is also registered in the directory (the SW path must not look there)."""
    cl = W.default_cluster(n_silos)
    eng = GrainDirectoryEngine(n_act=n_act, dir_capacity=N_DIR + N_SW, max_batch=1 << 17, device=device, placement=policy)
    eng.set_silos(n_silos, running=running, seed=0)
    o = cpu_ref.Oracle(n_silos, running=running, seed=0, policy=policy)
    for s in range(n_silos):
        eng.add_server(s, int(cl.hashes[s]))
        o.add_server(s, int(cl.hashes[s]))
    keys, uni, owner, reg = W.grain_population(cl, N_DIR, 0.9, 11)
    rng = np.random.default_rng(11)
    acts = rng.integers(0, n_act, N_DIR).astype(np.uint32)
    silos = np.where(rng.random(N_DIR) < 0.8, owner, rng.integers(0, n_silos, N_DIR)).astype(np.uint8)
    idx = np.nonzero(reg)[0]
    swk = sw_keys()
    both = swk[N_SW // 2::4]
    rk = np.concatenate([keys[idx], both])
    ra = np.concatenate([acts[idx], rng.integers(0, n_act, len(both)).astype(np.uint32)])
    rs = np.concatenate([silos[idx], cl.owner_of(W.jenkins3_np(both["tcd"], both["n0"], both["n1"])).astype(np.uint8)])
    st_e, _, _ = eng.register_single_activation(rk, ra, rs)
    st_o, _, _ = o.register(rk, ra, rs)
    np.testing.assert_array_equal(st_e, st_o)
    eng.set_stateless_types(list(TYPES), list(TYPES.values()))
    eng.stateless_config(N_SW * n_silos)
    eng.set_wire_types([W.grain_tcd(cl), T1, T4])
    cat = S.LocalCatalog(TYPES, n_act, n_silos)
    fill_catalog(eng, cat, n_act, n_silos, SEED)
    return cl, eng, o, cat


def messages(cl, n, seed):
    """About 60 % directory messages (~9 % of them to never-registered grains), 40 % to the stateless-worker grains: one
    hot grain gets n/8, 3 % of them carry a complete address, 10 % a precomputed hash of the sender's choosing."""
    m = W.uniform_messages(cl, N_DIR + 2000, n, seed=seed)
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    sw = np.nonzero(u < 0.4)[0]
    g = rng.integers(0, N_SW, len(sw))
    g[rng.random(len(sw)) < 0.125 / 0.4] = 0
    k = sw_keys()[g]
    m["tcd"][sw], m["n1"][sw] = k["tcd"], k["n1"]
    v = rng.random(len(sw))
    done = sw[v < 0.03]
    m["flags"][done] = L.HDR_ADDRESS_COMPLETE
    m["target_silo"][done] = rng.integers(0, cl.n_silos, len(done))
    hv = sw[(v >= 0.03) & (v < 0.13)]
    m["flags"][hv] = L.HDR_HASH_VALID
    m["aux"][hv] = rng.integers(0, 1 << 32, len(hv), dtype=np.uint64).astype(np.uint32)
    return m


def coverage(cat, o, msgs, r, a):
    """The cases the reference's own output holds for this batch."""
    got = set()
    sw = S.listed(msgs, TYPES)
    fl = (r >> 24) & 0xFF
    assert (((fl & L.RF_STATELESS) != 0) == sw).all()
    assert (((r[sw] >> 16) & 0xFF) != L.ST_OWNER_NULL).all() and ((r[sw] & 0xFF) == 0xFF).all()
    reg_dir = {(int(k["tcd"]), int(k["n1"])) for k in sw_keys()[N_SW // 2::4]}
    for i in np.nonzero(sw)[0]:
        row = S.row_of(cat, msgs[i])
        got.add(row)
        lst = cat.lookup(msgs[i], int(msgs["sending_silo"][i]))
        if row == "idle" and lst[0][1]:
            got.add("idle_later")
        if row == "absent" and any(cat.lookup(msgs[i], s) for s in range(cat.n_silos)):
            got.add("other_silo_only")
        if row == "fullN" and msgs["flags"][i] & L.HDR_HASH_VALID:
            got.add("fullN_hash_valid")
        if (int(msgs["tcd"][i]), int(msgs["n1"][i])) in reg_dir:
            got.add("also_in_directory")
    if (np.isin(msgs["tcd"], np.array(list(TYPES), np.uint64)) & ((msgs["flags"] & L.HDR_ADDRESS_COMPLETE) != 0)).any():
        got.add("complete_listed")
    return got


ALL_CASES = {"absent", "idle", "full1", "fullN", "grow", "idle_later", "other_silo_only", "fullN_hash_valid",
             "also_in_directory", "complete_listed"}


def _dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()


def _route_device(t, eng, fn, recs, n, n_act):
    d = _dev(t, recs)
    route, act, order = (t.empty(max(n, 1), dtype=t.int32, device="cuda") for _ in range(3))
    off = t.empty(n_act + 2, dtype=t.int32, device="cuda")
    fn(d, n, route, act, order, off, stream=t.cuda.current_stream().cuda_stream)
    t.cuda.synchronize()
    return tuple(x.cpu().numpy().view(np.uint32)[:k] for x, k in ((route, n), (act, n), (order, n), (off, n_act + 2)))


def _check_forms(t, eng, o, cat, msgs, n_act, opts, tag):
    r, a = S.route(o, cat, TYPES, msgs, opts)
    order, off = o.bucket(a, n_act)
    res = eng.address_messages(msgs, opts)
    for name, got, want in (("route", res.route, r), ("act", res.act, a), ("order", res.order, order),
                            ("offsets", res.offsets, off)):
        np.testing.assert_array_equal(got, want, err_msg=f"{tag} host form {name}")
    n = len(msgs)
    fn = lambda *x, **kw: eng.address_messages_device(*x, opts=opts, **kw)  # noqa: E731
    for name, got, want in zip(("route", "act", "order", "offsets"), _route_device(t, eng, fn, msgs, n, n_act),
                               (r, a, order, off)):
        np.testing.assert_array_equal(got, want, err_msg=f"{tag} device form {name}")
    # the exchange records, for the messages that have each form (the decoded record is what the kernel routes)
    rec16, ok16 = cpu_ref.wire_encode(msgs)
    rec8, ok8 = cpu_ref.narrow_encode(msgs, eng.wire_types)
    for width, recs, ok, back, fn in (
            (16, rec16, ok16, wire_records_to_headers, lambda *x, **kw: eng.address_compact_device(*x, opts=opts, **kw)),
            (8, rec8, ok8, lambda raw: narrow_records_to_headers(raw, eng.wire_types),
             lambda *x, **kw: eng.address_narrow_device(*x, opts=opts, **kw))):
        sub = np.ascontiguousarray(recs[ok])
        if len(sub) == 0:
            continue
        hdr = back(sub.view(np.uint8).reshape(-1))
        assert S.listed(hdr, TYPES).sum() == (S.listed(msgs, TYPES) & ok).sum()
        rw, aw = S.route(o, cat, TYPES, hdr, opts)
        ow, fw = o.bucket(aw, n_act)
        for name, got, want in zip(("route", "act", "order", "offsets"), _route_device(t, eng, fn, sub, len(sub), n_act),
                                   (rw, aw, ow, fw)):
            np.testing.assert_array_equal(got, want, err_msg=f"{tag} {width}-B form {name}")
    return r, a


@pytest.mark.parametrize("n", [1, 63, 4097, 65_553])
@pytest.mark.parametrize("n_act", [5, 5000, 3_000_000])
def test_stateless_batches_vs_reference(torch, n, n_act):
    """Route, act, order and offsets of every entry form, for 8 silos with both placement policies and 1 silo, with opts 0
    and EXCLUDE_IF_STOPPING while one sender is not running.  n_act 5 has no fused histogram, 5000 the two-level plan's,
    3 000 000 the LSD plan's; n covers one lane, a partial wave, a tile + 1 and 16 tiles + 17."""
    for n_silos, policy in ((8, L.POLICY_PREFER_LOCAL), (8, L.POLICY_HASH_SPREAD), (1, L.POLICY_PREFER_LOCAL)):
        running = [1, 1, 1, 0, 1, 1, 1, 1][:n_silos] if n_silos > 1 else [0]
        cl, eng, o, cat = setup(n_act, n_silos, policy, running)
        msgs = messages(cl, n, seed=n * 7 + n_act)
        for opts in (0, L.OPT_EXCLUDE_IF_STOPPING):
            r, a = S.route(o, cat, TYPES, msgs, opts)
            cases = coverage(cat, o, msgs, r, a)
            if n_silos == 8 and n >= 4097:  # before any GPU comparison: the reference's output holds every case
                assert cases == ALL_CASES, ALL_CASES - cases
            _check_forms(torch, eng, o, cat, msgs, n_act, opts, f"silos={n_silos} policy={policy} opts={opts}")
        eng.close()


def test_busy_bits_on_device_change_the_next_batch(torch):
    t = torch
    n_act = 5000
    cl, eng, o, cat = setup(n_act, 8, L.POLICY_PREFER_LOCAL, None)
    msgs = messages(cl, 20_001, seed=5)
    r0, a0 = _check_forms(t, eng, o, cat, msgs, n_act, 0, "before")
    # flip the busy bit of every third catalog activation (one value per activation), plus a few the catalog lacks
    rng = np.random.default_rng(9)
    items = [(k, a, not b) for k, lst in sorted(cat.lists.items()) for a, b in lst][::3]
    keys = np.zeros(len(items) + 5, L.KEY_DTYPE)
    acts, silos, busy = (np.zeros(len(keys), d) for d in (np.uint32, np.uint8, np.uint8))
    for i, ((tcd, n0, n1, s), a, b) in enumerate(items):
        keys[i] = (tcd, n0, n1)
        acts[i], silos[i], busy[i] = a, s, b
    keys["tcd"][len(items):], keys["n1"][len(items):] = T4, 100_000 + np.arange(5)
    found = t.zeros(len(keys), dtype=t.uint8, device="cuda")
    eng.stateless_set_busy_device(_dev(t, keys), _dev(t, acts), _dev(t, silos), _dev(t, busy), len(keys), found,
                                  stream=t.cuda.current_stream().cuda_stream)
    want = [int(cat.set_busy(keys[i], int(acts[i]), int(silos[i]), bool(busy[i]))) for i in range(len(keys))]
    r1, a1 = _check_forms(t, eng, o, cat, msgs, n_act, 0, "after")
    assert found.cpu().numpy().tolist() == want and sum(want) == len(items)
    assert (r0 != r1).sum() > 100 and (a0 != a1).sum() > 100  # the answers changed accordingly
    # the host mirror is re-read from the device on its next use
    gk = np.repeat(sw_keys(), 8)
    gs = np.tile(np.arange(8, dtype=np.uint8), N_SW)
    cnt, la, lb = eng.stateless_lookup(gk, gs)
    for i in rng.choice(len(gk), 400, replace=False):
        lst = cat.lookup(gk[i], int(gs[i]))
        assert (cnt[i], list(la[i][:cnt[i]]), lb[i]) == (len(lst), [x for x, _ in lst],
                                                        sum(1 << j for j, (_, b) in enumerate(lst) if b))
    # and a host change after it reaches the next batch
    k0 = sw_keys()[:1]
    lst = cat.lookup(k0[0], 2)
    eng.stateless_remove(np.repeat(k0, len(lst)), [x for x, _ in lst], np.full(len(lst), 2, np.uint8))
    for x, _ in lst:
        cat.remove(k0[0], x, 2)
    _check_forms(t, eng, o, cat, msgs, n_act, 0, "after host removal")
    eng.close()


def test_catalog_at_capacity_with_tombstones(torch):
    """The catalog filled to its limit (load 1/2: the longest chains it can have), half of the entries removed (tombstones
    on the chains), then refilled to the limit with other grains."""
    t = torch
    n_act, cap = 5000, 2048
    cl = W.default_cluster(8)
    eng = GrainDirectoryEngine(n_act=n_act, dir_capacity=64, max_batch=1 << 17, device=0)
    W.setup_engine(eng, cl)
    o = cpu_ref.Oracle(8, seed=0)
    for s in range(8):
        o.add_server(s, int(cl.hashes[s]))
    eng.set_stateless_types(list(TYPES), list(TYPES.values()))
    eng.stateless_config(cap)
    eng.set_wire_types([T1, T4])
    cat = S.LocalCatalog(TYPES, n_act, 8)
    rng = np.random.default_rng(3)
    keys = np.zeros(cap, L.KEY_DTYPE)
    keys["tcd"], keys["n1"] = T4, np.arange(cap) // 8
    silos = (np.arange(cap) % 8).astype(np.uint8)
    acts = rng.integers(0, n_act, cap).astype(np.uint32)
    assert (eng.stateless_add(keys, acts, silos) == L.SW_ADDED).all() and eng.stateless_count() == cap
    for i in range(cap):
        cat.add(keys[i], int(acts[i]), int(silos[i]))
    m = np.zeros(30_000, L.MSG_DTYPE)
    m["tcd"], m["category"] = T4, 2
    m["n1"] = rng.integers(0, cap // 8 + 300, len(m))  # some grains never had an entry; 256..555 come in the refill
    m["sending_silo"] = rng.integers(0, 8, len(m))
    _check_forms(t, eng, o, cat, m, n_act, 0, "full")
    gone = rng.permutation(cap)[:cap // 2]
    assert eng.stateless_remove(keys[gone], acts[gone], silos[gone]).all() and eng.stateless_count() == cap // 2
    for i in gone:
        cat.remove(keys[i], int(acts[i]), int(silos[i]))
    r, a = _check_forms(t, eng, o, cat, m, n_act, 0, "half removed")
    st = (r >> 16) & 0xFF
    assert (st == L.ST_HIT).sum() > 5000 and (st == L.ST_NEW_PLACEMENT).sum() > 5000
    k2 = np.zeros(cap // 2, L.KEY_DTYPE)
    k2["tcd"], k2["n1"] = T4, cap // 8 + np.arange(cap // 2) // 8
    s2 = (np.arange(cap // 2) % 8).astype(np.uint8)
    a2 = rng.integers(0, n_act, cap // 2).astype(np.uint32)
    assert (eng.stateless_add(k2, a2, s2) == L.SW_ADDED).all() and eng.stateless_count() == cap
    for i in range(cap // 2):
        cat.add(k2[i], int(a2[i]), int(s2[i]))
    _check_forms(t, eng, o, cat, m, n_act, 0, "refilled")
    eng.close()


@pytest.mark.parametrize("n_act", [5000, 3_000_000])
def test_types_set_without_such_messages_changes_nothing(torch, n_act):
    """With types set but no message of those types, every output equals that of the same context with types unset."""
    cl, eng, o, cat = setup(n_act, 8, L.POLICY_HASH_SPREAD, [1, 1, 1, 0, 1, 1, 1, 1])
    msgs = W.uniform_messages(cl, N_DIR + 2000, 50_001, seed=77)
    msgs["flags"][::50] = L.HDR_ADDRESS_COMPLETE
    with_types = [eng.address_messages(msgs, opts) for opts in (0, L.OPT_EXCLUDE_IF_STOPPING)]
    eng.set_stateless_types([], [])
    for opts, w in zip((0, L.OPT_EXCLUDE_IF_STOPPING), with_types):
        res = eng.address_messages(msgs, opts)
        r, a = o.route(msgs, opts)
        for name in ("route", "act", "order", "offsets"):
            np.testing.assert_array_equal(getattr(w, name), getattr(res, name), err_msg=name)
        np.testing.assert_array_equal(res.route, r)
        np.testing.assert_array_equal(res.act, a)
    eng.close()


# ---- the node exchange (LOCAL transport) ------------------------------------------------------------------------------
def _node_world(t, nranks, host_mix, wire, ros):
    from test_gpu_node import World
    world = World(nranks, n_grains=20_000, host_mix=host_mix, ros=ros, max_batch=1 << 18)  # >= the nodes' max_recv
    if wire == "both":  # the 8-B form for the stateless-worker types too (the same list on every rank)
        base = R.wire_types(world.p, "both")[0]
        for e in world.engs:
            e.set_wire_types(base + [T1, T4])
    cats = []
    for r, e in enumerate(world.engs):
        e.set_stateless_types(list(TYPES), list(TYPES.values()))
        e.stateless_config(N_SW * 8)
        cat = S.LocalCatalog(TYPES, world.n_act, 8)
        # each rank's catalog holds its own silos' lists, and a few foreign ones that nothing may read
        own = np.nonzero(world.ros == r)[0].tolist()
        fill_catalog(e, cat, world.n_act, 8, SEED + r, silos=own + [int(np.nonzero(world.ros != r)[0][0])])
        cats.append(cat)
    return world, cats


def _node_batch(world, rank, n, seed):
    m = world.messages(rank, n, seed)
    rng = np.random.default_rng(seed + 1000)
    sw = np.nonzero(rng.random(n) < 0.10)[0]
    k = sw_keys()[rng.integers(0, N_SW, len(sw))]
    m["tcd"][sw], m["n0"][sw], m["n1"][sw] = k["tcd"], 0, k["n1"]
    return m


@pytest.mark.parametrize("nranks,chunks,host_mix,wire,cache", [(2, 2, 0.3, None, False), (3, 3, 0.3, "both", False),
                                                               (3, 3, 0.3, "both", True)])
def test_node_stateless_vs_reference(torch, nranks, chunks, host_mix, wire, cache):
    """About 10 % of every rank's batch goes to stateless-worker grains: they stay in the self segment of hop 1 (no rank's
    send count to another rank includes one), are routed by the sending rank's catalog and are never forwarded by hop 2;
    everything else follows node_replay.  Hosted headers, route, act, order and offsets == stateless_ref.expected_node."""
    from test_gpu_node import _fill_caches, _run
    t = torch
    ros = None if nranks != 3 else [s % 3 for s in range(8)]
    world, cats = _node_world(t, nranks, host_mix, wire, ros)
    caches = _fill_caches(t, world, 0.5, 0.05, seed=nranks * 7 + chunks) if cache else None
    gid = b"node-sw-%d-%d-%s-%d" % (nranks, chunks, str(wire).encode(), int(cache))
    nodes = [GrainNode(world.engs[r], nranks, r, world.ros, max_batch=100_000, max_recv=200_000,
                       transport=L.TRANSPORT_LOCAL, group_id=gid, chunks=chunks) for r in range(nranks)]
    streams = [t.cuda.Stream() for _ in range(nranks)]
    for b in range(2):
        batches = [_node_batch(world, r, 60_000 - 3000 * r - 500 * b, seed=100 * b + r) for r in range(nranks)]
        exp, forward, sent, remote = S.expected_node(world.oracles, cats, TYPES, world.ros, batches, chunks, world.n_act,
                                                     caches=caches)
        assert sent.sum() > 0.08 * sum(len(x) for x in batches) and (sent - np.diag(np.diag(sent))).sum() == 0
        got = _run(t, world, nodes, batches, streams)
        for r in range(nranks):
            res, (route, act, order, off, hdrs) = got[r]
            er, ea, eo, ef, eh = exp[r]
            assert res.hop2 == forward
            assert res.n_sent_remote == remote[r], (res.n_sent_remote, remote[r])
            np.testing.assert_array_equal(hdrs, eh, err_msg=f"rank {r} batch {b} headers")
            np.testing.assert_array_equal(route, er, err_msg=f"rank {r} batch {b} route")
            np.testing.assert_array_equal(act, ea, err_msg=f"rank {r} batch {b} act")
            np.testing.assert_array_equal(order, eo, err_msg=f"rank {r} batch {b} order")
            np.testing.assert_array_equal(off, ef, err_msg=f"rank {r} batch {b} offsets")
            sw = S.listed(hdrs, TYPES)
            assert sw.sum() == sent[r, r]  # every one hosted where it was sent
            assert (world.ros[hdrs["sending_silo"][sw]] == r).all()
            assert ((decode_route(route[sw]).flags & L.RF_STATELESS) != 0).all()
    for nd in nodes:
        nd.close()
    world.close()
