"""Stage 4 at every key width, tile regime and out-of-range handle ("stage 4 by key width").

The launcher takes a different route through route_kernels.hip for every bit length w of n_act: one level (w <= 11: the
level-2 kernels read the handles directly, one instantiation per w), two levels (w = 12..22: an MSD pass of hb bits, then
level 2 of lb bits) and three LSD passes (w >= 23).  The tests of the BASELINE configs reach some of those widths; these
run all of w = 1..27 at both edges of each width (n_act = 2^(w-1): the unresolved key alone has the top bit; 2^w - 1: it
is all ones), with handles at and above n_act that are not ORL_NO_ACT, with the route kernel as the producer of pass 0's
histogram rows at every tile size it chooses, the dense LSD form at 23 bits and the two-level hot-key path off the widths
the config tests run it at.  Every comparison is exact: order and offsets == tests/stage4_ref.bucket_ref (a stable numpy
argsort of min(act, n_act) and the prefix of the counts: ActivationData.EnqueueMessage FIFO, ActivationData.cs:483-514).
stage4_ref.plan_of only chooses inputs here; tests/test_stage4_ref.py asserts what the matrix covers.

Widths 28..31 stay out: their offsets array alone is 1 to 8 GB and the host reference takes proportionally longer.
"""
import functools

import numpy as np
import pytest

import stage4_ref as S
from oracle import cpu_ref
from orleans_amd import _lib as L
from orleans_amd import workloads as W
from orleans_amd.engine import GrainDirectoryEngine

pytestmark = pytest.mark.gpu

NO_HOT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _u32(x):
    return x.cpu().numpy().view(np.uint32)


def _engine(n_act, max_batch, dir_capacity=16):
    eng = GrainDirectoryEngine(n_act=n_act, dir_capacity=dir_capacity, max_batch=max_batch, device=0)
    W.setup_engine(eng, W.default_cluster())
    return eng


def _assert_equal(got, exp, msg):
    """assert_array_equal; its report is built only on a mismatch (on 2^27 offsets it costs ten times the comparison)."""
    if got.shape != exp.shape or not np.array_equal(got, exp):
        np.testing.assert_array_equal(got, exp, err_msg=msg)
        raise AssertionError(msg)


def _offsets_equal_on_device(t, off, a, n_act):
    """off == bucket_ref's offsets without moving them: the reference's run-length form (numpy: stage4_ref.offsets_runs,
    held to the counts' prefix by test_stage4_ref.py) is expanded on the device and compared there, element for element."""
    totals, runs = S.offsets_runs(a, n_act)
    exp = t.repeat_interleave(t.from_numpy(totals.view(np.int32)).cuda(), t.from_numpy(runs).cuda(), output_size=n_act + 2)
    return exp.shape == off.shape and bool(t.equal(off, exp))


def _bucket_and_check(t, eng, a, n_act, off, ref=None, msg="", sparse=False):
    """One orl_bucket_device call over handles a, outputs pre-filled with -1, == bucket_ref.  sparse: far more buckets
    than messages (the LSD widths' 16 to 512 MB of offsets per call) — the offsets are compared on the device first, and
    only a mismatch brings them to the host for assert_array_equal's report."""
    d_act = t.from_numpy(a.view(np.int32)).cuda()
    order = t.full((len(a),), -1, dtype=t.int32, device="cuda")
    off.fill_(-1)
    t.cuda.synchronize()  # the fills are on torch's stream, the call on the context's
    eng.bucket_device(d_act, len(a), order, off)
    t.cuda.synchronize()
    if sparse and _offsets_equal_on_device(t, off, a, n_act):
        eo = S.order_ref(a, n_act)
    else:
        eo, ef = S.bucket_ref(a, n_act) if ref is None else ref
        _assert_equal(_u32(off), ef, f"n_act {n_act} {msg}: offsets")
    _assert_equal(_u32(order), eo, f"n_act {n_act} {msg}: order")


# ---- a. every width, stage 4 alone ------------------------------------------------------------------------------
@pytest.mark.parametrize("w,n_act", S.width_cases(), ids=[f"w{w}-{a}" for w, a in S.width_cases()])
def test_every_width_bucket_device_vs_ref(torch, w, n_act):
    """orl_bucket_device (16 items per thread: row_step0 = 1) at both edges of the width, batches of 1 to 40,001
    messages (one partial wave, one tile exactly, a tile and one, three tiles and one, ten tiles: several segments per
    bucket at small widths) from every builder: uniform with 5 % unresolved, only the width's edge keys, one bucket (the
    first, the last, the unresolved one), and aliases (the unresolved messages carry n_act, n_act + 1, 2^w, 0x80000000,
    0xFFFFFFFE or ORL_NO_ACT).  From w = 23 on the batches are sparse (k_offsets_gaps / k_offsets_long): the one-bucket,
    edge and far-apart-key batches leave millions of empty buckets before the first key, between keys and after the last
    one, and the whole offsets array (16 to 512 MB) is compared, on the device.  Compared on the host, with nine batches
    instead of 42, the two n_act = 2^27 - 1 and 2^26 cases took 4.8 s and 2.3 s on an MI355X box where
    test_lsd_offsets_long_gaps_vs_oracle takes 2.05 s."""
    t = torch
    p = S.plan_of(n_act)
    assert p.w == w
    eng = _engine(n_act, 1 << 16)
    off = t.empty(n_act + 2, dtype=t.int32, device="cuda")
    try:
        for name, n in S.width_batches(n_act):
            _bucket_and_check(t, eng, S.build(name, n_act, n), n_act, off, msg=f"{name} n {n}", sparse=not p.two_level)
        assert eng.query(L.Q_STAGE4_ERROR) == 0
    finally:
        eng.close()


def test_device_comparison_is_bucket_ref_and_sees_one_wrong_offset(torch):
    """The on-device comparison of the LSD widths accepts bucket_ref's own offsets (uploaded whole) and refuses them with
    one word changed: inside a run of empty buckets, at a key, at the first and at the last bucket."""
    t = torch
    n_act = (1 << 23) - 1
    a = S.build("aliases", n_act, 4097)
    _, ef = S.bucket_ref(a, n_act)
    off = t.from_numpy(ef.view(np.int32)).cuda()
    assert _offsets_equal_on_device(t, off, a, n_act)
    for b in (0, int(a.min()), n_act // 3, n_act, n_act + 1):
        bad = off.clone()
        bad[b] += 1
        assert not _offsets_equal_on_device(t, bad, a, n_act), b
    assert not _offsets_equal_on_device(t, off[:-1], a, n_act)


# ---- b. the dense LSD form at 23 bits ---------------------------------------------------------------------------
def _dense_batch(kind):
    n_act, n = S.dense_case()
    rng = np.random.default_rng(23)
    if kind == "uniform":
        return rng.integers(0, n_act, n, dtype=np.int64).astype(np.uint32)
    if kind == "zipf":
        r = np.minimum(rng.zipf(1.1, n), n_act) - 1
        return ((r.astype(np.uint64) * np.uint64(2654435761)) % np.uint64(n_act)).astype(np.uint32)
    if kind == "few":  # millions of empty buckets between and around the keys
        return rng.choice(np.array([3, 4, 2_000_000, 2_000_001, n_act - 100_000], np.uint32), n)
    assert kind == "aliases"
    return S.aliases(n_act, n, 23, unresolved=0.3)


@pytest.mark.parametrize("kind", ["uniform", "zipf", "few", "aliases"])
def test_lsd_dense_width23_vs_ref(torch, kind):
    """The LSD plan's last pass writing the offsets itself (OUT_FINAL_GAPS + the bound kernels) at the only dense width
    besides 24: n_act = 2^22 (8 + 8 + 7-bit digits: a 128-bin last pass, the top digit holds the unresolved key alone)
    and the smallest batch lsd_gaps takes.  From 25 bits on the last shift exceeds 16 and no batch is dense."""
    t = torch
    n_act, n = S.dense_case()
    assert S.lsd_gaps(n_act, n)
    eng = _engine(n_act, n)
    off = t.empty(n_act + 2, dtype=t.int32, device="cuda")
    try:
        _bucket_and_check(t, eng, _dense_batch(kind), n_act, off, msg=kind)
        assert eng.query(L.Q_STAGE4_ERROR) == 0
    finally:
        eng.close()


# ---- c. the route kernel as pass 0's producer -------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _route_messages(n):
    return W.uniform_messages(W.default_cluster(), 22_000, n, seed=n)  # ~9 % never-registered targets; shared, read only


@pytest.mark.parametrize("w,n_act,items,n", S.route_cases(), ids=[f"w{w}-items{i}" for w, _, i, _ in S.route_cases()])
def test_route_kernel_rows_feed_stage4_vs_ref(torch, w, n_act, items, n):
    """orl_route_batch_device: k_route writes pass 0's histogram rows, one per route tile of 256 * items messages, and
    stage 4 reads every row_step0-th (two levels: 8, 4, 2, 1 with the 2048-element MSD tile up to 8 items; LSD: 16, 8,
    4, 2, 1; one level: no histogram).  One batch size inside each route_items range, on 20,000 grains (90 % registered)
    whose handles are drawn over all of [0, n_act).  Route words and handles == the oracle; order and offsets ==
    bucket_ref of the oracle's handles."""
    t = torch
    assert S.route_items(n, S.plan_of(n_act).max_items) == items
    cl = W.default_cluster()
    n_grains = 20_000
    eng = _engine(n_act, n, dir_capacity=n_grains)
    o = cpu_ref.Oracle(cl.n_silos)
    for s in range(cl.n_silos):
        o.add_server(s, int(cl.hashes[s]))
    keys, uni, owner, reg = W.grain_population(cl, n_grains, 0.9, 11)
    rng = np.random.default_rng(w)
    acts = rng.integers(0, n_act, n_grains).astype(np.uint32)  # handles may collide: many grains, one bucket
    idx = np.nonzero(reg)[0]
    st_e, _, _ = eng.register_single_activation(keys[idx], acts[idx], owner[idx])
    st_o, _, _ = o.register(keys[idx], acts[idx], owner[idx])
    np.testing.assert_array_equal(st_e, st_o)
    msgs = _route_messages(n)
    try:
        d_in = t.from_numpy(msgs.view(np.int32).reshape(-1, 8)).cuda()
        route, act, order = (t.full((n,), -1, dtype=t.int32, device="cuda") for _ in range(3))
        off = t.full((n_act + 2,), -1, dtype=t.int32, device="cuda")
        t.cuda.synchronize()
        eng.address_messages_device(d_in, n, route, act, order, off)
        t.cuda.synchronize()
        r, a = o.route(msgs)
        _assert_equal(_u32(route), r, "route words")
        _assert_equal(_u32(act), a, "handles")
        eo, ef = S.bucket_ref(a, n_act)
        _assert_equal(_u32(off), ef, "offsets")
        _assert_equal(_u32(order), eo, "order")
        assert eng.query(L.Q_STAGE4_ERROR) == 0
    finally:
        eng.close()


# ---- d. the two-level hot-key path off the widths the config tests run it at ------------------------------------
@functools.lru_cache(maxsize=1)
def _hot_plan(n_act):
    """[(label, handles, reference, the key the batch leaves picked)]: pairs of batches with one key at > 1/32 of the
    batch and > 8192 messages at random positions (key 0, a key of the last MSD bucket that holds activations, the
    unresolved bucket through mixed aliases), then two uniform batches (1 % unresolved: nothing to pick)."""
    n = S.HOT_N
    count = n // 5
    assert count > n // S.K_HOT_SHARE and count > S.K_HOT_MIN_COUNT
    plan = []
    for j, hot in enumerate((0, n_act - 3, n_act)):
        for rep in range(2):
            a = S.hot_mix(n_act, n - rep, 10 * j + rep, hot, count + 1000 * rep)
            plan.append((f"hot key {hot} batch {rep}", a, S.bucket_ref(a, n_act), hot))
    for rep in range(2):
        a = S.uniform(n_act, n, 90 + rep, unresolved=0.01)
        plan.append((f"uniform {rep}", a, S.bucket_ref(a, n_act), NO_HOT))
    for _, _, ref, _ in plan:  # shared by both ranking modes
        for x in ref:
            x.setflags(write=False)
    return plan


@pytest.mark.parametrize("mode", [0, 1], ids=["lds", "ballot"])
@pytest.mark.parametrize("w,n_act", S.HOT_WIDTHS, ids=[f"w{w}" for w, _ in S.HOT_WIDTHS])
def test_two_level_hot_key_path_vs_ref(torch, w, n_act, mode):
    """The hot-key path (hb > 0, n >= 2^20) at w = 12, 15, 17, 21, 22 in both ranking modes: the first batch of a pair
    lets the tail kernel pick the key, the second places that key's messages without sorting them (ORL_Q_HOT_KEY is the
    expected key after each, ORL_Q_HOT_BATCHES grew over the second).  The first batch of the next pair runs the path on a
    key that is now rare; the first uniform batch runs it on a stale key and picks none; the second uniform batch does not
    take the path.  Every batch == bucket_ref."""
    t = torch
    p = S.plan_of(n_act)
    assert p.w == w and p.two_level and p.hb > 0 and S.HOT_N >= S.K_HOT_MIN_BATCH
    eng = _engine(n_act, S.HOT_N)
    off = t.empty(n_act + 2, dtype=t.int32, device="cuda")
    try:
        eng.set_rank_mode(mode)
        assert eng.query(L.Q_RANK_MODE) == mode
        for k, (label, a, ref, picked) in enumerate(_hot_plan(n_act)):
            before = eng.query(L.Q_HOT_BATCHES)
            _bucket_and_check(t, eng, a, n_act, off, ref=ref, msg=label)
            assert eng.query(L.Q_HOT_KEY) == picked, (label, eng.query(L.Q_HOT_KEY))
            ran = eng.query(L.Q_HOT_BATCHES) - before
            assert ran == (0 if k in (0, 7) else 1), (label, ran)  # no key known yet / none picked by the batch before
        assert eng.query(L.Q_STAGE4_ERROR) == 0
    finally:
        eng.set_rank_mode(0)  # the mode is process-wide
        eng.close()
