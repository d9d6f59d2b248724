"""The collector's reference model (collector_ref) without a GPU: one hand-derived case per coverage counter with the end
state written out; the numpy per-activation form against the literal model on random histories (admit -> touch ->
on-complete -> complete -> scan over several quanta, the table from admission_ref / completion_ref); the on-complete
property (the per-completion order and the batched rule condemn the same sets at every scan and agree on became_idle of
every inactive activation) with the R / B / W1 example; exports, constants and sizeof(orl_collector_view) against the
header; the host-only refusal; every GPU scenario through the model, which must leave every counter non-zero.
"""
import ctypes as C
import os
import re
from collections import Counter

import numpy as np
import pytest

import collector_ref as R
import completion_ref as Q
from orleans_amd import _lib as L
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
T0, QT = R.T0, R.QUANTUM


def _ref(n_act=4, age=QT, cov=None):
    r = R.RefCollector(n_act, QT, T0, cov)
    for it in r.items:
        it.age_limit = age
    return r


def _table(n_act=4):
    return R.idle_valid_state(n_act)


def _tickets(r):
    return [(it.ticket - T0) // QT if it.ticket else None for it in r.items]


# ---- hand-derived cases, one per counter -------------------------------------------------------------------------------
def test_ticket_arithmetic_at_a_multiple_and_one_past():
    """now + age = T0 + Q is a multiple of the quantum: the ticket is that instant; one tick later rounds up a whole
    quantum.  next_ticket = mk(T0) = T0."""
    cov = Counter()
    r = _ref(cov=cov)
    assert r.next_ticket == T0 and R.mk(T0 + 1, QT) == T0 + QT and R.mk(T0, QT) == T0
    assert list(r.schedule([0], T0))[:1] == [1] and list(r.schedule([1], T0 + 1))[:1] == [1]
    assert _tickets(r) == [1, 2, None, None]
    assert cov["ticket_exact_multiple"] == 1 and cov["ticket_one_past"] == 1


def test_schedule_exempt_zero_bad_timeout_and_ticketed():
    cov = Counter()
    r = _ref(cov=cov)
    r.items[0].exempt = True
    r.items[1].age_limit = 0
    r.items[2].age_limit = QT - 1
    counts = r.schedule([0, 1, 2, 3, 9], T0 + 1)
    assert list(counts) == [1, 1, 1, 1, 0, 1, 0, 0]
    counts = r.schedule([3], T0 + QT + 5)  # the reference throws; the entry stays
    assert list(counts) == [0, 0, 0, 0, 1, 0, 0, 0]
    assert _tickets(r) == [None, None, None, 2]
    assert cov["bad_timeout"] == 1 and cov["schedule_on_ticketed"] == 1


def test_cancel_needs_a_live_uncancelled_ticket():
    r = _ref()
    r.items[0].exempt = True
    r.schedule([1, 2], T0 + 1)
    assert list(r.cancel([0, 1, 3, 7])) == [1, 1, 1, 0, 0, 1, 0, 0]
    assert list(r.cancel([1])) == [0, 0, 0, 0, 1, 0, 0, 0]
    assert [it.cancelled for it in r.items] == [False, True, False, False] and _tickets(r) == [None, 2, 2, None]
    assert 1 not in r.buckets[T0 + 2 * QT].items and 2 in r.buckets[T0 + 2 * QT].items  # TryRemove took it out
    st = _table()
    r.scan_stale(st, T0 + 2 * QT)  # bucket T0 + 2Q dequeued: handle 2 condemned, handle 1 keeps its dead ticket
    assert list(r.cancel([1])) == [0, 0, 0, 1, 0, 0, 0, 0]  # expired


def test_touch_moves_drops_and_keeps():
    """Handle 0: a live ticket moves.  Handle 1: cancelled, the new ticket differs: dropped, the flag stays.  Handle 2:
    cancelled, the new ticket is the old one: nothing.  Handle 3: cancelled and expired by a scan: dropped."""
    cov = Counter()
    r = _ref(cov=cov)
    r.items[2].age_limit = 2 * QT
    r.schedule([0, 1, 2, 3], T0 + 1)
    assert _tickets(r) == [2, 2, 3, 2]
    r.cancel([1, 2, 3])
    st = _table()
    act = np.array([0, 1, 2], np.uint32)
    disp = np.full(3, L.ADM_RUN, np.uint8)
    counts = r.touch(act, disp, st, 0, 0, T0 + QT)  # new = mk(T0 + Q + age): 2 for handles 0, 1 (same), 3 for handle 2 (same)
    assert list(counts) == [3, 0, 3, 0, 0, 0, 0, 0] and cov["same_ticket_on_cancelled"] == 2
    counts = r.touch(act, disp, st, 0, 0, T0 + QT + 1)  # new = 3, 3, 4
    assert list(counts) == [3, 1, 0, 0, 2, 0, 0, 0]
    assert _tickets(r) == [3, None, None, 2] and [it.cancelled for it in r.items] == [False, True, True, True]
    assert cov["cancelled_touched_ticket_dropped"] == 2
    condemned, sc = r.scan_stale(st, T0 + 2 * QT)  # dequeues up to T0 + 2Q; handle 3's cancelled item is not returned
    assert condemned == [] and sc[L.SCAN_CANCELLED_SKIPPED] == 1 and r.next_ticket == T0 + 3 * QT
    counts = r.touch(np.array([3], np.uint32), disp[:1], st, 0, 0, T0 + 2 * QT + 1)
    assert list(counts) == [1, 0, 0, 1, 0, 0, 0, 0] and cov["expired_touched"] == 1 and _tickets(r)[3] is None


def test_rule_1_only_is_no_touch_and_rule_7_only_is():
    """L = 2.  Handle 0 holds c = 3 > L: IncomingMessageAgent rejects before the dispatcher.  Handle 1 holds c = 2 = L
    behind a read-write Running: EnqueueRequest rejects, after Catalog.GetOrCreateActivation."""
    cov = Counter()
    r = _ref(cov=cov)
    r.schedule([0, 1], T0 + 1)
    st = _table()
    st[0] = (L.ACT_VALID, L.ACTF_RUNNING_SET, 0, 1, 3, 0)
    st[1] = (L.ACT_VALID, L.ACTF_RUNNING_SET, 0, 1, 1, 1)
    act = np.array([0, 1, 0, 1], np.uint32)
    fl = np.full(4, L.MF_REQUEST, np.uint8)
    disp, after, _ = R.A.admit(act, fl, st, 4, 2, 0)
    assert list(disp) == [L.ADM_OVERLOADED] * 4 and np.array_equal(after, st)
    assert list(R.reaches_catalog(act, disp, st, 2, 0)) == [False, True, False, True]
    counts = r.touch(act, disp, st, 2, 0, T0 + QT + 1)
    assert list(counts) == [1, 1, 0, 0, 0, 0, 1, 1] and _tickets(r)[:2] == [2, 3]
    assert cov["rule1_only_not_touched"] == 1 and cov["rule7_only_touched"] == 1
    col = R.Col(4, QT, T0)
    col.age_limit[:] = QT
    R.np_schedule(col, [0, 1], T0 + 1)
    assert list(R.np_touch(col, act, disp, after, 2, 0, T0 + QT + 1)) == list(counts)
    assert not r.export().diff(col)


def test_scan_stale_branches_with_exact_boundaries():
    """collector_ref.branch_scenario by hand: handles 0..7 = bad state, kept alive (== now), condemned (keep-alive one tick
    past), running, waiting, one tick too young, cancelled (skipped), condemned with idleness == the age limit."""
    cov = Counter()
    sc = R.branch_scenario()
    steps = R.run_literal(sc, cov)
    s = steps[3]
    assert list(s.condemned) == [2, 7]
    assert list(s.counts) == [7, 1, 1, 2, 1, 2, 1, 0]
    q = lambda k: T0 + k * QT
    assert list(s.col.ticket) == [0, q(3), 0, q(3), q(3), q(3), q(1), 0]
    assert list(s.col.cflags) == [2, 0, 2, 0, 0, 0, 2, 2]
    assert list(s.state["state"]) == [3, 2, 3, 2, 2, 2, 2, 3]
    for c in ("stale_bad_state", "stale_kept_alive", "stale_active", "stale_not_stale", "stale_condemned",
              "keep_alive_eq_now", "idleness_eq_age_limit"):
        assert cov[c] >= 1, c
    # on-complete: handle 3 (k = 1 = num_running) and handle 5 (k = 1 > 0) become idle; pump and drain records do not count
    s = steps[4]
    assert list(s.counts) == [2, 2, 0, 0, 0, 0, 1, 2]
    assert s.col.became_idle[3] == s.col.became_idle[5] == q(2) + 1 and s.col.ticket[3] == s.col.ticket[5] == q(4)


def test_scan_all_cancels_in_place_and_cancel_all_skips_it():
    cov = Counter()
    steps = R.run_literal(R.quirk_scenario(), cov)
    s = steps[2]  # ScanAll: 0..4 condemned (cancelled in place, tickets stay), 5 kept alive
    assert list(s.condemned) == [0, 1, 2, 3, 4] and list(s.counts) == [6, 0, 1, 0, 0, 5, 0, 0]
    assert list(s.col.cflags) == [2, 2, 2, 2, 2, 0] and all(s.col.ticket != 0)
    assert list(steps[3].counts) == [1, 0, 1, 0, 0, 0, 0, 0]  # new == old on a cancelled item
    assert list(steps[4].counts) == [2, 0, 0, 0, 1, 1, 0, 0]  # dropped; bad timeout
    assert steps[4].col.ticket[0] == 0 and steps[4].col.ticket[3] == T0 + 2 * QT
    assert list(steps[5].counts) == [1, 0, 1, 0, 0, 0, 3, 0] and len(steps[5].condemned) == 0
    assert list(steps[6].counts) == [1, 0, 0, 1, 0, 0, 0, 0]
    assert list(steps[7].counts) == [0] * 8 and len(steps[7].condemned) == 0
    for c in ("cancelall_skipped_cancelled", "cancelled_touched_ticket_dropped", "expired_touched", "same_ticket_on_cancelled",
              "bad_timeout", "schedule_on_ticketed"):
        assert cov[c] >= 1, c


# ---- numpy form == literal model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(6))
def test_numpy_form_equals_the_literal_model_on_random_histories(block):
    for seed in range(50 * block, 50 * block + 50):
        assert R.play_numpy(seed) == [], seed


# ---- the on-complete choice ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(6))
def test_per_completion_order_and_batched_rule_condemn_the_same(block):
    later = 0
    for seed in range(50 * block, 50 * block + 50):
        a, b = R.play(seed, per_completion=False), R.play(seed, per_completion=True)
        for step, ((ca, ia, ea, wa), (cb, ib, eb, wb)) in enumerate(zip(a, b)):
            assert ca == cb, (seed, step, ca, cb)
            assert ia == ib, (seed, step)
            assert wa.same(wb), (seed, step)
            busy = (wa.state["num_running"] > 0) | (wa.state["waiting"] > 0)
            differ = ea.ticket != eb.ticket
            assert not (differ & ~busy & (wa.state["state"] == L.ACT_VALID)).any(), (seed, step)
            later += int(differ.sum())
    assert later > 0 or block > 0  # the two orders do differ somewhere in the first block


def test_r_b_w1_example():
    """R (Running, read-write) and B (always-interleave) run, W1 waits.  R and B complete in one batch.  Per completion,
    Running's first: the pump takes W1 before B completes and numRunning never reads 0.  Batched: k = 2 >= num_running
    = 2, so became_idle = now and the ticket moves a quantum later.  W1's own completion reaches 0 in both and rewrites
    became_idle and the ticket identically."""
    def start():
        s = np.zeros(1, R.STATE_DTYPE)
        s[0] = (L.ACT_VALID, L.ACTF_RUNNING_SET, 0, 2, 2, 1)
        w = Q.World(s, [0, 1], [700], [L.MF_REQUEST], [500])
        r = _ref(1)
        r.schedule([0], T0 + 1)
        return w, r

    now = T0 + QT + 5
    cact, ctok = np.array([0, 0], np.uint32), np.array([501, 500], np.uint32)
    w, lit = start()
    w_lit, out, _ = R.complete_per_completion(lit, w, cact, ctok, now)
    w, bat = start()
    bat.on_complete(cact, ctok, w.state, now)
    w_bat, out2, _ = Q.complete(w, cact, ctok)
    assert out == out2 == [(700, 0, L.MF_REQUEST, L.WQ_RUN)] and w_lit.same(w_bat) and w_bat.state[0]["num_running"] == 1
    assert (lit.items[0].became_idle, lit.items[0].ticket) == (0, T0 + 2 * QT)
    assert (bat.items[0].became_idle, bat.items[0].ticket) == (now, T0 + 3 * QT)  # the later ticket of a busy activation
    for r_ in (lit, bat):  # ScanStale at T0 + 2Q: the literal order defers an active activation; neither condemns
        st = w_bat.state.copy()
        assert r_.scan_stale(st, T0 + 2 * QT)[0] == []
    now2 = T0 + 2 * QT + 9
    for r_, w_ in ((lit, w_lit), (bat, w_bat)):
        complete = R.complete_per_completion if r_ is lit else None
        if complete:
            complete(r_, w_, [0], [700], now2)
        else:
            r_.on_complete([0], [700], w_.state, now2)
    assert (lit.items[0].became_idle, lit.items[0].ticket) == (bat.items[0].became_idle, bat.items[0].ticket) == \
        (now2, T0 + 4 * QT)


# ---- the interface ------------------------------------------------------------------------------------------------------
NAMES = ("orl_collector_create", "orl_collector_destroy", "orl_collector_view_get", "orl_collect_schedule_device",
         "orl_collect_cancel_device", "orl_collect_touch_device", "orl_collect_on_complete_device",
         "orl_collect_scan_stale_device", "orl_collect_scan_all_device")


def test_exports_constants_and_view_size_match_the_header():
    lib = L.load()
    text = open(os.path.join(ROOT, "include", "orleans_route.h")).read()
    for name in NAMES:
        assert name in L.EXPORTED and hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, text)
    defs = {k: int(v, 0) for k, v in re.findall(r"#define (ORL_COLF_[A-Z_]+) (0x[0-9A-Fa-f]+|\d+)u", text)}
    assert defs == {"ORL_COLF_EXEMPT": L.COLF_EXEMPT, "ORL_COLF_CANCELLED": L.COLF_CANCELLED} == \
        {"ORL_COLF_EXEMPT": 1, "ORL_COLF_CANCELLED": 2}
    assert re.search(r"#define ORL_ABI_VERSION 1u", text) and L.ABI_VERSION == 1
    m = re.search(r"typedef struct orl_collector_view \{(.*?)\} orl_collector_view;", text, re.S)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f for f, _ in L.orl_collector_view._fields_]
    assert C.sizeof(L.orl_collector_view) == 7 * C.sizeof(C.c_void_p) + 16 == 72
    assert (L.COL_TOUCHED, L.COL_MOVED, L.COL_SAME, L.COL_EXPIRED, L.COL_CANCELLED_DROPPED, L.COL_BAD_TIMEOUT,
            L.COL_RULE1_ONLY, L.COL_RULE7_ONLY) == tuple(range(8))
    assert (L.COL_BECAME_IDLE, L.COL_IGNORED, L.COL_COMPLETIONS) == (0, 6, 7)
    assert (L.SCAN_CANDIDATES, L.SCAN_BAD_STATE, L.SCAN_KEPT_ALIVE, L.SCAN_ACTIVE, L.SCAN_NOT_STALE, L.SCAN_CONDEMNED,
            L.SCAN_CANCELLED_SKIPPED, L.SCAN_UNSCHEDULED) == tuple(range(8))


def test_host_only_context_refuses_the_collector():
    eng = GrainDirectoryEngine(n_act=16, dir_capacity=16, device=-1)
    try:
        z, b, st = np.zeros(4, np.uint32), np.zeros(4, np.uint8), np.zeros(16, L.ACT_STATE_DTYPE)
        for call in (lambda: eng.collector_create(QT, T0),
                     lambda: eng.collect_schedule_device(None, z, 4, T0),
                     lambda: eng.collect_cancel_device(None, z, 4),
                     lambda: eng.collect_touch_device(None, z, b, 4, st, T0),
                     lambda: eng.collect_on_complete_device(None, z, z, 4, st, T0),
                     lambda: eng.collect_scan_stale_device(None, st, T0),
                     lambda: eng.collect_scan_all_device(None, st, QT, T0)):
            with pytest.raises(OrleansRouteError) as e:
                call()
            assert e.value.code == L.E_STATE
    finally:
        eng.close()


# ---- the GPU file's scenarios, through the model alone --------------------------------------------------------------------
def _same_steps(sc, a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        assert not x.col.diff(y.col), (sc.name, i, x.op[0], x.col.diff(y.col))
        assert np.array_equal(x.state, y.state), (sc.name, i, x.op[0])
        assert list(x.counts) == list(y.counts), (sc.name, i, x.op[0], list(x.counts), list(y.counts))
        assert (x.condemned is None) == (y.condemned is None)
        assert x.condemned is None or list(x.condemned) == list(y.condemned), (sc.name, i)


def test_gpu_scenarios_agree_in_both_forms_and_reach_every_counter():
    """The scenarios up to 5000 activations / 4097 messages through both forms (the larger ones differ only in size)."""
    cov = Counter()
    names = set()
    for sc in R.all_scenarios(big=False):
        assert sc.name not in names
        names.add(sc.name)
        _same_steps(sc, R.run_literal(sc, cov), R.run_numpy(sc))
    missing = [c for c in R.COUNTERS if cov[c] == 0]
    assert not missing, missing


def test_density_scenarios_condemn_what_their_names_say():
    for n_act in R.GPU_N_ACT:
        tiles = (n_act + 2047) // 2048
        for density, first, second in (("none", 0, 0), ("all", n_act, 0), ("one-per-tile", None, None)):
            steps = R.run_numpy(R.density_scenario(n_act, density))
            got = len(steps[1].condemned)
            if first is None:
                assert tiles <= got <= tiles + 1 and steps[1].condemned[-1] == n_act - 1
                assert np.array_equal(np.unique(steps[1].condemned // 2048), np.arange(tiles))
                assert len(steps[3].condemned) == n_act - got
            else:
                assert got == first and len(steps[3].condemned) == second
            assert len(steps[2].condemned) == 0 and list(steps[2].counts) == [0] * 8


def test_chained_rounds_condemn_something_in_every_kind_of_scan():
    rounds, _, expect = R.chain_rounds()
    kinds = {r[8]: len(e[3]) for r, e in zip(rounds, expect)}
    assert kinds["scan_all"] > 0 and kinds["scan_stale"] > 0
    assert all(e[4][L.COL_TOUCHED] > 0 and e[5][L.COL_BECAME_IDLE] > 0 for e in expect)
    assert any(e[4][L.COL_MOVED] > 0 for e in expect) and any(e[4][L.COL_RULE1_ONLY] > 0 for e in expect)
