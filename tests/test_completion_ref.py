"""The waiting-queue model (tests/completion_ref.py) without a GPU: one hand-derived case per coverage counter with the out
list and the end state written out; the B / R example of DESIGN §17 in both orders; the closed form against the loop and
the loop against itself under permutations of the non-Running completions on random small cases; the new exports,
constants and sizeof(orl_waitq_view) against the header; the host-only refusal; every GPU scenario through the model,
which must leave every counter non-zero; admit / append / complete chained, with the table's waiting counts and
running_tok held to the store.
"""
import ctypes as C
import os
import re
from collections import Counter

import numpy as np
import pytest

import admission_ref as A
import completion_ref as Q
from orleans_amd import _lib as L
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RW, RO, AI = L.MF_REQUEST, L.MF_READ_ONLY, L.MF_ALWAYS_INTERLEAVE
SET, SRO, REENT = L.ACTF_RUNNING_SET, L.ACTF_RUNNING_RO, L.ACTF_REENTRANT
NONE, DRAIN = L.TOK_NONE, L.TOK_DRAIN
RUN, DRAINED = L.WQ_RUN, L.WQ_DRAINED


def world(entry, waiting, rt, n_act=2):
    """Activation 0 = entry (state, flags, num_running, in_flight) with the waiting list [(tok, mflags)] and Running's
    token rt; activation 1 an idle VALID bystander with one waiting record that nothing may touch."""
    s = np.zeros(n_act, Q.STATE_DTYPE)
    s[0] = (entry[0], entry[1], 0, entry[2], entry[3], len(waiting))
    s[1] = (L.ACT_VALID, SET, 0, 1, 1, 1)
    off = [0, len(waiting)] + [len(waiting) + 1] * (n_act - 1)
    return Q.World(s, off, [t for t, _ in waiting] + [500], [f for _, f in waiting] + [RW], [rt, 600] + [NONE] * (n_act - 2))


def entry(w, a=0):
    e = w.state[a]
    return int(e["state"]), int(e["flags"]), int(e["num_running"]), int(e["in_flight"]), int(e["waiting"])


VALID = L.ACT_VALID
# name, (state, flags, num_running, in_flight), waiting, running_tok, records,
#   -> out list, (state, flags, num_running, in_flight, waiting), running_tok, waiting tokens left, counts by CMP_* index
HAND = [
    # Running (read-write) completes with another request still running: Running == null lets the read-write head in
    ("running_cleared_rw_head_taken", (VALID, SET, 2, 2), [(10, RW), (11, RW)], 7, [(0, 7)],
     [(10, 0, RW, RUN)], (VALID, SET, 2, 2, 1), 10, [11], {0: 1, 5: 1, 7: 2}),
    # a completion that is not Running's leaves Running; the read-write head stays behind it
    ("completion_not_running", (VALID, SET, 2, 2), [(10, RW)], 7, [(0, 99)],
     [], (VALID, SET, 1, 1, 1), 7, [10], {0: 1, 7: 2}),
    # a read-only head runs beside a read-only Running; the read-write record behind it stops the pump, and the
    # read-only one behind that waits too
    ("pump_stopped_by_head", (VALID, SET | SRO, 2, 2), [(10, RO), (11, RW), (12, RO)], 7, [(0, 99)],
     [(10, 0, RO, RUN)], (VALID, SET | SRO, 2, 2, 2), 7, [11, 12], {0: 1, 5: 1, 7: 3}),
    ("always_interleave_past_rw_running", (VALID, SET, 2, 2), [(10, AI), (11, RW)], 7, [(0, 99)],
     [(10, 0, AI, RUN)], (VALID, SET, 2, 2, 1), 7, [11], {0: 1, 5: 1, 7: 2}),
    ("read_only_run", (VALID, SET | SRO, 3, 3), [(10, RO), (11, RO), (12, RO)], 7, [(0, 99)],
     [(10, 0, RO, RUN), (11, 0, RO, RUN), (12, 0, RO, RUN)], (VALID, SET | SRO, 5, 5, 0), 7, [], {0: 1, 5: 3, 7: 1}),
    ("reentrant_emptied", (VALID, SET | REENT, 2, 2), [(10, RW), (11, RW)], 7, [(0, 99)],
     [(10, 0, RW, RUN), (11, 0, RW, RUN)], (VALID, SET | REENT, 3, 3, 0), 7, [], {0: 1, 5: 2, 7: 1}),
    ("non_valid_not_pumped", (L.ACT_DEACTIVATING, SET, 1, 1), [(10, RW)], 7, [(0, 7)],
     [], (L.ACT_DEACTIVATING, 0, 0, 0, 1), NONE, [10], {0: 1, 7: 2}),
    # an activation that finished activating: a pump request alone; the head becomes Running (read-write), which keeps
    # the read-only record behind it waiting
    ("pump_only_after_activating", (VALID, 0, 0, 0), [(10, RW), (11, RO)], NONE, [(0, NONE)],
     [(10, 0, RW, RUN)], (VALID, SET, 1, 1, 1), 10, [11], {1: 1, 5: 1, 7: 2}),
    ("drain", (VALID, SET, 1, 1), [(10, RW), (11, RO)], 7, [(0, DRAIN), (0, 7)],
     [(10, 0, RW, DRAINED), (11, 0, RO, DRAINED)], (VALID, 0, 0, 0, 0), NONE, [], {0: 1, 2: 1, 6: 2, 7: 1}),
    # two completions against in_flight 0: both counters saturate at 0, the activation is counted, the pump runs once
    ("underflow", (VALID, SET, 1, 0), [(10, RW)], 7, [(0, 7), (0, 99)],
     [(10, 0, RW, RUN)], (VALID, SET, 1, 1, 0), 10, [], {0: 2, 4: 1, 5: 1, 7: 1}),
    ("handle_out_of_range", (VALID, SET, 1, 1), [(10, RW)], 7, [(2, 7), (L.NO_ACT, NONE), (0x80000000, DRAIN)],
     [], (VALID, SET, 1, 1, 1), 7, [10], {3: 3, 7: 2}),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_derived_completion(case):
    name, ent, waiting, rt, recs, e_out, e_entry, e_rt, e_left, e_counts = case
    w = world(ent, waiting, rt)
    cov = Counter()
    cact, ctok = [a for a, _ in recs], [t for _, t in recs]
    for fn in (lambda: Q.complete(w, cact, ctok, cov), lambda: Q.complete_closed_form(w, cact, ctok)):
        nw, out, counts = fn()
        assert out == e_out
        assert entry(nw) == e_entry and int(nw.running_tok[0]) == e_rt
        assert nw.tok[nw.off[0]:nw.off[1]].tolist() == e_left
        assert list(counts) == [e_counts.get(i, 0) for i in range(8)]
        # the bystander keeps its entry, its record and its Running
        assert entry(nw, 1) == (VALID, SET, 1, 1, 1) and nw.tok[nw.off[1]:nw.off[2]].tolist() == [500]
        assert int(nw.running_tok[1]) == 600
        nw.check_invariants()
    assert cov[name] > 0, cov


def test_hand_derived_append():
    """Bucket 0: a response, then the first RUN (token 21) behind it, then a second RUN and two ENQUEUEs; bucket 1 already
    has Running and a waiting record; bucket 2 (= n_act) is unresolved."""
    s = np.zeros(2, Q.STATE_DTYPE)
    s["state"] = VALID
    w = Q.World(s, [0, 0, 1], [500], [RW], [NONE, 600])
    act = [0, 1, 0, 2, 0, 0, 1, 0]
    disp = [L.ADM_RESPONSE, L.ADM_RUN, L.ADM_RUN, L.ADM_ENQUEUE, L.ADM_RUN, L.ADM_ENQUEUE, L.ADM_ENQUEUE, L.ADM_ENQUEUE]
    tok = [20, 30, 21, 40, 22, 23, 31, 24]
    mf = [L.MF_RESPONSE, RO, RO, RW, RO, RW, AI, RO]
    cov = Counter()
    for nw in (Q.append(w, act, tok, mf, disp, cov), Q.append_ref(w, act, tok, mf, disp)):
        assert nw.off.tolist() == [0, 2, 4]
        assert nw.tok.tolist() == [23, 24, 500, 31] and nw.mflags.tolist() == [RW, RO, RW, AI]
        assert nw.running_tok.tolist() == [21, 600]
        assert np.array_equal(nw.state, w.state)
    assert cov["running_tok_from_later_run"] == 1


def test_running_first_is_a_real_choice():
    """Running = R (read-only, token 7), another read-only request B (token 8) running, waiting [W1 read-only, W2
    read-write].  B then R: W1 runs beside R, then Running == null lets W2 in ("we might be over-writing an already
    running read only request", Dispatcher.cs:680).  R then B: W1 becomes Running and W2 waits.  The model is R first,
    whatever the batch order."""
    w = world((VALID, SET | SRO, 2, 2), [(10, RO), (11, RW)], 7)
    b_then_r, out1, _ = Q.complete(w, [0], [8])
    b_then_r, out2, _ = Q.complete(b_then_r, [0], [7])
    assert out1 + out2 == [(10, 0, RO, RUN), (11, 0, RW, RUN)]
    assert entry(b_then_r) == (VALID, SET, 2, 2, 0) and int(b_then_r.running_tok[0]) == 11
    r_then_b, out1, _ = Q.complete(w, [0], [7])
    r_then_b, out2, _ = Q.complete(r_then_b, [0], [8])
    assert out1 + out2 == [(10, 0, RO, RUN)]
    assert entry(r_then_b) == (VALID, SET | SRO, 1, 1, 1) and int(r_then_b.running_tok[0]) == 10
    assert not b_then_r.same(r_then_b)
    for cact, ctok in (([0, 0], [8, 7]), ([0, 0], [7, 8])):
        for fn in (Q.complete, Q.complete_closed_form):
            nw, out, _ = fn(w, cact, ctok)
            assert nw.same(r_then_b) and out == [(10, 0, RO, RUN)]


def _random_cases(count=320):
    for i in range(count):
        rng = np.random.default_rng([i, 4242])
        n_act = int(rng.integers(1, 9))
        w = Q.consistent_world(rng, n_act, max_wait=5)
        m = int(rng.integers(0, 4 * n_act + 1))
        cact, ctok = Q.random_completions(rng, w, m, p_pump=0.1, p_drain=0.07, respect_counts=i % 5 != 0)
        yield rng, w, cact, ctok


def test_closed_form_equals_the_loop_and_the_order_of_the_rest_does_not_matter():
    seen = Counter()
    for rng, w, cact, ctok in _random_cases():
        e_w, e_out, e_counts = Q.complete(w, cact, ctok, seen)
        c_w, c_out, c_counts = Q.complete_closed_form(w, cact, ctok)
        assert c_w.same(e_w) and c_out == e_out and list(c_counts) == list(e_counts)
        e_w.check_invariants()
        for perm in (lambda r: r[::-1], lambda r: [r[j] for j in rng.permutation(len(r))]):
            p_w, p_out, p_counts = Q.complete(w, cact, ctok, perm=perm)
            assert p_w.same(e_w) and p_out == e_out and list(p_counts) == list(e_counts)
        # the batch order of the records does not matter either
        p = rng.permutation(len(cact))
        p_w, p_out, p_counts = Q.complete(w, cact[p], ctok[p])
        assert p_w.same(e_w) and p_out == e_out and list(p_counts) == list(e_counts)
    for name in ("completion_not_running", "pump_stopped_by_head", "drain", "underflow", "read_only_run"):
        assert seen[name] > 0, name


def test_append_in_numpy_equals_the_loop():
    for i in range(60):
        rng = np.random.default_rng([i, 77])
        n_act = int(rng.integers(1, 9))
        w = Q.consistent_world(rng, n_act, max_wait=4)
        n = int(rng.integers(0, 60))
        act = rng.integers(0, n_act + 2, n).astype(np.uint32)
        fl = A.random_flags(rng, n, p_ro=0.3)
        disp, st, _ = A.admit(act, fl, w.state, n_act, 6, 3)
        tok = (0x50000000 + np.arange(n)).astype(np.uint32)
        assert Q.append_ref(w, act, tok, fl, disp).same(Q.append(w, act, tok, fl, disp))


def test_exports_constants_and_view_size_match_the_header():
    lib = L.load()
    text = open(os.path.join(ROOT, "include", "orleans_route.h")).read()
    for name in ("orl_waitq_create", "orl_waitq_destroy", "orl_waitq_view_get", "orl_waitq_append_device",
                 "orl_complete_device"):
        assert name in L.EXPORTED and hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, text)
    defs = {k: int(v, 0) for k, v in re.findall(r"#define (ORL_(?:TOK|WQ)_[A-Z_]+) (0x[0-9A-Fa-f]+|\d+)u", text)}
    assert defs == {"ORL_TOK_NONE": L.TOK_NONE, "ORL_TOK_DRAIN": L.TOK_DRAIN, "ORL_WQ_RUN": L.WQ_RUN,
                    "ORL_WQ_DRAINED": L.WQ_DRAINED}
    assert (L.TOK_NONE, L.TOK_DRAIN, L.WQ_RUN, L.WQ_DRAINED) == (0xFFFFFFFF, 0xFFFFFFFE, 0, 1)
    assert re.search(r"#define ORL_ABI_VERSION 1u", text) and L.ABI_VERSION == 1
    m = re.search(r"typedef struct orl_waitq_view \{(.*?)\} orl_waitq_view;", text, re.S)
    fields = re.findall(r"(?:const )?(?:uint8_t|uint32_t|uint64_t)\* (\w+);", m.group(1))
    assert fields == [f for f, _ in L.orl_waitq_view._fields_] and len(fields) == 11
    assert C.sizeof(L.orl_waitq_view) == 11 * C.sizeof(C.c_void_p) == 88
    assert (L.CMP_COMPLETIONS, L.CMP_PUMPS, L.CMP_DRAINS, L.CMP_IGNORED, L.CMP_UNDERFLOWS, L.CMP_RUN, L.CMP_DRAINED,
            L.CMP_WAITING) == tuple(range(8))


def test_host_only_context_refuses_the_waiting_queue():
    eng = GrainDirectoryEngine(n_act=16, dir_capacity=16, device=-1)
    try:
        z, b = np.zeros(4, np.uint32), np.zeros(4, np.uint8)
        off = np.zeros(18, np.uint32)
        for call in (lambda: eng.waitq_create(64),
                     lambda: eng.waitq_append_device(None, z, b, 4, z, off, b),
                     lambda: eng.complete_device(None, z, z, 4, z, off, np.zeros(16, L.ACT_STATE_DTYPE))):
            with pytest.raises(OrleansRouteError) as e:
                call()
            assert e.value.code == L.E_STATE
    finally:
        eng.close()


# ---- the GPU file's scenarios, through the model alone --------------------------------------------------------------------
def test_gpu_scenarios_reach_every_counter():
    cov = Counter()
    names = set()
    for sc in Q.all_scenarios():
        assert sc.name not in names
        names.add(sc.name)
        sc.world.check_invariants()
        disp, _, w1, w2, out, counts = sc.expect(cov)
        w1.check_invariants()
        assert len(w1.tok) <= sc.capacity
        assert counts[:4].sum() == len(sc.cact) and counts[L.CMP_RUN] + counts[L.CMP_DRAINED] == len(out)
        assert counts[L.CMP_WAITING] == len(w2.tok) == len(w1.tok) - len(out)
        if not counts[L.CMP_UNDERFLOWS]:
            w2.check_invariants()
        assert Q.append_ref(sc.world, sc.act, sc.tok, sc.mflags, disp).off.tolist() == w1.off.tolist()
    for name in Q.COUNTERS:
        assert cov[name] > 0, (name, dict(cov))


def test_admit_append_complete_chained_keep_the_table_and_the_store_together():
    """After any sequence of admit / append / complete, `waiting` in the table equals the store's segment length for every
    activation and running_tok != NONE <=> RUNNING_SET."""
    w, rounds, (hard, hsw) = Q.chain_rounds()
    w.check_invariants()
    for act, fl, seed in rounds:
        disp, st, _ = A.admit(act, fl, w.state, w.n_act, hard, hsw)
        tok = (0x50000000 + np.arange(len(act))).astype(np.uint32)
        w = Q.append(w, act, tok, fl, disp)
        w.state = st
        w.check_invariants()
        assert Q.append_ref(w, [], [], [], []).same(w)  # an empty batch changes nothing
        cact, ctok = Q.chain_completions(w, seed)
        nw, out, counts = Q.complete(w, cact, ctok)
        c_w, c_out, c_counts = Q.complete_closed_form(w, cact, ctok)
        assert c_w.same(nw) and c_out == out and list(c_counts) == list(counts)
        assert counts[L.CMP_UNDERFLOWS] == 0 and len(out) > 0
        nw.check_invariants()
        w = nw
