"""Admission without a GPU: the sequential model (admission_ref.admit) pinned on hand-derived cases, one per rule and per
coverage counter, with dispositions and end state written out by hand from the cited reference lines; the closed form
the kernels compute held to the model; the new export, constants and struct size against the header; the host-only
refusal; and the GPU file's scenarios run through the model alone, which must make every counter non-zero.  Every
comparison is exact."""
import ctypes as C
import os
import re
from collections import Counter

import numpy as np
import pytest

import admission_ref as A
from orleans_amd import _lib as L
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RUN, ENQ, RESP, OVER, INV, NONE, EXP, UNRES = range(8)
REQ, RSP, OW = L.MF_REQUEST, L.MF_RESPONSE, L.MF_ONE_WAY
RO, AI, EXPIRED = L.MF_READ_ONLY, L.MF_ALWAYS_INTERLEAVE, L.MF_EXPIRED
SET, SET_RO, REENT, SW = L.ACTF_RUNNING_SET, L.ACTF_RUNNING_SET | L.ACTF_RUNNING_RO, L.ACTF_REENTRANT, L.ACTF_STATELESS


def _one(state, flags, num_running, in_flight, waiting, msgs, hard=0, hard_sw=0, cov=None):
    """One activation (handle 0) and its messages -> (dispositions, (flags, num_running, in_flight, waiting) after)."""
    s = np.zeros(1, A.STATE_DTYPE)
    s[0] = (state, flags, 0, num_running, in_flight, waiting)
    d, out, counts = A.admit(np.zeros(len(msgs), np.uint32), np.array(msgs, np.uint8), s, 1, hard, hard_sw, cov)
    assert out[0]["state"] == state and counts.sum() == len(msgs)
    d2, out2, counts2 = A.admit_closed_form(np.zeros(len(msgs), np.uint32), np.array(msgs, np.uint8), s, 1, hard, hard_sw)
    assert list(d2) == list(d) and out2.tobytes() == out.tobytes() and list(counts2) == list(counts)
    return list(d), (int(out[0]["flags"]), int(out[0]["num_running"]), int(out[0]["in_flight"]), int(out[0]["waiting"]))


# ---- one case per rule ------------------------------------------------------------------------------------------------
def test_rule1_overloaded_every_direction():
    """c = 2 + 2 > L = 3 on a VALID activation: IncomingMessageAgent.cs:153-161 rejects before anything else is looked
    at, a response and an expired message included; nothing changes."""
    cov = Counter()
    assert _one(L.ACT_VALID, SET, 1, 2, 2, [REQ, RSP, OW, EXPIRED, AI], 3, cov=cov) == ([OVER] * 5, (SET, 1, 2, 2))
    assert cov["rule1_on_response"] == 1
    # c == L is not over the limit, and a limit <= 0 is none
    assert _one(L.ACT_VALID, SET, 1, 2, 1, [RSP], 3) == ([RESP], (SET, 1, 2, 1))
    assert _one(L.ACT_VALID, SET, 1, 200, 100, [RSP, REQ], 0) == ([RESP, ENQ], (SET, 1, 200, 101))
    assert _one(L.ACT_VALID, SET, 1, 200, 100, [REQ], -1) == ([ENQ], (SET, 1, 200, 101))


def test_rule1_is_for_valid_activations_only():
    """CheckOverloaded is reached for state == Valid alone (IncomingMessageAgent.cs:153): over the limit, an ACTIVATING
    activation still takes its response, and rule 7 rejects its request."""
    assert _one(L.ACT_ACTIVATING, 0, 0, 5, 5, [RSP, REQ], 3) == ([RESP, OVER], (0, 0, 5, 5))


def test_rule2_expired_before_the_state_is_looked_at():
    for st in (L.ACT_CREATE, L.ACT_VALID, L.ACT_INVALID, L.ACT_ABSENT, 7):
        assert _one(st, 0, 0, 0, 0, [EXPIRED | REQ, EXPIRED | RSP]) == ([EXP, EXP], (0, 0, 0, 0)), st


def test_rule3_absent_and_larger_state_values():
    cov = Counter()
    for st in (L.ACT_ABSENT, 6, 255):
        assert _one(st, 0, 0, 0, 0, [REQ, RSP, OW], 1, cov=cov) == ([NONE] * 3, (0, 0, 0, 0))
    assert cov["state_absent"] == 9


def test_rule4_and_5_responses_and_the_invalid_activation():
    cov = Counter()
    assert _one(L.ACT_INVALID, 0, 0, 0, 0, [RSP, REQ, OW], cov=cov) == ([INV, INV, INV], (0, 0, 0, 0))
    assert _one(L.ACT_VALID, SET, 1, 1, 0, [RSP, RSP | RO]) == ([RESP, RESP], (SET, 1, 1, 0))
    assert _one(L.ACT_DEACTIVATING, 0, 0, 0, 0, [RSP], cov=cov) == ([RESP], (0, 0, 0, 0))
    assert cov["state_invalid"] == 3 and cov["state_deactivating"] == 1


def test_rule6_idle_activation_runs_the_first_request_and_records_it():
    """num_running == 0: the request runs, Running = it (read-write); the next request may not interleave, the
    always-interleave one may (Dispatcher.cs:316-338)."""
    cov = Counter()
    assert _one(L.ACT_VALID, 0, 0, 0, 0, [REQ, REQ, REQ | AI, OW | RO], cov=cov) == ([RUN, ENQ, RUN, ENQ], (SET, 2, 2, 2))
    assert cov["always_interleave_past_rw"] == 1 and cov["read_only_interleave"] == 0


def test_rule6_read_only_interleave():
    """Running read-only: read-only requests interleave, a read-write one waits; RecordRunning keeps the first."""
    cov = Counter()
    assert _one(L.ACT_VALID, 0, 0, 0, 0, [REQ | RO, REQ | RO, REQ, OW | RO], cov=cov) == ([RUN, RUN, ENQ, RUN], (SET_RO, 3, 3, 1))
    assert cov["read_only_interleave"] == 2
    assert _one(L.ACT_VALID, SET_RO, 1, 1, 0, [REQ | RO, REQ]) == ([RUN, ENQ], (SET_RO, 2, 2, 1))
    assert _one(L.ACT_VALID, SET, 1, 1, 0, [REQ | RO]) == ([ENQ], (SET, 1, 1, 1))  # Running read-write


def test_rule6_reentrant_runs_everything():
    assert _one(L.ACT_VALID, SET | REENT, 3, 3, 0, [REQ, OW, REQ | RO]) == ([RUN, RUN, RUN], (SET | REENT, 6, 6, 0))


def test_rule6_running_unset_with_num_running():
    """Running == null while numRunning > 0: the first request is accepted by the !RUNNING_SET clause and becomes
    Running with its own read-only bit, which replaces a stale RUNNING_RO; it need not be the bucket's first message."""
    cov = Counter()
    assert _one(L.ACT_VALID, L.ACTF_RUNNING_RO, 2, 2, 0, [RSP, EXPIRED, REQ, REQ | RO], cov=cov) == (
        [RESP, EXP, RUN, ENQ], (SET, 3, 3, 1))
    assert cov["running_set_by_later_request"] == 1 and cov["unset_running_with_num_running"] == 1
    assert _one(L.ACT_VALID, 0, 2, 2, 0, [REQ | RO, REQ | RO, REQ]) == ([RUN, RUN, ENQ], (SET_RO, 4, 4, 1))


def test_rule6_num_running_zero_with_running_set():
    """numRunning == 0 accepts whatever Running says; Running stays (RecordRunning: Running ??= message)."""
    assert _one(L.ACT_VALID, SET_RO, 0, 0, 0, [REQ, REQ, REQ | RO]) == ([RUN, ENQ, RUN], (SET_RO, 2, 2, 1))


def test_rule7_reject_at_the_limit_and_an_alpha_accepted_there():
    """L = 3, c0 = 1, Running read-only.  Two read-write requests wait (c = 2, 3); the third finds c + 1 = L + 1 and is
    rejected (EnqueueRequest :401-427); a read-only request still runs at c == L (c = 4); from then on rule 1 rejects
    every message, the response and the read-only request too."""
    cov = Counter()
    assert _one(L.ACT_VALID, SET_RO, 1, 1, 0, [REQ, REQ, REQ, REQ | RO, RSP, REQ | RO, REQ], 3, cov=cov) == (
        [ENQ, ENQ, OVER, RUN, OVER, OVER, OVER], (SET_RO, 2, 2, 2))
    assert (cov["rule7_reject_at_limit"], cov["alpha_at_limit"], cov["rule1_on_response"],
            cov["rule1_on_alpha_after_saturation"]) == (1, 1, 1, 1)


def test_rule7_counts_rejected_requests_as_nothing():
    """A rejected request changes no counter: after the rejections a response is still handed on (c stays L)."""
    assert _one(L.ACT_VALID, SET, 1, 1, 0, [REQ, REQ, REQ, RSP], 2) == ([ENQ, OVER, OVER, RESP], (SET, 1, 1, 1))


def test_rule7_on_activating_states_has_no_dispatcher_count():
    """Not VALID: no closure count, so a request is enqueued up to c == L (c + 0 > L rejects)."""
    cov = Counter()
    for st, name in ((L.ACT_CREATE, "state_create"), (L.ACT_ACTIVATING, "state_activating"),
                     (L.ACT_DEACTIVATING, "state_deactivating")):
        assert _one(st, REENT, 0, 1, 0, [REQ, REQ | AI, OW, REQ, RSP], 2, cov=cov) == (
            [ENQ, ENQ, OVER, OVER, RESP], (REENT, 0, 1, 2))
        assert cov[name] == 5


def test_stateless_limit_is_selected_by_the_flag():
    cov = Counter()
    assert _one(L.ACT_VALID, SET | SW, 1, 1, 0, [REQ, REQ], 100, 1, cov=cov) == ([OVER, OVER], (SET | SW, 1, 1, 0))
    assert cov["stateless_limit"] == 2
    assert _one(L.ACT_VALID, SET, 1, 1, 0, [REQ, REQ], 100, 1) == ([ENQ, ENQ], (SET, 1, 1, 2))


def test_unresolved_bucket_reads_no_state():
    s = np.zeros(2, A.STATE_DTYPE)
    s["state"] = L.ACT_VALID
    cov = Counter()
    d, out, counts = A.admit(np.array([2, 0x80000000, A.NO_ACT, 1], np.uint32), np.array([REQ, RSP, EXPIRED, REQ], np.uint8),
                             s, 2, cov=cov)
    assert list(d) == [UNRES, UNRES, UNRES, RUN] and cov["unresolved"] == 3
    assert list(counts) == [1, 0, 0, 0, 0, 0, 0, 3]
    assert out[0].tobytes() == s[0].tobytes() and tuple(out[1]) == (L.ACT_VALID, SET, 0, 1, 1, 0)


def test_messages_of_two_activations_do_not_see_each_other():
    s = np.zeros(2, A.STATE_DTYPE)
    s["state"] = L.ACT_VALID
    d, out, _ = A.admit(np.array([0, 1, 0, 1], np.uint32), np.array([REQ, REQ | RO, REQ, REQ | RO], np.uint8), s, 2)
    assert list(d) == [RUN, RUN, ENQ, RUN]
    assert tuple(out[0]) == (L.ACT_VALID, SET, 0, 1, 1, 1) and tuple(out[1]) == (L.ACT_VALID, SET_RO, 0, 2, 2, 0)


# ---- the closed form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_closed_form_equals_the_loop_on_random_batches(seed):
    """Small tables and tight limits, so that every bucket is long against its limit."""
    rng = np.random.default_rng(seed)
    for _ in range(60):
        n_act, n = int(rng.integers(1, 6)), int(rng.integers(0, 80))
        act = rng.integers(0, n_act + 1, n).astype(np.uint32)
        fl = A.random_flags(rng, n, p_ro=0.4, p_ai=0.15, p_exp=0.1)
        s = A.random_state(rng, n_act, p_valid=0.6, max_count=3)
        hard, hsw = int(rng.integers(-1, 9)), int(rng.integers(0, 5))
        d, out, c = A.admit(act, fl, s, n_act, hard, hsw)
        d2, out2, c2 = A.admit_closed_form(act, fl, s, n_act, hard, hsw)
        assert list(d) == list(d2) and out.tobytes() == out2.tobytes() and list(c) == list(c2), (seed, act, fl, s, hard, hsw)


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_export_constants_and_struct_size_match_the_header():
    lib = L.load()
    text = open(os.path.join(ROOT, "include", "orleans_route.h")).read()
    assert "orl_admit_device" in L.EXPORTED and hasattr(lib, "orl_admit_device")
    assert re.search(r"\bint orl_admit_device\(", text)
    defs = {k: int(v, 0) for k, v in re.findall(r"#define (ORL_(?:ACT|ACTF|MF|ADM)_[A-Z_]+) (0x[0-9A-Fa-f]+|\d+)u", text)}
    assert defs == {
        "ORL_ACT_CREATE": L.ACT_CREATE, "ORL_ACT_ACTIVATING": L.ACT_ACTIVATING, "ORL_ACT_VALID": L.ACT_VALID,
        "ORL_ACT_DEACTIVATING": L.ACT_DEACTIVATING, "ORL_ACT_INVALID": L.ACT_INVALID, "ORL_ACT_ABSENT": L.ACT_ABSENT,
        "ORL_ACTF_REENTRANT": L.ACTF_REENTRANT, "ORL_ACTF_RUNNING_SET": L.ACTF_RUNNING_SET,
        "ORL_ACTF_RUNNING_RO": L.ACTF_RUNNING_RO, "ORL_ACTF_STATELESS": L.ACTF_STATELESS,
        "ORL_MF_DIR_MASK": L.MF_DIR_MASK, "ORL_MF_REQUEST": L.MF_REQUEST, "ORL_MF_RESPONSE": L.MF_RESPONSE,
        "ORL_MF_ONE_WAY": L.MF_ONE_WAY, "ORL_MF_READ_ONLY": L.MF_READ_ONLY,
        "ORL_MF_ALWAYS_INTERLEAVE": L.MF_ALWAYS_INTERLEAVE, "ORL_MF_EXPIRED": L.MF_EXPIRED,
        "ORL_ADM_RUN": L.ADM_RUN, "ORL_ADM_ENQUEUE": L.ADM_ENQUEUE, "ORL_ADM_RESPONSE": L.ADM_RESPONSE,
        "ORL_ADM_OVERLOADED": L.ADM_OVERLOADED, "ORL_ADM_INVALID": L.ADM_INVALID, "ORL_ADM_NONEXISTENT": L.ADM_NONEXISTENT,
        "ORL_ADM_EXPIRED": L.ADM_EXPIRED, "ORL_ADM_UNRESOLVED": L.ADM_UNRESOLVED}
    assert (L.ACT_CREATE, L.ACT_ACTIVATING, L.ACT_VALID, L.ACT_DEACTIVATING, L.ACT_INVALID, L.ACT_ABSENT) == (0, 1, 2, 3, 4, 5)
    assert (L.ADM_RUN, L.ADM_ENQUEUE, L.ADM_RESPONSE, L.ADM_OVERLOADED, L.ADM_INVALID, L.ADM_NONEXISTENT, L.ADM_EXPIRED,
            L.ADM_UNRESOLVED) == (RUN, ENQ, RESP, OVER, INV, NONE, EXP, UNRES)
    # sizeof(orl_act_state) == 16, field by field as the header declares them
    m = re.search(r"typedef struct orl_act_state \{(.*?)\} orl_act_state;", text, re.S)
    fields = re.findall(r"(uint8_t|uint16_t|uint32_t) (\w+);", m.group(1))
    size = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4}
    assert [(f, size[t]) for t, f in fields] == [(nm, L.ACT_STATE_DTYPE[nm].itemsize) for nm in L.ACT_STATE_DTYPE.names]
    assert [L.ACT_STATE_DTYPE.fields[nm][1] for nm in L.ACT_STATE_DTYPE.names] == [0, 1, 2, 4, 8, 12]
    assert L.ACT_STATE_DTYPE.itemsize == 16 and C.sizeof(L.orl_admit_limits) == 8
    assert re.search(r"typedef struct orl_admit_limits \{\s*int32_t hard;\s*int32_t hard_stateless;\s*\} orl_admit_limits;", text)
    assert lib.orl_abi_version() == L.ABI_VERSION == 1


def test_host_only_context_refuses_admission():
    eng = GrainDirectoryEngine(n_act=16, dir_capacity=16, device=-1)
    try:
        z = np.zeros(4, np.uint32)
        with pytest.raises(OrleansRouteError) as e:
            eng.admit_device(z, np.zeros(4, np.uint8), 4, z, np.zeros(18, np.uint32), np.zeros(16, L.ACT_STATE_DTYPE),
                             np.zeros(4, np.uint8))
        assert e.value.code == L.E_STATE
    finally:
        eng.close()


# ---- the GPU file's scenarios, through the model alone --------------------------------------------------------------------
def test_gpu_scenarios_reach_every_counter():
    cov = Counter()
    names = set()
    for sc in A.all_scenarios():
        assert sc.name not in names
        names.add(sc.name)
        d, out, counts = sc.expect(cov)
        assert len(d) == sc.n and counts.sum() == sc.n
    n_act, s, batches, (hard, hsw) = A.chain_batches()
    for step, (act, fl) in enumerate(batches):
        _, s, _ = A.admit(act, fl, s, n_act, hard, hsw, cov)
        s = A.chain_complete(s, step)
    assert [c for c in A.COUNTERS if cov[c] == 0] == []
    assert set(A.SHAPE_N) == {0, 1, 63, 64, 65, 257, 4097, 40_001} and set(A.SHAPE_N_ACT) == {1, 5, 5000, 1 << 20}
