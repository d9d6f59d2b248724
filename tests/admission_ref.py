"""Admission (orl_admit_device): the reference's per-message decision as a sequential loop over plain Python state, the
coverage counters of that loop, and the seeded scenario builders that tests/test_gpu_admission.py runs on the device (no
GPU needed here; tests/test_admission_ref.py pins the loop on hand-derived cases and holds the builders to the counters).

The loop is the project's "reference called in batch order" rule: for each message, in arrival order,
IncomingMessageAgent.ReceiveMessage (IncomingMessageAgent.cs:144-181) and then its Dispatcher.ReceiveMessage closure
(Dispatcher.cs:78-204) run before the next message of the same activation; no request completes inside a batch.
"""
from collections import Counter

import numpy as np

from orleans_amd import _lib as L

NO_ACT = 0xFFFFFFFF
STATE_DTYPE = L.ACT_STATE_DTYPE
N_CODES = 8

COUNTERS = ("rule1_on_response", "rule1_on_alpha_after_saturation", "rule7_reject_at_limit", "alpha_at_limit",
            "running_set_by_later_request", "unset_running_with_num_running", "read_only_interleave",
            "always_interleave_past_rw", "state_create", "state_activating", "state_deactivating", "state_invalid",
            "state_absent", "stateless_limit", "unresolved")
_STATE_COUNTER = {L.ACT_CREATE: "state_create", L.ACT_ACTIVATING: "state_activating",
                  L.ACT_DEACTIVATING: "state_deactivating", L.ACT_INVALID: "state_invalid"}


def admit(act, mflags, state, n_act, hard=0, hard_stateless=0, cov=None):
    """(disp uint8[n], state after, counts uint64[8]) of one batch.  state: STATE_DTYPE[n_act], not modified.
    cov: a Counter that receives COUNTERS."""
    act = np.ascontiguousarray(act, np.uint32)
    mflags = np.ascontiguousarray(mflags, np.uint8)
    n = len(act)
    assert len(mflags) == n and len(state) == n_act
    cov = Counter() if cov is None else cov
    out = state.copy()
    disp = np.zeros(n, np.uint8)
    live = {}        # handle -> [state, flags, num_running, in_flight, waiting] of the activations the batch touches
    seen = set()     # activations that got an earlier message of this batch
    saturated = set()  # activations an accepted request took to c == L + 1 in this batch
    for i in range(n):
        a, f = int(act[i]), int(mflags[i])
        if a >= n_act:  # stage 4's bucket n_act: a new placement, the host activates it
            disp[i] = L.ADM_UNRESOLVED
            cov["unresolved"] += 1
            continue
        s = live.get(a)
        if s is None:
            r = state[a]
            s = live[a] = [int(r["state"]), int(r["flags"]), int(r["num_running"]), int(r["in_flight"]), int(r["waiting"])]
        st, fl = min(s[0], L.ACT_ABSENT), s[1]
        later = a in seen
        seen.add(a)
        if st != L.ACT_VALID:
            cov[_STATE_COUNTER.get(st, "state_absent")] += 1
        stateless = bool(fl & L.ACTF_STATELESS)
        lim = hard_stateless if stateless else hard  # ActivationData.cs:563-575
        c = s[3] + s[4]  # GetRequestCount: EnqueuedOnDispatcherCount is 0 between messages
        direction = f & L.MF_DIR_MASK
        read_only, interleave, expired = bool(f & L.MF_READ_ONLY), bool(f & L.MF_ALWAYS_INTERLEAVE), bool(f & L.MF_EXPIRED)
        response = direction == L.MF_RESPONSE
        may_accept = st == L.ACT_VALID and (                                     # Dispatcher.cs:316-338
            s[2] == 0 or bool(fl & L.ACTF_REENTRANT) or interleave or not fl & L.ACTF_RUNNING_SET
            or (bool(fl & L.ACTF_RUNNING_RO) and read_only))
        # 1. IncomingMessageAgent.cs:153-161, ActivationData.CheckOverloaded :522-561: every direction
        if st == L.ACT_VALID and lim > 0 and c > lim:
            disp[i] = L.ADM_OVERLOADED
            cov["rule1_on_response"] += response
            cov["rule1_on_alpha_after_saturation"] += (a in saturated and not expired and not response and may_accept)
            cov["stateless_limit"] += stateless
            continue
        if expired:                                                              # 2. Dispatcher.cs:82-88
            disp[i] = L.ADM_EXPIRED
            continue
        if st == L.ACT_ABSENT:                                                   # 3. :132-197
            disp[i] = L.ADM_NONEXISTENT
            continue
        if response:                                                             # 4. :245-251
            disp[i] = L.ADM_INVALID if st == L.ACT_INVALID else L.ADM_RESPONSE
            continue
        if st == L.ACT_INVALID:                                                  # 5. :269-276
            disp[i] = L.ADM_INVALID
            continue
        if may_accept:                                                           # 6. HandleIncomingRequest
            disp[i] = L.ADM_RUN
            if lim > 0 and c == lim:
                cov["alpha_at_limit"] += 1
                saturated.add(a)
            if s[2] > 0 and not fl & L.ACTF_REENTRANT and fl & L.ACTF_RUNNING_SET:
                cov["read_only_interleave"] += (not interleave)
                cov["always_interleave_past_rw"] += (interleave and not fl & L.ACTF_RUNNING_RO)
            s[2] = (s[2] + 1) & 0xFFFFFFFF
            s[3] = (s[3] + 1) & 0xFFFFFFFF
            if not fl & L.ACTF_RUNNING_SET:                                      # RecordRunning keeps the first
                cov["running_set_by_later_request"] += later
                cov["unset_running_with_num_running"] += (s[2] > 1)
                s[1] = (fl & ~L.ACTF_RUNNING_RO) | L.ACTF_RUNNING_SET | (L.ACTF_RUNNING_RO if read_only else 0)
            continue
        # 7. EnqueueRequest :401-427: during the closure of a VALID activation EnqueuedOnDispatcherCount is 1
        if lim > 0 and c + (1 if st == L.ACT_VALID else 0) > lim:
            disp[i] = L.ADM_OVERLOADED
            cov["rule7_reject_at_limit"] += (st == L.ACT_VALID and c == lim)
            cov["stateless_limit"] += stateless
            continue
        disp[i] = L.ADM_ENQUEUE
        s[4] = (s[4] + 1) & 0xFFFFFFFF
    for a, s in live.items():
        out[a]["flags"], out[a]["num_running"], out[a]["in_flight"], out[a]["waiting"] = s[1], s[2], s[3], s[4]
    return disp, out, np.bincount(disp, minlength=N_CODES).astype(np.uint64)


# ---- scenario builders ---------------------------------------------------------------------------------------------
class Scenario:
    """One batch: handles, message flags, the start state table and the limits."""

    def __init__(self, name, n_act, act, mflags, state, hard=0, hard_stateless=0):
        self.name, self.n_act, self.hard, self.hard_stateless = name, int(n_act), int(hard), int(hard_stateless)
        self.act = np.ascontiguousarray(act, np.uint32)
        self.mflags = np.ascontiguousarray(mflags, np.uint8)
        self.state = state
        assert len(self.act) == len(self.mflags) and len(state) == n_act and state.dtype == STATE_DTYPE

    @property
    def n(self):
        return len(self.act)

    def expect(self, cov=None):
        return admit(self.act, self.mflags, self.state, self.n_act, self.hard, self.hard_stateless, cov)


SHAPE_N = (0, 1, 63, 64, 65, 257, 4097, 40_001)
SHAPE_N_ACT = (1, 5, 5000, 1 << 20)


def random_flags(rng, n, p_resp=0.1, p_ro=0.2, p_ai=0.05, p_exp=0.05, p_oneway=0.1):
    """Directions Request / Response / OneWay (and the unassigned 3, a request like OneWay), with the three bits."""
    u = rng.random(n)
    d = np.where(u < p_resp, L.MF_RESPONSE, np.where(u < p_resp + p_oneway, L.MF_ONE_WAY, L.MF_REQUEST)).astype(np.uint8)
    d[rng.random(n) < 0.01] = 3
    return (d | np.where(rng.random(n) < p_ro, L.MF_READ_ONLY, 0).astype(np.uint8)
            | np.where(rng.random(n) < p_ai, L.MF_ALWAYS_INTERLEAVE, 0).astype(np.uint8)
            | np.where(rng.random(n) < p_exp, L.MF_EXPIRED, 0).astype(np.uint8))


def random_state(rng, n_act, p_valid=0.7, max_count=4):
    s = np.zeros(n_act, STATE_DTYPE)
    s["state"] = np.where(rng.random(n_act) < p_valid, L.ACT_VALID, rng.integers(0, 7, n_act)).astype(np.uint8)
    s["flags"] = rng.integers(0, 16, n_act).astype(np.uint8)
    s["num_running"] = rng.integers(0, 3, n_act)
    s["in_flight"] = rng.integers(0, max_count + 1, n_act)
    s["waiting"] = rng.integers(0, max_count + 1, n_act)
    return s


def shape_scenario(n, n_act, seed=0):
    """Random handles (5 % unresolved, a hot handle holding a fifth of the batch), flags and states; limits 6 and 3."""
    rng = np.random.default_rng([n, n_act, seed])
    act = rng.integers(0, n_act, n).astype(np.uint32)
    act[rng.random(n) < 0.2] = n_act // 2
    act[rng.random(n) < 0.05] = rng.choice(np.array([n_act, 0x80000000, NO_ACT], np.uint32), 1)[0]
    return Scenario(f"shape-n{n}-a{n_act}", n_act, act, random_flags(rng, n), random_state(rng, n_act), 6, 3)


def _valid(n_act, handle, flags=0, num_running=1, in_flight=0, waiting=0):
    s = np.zeros(n_act, STATE_DTYPE)
    s["state"] = L.ACT_ABSENT
    s[handle] = (L.ACT_VALID, flags, 0, num_running, in_flight, waiting)
    return s


def one_bucket_scenarios(n):
    """The whole batch in one bucket (handle 1 of 3), Running a read-only request so that read-only requests are the
    alphas: L in {0, 1, 2}, and L - c0 at 2047, 2048, 2049 and n - 1 (c0 = 3)."""
    out = []
    rng = np.random.default_rng([n, 77])
    act = np.full(n, 1, np.uint32)
    fl = random_flags(rng, n, p_ro=0.3, p_ai=0.02, p_exp=0.03)
    busy = L.ACTF_RUNNING_SET | L.ACTF_RUNNING_RO
    for lim in (0, 1, 2):
        out.append(Scenario(f"one-n{n}-L{lim}", 3, act, fl, _valid(3, 1, busy, 1, 1 if lim == 2 else 0, 0), lim, 9))
    for t in (2047, 2048, 2049, max(n - 1, 0)):
        out.append(Scenario(f"one-n{n}-T{t}", 3, act, fl, _valid(3, 1, busy, 2, 2, 1), 3 + t, 9))
    # the same on a stateless worker, an activating one and one that is not running yet
    out.append(Scenario(f"one-n{n}-sw", 3, act, fl, _valid(3, 1, busy | L.ACTF_STATELESS, 1, 1, 0), 0, 5))
    s = _valid(3, 1, 0, 0, 2, 1)
    s[1]["state"] = L.ACT_ACTIVATING
    out.append(Scenario(f"one-n{n}-activating", 3, act, fl, s, 40, 9))
    out.append(Scenario(f"one-n{n}-idle", 3, act, fl, _valid(3, 1, 0, 0, 0, 0), 50, 9))
    return out


def boundary_scenario(k, d_start, d_len):
    """Handle 0 holds 2^k + d_start messages, so handle 1's bucket starts there; it holds 2^k + d_len; handle 2 holds 5.
    Arrival order shuffled.  Handle 1 saturates inside its bucket (limit 2^(k-1) over c0 = 1) after a late first request."""
    n0, n1 = (1 << k) + d_start, (1 << k) + d_len
    rng = np.random.default_rng([k, d_start + 1, d_len + 1])
    act = rng.permutation(np.concatenate([np.zeros(n0, np.uint32), np.ones(n1, np.uint32), np.full(5, 2, np.uint32)]))
    fl = random_flags(rng, len(act), p_ro=0.3)
    first = np.nonzero(act == 1)[0][:40]
    fl[first] = L.MF_RESPONSE  # handle 1's first request is not its first message
    s = np.zeros(4, STATE_DTYPE)
    s[0] = (L.ACT_VALID, L.ACTF_REENTRANT, 0, 0, 0, 0)
    s[1] = (L.ACT_VALID, 0, 0, 2, 1, 0)  # Running unset with num_running > 0
    s[2] = (L.ACT_DEACTIVATING, 0, 0, 0, 0, 0)
    s[3] = (L.ACT_ABSENT, 0, 0, 0, 0, 0)
    return Scenario(f"edge-k{k}-s{d_start}-l{d_len}", 4, act, fl, s, 1 << (k - 1), 0)


def late_first_request_scenario():
    """Handle 3's first request comes after 9000 responses and expired messages (more than four tiles of either kind);
    Running is unset, so that request sets it, read-only, and the read-only requests behind it interleave."""
    rng = np.random.default_rng(9000)
    n_pre, n_post = 9000, 600
    pre = np.where(rng.random(n_pre) < 0.5, L.MF_RESPONSE, L.MF_EXPIRED | L.MF_REQUEST).astype(np.uint8)
    post = random_flags(rng, n_post, p_resp=0.1, p_ro=0.4)
    post[0] = L.MF_REQUEST | L.MF_READ_ONLY
    other = random_flags(rng, 500)
    act = np.concatenate([np.full(n_pre + n_post, 3, np.uint32), rng.integers(0, 8, 500).astype(np.uint32)])
    fl = np.concatenate([pre, post, other])
    # interleave the other handles' messages without changing handle 3's own order
    pos = np.sort(rng.permutation(len(act))[: n_pre + n_post])
    a2, f2 = np.empty_like(act), np.empty_like(fl)
    rest = np.setdiff1d(np.arange(len(act)), pos)
    a2[pos], f2[pos] = act[: n_pre + n_post], fl[: n_pre + n_post]
    a2[rest], f2[rest] = act[n_pre + n_post:], fl[n_pre + n_post:]
    s = random_state(rng, 8)
    s[3] = (L.ACT_VALID, 0, 0, 1, 1, 0)
    return Scenario("late-first-request", 8, a2, f2, s, 400, 0)


def state_matrix_scenario():
    """Every state value 0..7 x every flag combination x num_running 0 / 2 on neighbouring handles, 14 messages each in
    shuffled arrival order, c0 from 0 to 5 against limits 6 (ordinary) and 3 (stateless)."""
    combos = [(st, fl, nr) for st in range(8) for fl in range(16) for nr in (0, 2)]
    n_act = len(combos)
    rng = np.random.default_rng(256)
    s = np.zeros(n_act, STATE_DTYPE)
    for h, (st, fl, nr) in enumerate(combos):
        s[h] = (st, fl, 0, nr, rng.integers(0, 4), rng.integers(0, 3))
    act = rng.permutation(np.repeat(np.arange(n_act, dtype=np.uint32), 14))
    return Scenario("state-matrix", n_act, act, random_flags(rng, len(act), p_ro=0.35, p_ai=0.1), s, 6, 3)


def alias_scenario():
    """The unresolved bucket under its aliases (n_act, n_act + 1, 0x80000000, 0xFFFFFFFE, ORL_NO_ACT) among resolved
    messages; the last bucket before it and the first one are occupied."""
    rng = np.random.default_rng(5)
    n_act, n = 300, 3000
    act = rng.integers(0, n_act, n).astype(np.uint32)
    act[:3] = (0, n_act - 1, n_act - 1)
    al = np.array([n_act, n_act + 1, 0x80000000, 0xFFFFFFFE, NO_ACT], np.uint32)
    m = rng.random(n) < 0.3
    act[m] = al[rng.integers(0, len(al), int(m.sum()))]
    return Scenario("aliases", n_act, act, random_flags(rng, n), random_state(rng, n_act), 6, 3)


def chain_batches():
    """Three batches over one table of 64 activations; chain_complete is the host's edit between them."""
    rng = np.random.default_rng(33)
    n_act = 64
    s0 = random_state(rng, n_act, p_valid=0.85)
    return n_act, s0, [(rng.integers(0, n_act + 4, n).astype(np.uint32), random_flags(rng, n, p_ro=0.3))
                       for n in (5000, 2049, 7000)], (8, 4)


def chain_complete(state, step):
    """The host between two batches: every third activation completes its requests (ResetRunning, the message pump
    taking one waiting request to run) and one deactivates."""
    s = state.copy()
    for h in range(step, len(s), 3):
        if s[h]["state"] != L.ACT_VALID:
            continue
        done = int(s[h]["num_running"])
        s[h]["in_flight"] -= min(done, int(s[h]["in_flight"]))
        s[h]["num_running"] = 0
        s[h]["flags"] &= ~(L.ACTF_RUNNING_SET | L.ACTF_RUNNING_RO) & 0xFF
        if s[h]["waiting"]:
            s[h]["waiting"] -= 1
            s[h]["in_flight"] += 1
            s[h]["num_running"] = 1
            s[h]["flags"] |= L.ACTF_RUNNING_SET
    s[step]["state"] = L.ACT_DEACTIVATING
    return s


def all_scenarios():
    """Every single-batch scenario of the GPU file, by name."""
    out = [shape_scenario(n, a) for n in SHAPE_N for a in SHAPE_N_ACT]
    for n in SHAPE_N:
        out += one_bucket_scenarios(n)
    out += [boundary_scenario(k, ds, dl) for k in range(6, 14) for ds in (-1, 0, 1) for dl in (-1, 0, 1)]
    out += [late_first_request_scenario(), state_matrix_scenario(), alias_scenario()]
    return out


# ---- the chunked regime of the one-workgroup tile scan ---------------------------------------------------------------
# More tiles (2048 positions) than the scan workgroup has threads (1024): a thread owns a chunk of ceil(tiles / 1024)
# aggregates.  Exactly 1024 tiles (chunk 1, every thread busy), 1025 (chunk 2, the last working thread owns one
# aggregate) and 2049 (chunk 3).  tests/test_source_layout.py holds these to the constants in tile_scan_dev.h.  The
# loop above is too slow at 4 M messages; the GPU tests compare these with admit_closed_form below.
CHUNK_N = (1024 * 2048, 1024 * 2048 + 1, 2048 * 2048 + 1)
CHUNK_STRIDE = 3000  # a bucket head every 3000 positions: 3000 k is a multiple of 2048 only for every 256th head


def chunk_scenarios(n):
    """Two batches of n messages.  `one`: the whole batch in one bucket (handle 1 of 3, as one_bucket_scenarios), which
    saturates after n // 2 requests: some 60 % into the batch, many chunks behind the bucket head at position 0.
    `stride`: bucket b holds the positions [3000 b, 3000 b + 3000), arrival order shuffled, random states, and limits that
    saturate a bucket half-way."""
    rng = np.random.default_rng([n, 1024])
    busy = L.ACTF_RUNNING_SET | L.ACTF_RUNNING_RO
    one = Scenario(f"chunk-one-n{n}", 3, np.full(n, 1, np.uint32), random_flags(rng, n, p_ro=0.3, p_ai=0.02, p_exp=0.03),
                   _valid(3, 1, busy, 2, 2, 1), 3 + n // 2, 9)
    n_act = (n + CHUNK_STRIDE - 1) // CHUNK_STRIDE
    act = rng.permutation((np.arange(n) // CHUNK_STRIDE).astype(np.uint32))
    stride = Scenario(f"chunk-stride-n{n}", n_act, act, random_flags(rng, n, p_ro=0.3), random_state(rng, n_act),
                      CHUNK_STRIDE // 2, CHUNK_STRIDE // 3)
    return [one, stride]


# ---- the closed form, vectorised per bucket: what the kernels compute, stated in numpy ------------------
def admit_closed_form(act, mflags, state, n_act, hard=0, hard_stateless=0):
    """The same three results from per-bucket prefix counts instead of the loop (tests hold it to admit)."""
    act = np.ascontiguousarray(act, np.uint32)
    mflags = np.ascontiguousarray(mflags, np.uint8)
    n = len(act)
    out = state.copy()
    disp = np.full(n, L.ADM_UNRESOLVED, np.uint8)
    key = np.minimum(act, np.uint32(n_act))
    order = np.argsort(key, kind="stable")
    bounds = np.searchsorted(key[order], np.arange(n_act + 1))
    for a in np.unique(key[key < n_act]):
        idx = order[bounds[a]:bounds[a + 1]] if a < n_act else order[bounds[a]:]
        f = mflags[idx]
        exp, resp = (f & L.MF_EXPIRED) != 0, (f & L.MF_DIR_MASK) == L.MF_RESPONSE
        req, ro, ai = ~exp & ~resp, (f & L.MF_READ_ONLY) != 0, (f & L.MF_ALWAYS_INTERLEAVE) != 0
        q = np.cumsum(req) - req
        r = state[a]
        st, fl = min(int(r["state"]), L.ACT_ABSENT), int(r["flags"])
        lim = hard_stateless if fl & L.ACTF_STATELESS else hard
        c0 = int(r["in_flight"]) + int(r["waiting"])
        d = np.where(exp, L.ADM_EXPIRED, L.ADM_NONEXISTENT).astype(np.uint8)
        if st == L.ACT_VALID and lim > 0 and c0 > lim:
            d[:] = L.ADM_OVERLOADED
        elif st == L.ACT_VALID:
            first = req & (q == 0)
            set0 = bool(fl & L.ACTF_RUNNING_SET)
            run_ro = bool(fl & L.ACTF_RUNNING_RO) if set0 else bool(ro[first].any())
            alpha = req & (bool(fl & L.ACTF_REENTRANT) | ai | (run_ro & ro)
                           | (first & (int(r["num_running"]) == 0 or not set0)))
            full = (c0 + q >= lim) if lim > 0 else np.zeros(len(f), bool)
            sat = alpha & full
            after = (np.cumsum(sat) - sat) > 0
            d = np.where(resp, L.ADM_RESPONSE, d)
            d = np.where(exp, L.ADM_EXPIRED, d)
            d = np.where(req, np.where(alpha, L.ADM_RUN, np.where(full, L.ADM_OVERLOADED, L.ADM_ENQUEUE)), d)
            d = np.where(after, L.ADM_OVERLOADED, d).astype(np.uint8)
            runs, enq = int((d == L.ADM_RUN).sum()), int((d == L.ADM_ENQUEUE).sum())
            out[a]["num_running"] += runs
            out[a]["in_flight"] += runs
            out[a]["waiting"] += enq
            if runs and not set0:
                out[a]["flags"] = (fl & ~L.ACTF_RUNNING_RO) | L.ACTF_RUNNING_SET | (L.ACTF_RUNNING_RO if run_ro else 0)
        elif st == L.ACT_INVALID:
            d = np.where(exp, L.ADM_EXPIRED, L.ADM_INVALID).astype(np.uint8)
        elif st < L.ACT_INVALID:
            ok = (c0 + q <= lim) if lim > 0 else np.ones(len(f), bool)
            d = np.where(exp, L.ADM_EXPIRED, np.where(resp, L.ADM_RESPONSE, np.where(ok, L.ADM_ENQUEUE, L.ADM_OVERLOADED)))
            d = d.astype(np.uint8)
            out[a]["waiting"] += int((d == L.ADM_ENQUEUE).sum())
        disp[idx] = d
    return disp, out, np.bincount(disp, minlength=N_CODES).astype(np.uint64)
