"""Waiting queues (orl_waitq_append_device / orl_complete_device): the reference's append, request completion and message
pump as sequential loops over plain Python lists, the coverage counters of those loops, the same in numpy as the kernels
compute it (append_ref, complete_closed_form), and the seeded scenario builders that tests/test_gpu_completion.py runs on
the device (no GPU needed here; tests/test_completion_ref.py pins the loops on hand-derived cases and holds the builders to
the counters).

The model is "the reference called in batch order" with one fixed choice: an activation's completions are
applied with Running's own completion first, the others in batch order, each one followed by RunMessagePump
(Dispatcher.OnActivationCompletedRequest, Dispatcher.cs:633-656).
"""
from collections import Counter

import numpy as np

import admission_ref as A
from orleans_amd import _lib as L

STATE_DTYPE = L.ACT_STATE_DTYPE
NONE, DRAIN = L.TOK_NONE, L.TOK_DRAIN
U32 = 0xFFFFFFFF

COUNTERS = ("running_cleared_rw_head_taken", "completion_not_running", "pump_stopped_by_head",
            "always_interleave_past_rw_running", "read_only_run", "reentrant_emptied", "non_valid_not_pumped",
            "pump_only_after_activating", "drain", "underflow", "handle_out_of_range", "running_tok_from_later_run")


class World:
    """The device-resident state: the table, the store as a CSR (off, tok, act, mflags) and running_tok."""

    def __init__(self, state, off=None, tok=None, mflags=None, running_tok=None):
        n_act = len(state)
        self.state = state.copy()
        self.off = np.zeros(n_act + 1, np.uint32) if off is None else np.asarray(off, np.uint32).copy()
        self.tok = np.zeros(0, np.uint32) if tok is None else np.asarray(tok, np.uint32).copy()
        self.mflags = np.zeros(0, np.uint8) if mflags is None else np.asarray(mflags, np.uint8).copy()
        self.running_tok = (np.full(n_act, NONE, np.uint32) if running_tok is None
                            else np.asarray(running_tok, np.uint32).copy())
        assert self.state.dtype == STATE_DTYPE and len(self.off) == n_act + 1 and len(self.running_tok) == n_act
        assert len(self.tok) == len(self.mflags) == int(self.off[-1])

    @property
    def n_act(self):
        return len(self.state)

    @property
    def act(self):
        return np.repeat(np.arange(self.n_act, dtype=np.uint32), np.diff(self.off.astype(np.int64)))

    def copy(self):
        return World(self.state, self.off, self.tok, self.mflags, self.running_tok)

    def seg(self, a):
        """Activation a's waiting list as [(tok, mflags), ...]."""
        return [(int(self.tok[i]), int(self.mflags[i])) for i in range(int(self.off[a]), int(self.off[a + 1]))]

    def with_lists(self, state, changed, running_tok):
        """A World with the waiting lists of `changed` ({handle: [(tok, mflags), ...]}) replaced."""
        act = self.act
        keep = ~np.isin(act, np.fromiter(changed.keys(), np.uint32, len(changed)))
        a_new = np.array([a for a, q in changed.items() for _ in q], np.uint32)
        t_new = np.array([t for q in changed.values() for t, _ in q], np.uint32)
        f_new = np.array([f for q in changed.values() for _, f in q], np.uint8)
        all_act = np.concatenate([act[keep], a_new])
        order = np.argsort(all_act, kind="stable")
        off = np.searchsorted(all_act[order], np.arange(self.n_act + 1)).astype(np.uint32)
        return World(state, off, np.concatenate([self.tok[keep], t_new])[order],
                     np.concatenate([self.mflags[keep], f_new])[order], running_tok)

    def same(self, o):
        return (np.array_equal(self.state, o.state) and np.array_equal(self.off, o.off) and np.array_equal(self.tok, o.tok)
                and np.array_equal(self.mflags, o.mflags) and np.array_equal(self.running_tok, o.running_tok))

    def check_invariants(self):
        """waiting == the segment's length, and running_tok != NONE <=> RUNNING_SET, for every activation."""
        assert np.array_equal(self.state["waiting"], np.diff(self.off.astype(np.int64)).astype(np.uint32))
        assert np.array_equal(self.running_tok != NONE, (self.state["flags"] & L.ACTF_RUNNING_SET) != 0)


# ---- append ------------------------------------------------------------------------------------------------------------
def append(w, act, tok, mflags, disp, cov=None):
    """The loop: message by message in arrival order, EnqueueMessage (ActivationData.cs:487-514) for an ENQUEUE and
    RecordRunning keeping the first (:411-422) for a RUN.  -> the World after; the table is not touched."""
    cov = Counter() if cov is None else cov
    lists, rt = {}, w.running_tok.copy()
    seen = set()
    for i in range(len(act)):
        a = int(act[i])
        if a >= w.n_act:  # stage 4's bucket n_act contributes nothing
            continue
        if disp[i] == L.ADM_ENQUEUE:
            if a not in lists:
                lists[a] = w.seg(a)
            lists[a].append((int(tok[i]), int(mflags[i])))
        elif disp[i] == L.ADM_RUN and rt[a] == NONE:
            rt[a] = tok[i]
            cov["running_tok_from_later_run"] += a in seen
        seen.add(a)
    return w.with_lists(w.state, lists, rt)


def append_ref(w, act, tok, mflags, disp):
    """The same in numpy, as the kernels compute it: E(a) = ENQUEUEs of the buckets before a's; old record j of a moves to
    j + E(a); the ENQUEUE at position p of bucket a lands at old_off[a + 1] + enq_before[p]."""
    n_act = w.n_act
    act, tok, mflags, disp = (np.asarray(x) for x in (act, tok, mflags, disp))
    key = np.minimum(act.astype(np.int64), n_act)
    order = np.argsort(key, kind="stable")
    boff = np.searchsorted(key[order], np.arange(n_act + 2)).astype(np.int64)
    live = key[order] < n_act
    enq = live & (disp[order] == L.ADM_ENQUEUE)
    pre = np.concatenate([[0], np.cumsum(enq)])
    E = pre[boff[:n_act + 1]]
    old_off = w.off.astype(np.int64)
    new_off = old_off + E
    total = int(new_off[-1])
    n_tok, n_mf = np.zeros(total, np.uint32), np.zeros(total, np.uint8)
    old_act = w.act.astype(np.int64)
    dst = np.arange(len(w.tok)) + E[old_act]
    n_tok[dst], n_mf[dst] = w.tok, w.mflags
    p = np.nonzero(enq)[0]
    dst = old_off[key[order][p] + 1] + pre[p]
    n_tok[dst], n_mf[dst] = tok[order][p], mflags[order][p]
    rt = w.running_tok.copy()
    run = live & (disp[order] == L.ADM_RUN)
    pr = np.nonzero(run)[0]
    first = pr[np.unique(key[order][pr], return_index=True)[1]] if len(pr) else pr  # a bucket's first RUN position
    a = key[order][first]
    unset = rt[a] == NONE
    rt[a[unset]] = tok[order][first[unset]]
    return World(w.state, new_off, n_tok, n_mf, rt)


# ---- complete ----------------------------------------------------------------------------------------------------------
def _may_accept(s, mf):
    """ActivationMayAcceptRequest / CanInterleave (Dispatcher.cs:316-338): rule 6 of admission."""
    fl = s["flags"]
    return (s["num_running"] == 0 or bool(fl & L.ACTF_REENTRANT) or bool(mf & L.MF_ALWAYS_INTERLEAVE)
            or not fl & L.ACTF_RUNNING_SET or (bool(fl & L.ACTF_RUNNING_RO) and bool(mf & L.MF_READ_ONLY)))


def _pump(a, s, q, rt, out, cov, after_reset=False):
    """Dispatcher.RunMessagePump (Dispatcher.cs:658-685) -> the records taken."""
    if s["state"] != L.ACT_VALID:  # :669
        cov["non_valid_not_pumped"] += bool(q)
        return 0
    taken = 0
    while q:
        tok, mf = q[0]
        if not _may_accept(s, mf):
            cov["pump_stopped_by_head"] += 1
            break
        fl = s["flags"]
        if s["num_running"] > 0 and not fl & L.ACTF_REENTRANT and fl & L.ACTF_RUNNING_SET:
            cov["always_interleave_past_rw_running"] += bool(mf & L.MF_ALWAYS_INTERLEAVE) and not fl & L.ACTF_RUNNING_RO
            cov["read_only_run"] += not mf & L.MF_ALWAYS_INTERLEAVE
        cov["running_cleared_rw_head_taken"] += (after_reset and taken == 0 and s["num_running"] > 0
                                                 and not fl & L.ACTF_RUNNING_SET and not fl & L.ACTF_REENTRANT
                                                 and not mf & (L.MF_READ_ONLY | L.MF_ALWAYS_INTERLEAVE))
        q.pop(0)  # DequeueNextWaitingMessage, then HandleIncomingRequest: RecordRunning, InFlightCount++
        s["waiting"] = (s["waiting"] - 1) & U32
        s["num_running"] = (s["num_running"] + 1) & U32
        s["in_flight"] = (s["in_flight"] + 1) & U32
        if not fl & L.ACTF_RUNNING_SET:
            s["flags"] = (fl & ~L.ACTF_RUNNING_RO) | L.ACTF_RUNNING_SET | (L.ACTF_RUNNING_RO if mf & L.MF_READ_ONLY else 0)
            rt[a] = tok
        out.append((tok, a, mf, L.WQ_RUN))
        taken += 1
    if taken and not q and s["flags"] & L.ACTF_REENTRANT:
        cov["reentrant_emptied"] += 1
    return taken


def _reset_running(a, s, tok, rt, cov):
    """InvokeWorkItem's InFlightCount-- (InvokeWorkItem.cs:70,79) and ActivationData.ResetRunning (:424-442)."""
    s["in_flight"] -= 1
    s["num_running"] -= 1
    if rt[a] != NONE and rt[a] == tok:
        s["flags"] &= ~(L.ACTF_RUNNING_SET | L.ACTF_RUNNING_RO)
        rt[a] = NONE
        return True
    cov["completion_not_running"] += 1
    return False


def complete(w, cact, ctok, cov=None, perm=None):
    """The loop.  -> (World after, out list [(tok, act, mflags, kind)], counts uint64[8]).  perm: a function that
    reorders an activation's completions other than Running's (the model says their order does not matter)."""
    cov = Counter() if cov is None else cov
    lists, rt, state = {}, w.running_tok.copy(), w.state.copy()
    counts = np.zeros(8, np.uint64)
    recs = {}
    for a, t in zip(np.asarray(cact).tolist(), np.asarray(ctok).tolist()):
        if a >= w.n_act:
            counts[L.CMP_IGNORED] += 1
            cov["handle_out_of_range"] += 1
            continue
        recs.setdefault(a, []).append(t)
    out = []
    for a in sorted(recs):
        comps = [t for t in recs[a] if t not in (NONE, DRAIN)]
        pumps, drains = recs[a].count(NONE), recs[a].count(DRAIN)
        counts[L.CMP_COMPLETIONS] += len(comps)
        counts[L.CMP_PUMPS] += pumps
        counts[L.CMP_DRAINS] += drains
        s = {f: int(state[a][f]) for f in ("state", "flags", "num_running", "in_flight", "waiting")}
        q = lists[a] = w.seg(a)
        n_out = len(out)
        k = len(comps)
        if drains:  # DequeueAllWaitingMessages (ActivationData.cs:590-599): nothing is left to pump
            cov["drain"] += 1
            out += [(t, a, f, L.WQ_DRAINED) for t, f in q]
            counts[L.CMP_DRAINED] += len(q)
            q.clear()
            s["waiting"] = 0
        if k > s["in_flight"] or k > s["num_running"]:
            # a caller error with no reference behaviour: the steps of the header define it (saturate, count, pump once)
            cov["underflow"] += 1
            counts[L.CMP_UNDERFLOWS] += 1
            s["in_flight"], s["num_running"] = max(s["in_flight"] - k, 0), max(s["num_running"] - k, 0)
            if rt[a] != NONE and int(rt[a]) in comps:
                s["flags"] &= ~(L.ACTF_RUNNING_SET | L.ACTF_RUNNING_RO)
                rt[a] = NONE
            _pump(a, s, q, rt, out, cov)
        else:
            mine = [t for t in comps if rt[a] != NONE and t == rt[a]]
            rest = [t for t in comps if not (rt[a] != NONE and t == rt[a])]
            if perm is not None:
                rest = perm(rest)
            for t in mine + rest:  # OnActivationCompletedRequest: ResetRunning, then RunMessagePump
                was_running = _reset_running(a, s, t, rt, cov)
                _pump(a, s, q, rt, out, cov, after_reset=was_running)
            if pumps or not comps:
                before = len(out)
                _pump(a, s, q, rt, out, cov)
                cov["pump_only_after_activating"] += (not comps and not drains and len(out) > before)
        counts[L.CMP_RUN] += sum(1 for o in out[n_out:] if o[3] == L.WQ_RUN)
        for f in ("flags", "num_running", "in_flight", "waiting"):
            state[a][f] = s[f]
    nw = w.with_lists(state, lists, rt)
    counts[L.CMP_WAITING] = len(nw.tok)
    return nw, out, counts


def complete_closed_form(w, cact, ctok, as_arrays=False):
    """The same from the closed form, in numpy over the whole store: apply all completions, then a record is
    taken iff no record at or before it in its segment fails.  as_arrays: the out list as its four columns (tok, act,
    mflags, kind) instead of a list of tuples, for stores of millions of records."""
    n_act = w.n_act
    cact, ctok = np.asarray(cact, np.uint32).astype(np.int64), np.asarray(ctok, np.uint32)
    counts = np.zeros(8, np.uint64)
    ok = cact < n_act
    counts[L.CMP_IGNORED] = int((~ok).sum())
    ca, ct = cact[ok], ctok[ok]
    is_pump, is_drain = ct == NONE, ct == DRAIN
    is_comp = ~is_pump & ~is_drain
    counts[L.CMP_COMPLETIONS], counts[L.CMP_PUMPS], counts[L.CMP_DRAINS] = is_comp.sum(), is_pump.sum(), is_drain.sum()
    nrec = np.bincount(ca, minlength=n_act)
    k = np.bincount(ca[is_comp], minlength=n_act)
    drain = np.bincount(ca[is_drain], minlength=n_act) > 0
    r = np.zeros(n_act, bool)
    r[ca[is_comp & (ct == w.running_tok[ca])]] = True  # an ordinary token is never NONE
    st = w.state.copy()
    touched = nrec > 0
    nr0, inf0 = st["num_running"].astype(np.int64), st["in_flight"].astype(np.int64)
    counts[L.CMP_UNDERFLOWS] = int((touched & ((k > nr0) | (k > inf0))).sum())
    nr, inf = np.maximum(nr0 - k, 0), np.maximum(inf0 - k, 0)
    fl = st["flags"].astype(np.int64)
    fl = np.where(r, fl & ~(L.ACTF_RUNNING_SET | L.ACTF_RUNNING_RO), fl)
    rt = np.where(r, NONE, w.running_tok).astype(np.uint32)
    # per record
    act = w.act.astype(np.int64)
    off = w.off.astype(np.int64)
    n = len(act)
    mf = w.mflags.astype(np.int64)
    head = np.arange(n) == off[act]
    ai, ro = (mf & L.MF_ALWAYS_INTERLEAVE) != 0, (mf & L.MF_READ_ONLY) != 0
    set_, reent, rro_s = (fl[act] & L.ACTF_RUNNING_SET) != 0, (fl[act] & L.ACTF_REENTRANT) != 0, (fl[act] & L.ACTF_RUNNING_RO) != 0
    head_ro = (mf[np.minimum(off[act], max(n - 1, 0))] & L.MF_READ_ONLY) != 0 if n else np.zeros(0, bool)
    rro = np.where(set_, rro_s, head_ro)
    good = np.where(head, (nr[act] == 0) | reent | ai | ~set_ | (rro_s & ro), reent | ai | (rro & ro))
    good &= touched[act] & (st["state"][act] == L.ACT_VALID)
    good |= drain[act]
    fail = ~good
    # inclusive segmented OR of fail: failures up to i, minus those before the segment's head
    cf = np.cumsum(fail)
    before_head = np.concatenate([[0], cf])[off[act]]
    out_mask = (cf - before_head) == 0
    taken = np.bincount(act[out_mask], minlength=n_act)
    oi = np.nonzero(out_mask)[0]
    out = (w.tok[oi], act[oi].astype(np.uint32), w.mflags[oi], np.where(drain[act[oi]], L.WQ_DRAINED, L.WQ_RUN).astype(np.uint8))
    if not as_arrays:
        out = [tuple(int(x) for x in o) for o in zip(*out)]
    counts[L.CMP_DRAINED] = int(taken[drain].sum())
    counts[L.CMP_RUN] = int(taken[~drain].sum())
    pumped = touched & ~drain & (taken > 0)
    newly = pumped & ((fl & L.ACTF_RUNNING_SET) == 0)
    hro = np.zeros(n_act, bool)
    hro[newly] = ro[off[:-1][newly]]
    rt[newly] = w.tok[off[:-1][newly]]
    fl = np.where(newly, (fl & ~L.ACTF_RUNNING_RO) | L.ACTF_RUNNING_SET | np.where(hro, L.ACTF_RUNNING_RO, 0), fl)
    waiting = st["waiting"].astype(np.int64)
    waiting = np.where(touched & drain, 0, np.where(pumped, waiting - taken, waiting))
    nr, inf = np.where(pumped, nr + taken, nr), np.where(pumped, inf + taken, inf)
    st["flags"] = np.where(touched, fl, st["flags"]).astype(np.uint8)
    st["num_running"] = np.where(touched, nr, nr0).astype(np.uint32)
    st["in_flight"] = np.where(touched, inf, inf0).astype(np.uint32)
    st["waiting"] = (waiting & U32).astype(np.uint32)
    keep = ~out_mask
    new_off = off - np.concatenate([[0], np.cumsum(out_mask)])[off]
    nw = World(st, new_off, w.tok[keep], w.mflags[keep], np.where(touched, rt, w.running_tok))
    counts[L.CMP_WAITING] = int(keep.sum())
    return nw, out, counts


# ---- scenario builders -------------------------------------------------------------------------------------------------
SHAPE_N = A.SHAPE_N
SHAPE_N_ACT = A.SHAPE_N_ACT


def consistent_world(rng, n_act, max_wait=3, state=None, p_running=0.6, p_wait=1.0):
    """A random table whose waiting counts, RUNNING_SET bits and running_tok agree with a random store.  Tokens of
    waiting records are 0x40000000 + index, Running's 0x20000000 + handle."""
    s = A.random_state(rng, n_act) if state is None else state.copy()
    wait = np.where((s["state"] >= L.ACT_INVALID) | (rng.random(n_act) >= p_wait), 0,
                    rng.integers(0, max_wait + 1, n_act)).astype(np.uint32)
    s["waiting"] = wait
    running = (rng.random(n_act) < p_running) & (s["num_running"] > 0)
    s["flags"] = np.where(running, s["flags"] | L.ACTF_RUNNING_SET, s["flags"] & (0xFF ^ (L.ACTF_RUNNING_SET | L.ACTF_RUNNING_RO)))
    s["in_flight"] = np.maximum(s["in_flight"], s["num_running"])
    rt = np.where(running, 0x20000000 + np.arange(n_act), NONE).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(wait)]).astype(np.uint32)
    total = int(off[-1])
    return World(s, off, (0x40000000 + np.arange(total)).astype(np.uint32), request_flags(rng, total), rt)


def request_flags(rng, n, p_ro=0.35, p_ai=0.1):
    """Flags of waiting records: Request / OneWay with the read-only and always-interleave bits."""
    d = np.where(rng.random(n) < 0.1, L.MF_ONE_WAY, L.MF_REQUEST).astype(np.uint8)
    return (d | np.where(rng.random(n) < p_ro, L.MF_READ_ONLY, 0).astype(np.uint8)
            | np.where(rng.random(n) < p_ai, L.MF_ALWAYS_INTERLEAVE, 0).astype(np.uint8))


def random_completions(rng, w, m, p_running=0.5, p_pump=0.05, p_drain=0.03, p_bad=0.03, respect_counts=True):
    """m records: completions of Running or of other running requests (tokens 0x10000000 + j), never more per activation
    than it has running (unless respect_counts is off), pump and drain requests, handles >= n_act."""
    n_act = w.n_act
    cact = rng.integers(0, n_act, m).astype(np.uint32)
    ctok = (0x10000000 + np.arange(m)).astype(np.uint32)
    left = np.minimum(w.state["num_running"], w.state["in_flight"]).astype(np.int64)
    used_running = np.zeros(n_act, bool)
    u = rng.random(m)
    for j in range(m):
        a = int(cact[j])
        if u[j] < p_bad:
            cact[j] = [n_act, n_act + 7, 0x80000000, U32][j % 4]
        elif u[j] < p_bad + p_pump:
            ctok[j] = NONE
        elif u[j] < p_bad + p_pump + p_drain:
            ctok[j] = DRAIN
        elif respect_counts and left[a] == 0:
            ctok[j] = NONE
        else:
            left[a] -= 1
            if w.running_tok[a] != NONE and not used_running[a] and rng.random() < p_running:
                ctok[j] = w.running_tok[a]
                used_running[a] = True
    return cact, ctok


class Scenario:
    """A start World, one admitted batch to append (act, tok, mflags, limits) and one completion batch."""

    def __init__(self, name, world, act, mflags, cact, ctok, hard=0, hard_stateless=0, capacity=None):
        self.name, self.world, self.hard, self.hard_stateless = name, world, hard, hard_stateless
        self.act = np.ascontiguousarray(act, np.uint32)
        self.mflags = np.ascontiguousarray(mflags, np.uint8)
        self.tok = (0x50000000 + np.arange(len(self.act))).astype(np.uint32)
        self.cact = np.ascontiguousarray(cact, np.uint32)
        self.ctok = np.ascontiguousarray(ctok, np.uint32)
        self.capacity = capacity if capacity is not None else max(1, len(world.tok) + len(self.act))

    @property
    def n_act(self):
        return self.world.n_act

    def expect(self, cov=None):
        """-> (disp, admit counts, World after append, World after complete, out list, complete counts).  The completion
        batch is applied to the appended World."""
        disp, st, acounts = A.admit(self.act, self.mflags, self.world.state, self.n_act, self.hard, self.hard_stateless)
        w1 = append(self.world, self.act, self.tok, self.mflags, disp, cov)
        w1.state = st
        w2, out, counts = complete(w1, self.cact, self.ctok, cov)
        return disp, acounts, w1, w2, out, counts


def shape_scenario(n, n_act, seed=0):
    """Random everything: n admitted messages and m = n completion records over a consistent random World."""
    rng = np.random.default_rng([n, n_act, seed, 17])
    w = consistent_world(rng, n_act, p_wait=0.05 if n_act > 5000 else 1.0)  # 2^20 activations: a sparse store
    w.state[n_act // 2]["state"] = L.ACT_VALID  # the hot handle of the admitted batch takes part
    base = A.shape_scenario(n, n_act, seed)
    # completions refer to the state after admission; build them against it so that the counts are respected
    disp, st, _ = A.admit(base.act, base.mflags, w.state, n_act, 6, 3)
    tmp = w.copy()
    tmp.state = st
    cact, ctok = random_completions(rng, tmp, n)
    return Scenario(f"shape-n{n}-a{n_act}", w, base.act, base.mflags, cact, ctok, 6, 3)


def _one_act_world(n_act, h, flags, num_running, rec_flags, rt=NONE, state=L.ACT_VALID):
    s = np.zeros(n_act, STATE_DTYPE)
    s["state"] = L.ACT_VALID
    n = len(rec_flags)
    s[h] = (state, flags, 0, num_running, num_running, n)
    off = np.zeros(n_act + 1, np.uint32)
    off[h + 1:] = n
    rtk = np.full(n_act, NONE, np.uint32)
    rtk[h] = rt
    return World(s, off, (0x40000000 + np.arange(n)).astype(np.uint32), np.asarray(rec_flags, np.uint8), rtk)


def one_segment_scenarios(n_rec=3 * 2048 + 100):
    """Handle 1 of 3 holds the whole store across more than 3 tiles; Running is a read-only request R and the records are
    read-only, so that the first read-write record is the first failure: at tile boundary - 1, at it and + 1; nowhere
    (the whole segment taken); at the head (nothing taken).  A completion of another request triggers the pump."""
    out = []
    busy = L.ACTF_RUNNING_SET | L.ACTF_RUNNING_RO
    for name, first_fail in (("edge-1", 2047), ("edge", 2048), ("edge+1", 2049), ("edge2-1", 4095), ("edge2", 4096),
                             ("none", None), ("head", 0)):
        fl = np.full(n_rec, L.MF_REQUEST | L.MF_READ_ONLY, np.uint8)
        if first_fail is not None:
            fl[first_fail] = L.MF_REQUEST
            fl[first_fail + 5] = L.MF_REQUEST
        w = _one_act_world(3, 1, busy, 2, fl, rt=77)
        out.append(Scenario(f"one-seg-{name}", w, [], [], [1], [0x10000000]))
    return out


def boundary_scenario(k, d_start, d_len):
    """Handle 0 holds 2^k + d_start records, so handle 1's segment starts there; it holds 2^k + d_len; handle 2 holds 5.
    Handle 0 is reentrant (emptied), handle 1 stops in the middle, handle 2 is not touched.  The append adds a run to each
    (their new ends straddle tile edges for k = 10, 11), and bucket 3 is unresolved."""
    n0, n1 = (1 << k) + d_start, (1 << k) + d_len
    rng = np.random.default_rng([k, d_start + 1, d_len + 1, 5])
    s = np.zeros(3, STATE_DTYPE)
    s[0] = (L.ACT_VALID, L.ACTF_REENTRANT | L.ACTF_RUNNING_SET, 0, 1, 1, n0)
    s[1] = (L.ACT_VALID, L.ACTF_RUNNING_SET | L.ACTF_RUNNING_RO, 0, 2, 2, n1)
    s[2] = (L.ACT_VALID, L.ACTF_RUNNING_SET, 0, 1, 1, 5)
    fl = request_flags(rng, n0 + n1 + 5, p_ro=0.5, p_ai=0.0)
    fl[n0:n0 + n1 // 2] |= L.MF_READ_ONLY
    fl[n0 + n1 // 2] = L.MF_REQUEST
    w = World(s, [0, n0, n0 + n1, n0 + n1 + 5], (0x40000000 + np.arange(len(fl))).astype(np.uint32), fl,
              np.array([900, 901, 902], np.uint32))
    act = rng.permutation(np.concatenate([np.zeros(40, np.uint32), np.ones(70, np.uint32), np.full(9, 2, np.uint32),
                                          np.full(6, 3, np.uint32)]))
    mfl = np.full(len(act), L.MF_REQUEST, np.uint8)  # read-write requests: enqueued behind Running on 1 and 2
    return Scenario(f"edge-k{k}-s{d_start}-l{d_len}", w, act, mfl, [1, 0, 0, 1], [901, 900, NONE, 0x10000000])


def append_scenarios():
    """Appends into an empty store, and appends where an old segment and its new run straddle a tile edge."""
    out = []
    rng = np.random.default_rng(41)
    for n_act, n in ((3, 5000), (700, 9000)):
        s = np.zeros(n_act, STATE_DTYPE)
        s["state"] = L.ACT_VALID
        act = rng.integers(0, n_act + 1, n).astype(np.uint32)
        w = World(s)
        out.append(Scenario(f"append-empty-a{n_act}", w, act, A.random_flags(rng, n, p_ro=0.3), [0, 1, 2], [NONE] * 3))
    for old0, old1 in ((2040, 10), (2048, 2047), (1, 4095)):
        s = np.zeros(4, STATE_DTYPE)
        s["state"] = L.ACT_VALID
        s["flags"] = L.ACTF_RUNNING_SET
        s["num_running"] = s["in_flight"] = 1
        s["waiting"] = (old0, old1, 0, 3)
        off = np.cumsum([0, old0, old1, 0, 3]).astype(np.uint32)
        n = int(off[-1])
        w = World(s, off, (0x40000000 + np.arange(n)).astype(np.uint32), request_flags(rng, n, p_ai=0.0),
                  np.array([900, 901, 902, 903], np.uint32))
        act = rng.permutation(np.repeat(np.arange(5, dtype=np.uint32), (20, 30, 4, 0, 6)))
        out.append(Scenario(f"append-straddle-{old0}-{old1}", w, act, np.full(len(act), L.MF_REQUEST, np.uint8),
                            [0, 2], [900, 902]))
    return out


def state_matrix_scenario(with_r):
    """Every state value 0..7 x every flag combination x num_running 0 / 2 on neighbouring handles, three waiting records
    each (none on INVALID / ABSENT), and per activation two completions: with_r names Running's token in one of them."""
    combos = [(st, fl, nr) for st in range(8) for fl in range(16) for nr in (0, 2)]
    n_act = len(combos)
    rng = np.random.default_rng(256 + with_r)
    s = np.zeros(n_act, STATE_DTYPE)
    for h, (st, fl, nr) in enumerate(combos):
        s[h] = (st, fl, 0, nr, nr + int(rng.integers(0, 2)), 0)
    wait = np.where(s["state"] >= L.ACT_INVALID, 0, 3).astype(np.uint32)
    s["waiting"] = wait
    off = np.concatenate([[0], np.cumsum(wait)]).astype(np.uint32)
    total = int(off[-1])
    rt = np.where(s["flags"] & L.ACTF_RUNNING_SET, 0x20000000 + np.arange(n_act), NONE).astype(np.uint32)
    w = World(s, off, (0x40000000 + np.arange(total)).astype(np.uint32), request_flags(rng, total, p_ro=0.5, p_ai=0.15), rt)
    cact = np.repeat(np.arange(n_act, dtype=np.uint32), 2)
    ctok = (0x10000000 + np.arange(2 * n_act)).astype(np.uint32)
    if with_r:
        has = rt != NONE
        ctok[1::2][has] = rt[has]
    p = rng.permutation(2 * n_act)
    return Scenario(f"state-matrix-r{int(with_r)}", w, [], [], cact[p], ctok[p])


def drain_pump_scenario():
    """Drain and pump-only records, alone and mixed with completions of the same activation; an ACTIVATING activation
    that became VALID gets its pump request; a non-VALID one is not pumped; an underflow; handles >= n_act."""
    n_act = 12
    s = np.zeros(n_act, STATE_DTYPE)
    busy = L.ACTF_RUNNING_SET
    for h in range(n_act):
        s[h] = (L.ACT_VALID, busy, 0, 1, 1, 4)
    s[4] = (L.ACT_VALID, 0, 0, 0, 0, 4)          # was ACTIVATING, its host made it VALID: pump only
    s[5] = (L.ACT_DEACTIVATING, busy, 0, 1, 1, 4)  # completes, not pumped
    s[6] = (L.ACT_VALID, busy, 0, 1, 0, 4)       # underflow: in_flight 0
    s[7] = (L.ACT_VALID, busy | L.ACTF_REENTRANT, 0, 3, 3, 4)
    off = (4 * np.arange(n_act + 1)).astype(np.uint32)
    rng = np.random.default_rng(12)
    fl = request_flags(rng, 4 * n_act, p_ro=0.3)
    rt = (900 + np.arange(n_act)).astype(np.uint32)
    rt[4] = NONE
    w = World(s, off, (0x40000000 + np.arange(4 * n_act)).astype(np.uint32), fl, rt)
    cact = [0, 1, 1, 2, 3, 3, 3, 4, 5, 6, 6, 7, n_act, U32, 8, 8, 9, 9]
    ctok = [DRAIN, DRAIN, 901, NONE, 903, NONE, NONE, NONE, 905, 906, 55, 56, 1, NONE, NONE, DRAIN, 909, 57]
    return Scenario("drain-pump", w, [], [], cact, ctok)


# ---- the chunked regime of the one-workgroup tile scan (admission_ref.CHUNK_N has the shapes) --------------------------
# The loops above are too slow at 4 M records; the GPU tests compare these with append_ref and complete_closed_form.
CHUNK_N = A.CHUNK_N
CHUNK_STRIDE = A.CHUNK_STRIDE


def _chunk_acts(n, kind):
    """`one`: handle 1 of 3 holds all n positions; `stride`: handle a holds [3000 a, 3000 a + 3000)."""
    if kind == "one":
        return 3, np.full(n, 1, np.uint32)
    return (n + CHUNK_STRIDE - 1) // CHUNK_STRIDE, (np.arange(n) // CHUNK_STRIDE).astype(np.uint32)


def chunk_appends(n):
    """-> [(name, World, act, tok, mflags, disp)]: an empty store and a batch of n positions with dispositions drawn at
    random (half ENQUEUE, a fifth RUN).  `one`: the bucket's first RUN lies behind n // 2, so "a RUN was seen" crosses
    many chunks and every later RUN must leave running_tok alone.  `stride`: arrival order shuffled, and every third
    activation already has a Running."""
    out = []
    for kind in ("one", "stride"):
        rng = np.random.default_rng([n, 1024, kind == "one"])
        n_act, act = _chunk_acts(n, kind)
        s = np.zeros(n_act, STATE_DTYPE)
        s["state"] = L.ACT_VALID
        rt = np.full(n_act, NONE, np.uint32)
        disp = rng.choice(np.array([L.ADM_ENQUEUE, L.ADM_RUN, L.ADM_OVERLOADED, L.ADM_RESPONSE, L.ADM_EXPIRED], np.uint8), n,
                          p=[0.5, 0.2, 0.1, 0.1, 0.1])
        if kind == "one":
            early = np.arange(n) < n // 2 + 5
            disp[early & (disp == L.ADM_RUN)] = L.ADM_RESPONSE
        else:
            act = rng.permutation(act)
            rt[::3] = (0x20000000 + np.arange(n_act))[::3]
        tok = (0x50000000 + np.arange(n)).astype(np.uint32)
        out.append((f"chunk-append-{kind}-n{n}", World(s, running_tok=rt), act, tok, request_flags(rng, n), disp))
    return out


def chunk_completes(n):
    """-> [(name, World, cact, ctok)]: a store of n records.  `one`: Running is a read-only request and the records are
    read-only up to the first read-write one at n // 2 + 77, so the pump takes a prefix that ends many chunks behind the
    segment's head.  `stride`: random tables (half of the activations reentrant: their whole segment goes, across a tile
    edge), three activations of four get a record: a completion (Running's own for every other one), a pump or a drain."""
    out = []
    busy = L.ACTF_RUNNING_SET | L.ACTF_RUNNING_RO
    fl = np.full(n, L.MF_REQUEST | L.MF_READ_ONLY, np.uint8)
    fl[n // 2 + 77] = fl[n // 2 + 82] = L.MF_REQUEST
    out.append((f"chunk-complete-one-n{n}", _one_act_world(3, 1, busy, 2, fl, rt=77), np.array([1], np.uint32),
                np.array([0x10000000], np.uint32)))
    rng = np.random.default_rng([n, 1024, 7])
    n_act, act = _chunk_acts(n, "stride")
    s = np.zeros(n_act, STATE_DTYPE)
    s["state"] = np.where(rng.random(n_act) < 0.9, L.ACT_VALID, L.ACT_DEACTIVATING)
    s["flags"] = rng.integers(0, 16, n_act)
    s["num_running"] = rng.integers(0, 3, n_act)
    s["in_flight"] = s["num_running"] + rng.integers(0, 2, n_act)
    s["waiting"] = np.bincount(act, minlength=n_act)
    off = np.concatenate([[0], np.cumsum(s["waiting"])]).astype(np.uint32)
    h = np.arange(n_act)
    rt = np.where(s["flags"] & L.ACTF_RUNNING_SET, 0x20000000 + h, NONE).astype(np.uint32)
    w = World(s, off, (0x40000000 + np.arange(n)).astype(np.uint32), request_flags(rng, n, p_ro=0.9, p_ai=0.05), rt)
    cact = h[h % 4 != 3].astype(np.uint32)
    ctok = np.where((cact % 2 == 1) & (rt[cact] != NONE), rt[cact], 0x10000000 + cact).astype(np.uint32)
    ctok[cact % 16 == 5] = NONE
    ctok[cact % 32 == 9] = DRAIN
    cact = np.concatenate([cact, np.array([n_act, U32], np.uint32)])
    ctok = np.concatenate([ctok, np.array([1, NONE], np.uint32)])
    p = rng.permutation(len(cact))
    out.append((f"chunk-complete-stride-n{n}", w, cact[p], ctok[p]))
    return out


def chain_rounds():
    """Three rounds of (admitted batch, completion batch) over one table of 64 activations and one queue."""
    rng = np.random.default_rng(35)
    n_act = 64
    w = consistent_world(rng, n_act)
    rounds = []
    for n in (5000, 2049, 7000):
        act = rng.integers(0, n_act + 4, n).astype(np.uint32)
        rounds.append((act, A.random_flags(rng, n, p_ro=0.3), int(rng.integers(1 << 30))))
    return w, rounds, (60, 30)


def chain_completions(w, seed, m=300):
    return random_completions(np.random.default_rng(seed), w, m, p_running=0.7)


def all_scenarios():
    """Every single-round scenario of the GPU file, by name."""
    out = [shape_scenario(n, a) for n in SHAPE_N for a in SHAPE_N_ACT]
    out += one_segment_scenarios()
    out += [boundary_scenario(k, ds, dl) for k in range(6, 14) for ds in (-1, 0, 1) for dl in (-1, 0, 1)]
    out += append_scenarios()
    out += [state_matrix_scenario(False), state_matrix_scenario(True), drain_pump_scenario()]
    return out
