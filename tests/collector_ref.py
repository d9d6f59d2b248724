"""The idle-activation collector (orl_collector, orl_collect_*_device): the reference's ActivationCollector as literal
Python over plain objects (a dict of buckets keyed by ticket, holding items that can be nulled; the cancelled flag), the
coverage counters of that code, the same per activation in numpy as the kernels compute it (Col and the np_* functions),
and the seeded scenario builders that tests/test_gpu_collector.py runs on the device (no GPU needed here;
tests/test_collector_ref.py pins the literal code on hand-derived cases, holds the numpy form to it on random histories and
holds the builders to the counters).

Citations are to src/OrleansRuntime/Catalog/ActivationCollector.cs unless a file is named.  Time is a caller-supplied
`now` in ticks, > 0 and not decreasing; nothing reads a clock.
"""
from collections import Counter

import numpy as np

import admission_ref as A
import completion_ref as Q
from orleans_amd import _lib as L

STATE_DTYPE = L.ACT_STATE_DTYPE
EXEMPT, CANCELLED = L.COLF_EXEMPT, L.COLF_CANCELLED
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
CERTAIN = (L.ADM_RUN, L.ADM_ENQUEUE, L.ADM_RESPONSE, L.ADM_INVALID)  # always reach Catalog.GetOrCreateActivation

COUNTERS = ("stale_bad_state", "stale_kept_alive", "stale_active", "stale_not_stale", "stale_condemned",
            "cancelall_skipped_cancelled", "cancelled_touched_ticket_dropped", "expired_touched", "same_ticket_on_cancelled",
            "rule1_only_not_touched", "rule7_only_touched", "ticket_exact_multiple", "ticket_one_past",
            "keep_alive_eq_now", "idleness_eq_age_limit", "bad_timeout", "schedule_on_ticketed")


def mk(t, quantum):
    """MakeTicketFromDateTime :391-400; t > 0."""
    return ((t - 1) // quantum + 1) * quantum


# ---- the literal reference -----------------------------------------------------------------------------------------------
class BadTimeout(Exception):
    """MakeTicketFromTimeSpan's ArgumentException :402-410."""


class Item:
    """The collector's view of one ActivationData (ActivationData.cs:350-390, 409, 640)."""
    __slots__ = ("a", "ticket", "cancelled", "exempt", "age_limit", "keep_alive_until", "became_idle")

    def __init__(self, a):
        self.a, self.ticket, self.cancelled, self.exempt = a, 0, False, False
        self.age_limit = self.keep_alive_until = self.became_idle = 0

    def try_set_cancelled(self):  # TrySetCollectionCancelledFlag, ActivationData.cs:358-366
        if self.ticket == 0 or self.cancelled:
            return False
        self.cancelled = True
        return True


class Bucket:
    """:434-504.  items: handle -> Item, or None once cancelled in place."""

    def __init__(self, key):
        self.key, self.items = key, {}

    def add(self, it):
        assert it.a not in self.items, "item is already associated with this bucket"
        self.items[it.a] = it

    def try_cancel(self, it):  # :466-474
        if not it.try_set_cancelled():
            return False
        assert self.items.get(it.a) is it, "unexpected failure to cancel deactivation"
        self.items[it.a] = None
        return True

    def try_remove(self, it):  # :457-464
        if not self.try_cancel(it):
            return False
        del self.items[it.a]
        return True

    def cancel_all(self, cov):  # :476-494
        out = []
        for v in self.items.values():
            if v is None:  # the reference dereferences it; the device skips a cancelled entry
                cov["cancelall_skipped_cancelled"] += 1
            elif v.try_set_cancelled():
                out.append(v)
        return out


class RefCollector:
    def __init__(self, n_act, quantum, now0, cov=None):
        self.cov = Counter() if cov is None else cov
        self.quantum, self.now = int(quantum), int(now0)
        self.items = [Item(a) for a in range(n_act)]
        self.buckets = {}
        self.next_ticket = mk(int(now0), self.quantum)

    # -- construction from / export to the device form
    @classmethod
    def from_col(cls, col, cov=None):
        r = cls(col.n_act, col.quantum, 1, cov)
        r.next_ticket = int(col.next_ticket)
        for a, it in enumerate(r.items):
            it.ticket, it.became_idle = int(col.ticket[a]), int(col.became_idle[a])
            it.keep_alive_until, it.age_limit = int(col.keep_alive_until[a]), int(col.age_limit[a])
            it.exempt, it.cancelled = bool(col.cflags[a] & EXEMPT), bool(col.cflags[a] & CANCELLED)
            if it.ticket and not it.cancelled:
                assert it.ticket >= r.next_ticket, "a live ticket below next_ticket has no bucket to be dequeued from"
                r.buckets.setdefault(it.ticket, Bucket(it.ticket)).add(it)
            elif it.ticket and it.ticket >= r.next_ticket:  # cancelled in place by ScanAll: nulled, still in its bucket
                r.buckets.setdefault(it.ticket, Bucket(it.ticket)).items[a] = None
        return r

    def export(self):
        col = Col(len(self.items), self.quantum, 1)
        col.next_ticket = self.next_ticket
        for a, it in enumerate(self.items):
            col.ticket[a], col.became_idle[a] = it.ticket, it.became_idle
            col.keep_alive_until[a], col.age_limit[a] = it.keep_alive_until, it.age_limit
            col.cflags[a] = (EXEMPT if it.exempt else 0) | (CANCELLED if it.cancelled else 0)
        return col

    # -- tickets
    def is_expired(self, ticket):  # :386-389
        return ticket < self.next_ticket

    def make_ticket_from_datetime(self, ts):  # :391-400
        self.cov["ticket_exact_multiple"] += ts % self.quantum == 0
        self.cov["ticket_one_past"] += ts % self.quantum == 1
        ticket = mk(ts, self.quantum)
        assert ticket >= self.next_ticket, "The earliest collection that can be scheduled from now is later"
        return ticket

    def make_ticket_from_timespan(self, timeout):  # :402-410
        if timeout < self.quantum:
            self.cov["bad_timeout"] += 1
            raise BadTimeout(timeout)
        return self.make_ticket_from_datetime(self.now + timeout)

    def add(self, it, ticket):  # :412-424
        it.cancelled = False
        self.buckets.setdefault(ticket, Bucket(ticket)).add(it)
        assert ticket != 0 and it.ticket == 0  # SetCollectionTicket, ActivationData.cs:381-390
        it.ticket = ticket

    # -- the three per-item calls; each -> its d_counts slot (None: nothing to count)
    def schedule_collection(self, it):  # :103-128
        if it.exempt:
            return L.SCHED_EXEMPT
        if it.age_limit == 0:
            return L.SCHED_AGE_ZERO
        try:
            ticket = self.make_ticket_from_timespan(it.age_limit)
        except BadTimeout:
            return L.SCHED_BAD_TIMEOUT
        if it.ticket != 0:  # the reference throws InvalidOperationException; the device leaves the entry and counts
            self.cov["schedule_on_ticketed"] += 1
            return L.SCHED_TICKETED
        self.add(it, ticket)
        return L.SCHED_DONE

    def try_cancel_collection(self, it):  # :130-146
        if it.exempt:
            return L.CANCEL_EXEMPT
        if it.ticket == 0:
            return L.CANCEL_NO_TICKET
        if self.is_expired(it.ticket):
            return L.CANCEL_EXPIRED
        b = self.buckets.get(it.ticket)
        if b is None or not b.try_remove(it):
            return L.CANCEL_ALREADY
        return L.CANCEL_DONE

    def try_reschedule_collection(self, it):  # :148-159
        if it.exempt:
            return None
        had, was_expired, was_cancelled = it.ticket, it.ticket != 0 and self.is_expired(it.ticket), it.cancelled
        try:
            r = self._try_reschedule_impl(it, it.age_limit)
        except BadTimeout:  # the reference's exception leaves the item as it is
            return L.COL_BAD_TIMEOUT
        if r is not None:
            return r
        it.ticket = 0  # ResetCollectionTicket :156
        if not had:
            return None
        if was_expired:
            self.cov["expired_touched"] += 1
            return L.COL_EXPIRED
        assert was_cancelled
        self.cov["cancelled_touched_ticket_dropped"] += 1
        return L.COL_CANCELLED_DROPPED

    def _try_reschedule_impl(self, it, timeout):  # :161-184; None = false
        if it.ticket == 0:
            return None
        assert it.ticket % self.quantum == 0  # ThrowIfTicketIsInvalid
        if self.is_expired(it.ticket):
            return None
        old = it.ticket
        new = self.make_ticket_from_timespan(timeout)
        if new == old:
            self.cov["same_ticket_on_cancelled"] += it.cancelled
            return L.COL_SAME
        b = self.buckets.get(old)
        if b is None or not b.try_remove(it):
            return None
        it.ticket = 0
        self.add(it, new)
        return L.COL_MOVED

    # -- batch calls in batch order
    def schedule(self, handles, now):
        self.now = int(now)
        counts = np.zeros(8, np.uint64)
        for a in np.asarray(handles).tolist():
            counts[L.SCHED_IGNORED if a >= len(self.items) else self.schedule_collection(self.items[a])] += 1
        return counts

    def cancel(self, handles):
        counts = np.zeros(8, np.uint64)
        for a in np.asarray(handles).tolist():
            counts[L.CANCEL_IGNORED if a >= len(self.items) else self.try_cancel_collection(self.items[a])] += 1
        return counts

    def touch(self, act, disp, state_before, hard, hard_stateless, now):
        """Message by message in arrival order: every message that reaches Catalog.GetOrCreateActivation (Dispatcher.cs:108,
        Catalog.cs:427) with an existing ActivationData reschedules its activation.  -> counts (per activation: the first
        outcome; a repeat in one batch changes nothing, which the loop asserts)."""
        self.now = int(now)
        counts = np.zeros(8, np.uint64)
        reached = reaches_catalog(act, disp, state_before, hard, hard_stateless)
        first = {}
        for i in np.nonzero(reached)[0].tolist():
            it = self.items[int(act[i])]
            r = self.try_reschedule_collection(it)
            if it.a in first:
                assert r in (None, L.COL_SAME, L.COL_BAD_TIMEOUT), "reschedule is idempotent for one now"
            else:
                first[it.a] = r
        for r in first.values():
            counts[L.COL_TOUCHED] += 1
            if r is not None:
                counts[r] += 1
        act = np.asarray(act)
        ok = act < len(self.items)
        only = np.setdiff1d(act[ok & (np.asarray(disp) == L.ADM_OVERLOADED)], act[ok & np.isin(disp, CERTAIN)])
        for a in only.tolist():
            hit = a in first
            counts[L.COL_RULE7_ONLY if hit else L.COL_RULE1_ONLY] += 1
            self.cov["rule7_only_touched" if hit else "rule1_only_not_touched"] += 1
        return counts

    def reset_running_idle(self, it, now):
        """ResetRunning's branch for numRunning == 0 (ActivationData.cs:428-435)."""
        self.now = int(now)
        it.became_idle = int(now)
        return None if it.exempt else self.try_reschedule_collection(it)

    def on_complete(self, cact, ctok, state_before, now):
        """The batched rule of orl_collect_on_complete_device: an activation with k >= 1 ordinary-token records and
        k >= num_running goes through the idle branch once."""
        counts = np.zeros(8, np.uint64)
        k = Counter()
        for a, t in zip(np.asarray(cact).tolist(), np.asarray(ctok).tolist()):
            if a >= len(self.items):
                counts[L.COL_IGNORED] += 1
            elif t not in (L.TOK_NONE, L.TOK_DRAIN):
                counts[L.COL_COMPLETIONS] += 1
                k[a] += 1
        for a in sorted(k):
            if k[a] >= int(state_before[a]["num_running"]):
                counts[L.COL_BECAME_IDLE] += 1
                r = self.reset_running_idle(self.items[a], now)
                if r is not None:
                    counts[r] += 1
        return counts

    # -- the scans
    def dequeue_quantum(self, now):  # :186-210
        if self.next_ticket > now:
            return False, None
        key = self.next_ticket
        self.next_ticket += self.quantum
        b = self.buckets.pop(key, None)
        return True, ([] if b is None else b.cancel_all(self.cov))

    def _cancelled_below(self, bound):
        """Bookkeeping for d_counts only: entries the device scan passes over because they are cancelled."""
        return sum(1 for it in self.items if it.ticket != 0 and it.cancelled and (bound is None or it.ticket < bound))

    def scan_stale(self, state, now):
        """:226-284.  state: the table, updated in place.  -> (condemned handles ascending, counts)."""
        self.now = now = int(now)
        counts = np.zeros(8, np.uint64)
        nn = self.next_ticket
        if nn <= now:
            nn += ((now - nn) // self.quantum + 1) * self.quantum
        counts[L.SCAN_CANCELLED_SKIPPED] = self._cancelled_below(nn) if nn != self.next_ticket else 0
        result = []
        while True:
            ok, items = self.dequeue_quantum(now)
            if not ok:
                break
            for it in items:
                counts[L.SCAN_CANDIDATES] += 1
                it.ticket = 0  # ResetCollectionTicket
                s = state[it.a]
                r = None
                if s["state"] != L.ACT_VALID:
                    kind = "bad_state"
                elif it.keep_alive_until >= now:  # ShouldBeKeptAlive, ActivationData.cs:642
                    kind = "kept_alive"
                    self.cov["keep_alive_eq_now"] += it.keep_alive_until == now
                    r = self.schedule_collection(it)
                elif s["num_running"] > 0 or s["waiting"] > 0:  # !IsInactive, ActivationData.cs:605-611
                    kind = "active"
                    r = self.schedule_collection(it)
                elif not now - it.became_idle >= it.age_limit:  # !IsStale, ActivationData.cs:635-638
                    kind = "not_stale"
                    r = self.schedule_collection(it)
                else:
                    kind = "condemned"
                    self.cov["idleness_eq_age_limit"] += now - it.became_idle == it.age_limit
                    s["state"] = L.ACT_DEACTIVATING  # PrepareForDeactivation, ActivationData.cs:337-341
                    result.append(it.a)
                self.cov["stale_" + kind] += 1
                counts[{"bad_state": L.SCAN_BAD_STATE, "kept_alive": L.SCAN_KEPT_ALIVE, "active": L.SCAN_ACTIVE,
                        "not_stale": L.SCAN_NOT_STALE, "condemned": L.SCAN_CONDEMNED}[kind]] += 1
                counts[L.SCAN_UNSCHEDULED] += r is not None and r != L.SCHED_DONE
        return sorted(result), counts

    def scan_all(self, state, age_limit, now):
        """:291-345.  -> (condemned handles ascending, counts)."""
        self.now = now = int(now)
        counts = np.zeros(8, np.uint64)
        counts[L.SCAN_CANCELLED_SKIPPED] = self._cancelled_below(None)
        result = []
        for b in list(self.buckets.values()):
            for it in list(b.items.values()):
                if it is None:  # lock(null) in the reference
                    continue
                counts[L.SCAN_CANDIDATES] += 1
                s = state[it.a]
                if s["state"] != L.ACT_VALID:
                    counts[L.SCAN_BAD_STATE] += 1
                elif it.keep_alive_until >= now:
                    counts[L.SCAN_KEPT_ALIVE] += 1
                elif s["num_running"] > 0 or s["waiting"] > 0:
                    counts[L.SCAN_ACTIVE] += 1
                elif now - it.became_idle >= age_limit:
                    assert b.try_cancel(it)
                    s["state"] = L.ACT_DEACTIVATING
                    result.append(it.a)
                    counts[L.SCAN_CONDEMNED] += 1
                else:
                    counts[L.SCAN_NOT_STALE] += 1
        return sorted(result), counts


def reaches_catalog(act, disp, state_before, hard, hard_stateless):
    """Per message: does it reach Catalog.GetOrCreateActivation with an existing ActivationData?  A replay of the batch in
    arrival order: c = in_flight + waiting as the earlier messages left it decides whether an OVERLOADED was
    IncomingMessageAgent's (rule 1, before the dispatcher) or EnqueueRequest's (rule 7, after the lookup)."""
    n_act = len(state_before)
    out = np.zeros(len(act), bool)
    c = {}
    for i in range(len(act)):
        a, d = int(act[i]), int(disp[i])
        if a >= n_act:
            continue
        s = state_before[a]
        if a not in c:
            c[a] = int(s["in_flight"]) + int(s["waiting"])
        lim = hard_stateless if s["flags"] & L.ACTF_STATELESS else hard
        if d in CERTAIN:
            out[i] = True
            c[a] += d in (L.ADM_RUN, L.ADM_ENQUEUE)
        elif d == L.ADM_OVERLOADED:
            out[i] = not (s["state"] == L.ACT_VALID and lim > 0 and c[a] > lim)
    return out


def complete_per_completion(ref, w, cact, ctok, now):
    """The per-completion order: completion_ref.complete's loop (Running's completion first, RunMessagePump after each)
    with ResetRunning's idle branch run whenever numRunning reads 0.  -> completion_ref.complete's results."""
    orig = Q._reset_running

    def hooked(a, s, tok, rt, cov):
        r = orig(a, s, tok, rt, cov)
        if s["num_running"] == 0:
            ref.reset_running_idle(ref.items[a], now)
        return r

    Q._reset_running = hooked
    try:
        return Q.complete(w, cact, ctok)
    finally:
        Q._reset_running = orig


# ---- the device form: per-activation arrays, numpy ----------------------------------------------------------------------
class Col:
    ARRAYS = ("ticket", "became_idle", "keep_alive_until", "age_limit", "cflags")

    def __init__(self, n_act, quantum, now0):
        self.n_act, self.quantum = int(n_act), int(quantum)
        self.next_ticket = mk(int(now0), self.quantum)
        self.ticket, self.became_idle, self.keep_alive_until, self.age_limit = (np.zeros(n_act, np.int64) for _ in range(4))
        self.cflags = np.zeros(n_act, np.uint8)

    def copy(self):
        c = Col(self.n_act, self.quantum, 1)
        c.next_ticket = self.next_ticket
        for f in self.ARRAYS:
            setattr(c, f, getattr(self, f).copy())
        return c

    def diff(self, o):
        """Names of what differs (empty = equal)."""
        return [f for f in self.ARRAYS if not np.array_equal(getattr(self, f), getattr(o, f))] + \
            (["next_ticket"] if self.next_ticket != o.next_ticket else [])


def _np_schedule_mask(col, m, now):
    """schedule on the entries of mask m that pass exempt / age checks and hold no ticket -> the mask of those done."""
    done = m & ((col.cflags & EXEMPT) == 0) & (col.age_limit >= col.quantum) & (col.ticket == 0)
    col.ticket[done] = mk(now + col.age_limit[done], col.quantum)
    col.cflags[done] &= 0xFF ^ CANCELLED
    return done


def np_schedule(col, handles, now):
    h = np.asarray(handles, np.uint32).astype(np.int64)
    counts = np.zeros(8, np.uint64)
    counts[L.SCHED_IGNORED] = int((h >= col.n_act).sum())
    m = np.zeros(col.n_act, bool)
    m[h[h < col.n_act]] = True
    ex = m & ((col.cflags & EXEMPT) != 0)
    z = m & ~ex & (col.age_limit == 0)
    bad = m & ~ex & ~z & (col.age_limit < col.quantum)
    tk = m & ~ex & ~z & ~bad & (col.ticket != 0)
    done = _np_schedule_mask(col, m, now)
    for slot, x in ((L.SCHED_DONE, done), (L.SCHED_EXEMPT, ex), (L.SCHED_AGE_ZERO, z), (L.SCHED_BAD_TIMEOUT, bad),
                    (L.SCHED_TICKETED, tk)):
        counts[slot] = int(x.sum())
    return counts


def np_cancel(col, handles):
    h = np.asarray(handles, np.uint32).astype(np.int64)
    counts = np.zeros(8, np.uint64)
    counts[L.CANCEL_IGNORED] = int((h >= col.n_act).sum())
    m = np.zeros(col.n_act, bool)
    m[h[h < col.n_act]] = True
    ex = m & ((col.cflags & EXEMPT) != 0)
    none = m & ~ex & (col.ticket == 0)
    exp = m & ~ex & ~none & (col.ticket < col.next_ticket)
    already = m & ~ex & ~none & ~exp & ((col.cflags & CANCELLED) != 0)
    done = m & ~ex & ~none & ~exp & ~already
    col.cflags[done] |= CANCELLED
    for slot, x in ((L.CANCEL_DONE, done), (L.CANCEL_EXEMPT, ex), (L.CANCEL_NO_TICKET, none), (L.CANCEL_EXPIRED, exp),
                    (L.CANCEL_ALREADY, already)):
        counts[slot] = int(x.sum())
    return counts


def np_reschedule(col, m, now, counts):
    """reschedule(a) on the entries of mask m; adds its five outcome counts."""
    live = m & ((col.cflags & EXEMPT) == 0) & (col.ticket != 0)
    exp = live & (col.ticket < col.next_ticket)
    bad = live & ~exp & (col.age_limit < col.quantum)
    go = live & ~exp & ~bad
    new = np.where(go, mk(now + np.where(go, col.age_limit, 1), col.quantum), 0)
    same = go & (new == col.ticket)
    drop = go & ~same & ((col.cflags & CANCELLED) != 0)
    move = go & ~same & ~drop
    col.ticket[exp | drop] = 0
    col.ticket[move] = new[move]
    for slot, x in ((L.COL_MOVED, move), (L.COL_SAME, same), (L.COL_EXPIRED, exp), (L.COL_CANCELLED_DROPPED, drop),
                    (L.COL_BAD_TIMEOUT, bad)):
        counts[slot] += np.uint64(x.sum())


def np_touch(col, act, disp, state_after, hard, hard_stateless, now):
    """state_after: the table as admission left it."""
    n_act = col.n_act
    act, disp = np.asarray(act, np.uint32).astype(np.int64), np.asarray(disp, np.uint8)
    ok = act < n_act
    certain, ovl = np.zeros(n_act, bool), np.zeros(n_act, bool)
    certain[act[ok & np.isin(disp, CERTAIN)]] = True
    ovl[act[ok & (disp == L.ADM_OVERLOADED)]] = True
    only = ovl & ~certain
    lim = np.where(state_after["flags"] & L.ACTF_STATELESS, hard_stateless, hard).astype(np.int64)
    c = state_after["in_flight"].astype(np.int64) + state_after["waiting"].astype(np.int64)
    rule1 = only & (state_after["state"] == L.ACT_VALID) & (lim > 0) & (c > lim)
    touched = certain | (only & ~rule1)
    counts = np.zeros(8, np.uint64)
    counts[L.COL_TOUCHED], counts[L.COL_RULE1_ONLY], counts[L.COL_RULE7_ONLY] = touched.sum(), rule1.sum(), (only & ~rule1).sum()
    np_reschedule(col, touched, now, counts)
    return counts


def np_on_complete(col, cact, ctok, state_before, now):
    cact, ctok = np.asarray(cact, np.uint32).astype(np.int64), np.asarray(ctok, np.uint32)
    counts = np.zeros(8, np.uint64)
    ok = cact < col.n_act
    counts[L.COL_IGNORED] = int((~ok).sum())
    comp = ok & (ctok != L.TOK_NONE) & (ctok != L.TOK_DRAIN)
    counts[L.COL_COMPLETIONS] = int(comp.sum())
    k = np.bincount(cact[comp], minlength=col.n_act)
    idle = (k >= 1) & (k >= state_before["num_running"].astype(np.int64))
    counts[L.COL_BECAME_IDLE] = int(idle.sum())
    col.became_idle[idle] = now
    np_reschedule(col, idle, now, counts)
    return counts


def _np_decide(col, state, cand, age, now, counts):
    bad = cand & (state["state"] != L.ACT_VALID)
    kept = cand & ~bad & (col.keep_alive_until >= now)
    active = cand & ~bad & ~kept & ((state["num_running"] > 0) | (state["waiting"] > 0))
    young = cand & ~bad & ~kept & ~active & (now - col.became_idle < age)
    condemned = cand & ~bad & ~kept & ~active & ~young
    for slot, x in ((L.SCAN_CANDIDATES, cand), (L.SCAN_BAD_STATE, bad), (L.SCAN_KEPT_ALIVE, kept), (L.SCAN_ACTIVE, active),
                    (L.SCAN_NOT_STALE, young), (L.SCAN_CONDEMNED, condemned)):
        counts[slot] = int(x.sum())
    return kept | active | young, condemned


def np_scan_stale(col, state, now):
    """state updated in place.  -> (condemned handles ascending uint32, counts)."""
    counts = np.zeros(8, np.uint64)
    nn = col.next_ticket
    if nn <= now:
        nn += ((now - nn) // col.quantum + 1) * col.quantum
    if nn == col.next_ticket:
        return np.zeros(0, np.uint32), counts
    col.next_ticket = nn
    due = (col.ticket != 0) & (col.ticket < nn)
    cancelled = (col.cflags & CANCELLED) != 0
    counts[L.SCAN_CANCELLED_SKIPPED] = int((due & cancelled).sum())
    cand = due & ~cancelled
    deferred, condemned = _np_decide(col, state, cand, col.age_limit, now, counts)
    col.ticket[cand] = 0
    col.cflags[cand] |= CANCELLED  # CancelAll; Add clears it again
    done = _np_schedule_mask(col, deferred, now)
    counts[L.SCAN_UNSCHEDULED] = int((deferred & ~done).sum())
    state["state"][condemned] = L.ACT_DEACTIVATING
    return np.nonzero(condemned)[0].astype(np.uint32), counts


def np_scan_all(col, state, age_limit, now):
    counts = np.zeros(8, np.uint64)
    cancelled = (col.cflags & CANCELLED) != 0
    counts[L.SCAN_CANCELLED_SKIPPED] = int(((col.ticket != 0) & cancelled).sum())
    cand = (col.ticket != 0) & ~cancelled
    _, condemned = _np_decide(col, state, cand, age_limit, now, counts)
    col.cflags[condemned] |= CANCELLED
    state["state"][condemned] = L.ACT_DEACTIVATING
    return np.nonzero(condemned)[0].astype(np.uint32), counts


# ---- scenarios: a start (Col, table) and a list of calls -----------------------------------------------------------------
# An op is a tuple: ("schedule", handles, now), ("cancel", handles), ("touch", act, mflags, hard, hard_stateless, now) (the
# batch is admitted first, by orl_admit_device / admission_ref), ("on_complete", cact, ctok, now), ("scan_stale", now),
# ("scan_all", age_limit, now).
SEC = L.TICKS_PER_SECOND
T0 = 630_000_000 * SEC  # a DateTime in ticks; a multiple of every quantum used here
QUANTUM = 60 * SEC


class Scenario:
    def __init__(self, name, col, state, ops, max_batch=1 << 16):
        self.name, self.col, self.state, self.ops, self.max_batch = name, col, state, ops, max_batch

    @property
    def n_act(self):
        return self.col.n_act


class Step:
    """What the model says after one op: the collector, the table, the list (None unless a scan) and the counts; for a
    touch also admission's dispositions."""

    def __init__(self, op, col, state, condemned, counts, disp=None):
        self.op, self.col, self.state, self.condemned, self.counts, self.disp = op, col, state, condemned, counts, disp


def run_numpy(sc):
    """The numpy form over a scenario -> [Step]."""
    col, state = sc.col.copy(), sc.state.copy()
    out = []
    for op in sc.ops:
        condemned = disp = None
        if op[0] == "schedule":
            counts = np_schedule(col, op[1], op[2])
        elif op[0] == "cancel":
            counts = np_cancel(col, op[1])
        elif op[0] == "touch":
            disp, state, _ = A.admit(op[1], op[2], state, sc.n_act, op[3], op[4])
            counts = np_touch(col, op[1], disp, state, op[3], op[4], op[5])
        elif op[0] == "on_complete":
            counts = np_on_complete(col, op[1], op[2], state, op[3])
        elif op[0] == "scan_stale":
            condemned, counts = np_scan_stale(col, state, op[1])
        else:
            assert op[0] == "scan_all", op[0]
            condemned, counts = np_scan_all(col, state, op[1], op[2])
        out.append(Step(op, col.copy(), state.copy(), condemned, counts, disp))
    return out


def run_literal(sc, cov=None):
    """The literal reference over a scenario -> [Step] (Step.col is the export)."""
    ref, state = RefCollector.from_col(sc.col, cov), sc.state.copy()
    out = []
    for op in sc.ops:
        condemned = disp = None
        if op[0] == "schedule":
            counts = ref.schedule(op[1], op[2])
        elif op[0] == "cancel":
            counts = ref.cancel(op[1])
        elif op[0] == "touch":
            before = state
            disp, state, _ = A.admit(op[1], op[2], before, sc.n_act, op[3], op[4])
            counts = ref.touch(op[1], disp, before, op[3], op[4], op[5])
        elif op[0] == "on_complete":
            counts = ref.on_complete(op[1], op[2], state, op[3])
        elif op[0] == "scan_stale":
            condemned, counts = ref.scan_stale(state, op[1])
            condemned = np.asarray(condemned, np.uint32)
        else:
            condemned, counts = ref.scan_all(state, op[1], op[2])
            condemned = np.asarray(condemned, np.uint32)
        out.append(Step(op, ref.export(), state.copy(), condemned, counts, disp))
    return out


def idle_valid_state(n_act):
    s = np.zeros(n_act, STATE_DTYPE)
    s["state"] = L.ACT_VALID
    return s


def fresh_col(n_act, age=2 * QUANTUM, now0=T0):
    col = Col(n_act, QUANTUM, now0)
    col.age_limit[:] = age
    return col


GPU_N_ACT = (1, 5, 2047, 2048, 2049, 5000, 1 << 20)
# The chunked regime of the one-workgroup tile scan (admission_ref.CHUNK_N): 1024, 1025 and 2049 tiles of activations, so
# that a scan thread owns 1, 2 and 3 tile counts.  Compared with the numpy form only.
CHUNK_N_ACT = A.CHUNK_N
CHUNK_DENSITIES = ("one-per-tile", "all")


def density_scenario(n_act, density):
    """Everything scheduled at T0 + 1, idle since T0; ScanStale three quanta later (several quanta dequeued in one scan)
    with the condemned density `none` (all kept alive), `all`, or `one-per-tile` (the others kept alive; the survivor of
    tile t sits at 2047, 0, 1, 2047, ... and the last handle is one), then a scan with nothing to dequeue, then ScanAll
    (which condemns what ScanStale deferred once their keep-alive has passed)."""
    col, state = fresh_col(n_act), idle_valid_state(n_act)
    col.became_idle[:] = T0
    h = np.arange(n_act, dtype=np.uint32)
    if density == "none":
        col.keep_alive_until[:] = I64_MAX
    elif density == "one-per-tile":
        col.keep_alive_until[:] = T0 + 4 * QUANTUM
        tiles = (n_act + 2047) // 2048
        pick = np.minimum(np.arange(tiles) * 2048 + np.array([2047, 0, 1])[np.arange(tiles) % 3], n_act - 1)
        col.keep_alive_until[pick] = np.where(np.arange(tiles) % 2, 0, I64_MIN)
        col.keep_alive_until[n_act - 1] = 0
    now = T0 + 3 * QUANTUM + 1
    ops = [("schedule", np.concatenate([h, np.array([n_act, 0xFFFFFFFF], np.uint32)]), T0 + 1), ("scan_stale", now),
           ("scan_stale", now + 5), ("scan_all", QUANTUM, now + 2 * QUANTUM)]
    return Scenario(f"density-{density}-a{n_act}", col, state, ops, max_batch=max(1 << 16, n_act + 2))


def edge_scenario(n_act=5000):
    """Condemned handles exactly at 2047 / 2048 / 2049 / 4095 / 4096 and n_act - 1: only those are idle long enough."""
    col, state = fresh_col(n_act), idle_valid_state(n_act)
    col.became_idle[:] = T0 + 2 * QUANTUM  # too young at the scan
    edges = np.array([2047, 2048, 2049, 4095, 4096, n_act - 1])
    col.became_idle[edges] = T0
    now = T0 + 3 * QUANTUM
    return Scenario("edges", col, state, [("schedule", np.arange(n_act, dtype=np.uint32), T0 + 1), ("scan_stale", now),
                                          ("scan_all", 3 * QUANTUM, now + 1)])


def matrix_scenario():
    """Every state value 0..7 x cflags 0..3 x (idle, running, waiting) on neighbouring handles, ticketed for the first
    quantum where the flags allow a live ticket; ScanAll, then ScanStale, then the same again a quantum later."""
    combos = [(st, cf, busy) for st in range(8) for cf in range(4) for busy in range(3)]
    n_act = len(combos)
    col, state = fresh_col(n_act), np.zeros(n_act, STATE_DTYPE)
    for h, (st, cf, busy) in enumerate(combos):
        state[h] = (st, 0, 0, 1 if busy == 1 else 0, 1 if busy == 1 else 0, 1 if busy == 2 else 0)
        col.cflags[h] = cf
        col.ticket[h] = T0 + QUANTUM * (1 + h % 2)
    col.became_idle[:] = T0 - 5 * QUANTUM
    h = np.arange(n_act, dtype=np.uint32)
    return Scenario("state-x-cflags", col, state, [("scan_all", QUANTUM, T0 + 1), ("scan_stale", T0 + QUANTUM),
                                                   ("cancel", h), ("schedule", h, T0 + QUANTUM + 1),
                                                   ("scan_all", QUANTUM, T0 + 2 * QUANTUM), ("scan_stale", T0 + 2 * QUANTUM)])


def _requests(n, handle, flags=L.MF_REQUEST):
    return np.full(n, handle, np.uint32), np.full(n, flags, np.uint8)


def touch_scenario(n, n_act=300):
    """A random admitted batch of n messages (admission_ref.shape_scenario: a hot handle, 5 % unresolved) over random
    states, with the rule-1-only and rule-7-only activations for L = hard 2 and L = hard_stateless 1 planted on handles
    0..3 when the batch is long enough: c0 = L + 1 (rule 1: every message rejected before the dispatcher) and c0 = L with
    Running a read-write request (rule 7: every request rejected by EnqueueRequest).  Tickets: live, none, cancelled."""
    rng = np.random.default_rng([n, n_act, 18])
    base = A.shape_scenario(n, n_act)
    act, fl = base.act.copy(), base.mflags.copy()
    state = base.state.copy()
    state["waiting"] = np.minimum(state["waiting"], 1)
    state["in_flight"] = np.minimum(state["in_flight"], 1)
    busy = L.ACTF_RUNNING_SET
    planted = ((0, 0, 3), (1, 0, 2), (2, L.ACTF_STATELESS, 2), (3, L.ACTF_STATELESS, 1))  # handle, flags, c0
    for h, f, c0 in planted:
        if h < n_act:
            state[h] = (L.ACT_VALID, busy | f, 0, 1, c0, 0)
    if n >= 63 and n_act > 4:
        act[act < 4] = 4
        idx = rng.permutation(n)[:16]
        act[idx] = np.repeat(np.arange(4, dtype=np.uint32), 4)
        fl[idx] = L.MF_REQUEST
    col = fresh_col(n_act)
    col.ticket[:] = np.where(rng.random(n_act) < 0.7, T0 + QUANTUM * rng.integers(1, 3, n_act), 0)
    col.cflags[:] = np.where((rng.random(n_act) < 0.2) & (col.ticket != 0), CANCELLED, 0)
    col.cflags[rng.random(n_act) < 0.05] |= EXEMPT
    col.age_limit[rng.random(n_act) < 0.05] = QUANTUM - 1
    return Scenario(f"touch-n{n}-a{n_act}", col, state, [("touch", act, fl, 2, 1, T0 + 7), ("touch", act, fl, 2, 1, T0 + 7),
                                                         ("touch", act[: n // 2], fl[: n // 2], 2, 1, T0 + QUANTUM + 7)])


TOUCH_N = (0, 1, 63, 64, 65, 4097, 40_001)


def quirk_scenario():
    """ScanAll condemns handle 0 (cancelled in place, the ticket stays), then a message arrives for it: the touch finds a
    cancelled item and drops the ticket; handle 1 the same but touched when the new ticket equals the old one (nothing
    happens, the flag stays); handle 2's cancelled ticket has expired by the time it is touched; handle 3 has age limit
    below the quantum; handle 4 is scheduled twice."""
    n_act = 6
    col, state = fresh_col(n_act), idle_valid_state(n_act)
    col.became_idle[:] = T0 - 10 * QUANTUM
    col.age_limit[1] = 3 * QUANTUM
    col.age_limit[3] = QUANTUM - 1
    col.ticket[3] = T0 + 2 * QUANTUM
    col.keep_alive_until[5] = I64_MAX
    h = np.array([0, 1, 2, 4, 5], np.uint32)
    act0, fl0 = _requests(2, 0)
    act1, fl1 = _requests(1, 1)
    act2, fl2 = _requests(1, 2)
    act3, fl3 = _requests(1, 3)
    ops = [("schedule", h, T0 + 1), ("schedule", np.array([4], np.uint32), T0 + 2), ("scan_all", QUANTUM, T0 + 3),
           ("touch", act1, fl1, 0, 0, T0 + 4),                      # new == old on a cancelled item
           ("touch", np.concatenate([act0, act3]), np.concatenate([fl0, fl3]), 0, 0, T0 + QUANTUM + 4),  # dropped; bad timeout
           ("scan_stale", T0 + 3 * QUANTUM),                        # handle 2's cancelled item is skipped; 5 kept alive
           ("touch", act2, fl2, 0, 0, T0 + 3 * QUANTUM + 1),        # expired
           ("scan_stale", T0 + 3 * QUANTUM + 2)]                    # nothing dequeued
    return Scenario("scan-all-then-touch", col, state, ops)


def branch_scenario():
    """One activation per ScanStale branch, with the exact-boundary values: keep_alive_until == now, idleness == age limit,
    a schedule at an exact multiple of the quantum and one tick past it."""
    n_act = 8
    col, state = fresh_col(n_act, age=QUANTUM), idle_valid_state(n_act)
    now = T0 + 2 * QUANTUM
    col.became_idle[:] = now - QUANTUM          # idleness == age limit: stale
    state[0]["state"] = L.ACT_DEACTIVATING      # bad state
    col.keep_alive_until[1] = now               # kept alive, exactly
    col.keep_alive_until[2] = now - 1           # not kept alive: condemned
    state[3]["num_running"] = state[3]["in_flight"] = 1  # active
    state[4]["waiting"] = 1                     # active
    col.became_idle[5] = now - QUANTUM + 1      # not stale by one tick
    h = np.arange(n_act, dtype=np.uint32)
    ops = [("schedule", h[:7], T0), ("schedule", h[7:], T0 + 1), ("cancel", np.array([6, 6 + n_act], np.uint32)),
           ("scan_stale", now), ("on_complete", np.array([3, 3, 4, n_act, 5], np.uint32),
                                 np.array([9, L.TOK_NONE, L.TOK_DRAIN, 7, 8], np.uint32), now + 1),
           ("scan_stale", now + 3 * QUANTUM)]
    return Scenario("stale-branches", col, state, ops)


def list_scenario(n_act=5000):
    """schedule / cancel lists with out-of-range handles among distinct in-range ones."""
    rng = np.random.default_rng(77)
    col, state = fresh_col(n_act), idle_valid_state(n_act)
    col.cflags[rng.random(n_act) < 0.1] = EXEMPT
    col.age_limit[rng.random(n_act) < 0.1] = 0
    col.age_limit[rng.random(n_act) < 0.05] = 5
    bad = np.array([n_act, n_act + 1, 0x80000000, 0xFFFFFFFF], np.uint32)
    h1 = np.concatenate([rng.permutation(n_act)[:3000].astype(np.uint32), bad])
    h2 = np.concatenate([rng.permutation(n_act)[:2500].astype(np.uint32), bad[:2]])
    return Scenario("lists", col, state, [("schedule", rng.permutation(h1), T0 + 1), ("cancel", rng.permutation(h2)),
                                          ("schedule", rng.permutation(h1), T0 + 2), ("cancel", rng.permutation(h2)),
                                          ("scan_stale", T0 + 4 * QUANTUM)])


def all_scenarios(big=True):
    """Every scenario of the GPU file except the chained rounds."""
    out = [density_scenario(a, d) for a in GPU_N_ACT if big or a <= 5000 for d in ("none", "all", "one-per-tile")]
    out += [edge_scenario(), matrix_scenario(), quirk_scenario(), branch_scenario(), list_scenario()]
    out += [touch_scenario(n) for n in TOUCH_N if big or n <= 4097]
    return out


# ---- chained rounds and random histories -----------------------------------------------------------------------------------
def history(seed, n_act=24, rounds=6, respect_call_sites=True):
    """A random small history: a consistent World (completion_ref), a collector in which every VALID activation was
    scheduled, and per round (admitted batch, completion batch, times, which scan).  Generated lazily by play()."""
    rng = np.random.default_rng([seed, 4242])
    w = Q.consistent_world(rng, n_act, max_wait=2, p_wait=0.5)
    col = fresh_col(n_act, age=QUANTUM)
    col.age_limit[:] = QUANTUM * rng.integers(1, 4, n_act)
    col.cflags[rng.random(n_act) < 0.08] = EXEMPT
    col.keep_alive_until[rng.random(n_act) < 0.1] = T0 + QUANTUM * int(rng.integers(1, 5))
    return rng, w, col


def play(seed, per_completion=False, rounds=6, n_act=24, n_msgs=40, cov=None):
    """One history through the literal model: admit -> touch -> on-complete -> complete -> scan, several quanta long.
    per_completion: the completion step runs the literal per-completion loop instead of the batched rule.
    -> [(condemned of the round's scan, became_idle of the inactive activations {a: t}, export, World)]."""
    rng, w, col = history(seed, n_act, rounds)
    ref = RefCollector.from_col(col, cov)
    ref.schedule(np.nonzero(w.state["state"] == L.ACT_VALID)[0], T0 + 1)
    now = T0 + 1
    out = []
    hard, hsw = 5, 3
    for r in range(rounds):
        now += int(rng.integers(1, QUANTUM))
        n = int(rng.integers(0, n_msgs))
        act = rng.integers(0, n_act + 1, n).astype(np.uint32)
        fl = A.random_flags(rng, n, p_ro=0.3)
        tok = (0x50000000 + 1000 * r + np.arange(n)).astype(np.uint32)
        disp, st, _ = A.admit(act, fl, w.state, n_act, hard, hsw)
        ref.touch(act, disp, w.state, hard, hsw, now)
        w1 = Q.append(w, act, tok, fl, disp)
        w1.state = st
        now += int(rng.integers(1, QUANTUM // 2))
        cact, ctok = Q.random_completions(rng, w1, int(rng.integers(0, n_msgs)), p_running=0.8, p_bad=0.02)
        if per_completion:
            w, _, _ = complete_per_completion(ref, w1, cact, ctok, now)
        else:
            ref.on_complete(cact, ctok, w1.state, now)
            w, _, _ = Q.complete(w1, cact, ctok)
        now += int(rng.integers(1, 2 * QUANTUM))
        if rng.random() < 0.7:
            condemned, _ = ref.scan_stale(w.state, now)
        else:
            condemned, _ = ref.scan_all(w.state, QUANTUM * int(rng.integers(1, 3)), now)
        # Catalog's deactivation of the condemned: DequeueAllWaitingMessages, then the activation is gone; a new one takes
        # the handle later (ScheduleCollection after InvokeActivate, Catalog.cs:507)
        for a in condemned:
            if rng.random() < 0.5:
                w.state[a] = (L.ACT_VALID, w.state[a]["flags"] & L.ACTF_REENTRANT, 0, 0, 0, 0)
                ref.items[a].ticket, ref.items[a].cancelled, ref.items[a].became_idle = 0, False, now
                for b in ref.buckets.values():
                    b.items.pop(a, None)
                ref.schedule([a], now)
        idle = {a: ref.items[a].became_idle for a in range(n_act)
                if w.state[a]["num_running"] == 0 and w.state[a]["waiting"] == 0}
        out.append((list(condemned), idle, ref.export(), w.copy()))
    return out


def play_numpy(seed, rounds=6, n_act=24, n_msgs=40):
    """The same history through the numpy form and the literal model side by side -> [(what, literal Col, numpy Col)]
    wherever they differ (empty = equal), comparing arrays, tables, lists and counts after every call."""
    rng, w, col = history(seed, n_act, rounds)
    ref = RefCollector.from_col(col)
    col = col.copy()
    diffs = []

    def cmp(what, c1, c2, extra1=None, extra2=None):
        d = ref.export().diff(col)
        if d or not np.array_equal(c1, c2) or (extra1 is not None and list(extra1) != list(extra2)):
            diffs.append((what, d, list(c1), list(c2)))

    valid = np.nonzero(w.state["state"] == L.ACT_VALID)[0]
    cmp("schedule", ref.schedule(valid, T0 + 1), np_schedule(col, valid, T0 + 1))
    now = T0 + 1
    hard, hsw = 5, 3
    for r in range(rounds):
        now += int(rng.integers(1, QUANTUM))
        n = int(rng.integers(0, n_msgs))
        act = rng.integers(0, n_act + 1, n).astype(np.uint32)
        fl = A.random_flags(rng, n, p_ro=0.3)
        tok = (0x50000000 + 1000 * r + np.arange(n)).astype(np.uint32)
        disp, st, _ = A.admit(act, fl, w.state, n_act, hard, hsw)
        cmp(("touch", r), ref.touch(act, disp, w.state, hard, hsw, now), np_touch(col, act, disp, st, hard, hsw, now))
        w1 = Q.append(w, act, tok, fl, disp)
        w1.state = st
        now += int(rng.integers(1, QUANTUM // 2))
        cact, ctok = Q.random_completions(rng, w1, int(rng.integers(0, n_msgs)), p_running=0.8, p_bad=0.02)
        cmp(("on_complete", r), ref.on_complete(cact, ctok, w1.state, now), np_on_complete(col, cact, ctok, w1.state, now))
        w, _, _ = Q.complete(w1, cact, ctok)
        now += int(rng.integers(1, 2 * QUANTUM))
        s1, s2 = w.state.copy(), w.state.copy()
        if rng.random() < 0.7:
            (l1, c1), (l2, c2) = ref.scan_stale(s1, now), np_scan_stale(col, s2, now)
        else:
            age = QUANTUM * int(rng.integers(1, 3))
            (l1, c1), (l2, c2) = ref.scan_all(s1, age, now), np_scan_all(col, s2, age, now)
        cmp(("scan", r), c1, c2, l1, l2)
        if not np.array_equal(s1, s2):
            diffs.append((("scan table", r), [], [], []))
        w.state = s1
        if r % 2 == 1:  # Catalog's own deactivations: PrepareForDeactivation, then TryCancelCollection (Catalog.cs:803-804)
            h = rng.permutation(n_act)[:3]
            w.state["state"][h] = np.where(w.state["state"][h] == L.ACT_VALID, L.ACT_DEACTIVATING, w.state["state"][h])
            cmp(("cancel", r), ref.cancel(h), np_cancel(col, h))
    return diffs


def chain_rounds(n_act=64):
    """Three rounds of bucket -> admit -> append -> touch -> on-complete -> complete -> scan over one table, one queue and
    one collector: -> (World, Col, [(act, mflags, tok, cact, ctok, t_touch, t_complete, t_scan, scan kind)], limits, and
    the expected [(disp, Col, state, condemned, touch counts, on-complete counts, scan counts)])."""
    rng = np.random.default_rng(36)
    w = Q.consistent_world(rng, n_act, max_wait=2)
    col = fresh_col(n_act, age=QUANTUM)
    col.became_idle[:] = T0 - QUANTUM
    np_schedule(col, np.arange(n_act), T0 + 1)
    hard, hsw = 60, 30
    now = T0 + 1
    rounds, expect = [], []
    for r, n in enumerate((5000, 2049, 7000)):
        act = rng.integers(0, n_act + 4, n).astype(np.uint32)
        act[act % 4 == 1] = 0  # three quarters of the activations get messages; the others go stale
        fl = A.random_flags(rng, n, p_ro=0.3)
        tok = (0x50000000 + 10000 * r + np.arange(n)).astype(np.uint32)
        t_touch, t_cmp, t_scan = now + 5, now + 9, now + QUANTUM * (1 + r) + 11
        now = t_scan
        disp, st, _ = A.admit(act, fl, w.state, n_act, hard, hsw)
        c_touch = np_touch(col, act, disp, st, hard, hsw, t_touch)
        w1 = Q.append(w, act, tok, fl, disp)
        w1.state = st
        cact, ctok = Q.random_completions(rng, w1, 300, p_running=0.7)
        c_cmp = np_on_complete(col, cact, ctok, w1.state, t_cmp)
        w, _, _ = Q.complete(w1, cact, ctok)
        kind = "scan_all" if r == 1 else "scan_stale"
        condemned, c_scan = (np_scan_all(col, w.state, QUANTUM, t_scan) if r == 1 else np_scan_stale(col, w.state, t_scan))
        rounds.append((act, fl, tok, cact, ctok, t_touch, t_cmp, t_scan, kind))
        expect.append((disp, col.copy(), w.state.copy(), condemned, c_touch, c_cmp, c_scan))
    return rounds, (hard, hsw), expect


def chain_start(n_act=64):
    """The World and collector chain_rounds starts from (the same seed)."""
    rng = np.random.default_rng(36)
    w = Q.consistent_world(rng, n_act, max_wait=2)
    col = fresh_col(n_act, age=QUANTUM)
    col.became_idle[:] = T0 - QUANTUM
    np_schedule(col, np.arange(n_act), T0 + 1)
    return w, col
