"""orl_waitq_append_device and orl_complete_device on the GPU against the sequential model (completion_ref): a round is
orl_bucket_device -> orl_admit_device -> orl_waitq_append_device, then orl_bucket_device over the completion records ->
orl_complete_device, all on the context's stream with no synchronise between (the table and running_tok as the append left
them are kept by two device-to-device copies on that stream; the append's store is still in the buffer the complete read).
After the append and after the complete, the store (off, tok, act, mflags), running_tok, the whole state table, the out
list and d_counts are compared exactly.  The scenarios are completion_ref's builders; tests/test_completion_ref.py holds
them to the model's coverage counters.

A start store is loaded through the interface itself: its records as one batch whose dispositions are all ORL_ADM_ENQUEUE,
bucketed and appended, and running_tok written through the view.

Tile = 2048 records / positions (256 threads x 8).
"""
import numpy as np
import pytest

import admission_ref as A
import completion_ref as Q
from orleans_amd import _lib as L
from orleans_amd import workloads as W
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError

pytestmark = pytest.mark.gpu

MAX_BATCH = 1 << 16


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _engine(n_act, max_batch=MAX_BATCH):
    eng = GrainDirectoryEngine(n_act=n_act, dir_capacity=16, max_batch=max_batch, device=0)
    W.setup_engine(eng, W.default_cluster())
    return eng


def _dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _host(eng, p, count, dtype):
    out = np.zeros(count, dtype)
    if count:
        eng.copy_to_host(out, int(p))
    return out


class Snapshot:
    """What a view points at, downloaded."""

    def __init__(self, eng, v, n_act, d_state=None, d_running_tok=None):
        self.waiting_n = int(_host(eng, v.d_waiting_n, 1, np.uint64)[0])
        self.off = _host(eng, v.d_off, n_act + 1, np.uint32)
        n = int(self.off[-1])
        self.tok, self.act = _host(eng, v.d_tok, n, np.uint32), _host(eng, v.d_act, n, np.uint32)
        self.mflags = _host(eng, v.d_mflags, n, np.uint8)
        self.running_tok = _host(eng, v.d_running_tok if d_running_tok is None else d_running_tok.data_ptr(), n_act,
                                 np.uint32)
        self.state = None if d_state is None else d_state.cpu().numpy().view(Q.STATE_DTYPE)
        self.out_n = int(_host(eng, v.d_out_n, 1, np.uint64)[0])
        self.out = [_host(eng, p, self.out_n, d) for p, d in ((v.d_out_tok, np.uint32), (v.d_out_act, np.uint32),
                                                             (v.d_out_mflags, np.uint8), (v.d_out_kind, np.uint8))]

    def check_store(self, w, what, current=True):
        """current = False: an earlier view, whose store buffers the later call left alone; the two lengths are the
        queue's and have moved on."""
        assert np.array_equal(self.off, w.off), (what, "off", np.nonzero(self.off != w.off)[0][:8])
        assert not current or self.waiting_n == len(w.tok), what
        for name, got, exp in (("tok", self.tok, w.tok), ("act", self.act, w.act), ("mflags", self.mflags, w.mflags),
                               ("running_tok", self.running_tok, w.running_tok)):
            bad = np.nonzero(got != exp)[0]
            assert len(bad) == 0, (what, name, len(bad), bad[:8], got[bad[:8]], exp[bad[:8]])
        if self.state is not None:
            bad = np.nonzero(self.state != w.state)[0]
            assert len(bad) == 0, (what, "state", len(bad), bad[:4], self.state[bad[:4]], w.state[bad[:4]])

    def check_out(self, out, what):
        assert self.out_n == len(out), (what, self.out_n, len(out))
        for col, got in enumerate(self.out):
            exp = np.array([o[col] for o in out], got.dtype)
            bad = np.nonzero(got != exp)[0]
            assert len(bad) == 0, (what, "out column", col, len(bad), bad[:8], got[bad[:8]], exp[bad[:8]])


def _bucket_arrays(t, n, n_act):
    return (t.full((max(n, 1),), -1, dtype=t.int32, device="cuda"), t.full((n_act + 2,), -1, dtype=t.int32, device="cuda"))


def _load(t, eng, q, w):
    """The World's store and running_tok into an empty queue, through append and the view."""
    n = len(w.tok)
    if n:
        d_act, d_tok, d_fl = _dev(t, w.act), _dev(t, w.tok), _dev(t, w.mflags)
        disp = t.full((n,), L.ADM_ENQUEUE, dtype=t.uint8, device="cuda")
        order, off = _bucket_arrays(t, n, w.n_act)
        t.cuda.synchronize()
        eng.bucket_device(d_act, n, order, off)
        eng.waitq_append_device(q, d_tok, d_fl, n, order, off, disp)
        eng.sync()
    d_rt = _dev(t, w.running_tok)
    t.cuda.synchronize()
    eng.copy_on_device(eng.waitq_view(q).d_running_tok, d_rt, 4 * w.n_act)
    eng.sync()


def _round(t, eng, q, n_act, d_state, act, tok, mflags, hard, hsw, cact, ctok, with_counts=True):
    """One round on the context's stream; -> (disp, admit counts, Snapshot after the append, Snapshot after the complete,
    complete counts)."""
    n, m = len(act), len(cact)
    d_act, d_tok, d_fl, d_cact, d_ctok = (_dev(t, x) for x in (act, tok, mflags, cact, ctok))
    order, off = _bucket_arrays(t, n, n_act)
    corder, coff = _bucket_arrays(t, m, n_act)
    disp = t.full((max(n, 1),), 0xEE, dtype=t.uint8, device="cuda")
    acounts = t.full((8,), -1, dtype=t.int64, device="cuda")
    counts = t.full((8,), -1, dtype=t.int64, device="cuda") if with_counts else None
    state1 = t.zeros_like(d_state)
    rt1 = t.zeros(n_act, dtype=t.int32, device="cuda")
    t.cuda.synchronize()  # the uploads and fills are on torch's stream, the calls on the context's
    eng.bucket_device(d_act, n, order, off)
    eng.admit_device(d_act, d_fl, n, order, off, d_state, disp, hard, hsw, acounts)
    eng.waitq_append_device(q, d_tok, d_fl, n, order, off, disp)
    v1 = eng.waitq_view(q)
    eng.copy_on_device(state1, d_state, d_state.numel())
    eng.copy_on_device(rt1, v1.d_running_tok, 4 * n_act)
    eng.bucket_device(d_cact, m, corder, coff)
    eng.complete_device(q, d_cact, d_ctok, m, corder, coff, d_state, counts)
    v2 = eng.waitq_view(q)
    eng.sync()
    t.cuda.synchronize()
    s1 = Snapshot(eng, v1, n_act, state1, rt1)
    s2 = Snapshot(eng, v2, n_act, d_state)
    return (disp.cpu().numpy()[:n], acounts.cpu().numpy().view(np.uint64), s1, s2,
            counts.cpu().numpy().view(np.uint64) if with_counts else None)


def _check(t, eng, sc, with_counts=True):
    e_disp, e_acounts, w1, w2, e_out, e_counts = sc.expect()
    q = eng.waitq_create(sc.capacity)
    try:
        _load(t, eng, q, sc.world)
        d_state = _dev(t, sc.world.state)
        disp, acounts, s1, s2, counts = _round(t, eng, q, sc.n_act, d_state, sc.act, sc.tok, sc.mflags, sc.hard,
                                               sc.hard_stateless, sc.cact, sc.ctok, with_counts)
        assert np.array_equal(disp, e_disp) and list(acounts) == list(e_acounts), sc.name
        s1.check_store(w1, (sc.name, "after append"), current=False)
        s2.check_store(w2, (sc.name, "after complete"))
        s2.check_out(e_out, sc.name)
        if with_counts:
            assert list(counts) == list(e_counts), (sc.name, list(counts), list(e_counts))
    finally:
        eng.waitq_destroy(q)


@pytest.mark.parametrize("n_act", Q.SHAPE_N_ACT)
def test_shapes_vs_model(torch, n_act):
    """n = m in {0, 1, 63, 64, 65, 257, 4097, 40 001} at this n_act: a random consistent store, a random admitted batch
    with a hot handle and 5 % unresolved, random completion, pump and drain records and handles >= n_act."""
    eng = _engine(n_act, max_batch=1 << 18)
    try:
        for n in Q.SHAPE_N:
            _check(torch, eng, Q.shape_scenario(n, n_act))
    finally:
        eng.close()


def test_one_segment_across_tiles_vs_model(torch):
    """One activation holds the whole store across more than three tiles: the first failing record at a tile boundary
    - 1, at it and + 1 (both inner boundaries), no failing record (the whole segment taken), a failing head."""
    eng = _engine(3)
    try:
        for sc in Q.one_segment_scenarios():
            _check(torch, eng, sc)
    finally:
        eng.close()


@pytest.mark.parametrize("k", range(6, 14))
def test_segment_boundaries_vs_model(torch, k):
    """A segment whose start and whose length are each 2^k - 1, 2^k and 2^k + 1 (nine rounds)."""
    eng = _engine(3)
    try:
        for ds in (-1, 0, 1):
            for dl in (-1, 0, 1):
                _check(torch, eng, Q.boundary_scenario(k, ds, dl))
    finally:
        eng.close()


def test_appends_into_an_empty_store_and_across_tile_edges(torch):
    for sc in Q.append_scenarios():
        eng = _engine(sc.n_act)
        try:
            _check(torch, eng, sc)
        finally:
            eng.close()


@pytest.mark.parametrize("build", [lambda: Q.state_matrix_scenario(False), lambda: Q.state_matrix_scenario(True),
                                   Q.drain_pump_scenario], ids=["state-matrix", "state-matrix-r", "drain-pump"])
def test_scenario_vs_model(torch, build):
    """Every state x flag combination x num_running 0 / 2 on neighbouring handles, without and with Running's own
    completion; drain and pump-only records alone and mixed with completions of the same activation."""
    sc = build()
    eng = _engine(sc.n_act)
    try:
        _check(torch, eng, sc)
    finally:
        eng.close()


def test_three_rounds_chained_through_one_table_and_one_queue(torch):
    t = torch
    w, rounds, (hard, hsw) = Q.chain_rounds()
    eng = _engine(w.n_act)
    q = eng.waitq_create(len(w.tok) + sum(len(r[0]) for r in rounds))
    try:
        _load(t, eng, q, w)
        d_state = _dev(t, w.state)
        for step, (act, fl, seed) in enumerate(rounds):
            tok = (0x50000000 + np.arange(len(act))).astype(np.uint32)
            e_disp, st, _ = A.admit(act, fl, w.state, w.n_act, hard, hsw)
            w1 = Q.append(w, act, tok, fl, e_disp)
            w1.state = st
            cact, ctok = Q.chain_completions(w1, seed)
            w2, e_out, e_counts = Q.complete(w1, cact, ctok)
            disp, _, s1, s2, counts = _round(t, eng, q, w.n_act, d_state, act, tok, fl, hard, hsw, cact, ctok)
            assert np.array_equal(disp, e_disp), step
            s1.check_store(w1, (step, "after append"), current=False)
            s2.check_store(w2, (step, "after complete"))
            s2.check_out(e_out, step)
            assert list(counts) == list(e_counts), step
            w = w2
    finally:
        eng.waitq_destroy(q)
        eng.close()


def test_counts_are_optional(torch):
    eng = _engine(5000)
    try:
        _check(torch, eng, Q.shape_scenario(4097, 5000), with_counts=False)
    finally:
        eng.close()


def _append_raw(t, eng, q, n_act, act, tok, mflags, disp):
    d_act, d_tok, d_fl, d_disp = (_dev(t, x) for x in (act, tok, mflags, disp))
    order, off = _bucket_arrays(t, len(act), n_act)
    t.cuda.synchronize()
    eng.bucket_device(d_act, len(act), order, off)
    eng.waitq_append_device(q, d_tok, d_fl, len(act), order, off, d_disp)
    eng.sync()


@pytest.mark.parametrize("n", Q.CHUNK_N)
def test_chunked_tile_scan_vs_closed_form(torch, n):
    """1024, 1025 and 2049 tiles: the one-workgroup tile scan's threads own chunks of 1, 2 and 3 aggregates.  An append
    of n positions into an empty store and a complete over a store of n records, each with everything in one bucket /
    segment and with a head every 3000 positions; against the numpy forms (tests/test_completion_ref.py holds them to
    the model)."""
    t = torch
    for (a_name, w0, act, tok, fl, disp), (c_name, w, cact, ctok) in zip(Q.chunk_appends(n), Q.chunk_completes(n)):
        n_act = w.n_act
        assert w0.n_act == n_act and len(act) == len(w.tok) == n
        eng = _engine(n_act, max_batch=n)
        q = eng.waitq_create(n)
        try:
            _load(t, eng, q, w0)
            _append_raw(t, eng, q, n_act, act, tok, fl, disp)
            Snapshot(eng, eng.waitq_view(q), n_act).check_store(Q.append_ref(w0, act, tok, fl, disp), a_name)
            eng.waitq_destroy(q)
            q = eng.waitq_create(n)
            _load(t, eng, q, w)
            e_w, e_out, e_counts = Q.complete_closed_form(w, cact, ctok, as_arrays=True)
            d_state, d_cact, d_ctok = _dev(t, w.state), _dev(t, cact), _dev(t, ctok)
            corder, coff = _bucket_arrays(t, len(cact), n_act)
            counts = t.full((8,), -1, dtype=t.int64, device="cuda")
            t.cuda.synchronize()
            eng.bucket_device(d_cact, len(cact), corder, coff)
            eng.complete_device(q, d_cact, d_ctok, len(cact), corder, coff, d_state, counts)
            eng.sync()
            s = Snapshot(eng, eng.waitq_view(q), n_act, d_state)
            s.check_store(e_w, c_name)
            assert s.out_n == len(e_out[0]) > 3 * 2048, (c_name, s.out_n, len(e_out[0]))
            for col, (got, exp) in enumerate(zip(s.out, e_out)):
                bad = np.nonzero(got != exp)[0]
                assert len(bad) == 0, (c_name, "out column", col, len(bad), bad[:8], got[bad[:8]], exp[bad[:8]])
            assert list(counts.cpu().numpy().view(np.uint64)) == list(e_counts), c_name
        finally:
            eng.waitq_destroy(q)
            eng.close()


def test_capacity_refresh_then_success_and_true_overflow(torch):
    """Capacity 100.  Batches of 60 messages with 10 ENQUEUEs each: after the first the library's bound says 60, so the
    second (60 + 60 > 100) asks the device (10) and goes through.  Then 20 records and a batch of 90: ORL_E_CAPACITY, and
    the view and what it points at are what they were."""
    t = torch
    n_act = 4
    eng = _engine(n_act)
    q = eng.waitq_create(100)
    try:
        rng = np.random.default_rng(100)
        s = np.zeros(n_act, Q.STATE_DTYPE)
        s["state"] = L.ACT_VALID
        w = Q.World(s)
        for step in range(2):
            act = rng.integers(0, n_act, 60).astype(np.uint32)
            disp = np.full(60, L.ADM_RUN, np.uint8)
            disp[rng.permutation(60)[:10]] = L.ADM_ENQUEUE
            tok = (1000 * (step + 1) + np.arange(60)).astype(np.uint32)
            fl = Q.request_flags(rng, 60)
            w = Q.append(w, act, tok, fl, disp)
            _append_raw(t, eng, q, n_act, act, tok, fl, disp)
            Snapshot(eng, eng.waitq_view(q), n_act).check_store(w, ("append", step))
        assert len(w.tok) == 20
        v = eng.waitq_view(q)
        act = rng.integers(0, n_act, 90).astype(np.uint32)
        with pytest.raises(OrleansRouteError) as e:
            _append_raw(t, eng, q, n_act, act, np.arange(90, dtype=np.uint32), Q.request_flags(rng, 90),
                        np.full(90, L.ADM_ENQUEUE, np.uint8))
        assert e.value.code == L.E_CAPACITY
        v2 = eng.waitq_view(q)
        assert [getattr(v, f) for f, _ in v._fields_] == [getattr(v2, f) for f, _ in v2._fields_]
        Snapshot(eng, v2, n_act).check_store(w, "after the refused append")
        # 80 more fit exactly
        act = rng.integers(0, n_act, 80).astype(np.uint32)
        tok, fl, disp = (5000 + np.arange(80)).astype(np.uint32), Q.request_flags(rng, 80), np.full(80, L.ADM_ENQUEUE, np.uint8)
        w = Q.append(w, act, tok, fl, disp)
        _append_raw(t, eng, q, n_act, act, tok, fl, disp)
        Snapshot(eng, eng.waitq_view(q), n_act).check_store(w, "full")
    finally:
        eng.waitq_destroy(q)
        eng.close()


def test_batches_over_max_batch_are_refused(torch):
    t = torch
    eng = _engine(16)
    q = eng.waitq_create(64)
    try:
        n = eng.query(L.Q_MAX_BATCH) + 1
        z = t.zeros(64, dtype=t.int32, device="cuda")
        for call in (lambda: eng.waitq_append_device(q, z, z, n, z, z, z), lambda: eng.complete_device(q, z, z, n, z, z, z)):
            with pytest.raises(OrleansRouteError) as e:
                call()
            assert e.value.code == L.E_CAPACITY
    finally:
        eng.waitq_destroy(q)
        eng.close()
