"""orl_collector and the orl_collect_*_device calls on the GPU against the model (collector_ref's numpy form, which
tests/test_collector_ref.py holds to the literal reference).  After every call all five collector arrays, the whole state
table, the condemned list (after a scan), next_ticket and d_counts are compared exactly.  The scenarios are collector_ref's
builders; a start state is written through orl_collector_view_get's pointers, as a host would.

Tile = 2048 activations (256 threads x 8).
"""
import numpy as np
import pytest

import collector_ref as R
import completion_ref as Q
from orleans_amd import _lib as L
from orleans_amd import workloads as W
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


def _engine(n_act, max_batch=1 << 16):
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


def _bucket_arrays(t, n, n_act):
    return (t.full((max(n, 1),), -1, dtype=t.int32, device="cuda"), t.full((n_act + 2,), -1, dtype=t.int32, device="cuda"))


def _load(t, eng, col, c):
    """A Col into the collector, through the view."""
    v = eng.collector_view(col)
    assert (v.quantum, v.next_ticket) == (c.quantum, c.next_ticket)
    keep = [_dev(t, getattr(c, f)) for f in c.ARRAYS]
    t.cuda.synchronize()
    for d, p in zip(keep, (v.d_ticket, v.d_became_idle, v.d_keep_alive_until, v.d_age_limit, v.d_cflags)):
        eng.copy_on_device(p, d, d.numel())
    eng.sync()


def _check(eng, col, d_state, step, what, counts=None, n_act=None):
    v = eng.collector_view(col)
    n_act = len(step.state)
    for f, p in zip(R.Col.ARRAYS, (v.d_ticket, v.d_became_idle, v.d_keep_alive_until, v.d_age_limit, v.d_cflags)):
        exp = getattr(step.col, f)
        got = _host(eng, p, n_act, exp.dtype)
        bad = np.nonzero(got != exp)[0]
        assert len(bad) == 0, (what, f, len(bad), bad[:8], got[bad[:8]], exp[bad[:8]])
    assert v.next_ticket == step.col.next_ticket, (what, v.next_ticket, step.col.next_ticket)
    got = d_state.cpu().numpy().view(R.STATE_DTYPE)
    bad = np.nonzero(got != step.state)[0]
    assert len(bad) == 0, (what, "state", len(bad), bad[:4], got[bad[:4]], step.state[bad[:4]])
    if step.condemned is not None:
        n = int(_host(eng, v.d_out_n, 1, np.uint64)[0])
        assert n == len(step.condemned), (what, "condemned", n, len(step.condemned))
        got = _host(eng, v.d_out_act, n, np.uint32)
        bad = np.nonzero(got != step.condemned)[0]
        assert len(bad) == 0, (what, "condemned list", bad[:8], got[bad[:8]], step.condemned[bad[:8]])
    if counts is not None:
        got = counts.cpu().numpy().view(np.uint64)
        assert list(got) == list(step.counts), (what, "counts", list(got), list(step.counts))


def _run(t, sc, with_counts=True):
    """The scenario's calls one by one on the context's stream, everything compared after each."""
    steps = R.run_numpy(sc)
    eng = _engine(sc.n_act, sc.max_batch)
    col = eng.collector_create(sc.col.quantum, R.T0)
    try:
        _load(t, eng, col, sc.col)
        d_state = _dev(t, sc.state)
        for i, (op, step) in enumerate(zip(sc.ops, steps)):
            counts = t.full((8,), -1, dtype=t.int64, device="cuda") if with_counts else None
            kind = op[0]
            if kind in ("schedule", "cancel"):
                d_h = _dev(t, np.asarray(op[1], np.uint32))
                t.cuda.synchronize()
                if kind == "schedule":
                    eng.collect_schedule_device(col, d_h, len(op[1]), op[2], counts)
                else:
                    eng.collect_cancel_device(col, d_h, len(op[1]), counts)
            elif kind == "touch":
                _, act, fl, hard, hsw, now = op
                n = len(act)
                d_act, d_fl = _dev(t, act), _dev(t, fl)
                order, off = _bucket_arrays(t, n, sc.n_act)
                disp = t.full((max(n, 1),), 0xEE, dtype=t.uint8, device="cuda")
                t.cuda.synchronize()
                eng.bucket_device(d_act, n, order, off)
                eng.admit_device(d_act, d_fl, n, order, off, d_state, disp, hard, hsw)
                eng.collect_touch_device(col, d_act, disp, n, d_state, now, hard, hsw, counts)
                eng.sync()
                assert np.array_equal(disp.cpu().numpy()[:n], step.disp), (sc.name, i, "disp")
            elif kind == "on_complete":
                d_a, d_k = _dev(t, op[1]), _dev(t, op[2])
                t.cuda.synchronize()
                eng.collect_on_complete_device(col, d_a, d_k, len(op[1]), d_state, op[3], counts)
            elif kind == "scan_stale":
                t.cuda.synchronize()
                eng.collect_scan_stale_device(col, d_state, op[1], counts)
            else:
                t.cuda.synchronize()
                eng.collect_scan_all_device(col, d_state, op[1], op[2], counts)
            eng.sync()
            _check(eng, col, d_state, step, (sc.name, i, kind), counts)
    finally:
        eng.collector_destroy(col)
        eng.close()


@pytest.mark.parametrize("density", ["none", "all", "one-per-tile"])
@pytest.mark.parametrize("n_act", R.GPU_N_ACT)
def test_scan_density_vs_model(torch, n_act, density):
    """Schedule everything (a list with two handles >= n_act), ScanStale three quanta later (several quanta dequeued in one
    scan) condemning none / all / exactly one per tile, ScanStale again with nothing dequeued, ScanAll of the rest."""
    _run(torch, R.density_scenario(n_act, density))


@pytest.mark.parametrize("density", R.CHUNK_DENSITIES)
@pytest.mark.parametrize("n_act", R.CHUNK_N_ACT)
def test_chunked_tile_scan_vs_model(torch, n_act, density):
    """The same at 1024, 1025 and 2049 tiles, where the threads of the one-workgroup tile scan own chunks of 1, 2 and 3
    tile counts: one condemned activation per tile, and all of them."""
    _run(torch, R.density_scenario(n_act, density))


@pytest.mark.parametrize("build", [R.edge_scenario, R.matrix_scenario, R.quirk_scenario, R.branch_scenario, R.list_scenario],
                         ids=["tile-edges", "state-x-cflags", "scan-all-then-touch", "stale-branches", "lists"])
def test_scenario_vs_model(torch, build):
    """Condemned handles at 2047 / 2048 / 2049 / 4095 / 4096 and n_act - 1; every state x cflags combination on
    neighbouring handles; ScanAll's cancelled-in-place item touched, skipped and expired; one activation per ScanStale
    branch at the exact boundaries, then on-complete; schedule / cancel lists with handles >= n_act."""
    _run(torch, build())


@pytest.mark.parametrize("n", R.TOUCH_N)
def test_touch_vs_model(torch, n):
    """An admitted batch of n messages, touched twice at one `now` and once a quantum later, with the rule-1-only and
    rule-7-only activations for L = 1 and L = 2."""
    _run(torch, R.touch_scenario(n))


def test_counts_are_optional(torch):
    _run(torch, R.touch_scenario(4097), with_counts=False)
    _run(torch, R.branch_scenario(), with_counts=False)


def test_three_rounds_chained_on_one_stream_without_a_synchronise(torch):
    """bucket -> admit -> append -> touch -> on-complete -> bucket -> complete -> scan, three times, queued on the context's
    stream in one go; each round's results are kept by device-to-device copies on that stream and compared at the end."""
    t = torch
    w, c0 = R.chain_start()
    rounds, (hard, hsw), expect = R.chain_rounds()
    n_act = w.n_act
    eng = _engine(n_act)
    q = eng.waitq_create(len(w.tok) + sum(len(r[0]) for r in rounds))
    col = eng.collector_create(c0.quantum, R.T0)
    try:
        # the start store through the interface, as tests/test_gpu_completion.py loads it
        if len(w.tok):
            d_a, d_t, d_f = _dev(t, w.act), _dev(t, w.tok), _dev(t, w.mflags)
            disp = t.full((len(w.tok),), L.ADM_ENQUEUE, dtype=t.uint8, device="cuda")
            order, off = _bucket_arrays(t, len(w.tok), n_act)
            t.cuda.synchronize()
            eng.bucket_device(d_a, len(w.tok), order, off)
            eng.waitq_append_device(q, d_t, d_f, len(w.tok), order, off, disp)
            eng.sync()
        d_rt = _dev(t, w.running_tok)
        t.cuda.synchronize()
        eng.copy_on_device(eng.waitq_view(q).d_running_tok, d_rt, 4 * n_act)
        _load(t, eng, col, c0)
        d_state = _dev(t, w.state)
        v = eng.collector_view(col)
        ptrs = (v.d_ticket, v.d_became_idle, v.d_keep_alive_until, v.d_age_limit, v.d_cflags)
        bufs = []
        for act, fl, tok, cact, ctok, *_ in rounds:
            n, m = len(act), len(cact)
            b = dict(act=_dev(t, act), fl=_dev(t, fl), tok=_dev(t, tok), cact=_dev(t, cact), ctok=_dev(t, ctok),
                     disp=t.full((n,), 0xEE, dtype=t.uint8, device="cuda"),
                     counts=[t.full((8,), -1, dtype=t.int64, device="cuda") for _ in range(3)],
                     arrays=[t.zeros(n_act * (8 if f != "cflags" else 1), dtype=t.uint8, device="cuda") for f in R.Col.ARRAYS],
                     state=t.zeros_like(d_state), out=t.zeros(n_act, dtype=t.int32, device="cuda"),
                     out_n=t.zeros(1, dtype=t.int64, device="cuda"))
            b["order"], b["off"] = _bucket_arrays(t, n, n_act)
            b["corder"], b["coff"] = _bucket_arrays(t, m, n_act)
            bufs.append(b)
        t.cuda.synchronize()  # the uploads and fills are on torch's stream, the calls on the context's
        for b, (act, fl, tok, cact, ctok, t_touch, t_cmp, t_scan, kind) in zip(bufs, rounds):
            n, m = len(act), len(cact)
            eng.bucket_device(b["act"], n, b["order"], b["off"])
            eng.admit_device(b["act"], b["fl"], n, b["order"], b["off"], d_state, b["disp"], hard, hsw)
            eng.waitq_append_device(q, b["tok"], b["fl"], n, b["order"], b["off"], b["disp"])
            eng.collect_touch_device(col, b["act"], b["disp"], n, d_state, t_touch, hard, hsw, b["counts"][0])
            eng.collect_on_complete_device(col, b["cact"], b["ctok"], m, d_state, t_cmp, b["counts"][1])
            eng.bucket_device(b["cact"], m, b["corder"], b["coff"])
            eng.complete_device(q, b["cact"], b["ctok"], m, b["corder"], b["coff"], d_state)
            if kind == "scan_all":
                eng.collect_scan_all_device(col, d_state, R.QUANTUM, t_scan, b["counts"][2])
            else:
                eng.collect_scan_stale_device(col, d_state, t_scan, b["counts"][2])
            for dst, p in zip(b["arrays"], ptrs):
                eng.copy_on_device(dst, p, dst.numel())
            eng.copy_on_device(b["state"], d_state, d_state.numel())
            eng.copy_on_device(b["out"], v.d_out_act, 4 * n_act)
            eng.copy_on_device(b["out_n"], v.d_out_n, 8)
        eng.sync()
        t.cuda.synchronize()
        for step, (b, (disp, ecol, estate, condemned, c_touch, c_cmp, c_scan)) in enumerate(zip(bufs, expect)):
            assert np.array_equal(b["disp"].cpu().numpy(), disp), step
            for f, d in zip(R.Col.ARRAYS, b["arrays"]):
                exp = getattr(ecol, f)
                got = d.cpu().numpy().view(exp.dtype)
                assert np.array_equal(got, exp), (step, f, np.nonzero(got != exp)[0][:8])
            assert np.array_equal(b["state"].cpu().numpy().view(R.STATE_DTYPE), estate), (step, "state")
            n_out = int(b["out_n"].cpu().numpy()[0])
            assert n_out == len(condemned) and np.array_equal(b["out"].cpu().numpy().view(np.uint32)[:n_out], condemned), step
            for got, exp in zip(b["counts"], (c_touch, c_cmp, c_scan)):
                assert list(got.cpu().numpy().view(np.uint64)) == list(exp), (step, list(exp))
        assert eng.collector_view(col).next_ticket == expect[-1][1].next_ticket
    finally:
        eng.collector_destroy(col)
        eng.waitq_destroy(q)
        eng.close()


def test_create_has_finished_its_fills_before_the_first_call_on_the_stream(torch):
    """orl_collector_create and orl_waitq_create zero-fill (and 0xFF-fill running_tok) on the null stream; the context's
    stream does not wait for the null stream, so the create itself has to.  Eight times: create, write ticket[] /
    running_tok through the view on the context's stream at once, read back."""
    t = torch
    n_act = 1 << 20
    eng = _engine(n_act)
    try:
        src = t.arange(1, n_act + 1, dtype=t.int64, device="cuda")
        exp = src.cpu().numpy()
        t.cuda.synchronize()
        for _ in range(8):
            col = eng.collector_create(R.QUANTUM, R.T0)
            eng.copy_on_device(eng.collector_view(col).d_ticket, src, 8 * n_act)
            q = eng.waitq_create(1 << 20)
            eng.copy_on_device(eng.waitq_view(q).d_running_tok, src, 4 * n_act)
            eng.sync()
            got = _host(eng, eng.collector_view(col).d_ticket, n_act, np.int64)
            got_rt = _host(eng, eng.waitq_view(q).d_running_tok, n_act, np.uint32)
            eng.collector_destroy(col)
            eng.waitq_destroy(q)
            assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:8]
            assert np.array_equal(got_rt, exp.view(np.uint32)[:n_act]), np.nonzero(got_rt != exp.view(np.uint32)[:n_act])[0][:8]
    finally:
        eng.close()


def test_batches_over_max_batch_and_bad_times_are_refused(torch):
    t = torch
    eng = _engine(16)
    col = eng.collector_create(R.QUANTUM, R.T0)
    try:
        n = eng.query(L.Q_MAX_BATCH) + 1
        z = t.zeros(64, dtype=t.int32, device="cuda")
        for call in (lambda: eng.collect_schedule_device(col, z, n, R.T0), lambda: eng.collect_cancel_device(col, z, n),
                     lambda: eng.collect_touch_device(col, z, z, n, z, R.T0),
                     lambda: eng.collect_on_complete_device(col, z, z, n, z, R.T0)):
            with pytest.raises(OrleansRouteError) as e:
                call()
            assert e.value.code == L.E_CAPACITY
        for call in (lambda: eng.collect_schedule_device(col, z, 1, 0), lambda: eng.collect_scan_stale_device(col, z, 0),
                     lambda: eng.collect_scan_all_device(col, z, R.QUANTUM, -5), lambda: eng.collector_create(0, R.T0)):
            with pytest.raises(OrleansRouteError) as e:
                call()
            assert e.value.code == L.E_INVALID
        v = eng.collector_view(col)
        assert (v.quantum, v.next_ticket) == (R.QUANTUM, R.T0)
        assert not _host(eng, v.d_ticket, 16, np.int64).any() and not _host(eng, v.d_cflags, 16, np.uint8).any()
    finally:
        eng.collector_destroy(col)
        eng.close()
