"""orl_admit_device on the GPU against the sequential model (admission_ref.admit): order / offsets come from
orl_bucket_device (or the route) on the context's stream and admission follows on the same stream with no synchronise
between; d_disp, the whole state table and d_counts are compared exactly.  The scenarios are admission_ref's builders;
tests/test_admission_ref.py holds them to the model's coverage counters.

Tile = 2048 positions (256 threads x 8): the shapes and the boundary scenarios put bucket starts and ends on, before and
after tile and wave edges, the one-bucket batches carry one segment across up to 20 tiles, and L - c0 = 2047 / 2048 / 2049
puts the saturation point on either side of the first tile's edge.
"""
import numpy as np
import pytest

import admission_ref as A
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


def _engine(n_act, max_batch=MAX_BATCH, dir_capacity=16):
    eng = GrainDirectoryEngine(n_act=n_act, dir_capacity=dir_capacity, max_batch=max_batch, device=0)
    W.setup_engine(eng, W.default_cluster())
    return eng


def _dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _admit(t, eng, n_act, act, mflags, d_state, hard, hard_stateless, with_counts=True, bucket=True, d_act=None, order=None,
           off=None):
    """Bucket (unless the caller's route already did) and admit on the context's stream; -> (disp, counts) on the host."""
    n = len(act)
    if bucket:
        d_act = _dev(t, act)
        order = t.full((n,), -1, dtype=t.int32, device="cuda")
        off = t.full((n_act + 2,), -1, dtype=t.int32, device="cuda")
    d_fl = _dev(t, mflags)
    disp = t.full((n,), 0xEE, dtype=t.uint8, device="cuda")
    counts = t.full((8,), -1, dtype=t.int64, device="cuda") if with_counts else None
    t.cuda.synchronize()  # the uploads and fills are on torch's stream, the calls on the context's
    if bucket:
        eng.bucket_device(d_act, n, order, off)
    eng.admit_device(d_act, d_fl, n, order, off, d_state, disp, hard, hard_stateless, counts)
    t.cuda.synchronize()
    return disp.cpu().numpy(), (counts.cpu().numpy().view(np.uint64) if with_counts else None)


def _check(t, eng, sc, with_counts=True):
    e_disp, e_state, e_counts = sc.expect()
    d_state = _dev(t, sc.state)
    disp, counts = _admit(t, eng, sc.n_act, sc.act, sc.mflags, d_state, sc.hard, sc.hard_stateless, with_counts)
    bad = np.nonzero(disp != e_disp)[0]
    assert len(bad) == 0, (sc.name, len(bad), bad[:8], disp[bad[:8]], e_disp[bad[:8]], sc.act[bad[:8]], sc.mflags[bad[:8]])
    state = d_state.cpu().numpy().view(A.STATE_DTYPE)
    diff = np.nonzero(state != e_state)[0]
    assert len(diff) == 0, (sc.name, len(diff), diff[:4], state[diff[:4]], e_state[diff[:4]], sc.state[diff[:4]])
    if with_counts:
        assert list(counts) == list(e_counts), sc.name


@pytest.mark.parametrize("n_act", A.SHAPE_N_ACT)
def test_shapes_vs_model(torch, n_act):
    """n in {0, 1, 63, 64, 65, 257, 4097, 40 001} at this n_act: random handles with a hot one and 5 % unresolved, random
    flags and states, limits 6 / 3."""
    eng = _engine(n_act)
    try:
        for n in A.SHAPE_N:
            _check(torch, eng, A.shape_scenario(n, n_act))
    finally:
        eng.close()


@pytest.mark.parametrize("n", A.SHAPE_N)
def test_one_bucket_vs_model(torch, n):
    """The whole batch in one bucket: L in {0, 1, 2}; L - c0 at 2047, 2048, 2049 and n - 1; a stateless worker, an
    activating and an idle activation."""
    eng = _engine(3)
    try:
        for sc in A.one_bucket_scenarios(n):
            _check(torch, eng, sc)
    finally:
        eng.close()


@pytest.mark.parametrize("k", range(6, 14))
def test_bucket_boundaries_vs_model(torch, k):
    """A bucket whose start and whose length are each 2^k - 1, 2^k and 2^k + 1 (nine batches)."""
    eng = _engine(4)
    try:
        for ds in (-1, 0, 1):
            for dl in (-1, 0, 1):
                _check(torch, eng, A.boundary_scenario(k, ds, dl))
    finally:
        eng.close()


@pytest.mark.parametrize("n", A.CHUNK_N)
def test_chunked_tile_scan_vs_closed_form(torch, n):
    """1024, 1025 and 2049 tiles: the one-workgroup tile scan's threads own chunks of 1, 2 and 3 aggregates.  One bucket
    that saturates many chunks behind its head, and a bucket head every 3000 positions; against the numpy closed form
    (tests/test_admission_ref.py holds it to the model)."""
    t = torch
    for sc in A.chunk_scenarios(n):
        eng = _engine(sc.n_act, max_batch=n)
        try:
            e_disp, e_state, e_counts = A.admit_closed_form(sc.act, sc.mflags, sc.state, sc.n_act, sc.hard, sc.hard_stateless)
            d_state = _dev(t, sc.state)
            disp, counts = _admit(t, eng, sc.n_act, sc.act, sc.mflags, d_state, sc.hard, sc.hard_stateless)
            bad = np.nonzero(disp != e_disp)[0]
            assert len(bad) == 0, (sc.name, len(bad), bad[:8], disp[bad[:8]], e_disp[bad[:8]])
            state = d_state.cpu().numpy().view(A.STATE_DTYPE)
            diff = np.nonzero(state != e_state)[0]
            assert len(diff) == 0, (sc.name, len(diff), diff[:4], state[diff[:4]], e_state[diff[:4]])
            assert list(counts) == list(e_counts), sc.name
            if sc.n_act == 3:  # the saturation point lies behind the first chunk of every shape
                sat = int(np.nonzero(e_disp == L.ADM_OVERLOADED)[0][0])
                assert sat > 3 * 2048 and e_counts[L.ADM_RUN] > 0 and e_counts[L.ADM_ENQUEUE] > 0, (sc.name, sat)
        finally:
            eng.close()


@pytest.mark.parametrize("build", [A.late_first_request_scenario, A.state_matrix_scenario, A.alias_scenario],
                         ids=["late-first-request", "state-matrix", "aliases"])
def test_scenario_vs_model(torch, build):
    """A first request behind 9000 responses and expired messages; every state x flag combination on neighbouring
    handles; the unresolved bucket under its aliases."""
    sc = build()
    eng = _engine(sc.n_act)
    try:
        _check(torch, eng, sc)
    finally:
        eng.close()


def test_three_batches_chained_through_one_state_table(torch):
    """The state table stays on the device from batch to batch; between batches the host writes its completions into it
    (download, chain_complete, upload), as a silo's message pump would."""
    t = torch
    n_act, s, batches, (hard, hsw) = A.chain_batches()
    eng = _engine(n_act)
    try:
        d_state = _dev(t, s)
        for step, (act, fl) in enumerate(batches):
            e_disp, e_state, e_counts = A.admit(act, fl, s, n_act, hard, hsw)
            disp, counts = _admit(t, eng, n_act, act, fl, d_state, hard, hsw)
            assert np.array_equal(disp, e_disp), step
            state = d_state.cpu().numpy().view(A.STATE_DTYPE)
            assert np.array_equal(state, e_state), step
            assert list(counts) == list(e_counts), step
            s = A.chain_complete(state, step)
            d_state.copy_(_dev(t, s))
    finally:
        eng.close()


def test_counts_are_optional(torch):
    eng = _engine(5000)
    try:
        _check(torch, eng, A.shape_scenario(4097, 5000), with_counts=False)
    finally:
        eng.close()


def test_batch_over_max_batch_is_refused(torch):
    t = torch
    eng = _engine(16)
    try:
        n = eng.query(L.Q_MAX_BATCH) + 1
        z = t.zeros(64, dtype=t.int32, device="cuda")
        with pytest.raises(OrleansRouteError) as e:
            eng.admit_device(z, z, n, z, z, z, z)
        assert e.value.code == L.E_CAPACITY
    finally:
        eng.close()


def test_route_with_misses_then_admission(torch):
    """orl_route_batch_device over 20,000 grains of which 10 % were never registered: the unresolved bucket is the one
    k_route's handles make (ORL_NO_ACT), and admission runs behind the route on the same stream."""
    t = torch
    cl = W.default_cluster()
    n_grains, n_act, n = 20_000, 5000, 40_001
    eng = _engine(n_act, dir_capacity=n_grains)
    try:
        keys, _, owner, reg = W.grain_population(cl, n_grains, 0.9, 11)
        rng = np.random.default_rng(16)
        acts = rng.integers(0, n_act, n_grains).astype(np.uint32)
        idx = np.nonzero(reg)[0]
        eng.register_single_activation(keys[idx], acts[idx], owner[idx])
        msgs = W.uniform_messages(cl, n_grains, n, seed=16)
        fl = A.random_flags(rng, n)
        s = A.random_state(rng, n_act)
        d_in = t.from_numpy(msgs.view(np.int32).reshape(-1, 8)).cuda()
        route, d_act, order = (t.full((n,), -1, dtype=t.int32, device="cuda") for _ in range(3))
        off = t.full((n_act + 2,), -1, dtype=t.int32, device="cuda")
        d_state = _dev(t, s)
        t.cuda.synchronize()
        eng.address_messages_device(d_in, n, route, d_act, order, off)
        disp, counts = _admit(t, eng, n_act, np.zeros(n, np.uint32), fl, d_state, 6, 3, bucket=False, d_act=d_act,
                              order=order, off=off)
        act = d_act.cpu().numpy().view(np.uint32)
        miss = int((act >= n_act).sum())
        assert 0.05 * n < miss < 0.15 * n and (act[act >= n_act] == A.NO_ACT).all()
        e_disp, e_state, e_counts = A.admit(act, fl, s, n_act, 6, 3)
        assert np.array_equal(disp, e_disp)
        assert np.array_equal(d_state.cpu().numpy().view(A.STATE_DTYPE), e_state)
        assert list(counts) == list(e_counts) and int(counts[L.ADM_UNRESOLVED]) == miss
    finally:
        eng.close()
