"""tests/stage4_ref.py against the two oracles and against the plan table of DESIGN §2: the numpy reference, the Python
restatement of the stage-4 plan functions, the batch builders and the coverage of the GPU width matrix (no GPU)."""
import numpy as np
import pytest

import stage4_ref as S
from oracle import cpu_ref, pyref as P

# DESIGN §2's table: w = bit_length(n_act) -> (hb, lb) on the two-level plan, the LSD digits (low first) above it
TWO_LEVEL = {12: (6, 6), 13: (7, 6), 14: (7, 7), 15: (8, 7), 16: (8, 8), 17: (9, 8), 18: (9, 9), 19: (10, 9),
             20: (10, 10), 21: (11, 10), 22: (11, 11)}
LSD = {23: (8, 8, 7), 24: (8, 8, 8), 25: (9, 8, 8), 26: (9, 9, 8), 27: (9, 9, 9), 28: (10, 9, 9), 29: (10, 10, 9),
       30: (10, 10, 10), 31: (11, 10, 10)}


def _expected_plan(w):
    if w <= 11:
        return (True, 0, w, ())
    if w <= 22:
        return (True,) + TWO_LEVEL[w] + ((),)
    return (False, 0, 0, LSD[w])


SMALL_N_ACT = [1, 2, 3, 7, 8, 255, 256, 4095, 4096]


@pytest.mark.parametrize("n_act", SMALL_N_ACT)
def test_bucket_ref_equals_both_oracles(n_act):
    o = cpu_ref.Oracle(8)
    batches = [S.build(b, n_act, n) for b in S.BUILDERS for n in (1, 7, 300)]
    batches.append(S.hot_mix(n_act, 300, 1, n_act, 40))
    batches.append(np.zeros(0, np.uint32))
    for a in batches:
        order, off = S.bucket_ref(a, n_act)
        assert order.dtype == np.uint32 and off.dtype == np.uint32 and len(off) == n_act + 2
        p_off, p_order = P.bucket_stable([int(x) for x in a], n_act)
        np.testing.assert_array_equal(order, np.array(p_order, np.uint32))
        np.testing.assert_array_equal(off, np.array(p_off, np.uint32))
        c_order, c_off = o.bucket(a, n_act)
        np.testing.assert_array_equal(order, c_order)
        np.testing.assert_array_equal(off, c_off)


def test_bucket_ref_sparse_form_equals_the_counts_prefix():
    """bucket_ref writes the offsets run by run (offsets_runs) when a batch has far fewer messages than buckets; the same
    batches padded past that threshold take the bincount + cumsum form, and the offsets must agree bucket for bucket."""
    n_act = 100_000
    for name, a in [(b, S.build(b, n_act, 4097)) for b in S.BUILDERS] + [("empty", np.zeros(0, np.uint32))]:
        _, sparse = S.bucket_ref(a, n_act)
        key = np.minimum(a, np.uint32(n_act))
        exp = np.zeros(n_act + 2, np.int64)
        exp[1:] = np.cumsum(np.bincount(key, minlength=n_act + 1))
        np.testing.assert_array_equal(sparse, exp.astype(np.uint32), err_msg=name)
        totals, runs = S.offsets_runs(a, n_act)
        assert totals.dtype == np.uint32 and (runs > 0).all() and (np.diff(totals.astype(np.int64)) > 0).all()
        assert runs.sum() == n_act + 2 and totals[0] == 0 and totals[-1] == len(a)
        np.testing.assert_array_equal(np.repeat(totals, runs), exp.astype(np.uint32), err_msg=name)
        pad = np.full(n_act, S.NO_ACT, np.uint32)  # dense form: the padding only raises offsets[n_act + 1]
        _, dense = S.bucket_ref(np.concatenate([a, pad]), n_act)
        np.testing.assert_array_equal(dense[:-1], sparse[:-1])
        assert dense[-1] == sparse[-1] + n_act


@pytest.mark.parametrize("w", range(1, 32))
def test_plan_of_reproduces_the_table(w):
    for n_act in {1 << (w - 1), (1 << w) - 1}:
        p = S.plan_of(n_act)
        assert p.w == w == S.bit_length(n_act)
        assert (p.two_level, p.hb, p.lb, p.lsd) == _expected_plan(w), (n_act, p)
        assert sum(p.lsd) == (0 if p.two_level else w) and p.hb + p.lb == (w if p.two_level else 0)
        assert all(b <= S.K_MAX_DIGIT_BITS for b in (p.hb, p.lb) + p.lsd)
        assert p.max_items == 16


def test_route_items_ranges_at_the_default_grid():
    """route_items halves the tile until the grid has 2048 workgroups: items stays at i from the first n that fills 2047
    tiles of 256 * i / 2 ... (the 8192-row cap only binds below items = 1)."""
    assert (S.K_ROUTE_THREADS, S.K_ROUTE_MIN_WG, S.K_MAX_ROUTE_ROWS, S.K_ITEMS) == (256, 2048, 8192, 16)
    r = S.route_item_ranges()
    assert r == {1: (1, 1_048_064), 2: (1_048_065, 2_096_128), 4: (2_096_129, 4_192_256), 8: (4_192_257, 8_384_512),
                 16: (8_384_513, None)}
    for items, (lo, hi) in r.items():
        assert S.route_items(lo) == items and (hi is None or S.route_items(hi) == items)
        if hi is not None:
            assert hi == (S.K_ROUTE_MIN_WG - 1) * S.K_ROUTE_THREADS * 2 * items
            assert _rows(hi, items) == 2 * (S.K_ROUTE_MIN_WG - 1) <= S.K_MAX_ROUTE_ROWS
    assert S.route_items(1 << 30) == 16
    # the small MSD tile: 8 items or fewer and at most 8M messages
    assert (S.K_MSD_SMALL_MAX, S.K_MSD_ITEMS, S.K_MSD_ITEMS_SMALL) == (8 << 20, 16, 8)
    assert S.msd_items(8_384_512, 8) == 8 and S.msd_items(8_384_513, 16) == 16 and S.msd_items((8 << 20) + 1, 8) == 16


def _rows(n, items):
    return -(-n // (S.K_ROUTE_THREADS * items))


def test_builders_stay_in_their_sets():
    for n_act in SMALL_N_ACT + [(1 << 22), (1 << 23) - 1, 1 << 26]:
        al = S.alias_handles(n_act)
        assert (al >= n_act).all() and S.NO_ACT in al and n_act in al and len(set(al.tolist())) == len(al)
        if n_act < (1 << 31):
            assert {0x80000000, 0xFFFFFFFE, 1 << S.bit_length(n_act)} <= set(al.tolist())
        ek = S.edge_keys(n_act)
        assert ek.min() == 0 and ek.max() == n_act and n_act - 1 in ek
        p = S.plan_of(n_act)
        for s in ([p.lb] if p.hb else []) + list(np.cumsum(p.lsd)[:-1]):
            assert (1 << int(s)) - 1 in ek and (1 << int(s)) in ek
        n = 5000
        a = S.aliases(n_act, n, 3, 0.3)
        assert a.dtype == np.uint32 and set(a[a >= n_act].tolist()) <= set(al.tolist())
        if n_act > 1:
            assert len(set(a[a >= n_act].tolist())) >= min(len(al), 3)  # mixed, not ORL_NO_ACT only
        u = S.uniform(n_act, n, 3)
        assert ((u < n_act) | (u == S.NO_ACT)).all() and 0.02 < (u == S.NO_ACT).mean() < 0.09
        e = S.edges(n_act, n, 3)
        assert set(np.minimum(e, n_act).tolist()) <= set(ek.tolist())
        f = S.far_keys(n_act, n, 3)
        assert (f < n_act).all()
        np.testing.assert_array_equal(S.uniform(n_act, n, 3), u)  # seeded
        h = S.hot_mix(n_act, n, 3, n_act, 1000)
        assert (h >= n_act).sum() >= 1000
        h = S.hot_mix(n_act, n, 3, n_act - 1, 1000)
        assert (h == n_act - 1).sum() >= 1000


def test_width_matrix_covers_every_plan():
    """Fails when someone trims the matrix of tests/test_gpu_stage4_widths.py: every (hb, lb) pair of w = 1..22 and every
    LSD digit triple of w = 23..27 at both edge values of n_act, every builder at every size of every case, out-of-range
    aliases among them."""
    cases = S.width_cases()
    assert [w for w, _ in cases] == [1] + [w for w in range(2, 28) for _ in range(2)]
    seen = {}
    for w, n_act in cases:
        assert n_act in (1 << (w - 1), (1 << w) - 1)
        p = S.plan_of(n_act)
        assert p.w == w
        seen.setdefault((p.two_level, p.hb, p.lb, p.lsd), set()).add(n_act)
        b = S.width_batches(n_act)
        assert set(b) >= {(name, n) for name in S.BUILDERS if not (p.two_level and name == "far") for n in S.SIZES}
        for name, n in b:  # orl_bucket_device: full rows, and these batches never take the dense LSD form
            assert S.row_step0(n_act, n, S.K_ITEMS) in (None, 1) and not S.lsd_gaps(n_act, n)
    assert set(S.SIZES) == {1, 255, 4096, 4097, 12289, 40_001}
    for w in range(1, 28):
        assert len(seen[_expected_plan(w)]) == (1 if w == 1 else 2), w
    assert len(seen) == 27


def test_dense_route_and_hot_cases_cover_what_they_claim():
    n_act, n = S.dense_case()
    assert S.plan_of(n_act).lsd == (8, 8, 7) and S.lsd_gaps(n_act, n) and not S.lsd_gaps(n_act, n - 1001)
    assert not S.lsd_gaps(1 << 24, 1 << 30)  # from 25 bits on the last shift exceeds 16: no dense form
    rc = S.route_cases()
    steps = {True: set(), False: set()}
    for w, n_act, items, n in rc:
        p = S.plan_of(n_act)
        assert p.w == w and S.route_items(n, p.max_items) == items
        if p.hb or not p.two_level:
            steps[p.two_level].add(S.row_step0(n_act, n))
        else:
            assert S.row_step0(n_act, n) is None
    assert steps[True] == {8, 4, 2, 1} and steps[False] == {16, 8, 4, 2, 1}
    kinds = {(S.plan_of(a).two_level, S.plan_of(a).hb > 0) for _, a, _, _ in rc}
    assert kinds == {(True, False), (True, True), (False, False)}
    assert {i for _, _, i, _ in rc} == {1, 2, 4, 8, 16} and len(rc) == 15
    assert {w for w, _, _, n in rc if S.plan_of((1 << w) - 1).two_level and S.msd_items(n, S.route_items(n)) == 8}
    assert 19 in S.ROUTE_WIDTHS  # a two-level width no other GPU test runs
    assert [w for w, _ in S.HOT_WIDTHS] == [12, 15, 17, 21, 22]
    for w, n_act in S.HOT_WIDTHS:
        p = S.plan_of(n_act)
        assert p.w == w and p.two_level and p.hb > 0
    assert S.HOT_N == (1 << 20) + 4097 and (S.K_HOT_SHARE, S.K_HOT_MIN_COUNT) == (32, 8192)
