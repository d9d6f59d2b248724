"""tests/fanout_ref.py pinned on the CPU: its model of stage 5's publisher search against the brute-force publisher of
every message (np.repeat) and cpu_ref.fanout_expand, and what the case lists of tests/test_gpu_fanout_edges.py reach.

The coverage assertions are what keeps the GPU file honest: a constant that changes in route_kernels.hip (the LDS limit,
the serial / wave threshold of the block map, a scan chunk) moves the regimes the fixed case lists reach, and that must
fail here, without a GPU."""
import numpy as np
import pytest

import fanout_ref as F
import stage4_ref as S4
from oracle import cpu_ref

NDS = (0, 1, 255, 256, 257, 700)
TILES = (256, 512, 1024)


def test_constants_come_from_the_sources():
    assert F.FAN_BLK == 1 << F.FAN_BLK_SHIFT == S4.K_ROUTE_THREADS  # fan_range's tiles start on map blocks when nd = 0
    assert 0 < F.FAN_LDS_PF < F.FAN_LDS
    assert F.SCAN_SMALL_CHUNK < F.SCAN_CHUNK and F.FBLK_SERIAL < F.WAVE
    assert len(set(F.REGIMES)) == len(F.REGIMES)
    # the scan boundaries the GPU file runs are the launcher's own
    assert F.SCAN_M[2:] == (F.SCAN_SMALL_CHUNK, F.SCAN_SMALL_CHUNK + 1, F.SCAN_SMALL_CHUNK * F.SCAN_DIRECT_CHUNKS,
                            F.SCAN_SMALL_CHUNK * F.SCAN_DIRECT_CHUNKS + 1, F.SCAN_CHUNK * F.SCAN_DIRECT_CHUNKS,
                            F.SCAN_CHUNK * F.SCAN_DIRECT_CHUNKS + 1)


def test_csr_and_families_have_the_prescribed_shape():
    off, tgt, node_deg = F.small_csr()
    np.testing.assert_array_equal(np.diff(off.astype(np.int64)), node_deg)
    assert sorted(set(node_deg.tolist())) == sorted(F.DEGREES) and node_deg[0] == node_deg[-1] == 0
    assert len(tgt) == off[-1] > 0 and tgt.max() < F.N_FOLLOWERS
    for d in F.DEGREES:  # the copies of a degree name other followers (a wrong publisher shows)
        if d > 2:
            a, b = (tgt[int(off[F.node(d, c)]):int(off[F.node(d, c) + 1])] for c in (0, 1))
            assert not np.array_equal(a, b)
    deg = {k: F.degrees_of(F.family(k)) for k in F.FAMILIES}
    z = deg["zeros_edges"]
    assert z[0] == z[-1] == 0 and np.nonzero(z)[0][0] >= 256 and len(z) - np.nonzero(z)[0][-1] > 512
    assert (deg["ones"] == 1).all() and len(deg["ones"]) == 2049
    assert sorted(deg["giants"][deg["giants"] > 0].tolist()) == [2048, 2049, 16_641, 70_000]
    g = deg["giants"]
    assert all(g[i - 1] == 0 and g[i + 1] == 0 for i in np.nonzero(g)[0])
    for k, r in (("block_aligned", 0), ("block_aligned-1", F.FAN_BLK - 1), ("block_aligned+1", 1)):
        assert (deg[k][:-4] % F.FAN_BLK == 0).all() and deg[k].sum() % F.FAN_BLK == r
    d = F.family("duplicates")
    assert max(len(list(g)) for g in np.split(d, np.nonzero(np.diff(d))[0] + 1)) >= 600
    r = deg["random_mix"]
    assert (r == 0).mean() >= 0.30 and set(r.tolist()) >= {0, 1, 2, 255, 256, 257, 2048, 2049, 16_641}
    # zero_runs: sized so that tiles of one block with no direct message have exactly the spans named
    p = F.plan(deg["zero_runs"], 0, None, F.FAN_BLK, F.FAN_LDS, fcap=64)
    assert tuple(p.spans[:len(F.ZERO_RUN_SPANS)]) == F.ZERO_RUN_SPANS
    assert max(F.plan(deg["zero_runs"], 0, None, 512, F.FAN_LDS, fcap=64).spans) > 30_000


@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_model_is_the_brute_force_publisher(name):
    """Every family x nd x tile x both LDS limits, with and without the block map == np.repeat(arange(n_pub), deg), whose
    offsets and sending silos are cpu_ref.fanout_expand's."""
    pubs = F.family(name)
    deg = F.degrees_of(pubs)
    off, tgt, _ = F.small_csr()
    psilo = (np.arange(len(pubs)) % 251).astype(np.uint8)
    exp, poff = cpu_ref.fanout_expand(off, tgt, pubs, psilo, 7 << 8)
    brute = F.brute_pub_of(deg)
    np.testing.assert_array_equal(poff.astype(np.int64), F.offsets(deg))
    np.testing.assert_array_equal(exp["sending_silo"], psilo[brute])
    np.testing.assert_array_equal(exp["n1"], np.concatenate([tgt[int(off[p]):int(off[p + 1])] for p in pubs]))
    total = len(brute)
    for nd in NDS:
        for tile in TILES:
            for limit in (F.FAN_LDS_PF, F.FAN_LDS):
                for fcap in (0, (nd + total + 777) // F.FAN_BLK + 3):
                    for n in (None, nd + total + 777, nd + total - min(total, 300)):
                        p = F.plan(deg, nd, n, tile, limit, fcap)
                        assert p.used_map == bool(fcap)
                        np.testing.assert_array_equal(p.pub_of, F.brute_pub_of(deg, nd, n),
                                                      err_msg=str((nd, tile, limit, fcap, n)))


def test_wave_find_pub_and_block_map_on_random_degrees():
    rng = np.random.default_rng(3)
    for trial in range(60):
        n_pub = int(rng.integers(1, 5000))
        deg = rng.choice(np.array([0, 0, 0, 1, 2, 255, 256, 257, 3000]), n_pub)
        if trial % 5 == 0:
            deg[:] = 0
            deg[int(rng.integers(0, n_pub))] = 700
        poff = F.offsets(deg)
        total = int(poff[-1])
        if total == 0:
            continue
        vs = np.unique(np.concatenate([[0, total - 1], rng.integers(0, total, 40)]))
        want = np.searchsorted(poff[:n_pub], vs, side="right") - 1
        np.testing.assert_array_equal([F.wave_find_pub(poff, n_pub, int(v)) for v in vs], want)
        fcap = F._ceil_div(total, F.FAN_BLK) + 1 + trial % 3
        fblk, _ = F.block_map(poff, fcap)
        k = np.arange(F._ceil_div(total, F.FAN_BLK))
        np.testing.assert_array_equal(fblk[k], np.searchsorted(poff[:n_pub], k * F.FAN_BLK, side="right") - 1)
        assert fblk[len(k)] == n_pub - 1                # the sentinel: the block after the last one a message starts
        assert (fblk[len(k) + 1:] == -1).all()
        small, _ = F.block_map(poff, max(fcap - 3, 1))  # a clamped map: the same entries, never past its capacity
        np.testing.assert_array_equal(small[small >= 0], fblk[:len(small)][small >= 0])


def test_mutations_of_the_model_are_caught():
    """The upper block of fan_range without its + 1 must disagree with the brute force somewhere in the families (it
    must: a mutated GPU build would read the CSR out of range, so mutations live here only)."""
    bad = 0
    for name in F.FAMILIES:
        deg = F.degrees_of(F.family(name))
        total = int(deg.sum())
        try:
            p = F.plan(deg, 0, None, F.FAN_BLK, F.FAN_LDS, total // F.FAN_BLK + 3, upper_plus_one=False)
            bad += not np.array_equal(p.pub_of, F.brute_pub_of(deg))
        except AssertionError:
            bad += 1
    assert bad >= 5, bad


def _union(cases):
    seen, cache = set(), {}
    for c, f in cases:
        key = (c, f.limit, f.n_act, f.max_batch)
        if key not in cache:
            p = F.plan_of_call(c, f)
            real, n = F.n_of(c)
            np.testing.assert_array_equal(p.pub_of, F.brute_pub_of(F.degrees_of(c.pubs), c.nd, n), err_msg=c.id)
            cache[key] = p.regimes
        seen |= cache[key]
    return seen


def test_gpu_case_list_reaches_every_regime():
    groups = F.groups()
    flat = lambda g: [(c, f) for f, calls in groups[g] for c in calls]  # noqa: E731
    seen = {g: _union(flat(g)) for g in groups}
    everything = set().union(*seen.values())
    missing = [r for r in F.REGIMES if r not in everything]
    assert not missing, missing
    # and where each is expected: the route forms by their own LDS limit, the prefetch form included
    by_form = {}
    for f, calls in groups["route"]:
        by_form.setdefault(f.name, set()).update(_union([(c, f) for c in calls]))
    lo, lo1, hi, hi1 = F.SPAN_REGIMES
    for name, regs in by_form.items():
        want = {lo, lo1} if name == "32B" else {hi, hi1}
        assert want <= regs and not ({lo, lo1, hi, hi1} - want) & regs, name
        assert {"in_lds", "global_search", "fblk_serial", "fblk_serial:most", "fblk_wave", "fblk_wave:fewest",
                "fblk_wave_multi_round", "sentinel_on_block_boundary", "publisher_on_block_boundary", "first_tile_mid_nd",
                "zero_degree", "zero_degree_leading", "zero_degree_trailing"} <= regs, name
    assert {"self_cols"} <= by_form["8B"] and "no_self_cols" not in by_form["8B"]
    assert set(F.COL_REGIMES) <= seen["col"] and "global_search" in seen["col"]
    assert {"in_lds", "global_search", hi, hi1, "fblk_wave_multi_round", "sentinel_on_block_boundary"} <= seen["expand"]
    assert {"wave_search", "global_search", "in_lds", "fblk_serial"} <= seen["wave"]
    assert set(F.SCAN_REGIMES) | {"scan_sums", "scan_direct", "scan_small"} <= seen["scan"]
    with_map = [F.plan_of_call(c, F.WAVE_FORM).used_map for c in F.wave_calls()]
    assert with_map == [True, True, False, False, False, False]  # 17 blocks: the clamped map; overstated or + 1: searches


def test_gpu_cases_fit_their_contexts():
    one, two = (S4.plan_of(n) for n in F.ROUTE_N_ACT)
    assert one.two_level and one.hb == 0 and two.two_level and two.hb > 0 and S4.plan_of(F.COL_N_ACT).hb > 0
    for c, f in F.all_gpu_cases():
        real, n = F.n_of(c)
        mb = max(f.max_batch, F.TILE0)
        assert len(c.pubs) + 1 <= mb and c.nd <= n, c.id
        if c.entry == "expand":
            assert n <= (c.cap or n + 64)
        else:
            assert n <= mb, c.id
    items = {F.items_of(c, f) for f, calls in F.groups()["col"] for c in calls}
    assert items == {1, 2}  # the 2.1 M-message batch has tiles of 512
    assert len(F.many_zeros()) == 100_030 and int(F.degrees_of(F.many_zeros()).sum()) == 30 * 70_000
    for t in F.COL_TOTALS:
        assert int(F.degrees_of(F.exact_total(t)).sum()) == t
