"""Stage 5 (CSR fan-out) on the device at its own edges: zero-degree publishers, tile spans at and beyond the LDS limits
(the global-memory search), the publisher block map's serial / wave-written entries and its sentinel, the wave search
that replaces a clamped map, direct messages that end inside a tile, the degree scan's three launch regimes at their
boundaries, the self-summed columns' boundary, degenerate batches and back-to-back calls on one context.

The inputs and case lists are tests/fanout_ref.py's (tests/test_fanout_ref.py asserts, without a GPU, which regimes they
reach).  The expected outputs are not: cpu_ref.fanout_expand (with the key-table substitution), then the oracle's route
and bucket of concatenate([direct, expanded]), and the cumulative degrees + n_direct for pub_offsets.  Every comparison
is exact.  Outputs are pre-filled with a sentinel and the elements past n_out must keep it.

An understated ORL_OPT_TOTAL_GIVEN (include/orleans_route.h, stage 5): the first n messages of the batch, bucketed as a
batch of n; pub_offsets are those of the whole expansion; *n_out stays n.

No case passes an empty csr_tgt, a buffer shorter than the header asks for (orl_fanout_expand_device's d_out holds cap
records even where the call emits a quarter of that) or relies on CSR contents out of range; none is meant to make the
device fault.
"""
import numpy as np
import pytest

import fanout_ref as F
from oracle import cpu_ref
from orleans_amd import _lib as L
from orleans_amd import workloads as W
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError, grain_keys_from_guid_bytes, grain_keys_from_longs

pytestmark = pytest.mark.gpu

PAD = 64
SENT32 = np.uint32(0xA5A5A5A5)
SENT64 = np.uint64(0xA5A5A5A5A5A5A5A5)
PAST = np.uint32((L.ST_PAST_TOTAL << 16) | 0xFFFF)
N_REG, N_GONE = 1500, 500   # follower ids [0, N_REG) registered, the next N_GONE registered then removed, the rest never


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


class World:
    """What every case shares: the cluster, the follower graph (host and device), the follower keys, the direct messages,
    one oracle per n_act and the references computed so far (computed once, never changed)."""

    def __init__(self, t):
        self.t = t
        self.cl = W.default_cluster()
        self.tcd = W.grain_tcd(self.cl)
        self.off, self.tgt, _ = F.small_csr()
        ids = np.arange(F.N_FOLLOWERS, dtype=np.int64)
        self.long_keys = grain_keys_from_longs(self.cl.type_code, ids)
        # the key table: another long id for most followers, a Guid key nobody registers for every tenth
        fk = grain_keys_from_longs(self.cl.type_code, (ids * 7 + 3) % F.N_FOLLOWERS)
        gk = grain_keys_from_guid_bytes(self.cl.type_code, np.random.default_rng(9).integers(1, 256, (len(ids[::10]), 16),
                                                                                                dtype=np.int64).astype(np.uint8))
        fk[::10] = gk
        self.key_table = fk
        self.guid_grain = grain_keys_from_guid_bytes(self.cl.type_code, np.arange(100, 116, dtype=np.uint8).reshape(1, 16))
        self.owner = self.cl.owner_of(W.jenkins3_np(self.long_keys["tcd"], self.long_keys["n0"], self.long_keys["n1"]))
        rng = np.random.default_rng(21)
        d = np.zeros(1024, L.MSG_DTYPE)
        d["tcd"] = np.uint64(self.tcd)
        d["n1"] = rng.integers(0, F.N_FOLLOWERS, len(d))
        d["sending_silo"] = rng.integers(0, self.cl.n_silos, len(d))
        d["category"] = 2
        self.direct = d
        dv = "cuda"
        self.d_off = t.from_numpy(self.off.view(np.int64).copy()).to(dv)
        self.d_tgt = t.from_numpy(self.tgt.view(np.int32).copy()).to(dv)
        self.d_keys = t.from_numpy(self.key_table.view(np.uint8).reshape(-1, 24).copy()).to(dv)
        self.d_direct = t.from_numpy(d.view(np.int32).reshape(-1, 8).copy()).to(dv)
        self._oracles, self._expanded, self._routed, self._bucketed = {}, {}, {}, {}

    def acts(self, n_act):
        mult = 1 if n_act < 4096 else 257  # spread over the handle width; distinct (n_act is odd or 2^k > 257 * ids)
        a = (np.arange(N_REG + N_GONE, dtype=np.int64) * mult) % n_act
        assert len(set(a.tolist())) == len(a)
        return a.astype(np.uint32)

    def populate(self, register, unregister, n_act, guid=False):
        """The same registrations on an engine or an oracle: hits, removed keys and never-registered ids all occur."""
        k = self.long_keys[:N_REG + N_GONE]
        assert (register(k, self.acts(n_act), self.owner[:len(k)])[0] == L.INS_INSERTED).all()
        assert unregister(k[N_REG:]).all()
        if guid:
            g = self.guid_grain
            go = self.cl.owner_of(W.jenkins3_np(g["tcd"], g["n0"], g["n1"]))
            assert (register(g, np.array([n_act - 2], np.uint32), go)[0] == L.INS_INSERTED).all()

    def oracle(self, n_act):
        if n_act not in self._oracles:
            o = cpu_ref.Oracle(self.cl.n_silos, seed=0)
            for s in range(self.cl.n_silos):
                o.add_server(s, int(self.cl.hashes[s]))
            # (the Guid grain is nobody's follower: on a context it only selects the table form)
            self.populate(o.register, o.unregister, n_act, guid=True)
            self._oracles[n_act] = o
        return self._oracles[n_act]

    @staticmethod
    def pub_silo(n_pub):
        return ((np.arange(n_pub) * 5 + 1) % 8).astype(np.uint8)  # neighbours publish from different silos

    def expanded(self, call):
        """(records, pub_offsets relative to the fan-out) of the call's publishes: cpu_ref.fanout_expand, followers through
        the key table when the call names one."""
        key = (call.source, call.keyed)
        if key not in self._expanded:
            pubs = call.pubs
            exp, poff = cpu_ref.fanout_expand(self.off, self.tgt, pubs, self.pub_silo(len(pubs)), self.tcd)
            assert len(exp) == int(F.degrees_of(pubs).sum()) == int(poff[-1])
            if call.keyed:
                kk = self.key_table[exp["n1"].astype(np.int64)]
                exp["tcd"], exp["n0"], exp["n1"] = kk["tcd"], kk["n0"], kk["n1"]
            for a in (exp, poff):
                a.setflags(write=False)
            self._expanded[key] = (exp, poff)
        return self._expanded[key]

    def routed(self, call, n_act):
        """The oracle's (route, act) of concatenate([direct, expanded]), the whole batch whatever total the call gives."""
        key = (call.source, call.keyed, call.nd, n_act)
        if key not in self._routed:
            exp, _ = self.expanded(call)
            r, a = self.oracle(n_act).route(np.concatenate([self.direct[:call.nd], exp]))
            self._routed[key] = (r, a)
        return self._routed[key]

    def reference(self, call, n_act):
        """(route[n], act[n], order[n], offsets[n_act + 2]) for the n the call gives or gets: an overstated tail is
        ORL_ST_PAST_TOTAL / ORL_NO_ACT in the unresolved bucket; an understated total is the batch's first n messages."""
        key = (call.source, call.keyed, call.nd, n_act, call.total)
        if key not in self._bucketed:
            r, a = self.routed(call, n_act)
            real, n = F.n_of(call)
            assert real == len(r)
            if n > real:
                r = np.concatenate([r, np.full(n - real, PAST, np.uint32)])
                a = np.concatenate([a, np.full(n - real, L.NO_ACT, np.uint32)])
            r, a = r[:n], a[:n]
            od, of = self.oracle(n_act).bucket(a, n_act)
            self._bucketed[key] = (r, a, od, of)
        return self._bucketed[key]


@pytest.fixture(scope="module")
def world(torch):
    return World(torch)


def _engine(world, form, monkeypatch):
    """A context of the form: the knobs are read at orl_ctx_create."""
    for k, v in form.env:
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    eng = GrainDirectoryEngine(n_act=form.n_act, dir_capacity=4096, max_batch=form.max_batch, device=0)
    W.setup_engine(eng, world.cl)
    if form.n_act > N_REG + N_GONE:  # (the expand-only contexts route nothing: no directory)
        world.populate(eng.register_single_activation, eng.unregister, form.n_act, form.guid_grain)
    return eng


def _filled(t, n, dtype=None):
    dtype = dtype or t.int32
    v = int(SENT32.view(np.int32)) if dtype == t.int32 else int(SENT64.view(np.int64))
    return t.full((n,), v, dtype=dtype, device="cuda")


def _pub_args(world, call):
    t = world.t
    pubs = call.pubs
    if len(pubs) == 0:
        return None, None
    return (t.from_numpy(pubs.view(np.int32).copy()).cuda(), t.from_numpy(world.pub_silo(len(pubs))).cuda())


def _check_offsets(d_poff, poff_ref, nd, n_pub, label):
    got = d_poff.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got[:n_pub + 1], poff_ref + np.uint64(nd), err_msg=label + ": pub_offsets")
    assert (got[n_pub + 1:] == SENT64).all(), label + ": pub_offsets written past n_pub + 1"


def run_route(world, eng, form, call):
    """One call of a route entry point against its reference."""
    t = world.t
    label = f"{form.name}/{form.n_act}/{call.id}"
    real, n = F.n_of(call)
    n_pub = len(call.pubs)
    r_ref, a_ref, od_ref, of_ref = world.reference(call, form.n_act)
    _, poff_ref = world.expanded(call)
    d_pubs, d_ps = _pub_args(world, call)
    outs = [_filled(t, n + PAD) for _ in range(3)]
    of = _filled(t, form.n_act + 2 + PAD)
    poff = _filled(t, n_pub + 1 + PAD, t.int64)
    kw = dict(stream=t.cuda.current_stream().cuda_stream, total=None if call.total is None else n)
    if call.entry == "device":
        assert not call.keyed and call.nd == 0
        got = eng.fanout_device(world.d_off, world.d_tgt, d_pubs, d_ps, n_pub, world.tcd, poff, *outs, of, **kw)
    elif call.entry == "keys":
        assert call.keyed and call.nd == 0
        got = eng.fanout_keys_device(world.d_off, world.d_tgt, world.d_keys, d_pubs, d_ps, n_pub, poff, *outs, of, **kw)
    else:
        assert call.entry == "mixed" and call.nd > 0
        got = eng.fanout_mixed_device(world.d_direct, call.nd, world.d_off, world.d_tgt, world.d_keys if call.keyed else None,
                                      world.tcd, d_pubs, d_ps, n_pub, poff, *outs, of, **kw)
    t.cuda.synchronize()
    assert got == n, label
    _check_offsets(poff, poff_ref, call.nd, n_pub, label)
    for x, e, name in zip(outs, (r_ref, a_ref, od_ref), ("route", "act", "order")):
        g = x.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(g[:n], e, err_msg=f"{label}: {name}")
        assert (g[n:] == SENT32).all(), f"{label}: {name} written past n_out"
    g = of.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(g[:form.n_act + 2], of_ref, err_msg=label + ": offsets")
    assert (g[form.n_act + 2:] == SENT32).all(), label + ": offsets written past n_act + 2"
    if n > real:  # as test_fanout_overstated_total asserts
        assert (r_ref[real:] == PAST).all() and (a_ref[real:] == L.NO_ACT).all()
        assert of_ref[form.n_act + 1] - of_ref[form.n_act] >= n - real


def run_expand(world, eng, form, call):
    """One orl_fanout_expand_device call against cpu_ref.fanout_expand."""
    t = world.t
    label = f"{form.max_batch}/{call.id}"
    real, n = F.n_of(call)
    n_pub = len(call.pubs)
    exp, poff_ref = world.expanded(call)
    cap = call.cap or n + PAD
    assert cap >= n
    d_pubs, d_ps = _pub_args(world, call)
    d_out = _filled(t, (cap + PAD) * 8).view(-1, 8)  # the cap records the header asks for, whatever the call emits
    poff = _filled(t, n_pub + 1 + PAD, t.int64)
    got = eng.fanout_expand_device(world.d_off, world.d_tgt, world.d_keys if call.keyed else None, world.tcd, d_pubs, d_ps, n_pub,
                                   poff, d_out, cap, stream=t.cuda.current_stream().cuda_stream,
                                   total=None if call.total is None else n)
    t.cuda.synchronize()
    assert got == n, label
    _check_offsets(poff, poff_ref, 0, n_pub, label)
    out = d_out.cpu().numpy().view(L.MSG_DTYPE).reshape(-1)
    m = min(n, real)
    np.testing.assert_array_equal(out[:m], exp[:m], err_msg=label)
    tail = out[m:n]  # an overstated total: null, address-complete headers to nobody
    assert (tail["tcd"] == 0).all() and (tail["n0"] == 0).all() and (tail["n1"] == 0).all() and (tail["aux"] == 0).all(), label
    assert (tail["flags"] == L.HDR_ADDRESS_COMPLETE).all() and (tail["category"] == 0).all(), label
    assert (tail["target_silo"] == 0xFF).all() and (tail["sending_silo"] == 0xFF).all(), label
    assert (out[n:].view(np.uint32) == SENT32).all(), label + ": records written past n_out"


def _run_group(world, monkeypatch, form, calls):
    eng = _engine(world, form, monkeypatch)
    try:
        for c in calls:
            if c.entry == "expand":
                run_expand(world, eng, form, c)
            else:
                run_route(world, eng, form, c)
                assert eng.query(L.Q_PROBE_FORM) == form.probe_form, (form.name, c.id)
    finally:
        eng.close()


def _params(group):
    g = F.groups()[group]
    return pytest.mark.parametrize("form,calls", g, ids=[f"{f.name}-{f.n_act}-{f.max_batch}" for f, _ in g])


@_params("route")
def test_route_forms_every_family(world, monkeypatch, form, calls):
    """fanout_device, fanout_keys_device and fanout_mixed_device over every degree family, n_direct in {0, 1, 257, 700},
    the total read back, given exactly and overstated by 1, 255, 256 and 777, on the 8-B, the 16-B (ORL_FAN_U unset, 2, 4)
    and the 32-B table (whose kernel prefetches and stages 64 publishers fewer), on a one-level and a two-level stage 4."""
    assert {c.total for c in calls} == {None, 0, *F.OVERS} and {c.nd for c in calls} == set(F.ROUTE_ND)
    _run_group(world, monkeypatch, form, calls)


@_params("degenerate")
def test_degenerate_batches(world, monkeypatch, form, calls):
    """No publisher at all; every degree zero, without a direct message (returns 0, offsets all zero, nothing else
    written) and behind direct messages; totals of exactly 1."""
    totals = [F.n_of(c)[1] for c in calls]
    assert 0 in totals and 1 in totals and 700 in totals
    _run_group(world, monkeypatch, form, calls)


@_params("sequence")
def test_back_to_back_calls_on_one_context(world, monkeypatch, form, calls):
    """Giants, then zero runs with a smaller total, then giants again (and on): every call equals its own reference,
    whatever map entries and column sums the one before left."""
    _run_group(world, monkeypatch, form, calls)


@_params("col")
def test_tile_and_column_boundaries(world, monkeypatch, form, calls):
    """Fan-out totals of 64 | 65 tiles and 4096 | 4097 tiles (the self-summed columns' last chunk count and the first
    beyond it), and 2.1 M messages in tiles of 512 from thirty publishers of 70 000 among 100 000 of none."""
    _run_group(world, monkeypatch, form, calls)


@_params("understated")
def test_understated_total(world, monkeypatch, form, calls):
    """ORL_OPT_TOTAL_GIVEN below the emitted count, one case per entry point: the first n messages, bucketed as n; the
    publish offsets of the whole expansion; nothing past n."""
    assert all(c.total < 0 for c in calls)
    _run_group(world, monkeypatch, form, calls)


def test_total_below_n_direct_is_refused(world, monkeypatch):
    """ORL_OPT_TOTAL_GIVEN below n_direct is no understated total: ORL_E_INVALID before any device work, nothing
    written."""
    t = world.t
    form = F.FORM["8B"].at(F.ROUTE_N_ACT[0])
    call = F.Call("giants", "mixed", 257)
    eng = _engine(world, form, monkeypatch)
    d_pubs, d_ps = _pub_args(world, call)
    bufs = [_filled(t, 1024) for _ in range(3)] + [_filled(t, form.n_act + 2)]
    poff = _filled(t, len(call.pubs) + 1, t.int64)
    try:
        with pytest.raises(OrleansRouteError) as e:
            eng.fanout_mixed_device(world.d_direct, call.nd, world.d_off, world.d_tgt, None, world.tcd, d_pubs, d_ps,
                                    len(call.pubs), poff, *bufs, stream=t.cuda.current_stream().cuda_stream, total=call.nd - 1)
        assert e.value.code == L.E_INVALID
        t.cuda.synchronize()
        assert all((b.cpu().numpy().view(np.uint32) == SENT32).all() for b in bufs)
        assert (poff.cpu().numpy().view(np.uint64) == SENT64).all()
    finally:
        eng.close()


@_params("expand")
def test_expand_every_family(world, monkeypatch, form, calls):
    """orl_fanout_expand_device over every family, long-key and key-table followers, exact and overstated totals."""
    _run_group(world, monkeypatch, form, calls)


@_params("wave")
def test_expand_wave_search(world, monkeypatch, form, calls):
    """A cap beyond the context's max_batch clamps the block map: a total of 17 blocks still has it, one more message
    (or an overstated total) takes the two 64-way searches per tile instead."""
    _run_group(world, monkeypatch, form, calls)


@_params("scan")
def test_expand_scan_regimes(world, monkeypatch, form, calls):
    """n_pub + 1 on both sides of every launch regime of the degree scan (one chunk | more, 1024- | 4096-element chunks,
    in-kernel | launched chunk prefix), all degrees zero but a few at the chunk edges and the ends."""
    assert [len(c.pubs) + 1 for c in calls] == list(F.SCAN_M)
    _run_group(world, monkeypatch, form, calls)
