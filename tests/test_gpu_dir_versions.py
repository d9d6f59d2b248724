"""Version tags of the directory partition and LookUpMany on the device (orleans_amd/csrc/dir_versions.hip, the tag stores of
the registration and merge kernels, the uploads, slot patches and mirror downloads that carry the tags).  Partitions of 64
and 4096 slots hold the key families of tests/dir_layout.py, so the read-only walk wraps, crosses tombstones and ends on
ghosts and N1 + 2^32 aliases.  The reference is tests/versioned_partition_ref.py (pyref.Partition plus GrainInfo.VersionTag
and RemoteGrainDirectory.LookUpMany); every comparison is exact."""
import numpy as np
import pytest

import adaptive_cache_ref as A
import dir_layout as D
import versioned_partition_ref as V
from oracle import cpu_ref, pyref as P
from orleans_amd import _lib as L
from orleans_amd import workloads as W
from orleans_amd.engine import GrainDirectoryEngine, grain_keys_from_longs

pytestmark = pytest.mark.gpu

N_SILOS = 8
N_ACT = 1 << 14
MAX_BATCH = 1 << 13
LOCAL = [1, 1, 1, 1, 0, 1, 1, 1]       # silo 4's partition is not held here: REMOTE_OWNER
FUNCTIONAL = [1, 1, 1, 0, 1, 1, 1, 1]  # silo 3 is no valid host: INVALID_SILO
CASES = [(64, "tail(4)"), (64, "one_slot(63)"), (64, "line_edge(32)"), (4096, "tail(4)"), (4096, "random")]
IDS = [f"{s}-{n}" for s, n in CASES]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def cluster():
    return W.default_cluster(N_SILOS)


def _fits(slots, count, tombs, n):
    """The device registration's documented rule (every message might insert)."""
    return (count + n) * 2 <= slots and (count + tombs + n) * 8 <= slots * 7


class Pair:
    """One device context and the model, fed the same calls; every call's outputs are compared."""

    def __init__(self, t, cluster, slots, local=LOCAL, functional=None, versions=True, n_silos=N_SILOS, hashes=None):
        self.t, self.slots, self.n_silos = t, slots, n_silos
        hashes = cluster.hashes if hashes is None else hashes
        self.eng = GrainDirectoryEngine(n_act=N_ACT, dir_capacity=slots // 2, max_batch=MAX_BATCH, device=0)
        self.model = V.Model(n_silos, hashes, N_ACT, local=local)
        self.local = local
        self.set_functional(functional or [1] * n_silos)
        for s in range(len(hashes)):
            self.eng.add_server(s, int(hashes[s]))
        if versions:
            self.eng.enable_directory_versions()
        self.st = t.cuda.current_stream().cuda_stream
        self.tombs_hi = 0  # removals since the last compaction: an upper bound of the tombstones

    def set_functional(self, functional):
        self.eng.set_silos(self.n_silos, functional=functional, local=self.local, seed=0)
        self.model.view.functional[:] = [bool(x) for x in functional]

    def dev(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    def out(self, n, dtype):
        return self.t.zeros(max(n, 1) * np.dtype(dtype).itemsize, dtype=self.t.uint8, device="cuda")

    def host(self, d, n, dtype):
        return d.cpu().numpy().view(dtype)[:n]

    def count(self):
        return len(self.model.part.data)

    def register(self, keys, acts, silos, tags, versioned=True):
        """One device registration batch; tags None with versioned=False is the unversioned call."""
        n = len(keys)
        assert _fits(self.slots, self.count(), self.tombs_hi, n), "the test sized a batch the rule refuses"
        d_st, d_wa, d_ws, d_wt = self.out(n, np.uint8), self.out(n, np.uint32), self.out(n, np.uint8), self.out(n, np.int32)
        if versioned:
            self.eng.register_single_activation_versioned_device(self.dev(keys), self.dev(acts), self.dev(silos),
                                                                 self.dev(np.asarray(tags, np.int32)), n, d_st, d_wa, d_ws, d_wt,
                                                                 stream=self.st)
        else:
            self.eng.register_single_activation_device(self.dev(keys), self.dev(acts), self.dev(silos), n, d_st, d_wa, d_ws,
                                                       stream=self.st)
        self.t.cuda.synchronize()
        st, wa, ws, wt = self.model.register(keys, acts, silos, tags if versioned else None)
        np.testing.assert_array_equal(self.host(d_st, n, np.uint8), st, err_msg="status")
        np.testing.assert_array_equal(self.host(d_wa, n, np.uint32), wa, err_msg="winner act")
        np.testing.assert_array_equal(self.host(d_ws, n, np.uint8), ws, err_msg="winner silo")
        if versioned:
            np.testing.assert_array_equal(self.host(d_wt, n, np.int32), wt, err_msg="winner tag")
        return st

    def register_chunked(self, keys, acts, silos, tags):
        """The messages in batches as large as the rule allows; stops when the table takes no more.  Returns the statuses
        of the messages sent."""
        at, sts = 0, []
        while at < len(keys):
            n = 0
            while at + n < len(keys) and _fits(self.slots, self.count(), self.tombs_hi, n + 1):
                n += 1
            if n == 0:
                break
            sts.append(self.register(keys[at:at + n], acts[at:at + n], silos[at:at + n], tags[at:at + n]))
            at += n
        return np.concatenate(sts)

    def unregister(self, keys):
        d_rm = self.out(len(keys), np.uint8)
        self.eng.unregister_device(self.dev(keys), len(keys), d_rm, stream=self.st)
        self.t.cuda.synchronize()
        rm = self.model.unregister(keys)
        np.testing.assert_array_equal(self.host(d_rm, len(keys), np.uint8), rm)
        self.tombs_hi += int(rm.sum())
        return rm

    def compact(self):
        self.eng.compact_directory()
        self.tombs_hi = 0

    def lookup(self, keys, etags, counts=True, host_too=False):
        """lookup_many_device against the model (and, with host_too, against lookup_many on the host mirror)."""
        n = len(keys)
        etags = np.asarray(etags, np.int32)
        d_k, d_e, d_a, d_s = self.out(n, np.uint8), self.out(n, np.int32), self.out(n, np.uint32), self.out(n, np.uint8)
        d_c = self.t.full((5,), 77, dtype=self.t.int64, device="cuda") if counts else None  # written, not accumulated
        self.eng.lookup_many_device(self.dev(keys) if n else None, self.dev(etags) if n else None, n, d_k, d_e, d_a, d_s, d_c,
                                    stream=self.st)
        self.t.cuda.synchronize()
        got = (self.host(d_k, n, np.uint8), self.host(d_e, n, np.int32), self.host(d_a, n, np.uint32), self.host(d_s, n, np.uint8))
        exp = self.model.lookup_many(keys, etags)
        for g, e, what in zip(got, exp, ("kind", "etag", "act", "silo")):
            np.testing.assert_array_equal(g, e, err_msg=what)
        if counts:
            np.testing.assert_array_equal(d_c.cpu().numpy(), np.bincount(exp[0], minlength=5))
        if host_too:
            for g, h in zip(got, self.eng.lookup_many(keys, etags)):
                np.testing.assert_array_equal(g, h)
        assert self.eng.directory_count() == self.count()
        return got

    def read_back(self, everything, host_too=False):
        """Every key with etag -1 (reads the tags back), then with the tags just read (UNCHANGED for the present ones)."""
        kind, etag, _, _ = self.lookup(everything, np.full(len(everything), -1, np.int32), host_too=host_too)
        kind2, _, _, _ = self.lookup(everything, etag)
        present = (kind == L.LUM_UPDATED) | (kind == L.LUM_UPDATED_EMPTY)
        assert (kind2[present] == L.LUM_UNCHANGED).all() and (kind2[~present] == kind[~present]).all()
        return kind, etag

    def close(self):
        self.eng.close()


def _keyext_key():
    kx = np.zeros(1, L.KEY_DTYPE)
    kx["tcd"], kx["n1"] = (L.CAT_KEYEXT_GRAIN << 56) + 7, 3
    return kx


def _everything(f):
    st = np.zeros(1, L.KEY_DTYPE)
    st["tcd"], st["n1"] = L.CAT_SYSTEM_TARGET << 56, 12
    return np.concatenate([f.keys, f.ghosts, f.aliases, _keyext_key(), st])


def _messages(f, rng, tag_base):
    """Every key of the family up to three times under distinct draws, shuffled; then a handle and a silo out of range and
    a negative draw.  (Silo 3 is not functional, silo 4's partition is remote: those statuses come from the random silos.)"""
    keys = np.concatenate([f.keys, f.keys[::2], f.keys[::4]])
    keys = keys[rng.permutation(len(keys))]
    n = len(keys)
    acts = rng.integers(0, N_ACT, n).astype(np.uint32)
    silos = rng.integers(0, N_SILOS, n).astype(np.uint8)
    tags = (tag_base + rng.permutation(n)).astype(np.int32)
    acts[3], silos[7], tags[11] = N_ACT + 5, 200, -5
    tags[13] = -(1 << 31)
    return keys, acts, silos, tags


@pytest.mark.parametrize("slots,name", CASES, ids=IDS)
def test_device_registration(torch, cluster, slots, name):
    """1.  Versioned registration on the device: statuses, winners and winner tags equal the model message by message;
    then removals, and re-registration into the tombstones under new draws.  After every phase every key, ghost and alias
    is looked up with etag -1."""
    f = D.family(name, slots, W.grain_tcd(cluster))
    f.check()
    p = Pair(torch, cluster, slots, functional=FUNCTIONAL)
    rng = np.random.default_rng(slots + len(name))
    everything = _everything(f)
    st = p.register_chunked(*_messages(f, rng, 1000))
    assert set(st.tolist()) == {L.INS_INSERTED, L.INS_EXISTING, L.INS_INVALID_SILO, L.INS_REMOTE_OWNER, L.INS_UNSUPPORTED}
    assert p.count() * 8 >= slots * 3  # a crowded table: at least 3/4 of the full load despite the refused silos
    kind, _ = p.read_back(everything, host_too=True)
    assert set(kind.tolist()) == {L.LUM_UPDATED, L.LUM_ABSENT, L.LUM_UNSUPPORTED}
    p.unregister(np.concatenate([f.keys[::2], f.ghosts[:4], f.keys[:2]]))  # a key twice: the first removal removes it
    p.read_back(everything)
    back = f.keys[::2][::3]
    nb = len(back)
    st = p.register_chunked(np.concatenate([back, back]), rng.integers(0, N_ACT, 2 * nb).astype(np.uint32),
                            rng.integers(0, N_SILOS, 2 * nb).astype(np.uint8), (np.arange(2 * nb) + (1 << 24)).astype(np.int32))
    assert (st == L.INS_INSERTED).sum() >= 1 and (st == L.INS_EXISTING).sum() >= 1
    p.read_back(everything, host_too=True)
    p.close()


@pytest.mark.parametrize("slots,name", [(64, "tail(4)"), (4096, "one_slot(4095)")])
def test_lookup_kinds_and_counts(torch, cluster, slots, name):
    """2.  Request batches of 0, 1, 63, 64, 65 and 257 (the wave edges of the count ballots); from 63 on every batch holds
    all five kinds and repeated keys.  The table is registered from the host (a full upload of slots and tags), every other
    key removed, then the hosting silo of some entries loses its functional bit: UPDATED_EMPTY."""
    f = D.family(name, slots, W.grain_tcd(cluster))
    p = Pair(torch, cluster, slots)
    rng = np.random.default_rng(slots)
    m = len(f.keys)
    silos = rng.integers(0, N_SILOS, m).astype(np.uint8)
    got = p.eng.register_single_activation_versioned(f.keys, np.arange(m, dtype=np.uint32), silos, np.arange(m, dtype=np.int32) + 5)
    exp = p.model.register(f.keys, np.arange(m), silos, np.arange(m) + 5, device=False)
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)
    p.unregister(f.keys[::2])
    live = np.array([k for k in f.keys[1::2] if p.model.part.get_grain_etag(V.Model.key(k)) >= 0], L.KEY_DTYPE)
    dead = int(p.model.part.data[p.model.part._k(V.Model.key(live[0]))][1])
    fn = [int(s != dead) for s in range(N_SILOS)]
    p.set_functional(fn)
    tag_of = lambda k: p.model.part.get_grain_etag(V.Model.key(k))  # noqa: E731
    on_dead = np.array([p.model.part.data[p.model.part._k(V.Model.key(k))][1] == dead for k in live])
    pools = {L.LUM_UNCHANGED: [(k, tag_of(k)) for k in live],
             L.LUM_ABSENT: [(k, 9) for k in np.concatenate([f.keys[::2], f.ghosts, f.aliases])],
             L.LUM_UPDATED: [(k, e) for k in live[~on_dead] for e in (-1, tag_of(k) + 1)],
             L.LUM_UPDATED_EMPTY: [(k, -1) for k in live[on_dead]],
             L.LUM_UNSUPPORTED: [(_keyext_key()[0], 0)]}
    assert all(len(v) for v in pools.values())
    for n in (0, 1, 63, 64, 65, 257):
        kinds = rng.integers(0, 5, n)
        kinds[rng.permutation(n)[:5]] = np.arange(5)[: min(n, 5)]
        reqs = [pools[int(q)][int(rng.integers(0, len(pools[int(q)])))] for q in kinds]
        keys = np.array([r[0] for r in reqs], L.KEY_DTYPE) if n else np.zeros(0, L.KEY_DTYPE)
        etags = np.array([r[1] for r in reqs], np.int32)
        kind, _, _, _ = p.lookup(keys, etags, counts=n != 65, host_too=True)
        np.testing.assert_array_equal(kind, kinds.astype(np.uint8))
        if n >= 63:
            assert set(kind.tolist()) == set(range(5)) and len(np.unique(keys)) < n
    p.close()


@pytest.mark.parametrize("slots", [64, 4096])
def test_state_carried(torch, cluster, slots):
    """3.  The tags through everything that moves or rewrites slots: enabling with entries present (tag 0), an unversioned
    device registration on the versioned partition (tag 0), a host call after device mutations (mirror download), a device
    call after host mutations (slot patches), the compaction, and a split with removal followed by re-registration."""
    t = torch
    f = D.family("tail(4)", slots, W.grain_tcd(cluster))
    m = len(f.keys)
    kh = np.sort(W.jenkins3_np(f.keys["tcd"], f.keys["n0"], f.keys["n1"]).view(np.int32))
    h0, h1 = int(cluster.hashes[0]), int(kh[m // 2])
    assert h0 != h1
    p = Pair(t, cluster, slots, local=[1, 0], versions=False, n_silos=2, hashes=[h0])  # the ring holds silo 0 alone
    rng = np.random.default_rng(slots + 3)
    everything = _everything(f)
    q = m // 4
    z = np.zeros(m, np.uint8)
    acts = np.arange(m, dtype=np.uint32) + 10
    p.register(f.keys[:q], acts[:q], z[:q], None, versioned=False)  # on the device, before the tags exist
    p.eng.enable_directory_versions()
    _, etag = p.read_back(everything[:q])
    assert (etag == 0).all()
    p.register(f.keys[q:2 * q], acts[q:2 * q], z[:q], np.arange(q) + 100)              # device, versioned
    p.register(f.keys[2 * q:3 * q], acts[2 * q:3 * q], z[:q], None, versioned=False)   # device, unversioned: tag 0
    p.read_back(everything, host_too=True)                                             # the host reads both arrays back
    tags = (np.arange(m - 3 * q) + 500).astype(np.int32)                               # host mutations after device ones
    got = p.eng.register_single_activation_versioned(f.keys[3 * q:], acts[3 * q:], z[3 * q:], tags)
    for g, e in zip(got, p.model.register(f.keys[3 * q:], acts[3 * q:], z[3 * q:], tags, device=False)):
        np.testing.assert_array_equal(g, e)
    assert p.count() == m
    rm = p.eng.unregister(f.keys[1::4])
    np.testing.assert_array_equal(rm, p.model.unregister(f.keys[1::4]))
    p.tombs_hi += int(rm.sum())
    _, etag = p.read_back(everything, host_too=True)                                   # the device sees the slot patches
    assert {0, 100, 500} <= set(etag.tolist())
    p.compact()
    p.read_back(everything, host_too=True)
    # silo 1 joins: the entries it now owns leave with ORL_SPLIT_REMOVE (their tags die), the rest keep theirs
    p.eng.add_server(1, h1)
    p.model.ring.add_server(1, h1)
    d_k, d_a, d_s = p.out(m * 24, np.uint8), p.out(m, np.uint32), p.out(m, np.uint8)
    d_n = t.zeros(1, dtype=t.int64, device="cuda")
    p.eng.split_directory_device(0, d_k, d_a, d_s, m, d_n, remove=True, stream=p.st)
    t.cuda.synchronize()
    moved = [k for k in f.keys if p.model.part.get_grain_etag(V.Model.key(k)) >= 0 and
             P.calculate_target_silo(p.model.ring, V.Model.key(k), P.uniform_hash(V.Model.key(k)), 0, p.model.view, True)[0] == 1]
    assert 0 < len(moved) < p.count() and int(d_n.item()) == len(moved)
    p.tombs_hi += len(p.model.unregister(moved))
    p.read_back(everything, host_too=True)
    # the receiver's side is another context; here silo 1's partition becomes local and the grains come back under new draws
    p.local = [1, 1]
    p.model.view.local[:] = [True, True]
    p.set_functional([1, 1])
    back = np.array(moved, L.KEY_DTYPE)
    st = p.register_chunked(back, rng.integers(0, N_ACT, len(back)).astype(np.uint32), np.zeros(len(back), np.uint8),
                            (np.arange(len(back)) + 9000).astype(np.int32))
    assert (st == L.INS_INSERTED).all()
    _, etag = p.read_back(everything, host_too=True)
    assert (etag >= 9000).sum() == len(st)
    p.close()


@pytest.mark.parametrize("slots", [64, 4096])
def test_merge(torch, cluster, slots):
    """4.  orl_dir_merge_versioned_device: every status occurs; INSERTED stores the incoming tag, KEPT and REPLACED the
    draw, the others leave the tag alone.  Statuses, dropped activations and all tags afterwards equal the model."""
    t = torch
    f = D.family("tail(4)", slots, W.grain_tcd(cluster))
    p = Pair(t, cluster, slots, local=None)
    rng = np.random.default_rng(slots + 4)
    ak = np.zeros(N_ACT, L.KEY_DTYPE)
    ak["n1"] = np.arange(N_ACT, dtype=np.uint64)  # ActivationIds ordered like their handles; SAME needs the same handle
    akey = lambda a: (int(ak["tcd"][a]), int(ak["n0"][a]), int(ak["n1"][a]))  # noqa: E731
    d_ak = p.dev(ak)
    m = len(f.keys)
    pre = f.keys[: m // 4]
    pre_a = rng.integers(100, N_ACT - 100, len(pre)).astype(np.uint32)
    st = p.register(pre, pre_a, rng.integers(0, N_SILOS, len(pre)).astype(np.uint8), np.arange(len(pre)) + 50)
    assert (st == L.INS_INSERTED).all()
    p.unregister(pre[::4])
    live = np.setdiff1d(np.arange(len(pre)), np.arange(len(pre))[::4])
    fresh = f.keys[len(pre): len(pre) + m // 8]
    # absent grains, the present ones, two removed ones (into the tombstones), two repeated keys: shuffled; then one entry
    # each with a handle and a silo out of range, a negative tag, a negative draw, and a KeyExt key
    keys = np.concatenate([fresh, pre[live], pre[::4][:2], fresh[:2]])
    acts = rng.integers(100, N_ACT - 100, len(keys)).astype(np.uint32)
    acts[len(fresh): len(fresh) + 3] = pre_a[live[:3]] + np.array([0, -1, 1])  # SAME, REPLACED (smaller), KEPT (larger)
    order = rng.permutation(len(keys))
    keys, acts = np.concatenate([keys[order], f.ghosts[:4], _keyext_key()]), np.concatenate([acts[order], np.full(5, 7, np.uint32)])
    n = len(keys)
    silos = rng.integers(0, N_SILOS, n).astype(np.uint8)
    tags, draws = (np.arange(n) + 7000).astype(np.int32), (np.arange(n) + 80000).astype(np.int32)
    acts[n - 5], silos[n - 4], tags[n - 3], draws[n - 2] = N_ACT, 99, -1, -7
    assert _fits(slots, p.count(), p.tombs_hi, n)
    d_st, d_da, d_ds = p.out(n, np.uint8), p.out(n, np.uint32), p.out(n, np.uint8)
    p.eng.merge_directory_versioned_device(p.dev(keys), p.dev(acts), p.dev(silos), p.dev(tags), p.dev(draws), n, d_ak, N_ACT,
                                           d_st, d_da, d_ds, stream=p.st)
    t.cuda.synchronize()
    st, da, ds = p.model.merge(keys, acts, silos, tags, draws, akey, N_ACT)
    np.testing.assert_array_equal(p.host(d_st, n, np.uint8), st)
    np.testing.assert_array_equal(p.host(d_da, n, np.uint32), da)
    np.testing.assert_array_equal(p.host(d_ds, n, np.uint8), ds)
    assert set(st.tolist()) == set(range(6))
    _, etag = p.read_back(_everything(f), host_too=True)
    assert (etag >= 80000).sum() == ((st == L.MERGE_KEPT) | (st == L.MERGE_REPLACED)).sum() >= 2
    assert ((etag >= 7000) & (etag < 80000)).sum() == (st == L.MERGE_INSERTED).sum()
    # the unversioned merge on the versioned partition: tags and draws of 0
    more = f.keys[len(pre) + m // 4:][:6]
    k2 = np.concatenate([more, pre[live][:3]])
    a2 = rng.integers(0, N_ACT, len(k2)).astype(np.uint32)
    s2 = np.zeros(len(k2), np.uint8)
    d_st = p.out(len(k2), np.uint8)
    p.eng.merge_directory_device(p.dev(k2), p.dev(a2), p.dev(s2), len(k2), d_ak, N_ACT, d_st, stream=p.st)
    t.cuda.synchronize()
    st2, _, _ = p.model.merge(k2, a2, s2, np.zeros(len(k2), np.int32), np.zeros(len(k2), np.int32), akey, N_ACT)
    np.testing.assert_array_equal(p.host(d_st, len(k2), np.uint8), st2)
    p.read_back(_everything(f))
    p.close()


T0 = 638_000_000_000_000_000
INITIAL, MAX_TTL, GROWTH = 10_000_001, 60_000_000, 1.5


def test_refresh_loop_end_to_end(torch, cluster):
    """5.  Two contexts on one GPU: A is silo 0 with an adaptive cache, B holds silo 1's versioned partition.  A's sweep
    lists go to B's lookup_many_device as the device pointers they are; the response is applied to A in runs of one kind
    (UPDATED_EMPTY as a removal: the device cache holds no empty lists).  A's count and a peek of every grain then equal
    adaptive_cache_ref.process_cache_refresh_response fed the model partition's answers."""
    t = torch
    st_ = t.cuda.current_stream().cuda_stream
    keys_all = grain_keys_from_longs(cluster.type_code, np.arange(6000, dtype=np.int64))
    owner = cluster.owner_of(W.jenkins3_np(keys_all["tcd"], keys_all["n0"], keys_all["n1"]))
    keys = keys_all[owner == 1][:260]
    n = len(keys)
    assert n == 260
    kt = [(int(a), int(b), int(c)) for a, b, c in zip(keys["tcd"], keys["n0"], keys["n1"])]
    rng = np.random.default_rng(5)
    b = Pair(t, cluster, 1024, local=[0, 1, 0, 0, 0, 0, 0, 0])
    acts = rng.integers(0, N_ACT, n).astype(np.uint32)
    silos = rng.integers(0, N_SILOS, n).astype(np.uint8)
    tags = rng.integers(0, 1 << 31, n).astype(np.int32)
    assert (b.register(keys, acts, silos, tags) == L.INS_INSERTED).all()
    a = GrainDirectoryEngine(n_act=N_ACT, dir_capacity=64, max_batch=MAX_BATCH, device=0)
    a.set_silos(N_SILOS, local=[1, 0, 0, 0, 0, 0, 0, 0], seed=0)
    for s in range(N_SILOS):
        a.add_server(s, int(cluster.hashes[s]))
    a.cache_config_adaptive(300, INITIAL, MAX_TTL, GROWTH)
    m = A.AdaptiveCache(300, INITIAL, MAX_TTL, GROWTH)
    # fill A from B's entries
    a.cache_add_or_update_versioned_device(b.dev(keys), b.dev(acts), b.dev(silos), b.dev(tags), n, T0, stream=st_)
    for k, ac, s, e in zip(kt, acts.tolist(), silos.tolist(), tags.tolist()):
        m.add_or_update(k, (ac, s), e, T0)
    # messages from silo 0 look 200 of the grains up: those are accessed, the sweep lists them
    msgs = D.messages(keys[rng.permutation(n)[:200]], 1)
    a.address_messages(msgs)
    for k in zip(msgs["tcd"].tolist(), msgs["n0"].tolist(), msgs["n1"].tolist()):
        assert m.look_up(k) is not None
    # B changes: grains re-registered under new tags, grains removed, a hosting silo not functional any more
    changed, removed = keys[:60], keys[60:100]
    b.unregister(np.concatenate([changed, removed]))
    b.register(changed, rng.integers(0, N_ACT, 60).astype(np.uint32), rng.integers(0, N_SILOS, 60).astype(np.uint8),
               rng.integers(0, 1 << 31, 60).astype(np.int32))
    fn = [1, 1, 1, 1, 0, 1, 1, 1]
    b.set_functional(fn)
    # the sweep at the expiry boundary, on the device and in the model (in the device's emitted order)
    now = T0 + INITIAL
    sw = a.cache_maintain_device(0, now, stream=st_)
    off = a._from_device(sw.d_owner_offsets, N_SILOS + 1, np.uint32).astype(np.int64)
    cnt = a._from_device(sw.d_counts, 5, np.uint64)
    n_req = int(off[2] - off[1])
    assert n_req == 200 == int(off[-1]) and int(cnt[2]) == 60 and int(cnt[3]) == 200  # owner 1 holds every list entry
    fetch, _ = A.maintainer_run(m, list(m.lru.d), lambda k: 1, lambda s: s == 0, now)
    req_k = a._from_device(sw.d_keys, n_req, L.KEY_DTYPE)
    req_e = a._from_device(sw.d_etags, n_req, np.int32)
    req_kt = [(int(x), int(y), int(z)) for x, y, z in zip(req_k["tcd"], req_k["n0"], req_k["n1"])]
    assert set(req_kt) == set(fetch[1])
    assert A.build_grain_and_etag_list(m, req_kt) == list(zip(req_kt, req_e.tolist()))
    # owner 1's list, as the device pointers the sweep returned, straight into B's lookup
    d_kind, d_etag, d_act, d_silo = b.out(n_req, np.uint8), b.out(n_req, np.int32), b.out(n_req, np.uint32), b.out(n_req, np.uint8)
    d_cnt = t.zeros(5, dtype=t.int64, device="cuda")
    b.eng.lookup_many_device(int(sw.d_keys) + int(off[1]) * 24, int(sw.d_etags) + int(off[1]) * 4, n_req, d_kind, d_etag, d_act,
                             d_silo, d_cnt, stream=st_)
    t.cuda.synchronize()
    kind, etag = b.host(d_kind, n_req, np.uint8), b.host(d_etag, n_req, np.int32)
    act, silo = b.host(d_act, n_req, np.uint32), b.host(d_silo, n_req, np.uint8)
    requests = [(P.Key(*k), int(e)) for k, e in zip(req_kt, req_e)]
    answers = V.look_up_many(b.model.part, requests, b.model.view)
    assert list(zip(kind.tolist(), etag.tolist(), act.tolist(), silo.tolist())) == answers
    assert set(kind.tolist()) == {L.LUM_UNCHANGED, L.LUM_ABSENT, L.LUM_UPDATED, L.LUM_UPDATED_EMPTY}
    np.testing.assert_array_equal(d_cnt.cpu().numpy(), np.bincount(kind, minlength=5))
    # the response composed from the device's answer, applied to A in runs of one kind
    resp = [((k.tcd, k.n0, k.n1), e, v) for k, e, v in V.response_of(requests, list(zip(kind.tolist(), etag.tolist(),
                                                                                        act.tolist(), silo.tolist())))]
    t1 = now + 7
    runs = A.response_runs(resp)
    assert {r[0] for r in runs} == {"add", "remove", "fresh"} and len(runs) > 10
    index = {k: i for i, k in enumerate(req_kt)}
    for run_kind, items in runs:
        idx = np.array([index[x[0]] for x in items], np.int64)
        rk = b.dev(req_k[idx])
        if run_kind == "add":
            a.cache_add_or_update_versioned_device(rk, b.dev(act[idx]), b.dev(silo[idx]), b.dev(etag[idx]), len(idx), t1, stream=st_)
        elif run_kind == "remove":
            a.cache_remove_device(rk, len(idx), b.out(len(idx), np.uint8), stream=st_)
        else:
            a.cache_mark_fresh_device(rk, len(idx), t1, stream=st_)
    t.cuda.synchronize()
    cnt_ref = A.process_cache_refresh_response(m, resp, t1)
    assert min(cnt_ref) > 0
    # A against the model: the count and a peek of every grain
    assert a.cache_count() == len(m) < 200
    d_pa, d_ps, d_pe, d_pt, d_pl, d_pc = (b.out(n, np.uint32), b.out(n, np.uint8), b.out(n, np.int32), b.out(n, np.int64),
                                          b.out(n, np.int64), b.out(n, np.uint8))
    a.cache_peek_device(b.dev(keys), n, d_pa, d_ps, d_pe, d_pt, d_pl, d_pc, stream=st_)
    t.cuda.synchronize()
    ref = np.zeros(n, [("a", np.uint32), ("s", np.uint8), ("e", np.int32), ("t", np.int64), ("l", np.int64), ("c", np.uint8)])
    ref["a"], ref["s"], ref["e"] = L.NO_ACT, L.NULL_SILO, L.CACHE_NO_ETAG
    for g, k in enumerate(kt):
        en = m.entry(k)
        if en is not None:
            ref[g] = (en.value[0], en.value[1], en.etag, en.expiration_timer, en.last_refreshed, en.num_accesses > 0)
    for d, col, dt in ((d_pa, "a", np.uint32), (d_ps, "s", np.uint8), (d_pe, "e", np.int32), (d_pt, "t", np.int64),
                       (d_pl, "l", np.int64), (d_pc, "c", np.uint8)):
        np.testing.assert_array_equal(b.host(d, n, dt), ref[col], err_msg=col)
    a.close()
    b.close()


def test_context_without_versions(torch, cluster):
    """6.  A context that never enables versions: device insert, remove and merge, then a routed batch, against the model
    and the oracle.  The versioned calls refuse with E_STATE and change nothing."""
    t = torch
    slots = 64
    f = D.family("tail(4)", slots, W.grain_tcd(cluster))
    p = Pair(t, cluster, slots, local=None, versions=False)
    rng = np.random.default_rng(6)
    m = len(f.keys)
    acts = rng.integers(0, N_ACT, m).astype(np.uint32)
    silos = rng.integers(0, N_SILOS, m).astype(np.uint8)
    with pytest.raises(Exception) as e:
        p.eng.lookup_many_device(p.dev(f.keys), p.dev(np.zeros(m, np.int32)), m, p.out(m, np.uint8), p.out(m, np.int32),
                                 p.out(m, np.uint32), p.out(m, np.uint8), stream=p.st)
    assert e.value.code == L.E_STATE
    h = m // 2
    p.register(np.concatenate([f.keys[:h], f.keys[:4]]), np.concatenate([acts[:h], acts[:4] + 1]),
               np.concatenate([silos[:h], silos[:4]]), None, versioned=False)
    p.unregister(f.keys[:h:3])
    ak = np.zeros(N_ACT, L.KEY_DTYPE)
    ak["n1"] = rng.permutation(N_ACT).astype(np.uint64)
    akey = lambda a: (int(ak["tcd"][a]), int(ak["n0"][a]), int(ak["n1"][a]))  # noqa: E731
    mk = np.concatenate([f.keys[h:h + 8], f.keys[1:h:3][:4]])
    ma, ms = rng.integers(0, N_ACT, len(mk)).astype(np.uint32), rng.integers(0, N_SILOS, len(mk)).astype(np.uint8)
    d_st, d_da, d_ds = p.out(len(mk), np.uint8), p.out(len(mk), np.uint32), p.out(len(mk), np.uint8)
    p.eng.merge_directory_device(p.dev(mk), p.dev(ma), p.dev(ms), len(mk), p.dev(ak), N_ACT, d_st, d_da, d_ds, stream=p.st)
    t.cuda.synchronize()
    z = np.zeros(len(mk), np.int32)
    st, da, ds = p.model.merge(mk, ma, ms, z, z, akey, N_ACT)
    np.testing.assert_array_equal(p.host(d_st, len(mk), np.uint8), st)
    np.testing.assert_array_equal(p.host(d_da, len(mk), np.uint32), da)
    np.testing.assert_array_equal(p.host(d_ds, len(mk), np.uint8), ds)
    assert {L.MERGE_INSERTED} < set(st.tolist())
    # route: the oracle holds what the model's partition holds
    o = cpu_ref.Oracle(N_SILOS, seed=0)
    for s in range(N_SILOS):
        o.add_server(s, int(cluster.hashes[s]))
    held = np.array([(k[0], k[1], k[2]) for k in p.model.part.data], L.KEY_DTYPE)
    vals = list(p.model.part.data.values())
    st_o, _, _ = o.register(held, np.array([v[0] for v in vals], np.uint32), np.array([v[1] for v in vals], np.uint8))
    assert (st_o == L.INS_INSERTED).all()
    msgs = D.messages(np.concatenate([f.keys, f.ghosts, f.aliases]), N_SILOS, 1)
    res = p.eng.address_messages(msgs)
    r, a = o.route(msgs)
    np.testing.assert_array_equal(res.route, r)
    np.testing.assert_array_equal(res.act, a)
    order, off = o.bucket(a, N_ACT)
    np.testing.assert_array_equal(res.order, order)
    np.testing.assert_array_equal(res.offsets, off)
    assert p.eng.directory_count() == p.count() == o.size()
    p.close()
