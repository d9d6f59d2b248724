"""Version tags of the directory partition and LookUpMany, without a GPU: the model (versioned_partition_ref.py) pinned on
hand-derived cases, the new exports and constants against the header, and the library's host mirror (a host-only
context, device = -1) against the model through versioned registrations, removals, compaction, a membership change and
lookup_many.  Every comparison is exact."""
import os
import re

import numpy as np
import pytest

import dir_layout as D
import versioned_partition_ref as V
from oracle import pyref as P
from orleans_amd import _lib as L
from orleans_amd import workloads as W
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N_SILOS = 8
N_ACT = 1 << 14
VIEW = P.SiloView([True] * 3, [True, True, False], 0)
G = [P.key_from_long(i, 7) for i in range(8)]


# ---- the model, pinned -------------------------------------------------------------------------------------------------
def _part():
    """Grain 0 on silo 0 under tag 11, grain 1 on the non-functional silo 2 under tag 22 (registered while it was valid)."""
    p = V.VersionedPartition()
    up = P.SiloView([True] * 3, [True] * 3, 0)
    assert p.add_single_activation_versioned(G[0], 100, 0, 11, up) == (P.INS_INSERTED, 100, 0, 11)
    assert p.add_single_activation_versioned(G[1], 101, 2, 22, up) == (P.INS_INSERTED, 101, 2, 22)
    return p


def test_model_lookup_many_kinds_by_hand():
    """One request per row of the kind table (RemoteGrainDirectory.cs:349-380)."""
    p = _part()
    kx = P.key_from_long(5, 7, "ext")
    st = P.key_system_target(12)
    got = V.look_up_many(p, [(G[0], 11), (G[2], 5), (G[0], 10), (G[1], 9), (kx, 0), (st, 0), (G[0], -1), (G[1], 22)], VIEW)
    assert got == [(V.LUM_UNCHANGED, 11, P.NO_ACT, P.NULL_SILO),      # curGen == etag: (grain, curGen, null)
                   (V.LUM_ABSENT, -1, P.NO_ACT, P.NULL_SILO),         # curGen == NO_ETAG
                   (V.LUM_UPDATED, 11, 100, 0),                       # the current version
                   (V.LUM_UPDATED_EMPTY, 22, P.NO_ACT, P.NULL_SILO),  # LookUpGrain filtered the silo: empty list, the tag
                   (V.LUM_UNSUPPORTED, -1, P.NO_ACT, P.NULL_SILO),
                   (V.LUM_UNSUPPORTED, -1, P.NO_ACT, P.NULL_SILO),
                   (V.LUM_UPDATED, 11, 100, 0),                       # etag -1 against a present entry reads the tag back
                   (V.LUM_UNCHANGED, 22, P.NO_ACT, P.NULL_SILO)]      # unchanged needs no valid silo: no LookUpGrain is made
    assert V.response_of([(G[0], 10), (G[1], 9), (G[0], 11), (G[2], 5)], [got[2], got[3], got[0], got[1]]) == [
        (G[0], 11, (100, 0)), (G[1], -1, None), (G[0], 11, None), (G[2], -1, None)]


def test_model_registration_by_hand():
    p = _part()
    assert p.add_single_activation_versioned(G[0], 200, 1, 33, VIEW) == (P.INS_EXISTING, 100, 0, 11)  # the winner's tag
    assert p.add_single_activation_versioned(G[3], 201, 2, 34, VIEW) == (P.INS_INVALID_SILO, P.NO_ACT, P.NULL_SILO, -1)
    assert p.get_grain_etag(G[3]) == -1
    assert p.add_single_activation(G[4], 202, 1, VIEW) == (P.INS_INSERTED, 202, 1) and p.get_grain_etag(G[4]) == 0
    assert p.remove(G[0]) and p.get_grain_etag(G[0]) == -1 and not p.remove(G[0])
    assert p.add_single_activation_versioned(G[0], 203, 1, 35, VIEW) == (P.INS_INSERTED, 203, 1, 35)  # the new draw


def test_model_merge_statuses_by_hand():
    """One entry per merge status (GrainDirectoryPartition.cs:366-383, GrainInfo.Merge :146-183).  ActivationId keys:
    handle h has key (0, 0, order[h])."""
    order = {100: 50, 101: 60, 300: 70, 301: 40, 302: 50, 303: 1, 304: 2}
    akey = lambda h: (0, 0, order[h])  # noqa: E731
    p = _part()
    kx = P.key_from_long(5, 7, "ext")
    out = p.merge_versioned([(G[2], 303, 1, 7, 1000),    # absent: added as is, the incoming tag
                             (G[0], 300, 1, 8, 1001),    # present, ours (50) < theirs (70): kept, the draw
                             (G[1], 301, 1, 9, 1002),    # present, theirs (40) < ours (60): replaced, the draw
                             (G[2], 304, 1, 10, 1003),   # the copy is a dictionary: duplicate
                             (kx, 304, 1, 11, 1004)], akey)
    assert out == [(V.MERGE_INSERTED, P.NO_ACT, P.NULL_SILO), (V.MERGE_KEPT, 300, 1), (V.MERGE_REPLACED, 101, 2),
                   (V.MERGE_DUPLICATE, P.NO_ACT, P.NULL_SILO), (V.MERGE_UNSUPPORTED, P.NO_ACT, P.NULL_SILO)]
    assert [p.get_grain_etag(g) for g in G[:3]] == [1001, 1002, 7]
    assert p.data[p._k(G[1])] == (301, 1) and p.data[p._k(G[0])] == (100, 0)
    assert p.merge_versioned([(G[0], 302, 1, 12, 1005)], akey) == [(V.MERGE_SAME, P.NO_ACT, P.NULL_SILO)]  # same ActivationId
    assert p.get_grain_etag(G[0]) == 1001                                                                # not modified


# ---- the ABI -------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = ("orl_dir_versions_enable", "orl_dir_insert_single_versioned", "orl_dir_insert_single_versioned_device",
               "orl_dir_merge_versioned_device", "orl_dir_lookup_many_device", "orl_dir_lookup_many_host")


def test_exports_and_constants_match_the_header():
    lib = L.load()
    text = open(os.path.join(ROOT, "include", "orleans_route.h")).read()
    for name in NEW_EXPORTS:
        assert name in L.EXPORTED and hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, text), name
    defs = dict(re.findall(r"#define (ORL_(?:LUM_[A-Z_]+|DIR_NO_ETAG|ABI_VERSION)) \(?(-?\d+)u?\)?", text))
    assert {k: int(v) for k, v in defs.items()} == {
        "ORL_ABI_VERSION": 1, "ORL_DIR_NO_ETAG": L.DIR_NO_ETAG, "ORL_LUM_UNCHANGED": L.LUM_UNCHANGED,
        "ORL_LUM_ABSENT": L.LUM_ABSENT, "ORL_LUM_UPDATED": L.LUM_UPDATED, "ORL_LUM_UPDATED_EMPTY": L.LUM_UPDATED_EMPTY,
        "ORL_LUM_UNSUPPORTED": L.LUM_UNSUPPORTED}
    assert (L.LUM_UNCHANGED, L.LUM_ABSENT, L.LUM_UPDATED, L.LUM_UPDATED_EMPTY, L.LUM_UNSUPPORTED) == (
        V.LUM_UNCHANGED, V.LUM_ABSENT, V.LUM_UPDATED, V.LUM_UPDATED_EMPTY, V.LUM_UNSUPPORTED)
    assert L.DIR_NO_ETAG == V.NO_ETAG == -1
    assert lib.orl_abi_version() == L.ABI_VERSION == 1


# ---- the host mirror against the model -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cluster():
    return W.default_cluster(N_SILOS)


LOCAL = [1, 1, 1, 1, 0, 1, 1, 1]  # silo 4's partition is not held: some registrations are REMOTE_OWNER


def _pair(cluster, slots, local=LOCAL):
    eng = GrainDirectoryEngine(n_act=N_ACT, dir_capacity=slots // 2, device=-1)
    eng.set_silos(N_SILOS, local=local, seed=0)
    for s in range(N_SILOS):
        eng.add_server(s, int(cluster.hashes[s]))
    return eng, V.Model(N_SILOS, cluster.hashes, N_ACT, local=local)


def _lookup_equal(eng, model, keys, etags):
    got = eng.lookup_many(keys, etags)
    exp = model.lookup_many(keys, etags)
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)
    return got


def _register_equal(eng, model, keys, acts, silos, tags):
    got = eng.register_single_activation_versioned(keys, acts, silos, tags)
    exp = model.register(keys, acts, silos, tags, device=False)
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)
    return got[0]


@pytest.mark.parametrize("slots,name", [(64, "tail(4)"), (64, "one_slot(63)"), (64, "random"), (4096, "tail(1)")])
def test_host_scenario_against_the_model(cluster, slots, name):
    """Versioned host registrations (each key up to three times under distinct draws, one silo invalid, one owner remote),
    removals, re-registration into the tombstones, compaction, a silo made non-functional: after every step a lookup_many
    of every key, ghost and alias (etag -1, then the etags just read) equals the model."""
    tcd = W.grain_tcd(cluster)
    f = D.family(name, slots, tcd)
    f.check()
    remote = int(cluster.owner_of(W.jenkins3_np(f.keys["tcd"], f.keys["n0"], f.keys["n1"]))[0])
    local = [int(s != remote) for s in range(N_SILOS)]  # the first key's owner is not held here: REMOTE_OWNER occurs
    eng, model = _pair(cluster, slots, local)
    eng.enable_directory_versions()
    eng.enable_directory_versions()  # idempotent
    rng = np.random.default_rng(slots + len(name))
    kx = np.zeros(1, L.KEY_DTYPE)
    kx["tcd"], kx["n1"] = (L.CAT_KEYEXT_GRAIN << 56) + 7, 3
    everything = np.concatenate([f.keys, f.ghosts, f.aliases, kx])

    def check(expect_kinds):
        kind, etag, _, _ = _lookup_equal(eng, model, everything, np.full(len(everything), -1, np.int32))
        kind2, _, _, _ = _lookup_equal(eng, model, everything, etag)
        present = (kind == L.LUM_UPDATED) | (kind == L.LUM_UPDATED_EMPTY)
        assert (kind2[present] == L.LUM_UNCHANGED).all() and (kind2[~present] == kind[~present]).all()
        assert set(kind.tolist()) == expect_kinds
        assert eng.directory_count() == len(model.part.data)

    m = len(f.keys)
    keys = np.concatenate([f.keys, f.keys[::2], f.keys[::4]])
    keys = keys[rng.permutation(len(keys))]
    n = len(keys)
    tags = rng.permutation(1 << 20)[:n].astype(np.int32) + 1
    silos = rng.integers(0, N_SILOS, n).astype(np.uint8)
    eng.set_silos(N_SILOS, functional=[1, 1, 1, 0, 1, 1, 1, 1], local=local, seed=0)  # silo 3 invalid while registering
    model.view.functional[3] = False
    st = _register_equal(eng, model, keys, (np.arange(n) % N_ACT).astype(np.uint32), silos, tags)
    assert {L.INS_INSERTED, L.INS_EXISTING, L.INS_INVALID_SILO, L.INS_REMOTE_OWNER} <= set(st.tolist())
    check({L.LUM_UPDATED, L.LUM_ABSENT, L.LUM_UNSUPPORTED})
    eng.set_silos(N_SILOS, local=local, seed=0)
    model.view.functional[3] = True
    # every other key out; a third of them back under new draws, into the tombstones where the load rule allows it
    gone = f.keys[::2]
    rm = eng.unregister(gone)
    np.testing.assert_array_equal(rm, model.unregister(gone))
    check({L.LUM_UPDATED, L.LUM_ABSENT, L.LUM_UNSUPPORTED})
    back = gone[::3]
    count, tombs = eng.directory_count(), int(rm.sum())
    if (count + tombs + len(back)) * 2 > slots:  # the host insert's load rule counts tombstones
        eng.compact_directory()
        check({L.LUM_UPDATED, L.LUM_ABSENT, L.LUM_UNSUPPORTED})
    nb = len(back)
    _register_equal(eng, model, back, (np.arange(nb) + 9000).astype(np.uint32), rng.integers(0, N_SILOS, nb).astype(np.uint8),
                    (np.arange(nb) + (1 << 21)).astype(np.int32))
    check({L.LUM_UPDATED, L.LUM_ABSENT, L.LUM_UNSUPPORTED})
    eng.compact_directory()  # tags move with their entries
    check({L.LUM_UPDATED, L.LUM_ABSENT, L.LUM_UNSUPPORTED})
    # an unversioned registration on the versioned partition: a draw of 0
    rest = np.setdiff1d(gone, back)[:4]
    st_u, wa_u, ws_u = eng.register_single_activation(rest, np.arange(len(rest), dtype=np.uint32), np.zeros(len(rest), np.uint8))
    exp_u = model.register(rest, np.arange(len(rest)), np.zeros(len(rest), np.uint8), None, device=False)
    np.testing.assert_array_equal(st_u, exp_u[0])
    np.testing.assert_array_equal(wa_u, exp_u[1])
    check({L.LUM_UPDATED, L.LUM_ABSENT, L.LUM_UNSUPPORTED})
    dead = next(iter(model.part.data.values()))[1]  # a hosting silo dies
    eng.set_silos(N_SILOS, functional=[s != dead for s in range(N_SILOS)], local=local, seed=0)
    model.view.functional[dead] = False
    check({L.LUM_UPDATED, L.LUM_UPDATED_EMPTY, L.LUM_ABSENT, L.LUM_UNSUPPORTED})
    eng.close()


def test_enabling_with_entries_present_gives_tag_zero(cluster):
    eng, model = _pair(cluster, 64)
    f = D.family("random", 64, W.grain_tcd(cluster))
    st, _, _ = eng.register_single_activation(f.keys[:8], np.arange(8, dtype=np.uint32), np.zeros(8, np.uint8))
    model.register(f.keys[:8], np.arange(8), np.zeros(8, np.uint8), None, device=False)
    eng.enable_directory_versions()
    kind, etag, _, _ = _lookup_equal(eng, model, f.keys[:10], np.full(10, -1, np.int32))
    ins = st <= L.INS_EXISTING
    assert ins.any() and (etag[:8][ins] == 0).all() and (kind[8:] == L.LUM_ABSENT).all()
    eng.close()


def test_refusals(cluster):
    eng, _ = _pair(cluster, 64)
    k = D.family("random", 64, W.grain_tcd(cluster)).keys[:4]
    a, s, tg = np.arange(4, dtype=np.uint32), np.zeros(4, np.uint8), np.array([5, 6, -1, 7], np.int32)
    out = np.zeros(64, np.uint8)

    def code(fn, *args, **kw):
        with pytest.raises(OrleansRouteError) as e:
            fn(*args, **kw)
        return e.value.code

    # before enabling: every versioned call, host or device form
    assert code(eng.register_single_activation_versioned, k, a, s, np.abs(tg)) == L.E_STATE
    assert code(eng.lookup_many, k, tg) == L.E_STATE
    assert code(eng.register_single_activation_versioned_device, out, out, out, out, 4, out) == L.E_STATE
    assert code(eng.merge_directory_versioned_device, out, out, out, out, out, 4, out, 4, out) == L.E_STATE
    assert code(eng.lookup_many_device, out, out, 4, out, out, out, out) == L.E_STATE
    eng.enable_directory_versions()
    # a host-only context: the device forms still refuse (nothing is dereferenced)
    assert code(eng.register_single_activation_versioned_device, out, out, out, out, 4, out) == L.E_STATE
    assert code(eng.merge_directory_versioned_device, out, out, out, out, out, 4, out, 4, out) == L.E_STATE
    assert code(eng.lookup_many_device, out, out, 4, out, out, out, out) == L.E_STATE
    # a negative draw: E_INVALID, and the messages before it are not applied either
    assert code(eng.register_single_activation_versioned, k, a, s, tg) == L.E_INVALID
    assert eng.directory_count() == 0
    kind, _, _, _ = eng.lookup_many(k, np.full(4, -1, np.int32))
    assert (kind == L.LUM_ABSENT).all()
    eng.close()
