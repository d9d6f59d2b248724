"""The reference's directory partition with its version tags, and the owner's side of the cache refresh, restated in Python
over oracle/pyref.Partition (test infrastructure, like adaptive_cache_ref.py): what the tag stores of the registration and
merge kernels, the host mirror and orleans_amd/csrc/dir_versions.hip must compute.  Paths are relative to the reference's
src/OrleansRuntime/GrainDirectory/.

  VersionedPartition.add_single_activation_versioned   GrainDirectoryPartition.AddSingleActivation, GrainDirectoryPartition.cs:270-287
                                                       (GrainInfo.AddSingleActivation :100-114: VersionTag = rand.Next() on insert)
  VersionedPartition.remove                            RemoveGrain / RemoveActivation(force), :290-318 (the GrainInfo leaves the dictionary)
  VersionedPartition.merge_versioned                   Merge, :366-383, with GrainInfo.Merge, :146-183
  VersionedPartition.get_grain_etag / look_up_grain    GetGrainETag, :346-359, LookUpGrain, :326-344
  look_up_many                                         RemoteGrainDirectory.LookUpMany, RemoteGrainDirectory.cs:349-380
  register_versioned                                   LocalGrainDirectory.RegisterSingleActivationAsync (pyref.register_single_activation)
                                                       with the library's per-message refusals

rand.Next() is the caller's: every method that would draw takes the draw as an argument (DESIGN §2 does the same for
ActivationId.NewId and SafeRandom).  A GrainInfo is constructed with VersionTag = 0 (:57-70), which is what an entry
registered through the unversioned calls carries."""
from __future__ import annotations

import numpy as np

from oracle import pyref as P

NO_ETAG = -1  # GrainInfo.NO_ETAG
LUM_UNCHANGED, LUM_ABSENT, LUM_UPDATED, LUM_UPDATED_EMPTY, LUM_UNSUPPORTED = 0, 1, 2, 3, 4
MERGE_INSERTED, MERGE_KEPT, MERGE_REPLACED, MERGE_SAME, MERGE_DUPLICATE, MERGE_UNSUPPORTED = 0, 1, 2, 3, 4, 5


class VersionedPartition(P.Partition):
    """pyref.Partition plus GrainInfo.VersionTag per grain (self.tag, keyed like self.data)."""

    def __init__(self) -> None:
        super().__init__()
        self.tag = {}

    def add_single_activation(self, key, act, silo, view):  # the unversioned call: GrainInfo()'s tag, a draw of 0
        st, a, s, _ = self.add_single_activation_versioned(key, act, silo, 0, view)
        return st, a, s

    def add_single_activation_versioned(self, key, act, silo, draw, view):
        """Returns (status, winner act, winner silo, the grain's VersionTag after the call or NO_ETAG)."""
        st, a, s = super().add_single_activation(key, act, silo, view)
        k = self._k(key)
        if st == P.INS_INSERTED:
            self.tag[k] = draw                     # :111
        if st in (P.INS_INSERTED, P.INS_EXISTING):
            return st, a, s, self.tag[k]
        return st, a, s, NO_ETAG                   # AddSingleActivation returned null (:277-279)

    def remove(self, key) -> bool:
        self.tag.pop(self._k(key), None)
        return super().remove(key)

    def merge(self, entries, act_key_of):  # the unversioned call: tags and draws of 0
        return self.merge_versioned([(k, a, s, 0, 0) for k, a, s in entries], act_key_of)

    def merge_versioned(self, entries, act_key_of):
        """entries: (Key, act, silo, the incoming GrainInfo's VersionTag, a draw).  An absent grain's GrainInfo is added as
        is, tag included (:376-379).  For a present one GrainInfo.Merge adds the other's instance unless the same
        ActivationId is there (:149-155), and `modified` then draws a new tag (:157-160) before the single-activation
        clean-up picks the survivor: KEPT and REPLACED both carry the draw, SAME keeps the old tag."""
        out = super().merge([(k, a, s) for k, a, s, _, _ in entries], act_key_of)
        done = set()
        for (key, _, _, tag, draw), (st, _, _) in zip(entries, out):
            k = self._k(key)
            if st == MERGE_INSERTED:
                self.tag[k] = tag
            elif st in (MERGE_KEPT, MERGE_REPLACED):
                self.tag[k] = draw
            assert st in (MERGE_DUPLICATE, MERGE_UNSUPPORTED) or k not in done
            done.add(k)
        return out

    def get_grain_etag(self, key) -> int:  # :346-359
        return self.tag.get(self._k(key), NO_ETAG)

    def look_up_grain(self, key, view):
        """LookUpGrain :326-344: None when the grain is absent, else (the IsValidSilo-filtered activation list, tag)."""
        k = self._k(key)
        if k not in self.data:
            return None
        act, silo = self.data[k]
        return ([(act, silo)] if view.functional[silo] else []), self.tag[k]


def look_up_many(part: VersionedPartition, requests, view):
    """RemoteGrainDirectory.LookUpMany over (Key, etag) requests; per request (kind, etag, act, silo).  KeyExt and
    SystemTarget keys are not held in the engine's partition (LUM_UNSUPPORTED)."""
    out = []
    for key, etag in requests:
        if key.category in (P.CAT_KEYEXT_GRAIN, P.CAT_SYSTEM_TARGET):
            out.append((LUM_UNSUPPORTED, NO_ETAG, P.NO_ACT, P.NULL_SILO))
            continue
        cur = part.get_grain_etag(key)                                  # :358
        if cur == NO_ETAG:                                              # :359-363 (curGen = -1)
            out.append((LUM_ABSENT, NO_ETAG, P.NO_ACT, P.NULL_SILO))
        elif cur == etag:                                               # :359-363: (grain, curGen, null)
            out.append((LUM_UNCHANGED, cur, P.NO_ACT, P.NULL_SILO))
        else:
            acts, tag = part.look_up_grain(key, view)                   # :367-372 (not removed concurrently here)
            if acts:
                out.append((LUM_UPDATED, tag, acts[0][0], acts[0][1]))
            else:
                out.append((LUM_UPDATED_EMPTY, tag, P.NO_ACT, P.NULL_SILO))
    return out


def response_of(requests, answers):
    """A LookUpMany answer as the tuples adaptive_cache_ref.process_cache_refresh_response takes: (grain, etag, value or
    None).  The reference's value for LUM_UPDATED_EMPTY is an empty list; the device cache holds one activation per grain
    and no empty lists, so the requester removes the entry: (grain, NO_ETAG, None)."""
    out = []
    for (key, _), (kind, etag, act, silo) in zip(requests, answers):
        if kind == LUM_UPDATED:
            out.append((key, etag, (act, silo)))
        elif kind == LUM_UNCHANGED:
            out.append((key, etag, None))
        else:
            out.append((key, NO_ETAG, None))
    return out


def register_versioned(ring, part: VersionedPartition, view, key, act, silo, draw, n_act, n_silos, device=True):
    """One message of orl_dir_insert_single_versioned_device (device=True: an out-of-range handle or silo and a negative
    draw give INS_UNSUPPORTED for that message) or of the unversioned device call (draw None: a draw of 0).  Returns
    (status, winner act, winner silo, winner tag)."""
    bad = act >= n_act or silo >= n_silos or (draw is not None and draw < 0)
    if device and bad:
        return P.INS_UNSUPPORTED, P.NO_ACT, P.NULL_SILO, NO_ETAG
    assert not bad
    if key.category in (P.CAT_KEYEXT_GRAIN, P.CAT_SYSTEM_TARGET):
        return P.INS_UNSUPPORTED, P.NO_ACT, P.NULL_SILO, NO_ETAG
    owner, code = P.calculate_target_silo(ring, key, P.uniform_hash(key), silo, view, True)
    if code != P.OWN_OK:
        return P.INS_OWNER_NULL, P.NO_ACT, P.NULL_SILO, NO_ETAG
    if not view.is_local(owner):
        return P.INS_REMOTE_OWNER, P.NO_ACT, P.NULL_SILO, NO_ETAG
    return part.add_single_activation_versioned(key, act, silo, 0 if draw is None else draw, view)


class Model:
    """One context's ring, membership view and versioned partition, driven with the arrays the engine takes (KEY_DTYPE
    records, numpy arrays) and answering with the arrays it returns."""

    def __init__(self, n_silos, hashes, n_act, local=None, seed=0):
        self.n_silos, self.n_act = n_silos, n_act
        self.ring = P.Ring()
        for s in range(len(hashes)):  # the ring may hold fewer silos than the table
            self.ring.add_server(s, int(hashes[s]))
        self.view = P.SiloView([True] * n_silos, [True] * n_silos, seed, None if local is None else list(local))
        self.part = VersionedPartition()

    @staticmethod
    def key(rec) -> P.Key:
        return P.Key(int(rec["tcd"]), int(rec["n0"]), int(rec["n1"]))

    def register(self, keys, acts, silos, tags=None, device=True):
        """A registration batch, one message at a time in batch order; tags None = the unversioned call."""
        out = [register_versioned(self.ring, self.part, self.view, self.key(k), int(a), int(s),
                                  None if tags is None else int(tags[i]), self.n_act, self.n_silos, device)
               for i, (k, a, s) in enumerate(zip(keys, acts, silos))]
        return (np.array([o[0] for o in out], np.uint8), np.array([o[1] for o in out], np.uint32),
                np.array([o[2] for o in out], np.uint8), np.array([o[3] for o in out], np.int32))

    def unregister(self, keys):
        return np.array([self.part.remove(self.key(k)) for k in keys], np.uint8)

    def lookup_many(self, keys, etags):
        out = look_up_many(self.part, [(self.key(k), int(e)) for k, e in zip(keys, etags)], self.view)
        return (np.array([o[0] for o in out], np.uint8), np.array([o[1] for o in out], np.int32),
                np.array([o[2] for o in out], np.uint32), np.array([o[3] for o in out], np.uint8))

    def merge(self, keys, acts, silos, tags, draws, act_key_of, n_act_keys):
        """orl_dir_merge_versioned_device: an out-of-range handle or silo and a negative tag or draw give
        MERGE_UNSUPPORTED for that entry, which then takes no part (it is no first occurrence of its key)."""
        n = len(keys)
        bad = [int(acts[i]) >= min(self.n_act, n_act_keys) or int(silos[i]) >= self.n_silos or int(tags[i]) < 0 or int(draws[i]) < 0
               for i in range(n)]
        good = [i for i in range(n) if not bad[i]]
        res = self.part.merge_versioned([(self.key(keys[i]), int(acts[i]), int(silos[i]), int(tags[i]), int(draws[i]))
                                         for i in good], act_key_of)
        out = [(MERGE_UNSUPPORTED, P.NO_ACT, P.NULL_SILO)] * n
        for i, r in zip(good, res):
            out[i] = r
        return (np.array([o[0] for o in out], np.uint8), np.array([o[1] for o in out], np.uint32),
                np.array([o[2] for o in out], np.uint8))
