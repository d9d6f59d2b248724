"""Stateless-worker routing restated on the CPU (test infrastructure).

The reference never registers a [StatelessWorker] grain in the grain directory (Catalog.cs:1156-1185,
singleActivationMode = !activation.IsStatelessWorker); StatelessWorkerDirector (src/OrleansRuntime/Placement/
StatelessWorkerDirector.cs:35-80) picks one of the SENDING silo's own activations or asks for a new one there.
`LocalCatalog` is the per-silo activation list that director reads, `route` lays its decision over the directory
oracle's answer for the listed types, and `expected_node` is tests/node_replay.expected with the two changes such a
message makes to the node exchange.  Paths are relative to randa1/orleans.
"""
from __future__ import annotations

import numpy as np

from orleans_amd import _lib as L
from orleans_amd import workloads as W

import node_replay as NR

def pack(owner: int, host: int, status: int, flags: int) -> int:
    return (owner & 0xFF) | ((host & 0xFF) << 8) | ((status & 0xFF) << 16) | ((flags & 0xFF) << 24)


class LocalCatalog:
    """activations of stateless-worker grains per (grain, silo): List<ActivationData> in insertion order with a busy
    flag each (busy = not (State == Valid && IsInactive), StatelessWorkerDirector.cs:54-55)."""

    def __init__(self, types: dict, n_act: int, n_silos: int):
        self.types = {int(t): int(m) for t, m in types.items()}  # TypeCodeData -> MaxLocal (GrainTypeData.cs:43-50,115)
        self.n_act, self.n_silos = int(n_act), int(n_silos)
        self.lists = {}  # (tcd, n0, n1, silo) -> [[act, busy], ...]

    @staticmethod
    def _k(key, silo):
        return (int(key["tcd"]), int(key["n0"]), int(key["n1"]), int(silo))

    def add(self, key, act: int, silo: int) -> int:
        """Catalog.RegisterMessageTarget (Catalog.cs:1169-1181): appended, or DuplicateActivationException at MaxLocal."""
        tcd = int(key["tcd"])
        if tcd not in self.types or act >= self.n_act or silo >= self.n_silos:
            return L.SW_UNSUPPORTED
        lst = self.lists.get(self._k(key, silo), [])
        if any(a == act for a, _ in lst):
            return L.SW_UNSUPPORTED
        if len(lst) >= self.types[tcd]:
            return L.SW_DUPLICATE  # :1176-1180, the list is left as it is
        lst.append([int(act), False])
        self.lists[self._k(key, silo)] = lst
        return L.SW_ADDED

    def remove(self, key, act: int, silo: int) -> bool:
        """Activation destroy: List.Remove keeps the order of the rest; an emptied list goes away."""
        k = self._k(key, silo)
        lst = self.lists.get(k, [])
        for i, (a, _) in enumerate(lst):
            if a == act:
                del lst[i]
                if not lst:
                    del self.lists[k]
                return True
        return False

    def set_busy(self, key, act: int, silo: int, busy: bool) -> bool:
        for e in self.lists.get(self._k(key, silo), []):
            if e[0] == act:
                e[1] = bool(busy)
                return True
        return False

    def lookup(self, key, silo: int):
        return [tuple(e) for e in self.lists.get(self._k(key, silo), [])]

    def count(self) -> int:
        return len(self.lists)

    def select(self, tcd: int, n0: int, n1: int, me: int, h: int):
        """StatelessWorkerDirector.OnSelectActivation (:35-67) for a message sent by silo `me`: (route word, act).
        h % count stands in for random.Next (:62-63)."""
        rf = L.RF_STATELESS | L.RF_LOOPBACK
        lst = self.lists.get((tcd, n0, n1, me), [])
        new = (pack(0xFF, me, L.ST_NEW_PLACEMENT, rf | L.RF_NEW_PLACEMENT), L.NO_ACT)
        if not lst:                                   # :46-47 -> OnAddActivation on the local silo (:69-74)
            return new
        for a, busy in lst:                           # :51-58: the first idle activation in list order
            if not busy:
                return pack(0xFF, me, L.ST_HIT, rf), a
        if len(lst) >= self.types[tcd]:               # :60-64
            return pack(0xFF, me, L.ST_HIT, rf), lst[0 if len(lst) == 1 else h % len(lst)][0]
        return new                                    # :66


def listed(msgs: np.ndarray, types) -> np.ndarray:
    """Messages the stateless-worker path takes: a listed type and no complete address."""
    t = np.asarray([int(x) for x in types], np.uint64)
    return np.isin(msgs["tcd"], t) & ((msgs["flags"] & L.HDR_ADDRESS_COMPLETE) == 0)


def hashes(msgs: np.ndarray) -> np.ndarray:
    """The uniform hash, or aux when the header carries it (ORL_HDR_HASH_VALID)."""
    h = W.jenkins3_np(msgs["tcd"], msgs["n0"], msgs["n1"])
    return np.where(msgs["flags"] & L.HDR_HASH_VALID, msgs["aux"], h).astype(np.uint32)


def route(oracle, catalog: LocalCatalog, types, msgs: np.ndarray, opts: int = 0):
    """cpu_ref.Oracle.route with the StatelessWorkerDirector's decision laid over the listed-type messages."""
    r, a = oracle.route(msgs, opts)
    r, a = r.copy(), a.copy()
    sw = np.nonzero(listed(msgs, types))[0]
    if len(sw):
        h = hashes(msgs[sw])
        m = msgs[sw]
        for j, i in enumerate(sw):
            r[i], a[i] = catalog.select(int(m["tcd"][j]), int(m["n0"][j]), int(m["n1"][j]), int(m["sending_silo"][j]),
                                        int(h[j]))
    return r, a


def row_of(catalog: LocalCatalog, msg) -> str:
    """Which row of the semantics table decided a listed-type message (for the tests' coverage assertions)."""
    lst = catalog.lookup(msg, int(msg["sending_silo"]))
    if not lst:
        return "absent"
    if any(not b for _, b in lst):
        return "idle"
    if len(lst) >= catalog.types[int(msg["tcd"])]:
        return "full1" if len(lst) == 1 else "fullN"
    return "grow"


def expected_node(oracles, catalogs, types, ros, batches, chunks, n_act, caches=None, functional=None, opts: int = 0):
    """node_replay.expected restated with the two changes a stateless-worker message makes: its hop-1 destination is
    its sender's rank (it is never sent to a directory owner), and its route and act come from that rank's local
    catalog.  Also returns sent[s][d], the listed-type messages rank s sent to rank d in hop 1 (zero off the diagonal),
    and remote[s], all the messages rank s sent to other ranks in hop 1."""
    from oracle import pyref as P
    nr = len(batches)
    functional = functional if functional is not None else [1] * 8
    owned = [[] for _ in range(nr)]
    pre = [[] for _ in range(nr)]
    sent = np.zeros((nr, nr), np.int64)
    remote = np.zeros(nr, np.int64)
    for c in range(chunks):
        for s in range(nr):
            lo, hi = NR.chunk_bounds(len(batches[s]), chunks, c)
            ch = batches[s][lo:hi].copy()
            src, cnt = oracles[0].partition(ch, ros, nr, s, opts)
            dest = np.zeros(len(ch), np.int64)
            o0 = 0
            for d in range(nr):
                dest[src[o0:o0 + int(cnt[d])]] = d
                o0 += int(cnt[d])
            sw = listed(ch, types)
            dest[sw] = s  # change 1: routed where it was sent
            croute = np.full(len(ch), -1, np.int64)
            cact = np.zeros(len(ch), np.uint32)
            if caches is not None and caches[s] and len(ch):
                r0, a0 = oracles[s].route(ch)
                kt = list(zip(ch["tcd"].tolist(), ch["n0"].tolist(), ch["n1"].tolist()))
                r1, a1 = P.apply_directory_cache(r0.tolist(), a0.tolist(), ch["sending_silo"].tolist(), kt, caches[s],
                                                 functional)
                r1 = np.array(r1, np.uint32)
                hit = (r1 >> 24) & 0x08 != 0
                hit &= ((r0 >> 16) & 0xFF) == L.ST_REMOTE_OWNER
                hit &= ~sw  # the type test comes before the cache probe
                hs = ((r1 >> 8) & 0xFF).astype(np.int64)
                dest[hit] = ros[hs[hit]]
                croute[hit] = r1[hit]
                cact[hit] = np.array(a1, np.uint32)[hit]
                ch["target_silo"][hit] = hs[hit].astype(np.uint8)
            for d in range(nr):
                sent[s, d] += int((sw & (dest == d)).sum())
            remote[s] += int((dest != s).sum())
            order = np.argsort(dest, kind="stable")
            for d in range(nr):
                sel = order[dest[order] == d]
                owned[d].append(ch[sel])
                pre[d].append((croute[sel], cact[sel]))
    owned = [np.concatenate(x) if x else np.zeros(0, L.MSG_DTYPE) for x in owned]
    routed = []
    for d in range(nr):
        r, a = route(oracles[d], catalogs[d], types, owned[d], opts)  # change 2: rank d's catalog decides them
        if pre[d]:
            cr = np.concatenate([x[0] for x in pre[d]])
            ca = np.concatenate([x[1] for x in pre[d]])
            m = cr >= 0
            own_dir = ((r >> 16) & 0xFF) != L.ST_REMOTE_OWNER
            crw = cr.astype(np.uint32)
            same = (((r >> 16) & 0xFF) == L.ST_HIT) & (a == ca) & (((r >> 8) & 0xFF) == ((crw >> 8) & 0xFF))
            keep = m & (~own_dir | same)
            stale = m & own_dir & ~same
            r[keep] = crw[keep]
            a[keep] = ca[keep]
            r[stale] |= np.uint32(L.RF_CACHE_STALE << 24)
        routed.append((r, a))
    hostr = [NR.host_rank(routed[d][0], ros, d) for d in range(nr)]
    forward = any((hostr[d] != d).any() for d in range(nr))
    out = []
    for hr in range(nr):
        if forward:
            sel = [hostr[o] == hr for o in range(nr)]
            hdr = np.concatenate([owned[o][sel[o]] for o in range(nr)])
            rt = np.concatenate([routed[o][0][sel[o]] for o in range(nr)])
            act = np.concatenate([routed[o][1][sel[o]] for o in range(nr)])
        else:
            hdr, (rt, act) = owned[hr], routed[hr]
        order, off = oracles[hr].bucket(act, n_act)
        out.append((rt, act, order, off, hdr))
    return out, forward, sent, remote
