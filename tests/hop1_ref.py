"""The node protocol's hop 1 with the sender's directory cache, restated over the oracle (test infrastructure): what
orl_partition_cached_device and orl_route_received_device must compute, and the constructed batches their tests use.
Plain numpy and Python over oracle.cpu_ref.Oracle, cpu_ref's wire codecs, oracle.pyref's cache rules and the cache models
of tests/adaptive_cache_ref.py / tests/cache_evict_ref.py; the library under test is never called.

  sender          LocalLookup's non-owner branch per message (LocalGrainDirectory.cs:690-717: TryGetValue stamps a found
                  entry, GetLocalCacheData's IsValidSilo filters after, :711-717), Dispatcher.AddressMessage's TargetSilo
                  (Dispatcher.cs:555-579) and OutboundMessageQueue.SendMessage's per-target queues (:113-145) as padded
                  per-rank regions with the act lane beside them
  receiver        the receiving silo: the directory decides where it holds the grain's partition (a stale address is
                  re-addressed, NonExistentActivation → forward, Dispatcher.cs:138-182); elsewhere the record is taken as
                  addressed, under the receiver's IsValidSilo
  case_batch      a constructed sender batch with the classes S1-S9 (and a precomputed hash, 32-B records) at known
                  indices; null_owner_case: S8's null owner, which needs the sender alone on the ring (:483-493)
  receiver_cases  constructed received records with the classes R1-R7

tests/test_hop1_ref.py pins the builders' classes and pins sender + receiver to node_replay.expected."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import cpu_ref, pyref as P
from orleans_amd import _lib as L

NO_ACT = np.uint32(L.NO_ACT)
REC_DTYPE = {32: L.MSG_DTYPE, 16: cpu_ref.WIRE_DTYPE, 8: cpu_ref.WIRE8_DTYPE}
PART_TILE, WAVE_SHARE, ROUTE_TILE = 2048, 512, 4096  # kPartTile, a wave's share of it, kTile (route_kernels.hip)
PROBED = (L.ST_HIT, L.ST_NEW_PLACEMENT, L.ST_CLIENT_UNREGISTERED)  # the words a directory probe ends in


def status_of(route):
    return (np.asarray(route, np.uint32) >> 16) & 0xFF


def key_tuples(m):
    return list(zip(m["tcd"].tolist(), m["n0"].tolist(), m["n1"].tolist()))


def _look_up(cache, key):
    """One LookUp: AdaptiveCache.look_up (a stamp and NumAccesses), LRUCache.try_get (a stamp) or a plain dict."""
    if hasattr(cache, "look_up"):
        r = cache.look_up(key)
        return None if r is None else r[0]
    if hasattr(cache, "try_get"):
        return cache.try_get(key)
    return cache.get(key)


def encode(hdrs, fmt, wire_types=()):
    """-> (records of width fmt, has-16-B-form mask, has-8-B-form mask)."""
    r16, ok16 = cpu_ref.wire_encode(hdrs)
    if fmt == 32:
        return hdrs.copy(), ok16, np.ones(len(hdrs), bool)
    if fmt == 16:
        return r16, ok16, np.ones(len(hdrs), bool)
    assert fmt == 8, fmt
    r8, ok8 = cpu_ref.narrow_encode(hdrs, wire_types)
    return r8, ok16, ok8


@dataclass
class Hop1:
    regions: list          # per destination rank: the records, arrival order
    lanes: list            # per destination rank: uint32, the cached handle or ORL_NO_ACT
    counts: np.ndarray     # uint64[nranks]
    status: int            # the form bits | ORL_PART_CACHED
    dest: np.ndarray       # per message, batch order
    lane: np.ndarray       # per message, batch order
    hdr: np.ndarray        # per message, batch order: the header as sent (TargetSilo rewritten where addressed)
    looked: list = field(default_factory=list)  # indices of the messages that looked the cache up, batch order
    found: list = field(default_factory=list)   # those whose entry was there (stamped / accessed), valid silo or not

    def headers_for(self, d):
        return self.hdr[self.dest == d]


def sender(oracle, cache, msgs, ros, nranks, my_rank, fmt, opts=0, functional=None, wire_types=(), sw_types=()):
    """Hop 1 of one batch at the rank `oracle` describes (its `local` mask = the partitions the rank holds).  cache: None,
    a dict {key: (act, silo)}, a pyref.LRUCache or an adaptive_cache_ref.AdaptiveCache; the lookups' side effect is left on
    it.  sw_types: the rank's stateless-worker types (their messages never reach the directory, Catalog.cs:1156-1185)."""
    msgs = np.ascontiguousarray(msgs, L.MSG_DTYPE)
    n = len(msgs)
    ros = np.asarray(ros, np.uint8)
    functional = [1] * 8 if functional is None else functional
    src, cnt = oracle.partition(msgs, ros, nranks, my_rank, opts)
    dest = np.zeros(n, np.int64)
    o0 = 0
    for d in range(nranks):
        dest[src[o0:o0 + int(cnt[d])]] = d
        o0 += int(cnt[d])
    r0, _ = oracle.route(msgs, opts)  # this rank's view: REMOTE_OWNER where another rank holds the partition
    complete = (msgs["flags"] & L.HDR_ADDRESS_COMPLETE) != 0
    listed = np.isin(msgs["tcd"], np.asarray(list(sw_types), np.uint64)) & ~complete
    dest[listed] = my_rank
    lane = np.full(n, NO_ACT, np.uint32)
    hdr = msgs.copy()
    looked, found = [], []
    if cache is not None:
        kt = key_tuples(msgs)
        for i in np.nonzero((status_of(r0) == L.ST_REMOTE_OWNER) & ~listed)[0].tolist():
            looked.append(i)
            v = _look_up(cache, kt[i])  # TryGetValue: the stamp, before IsValidSilo
            if v is None:
                continue
            found.append(i)
            act, silo = v
            if not functional[silo]:
                continue
            dest[i], lane[i] = ros[silo], act
            hdr["target_silo"][i] = silo
    recs, ok16, ok8 = encode(hdr, fmt, wire_types)
    st = 0
    if fmt == 16:
        st = int(not ok16.all())
    elif fmt == 8:
        st = int(not ok16.all()) | (int(not ok8.all()) << 1)
    if (lane != NO_ACT).any():
        st |= L.PART_CACHED
    order = np.argsort(dest, kind="stable")
    regions, lanes = [], []
    for d in range(nranks):
        sel = order[dest[order] == d]
        regions.append(recs[sel])
        lanes.append(lane[sel])
    counts = np.bincount(dest, minlength=nranks).astype(np.uint64)
    return Hop1(regions, lanes, counts, st, dest, lane, hdr, looked, found)


def receiver(oracle, recs_as_headers, lane, functional, opts=0, cache=None):
    """(route, act) of received hop-1 records at the rank `oracle` describes (sender_cached / cached_verdict in
    route_kernels.hip; node_replay.expected restates the same rule).  cache (optional): the receiver's own directory cache;
    only the records that were NOT addressed by their sender look it up."""
    hdrs = np.ascontiguousarray(recs_as_headers, L.MSG_DTYPE)
    lane = np.asarray(lane, np.uint32)
    r, a = oracle.route(hdrs, opts)
    r, a = r.copy(), a.copy()
    st = status_of(r)
    kt = key_tuples(hdrs)
    plain = lane == NO_ACT
    if cache is not None and plain.any():
        idx = np.nonzero(plain)[0]
        r1, a1 = P.apply_directory_cache_lru(r[idx].tolist(), a[idx].tolist(), hdrs["sending_silo"][idx].tolist(),
                                             [kt[i] for i in idx.tolist()], _AsLRU(cache), functional)
        r[idx], a[idx] = np.array(r1, np.uint32), np.array(a1, np.uint32)
    for i in np.nonzero(~plain)[0].tolist():
        ts = int(hdrs["target_silo"][i])
        if st[i] == L.ST_REMOTE_OWNER:  # partition not held here: taken as addressed, under this rank's IsValidSilo
            r1, a1 = P.apply_directory_cache([int(r[i])], [int(a[i])], [int(hdrs["sending_silo"][i])], [kt[i]],
                                             {kt[i]: (int(lane[i]), ts)}, functional)
            r[i], a[i] = r1[0], a1[0]
        elif st[i] in PROBED:  # held here: the directory decides
            host = (int(r[i]) >> 8) & 0xFF
            if st[i] == L.ST_HIT and a[i] == lane[i] and host == ts and functional[ts]:
                r[i] |= np.uint32(L.RF_CACHED << 24)
            else:
                r[i] |= np.uint32(L.RF_CACHE_STALE << 24)
        else:
            raise ValueError(f"record {i}: a lane entry on a message that needs no directory (status {st[i]})")
    return r, a


class _AsLRU:
    """The try_get shape apply_directory_cache_lru asks for, over any cache _look_up takes."""

    def __init__(self, cache):
        self.cache = cache

    def try_get(self, key):
        return _look_up(self.cache, key)


# ---- the constructed sender batch -------------------------------------------------------------------------------------

CASE_N = 5 * PART_TILE + 1  # five partition tiles and one message
SYS_TCD = (L.CAT_SYSTEM_TARGET << 56) | 12
# class -> indices: both edges of a wave's share, of a tile, of the batch; S9 once per tile, its last the batch's last
CASE_AT = {
    "S1": [0, 63, 64, 2047],
    "S2": [1, 65, 2048, 10239],
    "S3": [2, 511, 512, 4095, 4096],
    "S4": [3, 513, 2049, 6143],
    "S5": [4, 1023, 1024, 6144, 8191],
    "S6": [5, 1535, 8192],
    "S7": [6, 7, 3000, 3001],           # even positions of the list: a system target; odd: a KeyExt-category key
    "S8": [8, 1536, 9000],
    "S9": [9, 700, 2050, 4100, 6150, 8200, 10240],
    "HV": [10, 5000],                    # 32-B records only
}


def keyext_tcd(cl):
    return ((L.CAT_KEYEXT_GRAIN << 56) + (cl.type_code & 0x00FFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF


def grain_tcd(cl):
    return ((L.CAT_GRAIN << 56) + (cl.type_code & 0x00FFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF


def wire_types_of(world):
    """Wire types under which every message of case_batch has the 8-B form (the grain type not at index 0)."""
    return [SYS_TCD, grain_tcd(world.cl), keyext_tcd(world.cl)]


@dataclass
class Case:
    msgs: np.ndarray
    cls: np.ndarray        # per message: "S1" ... "S9", "HV", or "" for the filler
    at: dict               # class -> indices
    opts: int
    cache_keys: np.ndarray  # the sender's cache, in add order: KEY_DTYPE, acts, silos (all valid entries, distinct keys)
    cache_acts: np.ndarray
    cache_silos: np.ndarray
    cold: np.ndarray       # positions in cache_keys of background entries no message targets
    stopped: int           # the local silo that is not running (S8's sender)
    s8_owner: int          # the owner of S8's grains once that silo is excluded (their owner when it is not: `stopped`)

    def entries(self):
        kt = key_tuples(self.cache_keys)
        return [(k, (int(a), int(s))) for k, a, s in zip(kt, self.cache_acts.tolist(), self.cache_silos.tolist())]


def stopping_world(n_grains=5000):
    """cache_evict_ref.World with local silo 1 not running (S8's sender)."""
    from cache_evict_ref import World
    return World(n_grains, running=[1, 0, 1, 1, 1, 1, 1, 1])


def case_batch(world, ros, my_rank, fmt=32, n=CASE_N, n_background=1500, seed=1):
    """The constructed batch for the rank of `world` (silos 0 and 1 local, silo 6 not functional, one local silo not
    running).  ros / my_rank choose S3's "third rank" silo; fmt 32 adds the precomputed-hash class."""
    w = world
    assert n >= CASE_N, n
    ros = np.asarray(ros, np.uint8)
    rng = np.random.default_rng(seed)
    stopped = [s for s in range(8) if w.local[s] and not w.running[s]]
    assert len(stopped) == 1 and ros[0] == my_rank and w.local[0] and w.running[0], "the world of stopping_world()"
    stopped = stopped[0]
    remote = rng.permutation(w.remote)
    own_of = w.owner
    take = iter(remote.tolist())

    def remote_grains(k, ok=lambda g: True):
        out = []
        while len(out) < k:
            g = next(take)
            if ok(g):
                out.append(g)
        return out

    ck, ca, cs = [], [], []

    def cache_add(g_or_key, act, silo):
        ck.append(w.kt[g_or_key] if isinstance(g_or_key, int) else g_or_key)
        ca.append(act)
        cs.append(silo)

    def third_silo(g):
        """A functional silo this rank does not host, on a rank that is neither mine nor the owner's where one exists."""
        c = [s for s in range(8) if w.functional[s] and not w.local[s] and s != own_of[g]]
        best = [s for s in c if ros[s] != my_rank and ros[s] != ros[own_of[g]]]
        return (best or c)[g % len(best or c)]

    m = np.zeros(n, L.MSG_DTYPE)
    cls = np.zeros(n, "U2")
    for name, at in CASE_AT.items():
        if name != "HV" or fmt == 32:
            cls[at] = name
    m["tcd"] = grain_tcd(w.cl)
    m["category"] = 2
    m["sending_silo"] = 0

    def put(name, grains, **kw):
        at = CASE_AT[name]
        m["n1"][at] = np.asarray(grains, np.uint64)
        for f, v in kw.items():
            m[f][at] = v

    mine_run = [g for g in w.mine.tolist() if own_of[g] != stopped]
    s1 = rng.choice(mine_run, len(CASE_AT["S1"]), replace=False).tolist()
    put("S1", s1)
    s2 = remote_grains(len(CASE_AT["S2"]))
    put("S2", s2)
    s3 = remote_grains(len(CASE_AT["S3"]))
    put("S3", s3)
    for g in s3:
        cache_add(g, 50_000 + g, third_silo(g))
    s4 = remote_grains(len(CASE_AT["S4"]))
    put("S4", s4)
    for g in s4:
        cache_add(g, 10_000 + g, 0)  # my own silo: the handle is in this rank's space [0, n_act)
    s5 = remote_grains(len(CASE_AT["S5"]))
    put("S5", s5)
    for g in s5:
        cache_add(g, 50_000 + g, 6)
    s6 = remote_grains(len(CASE_AT["S6"]))
    put("S6", s6, flags=L.HDR_ADDRESS_COMPLETE, target_silo=5)
    for g in s6:
        cache_add(g, 50_000 + g, third_silo(g))
    # S7: a system target, and a KeyExt-category key whose hash owner is remote; both keys cached
    kx = keyext_tcd(w.cl)
    kx_ids = [i for i in range(7000, 7400)
              if not w.local[int(w.cl.owner_of(np.array([P.jenkins_u64(kx, 0, i)], np.uint32))[0])]][:2]
    s7_keys = [(SYS_TCD, 0, 41), (kx, 0, kx_ids[0]), (SYS_TCD, 0, 42), (kx, 0, kx_ids[1])]
    for i, k in zip(CASE_AT["S7"], s7_keys):
        m["tcd"][i], m["n0"][i], m["n1"][i] = k
        cache_add(k, 50_000 + i, 3)
    # S8: the stopped silo sends, to cached grains it owns while it runs
    s8 = [g for g in w.mine.tolist() if own_of[g] == stopped][:len(CASE_AT["S8"])]
    put("S8", s8, sending_silo=stopped)
    for g in s8:
        cache_add(g, 50_000 + g, 3)
    s9 = remote_grains(1)[0]
    put("S9", [s9] * len(CASE_AT["S9"]))
    cache_add(s9, 50_000 + s9, third_silo(s9))
    hv = remote_grains(len(CASE_AT["HV"]))
    if fmt == 32:
        put("HV", hv, flags=L.HDR_HASH_VALID)
        for i, g in zip(CASE_AT["HV"], hv):
            m["aux"][i] = P.jenkins_u64(*w.kt[g])
    for g in hv:
        cache_add(g, 50_000 + g, third_silo(g))
    reserved = set(s1 + s2 + s3 + s4 + s5 + s6 + s8 + [s9] + hv)
    # background: cached remote grains on any silo (the local ones with a handle of this rank); a third of them cold
    bg = remote_grains(n_background)
    n_special = len(ck)
    for j, g in enumerate(bg):
        silo = int(rng.integers(0, 8))
        cache_add(g, (10_000 if w.local[silo] else 50_000) + g, silo)
    cold = np.arange(n_special, n_special + len(bg))[::3]
    reserved |= set(bg[::3])
    pool = np.array([g for g in range(w.n_grains) if g not in reserved], np.uint64)
    fill = cls == ""
    nf = int(fill.sum())
    m["n1"][fill] = rng.choice(pool, nf)
    m["sending_silo"][fill] = rng.integers(0, 8, nf)
    m["category"][fill] = rng.integers(0, 4, nf)
    done = np.nonzero(fill)[0][::97]
    m["flags"][done] = L.HDR_ADDRESS_COMPLETE
    m["target_silo"][done] = rng.integers(0, 8, len(done))
    # the owner of S8's grains with the stopped silo excluded: the oracle's word for one of them
    probe = m[CASE_AT["S8"][:1]]
    s8_owner = int(w.o.route(probe, L.OPT_EXCLUDE_IF_STOPPING)[0][0] & 0xFF)
    keys = np.zeros(len(ck), L.KEY_DTYPE)
    keys["tcd"], keys["n0"], keys["n1"] = [k[0] for k in ck], [k[1] for k in ck], [k[2] for k in ck]
    assert len(set(ck)) == len(ck)
    at = {k: list(v) for k, v in CASE_AT.items() if k != "HV" or fmt == 32}
    return Case(m, cls, at, L.OPT_EXCLUDE_IF_STOPPING, keys, np.array(ca, np.uint32), np.array(cs, np.uint8), cold, stopped,
                s8_owner)


class NullOwnerWorld:
    """S8's null owner: CalculateTargetSilo returns null only when the excluded sender is the ring's one silo
    (LocalGrainDirectory.cs:483-493).  Silo 0 alone on the ring, stopped; this rank hosts silo 1, so silo 0's partition is
    remote and silo 1's messages to a cached grain are looked up, while silo 0's have no owner at all."""

    def __init__(self):
        from orleans_amd import workloads as W
        self.cl = W.default_cluster()
        self.local = [0, 1, 0, 0, 0, 0, 0, 0]
        self.functional = [1] * 8
        self.running = [0, 1, 1, 1, 1, 1, 1, 1]
        self.ros = np.array([1, 0, 1, 1, 0, 0, 0, 0], np.uint8)
        self.my_rank, self.nranks, self.n_act = 0, 2, 60_000
        self.o = cpu_ref.Oracle(8, running=self.running, functional=self.functional, local=self.local)
        self.o.add_server(0, int(self.cl.hashes[0]))


def null_owner_case(n=130):
    """-> (world, msgs, opts, cache entries [(key, (act, silo))]): message i targets grain i, every grain cached on silo 2;
    even messages come from the stopped silo 0 (owner null: they stay, unaddressed, not looked up), odd ones from silo 1
    (looked up and addressed).  No grain is shared, so the even grains' entries stay unstamped and unaccessed."""
    w = NullOwnerWorld()
    m = np.zeros(n, L.MSG_DTYPE)
    m["tcd"] = grain_tcd(w.cl)
    m["n1"] = np.arange(n)
    m["category"] = 2
    m["sending_silo"] = np.arange(n) % 2
    ent = [((grain_tcd(w.cl), 0, g), (50_000 + g, 2)) for g in range(n)]
    return w, m, L.OPT_EXCLUDE_IF_STOPPING, ent


# ---- the constructed received records -----------------------------------------------------------------------------------

class ReceivingWorld:
    """A receiving rank over a cache_evict_ref.World's population: it holds the partitions of the silos in `local`, every
    grain they own registered with its grain number as handle, on its owner — or, one in five, on silo 5, which stops being
    functional AFTER the registration (a directory entry on a silo the receiver no longer counts as valid: R6)."""

    def __init__(self, world, local=(1, 1, 0, 0, 0, 0, 0, 0)):
        w = self.w = world
        self.local = list(local)
        self.functional_at_registration = list(w.functional)
        self.functional = [f and s != 5 for s, f in enumerate(w.functional)]
        self.functional = [int(f) for f in self.functional]
        self.o = cpu_ref.Oracle(8, functional=self.functional_at_registration, local=self.local)
        for s in range(8):
            self.o.add_server(s, int(w.cl.hashes[s]))
        self.held = np.nonzero(np.asarray(self.local, bool)[w.owner])[0]
        self.acts = self.held.astype(np.uint32)
        self.silos = np.where(self.held % 5 == 0, 5, w.owner[self.held]).astype(np.uint8)
        self.silos[~np.asarray(self.functional_at_registration, bool)[self.silos]] = 7  # no activation on an invalid silo
        st, _, _ = self.o.register(w.keys[self.held], self.acts, self.silos)
        assert (st == L.INS_INSERTED).all()
        self.o.cl.functional[5] = 0
        self.n_act = w.n_act
        # ids past the population that these silos own: no directory entry
        ids = np.arange(w.n_grains, w.n_grains + 4000, dtype=np.uint64)
        t = np.full(len(ids), grain_tcd(w.cl), np.uint64)
        own = w.cl.owner_of(w.W.jenkins3_np(t, np.zeros(len(ids), np.uint64), ids))
        self.unregistered = ids[np.asarray(self.local, bool)[own]]
        self.not_held = np.nonzero(~np.asarray(self.local, bool)[w.owner])[0]


RECV_PATTERN = ["R1", "R2", "R3", "R4", "R5", "R6", "R7", "R7x", "R7f", "R1r", "R7c"]


def receiver_cases(rw, n, seed=2, only_r1=False):
    """-> (headers, lane, cls, receiver cache entries).  Classes cycle through RECV_PATTERN, so every class sits on both
    sides of every tile edge n reaches: R1 lane NO_ACT on a held grain, R1r the same on a grain held elsewhere, R2
    confirmed, R3 another handle, R4 the same handle on another silo, R5 no directory entry, R6 the entry's silo not
    functional, R7 not held (valid target silo), R7x the same with the target silo the sender's own (LOOPBACK), R7f with
    the target silo not functional here, R7c a grain the receiver's OWN cache holds with a different entry."""
    w = rw.w
    rng = np.random.default_rng(seed)
    cls = np.array([RECV_PATTERN[i % len(RECV_PATTERN)] for i in range(n)])
    if only_r1:
        cls = np.where(np.arange(n) % 2 == 0, "R1", "R1r")
    m = np.zeros(n, L.MSG_DTYPE)
    m["tcd"] = grain_tcd(w.cl)
    m["category"] = 2
    m["sending_silo"] = rng.integers(2, 8, n)  # the senders are other ranks' silos
    lane = np.full(n, NO_ACT, np.uint32)
    ok_held = rw.held[rw.silos != 5]   # entries on a functional silo
    off_held = rw.held[rw.silos == 5]  # entries on the silo that stopped being functional
    cache = {}
    for i in range(n):
        c = cls[i]
        if c in ("R1", "R2", "R3", "R4"):
            g = int(rng.choice(ok_held))
            m["n1"][i] = g
            host = int(w.owner[g])
            if c == "R2":
                lane[i], m["target_silo"][i] = g, host
            elif c == "R3":
                lane[i], m["target_silo"][i] = g + 1, host
            elif c == "R4":
                lane[i], m["target_silo"][i] = g, 3 if host != 3 else 4
        elif c == "R5":
            m["n1"][i] = int(rng.choice(rw.unregistered))
            lane[i], m["target_silo"][i] = 50_000 + i, 3
        elif c == "R6":
            g = int(rng.choice(off_held))
            m["n1"][i] = g
            lane[i], m["target_silo"][i] = g, 5
        else:  # the partition is held elsewhere
            g = int(rng.choice(rw.not_held))
            m["n1"][i] = g
            if c == "R1r":
                continue
            lane[i] = 50_000 + i
            m["target_silo"][i] = {"R7": 3, "R7c": 4, "R7x": int(m["sending_silo"][i]), "R7f": 6}[c]
            if c == "R7x" and not rw.functional[m["target_silo"][i]]:
                m["sending_silo"][i] = m["target_silo"][i] = 7
            if c == "R7c":
                cache[w.kt[g]] = (40_000 + g % 1000, 2)
    taken = {w.kt[int(g)] for g in m["n1"][cls != "R7c"].tolist() if g < w.n_grains}
    cache = {k: v for k, v in cache.items() if k not in taken}  # an R7c grain is no other record's target
    return m, lane, cls, cache
