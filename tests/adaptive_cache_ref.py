"""The reference's adaptive directory cache and its maintainer restated in Python over oracle/pyref.LRUCache (test
infrastructure, like cache_evict_ref.py): what orleans_amd/csrc/cache_adaptive.hip and the adaptive state of the update,
eviction and rebuild kernels must compute.  Paths are relative to the reference's src/.

  AdaptiveCache                        OrleansRuntime/GrainDirectory/AdaptiveGrainDirectoryCache.cs
  maintainer_run                       AdaptiveDirectoryCacheMaintainer.Run's loop, AdaptiveDirectoryCacheMaintainer.cs:54-143
  build_grain_and_etag_list            BuildGrainAndETagList, :216-238
  process_cache_refresh_response       ProcessCacheRefreshResponse, :167-207
  adjust_local_cache                   LocalGrainDirectory.AdjustLocalCache, LocalGrainDirectory.cs:330-344

DateTime.UtcNow is the `now` argument (.NET ticks); CalculateTargetSilo and owner.Equals(MyAddress) are injected
(owner_of(key) -> silo or None, is_local(silo)).  The reference walks a ConcurrentDictionary, whose enumeration order is
unspecified, so the walks take the order as an argument."""
from __future__ import annotations

from oracle import pyref as P

NO_ETAG = -1  # GrainInfo.NO_ETAG
TICKS_PER_SECOND = 10_000_000
DEFAULT_INITIAL, DEFAULT_MAX, DEFAULT_GROWTH = 30 * TICKS_PER_SECOND, 240 * TICKS_PER_SECOND, 2.0  # GlobalConfiguration.cs:413-417


def multiply(ticks: int, value: float) -> int:
    """TimeSpan.Multiply (Orleans/Utils/StandardExtensions.cs:34-39): checked((long)checked((double)ticks * value)) — the
    conversion to double rounds to nearest, one IEEE multiply, the conversion back truncates toward zero."""
    out = int(float(ticks) * value)
    assert -(1 << 63) <= out < (1 << 63), "checked((long)...) would throw"
    return out


class Entry:
    """GrainDirectoryCacheEntry (AdaptiveGrainDirectoryCache.cs:32-70)."""

    def __init__(self, value, etag, now, expiration_timer):  # the constructor, :50-58
        self.value, self.etag, self.expiration_timer = value, etag, expiration_timer
        self.last_refreshed = now
        self.num_accesses = 0

    def is_expired(self, now) -> bool:  # :60-63: UtcNow >= LastRefreshed.Add(ExpirationTimer)
        return now >= self.last_refreshed + self.expiration_timer

    def refresh(self, now, new_expiration_timer):  # :65-69
        self.last_refreshed = now
        self.expiration_timer = new_expiration_timer


class CountingLRU(P.LRUCache):
    """pyref.LRUCache that counts the entries AdjustSize frees (LRU.cs:188-205)."""

    def __init__(self, m):
        super().__init__(m)
        self.victims = 0

    def add(self, key, value):
        while len(self.d) >= self.max:
            self.gen_free += 1
            victim = self.by_gen.pop(self.gen_free, None)
            if victim is not None:
                del self.d[victim]
                self.victims += 1
        super().add(key, value)  # Count < MaximumSize now: its own AdjustSize loop does not run


class AdaptiveCache:
    """AdaptiveGrainDirectoryCache over LRU<GrainId, GrainDirectoryCacheEntry> (:72-95).  self.lru.d: key -> [Entry, gen]."""

    def __init__(self, max_size, initial=DEFAULT_INITIAL, max_timer=DEFAULT_MAX, growth=DEFAULT_GROWTH):
        self.lru = CountingLRU(max_size)
        self.initial, self.max_timer, self.growth = initial, max_timer, growth

    def add_or_update(self, key, value, version, now):  # :97-103
        self.lru.add(key, Entry(value, version, now, self.initial))

    def remove(self, key) -> bool:  # :105-109
        return self.lru.remove(key)

    def look_up(self, key):  # :116-133: TryGetValue (an LRU generation), then NumAccesses++
        e = self.lru.try_get(key)
        if e is None:
            return None
        e.num_accesses += 1
        return e.value, e.etag

    def try_get(self, key):
        """The shape pyref.apply_directory_cache_lru asks its cache for: LookUp's value, or None."""
        r = self.look_up(key)
        return None if r is None else r[0]

    def key_values(self):  # :135-148: no LRU generation, no access
        return [(k, v[0].value, v[0].etag) for k, v in self.lru.d.items()]

    def mark_as_fresh(self, key, now) -> bool:  # :150-159
        e = self.lru.try_get(key)
        if e is None:
            return False
        e.refresh(now, min(self.max_timer, multiply(e.expiration_timer, self.growth)))  # StandardExtensions.Min, :60-63
        return True

    def get(self, key):  # :161-164 → LRU.Get (LRU.cs:176-183) = TryGetValue: a generation, no NumAccesses
        return self.lru.try_get(key)

    # what the tests compare the device with
    def entry(self, key):
        v = self.lru.d.get(key)
        return None if v is None else v[0]

    def __len__(self):
        return len(self.lru.d)

    def lru_order(self):
        """Keys from least to most recently used."""
        return [k for k, _ in sorted(self.lru.d.items(), key=lambda kv: kv[1][1])]


def maintainer_run(cache: AdaptiveCache, order, owner_of, is_local, now):
    """One iteration of Run's loop over the entries in `order` (Maintainer.cs:77-131).  Returns (fetch, counts):
    fetch = {owner: [grain, ...]} in insertion order (fetchInBatchList) and counts = [cnt1, cnt2, cnt3, cnt4, skipped]."""
    fetch, cnt = {}, [0, 0, 0, 0, 0]
    for grain in order:
        entry = cache.entry(grain)
        owner = owner_of(grain)                      # :85
        if owner is None:                            # :86-89
            cnt[4] += 1
            continue
        if is_local(owner):                          # :91-98
            cache.remove(grain)
            cnt[0] += 1
        elif entry is None:                          # :101-106 (deleted in parallel: not reachable from a fixed order)
            cache.remove(grain)
            cnt[2] += 1
        elif not entry.is_expired(now):              # :107-111
            cnt[1] += 1
        elif entry.num_accesses == 0:                # :112-117
            cache.remove(grain)
            cnt[2] += 1
        else:                                        # :118-129
            fetch.setdefault(owner, []).append(grain)
            entry.num_accesses = 0
            cnt[3] += 1
    return fetch, cnt


def build_grain_and_etag_list(cache: AdaptiveCache, grains):
    """:216-238: cache.Get per grain — it takes an LRU generation and leaves NumAccesses alone."""
    out = []
    for grain in grains:
        entry = cache.get(grain)
        if entry is not None:
            out.append((grain, entry.etag))
    return out


def process_cache_refresh_response(cache: AdaptiveCache, response, now):
    """:167-207.  response: (grain, etag, value or None) tuples.  Returns [updated, removed, unchanged]."""
    cnt = [0, 0, 0]
    for grain, etag, value in response:
        if value is not None:                        # :181-186
            cache.add_or_update(grain, value, etag, now)
            cnt[0] += 1
        elif etag == NO_ETAG:                        # :187-194
            cache.remove(grain)
            cnt[1] += 1
        else:                                        # :195-204
            cache.mark_as_fresh(grain, now)
            cnt[2] += 1
    return cnt


def response_runs(response):
    """The host composition of a response for the device: maximal runs of one kind, in order — ('add' | 'remove' | 'fresh',
    [tuples])."""
    runs = []
    for t in response:
        kind = "add" if t[2] is not None else "remove" if t[1] == NO_ETAG else "fresh"
        if runs and runs[-1][0] == kind:
            runs[-1][1].append(t)
        else:
            runs.append((kind, [t]))
    return runs


def adjust_local_cache(cache: AdaptiveCache, removed_silo, owner_of, is_local) -> int:
    """LocalGrainDirectory.cs:330-344 over KeyValues, after the ring change.  Values are single activations (act, silo), so
    RemoveActivations (:959-977) with a match always ends in Remove.  Returns the number of entries removed."""
    removed = 0
    for grain, value, _etag in cache.key_values():
        gone = False
        owner = owner_of(grain)
        if owner is not None and is_local(owner):    # 2) now owned by me, :335-339
            gone = cache.remove(grain) or gone
        if value[1] == removed_silo:                 # 1) the activation sat on the removed silo, :341-342
            gone = cache.remove(grain) or gone
        removed += gone
    return removed
