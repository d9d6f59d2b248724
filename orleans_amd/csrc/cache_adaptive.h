// cache_adaptive.h — the adaptive directory cache's maintainer on the device (cache_adaptive.hip), as orl_api.cpp calls
// it.  Nothing here is part of the public ABI.
#pragma once

#include "orl_internal.h"

namespace orl {

constexpr uint32_t kSweepTile = 2048;  // slots per sweep tile (256 threads x 8)

// Scratch and output of one context's sweeps, allocated once by orl_cache_config_adaptive (sized by the capacity and the
// slot count): a sweep allocates nothing and its output cannot overflow (it emits at most `capacity` entries).
// One device allocation (`base`) carved into the arrays below.
struct CacheSweepScratch {
    void* base = nullptr;
    uint64_t slots = 0, capacity = 0;
    uint32_t ntiles = 0;            // ceil(slots / kSweepTile)
    uint16_t* cls = nullptr;        // [slots] the sweep's verdict per slot: class << 8 | owner
    uint32_t* tile_cnt = nullptr;   // [256 * ntiles] owner-major (owner * ntiles + tile): emitted counts, then offsets
    orl_grain_key* keys = nullptr;  // [capacity] the refresh lists, owner-major
    int32_t* etags = nullptr;       // [capacity]
    uint32_t* owner_off = nullptr;  // [257] list of owner o = [owner_off[o], owner_off[o + 1])
    uint64_t* counts = nullptr;     // [8] {self-owned removed, kept, expired removed, to refresh, owner null}
};

// hipError_t as int (0 = ok).
int cache_sweep_alloc(CacheSweepScratch* s, uint64_t capacity, uint64_t slots);
void cache_sweep_free(CacheSweepScratch* s);

// AdaptiveDirectoryCacheMaintainer.Run's walk (AdaptiveDirectoryCacheMaintainer.cs:77-131) and BuildGrainAndETagList's
// Gets (:216-238) over the whole table, stream-ordered: classify + count per (owner, tile), scan, apply + emit.  me, excl:
// CalculateTargetSilo's caller and excludeThisSiloIfStopping.  d_cnt = the cache's {entries, tombstones, ...}.
int launch_cache_sweep(const RouteParams* d_params, DirSlot* d_cache, uint64_t mask, uint64_t* d_cnt, uint32_t me, bool excl,
                       uint32_t n_silos, int64_t now, const CacheSweepScratch& s, void* stream);

// LocalGrainDirectory.AdjustLocalCache (LocalGrainDirectory.cs:330-344) after the ring change: the same walk and owner
// computation; entries whose owner's partition is local or whose activation sits on `removed_silo` are tombstoned.
// d_removed (optional): their count.  Works on a plain cache too (no adaptive state is read).
int launch_cache_adjust(const RouteParams* d_params, DirSlot* d_cache, uint64_t mask, uint64_t* d_cnt, uint32_t me, bool excl,
                        uint32_t n_silos, uint32_t removed_silo, uint64_t* d_removed, void* stream);

// AdaptiveGrainDirectoryCache.MarkAsFresh (AdaptiveGrainDirectoryCache.cs:150-159) per key (distinct within the batch);
// G advances by n.  d_found optional.
int launch_cache_mark_fresh(DirSlot* d_cache, uint64_t mask, const orl_grain_key* d_keys, size_t n, int64_t now, int64_t max_ttl,
                            double growth, uint8_t* d_found, void* stream);

#ifdef __HIPCC__
// MarkAsFresh's change to a found entry (slot s of an adaptive table), shared by k_mark_fresh and the refresh apply
// (cache_evict.hip k_ra_apply): TryGetValue takes the generation `stamp` — NumAccesses untouched, so `seen` follows the
// stamp of an unaccessed entry — ExpirationTimer = Min(max, ExpirationTimer.Multiply(growth)) =
// (long)((double)ticks * growth) (StandardExtensions.cs:34-39), LastRefreshed = now.
__device__ __forceinline__ void cache_mark_fresh_slot(const DirSlot* cache, uint64_t mask, uint64_t s, unsigned long long stamp,
                                                      int64_t now, int64_t max_ttl, double growth) {
    const CacheAdaptive a = cache_adaptive(cache, mask);
    unsigned long long* gen = reinterpret_cast<unsigned long long*>(const_cast<DirSlot*>(cache + mask + 1));
    if (gen[s] == a.seen[s]) a.seen[s] = stamp;
    gen[s] = stamp;
    const int64_t grown = (int64_t)__dmul_rn(__ll2double_rn((long long)a.ttl[s]), growth);
    a.ttl[s] = max_ttl < grown ? max_ttl : grown;
    a.last_refreshed[s] = now;
}
#endif

// A lookup that stamps nothing.  Every output optional; the last four need an adaptive table (adaptive = true).
int launch_cache_peek(const DirSlot* d_cache, uint64_t mask, bool adaptive, const orl_grain_key* d_keys, size_t n, uint32_t* d_act,
                      uint8_t* d_silo, int32_t* d_etag, int64_t* d_ttl, int64_t* d_last_refreshed, uint8_t* d_accessed,
                      void* stream);

}  // namespace orl
