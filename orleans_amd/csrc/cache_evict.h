// cache_evict.h — the directory cache's device-side LRU eviction and tombstone compaction (cache_evict.hip), as
// orl_api.cpp calls them.  Nothing here is part of the public ABI.
#pragma once

#include "orl_internal.h"

namespace orl {

// Scratch of one context's cache, allocated once by orl_cache_config (sized by max_batch and the slot count): the hot
// path allocates nothing.  One device allocation (`base`) carved into the arrays below.
struct CacheEvictScratch {
    void* base = nullptr;
    uint64_t max_batch = 0, slots = 0;
    uint32_t group_mask = 0;     // the batch-local claim table has group_mask + 1 >= 2 * max_batch entries
    uint32_t ntiles = 0;         // ceil(slots / kEvTile)
    // per batch entry [max_batch]
    uint32_t* old_slot = nullptr;   // the key's FULL slot before the batch, or none
    uint64_t* gkey = nullptr;       // (group << 32 | index), ~0 for an invalid entry; and its sorted copy
    uint64_t* gkey_sorted = nullptr;
    uint32_t* prev_b = nullptr;     // latest earlier valid entry of the same key
    uint32_t* nxt_b = nullptr;      // first later valid entry of the same key (the queue's nxt of a batch entry)
    uint32_t* prevpos = nullptr;    // queue position of the key's latest earlier occurrence
    uint8_t* ev_b = nullptr;        // the serial pass evicted this batch entry
    uint8_t* keep = nullptr;        // last occurrence of its key and not evicted: inserted / updated
    uint32_t* group_tab = nullptr;  // [group_mask + 1] claim table: one entry index per distinct key
    // per entry of a refresh response [max_batch] (launch_cache_apply_refresh)
    uint32_t* grp_b = nullptr;      // the key's claim-table slot
    uint32_t* live_b = nullptr;     // the serial pass left this batch element in the queue (an ADD, a FRESH that found its key)
    uint8_t* op_b = nullptr;        // the entry's operation: ignore / ADD / REMOVE / FRESH
    uint8_t* present_b = nullptr;   // the serial pass found the entry's key in the cache at its turn
    // per candidate [min(2 * max_batch, slots)]
    uint64_t* cand_stamp = nullptr;
    uint64_t* cand_stamp_s = nullptr;  // sorted ascending (stable: ties by slot index)
    uint32_t* cand_slot = nullptr;
    uint32_t* cand_slot_s = nullptr;
    uint32_t* nxt_c = nullptr;      // first valid batch entry with the candidate's key
    uint8_t* ev_c = nullptr;        // the serial pass evicted this candidate
    // per cache slot [slots]
    uint64_t* skey = nullptr;       // FULL ? stamp : ~0
    uint32_t* slotpos = nullptr;    // slot -> candidate position (none outside a batch)
    uint32_t* tile_cnt = nullptr;   // [ntiles] compaction counts / offsets
    uint64_t* st = nullptr;         // [16] {n_valid, K, threshold, rank, ncand, final count, evicted, rebuilt}
    uint32_t* hist = nullptr;       // [256] radix-select digit counts
    void* sort_temp = nullptr;
    size_t sort_temp_bytes = 0;
};

// hipError_t as int (0 = ok).
int cache_evict_alloc(CacheEvictScratch* s, uint64_t max_batch, uint64_t slots);
void cache_evict_free(CacheEvictScratch* s);

// The exact sequential LRU.Add of a batch, stream-ordered (DESIGN "Directory cache: eviction on the device").
// d_cache_ins: the table the surviving entries are inserted into — d_cache, or the second table when the caller
// asked for a compaction between the tombstoning and the inserts (`d_rebuild_into` != nullptr, same geometry).
// d_cnt = {entries, tombstones, error word, cumulative evictions}.  fresh: the adaptive state of the entries the batch
// leaves (fresh.on == 0: a plain cache).
int launch_cache_evict_add(DirSlot* d_cache, uint64_t mask, DirSlot* d_rebuild_into, uint64_t* d_cnt, uint64_t capacity,
                           const orl_grain_key* d_keys, const uint32_t* d_acts, const uint8_t* d_silos, size_t n,
                           uint32_t n_act, uint32_t n_silos, const uint32_t* d_local, const CacheEvictScratch& s, void* stream,
                           const CacheFresh& fresh = CacheFresh{});

// ProcessCacheRefreshResponse (AdaptiveDirectoryCacheMaintainer.cs:167-207) over a whole response, stream-ordered: per
// entry AddOrUpdate, Remove or MarkAsFresh by d_kind[i] (an ORL_LUM_* value), exactly the sequential loop.
// may_evict: the host's bounds allow an eviction, so the candidate selection and the serial pass are enqueued (each
// leaves at once when the response holds no valid ADD); otherwise the data-parallel apply alone.  fresh: as for the add,
// on an adaptive table (fresh.on != 0 is required).  d_present [n] and d_counts [4] optional.
struct CacheRefresh {
    const uint8_t* kind = nullptr;
    int64_t max_ttl = 0;   // MarkAsFresh: ExpirationTimer = min(max_ttl, (int64)((double)timer * growth))
    double growth = 0;
    uint8_t* present = nullptr;
    uint64_t* counts = nullptr;
};
int launch_cache_apply_refresh(DirSlot* d_cache, uint64_t mask, DirSlot* d_rebuild_into, uint64_t* d_cnt, uint64_t capacity,
                               const orl_grain_key* d_keys, const uint32_t* d_acts, const uint8_t* d_silos, size_t n,
                               uint32_t n_act, uint32_t n_silos, const uint32_t* d_local, const CacheEvictScratch& s,
                               void* stream, const CacheFresh& fresh, const CacheRefresh& refresh, bool may_evict);

// Tombstone compaction alone: the FULL slots of d_src, with their stamps and the generation base, rehashed into d_dst
// (same geometry, no tombstones); the counters reset to {entries, 0}.  adaptive: both tables carry the per-slot adaptive
// state (orl_internal.h CacheAdaptive), which moves with its entry.
int launch_cache_rebuild(const DirSlot* d_src, DirSlot* d_dst, uint64_t mask, uint64_t* d_cnt, const CacheEvictScratch& s,
                         void* stream, bool adaptive = false);

}  // namespace orl
