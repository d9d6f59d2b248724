// api_cache.cpp — the directory cache (AdaptiveGrainDirectoryCache, f4) on the host side: everything orl_cache_*.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <tuple>
#include <vector>

#include "orl_ctx.h"
#include "cache_adaptive.h"
#include "cache_evict.h"

namespace {

void set_cache_on(orl_ctx* c, bool on) {
    if (c->hp.cache_on != (on ? 1u : 0u)) {
        c->hp.cache_on = on ? 1u : 0u;
        c->params_dirty = true;
    }
}

int cache_config(orl_ctx* c, uint64_t capacity, bool adaptive) {
    if (int r = need_device(c)) return r;
    if (capacity == 0) return fail(c, ORL_E_INVALID, "capacity must be >= 1");
    ORL_HIP(c, hipSetDevice(c->cfg.device));
    ORL_HIP(c, hipDeviceSynchronize());
    (void)hipFree(c->d_cache); (void)hipFree(c->d_cache2); (void)hipFree(c->d_cclaim); (void)hipFree(c->d_cstate);
    c->d_cache = nullptr; c->d_cache2 = nullptr; c->d_cclaim = nullptr; c->d_cstate = nullptr;
    cache_evict_free(&c->cev);
    cache_sweep_free(&c->csw);
    c->cache_slots = 0;
    c->cache_adaptive = false;
    const uint64_t slots = next_pow2(2 * capacity);
    // the table, then one u64 LRU generation per slot and the generation base (dir_table_dev.h cache_gens), then, in
    // adaptive mode, the per-slot adaptive state (orl_internal.h CacheAdaptive)
    const size_t bytes = cache_table_bytes(slots, adaptive);
    ORL_HIP(c, hipMalloc((void**)&c->d_cache, bytes));
    ORL_HIP(c, hipMalloc((void**)&c->d_cache2, bytes));
    ORL_HIP(c, hipMemset(c->d_cache2, 0, bytes));
    if (int e = cache_evict_alloc(&c->cev, c->s.max_batch, slots)) return hipfail(c, (hipError_t)e, "cache eviction scratch");
    if (adaptive)
        if (int e = cache_sweep_alloc(&c->csw, capacity, slots)) return hipfail(c, (hipError_t)e, "cache sweep scratch");
    ORL_HIP(c, hipMalloc((void**)&c->d_cclaim, slots * 4));
    ORL_HIP(c, hipMalloc((void**)&c->d_cstate, 32));
    ORL_HIP(c, hipMemset(c->d_cache, 0, bytes));
    ORL_HIP(c, hipMemset(c->d_cclaim, 0xFF, slots * 4));
    ORL_HIP(c, hipMemset(c->d_cstate, 0, 32));
    c->cache_slots = slots;
    c->cache_cap = capacity;
    c->cache_gen_free = 0;
    c->cache_ub = c->cache_tombs_ub = 0;
    c->cache_host_evictions = c->cache_evict_batches = c->cache_rebuilds = c->cache_host_fallbacks = 0;
    c->cache_adaptive = adaptive;
    set_cache_on(c, false);
    return ORL_OK;
}

// AddOrUpdate of a batch that can overflow the capacity: the reference's sequential LRU on the host, exactly
// (AdaptiveGrainDirectoryCache.AddOrUpdate → LRU.Add: AdjustSize — while Count >= MaximumSize free the entry of the next
// generation, LRU.cs:188-205 — then AddOrUpdate with the next generation, :104-108), over the device table read back, then
// the table rebuilt and uploaded (no tombstones).  Entries the device path would not keep (an invalid silo, a handle
// outside this context's space on a local silo: k_cache_probe) are skipped as there.  Generations stay the device's
// sparse stamps (only their order matters); G advances by n as on the fast path.
int cache_add_host_lru(orl_ctx* c, const orl_grain_key* d_keys, const uint32_t* d_acts, const uint8_t* d_silos, size_t n) {
    const uint64_t slots = c->cache_slots, mask = slots - 1;
    ORL_HIP(c, hipDeviceSynchronize());
    std::vector<DirSlot> tab(slots);
    std::vector<uint64_t> gen(slots + 1);
    ORL_HIP(c, hipMemcpy(tab.data(), c->d_cache, slots * sizeof(DirSlot), hipMemcpyDeviceToHost));
    ORL_HIP(c, hipMemcpy(gen.data(), reinterpret_cast<uint8_t*>(c->d_cache) + slots * sizeof(DirSlot), (slots + 1) * 8,
                         hipMemcpyDeviceToHost));
    std::vector<orl_grain_key> keys(n);
    std::vector<uint32_t> acts(n);
    std::vector<uint8_t> silos(n);
    if (n) {
        ORL_HIP(c, hipMemcpy(keys.data(), d_keys, n * sizeof(orl_grain_key), hipMemcpyDeviceToHost));
        ORL_HIP(c, hipMemcpy(acts.data(), d_acts, n * 4, hipMemcpyDeviceToHost));
        ORL_HIP(c, hipMemcpy(silos.data(), d_silos, n, hipMemcpyDeviceToHost));
    }
    struct Ent {
        orl_grain_key k;
        uint32_t act;
        uint8_t silo;
        uint64_t gen;
    };
    auto kk = [](const orl_grain_key& k) { return std::make_tuple(k.type_code_data, k.n0, k.n1); };
    std::map<std::tuple<uint64_t, uint64_t, uint64_t>, Ent> ents;  // the cache
    std::map<uint64_t, std::tuple<uint64_t, uint64_t, uint64_t>> by_gen;  // LRU order
    for (uint64_t i = 0; i < slots; ++i)
        if (tab[i].state == SLOT_FULL) {
            const orl_grain_key k{tab[i].tcd, tab[i].n0, tab[i].n1};
            ents[kk(k)] = Ent{k, tab[i].act, tab[i].silo, gen[i]};
            by_gen[gen[i]] = kk(k);
        }
    const uint64_t G = gen[slots];
    for (size_t i = 0; i < n; ++i) {
        const uint32_t sl = silos[i];
        if (!(sl < c->n_silos && (acts[i] < c->cfg.n_act || (acts[i] != ORL_NO_ACT && !c->local[sl])))) continue;
        while (ents.size() >= c->cache_cap && !by_gen.empty()) {  // AdjustSize
            auto v = by_gen.begin();
            c->cache_gen_free = v->first;
            ++c->cache_host_evictions;
            ents.erase(v->second);
            by_gen.erase(v);
        }
        const auto key = kk(keys[i]);
        const uint64_t g = G + i + 1;
        auto it = ents.find(key);
        if (it != ents.end()) {
            by_gen.erase(it->second.gen);
            it->second = Ent{keys[i], acts[i], (uint8_t)sl, g};
        } else {
            ents[key] = Ent{keys[i], acts[i], (uint8_t)sl, g};
        }
        by_gen[g] = key;
    }
    std::fill(tab.begin(), tab.end(), DirSlot{});
    std::fill(gen.begin(), gen.end() - 1, 0ull);
    gen[slots] = G + n;
    for (const auto& kv : ents) {
        const Ent& e = kv.second;
        uint64_t i = dir_slot(jenkins3(e.k.type_code_data, e.k.n0, e.k.n1), mask);
        while (tab[i].state != SLOT_EMPTY) i = (i + 1) & mask;
        tab[i].tcd = e.k.type_code_data; tab[i].n0 = e.k.n0; tab[i].n1 = e.k.n1;
        tab[i].act = e.act; tab[i].silo = e.silo; tab[i].state = SLOT_FULL;
        gen[i] = e.gen;
    }
    ORL_HIP(c, hipMemcpy(c->d_cache, tab.data(), slots * sizeof(DirSlot), hipMemcpyHostToDevice));
    ORL_HIP(c, hipMemcpy(reinterpret_cast<uint8_t*>(c->d_cache) + slots * sizeof(DirSlot), gen.data(), (slots + 1) * 8,
                         hipMemcpyHostToDevice));
    const uint64_t stw[3] = {ents.size(), 0, 0};
    ORL_HIP(c, hipMemcpy(c->d_cstate, stw, sizeof stw, hipMemcpyHostToDevice));
    c->cache_ub = ents.size();
    c->cache_tombs_ub = 0;
    return ORL_OK;
}

// LRU.Add per entry in batch order, on the caller's stream.  No entry can be evicted while the cache holds <= capacity - n
// entries before the batch (every add then finds Count < MaximumSize): the plain update (the batch's last writer of a key
// wins, its generation stamped).  When the host's upper bounds say an eviction is possible, the exact sequential LRU as one
// preparation, one serial pass and one apply on the device (cache_evict.hip); when they say the table's load (entries +
// tombstones + new entries) could pass 7/8, a tombstone compaction into the second table first — between the tombstoning
// and the inserts of an evicting batch, so that even a batch larger than the cache ends with load <= 1/2.  No device-wide
// sync, no copy to the host.  ORL_CACHE_EVICT_HOST keeps the earlier path (exact counters read back, then the LRU on the
// host) for A/B runs and as the tests' cross-check.
// On an adaptive cache every entry the batch leaves is a new GrainDirectoryCacheEntry (AdaptiveGrainDirectoryCache.cs:
// 97-103): d_etags[i] (0 when null), the initial timer, LastRefreshed = the context's `cache_now`, NumAccesses = 0.
int cache_add(orl_ctx* c, const orl_grain_key* d_keys, const uint32_t* d_acts, const uint8_t* d_silos, const int32_t* d_etags,
              size_t n, void* stream) {
    if (!c->cache_slots) return fail(c, ORL_E_STATE, "directory cache not configured (orl_cache_config)");
    CacheFresh fresh;
    if (c->cache_adaptive) {
        fresh.etags = d_etags;
        fresh.now = c->cache_now;
        fresh.initial_ttl = c->cache_initial_ttl;
        fresh.on = 1;
    }
    if (n && (!d_keys || !d_acts || !d_silos)) return fail(c, ORL_E_INVALID, "null device buffer");
    if (int r = check_batch(c, n)) return r;
    auto fits = [&](uint64_t cnt, uint64_t tombs) {  // no eviction possible, and the table's load stays <= 7/8
        return cnt + n <= c->cache_cap && (cnt + tombs + n) * 8 <= c->cache_slots * 7;
    };
    int r = sync_device_state(c);
    if (r) return r;
    set_cache_on(c, true);
    if ((r = sync_device_state(c))) return r;
    hipStream_t st = stream_of(c, stream);
    const uint64_t mask = c->cache_slots - 1;
    if (!fits(c->cache_ub, c->cache_tombs_ub)) {
        if (c->cache_mode == ORL_CACHE_EVICT_HOST) {  // exact counters (a sync), then the host LRU if still needed
            ORL_HIP(c, hipDeviceSynchronize());
            uint64_t stw[3];
            ORL_HIP(c, hipMemcpy(stw, c->d_cstate, sizeof stw, hipMemcpyDeviceToHost));
            c->cache_ub = stw[0];
            c->cache_tombs_ub = stw[1];
            if (!fits(c->cache_ub, c->cache_tombs_ub)) {
                ++c->cache_host_fallbacks;
                return cache_add_host_lru(c, d_keys, d_acts, d_silos, n);
            }
        } else {
            if (n == 0) return ORL_OK;
            const uint64_t fresh_ub = std::min<uint64_t>(n, c->cache_cap);  // the batch leaves at most capacity entries
            const bool evicts = c->cache_ub + n > c->cache_cap;
            const bool crowded = (c->cache_ub + c->cache_tombs_ub + (evicts ? fresh_ub : n)) * 8 > c->cache_slots * 7;
            if (evicts) {
                int e = launch_cache_evict_add(c->d_cache, mask, crowded ? c->d_cache2 : nullptr, c->d_cstate, c->cache_cap, d_keys,
                                               d_acts, d_silos, n, c->cfg.n_act, c->n_silos, c->d_params->local, c->cev, st, fresh);
                if (e) return hipfail(c, (hipError_t)e, "cache eviction launch");
                ++c->cache_evict_batches;
                // FULL + TOMB slots grow by at most the new entries (an eviction turns a FULL slot into a tombstone)
                const uint64_t occupied = c->cache_ub + c->cache_tombs_ub + fresh_ub;
                c->cache_ub = std::min(c->cache_ub + n, c->cache_cap);
                c->cache_tombs_ub = occupied > c->cache_ub ? occupied - c->cache_ub : 0;
                if (crowded) {  // compacted after the tombstoning: what is left is the batch's result, no tombstones
                    std::swap(c->d_cache, c->d_cache2);
                    ++c->cache_rebuilds;
                    c->cache_tombs_ub = 0;
                }
                return ORL_OK;
            }
            // no eviction possible, only tombstones in the way: compact, then the plain update below
            int e = launch_cache_rebuild(c->d_cache, c->d_cache2, mask, c->d_cstate, c->cev, st, c->cache_adaptive);
            if (e) return hipfail(c, (hipError_t)e, "cache rebuild launch");
            std::swap(c->d_cache, c->d_cache2);
            ++c->cache_rebuilds;
            c->cache_tombs_ub = 0;
        }
    }
    int e = launch_cache_update(c->d_cache, mask, c->d_cclaim, c->d_cstate, d_keys, d_acts, d_silos, n, c->cfg.n_act,
                                c->n_silos, c->d_dslot, c->d_dflag, reinterpret_cast<uint32_t*>(c->d_cstate + 2), st, c->d_params,
                                fresh);
    if (e) return hipfail(c, (hipError_t)e, "cache update launch");
    c->cache_ub += n;
    return ORL_OK;
}

// The adaptive calls' common refusals.
int need_adaptive(orl_ctx* c) {
    if (int r = need_device(c)) return r;
    if (!c->cache_slots || !c->cache_adaptive)
        return fail(c, ORL_E_STATE, "directory cache not configured in adaptive mode (orl_cache_config_adaptive)");
    return ORL_OK;
}

}  // namespace

extern "C" {

int orl_cache_config(orl_ctx* c, uint64_t capacity) {
    if (!c) return ORL_E_INVALID;
    return cache_config(c, capacity, false);
}

int orl_cache_config_adaptive(orl_ctx* c, uint64_t capacity, int64_t initial_ttl_ticks, int64_t max_ttl_ticks, double ttl_growth) {
    if (!c) return ORL_E_INVALID;
    if (int r = need_device(c)) return r;
    // what keeps the reference's checked arithmetic from throwing: LastRefreshed.Add(ExpirationTimer) and
    // ExpirationTimer.Multiply(growth) = checked((long)checked((double)ticks * growth)) (StandardExtensions.cs:34-39)
    if (initial_ttl_ticks < 0 || initial_ttl_ticks > max_ttl_ticks || max_ttl_ticks > ((int64_t)1 << 61))
        return fail(c, ORL_E_INVALID, "timers must satisfy 0 <= initial <= max <= 2^61 ticks");
    if (!std::isfinite(ttl_growth) || ttl_growth < 0 || !((double)max_ttl_ticks * ttl_growth < 9223372036854775808.0))
        return fail(c, ORL_E_INVALID, "growth must be finite, >= 0 and keep max * growth below 2^63");
    if (int r = cache_config(c, capacity, true)) return r;
    c->cache_initial_ttl = initial_ttl_ticks;
    c->cache_max_ttl = max_ttl_ticks;
    c->cache_growth = ttl_growth;
    c->cache_now = 0;
    c->cache_mode = ORL_CACHE_EVICT_DEVICE;  // the host LRU does not carry the adaptive state
    return ORL_OK;
}

int orl_cache_clear(orl_ctx* c) {  // LRU.Clear: the entries go, the generation counters run on
    if (!c) return ORL_E_INVALID;
    if (!c->cache_slots) return ORL_OK;
    ORL_HIP(c, hipDeviceSynchronize());
    ORL_HIP(c, hipMemset(c->d_cache, 0, c->cache_slots * sizeof(DirSlot)));
    ORL_HIP(c, hipMemset(c->d_cstate, 0, 24));  // the cumulative eviction count runs on
    c->cache_ub = c->cache_tombs_ub = 0;
    set_cache_on(c, false);
    return ORL_OK;
}

int orl_cache_add_or_update_device(orl_ctx* c, const orl_grain_key* d_keys, const uint32_t* d_acts, const uint8_t* d_silos,
                                   size_t n, void* stream) {
    if (!c) return ORL_E_INVALID;
    return cache_add(c, d_keys, d_acts, d_silos, nullptr, n, stream);
}

int orl_cache_add_or_update_versioned_device(orl_ctx* c, const orl_grain_key* d_keys, const uint32_t* d_acts,
                                             const uint8_t* d_silos, const int32_t* d_etags, size_t n, int64_t now_ticks,
                                             void* stream) {
    if (!c) return ORL_E_INVALID;
    if (int r = need_adaptive(c)) return r;
    if (n && !d_etags) return fail(c, ORL_E_INVALID, "null device buffer");
    c->cache_now = now_ticks;
    return cache_add(c, d_keys, d_acts, d_silos, d_etags, n, stream);
}

// One pass of the maintainer (cache_adaptive.hip).  The host's bounds stay as they are: the pass turns FULL slots into
// tombstones and nothing else, so the entries only shrink (cache_ub bounds them still) and the occupied slots, FULL +
// TOMB, do not change (cache_ub + cache_tombs_ub bounds them still) — and the add's path choice reads the bounds only
// as cache_ub alone and as that sum.
int orl_cache_maintain_device(orl_ctx* c, uint32_t me, uint32_t opts, int64_t now_ticks, struct orl_cache_sweep* out,
                              void* stream) {
    if (!c) return ORL_E_INVALID;
    if (int r = need_adaptive(c)) return r;
    if (!out) return fail(c, ORL_E_INVALID, "null result struct");
    if (me >= c->n_silos) return fail(c, ORL_E_INVALID, "silo %u out of range", me);
    if (int r = sync_device_state(c)) return r;
    c->cache_now = now_ticks;
    hipStream_t st = stream_of(c, stream);
    int e = launch_cache_sweep(c->d_params, c->d_cache, c->cache_slots - 1, c->d_cstate, me,
                               (opts & ORL_OPT_EXCLUDE_IF_STOPPING) != 0, c->n_silos, now_ticks, c->csw, st);
    if (e) return hipfail(c, (hipError_t)e, "cache sweep launch");
    out->d_keys = c->csw.keys;
    out->d_etags = c->csw.etags;
    out->d_owner_offsets = c->csw.owner_off;
    out->d_counts = c->csw.counts;
    return ORL_OK;
}

int orl_cache_mark_fresh_device(orl_ctx* c, const orl_grain_key* d_keys, size_t n, int64_t now_ticks, uint8_t* d_found,
                                void* stream) {
    if (!c) return ORL_E_INVALID;
    if (int r = need_adaptive(c)) return r;
    if (n && !d_keys) return fail(c, ORL_E_INVALID, "null device buffer");
    if (int r = check_batch(c, n)) return r;
    c->cache_now = now_ticks;
    hipStream_t st = stream_of(c, stream);
    int e = launch_cache_mark_fresh(c->d_cache, c->cache_slots - 1, d_keys, n, now_ticks, c->cache_max_ttl, c->cache_growth, d_found,
                                    st);
    if (e) return hipfail(c, (hipError_t)e, "cache mark-fresh launch");
    return ORL_OK;
}

// ProcessCacheRefreshResponse (AdaptiveDirectoryCacheMaintainer.cs:167-207) over the owner's whole answer, on the
// caller's stream (cache_evict.hip).  The path choice is the versioned add's, from the host's upper bounds
// with n as the bound on new entries: no eviction possible → the data-parallel apply alone (after a compaction when the
// load bound asks for one); else the selection and the serial pass are enqueued too — they leave at once on the device
// when the response holds no valid ADD, which the host cannot know — with the compaction between the tombstoning and the
// inserts when the load bound asks for it.  Removes only turn FULL slots into tombstones: the bounds hold as after a sweep.
int orl_cache_apply_refresh_device(orl_ctx* c, const orl_grain_key* d_keys, const uint8_t* d_kind, const int32_t* d_etags,
                                   const uint32_t* d_acts, const uint8_t* d_silos, size_t n, int64_t now_ticks,
                                   uint8_t* d_present, uint64_t* d_counts, void* stream) {
    if (!c) return ORL_E_INVALID;
    if (int r = need_adaptive(c)) return r;
    if (n && (!d_keys || !d_kind || !d_etags || !d_acts || !d_silos)) return fail(c, ORL_E_INVALID, "null device buffer");
    if (int r = check_batch(c, n)) return r;
    c->cache_now = now_ticks;
    int r = sync_device_state(c);
    if (r) return r;
    set_cache_on(c, true);
    if ((r = sync_device_state(c))) return r;
    hipStream_t st = stream_of(c, stream);
    const uint64_t mask = c->cache_slots - 1;
    CacheFresh fresh;
    fresh.etags = d_etags;
    fresh.now = now_ticks;
    fresh.initial_ttl = c->cache_initial_ttl;
    fresh.on = 1;
    CacheRefresh rf;
    rf.kind = d_kind;
    rf.max_ttl = c->cache_max_ttl;
    rf.growth = c->cache_growth;
    rf.present = d_present;
    rf.counts = d_counts;
    const bool evicts = c->cache_ub + n > c->cache_cap;
    const uint64_t fresh_ub = evicts ? std::min<uint64_t>(n, c->cache_cap) : n;  // an evicting call leaves at most capacity entries
    const bool crowded = (c->cache_ub + c->cache_tombs_ub + fresh_ub) * 8 > c->cache_slots * 7;
    if (crowded && !evicts && n) {  // only tombstones in the way: compact first
        int e = launch_cache_rebuild(c->d_cache, c->d_cache2, mask, c->d_cstate, c->cev, st, true);
        if (e) return hipfail(c, (hipError_t)e, "cache rebuild launch");
        std::swap(c->d_cache, c->d_cache2);
        ++c->cache_rebuilds;
        c->cache_tombs_ub = 0;
    }
    int e = launch_cache_apply_refresh(c->d_cache, mask, crowded && evicts ? c->d_cache2 : nullptr, c->d_cstate, c->cache_cap, d_keys,
                                       d_acts, d_silos, n, c->cfg.n_act, c->n_silos, c->d_params->local, c->cev, st, fresh, rf,
                                       evicts);
    if (e) return hipfail(c, (hipError_t)e, "cache refresh-apply launch");
    if (n == 0) return ORL_OK;
    const uint64_t occupied = c->cache_ub + c->cache_tombs_ub + fresh_ub;  // FULL + TOMB slots grow by at most the new entries
    c->cache_ub = std::min(c->cache_ub + n, c->cache_cap);
    c->cache_tombs_ub = occupied > c->cache_ub ? occupied - c->cache_ub : 0;
    if (evicts) {
        ++c->cache_evict_batches;
        if (crowded) {
            std::swap(c->d_cache, c->d_cache2);
            ++c->cache_rebuilds;
            c->cache_tombs_ub = 0;
        }
    }
    return ORL_OK;
}

int orl_cache_adjust_for_removed_silo_device(orl_ctx* c, uint32_t me, uint32_t opts, uint32_t removed_silo,
                                             uint64_t* d_removed_count, void* stream) {
    if (!c) return ORL_E_INVALID;
    if (int r = need_device(c)) return r;
    if (!c->cache_slots) return fail(c, ORL_E_STATE, "directory cache not configured (orl_cache_config)");
    if (me >= c->n_silos || removed_silo >= c->n_silos) return fail(c, ORL_E_INVALID, "silo out of range");
    if (int r = sync_device_state(c)) return r;
    hipStream_t st = stream_of(c, stream);
    int e = launch_cache_adjust(c->d_params, c->d_cache, c->cache_slots - 1, c->d_cstate, me,
                                (opts & ORL_OPT_EXCLUDE_IF_STOPPING) != 0, c->n_silos, removed_silo, d_removed_count, st);
    if (e) return hipfail(c, (hipError_t)e, "cache adjust launch");
    return ORL_OK;  // the host's bounds stay valid, as after a sweep
}

int orl_cache_peek_device(orl_ctx* c, const orl_grain_key* d_keys, size_t n, uint32_t* d_act, uint8_t* d_silo, int32_t* d_etag,
                          int64_t* d_ttl, int64_t* d_last_refreshed, uint8_t* d_accessed, void* stream) {
    if (!c) return ORL_E_INVALID;
    if (int r = need_device(c)) return r;
    if (!c->cache_slots) return fail(c, ORL_E_STATE, "directory cache not configured (orl_cache_config)");
    if (!c->cache_adaptive && (d_etag || d_ttl || d_last_refreshed || d_accessed))
        return fail(c, ORL_E_STATE, "etag, timer, refresh time and access mark exist only in an adaptive cache");
    if (n && !d_keys) return fail(c, ORL_E_INVALID, "null device buffer");
    if (n > 0xFFFFFFFFull) return fail(c, ORL_E_CAPACITY, "batch too large");
    hipStream_t st = stream_of(c, stream);
    int e = launch_cache_peek(c->d_cache, c->cache_slots - 1, c->cache_adaptive, d_keys, n, d_act, d_silo, d_etag, d_ttl,
                              d_last_refreshed, d_accessed, st);
    if (e) return hipfail(c, (hipError_t)e, "cache peek launch");
    return ORL_OK;
}

int orl_cache_remove_device(orl_ctx* c, const orl_grain_key* d_keys, size_t n, uint8_t* d_removed, void* stream) {
    if (!c) return ORL_E_INVALID;
    if (!c->cache_slots) return fail(c, ORL_E_STATE, "directory cache not configured (orl_cache_config)");
    if (n && (!d_keys || !d_removed)) return fail(c, ORL_E_INVALID, "null device buffer");
    if (int r = check_batch(c, n)) return r;
    hipStream_t st = stream_of(c, stream);
    int e = launch_dir_remove(c->d_cache, c->cache_slots - 1, c->d_cclaim, c->d_cstate, d_keys, n, c->d_dslot, d_removed, st);
    if (e) return hipfail(c, (hipError_t)e, "cache remove launch");
    c->cache_tombs_ub += n;
    return ORL_OK;
}

int orl_cache_stats(orl_ctx* c, struct orl_cache_stats* out) {
    if (!c || !out) return ORL_E_INVALID;
    *out = {};
    if (int r = need_device(c)) return r;
    if (!c->cache_slots) return fail(c, ORL_E_STATE, "directory cache not configured (orl_cache_config)");
    ORL_HIP(c, hipDeviceSynchronize());
    uint64_t st[4];
    ORL_HIP(c, hipMemcpy(st, c->d_cstate, sizeof st, hipMemcpyDeviceToHost));
    out->entries = st[0];
    out->tombstones = st[1];
    out->evictions = st[3] + c->cache_host_evictions;
    out->evict_batches = c->cache_evict_batches;
    out->rebuilds = c->cache_rebuilds;
    out->host_fallbacks = c->cache_host_fallbacks;
    if ((uint32_t)st[2]) return fail(c, ORL_E_STATE, "directory cache: the device raised error word 0x%x", (unsigned)(uint32_t)st[2]);
    return ORL_OK;
}

int orl_cache_evict_mode(orl_ctx* c, uint32_t mode) {
    if (!c) return ORL_E_INVALID;
    if (int r = need_device(c)) return r;
    if (mode != ORL_CACHE_EVICT_DEVICE && mode != ORL_CACHE_EVICT_HOST) return fail(c, ORL_E_INVALID, "unknown eviction mode %u", mode);
    if (mode == ORL_CACHE_EVICT_HOST && c->cache_adaptive)
        return fail(c, ORL_E_STATE, "the host LRU does not carry an adaptive cache's per-entry state");
    c->cache_mode = mode;
    return ORL_OK;
}

int orl_cache_count(orl_ctx* c, uint64_t* n) {
    if (!c || !n) return ORL_E_INVALID;
    *n = 0;
    if (!c->cache_slots) return ORL_OK;
    ORL_HIP(c, hipDeviceSynchronize());
    uint64_t st[3];
    ORL_HIP(c, hipMemcpy(st, c->d_cstate, sizeof st, hipMemcpyDeviceToHost));
    *n = st[0];
    return ORL_OK;
}

}  // extern "C"
