// cache_adaptive.hip — the adaptive directory cache's maintainer on the device (gfx950).
//
// AdaptiveDirectoryCacheMaintainer.Run (AdaptiveDirectoryCacheMaintainer.cs:54-143) walks every cache entry once a
// minute: entries this silo now owns and entries that expired unaccessed go, expired entries that were accessed are
// listed per directory owner with their ETags (BuildGrainAndETagList, :216-238) for one LookUpMany each.  The table
// lives only on the device, so the walk runs here, on the caller's stream: one pass that classifies every slot and
// counts the emitted entries per (owner, tile), one scan, one pass that tombstones, emits and restamps.
// MarkAsFresh, AdjustLocalCache's walk and a stamp-free lookup live here too.
//
// No kernel waits for another workgroup; every loop is bounded by the slot count or the silo count.

#include <hip/hip_runtime.h>

#include "cache_adaptive.h"
#include "dir_table_dev.h"
#include "tile_scan_dev.h"

namespace orl {

namespace {

constexpr uint32_t kPerThread = kSweepTile / 256u;  // slots per thread and tile
constexpr uint32_t kOwners = 256;                   // silo indices are bytes

// The sweep's verdict on a slot (the high byte of CacheSweepScratch::cls; the low byte is the owner).
enum : uint32_t { CL_NONE = 0, CL_SELF = 1, CL_KEPT = 2, CL_EXPIRED = 3, CL_REFRESH = 4, CL_NULL = 5 };

// The table walk both the sweep and AdjustLocalCache use: tile `blockIdx.x`, round j, every wave reads 64 consecutive
// slots (coalesced), and (wave, round, lane) ascending is slot order.
__device__ __forceinline__ uint64_t walk_slot(uint32_t j) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    return (uint64_t)blockIdx.x * kSweepTile + wave * (64u * kPerThread) + j * 64u + lane;
}

// ---- the sweep -------------------------------------------------------------------------------------------------------

// Pass 1: the verdict per slot (Maintainer.cs:85-130), the verdict counts, and the emitted entries per (owner, tile).
__global__ __launch_bounds__(256) void k_sw_classify(const RouteParams* __restrict__ gp, const DirSlot* __restrict__ cache,
                                                     uint64_t mask, uint32_t me, uint32_t excl, uint32_t n_silos, int64_t now,
                                                     uint16_t* __restrict__ cls, uint32_t* __restrict__ tile_cnt, uint32_t ntiles,
                                                     uint64_t* __restrict__ counts) {
    __shared__ RouteParams P;
    __shared__ uint32_t hist[kOwners];
    __shared__ uint32_t ccnt[8];
    stage_params(&P, gp);
    hist[threadIdx.x] = 0;
    if (threadIdx.x < 8) ccnt[threadIdx.x] = 0;
    __syncthreads();
    const CacheAdaptive a = cache_adaptive(cache, mask);
    const unsigned long long* gen = cache_gens(cache, mask);
    uint32_t c[CL_NULL + 1] = {0, 0, 0, 0, 0, 0};
    for (uint32_t j = 0; j < kPerThread; ++j) {
        const uint64_t s = walk_slot(j);
        if (s > mask) continue;
        const DirSlot d = cache[s];
        uint32_t verdict = CL_NONE, owner = 0xFFu;
        if (d.state == SLOT_FULL) {
            owner = target_silo<true>(P, d.tcd, d.n0, d.n1, me, excl != 0);
            if (owner >= n_silos) {
                verdict = CL_NULL;  // "there's no other silo and we're shutting down, so skip this entry" (:86-89)
                owner = 0xFFu;
            } else if (mask_bit(P.local, owner)) {
                verdict = CL_SELF;  // owner.Equals(MyAddress), for every partition this context holds (:91-98)
            } else if (now < a.last_refreshed[s] + a.ttl[s]) {
                verdict = CL_KEPT;  // !IsExpired() (:107-111; expired means now >= LastRefreshed + ExpirationTimer)
            } else if (gen[s] == a.seen[s]) {
                verdict = CL_EXPIRED;  // NumAccesses == 0 (:112-117)
            } else {
                verdict = CL_REFRESH;  // (:118-129)
                atomicAdd(&hist[owner], 1u);
            }
#pragma unroll
            for (uint32_t v = CL_SELF; v <= CL_NULL; ++v) c[v] += verdict == v ? 1u : 0u;
        }
        cls[s] = (uint16_t)(verdict << 8 | owner);
    }
#pragma unroll
    for (uint32_t v = CL_SELF; v <= CL_NULL; ++v)
        if (c[v]) atomicAdd(&ccnt[v], c[v]);
    __syncthreads();
    if (threadIdx.x < n_silos) tile_cnt[(size_t)threadIdx.x * ntiles + blockIdx.x] = hist[threadIdx.x];
    if (threadIdx.x >= CL_SELF && threadIdx.x <= CL_NULL && ccnt[threadIdx.x]) add64(&counts[threadIdx.x - 1], ccnt[threadIdx.x]);
}

// Exclusive scan of tile_cnt[n_silos * ntiles] (owner-major, so the result is each (owner, tile)'s first output position)
// by one workgroup, each thread a contiguous piece; owner_off[o] = the position where owner o's list begins.
__global__ __launch_bounds__(256) void k_sw_scan(uint32_t* __restrict__ tile_cnt, uint32_t ntiles, uint32_t n_silos,
                                                 uint32_t* __restrict__ owner_off) {
    __shared__ uint32_t lds[2 * 256];
    const uint32_t len = n_silos * ntiles;
    const uint32_t per = (len + 255u) / 256u;
    const uint32_t b = threadIdx.x * per < len ? threadIdx.x * per : len, e = b + per < len ? b + per : len;
    uint32_t sum = 0;
    for (uint32_t t = b; t < e; ++t) sum += tile_cnt[t];
    uint32_t total;
    uint32_t run = block_exclusive<uint32_t, OpAdd, 256>(sum, lds, &total);
    uint32_t next_owner = (b + ntiles - 1) / ntiles;  // the first owner whose list begins at or after b
    for (uint32_t t = b; t < e; ++t) {
        if (t == next_owner * ntiles) owner_off[next_owner++] = run;
        const uint32_t v = tile_cnt[t];
        tile_cnt[t] = run;
        run += v;
    }
    if (threadIdx.x == 255) owner_off[n_silos] = total;
}

// Pass 2: tombstones for the self-owned and the expired, and for every entry to refresh its (grain, ETag) at the
// owner's next output position p, the stamp G + p + 1 of BuildGrainAndETagList's cache.Get (LRU.Get takes the next
// generation) and NumAccesses = 0 (seen = that stamp).  An entry's position: its (owner, tile) offset, plus the owner's
// entries in the tile's earlier waves, plus its rank among the wave's — ballots over one owner at a time, in slot order.
__global__ __launch_bounds__(256) void k_sw_apply(DirSlot* __restrict__ cache, uint64_t mask, uint32_t n_silos,
                                                  const uint16_t* __restrict__ cls, const uint32_t* __restrict__ tile_off,
                                                  uint32_t ntiles, orl_grain_key* __restrict__ out_keys,
                                                  int32_t* __restrict__ out_etags, uint64_t out_cap, uint64_t* __restrict__ cnt) {
    __shared__ uint32_t wave_cnt[4][kOwners];  // per wave and owner: entries so far, then the wave's first position
    __shared__ uint32_t gone_tot;
    for (uint32_t w = 0; w < 4; ++w) wave_cnt[w][threadIdx.x] = 0;
    if (threadIdx.x == 0) gone_tot = 0;
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t verdict[kPerThread], rank[kPerThread];
    uint32_t gone = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPerThread; ++j) {
        const uint64_t s = walk_slot(j);
        const uint32_t v = s <= mask ? cls[s] : 0u;
        verdict[j] = v;
        rank[j] = 0;
        const bool emit = (v >> 8) == CL_REFRESH;
        unsigned long long todo = __ballot(emit);
        for (uint32_t it = 0; it < 64 && todo; ++it) {  // one owner of this round's entries per iteration
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t o = __shfl(v, (int)leader) & 0xFFu;
            const unsigned long long m = __ballot(emit && (v & 0xFFu) == o);
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(&wave_cnt[wave][o], (uint32_t)__popcll(m));
            base = __shfl(base, (int)leader);
            if (emit && (v & 0xFFu) == o) rank[j] = base + (uint32_t)__popcll(m & lt);
            todo &= ~m;
        }
        if ((v >> 8) == CL_SELF || (v >> 8) == CL_EXPIRED) {
            cache[s].state = SLOT_TOMB;
            ++gone;
        }
    }
    __syncthreads();
    if (threadIdx.x < n_silos) {  // counts → first positions
        uint32_t run = tile_off[(size_t)threadIdx.x * ntiles + blockIdx.x];
        for (uint32_t w = 0; w < 4; ++w) {
            const uint32_t k = wave_cnt[w][threadIdx.x];
            wave_cnt[w][threadIdx.x] = run;
            run += k;
        }
    }
    __syncthreads();
    const CacheAdaptive a = cache_adaptive(cache, mask);
    unsigned long long* gen = cache_gens(cache, mask);
    const unsigned long long G = gen[mask + 1];
#pragma unroll
    for (uint32_t j = 0; j < kPerThread; ++j) {
        if ((verdict[j] >> 8) != CL_REFRESH) continue;
        const uint64_t s = walk_slot(j);
        const uint64_t p = (uint64_t)wave_cnt[wave][verdict[j] & 0xFFu] + rank[j];
        if (p < out_cap) {  // at most `entries` <= capacity positions exist
            const DirSlot d = cache[s];
            out_keys[p] = orl_grain_key{d.tcd, d.n0, d.n1};
            out_etags[p] = a.etag[s];
        }
        gen[s] = G + p + 1ull;
        a.seen[s] = G + p + 1ull;
    }
    if (gone) atomicAdd(&gone_tot, gone);
    __syncthreads();
    if (threadIdx.x == 0 && gone_tot) {  // as orl_cache_remove_device: entries - k, tombstones + k
        add64(&cnt[0], ~(uint64_t)gone_tot + 1);
        add64(&cnt[1], (uint64_t)gone_tot);
    }
}

// G += the emitted count (the Gets' generations).
__global__ void k_sw_finish(const DirSlot* __restrict__ cache, uint64_t mask, const uint64_t* __restrict__ counts) {
    if (threadIdx.x == 0) cache_gens(cache, mask)[mask + 1] += counts[CL_REFRESH - 1];
}

// ---- AdjustLocalCache -----------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_adjust(const RouteParams* __restrict__ gp, DirSlot* __restrict__ cache, uint64_t mask,
                                                uint32_t me, uint32_t excl, uint32_t n_silos, uint32_t removed_silo,
                                                uint64_t* __restrict__ removed, uint64_t* __restrict__ cnt) {
    __shared__ RouteParams P;
    __shared__ uint32_t gone_tot;
    stage_params(&P, gp);
    if (threadIdx.x == 0) gone_tot = 0;
    __syncthreads();
    uint32_t gone = 0;
    for (uint32_t j = 0; j < kPerThread; ++j) {
        const uint64_t s = walk_slot(j);
        if (s > mask) continue;
        const DirSlot d = cache[s];
        if (d.state != SLOT_FULL) continue;
        const uint32_t owner = target_silo<true>(P, d.tcd, d.n0, d.n1, me, excl != 0);
        // 2) now owned by me (LocalGrainDirectory.cs:335-339); 1) the activation sat on the removed silo (:341-342:
        // RemoveActivations of a single-activation entry ends in Remove, :973-976)
        if ((owner < n_silos && mask_bit(P.local, owner)) || d.silo == removed_silo) {
            cache[s].state = SLOT_TOMB;
            ++gone;
        }
    }
    if (gone) atomicAdd(&gone_tot, gone);
    __syncthreads();
    if (threadIdx.x == 0 && gone_tot) {
        add64(&cnt[0], ~(uint64_t)gone_tot + 1);
        add64(&cnt[1], (uint64_t)gone_tot);
        if (removed) add64(removed, (uint64_t)gone_tot);
    }
}

// ---- per-key calls ---------------------------------------------------------------------------------------------------

// MarkAsFresh: TryGetValue (the next generation; NumAccesses untouched, so `seen` follows the stamp of an unaccessed
// entry), ExpirationTimer = Min(max, ExpirationTimer.Multiply(growth)) — (long)((double)ticks * growth),
// StandardExtensions.cs:34-39 — and LastRefreshed = now.
__global__ __launch_bounds__(256) void k_mark_fresh(DirSlot* __restrict__ cache, uint64_t mask, const orl_grain_key* __restrict__ keys,
                                                    uint32_t n, int64_t now, int64_t max_ttl, double growth,
                                                    uint8_t* __restrict__ found) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = find_full<false>(cache, mask, keys[i]);
    if (found) found[i] = s != ~0ull ? 1u : 0u;
    if (s == ~0ull) return;
    cache_mark_fresh_slot(cache, mask, s, cache_gens(cache, mask)[mask + 1] + i + 1ull, now, max_ttl, growth);
}

__global__ __launch_bounds__(256) void k_peek(const DirSlot* __restrict__ cache, uint64_t mask, uint32_t adaptive,
                                              const orl_grain_key* __restrict__ keys, uint32_t n, uint32_t* __restrict__ act,
                                              uint8_t* __restrict__ silo, int32_t* __restrict__ etag, int64_t* __restrict__ ttl,
                                              int64_t* __restrict__ last_refreshed, uint8_t* __restrict__ accessed) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = find_full<false>(cache, mask, keys[i]);
    const bool hit = s != ~0ull;
    if (act) act[i] = hit ? cache[s].act : ORL_NO_ACT;
    if (silo) silo[i] = hit ? cache[s].silo : (uint8_t)ORL_NULL_SILO;
    if (!adaptive) return;
    const CacheAdaptive a = cache_adaptive(cache, mask);
    if (etag) etag[i] = hit ? a.etag[s] : ORL_CACHE_NO_ETAG;
    if (ttl) ttl[i] = hit ? a.ttl[s] : 0;
    if (last_refreshed) last_refreshed[i] = hit ? a.last_refreshed[s] : 0;
    if (accessed) accessed[i] = hit && cache_gens(cache, mask)[s] > a.seen[s] ? 1u : 0u;
}

size_t carve(size_t& off, size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) & ~(size_t)255;
    return at;
}

}  // namespace

int cache_sweep_alloc(CacheSweepScratch* s, uint64_t capacity, uint64_t slots) {
    cache_sweep_free(s);
    const uint32_t ntiles = (uint32_t)((slots + kSweepTile - 1) / kSweepTile);
    size_t off = 0;
    const size_t o_cls = carve(off, slots * 2), o_tc = carve(off, (size_t)kOwners * ntiles * 4),
                 o_k = carve(off, capacity * sizeof(orl_grain_key)), o_e = carve(off, capacity * 4),
                 o_oo = carve(off, (kOwners + 1) * 4), o_c = carve(off, 8 * 8);
    uint8_t* b = nullptr;
    hipError_t e = hipMalloc((void**)&b, off);
    if (e != hipSuccess) return (int)e;
    s->base = b;
    s->slots = slots;
    s->capacity = capacity;
    s->ntiles = ntiles;
    s->cls = (uint16_t*)(b + o_cls); s->tile_cnt = (uint32_t*)(b + o_tc); s->keys = (orl_grain_key*)(b + o_k);
    s->etags = (int32_t*)(b + o_e); s->owner_off = (uint32_t*)(b + o_oo); s->counts = (uint64_t*)(b + o_c);
    return (int)hipMemset(b, 0, off);
}

void cache_sweep_free(CacheSweepScratch* s) {
    if (s->base) (void)hipFree(s->base);
    *s = CacheSweepScratch{};
}

int launch_cache_sweep(const RouteParams* d_params, DirSlot* d_cache, uint64_t mask, uint64_t* d_cnt, uint32_t me, bool excl,
                       uint32_t n_silos, int64_t now, const CacheSweepScratch& s, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (mask + 1 != s.slots || n_silos == 0 || n_silos > kOwners) return (int)hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(s.counts, 0, 8 * 8, st);
    if (e != hipSuccess) return (int)e;
    const dim3 g(s.ntiles), b(256);
    hipLaunchKernelGGL(k_sw_classify, g, b, 0, st, d_params, d_cache, mask, me, excl ? 1u : 0u, n_silos, now, s.cls, s.tile_cnt,
                       s.ntiles, s.counts);
    hipLaunchKernelGGL(k_sw_scan, dim3(1), b, 0, st, s.tile_cnt, s.ntiles, n_silos, s.owner_off);
    hipLaunchKernelGGL(k_sw_apply, g, b, 0, st, d_cache, mask, n_silos, s.cls, s.tile_cnt, s.ntiles, s.keys, s.etags, s.capacity,
                       d_cnt);
    hipLaunchKernelGGL(k_sw_finish, dim3(1), dim3(64), 0, st, d_cache, mask, s.counts);
    return (int)hipGetLastError();
}

int launch_cache_adjust(const RouteParams* d_params, DirSlot* d_cache, uint64_t mask, uint64_t* d_cnt, uint32_t me, bool excl,
                        uint32_t n_silos, uint32_t removed_silo, uint64_t* d_removed, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (d_removed) {
        hipError_t e = hipMemsetAsync(d_removed, 0, 8, st);
        if (e != hipSuccess) return (int)e;
    }
    const uint32_t ntiles = (uint32_t)((mask + kSweepTile) / kSweepTile);
    hipLaunchKernelGGL(k_adjust, dim3(ntiles), dim3(256), 0, st, d_params, d_cache, mask, me, excl ? 1u : 0u, n_silos, removed_silo,
                       d_removed, d_cnt);
    return (int)hipGetLastError();
}

int launch_cache_mark_fresh(DirSlot* d_cache, uint64_t mask, const orl_grain_key* d_keys, size_t n, int64_t now, int64_t max_ttl,
                            double growth, uint8_t* d_found, void* stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_mark_fresh, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_cache, mask, d_keys,
                       (uint32_t)n, now, max_ttl, growth, d_found);
    return launch_cache_gen_advance(d_cache, mask, n, stream);
}

int launch_cache_peek(const DirSlot* d_cache, uint64_t mask, bool adaptive, const orl_grain_key* d_keys, size_t n, uint32_t* d_act,
                      uint8_t* d_silo, int32_t* d_etag, int64_t* d_ttl, int64_t* d_last_refreshed, uint8_t* d_accessed,
                      void* stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_peek, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_cache, mask,
                       adaptive ? 1u : 0u, d_keys, (uint32_t)n, d_act, d_silo, d_etag, d_ttl, d_last_refreshed, d_accessed);
    return (int)hipGetLastError();
}

}  // namespace orl
