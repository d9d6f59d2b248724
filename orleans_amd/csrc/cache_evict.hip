// cache_evict.hip — the directory cache's LRU eviction on the device (gfx950).
//
// AdaptiveGrainDirectoryCache.AddOrUpdate → LRU.Add runs AdjustSize before every add (LRU.cs:104-116,188-205): while
// Count >= MaximumSize the entry of the smallest generation goes.  A batch of n adds at capacity is therefore a
// sequential process; here it runs, bit for bit, as one data-parallel preparation, one short serial pass over
// sequential arrays and one data-parallel apply, all on the caller's stream (DESIGN "Directory cache: eviction on
// the device" has the algorithm and its bound).  Tombstone compaction (the rebuild) lives here too.
//
// Every loop is bounded by a size; a violated invariant sets the error word (d_cnt[2]) and the pass ends.

#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "cache_adaptive.h"
#include "cache_evict.h"
#include "dir_table_dev.h"
#include "tile_scan_dev.h"

namespace orl {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;     // no index; as nxt: never touched again (infinity)
constexpr uint32_t kInvalid = 0xFFFFFFFEu;  // an invalid batch entry: takes no step, is never evicted
constexpr uint32_t kAlways = 0xFFFFFFFDu;   // prevpos: the old entry is no candidate, so it is present throughout
constexpr uint32_t kEvTile = 2048;          // slots per compaction tile (256 threads x 8)
constexpr uint32_t kChunk = 2048;           // queue / batch elements the serial pass stages in LDS at a time
constexpr uint32_t kErrNoSlot = 1u;         // the existing "no free slot" bit
constexpr uint32_t kErrInvariant = 2u;

enum { ST_NVALID = 0, ST_K = 1, ST_PREFIX = 2, ST_RANK = 3, ST_NCAND = 4, ST_FINAL = 5, ST_EVICTED = 6, ST_REBUILT = 7 };

__device__ __forceinline__ void raise(uint64_t* cnt, uint32_t bit) { atomicOr(reinterpret_cast<uint32_t*>(cnt + 2), bit); }

// ---- preparation ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_ev_fill(uint32_t ncap, uint64_t* __restrict__ cand_stamp, uint32_t* __restrict__ cand_slot,
                                                 uint32_t* __restrict__ nxt_c, uint8_t* __restrict__ ev_c, uint64_t* __restrict__ st) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q < 16) st[q] = 0;
    if (q >= ncap) return;
    cand_stamp[q] = ~0ull;
    cand_slot[q] = kNone;
    nxt_c[q] = kNone;
    ev_c[q] = 0;
}

// Per batch entry: the validity predicate of k_cache_probe, the key's FULL slot in the table (a read-only walk) and its
// batch-local group (each distinct key claims one entry of group_tab; equal means equal keys, never equal hashes).
__global__ __launch_bounds__(256) void k_ev_prep(const DirSlot* __restrict__ cache, uint64_t mask, const orl_grain_key* __restrict__ keys,
                                                 const uint32_t* __restrict__ acts, const uint8_t* __restrict__ silos, uint32_t n,
                                                 uint32_t n_act, uint32_t n_silos, const uint32_t* __restrict__ local,
                                                 uint32_t* __restrict__ group_tab, uint32_t gmask, uint32_t* __restrict__ old_slot,
                                                 uint64_t* __restrict__ gkey, uint32_t* __restrict__ prev_b, uint32_t* __restrict__ nxt_b,
                                                 uint8_t* __restrict__ ev_b, uint64_t* __restrict__ st, uint64_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool valid = false;
    if (i < n) {
        const uint32_t sl = silos[i], a = acts[i];
        valid = sl < n_silos && (a < n_act || (a != ORL_NO_ACT && !mask_bit(local, sl)));
        uint32_t os = kNone, grp = kNone;
        if (valid) {
            const orl_grain_key k = keys[i];
            os = (uint32_t)find_full<true>(cache, mask, k);  // not found: ~0 truncates to kNone
            uint32_t g = fmix32(jenkins3(k.type_code_data, k.n0, k.n1)) & gmask;
            for (uint32_t step = 0; step <= gmask; ++step) {
                const uint32_t occ = atomicCAS(&group_tab[g], kNone, i);
                if (occ == kNone) {
                    grp = g;
                    break;
                }
                const orl_grain_key o = keys[occ];
                if (o.type_code_data == k.type_code_data && o.n0 == k.n0 && o.n1 == k.n1) {
                    grp = g;
                    break;
                }
                g = (g + 1) & gmask;
            }
            if (grp == kNone) {  // group_tab holds >= 2 n entries: cannot be full
                raise(cnt, kErrInvariant);
                valid = false;
            }
        }
        old_slot[i] = os;
        gkey[i] = valid ? (((uint64_t)grp << 32) | i) : ~0ull;
        prev_b[i] = kNone;
        nxt_b[i] = valid ? kNone : kInvalid;
        ev_b[i] = 0;
    }
    const int nv = __syncthreads_count(valid ? 1 : 0);
    if (threadIdx.x == 0 && nv) add64(&st[ST_NVALID], (uint64_t)nv);
}

// Over the (group, index) pairs sorted: neighbours of one group are the key's occurrences in batch order.
__global__ __launch_bounds__(256) void k_ev_link(const uint64_t* __restrict__ gs, uint32_t n, uint32_t* __restrict__ prev_b,
                                                 uint32_t* __restrict__ nxt_b, uint32_t* __restrict__ group_tab) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint64_t v = gs[j];
    if (v == ~0ull) return;
    const uint32_t grp = (uint32_t)(v >> 32), i = (uint32_t)v;
    if (j > 0 && (uint32_t)(gs[j - 1] >> 32) == grp)
        prev_b[i] = (uint32_t)gs[j - 1];
    else
        group_tab[grp] = kNone;  // the group's first entry leaves the claim table clean for the next batch
    if (j + 1 < n && (uint32_t)(gs[j + 1] >> 32) == grp) nxt_b[i] = (uint32_t)gs[j + 1];
}

// ---- candidates: the K = min(entries, 2 n_valid) FULL slots with the smallest stamps -------------------------------

__global__ __launch_bounds__(256) void k_ev_snapshot(const DirSlot* __restrict__ cache, uint64_t mask, uint64_t* __restrict__ skey,
                                                     uint64_t* __restrict__ st, uint32_t* __restrict__ hist,
                                                     const uint64_t* __restrict__ cnt) {
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.x == 0) {
        hist[threadIdx.x] = 0;
        if (threadIdx.x == 0) {
            const uint64_t entries = cnt[0], nv2 = 2 * st[ST_NVALID];
            const uint64_t K = entries < nv2 ? entries : nv2;
            st[ST_K] = K;
            st[ST_PREFIX] = 0;
            st[ST_RANK] = K;
        }
    }
    if (s > mask) return;
    skey[s] = slot_state(cache, s) == SLOT_FULL ? cache_gens(cache, mask)[s] : ~0ull;
}

// One 8-bit digit of the radix select: counts, per digit value, the stamps that match the prefix found so far.
__global__ __launch_bounds__(256) void k_ev_hist(const uint64_t* __restrict__ skey, uint64_t slots, uint32_t shift,
                                                 const uint64_t* __restrict__ st, uint32_t* __restrict__ hist) {
    __shared__ uint32_t lh[256];
    if (st[ST_K] == 0) return;
    lh[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t prefix = st[ST_PREFIX];
    const uint64_t himask = shift >= 56 ? 0ull : (~0ull << (shift + 8));
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256u) {
        const uint64_t v = skey[s];
        if (v != ~0ull && (v & himask) == prefix) atomicAdd(&lh[(uint32_t)(v >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    if (lh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], lh[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_ev_pick(uint64_t* __restrict__ st, uint32_t* __restrict__ hist, uint32_t shift,
                                                 uint64_t* __restrict__ cnt) {
    __shared__ uint32_t lh[256];
    lh[threadIdx.x] = hist[threadIdx.x];
    hist[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x != 0 || st[ST_K] == 0) return;
    uint64_t rank = st[ST_RANK], cum = 0;
    uint32_t d = 0;
    for (; d < 256; ++d) {
        if (cum + lh[d] >= rank) break;
        cum += lh[d];
    }
    if (d == 256) {  // fewer FULL slots than the entry counter says
        raise(cnt, kErrInvariant);
        st[ST_K] = 0;
        return;
    }
    st[ST_PREFIX] |= (uint64_t)d << shift;
    st[ST_RANK] = rank - cum;
}

// Compaction in slot order (so the stable sort breaks stamp ties by slot index): count, scan, emit.
__global__ __launch_bounds__(256) void k_ev_ccount(const uint64_t* __restrict__ skey, uint64_t slots, const uint64_t* __restrict__ st,
                                                   uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    const uint64_t K = st[ST_K], T = st[ST_PREFIX];
    const uint64_t s0 = (uint64_t)blockIdx.x * kEvTile + threadIdx.x * 8u;
    uint32_t c = 0;
    for (uint32_t e = 0; e < 8; ++e) {
        const uint64_t s = s0 + e;
        if (s < slots && K) {
            const uint64_t v = skey[s];
            c += (v != ~0ull && v <= T) ? 1u : 0u;
        }
    }
    if (c) atomicAdd(&tot, c);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_ev_cscan(uint32_t* __restrict__ tile_cnt, uint32_t ntiles, uint64_t* __restrict__ st,
                                                  uint32_t ncap, uint64_t* __restrict__ cnt) {
    __shared__ uint32_t lds[2 * 256];
    const uint32_t per = (ntiles + 255u) / 256u;
    const uint32_t b = threadIdx.x * per, e = b + per < ntiles ? b + per : ntiles;
    uint32_t sum = 0;
    for (uint32_t t = b; t < e; ++t) sum += tile_cnt[t];
    uint32_t total;
    uint32_t run = block_exclusive<uint32_t, OpAdd, 256>(sum, lds, &total);
    for (uint32_t t = b; t < e; ++t) {
        const uint32_t v = tile_cnt[t];
        tile_cnt[t] = run;
        run += v;
    }
    if (threadIdx.x == 0) {
        if (total > ncap) {  // more stamp ties at the threshold than the candidate arrays hold
            raise(cnt, kErrInvariant);
            total = ncap;
        }
        st[ST_NCAND] = total;
    }
}

__global__ __launch_bounds__(256) void k_ev_cemit(const uint64_t* __restrict__ skey, uint64_t slots, const uint64_t* __restrict__ st,
                                                  const uint32_t* __restrict__ tile_off, uint64_t* __restrict__ cand_stamp,
                                                  uint32_t* __restrict__ cand_slot, uint32_t ncap) {
    __shared__ uint32_t lds[2 * 256];
    const uint64_t K = st[ST_K], T = st[ST_PREFIX];
    const uint64_t s0 = (uint64_t)blockIdx.x * kEvTile + threadIdx.x * 8u;
    uint64_t v[8];
    uint32_t c = 0;
    for (uint32_t e = 0; e < 8; ++e) {
        const uint64_t s = s0 + e;
        v[e] = (s < slots && K) ? skey[s] : ~0ull;
        c += (v[e] != ~0ull && v[e] <= T) ? 1u : 0u;
    }
    uint32_t total;
    uint32_t pos = tile_off[blockIdx.x] + block_exclusive<uint32_t, OpAdd, 256>(c, lds, &total);
    for (uint32_t e = 0; e < 8; ++e)
        if (v[e] != ~0ull && v[e] <= T) {
            if (pos < ncap) {
                cand_stamp[pos] = v[e];
                cand_slot[pos] = (uint32_t)(s0 + e);
            }
            ++pos;
        }
}

__global__ __launch_bounds__(256) void k_ev_mark(const uint32_t* __restrict__ cand_slot_s, const uint64_t* __restrict__ st,
                                                 uint32_t* __restrict__ slotpos, uint64_t slots) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= st[ST_NCAND]) return;
    const uint32_t s = cand_slot_s[q];
    if (s < slots) slotpos[s] = q;
}

// prevpos of every batch entry, and nxt of the candidates the batch touches.
__global__ __launch_bounds__(256) void k_ev_prev(uint32_t n, const uint32_t* __restrict__ prev_b, const uint32_t* __restrict__ nxt_b,
                                                 const uint32_t* __restrict__ old_slot, const uint32_t* __restrict__ slotpos,
                                                 const uint64_t* __restrict__ st, uint32_t* __restrict__ prevpos,
                                                 uint32_t* __restrict__ nxt_c) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t pp = kNone;
    if (nxt_b[i] == kInvalid) {
        pp = kInvalid;
    } else if (prev_b[i] != kNone) {
        pp = (uint32_t)st[ST_NCAND] + prev_b[i];
    } else if (old_slot[i] != kNone) {
        const uint32_t cp = slotpos[old_slot[i]];
        if (cp != kNone) {
            pp = cp;
            nxt_c[cp] = i;  // the key's first occurrence in the batch: one writer
        } else {
            pp = kAlways;
        }
    }
    prevpos[i] = pp;
}

// ---- the serial pass ------------------------------------------------------------------------------------------------
// One workgroup stages kChunk-element windows of the two sequential arrays (nxt in queue order from the pointer p,
// prevpos in batch order from the entry i) through LDS; one lane steps.  No data-dependent global load.
__global__ __launch_bounds__(256) void k_ev_serial(const uint32_t* __restrict__ nxt_c, const uint32_t* __restrict__ nxt_b,
                                                   const uint32_t* __restrict__ prevpos, uint32_t n, uint64_t capacity,
                                                   uint64_t* __restrict__ cnt, uint64_t* __restrict__ st, uint8_t* __restrict__ ev_c,
                                                   uint8_t* __restrict__ ev_b) {
    __shared__ uint32_t qbuf[kChunk], bbuf[kChunk];
    __shared__ uint32_t s_p, s_i, s_done;
    __shared__ uint64_t s_c, s_ev;
    const uint32_t ncand = (uint32_t)st[ST_NCAND];
    const uint64_t entries0 = cnt[0];
    const uint64_t Q = (uint64_t)ncand + n;
    if (threadIdx.x == 0) {
        s_p = 0;
        s_i = 0;
        s_done = 0;
        s_c = entries0;
        s_ev = 0;
    }
    __syncthreads();
    const uint64_t max_rounds = (Q + n) / kChunk + 4;
    for (uint64_t round = 0; round < max_rounds; ++round) {
        const uint32_t q0 = s_p, b0 = s_i;
        if (s_done || b0 >= n) break;
        for (uint32_t t = threadIdx.x; t < kChunk; t += 256u) {
            const uint64_t q = (uint64_t)q0 + t;
            qbuf[t] = q < ncand ? nxt_c[q] : (q < Q ? nxt_b[q - ncand] : kInvalid);
            const uint64_t b = (uint64_t)b0 + t;
            bbuf[t] = b < n ? prevpos[b] : kInvalid;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t p = q0, i = b0;
            uint64_t c = s_c, ev = s_ev;
            bool stop = false, bad = false;
            while (i < n && i - b0 < kChunk && !stop) {
                const uint32_t pp = bbuf[i - b0];
                if (pp == kInvalid) {
                    ++i;
                    continue;
                }
                while (c >= capacity && !stop) {  // AdjustSize
                    // advance over invalid batch entries and over elements the batch re-stamped before i
                    while (p - q0 < kChunk && p < Q && (qbuf[p - q0] == kInvalid || qbuf[p - q0] < i)) ++p;
                    if (p >= Q || (p >= ncand && p - ncand >= i) || (p >= ncand && ncand < entries0)) {
                        bad = stop = true;  // nothing left to evict / the pointer left the candidates
                    } else if (p - q0 >= kChunk) {
                        stop = true;  // refill the queue window, then resume at this entry
                    } else {
                        if (p < ncand) ev_c[p] = 1; else ev_b[p - ncand] = 1;
                        ++p;
                        --c;
                        ++ev;
                    }
                }
                if (stop) break;
                const bool present = pp != kNone && (pp == kAlways || pp >= p);
                if (!present) ++c;
                ++i;
            }
            s_p = p;
            s_i = i;
            s_c = c;
            s_ev = ev;
            if (bad) {
                raise(cnt, kErrInvariant);
                s_done = 1;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (!s_done && s_i < n) raise(cnt, kErrInvariant);  // the round bound ran out
        st[ST_FINAL] = s_c;
        st[ST_EVICTED] = s_ev;
        cnt[3] += s_ev;
    }
}

// ---- apply ----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_ev_tomb_c(DirSlot* __restrict__ cache, uint64_t slots, const uint32_t* __restrict__ cand_slot_s,
                                                   const uint8_t* __restrict__ ev_c, const uint64_t* __restrict__ st,
                                                   uint32_t* __restrict__ slotpos, uint64_t* __restrict__ cnt) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    bool gone = false;
    if (q < st[ST_NCAND]) {
        const uint32_t s = cand_slot_s[q];
        if (s < slots) {
            slotpos[s] = kNone;
            if (ev_c[q]) {
                cache[s].state = SLOT_TOMB;
                gone = true;
            }
        }
    }
    const int k = __syncthreads_count(gone ? 1 : 0);
    if (threadIdx.x == 0 && k) {
        add64(&cnt[0], ~(uint64_t)k + 1);  // entries - k
        add64(&cnt[1], (uint64_t)k);       // tombstones + k
    }
}

// A key's fate is that of its last incarnation: when the batch's last occurrence of a key was evicted, the key's old slot
// (still FULL when the old entry was only superseded, never evicted itself) goes too.  keep = last occurrence, not evicted.
__global__ __launch_bounds__(256) void k_ev_tomb_b(DirSlot* __restrict__ cache, uint32_t n, const uint32_t* __restrict__ nxt_b,
                                                   const uint8_t* __restrict__ ev_b, const uint32_t* __restrict__ old_slot,
                                                   uint8_t* __restrict__ keep, uint64_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool gone = false;
    if (i < n) {
        const bool last = nxt_b[i] == kNone;
        keep[i] = (last && !ev_b[i]) ? 1 : 0;
        if (last && ev_b[i] && old_slot[i] != kNone && cache[old_slot[i]].state == SLOT_FULL) {
            cache[old_slot[i]].state = SLOT_TOMB;
            gone = true;
        }
    }
    const int k = __syncthreads_count(gone ? 1 : 0);
    if (threadIdx.x == 0 && k) {
        add64(&cnt[0], ~(uint64_t)k + 1);
        add64(&cnt[1], (uint64_t)k);
    }
}

// Insert or update the kept entries (one per key, so no two threads write one key): an equal FULL entry is updated in
// place, else the first free slot of the chain is claimed by CAS.  Stamp = G + i + 1.
__global__ __launch_bounds__(256) void k_ev_insert(DirSlot* __restrict__ cache, uint64_t mask, const orl_grain_key* __restrict__ keys,
                                                   const uint32_t* __restrict__ acts, const uint8_t* __restrict__ silos, uint32_t n,
                                                   const uint8_t* __restrict__ keep, uint64_t* __restrict__ cnt, CacheFresh fresh) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const orl_grain_key k = keys[i];
    unsigned long long* gen = cache_gens(cache, mask);
    const unsigned long long stamp = gen[mask + 1] + i + 1ull;
    // adaptive cache: the new GrainDirectoryCacheEntry's state goes where the stamp goes
    const auto fresh_state = [&](uint64_t slot) {
        if (!fresh.on) return;
        const CacheAdaptive a = cache_adaptive(cache, mask);
        a.etag[slot] = fresh.etags ? fresh.etags[i] : 0;
        a.ttl[slot] = fresh.initial_ttl;
        a.last_refreshed[slot] = fresh.now;
        a.seen[slot] = stamp;
    };
    const uint64_t w24 = (uint64_t)acts[i] | ((uint64_t)silos[i] << 32) | ((uint64_t)SLOT_FULL << 40);
    const uint64_t old = find_full<true>(cache, mask, k);
    if (old != ~0ull) {  // an equal FULL entry: update
        uint64_t* p24 = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(cache + old) + 24);
        __hip_atomic_store(p24, w24, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        gen[old] = stamp;
        fresh_state(old);
        return;
    }
    uint64_t cur = key_start(k, mask);
    for (uint64_t step = 0; step <= mask; ++step) {  // a new entry: the chain's first free slot nobody else takes
        const uint32_t v = __hip_atomic_load(slot_word28(cache, cur), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t state = (v >> 8) & 0xFFu;
        if (state == SLOT_EMPTY || state == SLOT_TOMB) {
            uint32_t expect = v;
            if (__hip_atomic_compare_exchange_strong(slot_word28(cache, cur), &expect, (uint32_t)SLOT_CLAIMING << 8, __ATOMIC_RELAXED,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                uint64_t* kw = reinterpret_cast<uint64_t*>(cache + cur);
                __hip_atomic_store(kw, k.type_code_data, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(kw + 1, k.n0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(kw + 2, k.n1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                gen[cur] = stamp;
                fresh_state(cur);
                __atomic_thread_fence(__ATOMIC_RELEASE);  // the key is visible before the slot reads FULL
                __hip_atomic_store(kw + 3, w24, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                add64(&cnt[0], 1);
                if (state == SLOT_TOMB) add64(&cnt[1], ~0ull);
                return;
            }
        }
        cur = (cur + 1) & mask;
    }
    raise(cnt, kErrNoSlot);
}

__global__ void k_ev_finish(DirSlot* __restrict__ cache, uint64_t mask, uint64_t n, uint64_t* __restrict__ cnt,
                            const uint64_t* __restrict__ st) {
    if (threadIdx.x != 0) return;
    if (cnt[0] != st[ST_FINAL]) raise(cnt, kErrInvariant);  // the apply and the serial pass disagree on the live count
    cache_gens(cache, mask)[mask + 1] += n;
}

// ---- tombstone compaction -------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_rb_move(const DirSlot* __restrict__ src, DirSlot* __restrict__ dst, uint64_t mask,
                                                 uint64_t* __restrict__ st, uint64_t* __restrict__ cnt, uint32_t adaptive) {
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool moved = false;
    if (s <= mask && src[s].state == SLOT_FULL) {
        const DirSlot e = src[s];
        const unsigned long long stamp = cache_gens(src, mask)[s];
        uint64_t cur = dir_slot(jenkins3(e.tcd, e.n0, e.n1), mask);
        for (uint64_t step = 0; step <= mask && !moved; ++step) {
            uint32_t expect = 0;  // EMPTY (the table was zeroed); keys are distinct, so the first free slot is the place
            if (__hip_atomic_compare_exchange_strong(slot_word28(dst, cur), &expect, (uint32_t)SLOT_CLAIMING << 8, __ATOMIC_RELAXED,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                uint64_t* w = reinterpret_cast<uint64_t*>(dst + cur);
                w[0] = e.tcd;
                w[1] = e.n0;
                w[2] = e.n1;
                w[3] = (uint64_t)e.act | ((uint64_t)e.silo << 32) | ((uint64_t)SLOT_FULL << 40);
                cache_gens(dst, mask)[cur] = stamp;
                if (adaptive) {  // the entry keeps its ETag, timer and access mark (`seen` beside its unchanged stamp)
                    const CacheAdaptive from = cache_adaptive(src, mask), to = cache_adaptive(dst, mask);
                    to.etag[cur] = from.etag[s];
                    to.ttl[cur] = from.ttl[s];
                    to.last_refreshed[cur] = from.last_refreshed[s];
                    to.seen[cur] = from.seen[s];
                }
                moved = true;
            }
            cur = (cur + 1) & mask;
        }
        if (!moved) raise(cnt, kErrNoSlot);
    }
    const int k = __syncthreads_count(moved ? 1 : 0);
    if (threadIdx.x == 0 && k) add64(&st[ST_REBUILT], (uint64_t)k);
}

__global__ void k_rb_begin(uint64_t* __restrict__ st) {
    if (threadIdx.x == 0) st[ST_REBUILT] = 0;
}

__global__ void k_rb_finish(const DirSlot* __restrict__ src, DirSlot* __restrict__ dst, uint64_t mask, uint64_t* __restrict__ st,
                            uint64_t* __restrict__ cnt) {
    if (threadIdx.x != 0) return;
    cache_gens(dst, mask)[mask + 1] = cache_gens(src, mask)[mask + 1];  // G runs on
    if (st[ST_REBUILT] != cnt[0]) raise(cnt, kErrInvariant);
    cnt[0] = st[ST_REBUILT];
    cnt[1] = 0;
}

// ---- a refresh response: one operation per entry (orl_cache_apply_refresh_device) ----------------------------------
// ProcessCacheRefreshResponse (AdaptiveDirectoryCacheMaintainer.cs:167-207) is the batch add's sequential process with
// three kinds of step: AddOrUpdate (AdjustSize first), Remove, MarkAsFresh.  Same three phases; the keys of the entries
// that take a step are distinct (a later occurrence of a key is ignored), so a batch element is never superseded and the
// queue's batch part carries one bit, `live`: an ADD's element always, a FRESH's when it found its key, a REMOVE's never.
// The counts that size the work (valid ADDs, operations) exist only on the device: every kernel of the selection and the
// serial pass leaves at once when the response holds no ADD.

enum : uint8_t { OP_IGNORE = 0, OP_ADD = 1, OP_REMOVE = 2, OP_FRESH = 3 };
enum { ST_ADDS = 8, ST_REMOVES = 9, ST_FRESHES = 10 };  // after ST_REBUILT: the operations of the call

// Per entry: its operation, the key's FULL slot (a read-only walk) and its claim-table group.  The claim keeps the
// smallest index of a key's occurrences: a slot only ever goes from one occurrence of a key to an earlier one of the same.
__global__ __launch_bounds__(256) void k_ra_prep(const DirSlot* __restrict__ cache, uint64_t mask, const orl_grain_key* __restrict__ keys,
                                                 const uint8_t* __restrict__ kind, const uint32_t* __restrict__ acts,
                                                 const uint8_t* __restrict__ silos, uint32_t n, uint32_t n_act, uint32_t n_silos,
                                                 const uint32_t* __restrict__ local, uint32_t* group_tab, uint32_t gmask,
                                                 uint32_t* __restrict__ old_slot, uint32_t* __restrict__ grp_b,
                                                 uint8_t* __restrict__ op_b, uint64_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint8_t op = OP_IGNORE;
    const uint32_t kd = kind[i];
    if (kd == ORL_LUM_UPDATED) {
        const uint32_t sl = silos[i], a = acts[i];  // k_cache_probe's predicate
        if (sl < n_silos && (a < n_act || (a != ORL_NO_ACT && !mask_bit(local, sl)))) op = OP_ADD;
    } else if (kd == ORL_LUM_ABSENT || kd == ORL_LUM_UNSUPPORTED || kd == ORL_LUM_UPDATED_EMPTY) {
        op = OP_REMOVE;
    } else if (kd == ORL_LUM_UNCHANGED) {
        op = OP_FRESH;
    }
    uint32_t os = kNone, grp = kNone;
    if (op != OP_IGNORE) {
        const orl_grain_key k = keys[i];
        os = (uint32_t)find_full<true>(cache, mask, k);  // not found: ~0 truncates to kNone
        uint32_t g = fmix32(jenkins3(k.type_code_data, k.n0, k.n1)) & gmask;
        for (uint32_t step = 0; step <= gmask; ++step) {
            const uint32_t occ = atomicCAS(&group_tab[g], kNone, i);
            if (occ == kNone) {
                grp = g;
                break;
            }
            const orl_grain_key o = keys[occ];
            if (o.type_code_data == k.type_code_data && o.n0 == k.n0 && o.n1 == k.n1) {
                atomicMin(&group_tab[g], i);
                grp = g;
                break;
            }
            g = (g + 1) & gmask;
        }
        if (grp == kNone) {  // group_tab holds >= 2 n entries: cannot be full
            raise(cnt, kErrInvariant);
            op = OP_IGNORE;
        }
    }
    old_slot[i] = os;
    grp_b[i] = grp;
    op_b[i] = op;
}

// A key's first occurrence keeps its operation, the later ones are ignored; the operations are counted.
__global__ __launch_bounds__(256) void k_ra_resolve(uint32_t n, const uint32_t* __restrict__ group_tab, const uint32_t* __restrict__ grp_b,
                                                    uint8_t* __restrict__ op_b, uint8_t* __restrict__ ev_b, uint32_t* __restrict__ live_b,
                                                    uint8_t* __restrict__ present_b, uint64_t* __restrict__ st) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint8_t op = OP_IGNORE;
    if (i < n) {
        op = op_b[i];
        if (op != OP_IGNORE && group_tab[grp_b[i]] != i) op_b[i] = op = OP_IGNORE;
        ev_b[i] = 0;
        live_b[i] = 0;
        present_b[i] = 0;
    }
    const int na = __syncthreads_count(op == OP_ADD), nr = __syncthreads_count(op == OP_REMOVE),
              nf = __syncthreads_count(op == OP_FRESH);
    if (threadIdx.x == 0) {
        if (na) add64(&st[ST_ADDS], (uint64_t)na);
        if (nr) add64(&st[ST_REMOVES], (uint64_t)nr);
        if (nf) add64(&st[ST_FRESHES], (uint64_t)nf);
    }
}

// k_ev_snapshot with K = min(entries, n_add + n_ops): at most n_add evictions, at most n_ops old entries skipped because
// an earlier operation re-stamped or removed them.  No ADD: K = 0 and the table is not read.
__global__ __launch_bounds__(256) void k_ra_snapshot(const DirSlot* __restrict__ cache, uint64_t mask, uint64_t* __restrict__ skey,
                                                     uint64_t* __restrict__ st, uint32_t* __restrict__ hist,
                                                     const uint64_t* __restrict__ cnt) {
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t n_add = st[ST_ADDS];
    if (blockIdx.x == 0) {
        hist[threadIdx.x] = 0;
        if (threadIdx.x == 0) {
            const uint64_t entries = cnt[0], bound = n_add + n_add + st[ST_REMOVES] + st[ST_FRESHES];
            const uint64_t K = n_add == 0 ? 0 : (entries < bound ? entries : bound);
            st[ST_K] = K;
            st[ST_PREFIX] = 0;
            st[ST_RANK] = K;
        }
    }
    if (n_add == 0 || s > mask) return;
    skey[s] = slot_state(cache, s) == SLOT_FULL ? cache_gens(cache, mask)[s] : ~0ull;
}

// prevpos of every entry that takes a step, and nxt of the candidates the response names (each by one entry).
__global__ __launch_bounds__(256) void k_ra_prev(uint32_t n, const uint8_t* __restrict__ op_b, const uint32_t* __restrict__ old_slot,
                                                 const uint32_t* __restrict__ slotpos, const uint64_t* __restrict__ st,
                                                 uint32_t* __restrict__ prevpos, uint32_t* __restrict__ nxt_c) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (st[ST_ADDS] == 0 || i >= n) return;
    uint32_t pp = kNone;
    if (op_b[i] == OP_IGNORE) {
        pp = kInvalid;
    } else if (old_slot[i] != kNone) {
        const uint32_t cp = slotpos[old_slot[i]];
        if (cp != kNone) {
            pp = cp;
            nxt_c[cp] = i;
        } else {
            pp = kAlways;
        }
    }
    prevpos[i] = pp;
}

// k_ev_serial with an operation per entry.  The queue's batch part is read from live_b (written by the stepping lane in
// earlier rounds, and patched into the staged window when the element lies inside it).
__global__ __launch_bounds__(256) void k_ra_serial(const uint32_t* __restrict__ nxt_c, const uint8_t* __restrict__ op_b,
                                                   const uint32_t* __restrict__ prevpos, uint32_t n, uint64_t capacity,
                                                   uint64_t* __restrict__ cnt, uint64_t* __restrict__ st, uint8_t* __restrict__ ev_c,
                                                   uint8_t* __restrict__ ev_b, uint32_t* live_b, uint8_t* __restrict__ present_b) {
    __shared__ uint32_t qbuf[kChunk], bbuf[kChunk];
    __shared__ uint8_t obuf[kChunk];
    __shared__ uint32_t s_p, s_i, s_done;
    __shared__ uint64_t s_c, s_ev;
    if (st[ST_ADDS] == 0) return;  // nothing can be evicted: every operation finds what the table held before the call
    const uint32_t ncand = (uint32_t)st[ST_NCAND];
    const uint64_t entries0 = cnt[0];
    const uint64_t Q = (uint64_t)ncand + n;
    if (threadIdx.x == 0) {
        s_p = 0;
        s_i = 0;
        s_done = 0;
        s_c = entries0;
        s_ev = 0;
    }
    __syncthreads();
    const uint64_t max_rounds = (Q + n) / kChunk + 4;
    for (uint64_t round = 0; round < max_rounds; ++round) {
        const uint32_t q0 = s_p, b0 = s_i;
        if (s_done || b0 >= n) break;
        for (uint32_t t = threadIdx.x; t < kChunk; t += 256u) {
            const uint64_t q = (uint64_t)q0 + t;
            uint32_t v = kInvalid;
            if (q < ncand)
                v = nxt_c[q];
            else if (q < Q && __hip_atomic_load(&live_b[q - ncand], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                v = kNone;
            qbuf[t] = v;
            const uint64_t b = (uint64_t)b0 + t;
            bbuf[t] = b < n ? prevpos[b] : kInvalid;
            obuf[t] = b < n ? op_b[b] : (uint8_t)OP_IGNORE;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t p = q0, i = b0;
            uint64_t c = s_c, ev = s_ev;
            bool stop = false, bad = false;
            while (i < n && i - b0 < kChunk && !stop) {
                const uint32_t pp = bbuf[i - b0];
                const uint32_t op = obuf[i - b0];
                if (op == OP_IGNORE) {
                    ++i;
                    continue;
                }
                while (op == OP_ADD && c >= capacity && !stop) {  // AdjustSize
                    // advance over batch elements that are not live and over candidates an operation before i took
                    while (p - q0 < kChunk && p < Q && (qbuf[p - q0] == kInvalid || qbuf[p - q0] < i)) ++p;
                    if (p >= Q || (p >= ncand && p - ncand >= i) || (p >= ncand && ncand < entries0)) {
                        bad = stop = true;  // nothing left to evict / the pointer left the candidates
                    } else if (p - q0 >= kChunk) {
                        stop = true;  // refill the queue window, then resume at this entry
                    } else {
                        if (p < ncand) ev_c[p] = 1; else ev_b[p - ncand] = 1;
                        ++p;
                        --c;
                        ++ev;
                    }
                }
                if (stop) break;
                const bool present = pp != kNone && (pp == kAlways || pp >= p);
                bool live = false;
                if (op == OP_ADD) {
                    live = true;
                    if (!present) ++c;
                } else if (op == OP_REMOVE) {
                    if (present) --c;
                } else {
                    live = present;
                }
                present_b[i] = present ? 1 : 0;
                if (live) {
                    __hip_atomic_store(&live_b[i], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint64_t qp = (uint64_t)ncand + i;
                    if (qp >= q0 && qp - q0 < kChunk) qbuf[qp - q0] = kNone;
                }
                ++i;
            }
            s_p = p;
            s_i = i;
            s_c = c;
            s_ev = ev;
            if (bad) {
                raise(cnt, kErrInvariant);
                s_done = 1;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (!s_done && s_i < n) raise(cnt, kErrInvariant);  // the round bound ran out
        st[ST_FINAL] = s_c;
        st[ST_EVICTED] = s_ev;
        cnt[3] += s_ev;
    }
}

// The apply of everything but the inserts: tombstones (a REMOVE's entry, the old slot of an evicted ADD or FRESH), the
// state change of MarkAsFresh, `keep` for k_ev_insert, d_present.  serial == 0 (the host knows that nothing can be
// evicted) or no ADD in the response: the serial pass did not run, and an operation is present when its key had a slot.
__global__ __launch_bounds__(256) void k_ra_apply(DirSlot* __restrict__ cache, uint64_t mask, uint32_t n, const uint8_t* __restrict__ op_b,
                                                  const uint8_t* __restrict__ ev_b, const uint8_t* __restrict__ present_b,
                                                  const uint32_t* __restrict__ old_slot, const uint32_t* __restrict__ grp_b,
                                                  uint32_t* __restrict__ group_tab, uint8_t* __restrict__ keep,
                                                  uint8_t* __restrict__ d_present, uint64_t* __restrict__ cnt,
                                                  const uint64_t* __restrict__ st, uint32_t serial, int64_t now, int64_t max_ttl,
                                                  double growth) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool gone = false;
    if (i < n) {
        const uint32_t op = op_b[i];
        bool present = false, kept = false;
        if (op != OP_IGNORE) {
            group_tab[grp_b[i]] = kNone;  // the key's first occurrence leaves the claim table clean for the next call
            const bool ran = serial && st[ST_ADDS] != 0;
            const uint32_t os = old_slot[i];
            present = ran ? present_b[i] != 0 : os != kNone;
            const bool evicted = ran && ev_b[i];
            const bool full = os != kNone && cache[os].state == SLOT_FULL;  // not an evicted candidate (k_ev_tomb_c ran)
            if (op == OP_ADD) {
                if (evicted) gone = full; else kept = true;
            } else if (op == OP_REMOVE) {
                gone = full;
            } else if (present && full) {
                if (evicted)
                    gone = true;
                else
                    cache_mark_fresh_slot(cache, mask, os, cache_gens(cache, mask)[mask + 1] + i + 1ull, now, max_ttl, growth);
            }
            if (gone) cache[os].state = SLOT_TOMB;
        }
        keep[i] = kept ? 1 : 0;
        if (d_present) d_present[i] = present ? 1 : 0;
    }
    const int k = __syncthreads_count(gone ? 1 : 0);
    if (threadIdx.x == 0 && k) {
        add64(&cnt[0], ~(uint64_t)k + 1);
        add64(&cnt[1], (uint64_t)k);
    }
}

__global__ void k_ra_finish(DirSlot* __restrict__ cache, uint64_t mask, uint64_t n, uint64_t* __restrict__ cnt,
                            const uint64_t* __restrict__ st, uint32_t serial, uint64_t* __restrict__ d_counts) {
    if (threadIdx.x != 0) return;
    if (serial && st[ST_ADDS] != 0 && cnt[0] != st[ST_FINAL]) raise(cnt, kErrInvariant);  // as k_ev_finish
    cache_gens(cache, mask)[mask + 1] += n;
    if (d_counts) {
        const uint64_t a = st[ST_ADDS], r = st[ST_REMOVES], f = st[ST_FRESHES];
        d_counts[0] = a;
        d_counts[1] = r;
        d_counts[2] = f;
        d_counts[3] = n - a - r - f;
    }
}

inline uint32_t blocks(uint64_t n) { return (uint32_t)((n + 255) / 256); }

size_t carve(size_t& off, size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) & ~(size_t)255;
    return at;
}

}  // namespace

int cache_evict_alloc(CacheEvictScratch* s, uint64_t max_batch, uint64_t slots) {
    cache_evict_free(s);
    const uint64_t mb = max_batch ? max_batch : 1;
    uint64_t groups = 2;
    while (groups < 2 * mb) groups <<= 1;
    const uint64_t ncap = std::min<uint64_t>(2 * mb, slots);
    const uint32_t ntiles = (uint32_t)((slots + kEvTile - 1) / kEvTile);
    size_t t1 = 0, t2 = 0;
    hipError_t e = rocprim::radix_sort_keys(nullptr, t1, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)mb, 0u, 64u,
                                            (hipStream_t)0);
    if (e == hipSuccess)
        e = rocprim::radix_sort_pairs(nullptr, t2, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                      (uint32_t*)nullptr, (size_t)ncap, 0u, 64u, (hipStream_t)0);
    if (e != hipSuccess) return (int)e;
    const size_t temp = std::max(t1, t2) + 256;
    size_t off = 0;
    const size_t o_old = carve(off, mb * 4), o_gk = carve(off, mb * 8), o_gks = carve(off, mb * 8), o_pb = carve(off, mb * 4),
                 o_nb = carve(off, mb * 4), o_pp = carve(off, mb * 4), o_eb = carve(off, mb), o_kp = carve(off, mb),
                 o_gt = carve(off, groups * 4), o_cs = carve(off, ncap * 8), o_css = carve(off, ncap * 8),
                 o_cl = carve(off, ncap * 4), o_cls = carve(off, ncap * 4), o_nc = carve(off, ncap * 4), o_ec = carve(off, ncap),
                 o_sk = carve(off, slots * 8), o_sp = carve(off, slots * 4), o_tc = carve(off, (size_t)ntiles * 4),
                 o_st = carve(off, 16 * 8), o_h = carve(off, 256 * 4), o_tmp = carve(off, temp), o_gb = carve(off, mb * 4),
                 o_lb = carve(off, mb * 4), o_ob = carve(off, mb), o_prb = carve(off, mb);
    uint8_t* b = nullptr;
    if ((e = hipMalloc((void**)&b, off)) != hipSuccess) return (int)e;
    s->base = b;
    s->max_batch = mb;
    s->slots = slots;
    s->group_mask = (uint32_t)(groups - 1);
    s->ntiles = ntiles;
    s->old_slot = (uint32_t*)(b + o_old); s->gkey = (uint64_t*)(b + o_gk); s->gkey_sorted = (uint64_t*)(b + o_gks);
    s->prev_b = (uint32_t*)(b + o_pb); s->nxt_b = (uint32_t*)(b + o_nb); s->prevpos = (uint32_t*)(b + o_pp);
    s->ev_b = b + o_eb; s->keep = b + o_kp; s->group_tab = (uint32_t*)(b + o_gt);
    s->cand_stamp = (uint64_t*)(b + o_cs); s->cand_stamp_s = (uint64_t*)(b + o_css);
    s->cand_slot = (uint32_t*)(b + o_cl); s->cand_slot_s = (uint32_t*)(b + o_cls); s->nxt_c = (uint32_t*)(b + o_nc);
    s->ev_c = b + o_ec; s->skey = (uint64_t*)(b + o_sk); s->slotpos = (uint32_t*)(b + o_sp); s->tile_cnt = (uint32_t*)(b + o_tc);
    s->st = (uint64_t*)(b + o_st); s->hist = (uint32_t*)(b + o_h); s->sort_temp = b + o_tmp; s->sort_temp_bytes = temp;
    s->grp_b = (uint32_t*)(b + o_gb); s->live_b = (uint32_t*)(b + o_lb); s->op_b = b + o_ob; s->present_b = b + o_prb;
    if ((e = hipMemset(b, 0, off)) != hipSuccess) return (int)e;
    if ((e = hipMemset(s->group_tab, 0xFF, groups * 4)) != hipSuccess) return (int)e;
    if ((e = hipMemset(s->slotpos, 0xFF, slots * 4)) != hipSuccess) return (int)e;
    return 0;
}

void cache_evict_free(CacheEvictScratch* s) {
    if (s->base) (void)hipFree(s->base);
    *s = CacheEvictScratch{};
}

int launch_cache_rebuild(const DirSlot* d_src, DirSlot* d_dst, uint64_t mask, uint64_t* d_cnt, const CacheEvictScratch& s,
                         void* stream, bool adaptive) {
    hipStream_t st = (hipStream_t)stream;
    const uint64_t slots = mask + 1;
    hipError_t e = hipMemsetAsync(d_dst, 0, slots * sizeof(DirSlot) + (slots + 1) * 8, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_rb_begin, dim3(1), dim3(64), 0, st, s.st);
    hipLaunchKernelGGL(k_rb_move, dim3(blocks(slots)), dim3(256), 0, st, d_src, d_dst, mask, s.st, d_cnt,
                       adaptive ? 1u : 0u);
    hipLaunchKernelGGL(k_rb_finish, dim3(1), dim3(64), 0, st, d_src, d_dst, mask, s.st, d_cnt);
    return (int)hipGetLastError();
}

int launch_cache_evict_add(DirSlot* d_cache, uint64_t mask, DirSlot* d_rebuild_into, uint64_t* d_cnt, uint64_t capacity,
                           const orl_grain_key* d_keys, const uint32_t* d_acts, const uint8_t* d_silos, size_t n,
                           uint32_t n_act, uint32_t n_silos, const uint32_t* d_local, const CacheEvictScratch& s, void* stream,
                           const CacheFresh& fresh) {
    hipStream_t st = (hipStream_t)stream;
    const uint64_t slots = mask + 1;
    if (n == 0) return 0;
    if (n > s.max_batch || slots != s.slots) return (int)hipErrorInvalidValue;
    const uint32_t un = (uint32_t)n;
    const uint32_t ncap = (uint32_t)std::min<uint64_t>(2 * (uint64_t)n, slots);
    const dim3 b(256), gn(blocks(n)), gc(blocks(ncap)), gs(blocks(slots)), gt(s.ntiles);
    hipError_t e;
    size_t tb = 0, tb2 = 0;
    // the sorts' temporary storage was sized for max_batch by cache_evict_alloc: checked before anything is enqueued
    if ((e = rocprim::radix_sort_keys(nullptr, tb, s.gkey, s.gkey_sorted, n, 0u, 64u, st)) != hipSuccess) return (int)e;
    if ((e = rocprim::radix_sort_pairs(nullptr, tb2, s.cand_stamp, s.cand_stamp_s, s.cand_slot, s.cand_slot_s, (size_t)ncap, 0u,
                                       64u, st)) != hipSuccess)
        return (int)e;
    if (tb > s.sort_temp_bytes || tb2 > s.sort_temp_bytes) return (int)hipErrorOutOfMemory;

    hipLaunchKernelGGL(k_ev_fill, dim3(blocks(std::max<uint32_t>(ncap, 16))), b, 0, st, ncap, s.cand_stamp, s.cand_slot, s.nxt_c,
                       s.ev_c, s.st);
    hipLaunchKernelGGL(k_ev_prep, gn, b, 0, st, d_cache, mask, d_keys, d_acts, d_silos, un, n_act, n_silos, d_local, s.group_tab,
                       s.group_mask, s.old_slot, s.gkey, s.prev_b, s.nxt_b, s.ev_b, s.st, d_cnt);
    tb = s.sort_temp_bytes;
    if ((e = rocprim::radix_sort_keys(s.sort_temp, tb, s.gkey, s.gkey_sorted, n, 0u, 64u, st)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_ev_link, gn, b, 0, st, s.gkey_sorted, un, s.prev_b, s.nxt_b, s.group_tab);

    hipLaunchKernelGGL(k_ev_snapshot, gs, b, 0, st, d_cache, mask, s.skey, s.st, s.hist, d_cnt);
    const dim3 gh(std::min<uint32_t>(blocks(slots), 2048));
    for (int pass = 7; pass >= 0; --pass) {  // 64-bit stamps, eight 8-bit digits from the top
        hipLaunchKernelGGL(k_ev_hist, gh, b, 0, st, s.skey, slots, (uint32_t)pass * 8u, s.st, s.hist);
        hipLaunchKernelGGL(k_ev_pick, dim3(1), b, 0, st, s.st, s.hist, (uint32_t)pass * 8u, d_cnt);
    }
    hipLaunchKernelGGL(k_ev_ccount, gt, b, 0, st, s.skey, slots, s.st, s.tile_cnt);
    hipLaunchKernelGGL(k_ev_cscan, dim3(1), b, 0, st, s.tile_cnt, s.ntiles, s.st, ncap, d_cnt);
    hipLaunchKernelGGL(k_ev_cemit, gt, b, 0, st, s.skey, slots, s.st, s.tile_cnt, s.cand_stamp, s.cand_slot, ncap);
    tb = s.sort_temp_bytes;
    if ((e = rocprim::radix_sort_pairs(s.sort_temp, tb, s.cand_stamp, s.cand_stamp_s, s.cand_slot, s.cand_slot_s, (size_t)ncap,
                                       0u, 64u, st)) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_ev_mark, gc, b, 0, st, s.cand_slot_s, s.st, s.slotpos, slots);
    hipLaunchKernelGGL(k_ev_prev, gn, b, 0, st, un, s.prev_b, s.nxt_b, s.old_slot, s.slotpos, s.st, s.prevpos, s.nxt_c);

    hipLaunchKernelGGL(k_ev_serial, dim3(1), b, 0, st, s.nxt_c, s.nxt_b, s.prevpos, un, capacity, d_cnt, s.st, s.ev_c, s.ev_b);

    hipLaunchKernelGGL(k_ev_tomb_c, gc, b, 0, st, d_cache, slots, s.cand_slot_s, s.ev_c, s.st, s.slotpos, d_cnt);
    hipLaunchKernelGGL(k_ev_tomb_b, gn, b, 0, st, d_cache, un, s.nxt_b, s.ev_b, s.old_slot, s.keep, d_cnt);
    DirSlot* into = d_cache;
    if (d_rebuild_into) {
        if (int r = launch_cache_rebuild(d_cache, d_rebuild_into, mask, d_cnt, s, stream, fresh.on != 0)) return r;
        into = d_rebuild_into;
    }
    hipLaunchKernelGGL(k_ev_insert, gn, b, 0, st, into, mask, d_keys, d_acts, d_silos, un, s.keep, d_cnt, fresh);
    hipLaunchKernelGGL(k_ev_finish, dim3(1), dim3(64), 0, st, into, mask, (uint64_t)n, d_cnt, s.st);
    return (int)hipGetLastError();
}

int launch_cache_apply_refresh(DirSlot* d_cache, uint64_t mask, DirSlot* d_rebuild_into, uint64_t* d_cnt, uint64_t capacity,
                               const orl_grain_key* d_keys, const uint32_t* d_acts, const uint8_t* d_silos, size_t n,
                               uint32_t n_act, uint32_t n_silos, const uint32_t* d_local, const CacheEvictScratch& s,
                               void* stream, const CacheFresh& fresh, const CacheRefresh& rf, bool may_evict) {
    hipStream_t st = (hipStream_t)stream;
    const uint64_t slots = mask + 1;
    if (n == 0) return rf.counts ? (int)hipMemsetAsync(rf.counts, 0, 4 * 8, st) : 0;
    if (n > s.max_batch || slots != s.slots || !fresh.on) return (int)hipErrorInvalidValue;
    const uint32_t un = (uint32_t)n;
    const uint32_t ncap = may_evict ? (uint32_t)std::min<uint64_t>(2 * (uint64_t)n, slots) : 0u;  // n_add + n_ops <= 2 n
    const dim3 b(256), gn(blocks(n)), gc(blocks(std::max<uint32_t>(ncap, 1))), gs(blocks(slots)), gt(s.ntiles);
    hipError_t e;
    size_t tb = 0;
    if (may_evict) {  // the sort's temporary storage was sized for max_batch by cache_evict_alloc
        if ((e = rocprim::radix_sort_pairs(nullptr, tb, s.cand_stamp, s.cand_stamp_s, s.cand_slot, s.cand_slot_s, (size_t)ncap, 0u,
                                           64u, st)) != hipSuccess)
            return (int)e;
        if (tb > s.sort_temp_bytes) return (int)hipErrorOutOfMemory;
    }
    hipLaunchKernelGGL(k_ev_fill, dim3(blocks(std::max<uint32_t>(ncap, 16))), b, 0, st, ncap, s.cand_stamp, s.cand_slot, s.nxt_c,
                       s.ev_c, s.st);
    hipLaunchKernelGGL(k_ra_prep, gn, b, 0, st, d_cache, mask, d_keys, rf.kind, d_acts, d_silos, un, n_act, n_silos, d_local,
                       s.group_tab, s.group_mask, s.old_slot, s.grp_b, s.op_b, d_cnt);
    hipLaunchKernelGGL(k_ra_resolve, gn, b, 0, st, un, s.group_tab, s.grp_b, s.op_b, s.ev_b, s.live_b, s.present_b, s.st);
    if (may_evict) {
        hipLaunchKernelGGL(k_ra_snapshot, gs, b, 0, st, d_cache, mask, s.skey, s.st, s.hist, d_cnt);
        const dim3 gh(std::min<uint32_t>(blocks(slots), 2048));
        for (int pass = 7; pass >= 0; --pass) {  // each leaves at once when K = 0
            hipLaunchKernelGGL(k_ev_hist, gh, b, 0, st, s.skey, slots, (uint32_t)pass * 8u, s.st, s.hist);
            hipLaunchKernelGGL(k_ev_pick, dim3(1), b, 0, st, s.st, s.hist, (uint32_t)pass * 8u, d_cnt);
        }
        hipLaunchKernelGGL(k_ev_ccount, gt, b, 0, st, s.skey, slots, s.st, s.tile_cnt);
        hipLaunchKernelGGL(k_ev_cscan, dim3(1), b, 0, st, s.tile_cnt, s.ntiles, s.st, ncap, d_cnt);
        hipLaunchKernelGGL(k_ev_cemit, gt, b, 0, st, s.skey, slots, s.st, s.tile_cnt, s.cand_stamp, s.cand_slot, ncap);
        tb = s.sort_temp_bytes;
        if ((e = rocprim::radix_sort_pairs(s.sort_temp, tb, s.cand_stamp, s.cand_stamp_s, s.cand_slot, s.cand_slot_s, (size_t)ncap,
                                           0u, 64u, st)) != hipSuccess)
            return (int)e;
        hipLaunchKernelGGL(k_ev_mark, gc, b, 0, st, s.cand_slot_s, s.st, s.slotpos, slots);
        hipLaunchKernelGGL(k_ra_prev, gn, b, 0, st, un, s.op_b, s.old_slot, s.slotpos, s.st, s.prevpos, s.nxt_c);
        hipLaunchKernelGGL(k_ra_serial, dim3(1), b, 0, st, s.nxt_c, s.op_b, s.prevpos, un, capacity, d_cnt, s.st, s.ev_c, s.ev_b,
                           s.live_b, s.present_b);
        hipLaunchKernelGGL(k_ev_tomb_c, gc, b, 0, st, d_cache, slots, s.cand_slot_s, s.ev_c, s.st, s.slotpos, d_cnt);
    }
    const uint32_t serial = may_evict ? 1u : 0u;
    hipLaunchKernelGGL(k_ra_apply, gn, b, 0, st, d_cache, mask, un, s.op_b, s.ev_b, s.present_b, s.old_slot, s.grp_b, s.group_tab,
                       s.keep, rf.present, d_cnt, s.st, serial, fresh.now, rf.max_ttl, rf.growth);
    DirSlot* into = d_cache;
    if (d_rebuild_into) {
        if (int r = launch_cache_rebuild(d_cache, d_rebuild_into, mask, d_cnt, s, stream, true)) return r;
        into = d_rebuild_into;
    }
    hipLaunchKernelGGL(k_ev_insert, gn, b, 0, st, into, mask, d_keys, d_acts, d_silos, un, s.keep, d_cnt, fresh);
    hipLaunchKernelGGL(k_ra_finish, dim3(1), dim3(64), 0, st, into, mask, (uint64_t)n, d_cnt, s.st, serial, rf.counts);
    return (int)hipGetLastError();
}

}  // namespace orl
