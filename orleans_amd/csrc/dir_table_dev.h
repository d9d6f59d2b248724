// dir_table_dev.h — device-side helpers of the directory tables (partition, directory cache, KeyExt table), shared by
// the .hip files: the ring search, the slot accessors, the read-only chain walk and the lock-free claim loop, each
// written once.  Device code only: the host side (orl_api.cpp, orl_node.cpp) does not include it.
#pragma once

#include <hip/hip_runtime.h>

#include "orl_internal.h"

namespace orl {

namespace {

__device__ __forceinline__ bool mask_bit(const uint32_t* m, uint32_t i) { return (m[i >> 5] >> (i & 31u)) & 1u; }

// Cooperative copy of the launch parameters into LDS (1.8 KB, 16-B granules).
__device__ __forceinline__ void stage_params(RouteParams* sp, const RouteParams* __restrict__ gp) {
    const uint4* src = reinterpret_cast<const uint4*>(gp);
    uint4* dst = reinterpret_cast<uint4*>(sp);
    for (uint32_t i = threadIdx.x; i < sizeof(RouteParams) / 16; i += blockDim.x) dst[i] = src[i];
}

__device__ __forceinline__ void add64(uint64_t* p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

// Directory owner of a non-special grain: LocalGrainDirectory.CalculateTargetSilo(:466-494).
// Ring sorted ascending by signed hash; FindLast(hash_s <= h && !(s == me && excludeMySelf)) is the
// upper bound minus one, stepped back over the (single) excluded entry; none found → wrap to ring[n-1]
// (ring[n-2] if that is the excluded me, null if n == 1).  Returns 0xFF for null.
__device__ __forceinline__ uint32_t ring_owner(const RouteParams& P, int32_t h, uint32_t me, bool exclude_me) {
    const int n = (int)P.ring_n;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (P.ring_hash[mid] <= h) lo = mid + 1; else hi = mid;
    }
    int idx = lo - 1;
    if (idx >= 0 && exclude_me && P.ring_silo[idx] == me) --idx;
    if (idx < 0) {
        idx = n - 1;
        if (exclude_me && P.ring_silo[idx] == me) {
            if (n > 1) idx = n - 2; else return 0xFFu;
        }
    }
    return P.ring_silo[idx];
}

// LocalGrainDirectory.CalculateTargetSilo (LocalGrainDirectory.cs:439-497) of a grain with a 24-B key, for caller `me`:
// the membership-table grain is the seed's, an empty ring is the caller's (null while it is excluded), else ring_owner.
// 0xFF = null (and the membership grain without a seed, which the reference throws on).  Its callers differ in two
// things, kept as they were:
//   SYSTEM_TARGETS  a system target is the caller's own (the cache's maintainer and AdjustLocalCache walk entries of
//                   any category; registration and the hand-off split reject or never hold system targets);
//   excl_opt        excludeThisSiloIfStopping: `me` is excluded while it is not running (always set for a registering
//                   silo, RegisterSingleActivationAsync :510-544, and for the split; the caller's option for the cache).
template <bool SYSTEM_TARGETS>
__device__ __forceinline__ uint32_t target_silo(const RouteParams& P, uint64_t tcd, uint64_t n0, uint64_t n1, uint32_t me,
                                                bool excl_opt) {
    if (SYSTEM_TARGETS && (uint32_t)(tcd >> 56) == ORL_CAT_SYSTEM_TARGET) return me;
    if (tcd == P.mem_tcd && n0 == P.mem_n0 && n1 == P.mem_n1) return P.seed;
    const uint32_t h = jenkins3(tcd, n0, n1);
    const bool exclude_me = excl_opt && !mask_bit(P.running, me);
    if (P.ring_n == 0) return exclude_me ? 0xFFu : me;
    return ring_owner(P, (int32_t)h, me, exclude_me);
}

// Jenkins lookup2 over the virtual byte string {N0, N1, TCD (LE8 each), len (LE4), s[0, len)}: the uniform hash of a
// KeyExt grain (UniqueKey.cs:288-294, JenkinsHash.cs:68-115).
__device__ uint32_t keyext_hash_dev(uint64_t n0, uint64_t n1, uint64_t tcd, const uint8_t* __restrict__ s, uint32_t len) {
    auto at = [&](uint32_t k) -> uint32_t {
        if (k < 8) return (uint32_t)(n0 >> (8 * k)) & 0xFFu;
        if (k < 16) return (uint32_t)(n1 >> (8 * (k - 8))) & 0xFFu;
        if (k < 24) return (uint32_t)(tcd >> (8 * (k - 16))) & 0xFFu;
        if (k < 28) return (len >> (8 * (k - 24))) & 0xFFu;
        return s[k - 28];
    };
    auto rd = [&](uint32_t k) { return at(k) | at(k + 1) << 8 | at(k + 2) << 16 | at(k + 3) << 24; };
    const uint32_t total = 28u + len;
    uint32_t a = 0x9e3779b9u, b = 0x9e3779b9u, c = 0, i = 0;
    for (; i + 12 <= total; i += 12) {
        a += rd(i);
        b += rd(i + 4);
        c += rd(i + 8);
        ORL_MIX(a, b, c);
    }
    c += total;
    for (uint32_t k = 0; i + k < total; ++k) {
        const uint32_t v = at(i + k);
        if (k < 4) a += v << (8 * k);
        else if (k < 8) b += v << (8 * (k - 4));
        else c += v << (8 * (k - 7));
    }
    ORL_MIX(a, b, c);
    return c;
}

// ---- DirSlot accessors ----------------------------------------------------------------------------------------------
// COHERENT = agent-scope atomic loads (the slot may be another workgroup's write of this launch); else plain loads.

__device__ __forceinline__ uint32_t* slot_word28(const DirSlot* t, uint64_t slot) {
    return reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(const_cast<DirSlot*>(t + slot)) + 28);  // {silo, state, pad}
}
__device__ __forceinline__ uint32_t slot_state(const DirSlot* t, uint64_t slot) {
    return (__hip_atomic_load(slot_word28(t, slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 8) & 0xFFu;
}
template <bool COHERENT>
__device__ __forceinline__ bool slot_key_eq(const DirSlot* t, uint64_t slot, const orl_grain_key& k) {
    const uint64_t* w = reinterpret_cast<const uint64_t*>(t + slot);
    if (COHERENT)
        return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == k.type_code_data &&
               __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == k.n0 &&
               __hip_atomic_load(w + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == k.n1;
    return w[0] == k.type_code_data && w[1] == k.n0 && w[2] == k.n1;
}
__device__ __forceinline__ uint64_t key_start(const orl_grain_key& k, uint64_t mask) {
    return dir_slot(jenkins3(k.type_code_data, k.n0, k.n1), mask);
}

// The directory cache's LRU generations: the cache table of cmask + 1 slots is followed by one u64 generation per slot
// and the generation base G (gen[cmask + 1]).
__device__ __forceinline__ unsigned long long* cache_gens(const DirSlot* cache, uint64_t cmask) {
    return reinterpret_cast<unsigned long long*>(const_cast<DirSlot*>(cache + cmask + 1));
}

// The key's FULL slot (a read-only chain walk that stops at EMPTY), or ~0.
template <bool COHERENT>
__device__ __forceinline__ uint64_t find_full(const DirSlot* __restrict__ t, uint64_t mask, const orl_grain_key& k) {
    uint64_t cur = key_start(k, mask);
    for (uint64_t step = 0; step <= mask; ++step) {
        const uint32_t state = COHERENT ? slot_state(t, cur) : t[cur].state;
        if (state == SLOT_EMPTY) break;
        if (state == SLOT_FULL && slot_key_eq<COHERENT>(t, cur, k)) return cur;
        cur = (cur + 1) & mask;
    }
    return ~0ull;
}

// ---- the claim protocol (directory mutation, dir_mutate.hip) --------------------------------------------------------
constexpr uint32_t kSlotNone = 0xFFFFFFFFu;
constexpr uint32_t kSlotWasTomb = 0x80000000u;  // probe → commit: the claimed slot was a tombstone
constexpr uint32_t kSlotMask = 0x7FFFFFFFu;
constexpr uint8_t kInsCandidate = 0xFE;  // probe outcome: joined / claimed a slot (resolved by the resolve kernel)
constexpr uint32_t kRetryLimit = 1u << 22;

// Find a key on its chain (from `start`) or claim a slot for it: returns 0 = an equal FULL entry at slot_out, 1 = joined
// or claimed the slot slot_out (claim word atomicMin'ed with `tag`), -1 = no free slot, or the table could not take the
// key.  LAST_WINS (cache AddOrUpdate, merge) also claims a FULL entry, so the batch's owner of the key updates it.
// Table is the per-table part:
//   uint32_t* word(slot)        the u32 that holds the slot's state in bits 8-15
//   bool claimed_eq(slot)       a CLAIMED slot (possibly another workgroup's claim of this launch) holds the key
//   bool full_eq(slot)          a FULL slot holds the key
//   bool write_key(slot, word)  between CLAIMING and CLAIMED: the key, write-through; false = it could not (the table
//                               put `word`, the slot's word before the claim, back and recorded why): the probe gives up.
// A claim takes the first tombstone or the EMPTY end of the chain, once the whole chain shows the key absent (as the
// host mirror does).  Each attempt walks the chain without waiting; a lane that meets a slot some registration is still
// CLAIMING abandons the attempt and retries, and the claimer publishes within its own attempt, so lanes of one wave
// never wait on each other.
template <bool LAST_WINS, class Table>
__device__ __forceinline__ int find_or_claim(const Table& T, uint64_t start, uint64_t mask, uint32_t* __restrict__ claim,
                                             uint32_t tag, uint64_t& slot_out, bool& was_tomb_out) {
    int outcome = -1;  // 0 = existing FULL entry, 1 = candidate for a claimed slot
    uint64_t slot = start;
    bool was_tomb = false;
    for (uint32_t attempt = 0; outcome < 0 && attempt < kRetryLimit; ++attempt) {
        // one attempt: walk the chain to its end (EMPTY), looking for the key and remembering the first
        // reusable slot (tombstone or the EMPTY end); a slot another registration is still CLAIMING hides
        // its key, so the attempt is abandoned and retried (its owner publishes within its own iteration)
        uint64_t cur = start, free_slot = ~0ull;
        uint32_t free_word = 0;
        bool blocked = false, ended = false;
        for (uint64_t step = 0; step <= mask && outcome < 0 && !blocked && !ended; ++step) {
            const uint32_t v = __hip_atomic_load(T.word(cur), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t state = (v >> 8) & 0xFFu;
            if (state == SLOT_EMPTY || state == SLOT_TOMB) {
                if (free_slot == ~0ull) {
                    free_slot = cur;
                    free_word = v;
                }
                ended = state == SLOT_EMPTY;
            } else if (state == SLOT_CLAIMING) {
                blocked = true;
            } else if (state == SLOT_CLAIMED) {
                if (T.claimed_eq(cur)) {
                    atomicMin(&claim[cur], tag);
                    slot = cur;
                    outcome = 1;
                }
            } else if (T.full_eq(cur)) {  // FULL
                slot = cur;
                outcome = 0;
                if (LAST_WINS) atomicMin(&claim[cur], tag);  // an update of the present entry
            }
            cur = (cur + 1) & mask;
        }
        if (outcome >= 0) break;
        if (blocked || free_slot == ~0ull) {
            __builtin_amdgcn_s_sleep(1);
            continue;
        }
        uint32_t expect = free_word;
        if (__hip_atomic_compare_exchange_strong(T.word(free_slot), &expect, (uint32_t)SLOT_CLAIMING << 8, __ATOMIC_RELAXED,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            if (!T.write_key(free_slot, free_word)) break;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // key write-through before the state flips
            __hip_atomic_store(T.word(free_slot), (uint32_t)SLOT_CLAIMED << 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicMin(&claim[free_slot], tag);
            slot = free_slot;
            was_tomb = ((free_word >> 8) & 0xFFu) == SLOT_TOMB;
            outcome = 1;
        }  // else: another registration took that slot first: walk again
    }
    slot_out = slot;
    was_tomb_out = was_tomb;
    return outcome;
}

// The partition and the directory cache: 32-B slots keyed by the 24-B GrainId.
struct DirClaim {
    DirSlot* dir;
    const orl_grain_key& k;
    __device__ __forceinline__ uint32_t* word(uint64_t slot) const { return slot_word28(dir, slot); }
    __device__ __forceinline__ bool claimed_eq(uint64_t slot) const { return slot_key_eq<true>(dir, slot, k); }
    __device__ __forceinline__ bool full_eq(uint64_t slot) const { return slot_key_eq<false>(dir, slot, k); }
    __device__ __forceinline__ bool write_key(uint64_t slot, uint32_t) const {
        uint64_t* kw = reinterpret_cast<uint64_t*>(dir + slot);
        __hip_atomic_store(kw, k.type_code_data, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(kw + 1, k.n0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(kw + 2, k.n1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return true;
    }
};

}  // namespace

}  // namespace orl
