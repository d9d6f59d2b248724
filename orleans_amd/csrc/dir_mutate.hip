// dir_mutate.hip — directory mutation on the device (gfx950): registration, KeyExt registration, the directory cache's
// AddOrUpdate, the partition merge and unregistration, each as probe → resolve → commit over a batch.
//
// The batch gets the reference's sequential semantics, i.e. the result of applying it one message at a time in batch
// order.  Every message of one key meets in one slot of the table (the claim protocol, dir_table_dev.h find_or_claim),
// atomicMin on that slot's claim word picks the key's owner in the batch, and only the owner commits.  None of these
// kernels is on the routing hot path; they call no route or stage-4 code.
#include <hip/hip_runtime.h>

#include "dir_table_dev.h"

namespace orl {

namespace {

inline uint32_t blocks(uint64_t n) { return (uint32_t)((n + 255) / 256); }

// ---------------------------------------------------------------------------------------------------
// RegisterSingleActivation / Unregister batches with the reference's sequential semantics
// (GrainDirectoryPartition.AddSingleActivation, GrainDirectoryPartition.cs:270-287 + GrainInfo.AddSingleActivation
// :100-114: an existing instance wins; RemoveActivation :290-318):
//   probe   : each registration walks its key's probe chain; an equal FULL entry → EXISTING; an equal key just
//             claimed by another registration of this batch → join it; else claim the chain's first reusable slot.
//             Every registration of one key meets in one slot, and atomicMin on the slot's claim word keeps the
//             earliest batch index;
//   resolve : the earliest registration of a claimed key is INSERTED, later ones EXISTING with its activation;
//   commit  : the winner writes activation + silo + FULL and resets the claim word.
__global__ __launch_bounds__(256) void k_dir_ins_probe(const RouteParams* __restrict__ gp, DirSlot* __restrict__ dir, uint64_t mask,
                                                       uint32_t* __restrict__ claim, const orl_grain_key* __restrict__ keys,
                                                       const uint32_t* __restrict__ acts, const uint8_t* __restrict__ silos,
                                                       uint32_t n, uint32_t n_act, uint32_t n_silos, uint32_t* __restrict__ slot_out,
                                                       uint8_t* __restrict__ status, uint32_t* __restrict__ err,
                                                       const int32_t* __restrict__ tags) {
    __shared__ RouteParams P;
    stage_params(&P, gp);
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const orl_grain_key k = keys[i];
    const uint32_t silo = silos[i], cat = (uint32_t)(k.type_code_data >> 56);
    uint8_t st;
    if (acts[i] >= n_act || silo >= n_silos || cat == ORL_CAT_KEYEXT_GRAIN || cat == ORL_CAT_SYSTEM_TARGET ||
        (tags && tags[i] < 0)) {  // a versioned registration's draw is a Random.Next(): never negative
        st = ORL_INS_UNSUPPORTED;
    } else {
        // CalculateTargetSilo(grain, excludeThisSiloIfStopping = true) seen from the registering silo
        // (LocalGrainDirectory.RegisterSingleActivationAsync :510-544; the host mirror's host_owner)
        const uint32_t owner = target_silo<false>(P, k.type_code_data, k.n0, k.n1, silo, true);
        if (owner == 0xFFu) st = ORL_INS_OWNER_NULL;
        else if (!mask_bit(P.local, owner)) st = ORL_INS_REMOTE_OWNER;
        else if (!mask_bit(P.functional, silo)) st = ORL_INS_INVALID_SILO;  // AddSingleActivation :277-279
        else st = kInsCandidate;
    }
    uint32_t out_slot = kSlotNone;
    if (st == kInsCandidate) {
        uint64_t slot = 0;
        bool was_tomb = false;
        const int outcome = find_or_claim<false>(DirClaim{dir, k}, key_start(k, mask), mask, claim, i, slot, was_tomb);
        if (outcome < 0) {  // no free slot on the whole table (or a claim that never published)
            atomicOr(err, 1u);
            st = ORL_INS_UNSUPPORTED;
        } else {
            out_slot = (uint32_t)slot | (was_tomb ? kSlotWasTomb : 0u);
            st = outcome == 0 ? (uint8_t)ORL_INS_EXISTING : kInsCandidate;
        }
    }
    slot_out[i] = out_slot;
    status[i] = st;
}

__global__ __launch_bounds__(256) void k_dir_ins_resolve(const DirSlot* __restrict__ dir, const uint32_t* __restrict__ claim,
                                                         const uint32_t* __restrict__ acts, const uint8_t* __restrict__ silos,
                                                         uint32_t n, const uint32_t* __restrict__ slot_in,
                                                         uint8_t* __restrict__ status, uint32_t* __restrict__ wact,
                                                         uint8_t* __restrict__ wsilo, DirTags vt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint8_t st = status[i];
    const uint32_t slot = slot_in[i] & kSlotMask;
    uint32_t a = ORL_NO_ACT;
    uint8_t sl = (uint8_t)ORL_NULL_SILO;
    int32_t wt = ORL_DIR_NO_ETAG;
    if (st == kInsCandidate) {
        const uint32_t c = claim[slot];
        a = acts[c];
        sl = silos[c];
        if (vt.winner) wt = vt.in ? vt.in[c] : 0;  // the tag the slot's winner commits below
        status[i] = c == i ? (uint8_t)ORL_INS_INSERTED : (uint8_t)ORL_INS_EXISTING;
    } else if (st == ORL_INS_EXISTING) {
        a = dir[slot].act;
        sl = dir[slot].silo;
        if (vt.winner) wt = vt.slot[slot];  // an entry from before the batch: no registration changes its tag
    }
    if (wact) wact[i] = a;
    if (wsilo) wsilo[i] = sl;
    if (vt.winner) vt.winner[i] = wt;
}

__global__ __launch_bounds__(256) void k_dir_ins_commit(DirSlot* __restrict__ dir, uint32_t* __restrict__ claim,
                                                        const uint32_t* __restrict__ acts, const uint8_t* __restrict__ silos,
                                                        uint32_t n, const uint32_t* __restrict__ slot_in,
                                                        const uint8_t* __restrict__ status, uint64_t* __restrict__ cnt,
                                                        DirTags vt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || status[i] != ORL_INS_INSERTED) return;
    const uint32_t slot = slot_in[i] & kSlotMask;
    if (vt.slot) vt.slot[slot] = vt.in ? vt.in[i] : 0;  // VersionTag = rand.Next() (GrainInfo.AddSingleActivation :111)
    uint64_t* w24 = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(dir + slot) + 24);
    *w24 = (uint64_t)acts[i] | ((uint64_t)silos[i] << 32) | ((uint64_t)SLOT_FULL << 40);
    claim[slot] = kSlotNone;
    add64(cnt, 1);
    if (slot_in[i] & kSlotWasTomb) add64(cnt + 1, ~0ull);  // tombstones - 1
}

// ---------------------------------------------------------------------------------------------------
// KeyExt registration on the device (round 6, VERDICT r5 item 6: GrainDirectoryPartition.AddSingleActivation over any
// GrainId, GrainDirectoryPartition.cs:270-287, first writer wins, GrainInfo.AddSingleActivation :103-107).  The same claim
// protocol as k_dir_ins_* over the KeyExt table: the claimer writes the key, its hash, length and its string (appended to
// the table's string store at a 4-B aligned cursor) write-through before it publishes CLAIMED.
// state[0] = bytes used in the string store, [1] = entries, [2] = tombstones, [3] = error (no slot / store full).
__device__ __forceinline__ uint32_t* ext_word40(ExtSlot* t, uint64_t slot) {
    return reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(t + slot) + 40);  // {silo, state, pad, pad}
}

// The caller's string bytes [s, s + len) as little-endian word w (bytes past len read as 0).
__device__ __forceinline__ uint32_t ext_in_word(const uint8_t* __restrict__ s, uint32_t len, uint32_t w) {
    uint32_t v = 0;
    for (uint32_t b = 0; b < 4; ++b) {
        const uint32_t k = w * 4u + b;
        if (k < len) v |= (uint32_t)s[k] << (8u * b);
    }
    return v;
}

// The KeyExt table under the claim loop: 48-B slots keyed by the 24-B key, the hash, the length and the string's bytes.
struct ExtClaim {
    ExtSlot* table;
    uint8_t* tblob;
    uint64_t tblob_cap;
    unsigned long long* state;
    const orl_grain_key& k;
    uint32_t h;
    const uint8_t* s;  // the caller's string
    uint32_t len;

    __device__ __forceinline__ uint32_t* word(uint64_t slot) const { return ext_word40(table, slot); }
    // Write-through loads whatever the state: the slot may be another workgroup's claim of this launch.
    __device__ __forceinline__ bool claimed_eq(uint64_t slot) const {
        const uint64_t* w = reinterpret_cast<const uint64_t*>(table + slot);
        const uint32_t* w32 = reinterpret_cast<const uint32_t*>(table + slot);
        if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != k.type_code_data ||
            __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != k.n0 ||
            __hip_atomic_load(w + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != k.n1 ||
            __hip_atomic_load(w32 + 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != h ||
            __hip_atomic_load(w32 + 9, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != len)
            return false;
        const uint32_t off = __hip_atomic_load(w32 + 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t* tw = reinterpret_cast<const uint32_t*>(tblob + off);  // claims start 4-B aligned
        for (uint32_t q = 0; q * 4u < len; ++q) {
            const uint32_t have = __hip_atomic_load(tw + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t keep = len - q * 4u >= 4u ? 0xFFFFFFFFu : (1u << (8u * (len - q * 4u))) - 1u;
            if ((have & keep) != ext_in_word(s, len, q)) return false;
        }
        return true;
    }
    __device__ __forceinline__ bool full_eq(uint64_t slot) const { return claimed_eq(slot); }
    // Reserves the string's bytes in the store first; the host sized the store for the batch, so that never fails.
    __device__ __forceinline__ bool write_key(uint64_t slot, uint32_t word_before) const {
        const uint32_t padded = (len + 3u) & ~3u;
        const unsigned long long off = atomicAdd(&state[0], (unsigned long long)padded);
        if (off + padded > tblob_cap) {
            atomicOr(&state[3], 2ull);
            __hip_atomic_store(word(slot), word_before, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        uint32_t* tw = reinterpret_cast<uint32_t*>(tblob + off);
        for (uint32_t q = 0; q * 4u < len; ++q)
            __hip_atomic_store(tw + q, ext_in_word(s, len, q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint64_t* kw = reinterpret_cast<uint64_t*>(table + slot);
        uint32_t* k32 = reinterpret_cast<uint32_t*>(table + slot);
        __hip_atomic_store(kw, k.type_code_data, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(kw + 1, k.n0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(kw + 2, k.n1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(k32 + 6, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(k32 + 8, (uint32_t)off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(k32 + 9, len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return true;
    }
};

__global__ __launch_bounds__(256) void k_kx_ins_probe(const RouteParams* __restrict__ gp, ExtSlot* __restrict__ table,
                                                      uint64_t mask, uint32_t* __restrict__ claim, uint8_t* __restrict__ tblob,
                                                      uint64_t tblob_cap, const orl_grain_key* __restrict__ keys,
                                                      const orl_ext_ref* __restrict__ ext, const uint8_t* __restrict__ blob,
                                                      uint64_t blob_bytes, const uint32_t* __restrict__ acts,
                                                      const uint8_t* __restrict__ silos, uint32_t n, uint32_t n_act,
                                                      uint32_t n_silos, uint32_t* __restrict__ slot_out,
                                                      uint8_t* __restrict__ status, unsigned long long* __restrict__ state) {
    __shared__ RouteParams P;
    stage_params(&P, gp);
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const orl_grain_key k = keys[i];
    const orl_ext_ref x = ext[i];
    const uint32_t silo = silos[i];
    uint8_t st;
    uint32_t h = 0;
    if (acts[i] >= n_act || silo >= n_silos || (uint64_t)x.off + x.len > blob_bytes) {
        st = ORL_INS_UNSUPPORTED;
    } else if ((uint32_t)(k.type_code_data >> 56) != ORL_CAT_KEYEXT_GRAIN) {
        st = ORL_INS_UNSUPPORTED;
    } else {
        h = keyext_hash_dev(k.n0, k.n1, k.type_code_data, blob + x.off, x.len);
        const bool running = mask_bit(P.running, silo);  // CalculateTargetSilo(excludeThisSiloIfStopping) from `silo`
        const uint32_t owner = P.ring_n == 0 ? (running ? silo : 0xFFu) : ring_owner(P, (int32_t)h, silo, !running);
        if (owner == 0xFFu) st = ORL_INS_OWNER_NULL;
        else if (!mask_bit(P.local, owner)) st = ORL_INS_REMOTE_OWNER;
        else if (!mask_bit(P.functional, silo)) st = ORL_INS_INVALID_SILO;  // AddSingleActivation :277-279
        else st = kInsCandidate;
    }
    uint32_t out_slot = kSlotNone;
    if (st == kInsCandidate) {
        uint64_t slot = 0;
        bool was_tomb = false;
        const ExtClaim T{table, tblob, tblob_cap, state, k, h, blob + x.off, x.len};
        const int outcome = find_or_claim<false>(T, dir_slot(h, mask), mask, claim, i, slot, was_tomb);
        if (outcome < 0) {
            atomicOr(&state[3], 1ull);
            st = ORL_INS_UNSUPPORTED;
        } else {
            out_slot = (uint32_t)slot | (was_tomb ? kSlotWasTomb : 0u);
            st = outcome == 0 ? (uint8_t)ORL_INS_EXISTING : kInsCandidate;
        }
    }
    slot_out[i] = out_slot;
    status[i] = st;
}

__global__ __launch_bounds__(256) void k_kx_ins_resolve(const ExtSlot* __restrict__ table, const uint32_t* __restrict__ claim,
                                                        const uint32_t* __restrict__ acts, const uint8_t* __restrict__ silos,
                                                        uint32_t n, const uint32_t* __restrict__ slot_in,
                                                        uint8_t* __restrict__ status, uint32_t* __restrict__ wact,
                                                        uint8_t* __restrict__ wsilo) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint8_t st = status[i];
    const uint32_t slot = slot_in[i] & kSlotMask;
    uint32_t a = ORL_NO_ACT;
    uint8_t sl = (uint8_t)ORL_NULL_SILO;
    if (st == kInsCandidate) {
        const uint32_t c = claim[slot];
        a = acts[c];
        sl = silos[c];
        status[i] = c == i ? (uint8_t)ORL_INS_INSERTED : (uint8_t)ORL_INS_EXISTING;
    } else if (st == ORL_INS_EXISTING) {
        a = table[slot].act;
        sl = table[slot].silo;
    }
    if (wact) wact[i] = a;
    if (wsilo) wsilo[i] = sl;
}

__global__ __launch_bounds__(256) void k_kx_ins_commit(ExtSlot* __restrict__ table, uint32_t* __restrict__ claim,
                                                       const uint32_t* __restrict__ acts, const uint8_t* __restrict__ silos,
                                                       uint32_t n, const uint32_t* __restrict__ slot_in,
                                                       const uint8_t* __restrict__ status, unsigned long long* __restrict__ state) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || status[i] != ORL_INS_INSERTED) return;
    const uint32_t slot = slot_in[i] & kSlotMask;
    table[slot].act = acts[i];
    *ext_word40(table, slot) = (uint32_t)silos[i] | ((uint32_t)SLOT_FULL << 8);
    claim[slot] = kSlotNone;
    atomicAdd(&state[1], 1ull);
    if (slot_in[i] & kSlotWasTomb) atomicAdd(&state[2], ~0ull);  // tombstones - 1
}

// ---------------------------------------------------------------------------------------------------
// Directory cache AddOrUpdate (AdaptiveGrainDirectoryCache.AddOrUpdate; f4): the batch's LAST writer of a key
// sets its entry (insert or update).  Claim tag = ~index, so atomicMin keeps the largest index.  Entries with an
// activation handle >= n_act or a silo outside the table are skipped.
// An entry is kept when its silo is known and its handle is in this context's space [0, n_act) — or, for a silo this
// context does not host (`local`, a node's other ranks), any handle but ORL_NO_ACT: the host rank's catalog numbers it
// (round 5: the node exchange delivers cached messages to that rank, whose stage 4 buckets them).
__global__ __launch_bounds__(256) void k_cache_probe(DirSlot* __restrict__ cache, uint64_t mask, uint32_t* __restrict__ claim,
                                                     const orl_grain_key* __restrict__ keys, const uint32_t* __restrict__ acts,
                                                     const uint8_t* __restrict__ silos, uint32_t n, uint32_t n_act,
                                                     uint32_t n_silos, const uint32_t* __restrict__ local,
                                                     uint32_t* __restrict__ slot_out, uint32_t* __restrict__ err) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t out = kSlotNone;
    const uint32_t sl = silos[i];
    if (sl < n_silos && (acts[i] < n_act || (acts[i] != ORL_NO_ACT && !mask_bit(local, sl)))) {
        uint64_t slot = 0;
        bool was_tomb = false;
        if (find_or_claim<true>(DirClaim{cache, keys[i]}, key_start(keys[i], mask), mask, claim, ~i, slot, was_tomb) >= 0)
            out = (uint32_t)slot | (was_tomb ? kSlotWasTomb : 0u);
        else
            atomicOr(err, 1u);
    }
    slot_out[i] = out;
}

__global__ __launch_bounds__(256) void k_cache_resolve(const uint32_t* __restrict__ claim, uint32_t n, const uint32_t* __restrict__ slot_in,
                                                       uint8_t* __restrict__ win) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t sl = slot_in[i];
    win[i] = (sl != kSlotNone && claim[sl & kSlotMask] == ~i) ? 1u : 0u;
}

// The winner (the batch's last writer i of its key) also stamps the entry's LRU generation G + i + 1 (LRU.Add: a new
// TimestampedValue takes the next generation, LRU.cs:104-108); G advances by n afterwards (k_gen_advance).
__global__ __launch_bounds__(256) void k_cache_commit(DirSlot* __restrict__ cache, uint32_t* __restrict__ claim,
                                                      const uint32_t* __restrict__ acts, const uint8_t* __restrict__ silos, uint32_t n,
                                                      const uint32_t* __restrict__ slot_in, const uint8_t* __restrict__ win,
                                                      uint64_t* __restrict__ cnt, uint64_t mask, CacheFresh fresh_state) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || !win[i]) return;
    const uint32_t slot = slot_in[i] & kSlotMask;
    unsigned long long* gen = cache_gens(cache, mask);
    const unsigned long long stamp = gen[mask + 1] + i + 1ull;
    gen[slot] = stamp;
    if (fresh_state.on) {  // adaptive cache: a new GrainDirectoryCacheEntry (AdaptiveGrainDirectoryCache.cs:50-58, 97-103)
        const CacheAdaptive a = cache_adaptive(cache, mask);
        a.etag[slot] = fresh_state.etags ? fresh_state.etags[i] : 0;
        a.ttl[slot] = fresh_state.initial_ttl;
        a.last_refreshed[slot] = fresh_state.now;
        a.seen[slot] = stamp;
    }
    const bool fresh = cache[slot].state == SLOT_CLAIMED;  // a new entry (else an update of a FULL one)
    uint64_t* w24 = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(cache + slot) + 24);
    *w24 = (uint64_t)acts[i] | ((uint64_t)silos[i] << 32) | ((uint64_t)SLOT_FULL << 40);
    claim[slot] = kSlotNone;
    if (fresh) {
        add64(cnt, 1);
        if (slot_in[i] & kSlotWasTomb) add64(cnt + 1, ~0ull);
    }
}

// The cache's generation base after a batch that stamped generations (lookups or adds): G += the batch size.
__global__ void k_gen_advance(unsigned long long* __restrict__ g, uint64_t n) {
    if (threadIdx.x == 0) *g += n;
}

// ---------------------------------------------------------------------------------------------------
// Merge of a partition copy (GrainDirectoryPartition.Merge, GrainDirectoryPartition.cs:366-383, on
// ProcessSiloRemoveEvent, GrainDirectoryHandoffManager.cs:141-168): an absent grain is added as is; for a grain
// present on both sides GrainInfo.Merge (:158-183) keeps, of the single-activation grain's activations, the one
// with the smallest ActivationId (UniqueKey.CompareTo: TypeCodeData, N0, N1 unsigned) and the other is dropped
// (reported for Catalog.DeleteActivations).  A copy is a dictionary: a key appearing twice in one batch gets
// ORL_MERGE_DUPLICATE (only the first is applied).  probe (find or claim; FULL entries claimed too, so the first
// batch entry of a key owns it) → resolve (compare ActivationIds) → commit.
__device__ __forceinline__ bool act_key_less(const orl_grain_key& a, const orl_grain_key& b) {
    return a.type_code_data != b.type_code_data ? a.type_code_data < b.type_code_data
         : a.n0 != b.n0 ? a.n0 < b.n0 : a.n1 < b.n1;
}
__device__ __forceinline__ bool act_key_eq(const orl_grain_key& a, const orl_grain_key& b) {
    return a.type_code_data == b.type_code_data && a.n0 == b.n0 && a.n1 == b.n1;
}

__global__ __launch_bounds__(256) void k_dir_merge_probe(DirSlot* __restrict__ dir, uint64_t mask, uint32_t* __restrict__ claim,
                                                         const orl_grain_key* __restrict__ keys, const uint32_t* __restrict__ acts,
                                                         const uint8_t* __restrict__ silos, uint32_t n, uint32_t n_act,
                                                         uint32_t n_silos, uint32_t n_act_keys, uint32_t* __restrict__ slot_out,
                                                         uint8_t* __restrict__ status, uint32_t* __restrict__ err, DirTags vt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const orl_grain_key k = keys[i];
    const uint32_t cat = (uint32_t)(k.type_code_data >> 56);
    uint32_t out = kSlotNone;
    uint8_t st = kInsCandidate;
    if (acts[i] >= n_act || acts[i] >= n_act_keys || silos[i] >= n_silos || cat == ORL_CAT_KEYEXT_GRAIN ||
        (vt.in && vt.in[i] < 0) || (vt.draws && vt.draws[i] < 0)) {
        st = ORL_MERGE_UNSUPPORTED;
    } else {
        uint64_t slot = 0;
        bool was_tomb = false;
        const int outcome = find_or_claim<true>(DirClaim{dir, k}, key_start(k, mask), mask, claim, i, slot, was_tomb);
        if (outcome < 0) {
            atomicOr(err, 1u);
            st = ORL_MERGE_UNSUPPORTED;
        } else {
            out = (uint32_t)slot | (was_tomb ? kSlotWasTomb : 0u);
            st = outcome == 0 ? (uint8_t)ORL_MERGE_KEPT : kInsCandidate;  // resolved below
        }
    }
    slot_out[i] = out;
    status[i] = st;
}

__global__ __launch_bounds__(256) void k_dir_merge_resolve(const DirSlot* __restrict__ dir, const uint32_t* __restrict__ claim,
                                                           const uint32_t* __restrict__ acts, const uint8_t* __restrict__ silos,
                                                           const orl_grain_key* __restrict__ act_keys, uint32_t n,
                                                           const uint32_t* __restrict__ slot_in, uint8_t* __restrict__ status,
                                                           uint32_t* __restrict__ dropped_act, uint8_t* __restrict__ dropped_silo) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint8_t st = status[i];
    uint32_t da = ORL_NO_ACT;
    uint8_t ds = (uint8_t)ORL_NULL_SILO;
    if (st != ORL_MERGE_UNSUPPORTED) {
        const uint32_t slot = slot_in[i] & kSlotMask;
        if (claim[slot] != i) {
            st = ORL_MERGE_DUPLICATE;
        } else if (st == kInsCandidate) {
            st = ORL_MERGE_INSERTED;
        } else {  // present on both sides: keep the smaller ActivationId
            const uint32_t a_old = dir[slot].act;
            const orl_grain_key ko = act_keys[a_old], kn = act_keys[acts[i]];
            if (act_key_eq(ko, kn)) {
                st = ORL_MERGE_SAME;
            } else if (act_key_less(kn, ko)) {
                st = ORL_MERGE_REPLACED;
                da = a_old;
                ds = dir[slot].silo;
            } else {
                st = ORL_MERGE_KEPT;
                da = acts[i];
                ds = silos[i];
            }
        }
    }
    status[i] = st;
    if (dropped_act) dropped_act[i] = da;
    if (dropped_silo) dropped_silo[i] = ds;
}

__global__ __launch_bounds__(256) void k_dir_merge_commit(DirSlot* __restrict__ dir, uint32_t* __restrict__ claim,
                                                          const uint32_t* __restrict__ acts, const uint8_t* __restrict__ silos,
                                                          uint32_t n, const uint32_t* __restrict__ slot_in,
                                                          const uint8_t* __restrict__ status, uint64_t* __restrict__ cnt,
                                                          DirTags vt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint8_t st = status[i];
    if (st == ORL_MERGE_UNSUPPORTED || st == ORL_MERGE_DUPLICATE) return;
    const uint32_t slot = slot_in[i] & kSlotMask;
    if (vt.slot) {
        // an absent grain's GrainInfo is added as is, tag included (GrainDirectoryPartition.Merge :366-383); GrainInfo.Merge
        // added an instance to a present one, so it drew a new tag whichever activation survives (:146-160)
        if (st == ORL_MERGE_INSERTED) vt.slot[slot] = vt.in ? vt.in[i] : 0;
        else if (st == ORL_MERGE_KEPT || st == ORL_MERGE_REPLACED) vt.slot[slot] = vt.draws ? vt.draws[i] : 0;
    }
    if (st == ORL_MERGE_INSERTED || st == ORL_MERGE_REPLACED) {
        uint64_t* w24 = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(dir + slot) + 24);
        *w24 = (uint64_t)acts[i] | ((uint64_t)silos[i] << 32) | ((uint64_t)SLOT_FULL << 40);
    }
    if (st == ORL_MERGE_INSERTED) {
        add64(cnt, 1);
        if (slot_in[i] & kSlotWasTomb) add64(cnt + 1, ~0ull);
    }
    claim[slot] = kSlotNone;  // this entry owned the slot's claim (duplicates returned above)
}

// ---------------------------------------------------------------------------------------------------
// Unregister: the first removal of a key in batch order removes it (RemoveActivation on the entry; later ones
// find nothing).  probe → atomicMin on the entry's claim word; resolve; commit (FULL → TOMB).
__global__ __launch_bounds__(256) void k_dir_rm_probe(const DirSlot* __restrict__ dir, uint64_t mask, uint32_t* __restrict__ claim,
                                                      const orl_grain_key* __restrict__ keys, uint32_t n,
                                                      uint32_t* __restrict__ slot_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t slot = find_full<false>(dir, mask, keys[i]);
    if (slot != ~0ull) atomicMin(&claim[slot], i);
    slot_out[i] = slot != ~0ull ? (uint32_t)slot : kSlotNone;
}

__global__ __launch_bounds__(256) void k_dir_rm_resolve(const uint32_t* __restrict__ claim, uint32_t n,
                                                        const uint32_t* __restrict__ slot_in, uint8_t* __restrict__ removed) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = slot_in[i];
    removed[i] = (slot != kSlotNone && claim[slot] == i) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_dir_rm_commit(DirSlot* __restrict__ dir, uint32_t* __restrict__ claim, uint32_t n,
                                                       const uint32_t* __restrict__ slot_in, const uint8_t* __restrict__ removed,
                                                       uint64_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || !removed[i]) return;
    const uint32_t slot = slot_in[i];
    dir[slot].state = SLOT_TOMB;
    claim[slot] = kSlotNone;
    add64(cnt, ~0ull);    // entries - 1
    add64(cnt + 1, 1);    // tombstones + 1
}

}  // namespace

int launch_dir_insert(const RouteParams* d_params, DirSlot* d_dir, uint64_t dir_mask, uint32_t* d_claim, uint64_t* d_cnt,
                      const orl_grain_key* d_keys, const uint32_t* d_acts, const uint8_t* d_silos, size_t n, uint32_t n_act,
                      uint32_t n_silos, uint32_t* d_slot, uint32_t* d_wact, uint8_t* d_wsilo, uint8_t* d_status, uint32_t* d_err,
                      void* stream, const DirTags& vt) {
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return 0;
    const dim3 g(blocks(n)), b(256);
    hipLaunchKernelGGL(k_dir_ins_probe, g, b, 0, st, d_params, d_dir, dir_mask, d_claim, d_keys, d_acts, d_silos, (uint32_t)n,
                       n_act, n_silos, d_slot, d_status, d_err, vt.slot ? vt.in : nullptr);
    hipLaunchKernelGGL(k_dir_ins_resolve, g, b, 0, st, d_dir, d_claim, d_acts, d_silos, (uint32_t)n, d_slot, d_status, d_wact,
                       d_wsilo, vt);
    hipLaunchKernelGGL(k_dir_ins_commit, g, b, 0, st, d_dir, d_claim, d_acts, d_silos, (uint32_t)n, d_slot, d_status, d_cnt, vt);
    return (int)hipGetLastError();
}

int launch_dir_merge(DirSlot* d_dir, uint64_t dir_mask, uint32_t* d_claim, uint64_t* d_cnt, const orl_grain_key* d_keys,
                     const uint32_t* d_acts, const uint8_t* d_silos, size_t n, uint32_t n_act, uint32_t n_silos,
                     const orl_grain_key* d_act_keys, uint32_t n_act_keys, uint32_t* d_slot, uint8_t* d_status,
                     uint32_t* d_dropped_act, uint8_t* d_dropped_silo, uint32_t* d_err, void* stream, const DirTags& vt) {
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return 0;
    const dim3 g(blocks(n)), b(256);
    hipLaunchKernelGGL(k_dir_merge_probe, g, b, 0, st, d_dir, dir_mask, d_claim, d_keys, d_acts, d_silos, (uint32_t)n, n_act,
                       n_silos, n_act_keys, d_slot, d_status, d_err, vt);
    hipLaunchKernelGGL(k_dir_merge_resolve, g, b, 0, st, d_dir, d_claim, d_acts, d_silos, d_act_keys, (uint32_t)n, d_slot,
                       d_status, d_dropped_act, d_dropped_silo);
    hipLaunchKernelGGL(k_dir_merge_commit, g, b, 0, st, d_dir, d_claim, d_acts, d_silos, (uint32_t)n, d_slot, d_status, d_cnt, vt);
    return (int)hipGetLastError();
}

int launch_cache_update(DirSlot* d_cache, uint64_t mask, uint32_t* d_claim, uint64_t* d_cnt, const orl_grain_key* d_keys,
                        const uint32_t* d_acts, const uint8_t* d_silos, size_t n, uint32_t n_act, uint32_t n_silos, uint32_t* d_slot,
                        uint8_t* d_flag, uint32_t* d_err, void* stream, const RouteParams* d_params, const CacheFresh& fresh) {
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return 0;
    const dim3 g(blocks(n)), b(256);
    hipLaunchKernelGGL(k_cache_probe, g, b, 0, st, d_cache, mask, d_claim, d_keys, d_acts, d_silos, (uint32_t)n, n_act, n_silos,
                       d_params->local, d_slot, d_err);
    hipLaunchKernelGGL(k_cache_resolve, g, b, 0, st, d_claim, (uint32_t)n, d_slot, d_flag);
    hipLaunchKernelGGL(k_cache_commit, g, b, 0, st, d_cache, d_claim, d_acts, d_silos, (uint32_t)n, d_slot, d_flag, d_cnt, mask,
                       fresh);
    return launch_cache_gen_advance(d_cache, mask, n, stream);
}

int launch_cache_gen_advance(const DirSlot* d_cache, uint64_t mask, uint64_t n, void* stream) {
    if (!d_cache || n == 0) return 0;
    hipLaunchKernelGGL(k_gen_advance, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<unsigned long long*>(const_cast<DirSlot*>(d_cache + mask + 1)) + mask + 1, n);
    return (int)hipGetLastError();
}

int launch_dir_remove(DirSlot* d_dir, uint64_t dir_mask, uint32_t* d_claim, uint64_t* d_cnt, const orl_grain_key* d_keys,
                      size_t n, uint32_t* d_slot, uint8_t* d_removed, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return 0;
    const dim3 g(blocks(n)), b(256);
    hipLaunchKernelGGL(k_dir_rm_probe, g, b, 0, st, d_dir, dir_mask, d_claim, d_keys, (uint32_t)n, d_slot);
    hipLaunchKernelGGL(k_dir_rm_resolve, g, b, 0, st, d_claim, (uint32_t)n, d_slot, d_removed);
    hipLaunchKernelGGL(k_dir_rm_commit, g, b, 0, st, d_dir, d_claim, (uint32_t)n, d_slot, d_removed, d_cnt);
    return (int)hipGetLastError();
}

int launch_keyext_insert(const RouteParams* d_params, ExtSlot* d_table, uint64_t mask, uint32_t* d_claim, uint8_t* d_tblob,
                         uint64_t tblob_cap, const orl_grain_key* d_keys, const orl_ext_ref* d_ext, const uint8_t* d_blob,
                         uint64_t blob_bytes, const uint32_t* d_acts, const uint8_t* d_silos, size_t n, uint32_t n_act,
                         uint32_t n_silos, uint32_t* d_slot, uint32_t* d_wact, uint8_t* d_wsilo, uint8_t* d_status,
                         uint64_t* d_state, void* stream) {
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(blocks(n)), b(256);
    unsigned long long* state = reinterpret_cast<unsigned long long*>(d_state);
    hipLaunchKernelGGL(k_kx_ins_probe, g, b, 0, st, d_params, d_table, mask, d_claim, d_tblob, tblob_cap, d_keys, d_ext, d_blob,
                       blob_bytes, d_acts, d_silos, (uint32_t)n, n_act, n_silos, d_slot, d_status, state);
    hipLaunchKernelGGL(k_kx_ins_resolve, g, b, 0, st, d_table, d_claim, d_acts, d_silos, (uint32_t)n, d_slot, d_status, d_wact,
                       d_wsilo);
    hipLaunchKernelGGL(k_kx_ins_commit, g, b, 0, st, d_table, d_claim, d_acts, d_silos, (uint32_t)n, d_slot, d_status, state);
    return (int)hipGetLastError();
}

}  // namespace orl
