// dir_versions.hip — the owner's side of the directory cache's refresh on the device (gfx950).
//
// AdaptiveDirectoryCacheMaintainer sends each directory owner one LookUpMany request: the (grain, etag) pairs of the
// requester's expired, accessed cache entries.  RemoteGrainDirectory.LookUpMany (RemoteGrainDirectory.cs:349-380) answers
// per pair from GrainDirectoryPartition.GetGrainETag and LookUpGrain (GrainDirectoryPartition.cs:326-359): the same etag
// back with no activation list when the entry's VersionTag still equals the requester's, else the current list and tag,
// and (null, -1) for a grain the partition no longer holds.  The partition lives on the device and is mutated there, so
// the answer is computed here, on the caller's stream, from the 32-B table and the per-slot tag array beside it (DESIGN
// §13).  The call only reads: a key may repeat, nothing is claimed, and no kernel waits for another workgroup; the chain
// walk is bounded by the slot count.

#include <hip/hip_runtime.h>

#include "dir_table_dev.h"
#include "dir_versions.h"

namespace orl {

namespace {

constexpr uint32_t kLumKinds = 5;           // ORL_LUM_UNCHANGED .. ORL_LUM_UNSUPPORTED
constexpr uint32_t kLumNone = 0xFFu;        // a lane past the batch's end: no kind
constexpr size_t kLumChunk = (size_t)1 << 30;  // requests per launch (2^22 blocks of 256)

// One lane per request.  The walk reads a slot's last 8 bytes first (act | silo << 32 | state << 40: the state decides
// whether the 24-B key is compared at all, and a match needs nothing more from the slot), then the key of FULL slots.
// A matching request reads its slot's tag: a second dependent random line (measured in DESIGN §13).
__global__ __launch_bounds__(256) void k_lookup_many(const RouteParams* __restrict__ gp, const DirSlot* __restrict__ dir,
                                                     uint64_t mask, const int32_t* __restrict__ tags,
                                                     const orl_grain_key* __restrict__ keys, const int32_t* __restrict__ etags,
                                                     size_t n, uint8_t* __restrict__ kind_out, int32_t* __restrict__ etag_out,
                                                     uint32_t* __restrict__ act_out, uint8_t* __restrict__ silo_out,
                                                     uint64_t* __restrict__ counts) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t kind = kLumNone;
    if (i < n) {
        const orl_grain_key k = keys[i];
        const uint32_t cat = (uint32_t)(k.type_code_data >> 56);
        int32_t cur = ORL_DIR_NO_ETAG;
        uint32_t a = ORL_NO_ACT;
        uint8_t s = (uint8_t)ORL_NULL_SILO;
        if (cat == ORL_CAT_KEYEXT_GRAIN || cat == ORL_CAT_SYSTEM_TARGET) {
            kind = ORL_LUM_UNSUPPORTED;  // not held in this table
        } else {
            kind = ORL_LUM_ABSENT;
            uint64_t slot = dir_slot(jenkins3(k.type_code_data, k.n0, k.n1), mask);
            for (uint64_t step = 0; step <= mask; ++step) {
                const uint64_t* w = reinterpret_cast<const uint64_t*>(dir + slot);
                const uint64_t w24 = w[3];
                const uint32_t state = (uint32_t)(w24 >> 40) & 0xFFu;
                if (state == SLOT_EMPTY) break;
                if (state == SLOT_FULL && w[0] == k.type_code_data && w[1] == k.n0 && w[2] == k.n1) {
                    cur = tags[slot];  // GetGrainETag
                    const uint32_t silo = (uint32_t)(w24 >> 32) & 0xFFu;
                    if (cur == etags[i]) {
                        kind = ORL_LUM_UNCHANGED;  // "the directory entry has not changed": (null, curGen)
                    } else if (mask_bit(gp->functional, silo)) {
                        kind = ORL_LUM_UPDATED;
                        a = (uint32_t)w24;
                        s = (uint8_t)silo;
                    } else {
                        kind = ORL_LUM_UPDATED_EMPTY;  // LookUpGrain filtered the only activation: an empty list with the tag
                    }
                    break;
                }
                slot = (slot + 1) & mask;
            }
        }
        kind_out[i] = (uint8_t)kind;
        etag_out[i] = cur;
        act_out[i] = a;
        silo_out[i] = s;
    }
    if (counts) {  // wave-uniform; every lane of the wave reaches the ballots
        const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
        for (uint32_t q = 0; q < kLumKinds; ++q) {
            const unsigned long long b = __ballot(kind == q);
            if (lane == 0 && b) atomicAdd(reinterpret_cast<unsigned long long*>(counts + q), (unsigned long long)__popcll(b));
        }
    }
}

__global__ __launch_bounds__(256) void k_tag_patch(const uint32_t* __restrict__ idx, const int32_t* __restrict__ nw, uint32_t n,
                                                   int32_t* __restrict__ tags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) tags[idx[i]] = nw[i];
}

}  // namespace

int launch_lookup_many(const RouteParams* d_params, const DirSlot* d_dir, uint64_t mask, const int32_t* d_tags,
                       const orl_grain_key* d_keys, const int32_t* d_etags, size_t n, uint8_t* d_kind, int32_t* d_etag_out,
                       uint32_t* d_act, uint8_t* d_silo, uint64_t* d_counts, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (d_counts) {
        hipError_t e = hipMemsetAsync(d_counts, 0, kLumKinds * sizeof(uint64_t), st);
        if (e != hipSuccess) return (int)e;
    }
    for (size_t at = 0; at < n; at += kLumChunk) {
        const size_t m = n - at < kLumChunk ? n - at : kLumChunk;
        hipLaunchKernelGGL(k_lookup_many, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, d_params, d_dir, mask, d_tags,
                           d_keys + at, d_etags + at, m, d_kind + at, d_etag_out + at, d_act + at, d_silo + at, d_counts);
    }
    return (int)hipGetLastError();
}

int launch_tag_patch(const uint32_t* d_idx, const int32_t* d_new, uint32_t n, int32_t* d_tags, void* stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_tag_patch, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_idx, d_new, n, d_tags);
    return (int)hipGetLastError();
}

}  // namespace orl
