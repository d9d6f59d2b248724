// tile_scan_dev.h — device-side helpers of the scan-shaped files (admit.hip, waitq.hip, collect.hip, and the block scan
// of cache_evict.hip / cache_adaptive.hip): the tile constants, the scan value and its stored per-tile aggregate, the
// block scan, the one-workgroup tile scan, the 8-item loads and stores, the bucket search of a bucketed batch and the
// d_counts sums of a workgroup, each written once.  What a scan means (the ops and the seg_* functions)
// stays in the file that uses it.  Device code only: the host side (orl_api.cpp, orl_node.cpp) does not include it.
#pragma once

#include <hip/hip_runtime.h>

#include "orl_internal.h"

namespace orl {

// A segment-scan value (the including file's ops give a, b, f their meaning) ...
struct Seg {
    uint32_t a, b, f;
};

// ... and its 16-byte stored form: one per tile, the tile's aggregate and then the carry into it.
struct SegAgg {
    uint32_t a, b, f, pad;
    SegAgg() = default;
    __device__ __forceinline__ explicit SegAgg(Seg s) : a(s.a), b(s.b), f(s.f), pad(0) {}
    __device__ __forceinline__ explicit operator Seg() const { return Seg{a, b, f}; }
};

namespace {

// A tile: 256 threads x 8 consecutive items.  (orl_internal.h's kTile is the route tile, 4096.)
constexpr uint32_t kTileThreads = 256;
constexpr uint32_t kTileItems = 8;
constexpr uint32_t kScanTile = kTileThreads * kTileItems;  // 2048 positions / records / activations per workgroup
constexpr uint32_t kScanThreads = 1024;                    // the one workgroup that scans the tile aggregates

struct OpAdd {
    static __device__ __forceinline__ uint32_t op(uint32_t x, uint32_t y) { return x + y; }
};

// Inclusive Hillis-Steele scan of one value per thread through LDS (2 * N values); returns the exclusive prefix of
// thread t and the workgroup's total.  Ends on a barrier: `lds` may be reused at once.  T{} is Op's identity.
template <class T, class Op, uint32_t N>
__device__ __forceinline__ T block_exclusive(T mine, T* lds, T* total) {
    const uint32_t t = threadIdx.x;
    T* src = lds;
    T* dst = lds + N;
    src[t] = mine;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < N; d <<= 1) {
        T v = src[t];
        if (t >= d) v = Op::op(src[t - d], v);
        dst[t] = v;
        __syncthreads();
        T* sw = src;
        src = dst;
        dst = sw;
    }
    const T ex = t ? src[t - 1] : T{};
    *total = src[N - 1];
    __syncthreads();
    return ex;
}

// In place: agg[i] = the fold of agg[0 .. i), *total (when given) = the fold of all.  One workgroup of kScanThreads;
// thread t owns the chunk [t * chunk, (t + 1) * chunk), clamped to ntiles.  `lds` holds 2 * kScanThreads values.
template <class T, class Stored, class Op>
__device__ __forceinline__ void tile_scan_body(Stored* agg, uint32_t ntiles, T* lds, T* total = nullptr) {
    const uint32_t chunk = (ntiles + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = threadIdx.x * chunk < ntiles ? threadIdx.x * chunk : ntiles;
    const uint32_t hi = ntiles - lo < chunk ? ntiles : lo + chunk;
    T sum{};
    for (uint32_t i = lo; i < hi; ++i) sum = Op::op(sum, T(agg[i]));
    T all;
    T run = block_exclusive<T, Op, kScanThreads>(sum, lds, &all);
    for (uint32_t i = lo; i < hi; ++i) {
        const T v = T(agg[i]);
        agg[i] = Stored(run);
        run = Op::op(run, v);
    }
    if (total) *total = all;
}

// The 8 bytes / 8 words of thread t's items in a tile-padded scratch array.
__device__ __forceinline__ void load_bytes(const uint8_t* p, uint32_t (&v)[kTileItems]) {
    const uint2 w = *reinterpret_cast<const uint2*>(p);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        v[k] = (w.x >> (8 * k)) & 0xFFu;
        v[k + 4] = (w.y >> (8 * k)) & 0xFFu;
    }
}

__device__ __forceinline__ void store_bytes(uint8_t* p, const uint32_t (&v)[kTileItems]) {
    uint2 w;
    w.x = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
    w.y = v[4] | v[5] << 8 | v[6] << 16 | v[7] << 24;
    *reinterpret_cast<uint2*>(p) = w;
}

__device__ __forceinline__ void load_words(const uint32_t* p, uint32_t (&v)[kTileItems]) {
    const uint4 lo = *reinterpret_cast<const uint4*>(p), hi = *reinterpret_cast<const uint4*>(p + 4);
    v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
    v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}

// The same of a store array (tile-padded, 16-byte aligned), read once: non-temporal.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void stream_words(const uint32_t* p, uint32_t (&v)[kTileItems]) {
    const u32x4 lo = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    const u32x4 hi = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + 4));
    v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
    v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}

__device__ __forceinline__ void stream_bytes(const uint8_t* p, uint32_t (&v)[kTileItems]) {
    const u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        v[k] = (w.x >> (8 * k)) & 0xFFu;
        v[k + 4] = (w.y >> (8 * k)) & 0xFFu;
    }
}

// Eight 64-bit values of a tile-padded array, read once: non-temporal.
__device__ __forceinline__ void stream_i64(const int64_t* p, int64_t (&v)[kTileItems]) {
    const u32x4* q = reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (uint32_t k = 0; k < kTileItems / 2; ++k) {
        const u32x4 w = __builtin_nontemporal_load(q + k);
        v[2 * k] = (int64_t)((uint64_t)w.x | (uint64_t)w.y << 32);
        v[2 * k + 1] = (int64_t)((uint64_t)w.z | (uint64_t)w.w << 32);
    }
}

// order[p0 .. p0 + 8) of the caller's array, streamed (non-temporal); 0 past n.
__device__ __forceinline__ void load_order(const uint32_t* __restrict__ order, size_t p0, size_t n, bool vec,
                                           uint32_t (&v)[kTileItems]) {
    if (vec && p0 + kTileItems <= n) {
        stream_words(order + p0, v);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < kTileItems; ++k) v[k] = p0 + k < n ? __builtin_nontemporal_load(order + p0 + k) : 0u;
    }
}

// The bucket of position p: the smallest b in [lo, n_act] with off[b + 1] > p (off[n_act + 1] = n > p).  At most 32 steps.
__device__ __forceinline__ uint32_t bucket_of(const uint32_t* __restrict__ off, uint32_t lo, uint32_t n_act, size_t p) {
    uint32_t hi = n_act;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((size_t)off[mid + 1] > p) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// key[k] = the bucket of position p0 + k (n_act past n); bit k is ORed into *head_bits when the position is its bucket's
// first (the caller clears it).
// The key of a position comes from the offsets, not from act[order[p]]: a search per thread and one more per bucket
// boundary inside its 8 positions (the next bucket first), against a random 4-byte gather per position.
__device__ __forceinline__ void bucket_keys(const uint32_t* off, uint32_t n_act, size_t p0, size_t n,
                                            uint32_t (&key)[kTileItems], uint32_t* head_bits) {
    uint32_t b = n_act;
    size_t begin = 0, end = 0;  // bucket b = [begin, end)
    if (p0 < n) {
        b = bucket_of(off, 0, n_act, p0);
        begin = off[b];
        end = off[b + 1];
    }
#pragma unroll
    for (uint32_t k = 0; k < kTileItems; ++k) {
        const size_t p = p0 + k;
        if (p < n && p >= end && b < n_act) {  // the last bucket ends at n: b < n_act holds for stage 4's offsets
            const size_t next_end = off[b + 2];
            if (p < next_end) {
                b += 1;
                begin = end;
                end = next_end;
            } else {
                b = bucket_of(off, b + 2 < n_act ? b + 2 : n_act, n_act, p);
                begin = off[b];
                end = off[b + 1];
            }
        }
        key[k] = p < n ? b : n_act;
        *head_bits |= (p < n && p == begin ? 1u : 0u) << k;
    }
}

// The last step of a workgroup's d_counts sums: kSlots lanes add the non-zero LDS sums to base[0 .. kSlots).  After a
// barrier that orders the LDS sums before it.
template <uint32_t kSlots>
__device__ __forceinline__ void flush_counts(const uint32_t* lds, uint64_t* base) {
    if (threadIdx.x < kSlots && lds[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(base + threadIdx.x), (unsigned long long)lds[threadIdx.x]);
}

// The sums of "what[k] == q", q < kSlots, over a workgroup's items: a ballot per wave, the wave's first lane adds to LDS
// (zeroed by the caller, before a barrier), then the flush.  Every lane of every wave reaches the ballots.
template <uint32_t kSlots>
__device__ __forceinline__ void ballot_counts(const uint32_t (&what)[kTileItems], uint32_t* lds, uint64_t* base) {
    uint32_t wc[kSlots];
#pragma unroll
    for (uint32_t q = 0; q < kSlots; ++q) wc[q] = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTileItems; ++k) {
#pragma unroll
        for (uint32_t q = 0; q < kSlots; ++q) wc[q] += (uint32_t)__popcll(__ballot(what[k] == q));
    }
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (uint32_t q = 0; q < kSlots; ++q)
            if (wc[q]) atomicAdd(&lds[q], wc[q]);
    }
    __syncthreads();
    flush_counts<kSlots>(lds, base);
}

// d_counts sums of one workgroup where few lanes count: lanes add to LDS, then the flush.
struct BlockCounts {
    uint32_t* lds;
    __device__ __forceinline__ void init(uint32_t* p) {
        lds = p;
        if (threadIdx.x < 8) lds[threadIdx.x] = 0;
        __syncthreads();
    }
    __device__ __forceinline__ void add(uint32_t q, uint32_t v = 1) { atomicAdd(&lds[q], v); }
    __device__ __forceinline__ void flush(uint64_t* counts) {  // every thread of the workgroup calls it
        __syncthreads();
        if (counts) flush_counts<8>(lds, counts);
    }
};

}  // namespace

}  // namespace orl
