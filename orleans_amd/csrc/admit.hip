// admit.hip — admission of a bucketed batch on the device (gfx950): run, enqueue or reject each message.
//
// After stage 4 grouped a batch by activation, the reference decides per message, under the activation's lock, what the
// activation does with it (IncomingMessageAgent.ReceiveMessage, IncomingMessageAgent.cs:144-181; Dispatcher.ReceiveMessage
// -> ReceiveRequest -> ActivationMayAcceptRequest / EnqueueRequest, Dispatcher.cs:78-204, 265-338, 375-427); the rules are
// listed at orl_admit_device in include/orleans_route.h.  Each decision depends on the state the earlier messages of the
// same activation left, but only through counts.  Inside one bucket with start state c0 = in_flight +
// waiting, limit L and T = L - c0, for the message at position p:
//   q_p     = the bucket's earlier non-expired Request / OneWay messages ("requests");
//   Running = the start state's if set, else the bucket's first request, which is then accepted whatever it is; so is the
//             first request of an activation with num_running == 0.  After it a request is accepted ("alpha") iff the
//             activation is reentrant, or the message is always-interleave, or Running and the message are both read-only:
//             a function of the message and the bucket alone;
//   VALID, L > 0, T < 0:   rule 1 rejects every message and nothing changes;
//   VALID otherwise:       c grows by one per request up to L; there an alpha still runs (c = L + 1, "saturation") and a
//                          non-alpha is rejected by rule 7; after saturation rule 1 rejects every message.  So before
//                          saturation an alpha runs and a non-alpha is enqueued iff q_p < T, and the saturating message is
//                          the first alpha with q_p >= T;
//   CREATE / ACTIVATING / DEACTIVATING: a request is enqueued iff L <= 0 || c0 + q_p <= L.
// That is two segmented scans over the positions of `order` (segments = buckets): the first carries the request count
// and the first request's read-only bit, the second "saturated yet", and, for the state update, the runs and enqueues
// up to saturation.  Both are reduce-then-scan: a pass that leaves one aggregate per tile, one workgroup that scans the
// aggregates, a pass that redoes the tile with its carry-in.  No workgroup waits for another, no lane walks a bucket,
// every loop is bounded by a count.
//
//   k_adm_classify   gathers mflags[order[p]], finds the bucket and its head in the offsets; writes key[p], cls[p],
//                    aggregate 1
//   k_adm_tilescan   exclusive scan of the tile aggregates (one workgroup)
//   k_adm_decide     scan 1 inside the tile, reads the activation's state, writes the provisional disposition over
//                    cls[p], aggregate 2
//   k_adm_tilescan
//   k_adm_resolve    scan 2 inside the tile, writes d_disp[order[p]], counts; the lane at a bucket's last position adds
//                    the bucket's runs and enqueues to its orl_act_state
// The state table is read by k_adm_decide only and written by k_adm_resolve only (one lane per entry).

#include <hip/hip_runtime.h>

#include "admit.h"

namespace orl {

namespace {

constexpr uint32_t kT = kAdmitThreads, kI = kAdmitItems;
constexpr uint32_t kScanThreads = 1024;  // k_adm_tilescan's one workgroup

// cls[p] as k_adm_classify writes it
constexpr uint32_t kClsReq = 0x01, kClsRo = 0x02, kClsAi = 0x04, kClsExp = 0x08, kClsResp = 0x10, kClsHead = 0x20;
// cls[p] as k_adm_decide rewrites it: code | kDecSat (this message saturates its bucket) | kDecHead | kDecRo, kDecKnown
// (the bucket's first request is known at p, and read-only)
constexpr uint32_t kDecCode = 0x07, kDecSat = 0x08, kDecHead = 0x10, kDecRo = 0x20, kDecKnown = 0x40;
constexpr uint32_t kNoCode = 0xFF;

struct Seg {
    uint32_t a, b, f;
};

// Scan 1.  a = requests since the span's last bucket head, b = the first of them (0 none, 1 read-write, 2 read-only),
// f = 1: the span holds a bucket head.
struct OpReq {
    static __device__ __forceinline__ Seg op(Seg x, Seg y) {
        if (y.f & 1u) return y;
        return Seg{x.a + y.a, x.b ? x.b : y.b, x.f};
    }
};

// Scan 2.  a = runs, b = enqueues since the span's last bucket head and up to its saturation; f = 1: holds a head, 2:
// saturated.
struct OpAdm {
    static __device__ __forceinline__ Seg op(Seg x, Seg y) {
        if (y.f & 1u) return y;
        if (x.f & 2u) return x;
        return Seg{x.a + y.a, x.b + y.b, x.f | (y.f & 2u)};
    }
};

__device__ __forceinline__ Seg seg_req(uint32_t cls) {
    const uint32_t r = cls & kClsReq;
    return Seg{r, r ? ((cls & kClsRo) ? 2u : 1u) : 0u, (cls & kClsHead) ? 1u : 0u};
}

__device__ __forceinline__ Seg seg_adm(uint32_t dec) {
    const uint32_t code = dec & kDecCode;
    return Seg{code == ORL_ADM_RUN ? 1u : 0u, code == ORL_ADM_ENQUEUE ? 1u : 0u,
               ((dec & kDecHead) ? 1u : 0u) | ((dec & kDecSat) ? 2u : 0u)};
}

// Inclusive Hillis-Steele scan of one value per thread through LDS (2 * N values); returns the exclusive prefix of
// thread t and the workgroup's total.  Ends on a barrier: `lds` may be reused at once.
template <class Op, uint32_t N>
__device__ __forceinline__ Seg block_exclusive(Seg mine, Seg* lds, Seg* total) {
    const uint32_t t = threadIdx.x;
    Seg* src = lds;
    Seg* dst = lds + N;
    src[t] = mine;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < N; d <<= 1) {
        Seg v = src[t];
        if (t >= d) v = Op::op(src[t - d], v);
        dst[t] = v;
        __syncthreads();
        Seg* sw = src;
        src = dst;
        dst = sw;
    }
    const Seg ex = t ? src[t - 1] : Seg{0, 0, 0};
    *total = src[N - 1];
    __syncthreads();
    return ex;
}

// The 8 bytes / 8 words of thread t's positions in a tile-padded scratch array.
__device__ __forceinline__ void load_bytes(const uint8_t* p, uint32_t (&v)[kI]) {
    const uint2 w = *reinterpret_cast<const uint2*>(p);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        v[k] = (w.x >> (8 * k)) & 0xFFu;
        v[k + 4] = (w.y >> (8 * k)) & 0xFFu;
    }
}

__device__ __forceinline__ void store_bytes(uint8_t* p, const uint32_t (&v)[kI]) {
    uint2 w;
    w.x = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
    w.y = v[4] | v[5] << 8 | v[6] << 16 | v[7] << 24;
    *reinterpret_cast<uint2*>(p) = w;
}

__device__ __forceinline__ void load_words(const uint32_t* p, uint32_t (&v)[kI]) {
    const uint4 lo = *reinterpret_cast<const uint4*>(p), hi = *reinterpret_cast<const uint4*>(p + 4);
    v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
    v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}

// order[p0 .. p0 + 8) of the caller's array, streamed (non-temporal); 0 past n.
__device__ __forceinline__ void load_order(const uint32_t* __restrict__ order, size_t p0, size_t n, bool vec,
                                           uint32_t (&v)[kI]) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    if (vec && p0 + kI <= n) {
        const u32x4 lo = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(order + p0));
        const u32x4 hi = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(order + p0 + 4));
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
        v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < kI; ++k) v[k] = p0 + k < n ? __builtin_nontemporal_load(order + p0 + k) : 0u;
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

// The key of a position comes from the offsets, not from act[order[p]]: a search per thread and one more per bucket
// boundary inside its 8 positions (the next bucket first), against a random 4-byte gather per position.
__global__ __launch_bounds__(kT) void k_adm_classify(const uint8_t* __restrict__ mflags, size_t n, uint32_t n_act,
                                                     const uint32_t* __restrict__ order, bool order_vec,
                                                     const uint32_t* __restrict__ off, uint32_t* __restrict__ key_out,
                                                     uint8_t* __restrict__ cls_out, AdmitSeg* __restrict__ agg) {
    __shared__ Seg lds[2 * kT];
    const size_t p0 = (size_t)blockIdx.x * kAdmitTile + (size_t)threadIdx.x * kI;
    uint32_t idx[kI], key[kI], cls[kI], head = 0;
    load_order(order, p0, n, order_vec, idx);
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) cls[k] = p0 + k < n ? mflags[idx[k]] : 0u;  // 8 gathers in flight together
    uint32_t b = n_act;
    size_t begin = 0, end = 0;  // bucket b = [begin, end)
    if (p0 < n) {
        b = bucket_of(off, 0, n_act, p0);
        begin = off[b];
        end = off[b + 1];
    }
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
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
        head |= (p < n && p == begin ? 1u : 0u) << k;
    }
    Seg sum{0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        if (p0 + k < n) {
            const uint32_t f = cls[k];
            const bool exp = (f & ORL_MF_EXPIRED) != 0, resp = (f & ORL_MF_DIR_MASK) == ORL_MF_RESPONSE;
            cls[k] = (!exp && !resp ? kClsReq : 0u) | ((f & ORL_MF_READ_ONLY) ? kClsRo : 0u) |
                     ((f & ORL_MF_ALWAYS_INTERLEAVE) ? kClsAi : 0u) | (exp ? kClsExp : 0u) | (resp ? kClsResp : 0u) |
                     ((head >> k & 1u) ? kClsHead : 0u);
        }
        sum = OpReq::op(sum, seg_req(cls[k]));
    }
    uint4* ko = reinterpret_cast<uint4*>(key_out + p0);
    ko[0] = make_uint4(key[0], key[1], key[2], key[3]);
    ko[1] = make_uint4(key[4], key[5], key[6], key[7]);
    store_bytes(cls_out + p0, cls);
    Seg total;
    (void)block_exclusive<OpReq, kT>(sum, lds, &total);
    if (threadIdx.x == 0) agg[blockIdx.x] = AdmitSeg{total.a, total.b, total.f, 0};
}

// In place: agg[i] = the fold of agg[0 .. i).  One workgroup; thread t owns the chunk [t * chunk, (t + 1) * chunk).
template <class Op>
__global__ __launch_bounds__(kScanThreads) void k_adm_tilescan(AdmitSeg* __restrict__ agg, uint32_t ntiles) {
    __shared__ Seg lds[2 * kScanThreads];
    const uint32_t chunk = (ntiles + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = threadIdx.x * chunk < ntiles ? threadIdx.x * chunk : ntiles;
    const uint32_t hi = ntiles - lo < chunk ? ntiles : lo + chunk;
    Seg sum{0, 0, 0};
    for (uint32_t i = lo; i < hi; ++i) {
        const AdmitSeg v = agg[i];
        sum = Op::op(sum, Seg{v.a, v.b, v.f});
    }
    Seg total;
    Seg run = block_exclusive<Op, kScanThreads>(sum, lds, &total);
    for (uint32_t i = lo; i < hi; ++i) {
        const AdmitSeg v = agg[i];
        agg[i] = AdmitSeg{run.a, run.b, run.f, 0};
        run = Op::op(run, Seg{v.a, v.b, v.f});
    }
}

__global__ __launch_bounds__(kT) void k_adm_decide(uint32_t n_act, const orl_act_state* __restrict__ state,
                                                   orl_admit_limits lim, const uint32_t* __restrict__ key_in,
                                                   uint8_t* __restrict__ cls_io, const AdmitSeg* __restrict__ carry1,
                                                   AdmitSeg* __restrict__ agg2) {
    __shared__ Seg lds[2 * kT];
    const size_t p0 = (size_t)blockIdx.x * kAdmitTile + (size_t)threadIdx.x * kI;
    uint32_t key[kI], cls[kI];
    load_words(key_in + p0, key);
    load_bytes(cls_io + p0, cls);
    Seg sum{0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) sum = OpReq::op(sum, seg_req(cls[k]));
    Seg total;
    const Seg ex = block_exclusive<OpReq, kT>(sum, lds, &total);
    const AdmitSeg cin = carry1[blockIdx.x];
    Seg run = OpReq::op(Seg{cin.a, cin.b, cin.f}, ex);
    Seg sum2{0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        const uint32_t c = cls[k];
        const Seg e = seg_req(c);
        const Seg x = e.f ? Seg{0, 0, 0} : run;  // the bucket's messages before p
        run = OpReq::op(run, e);
        const bool req = (c & kClsReq) != 0, ro = (c & kClsRo) != 0, exp = (c & kClsExp) != 0, resp = (c & kClsResp) != 0;
        const bool first = req && x.a == 0;
        const bool first_ro = first ? ro : x.b == 2u;
        uint32_t code = ORL_ADM_UNRESOLVED, sat = 0;
        if (key[k] < n_act) {
            const uint32_t* sw = reinterpret_cast<const uint32_t*>(state + key[k]);
            const uint32_t w0 = sw[0], num_running = sw[1];
            const uint32_t st = w0 & 0xFFu, fl = (w0 >> 8) & 0xFFu;
            const int64_t L = (fl & ORL_ACTF_STATELESS) ? lim.hard_stateless : lim.hard;
            const int64_t c0 = (int64_t)sw[2] + (int64_t)sw[3], q = (int64_t)x.a;
            const bool limited = L > 0;
            if (st == ORL_ACT_VALID) {
                if (limited && c0 > L) {
                    code = ORL_ADM_OVERLOADED;  // rule 1 from the first message on
                } else if (exp) {
                    code = ORL_ADM_EXPIRED;
                } else if (resp) {
                    code = ORL_ADM_RESPONSE;
                } else {
                    const bool set0 = (fl & ORL_ACTF_RUNNING_SET) != 0;
                    const bool run_ro = set0 ? (fl & ORL_ACTF_RUNNING_RO) != 0 : first_ro;
                    const bool alpha = (fl & ORL_ACTF_REENTRANT) || (c & kClsAi) || (run_ro && ro) ||
                                       (first && (num_running == 0 || !set0));
                    const bool full = limited && c0 + q >= L;  // q >= T
                    if (alpha) {
                        code = ORL_ADM_RUN;
                        sat = full ? kDecSat : 0u;
                    } else {
                        code = full ? ORL_ADM_OVERLOADED : ORL_ADM_ENQUEUE;
                    }
                }
            } else if (exp) {
                code = ORL_ADM_EXPIRED;
            } else if (st >= ORL_ACT_ABSENT) {
                code = ORL_ADM_NONEXISTENT;
            } else if (st == ORL_ACT_INVALID) {
                code = ORL_ADM_INVALID;
            } else if (resp) {
                code = ORL_ADM_RESPONSE;
            } else {
                code = (!limited || c0 + q <= L) ? ORL_ADM_ENQUEUE : ORL_ADM_OVERLOADED;
            }
        }
        const uint32_t dec = code | sat | ((c & kClsHead) ? kDecHead : 0u) | (first_ro ? kDecRo : 0u) |
                             ((req || x.a) ? kDecKnown : 0u);
        cls[k] = dec;
        sum2 = OpAdm::op(sum2, seg_adm(dec));
    }
    store_bytes(cls_io + p0, cls);
    (void)block_exclusive<OpAdm, kT>(sum2, lds, &total);
    if (threadIdx.x == 0) agg2[blockIdx.x] = AdmitSeg{total.a, total.b, total.f, 0};
}

__global__ __launch_bounds__(kT) void k_adm_resolve(size_t n, uint32_t n_act, const uint32_t* __restrict__ order,
                                                    bool order_vec, const uint32_t* __restrict__ key_in,
                                                    const uint8_t* __restrict__ dec_in, const AdmitSeg* __restrict__ carry2,
                                                    orl_act_state* __restrict__ state, uint8_t* __restrict__ disp,
                                                    uint64_t* __restrict__ counts) {
    __shared__ Seg lds[2 * kT];
    __shared__ uint32_t cnt_lds[8];
    const size_t p0 = (size_t)blockIdx.x * kAdmitTile + (size_t)threadIdx.x * kI;
    uint32_t idx[kI], dec[kI];
    load_order(order, p0, n, order_vec, idx);
    load_bytes(dec_in + p0, dec);
    if (threadIdx.x < 8) cnt_lds[threadIdx.x] = 0;  // ordered before its use by block_exclusive's barriers
    Seg sum{0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) sum = OpAdm::op(sum, seg_adm(dec[k]));
    Seg total;
    const Seg ex = block_exclusive<OpAdm, kT>(sum, lds, &total);
    const AdmitSeg cin = carry2[blockIdx.x];
    Seg run = OpAdm::op(Seg{cin.a, cin.b, cin.f}, ex);
    // the head bit of the position after this thread's last: the next thread's first, in the padded array
    const uint32_t next_dec = p0 + kI < n ? dec_in[p0 + kI] : 0u;
    uint32_t code[kI];
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        const Seg e = seg_adm(dec[k]);
        const Seg x = (e.f & 1u) ? Seg{0, 0, 0} : run;
        run = OpAdm::op(run, e);
        code[k] = kNoCode;
        if (p0 + k < n) {
            code[k] = (x.f & 2u) ? ORL_ADM_OVERLOADED : (dec[k] & kDecCode);  // rule 1 after saturation
            disp[idx[k]] = (uint8_t)code[k];
            const uint32_t nd = k + 1 < kI ? dec[(k + 1) % kI] : next_dec;
            const bool last = p0 + k + 1 == n || (nd & kDecHead);
            if (last && (run.a | run.b)) {  // run = the whole bucket's runs and enqueues
                const uint32_t a = key_in[p0 + k];
                if (a < n_act) {
                    uint32_t* sw = reinterpret_cast<uint32_t*>(state + a);
                    if (run.a) {
                        uint32_t w0 = sw[0];
                        if (!(w0 & (ORL_ACTF_RUNNING_SET << 8))) {  // RecordRunning: the bucket's first request
                            w0 = (w0 & ~(ORL_ACTF_RUNNING_RO << 8)) | (ORL_ACTF_RUNNING_SET << 8) |
                                 ((dec[k] & kDecRo) ? ORL_ACTF_RUNNING_RO << 8 : 0u);
                            sw[0] = w0;
                        }
                        sw[1] += run.a;
                        sw[2] += run.a;
                    }
                    if (run.b) sw[3] += run.b;
                }
            }
        }
    }
    if (counts) {  // uniform; every lane of the wave reaches the ballots
        uint32_t wc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < kI; ++k) {
#pragma unroll
            for (uint32_t q = 0; q < 8; ++q) wc[q] += (uint32_t)__popcll(__ballot(code[k] == q));
        }
        if ((threadIdx.x & 63u) == 0) {
#pragma unroll
            for (uint32_t q = 0; q < 8; ++q)
                if (wc[q]) atomicAdd(&cnt_lds[q], wc[q]);
        }
        __syncthreads();
        if (threadIdx.x < 8 && cnt_lds[threadIdx.x])
            atomicAdd(reinterpret_cast<unsigned long long*>(counts + threadIdx.x), (unsigned long long)cnt_lds[threadIdx.x]);
    }
}

uint64_t pad_tile(uint64_t v) { return (v + kAdmitTile - 1) / kAdmitTile * kAdmitTile; }

}  // namespace

int admit_alloc(AdmitScratch* s, uint64_t max_batch) {
    if (s->base) return 0;
    const uint64_t cap = pad_tile(max_batch ? max_batch : 1), tiles = cap / kAdmitTile;
    const uint64_t b_key = cap * sizeof(uint32_t), b_cls = pad_tile(cap), b_agg = tiles * sizeof(AdmitSeg);
    void* base = nullptr;
    hipError_t e = hipMalloc(&base, b_key + b_cls + 2 * b_agg);
    if (e != hipSuccess) return (int)e;
    uint8_t* p = static_cast<uint8_t*>(base);
    s->base = base;
    s->cap = max_batch;
    s->key = reinterpret_cast<uint32_t*>(p);
    s->cls = p + b_key;
    s->agg1 = reinterpret_cast<AdmitSeg*>(p + b_key + b_cls);
    s->agg2 = s->agg1 + tiles;
    return 0;
}

void admit_free(AdmitScratch* s) {
    if (s->base) (void)hipFree(s->base);
    *s = AdmitScratch{};
}

int launch_admit(const uint8_t* d_mflags, size_t n, uint32_t n_act, const uint32_t* d_order,
                 const uint32_t* d_off, orl_act_state* d_state, orl_admit_limits lim, uint8_t* d_disp, uint64_t* d_counts,
                 const AdmitScratch& s, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (d_counts) {
        hipError_t e = hipMemsetAsync(d_counts, 0, 8 * sizeof(uint64_t), st);
        if (e != hipSuccess) return (int)e;
    }
    if (n == 0) return 0;
    const uint32_t tiles = (uint32_t)((n + kAdmitTile - 1) / kAdmitTile);
    const bool order_vec = ((uintptr_t)d_order & 15u) == 0;
    hipLaunchKernelGGL(k_adm_classify, dim3(tiles), dim3(kT), 0, st, d_mflags, n, n_act, d_order, order_vec, d_off,
                       s.key, s.cls, s.agg1);
    hipLaunchKernelGGL(k_adm_tilescan<OpReq>, dim3(1), dim3(kScanThreads), 0, st, s.agg1, tiles);
    hipLaunchKernelGGL(k_adm_decide, dim3(tiles), dim3(kT), 0, st, n_act, d_state, lim, s.key, s.cls, s.agg1, s.agg2);
    hipLaunchKernelGGL(k_adm_tilescan<OpAdm>, dim3(1), dim3(kScanThreads), 0, st, s.agg2, tiles);
    hipLaunchKernelGGL(k_adm_resolve, dim3(tiles), dim3(kT), 0, st, n, n_act, d_order, order_vec, s.key, s.cls, s.agg2,
                       d_state, d_disp, d_counts);
    return (int)hipGetLastError();
}

}  // namespace orl
