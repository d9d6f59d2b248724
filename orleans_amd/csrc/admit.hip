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
#include "tile_scan_dev.h"

namespace orl {

namespace {

constexpr uint32_t kT = kTileThreads, kI = kTileItems;

// cls[p] as k_adm_classify writes it
constexpr uint32_t kClsReq = 0x01, kClsRo = 0x02, kClsAi = 0x04, kClsExp = 0x08, kClsResp = 0x10, kClsHead = 0x20;
// cls[p] as k_adm_decide rewrites it: code | kDecSat (this message saturates its bucket) | kDecHead | kDecRo, kDecKnown
// (the bucket's first request is known at p, and read-only)
constexpr uint32_t kDecCode = 0x07, kDecSat = 0x08, kDecHead = 0x10, kDecRo = 0x20, kDecKnown = 0x40;
constexpr uint32_t kNoCode = 0xFF;

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

// The key of a position comes from the offsets, not from act[order[p]]: a search per thread and one more per bucket
// boundary inside its 8 positions (the next bucket first), against a random 4-byte gather per position.
__global__ __launch_bounds__(kT) void k_adm_classify(const uint8_t* __restrict__ mflags, size_t n, uint32_t n_act,
                                                     const uint32_t* __restrict__ order, bool order_vec,
                                                     const uint32_t* __restrict__ off, uint32_t* __restrict__ key_out,
                                                     uint8_t* __restrict__ cls_out, SegAgg* __restrict__ agg) {
    __shared__ Seg lds[2 * kT];
    const size_t p0 = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kI;
    uint32_t idx[kI], key[kI], cls[kI], head = 0;
    load_order(order, p0, n, order_vec, idx);
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) cls[k] = p0 + k < n ? mflags[idx[k]] : 0u;  // 8 gathers in flight together
    bucket_keys(off, n_act, p0, n, key, &head);
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
    (void)block_exclusive<Seg, OpReq, kT>(sum, lds, &total);
    if (threadIdx.x == 0) agg[blockIdx.x] = SegAgg(total);
}

// In place: agg[i] = the fold of agg[0 .. i) (tile_scan_body).
template <class Op>
__global__ __launch_bounds__(kScanThreads) void k_adm_tilescan(SegAgg* __restrict__ agg, uint32_t ntiles) {
    __shared__ Seg lds[2 * kScanThreads];
    tile_scan_body<Seg, SegAgg, Op>(agg, ntiles, lds);
}

__global__ __launch_bounds__(kT) void k_adm_decide(uint32_t n_act, const orl_act_state* __restrict__ state,
                                                   orl_admit_limits lim, const uint32_t* __restrict__ key_in,
                                                   uint8_t* __restrict__ cls_io, const SegAgg* __restrict__ carry1,
                                                   SegAgg* __restrict__ agg2) {
    __shared__ Seg lds[2 * kT];
    const size_t p0 = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kI;
    uint32_t key[kI], cls[kI];
    load_words(key_in + p0, key);
    load_bytes(cls_io + p0, cls);
    Seg sum{0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) sum = OpReq::op(sum, seg_req(cls[k]));
    Seg total;
    const Seg ex = block_exclusive<Seg, OpReq, kT>(sum, lds, &total);
    const SegAgg cin = carry1[blockIdx.x];
    Seg run = OpReq::op(Seg(cin), ex);
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
    (void)block_exclusive<Seg, OpAdm, kT>(sum2, lds, &total);
    if (threadIdx.x == 0) agg2[blockIdx.x] = SegAgg(total);
}

__global__ __launch_bounds__(kT) void k_adm_resolve(size_t n, uint32_t n_act, const uint32_t* __restrict__ order,
                                                    bool order_vec, const uint32_t* __restrict__ key_in,
                                                    const uint8_t* __restrict__ dec_in, const SegAgg* __restrict__ carry2,
                                                    orl_act_state* __restrict__ state, uint8_t* __restrict__ disp,
                                                    uint64_t* __restrict__ counts) {
    __shared__ Seg lds[2 * kT];
    __shared__ uint32_t cnt_lds[8];
    const size_t p0 = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kI;
    uint32_t idx[kI], dec[kI];
    load_order(order, p0, n, order_vec, idx);
    load_bytes(dec_in + p0, dec);
    if (threadIdx.x < 8) cnt_lds[threadIdx.x] = 0;  // ordered before its use by block_exclusive's barriers
    Seg sum{0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) sum = OpAdm::op(sum, seg_adm(dec[k]));
    Seg total;
    const Seg ex = block_exclusive<Seg, OpAdm, kT>(sum, lds, &total);
    const SegAgg cin = carry2[blockIdx.x];
    Seg run = OpAdm::op(Seg(cin), ex);
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
    if (counts) ballot_counts<8>(code, cnt_lds, counts);  // uniform; every lane of the wave reaches the ballots
}

}  // namespace

int admit_alloc(AdmitScratch* s, uint64_t max_batch) {
    if (s->base) return 0;
    const uint64_t cap = pad_to(max_batch ? max_batch : 1, kScanTile), tiles = cap / kScanTile;
    const uint64_t b_key = cap * sizeof(uint32_t), b_cls = cap, b_agg = tiles * sizeof(SegAgg);
    void* base = nullptr;
    hipError_t e = hipMalloc(&base, b_key + b_cls + 2 * b_agg);
    if (e != hipSuccess) return (int)e;
    Carve c(base);
    s->base = base;
    s->cap = max_batch;
    s->key = c.take<uint32_t>(b_key);
    s->cls = c.take(b_cls);
    s->agg1 = c.take<SegAgg>(b_agg);
    s->agg2 = c.take<SegAgg>(b_agg);
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
    const uint32_t tiles = (uint32_t)((n + kScanTile - 1) / kScanTile);
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
