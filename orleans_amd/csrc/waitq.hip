// waitq.hip — the per-activation waiting queues on the device (gfx950): the append that follows admission, and request
// completion with the message pump.
//
// Admission (admit.hip) answers ORL_ADM_ENQUEUE for a message that has to wait; the reference then puts it on the
// activation's waiting list (ActivationData.EnqueueMessage, ActivationData.cs:487-514), and when a request completes it
// resets Running (ActivationData.ResetRunning, :424-442) and runs the message pump (Dispatcher.RunMessagePump,
// Dispatcher.cs:633-685), which takes waiting messages from the head while ActivationMayAcceptRequest (:316-338) holds.
// The model and its citations are at orl_waitq in include/orleans_route.h and in DESIGN §17.  Here the store is one CSR
// (off[n_act + 1]; tok / act / mflags per record, sorted by activation, FIFO inside it), double-buffered: every call
// streams the current buffer into the other one.
//
// Append.  One scan over the positions of `order` carries (ENQUEUEs before the position, "a RUN was seen since the
// bucket head").  With E(a) = the scan value at bucket_offsets[a]: old record j of activation a moves to j + E(a), the
// ENQUEUE at position p of bucket a lands at old_off[a + 1] + enq_before[p], new_off[a] = old_off[a] + E(a).
//   k_wq_app_classify  gathers disp[order[p]], finds the bucket and its head in the offsets; writes key[p], cls[p], aggregate
//   k_wq_tilescan      exclusive scan of the tile aggregates (one workgroup)
//   k_wq_app_scatter   the scan inside the tile; writes pre[p] and the new records; the bucket's first RUN records Running
//   k_wq_app_offsets   new_off[a] = old_off[a] + pre[bucket_offsets[a]]
//   k_wq_app_move      old records to their new places
//
// Complete.  With Running's own completion first, an activation's records equal "apply all completions, then pump
// once" (DESIGN §17), and the pump's result is a closed form over the segment: a record is taken iff no record at or
// before it in its segment fails.
//   k_wq_mark          per record (message order): marks (Running completed, pump, drain) and the count of pump / drain
//                      records per activation in dense scratch; k = the bucket's length - that count
//   k_wq_cmp_classify  per waiting record: gathers its activation's state, marks and the segment head's flags; writes the
//                      record's class (fails, head, drained), aggregate
//   k_wq_tilescan
//   k_wq_cmp_resolve   the scan inside the tile: (records out before the record, "a failure was seen in this segment");
//                      writes the out list, the surviving store and pre[i]
//   k_wq_cmp_finish    per activation: new_off[a] = off[a] - pre[off[a]]; one lane per touched activation writes its
//                      orl_act_state and running_tok
// orl_act_state is read by k_wq_cmp_classify only and written by k_wq_cmp_finish only (one lane per entry).  Both scans
// are reduce-then-scan over fixed tiles; no workgroup waits for another, no lane walks a segment, every loop is bounded by
// a count.  The only atomics are k_wq_mark's marks and the d_counts sums.

#include <hip/hip_runtime.h>

#include "tile_scan_dev.h"
#include "waitq.h"

namespace orl {

namespace {

constexpr uint32_t kT = kTileThreads, kI = kTileItems;

// cls[p] of append
constexpr uint32_t kAppEnq = 0x01, kAppRun = 0x02, kAppHead = 0x04;
// cls[i] of complete
constexpr uint32_t kCmpFail = 0x01, kCmpHead = 0x02, kCmpDrained = 0x04;
// mark[a]
constexpr uint32_t kMarkR = 0x01, kMarkPump = 0x02, kMarkDrain = 0x04;

// Append's scan.  a = ENQUEUEs (never reset), b = 1: a RUN since the span's last bucket head, f = 1: holds a head.
struct OpApp {
    static __device__ __forceinline__ Seg op(Seg x, Seg y) { return Seg{x.a + y.a, (y.f & 1u) ? y.b : (x.b | y.b), x.f | y.f}; }
};

__device__ __forceinline__ Seg seg_app(uint32_t cls) {
    return Seg{cls & kAppEnq, (cls & kAppRun) ? 1u : 0u, (cls & kAppHead) ? 1u : 0u};
}

// Complete's scan.  A span is a function of "a failure is carried into it" (c): records out = a + (c ? 0 : b), where b
// counts the records before the span's first head; failure carried out = f & 2 if the span holds a head (f & 1), else
// c | (f & 2).  op is the composition.
struct OpOut {
    static __device__ __forceinline__ Seg op(Seg x, Seg y) {
        const uint32_t add = (x.f & 2u) ? 0u : y.b;
        Seg r;
        if (x.f & 1u) {
            r.a = x.a + y.a + add;
            r.b = x.b;
        } else {
            r.a = y.a;
            r.b = x.b + add;
        }
        r.f = ((x.f | y.f) & 1u) | ((y.f & 1u) ? (y.f & 2u) : ((x.f | y.f) & 2u));
        return r;
    }
};

__device__ __forceinline__ Seg seg_out(uint32_t cls) {
    const uint32_t ok = (cls & kCmpFail) ? 0u : 1u;
    if (cls & kCmpHead) return Seg{ok, 0u, 1u | (ok ? 0u : 2u)};
    return Seg{0u, ok, ok ? 0u : 2u};
}

// ---- append ----------------------------------------------------------------------------------------------------------
// The key of a position comes from the offsets, as in admission: a search per thread and one more per
// bucket boundary inside its 8 positions (the next bucket first).
__global__ __launch_bounds__(kT) void k_wq_app_classify(const uint8_t* __restrict__ disp, size_t n, uint32_t n_act,
                                                        const uint32_t* __restrict__ order, bool order_vec,
                                                        const uint32_t* __restrict__ off, uint32_t* __restrict__ key_out,
                                                        uint8_t* __restrict__ cls_out, SegAgg* __restrict__ agg) {
    __shared__ Seg lds[2 * kT];
    const size_t p0 = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kI;
    uint32_t idx[kI], key[kI], cls[kI], head = 0;
    load_order(order, p0, n, order_vec, idx);
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) cls[k] = p0 + k < n ? disp[idx[k]] : 0xFFu;  // 8 gathers in flight together
    bucket_keys(off, n_act, p0, n, key, &head);
    Seg sum{0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        const bool live = key[k] < n_act;  // bucket n_act (unresolved) contributes nothing
        cls[k] = (live && cls[k] == ORL_ADM_ENQUEUE ? kAppEnq : 0u) | (live && cls[k] == ORL_ADM_RUN ? kAppRun : 0u) |
                 ((head >> k & 1u) ? kAppHead : 0u);
        sum = OpApp::op(sum, seg_app(cls[k]));
    }
    uint4* ko = reinterpret_cast<uint4*>(key_out + p0);
    ko[0] = make_uint4(key[0], key[1], key[2], key[3]);
    ko[1] = make_uint4(key[4], key[5], key[6], key[7]);
    store_bytes(cls_out + p0, cls);
    Seg total;
    (void)block_exclusive<Seg, OpApp, kT>(sum, lds, &total);
    if (threadIdx.x == 0) agg[blockIdx.x] = SegAgg(total);
}

// In place: agg[i] = the fold of agg[0 .. i) (tile_scan_body).
template <class Op>
__global__ __launch_bounds__(kScanThreads) void k_wq_tilescan(SegAgg* __restrict__ agg, uint32_t ntiles) {
    __shared__ Seg lds[2 * kScanThreads];
    tile_scan_body<Seg, SegAgg, Op>(agg, ntiles, lds);
}

__global__ __launch_bounds__(kT) void k_wq_app_scatter(const uint32_t* __restrict__ tok, const uint8_t* __restrict__ mflags,
                                                       size_t n, const uint32_t* __restrict__ order, bool order_vec,
                                                       const uint32_t* __restrict__ key_in, const uint8_t* __restrict__ cls_in,
                                                       const SegAgg* __restrict__ carry, const uint32_t* __restrict__ old_off,
                                                       uint32_t* __restrict__ new_tok, uint32_t* __restrict__ new_act,
                                                       uint8_t* __restrict__ new_mflags, uint32_t* __restrict__ running_tok,
                                                       uint32_t* __restrict__ pre) {
    __shared__ Seg lds[2 * kT];
    const size_t p0 = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kI;
    uint32_t idx[kI], key[kI], cls[kI];
    load_order(order, p0, n, order_vec, idx);
    load_words(key_in + p0, key);
    load_bytes(cls_in + p0, cls);
    Seg sum{0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) sum = OpApp::op(sum, seg_app(cls[k]));
    Seg total;
    const Seg ex = block_exclusive<Seg, OpApp, kT>(sum, lds, &total);
    const SegAgg cin = carry[blockIdx.x];
    Seg run = OpApp::op(Seg(cin), ex);
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        const uint32_t c = cls[k];
        const uint32_t before = run.a, seen = (c & kAppHead) ? 0u : run.b;
        run = OpApp::op(run, seg_app(c));
        if (p0 + k < n) {
            pre[p0 + k] = before;
            if (p0 + k + 1 == n) pre[n] = run.a;
            if (c & kAppEnq) {  // EnqueueMessage: behind the activation's old records and its earlier ENQUEUEs
                const size_t dst = (size_t)old_off[key[k] + 1] + before;
                new_tok[dst] = tok[idx[k]];
                new_act[dst] = key[k];
                new_mflags[dst] = mflags[idx[k]];
            }
            if ((c & kAppRun) && !seen && running_tok[key[k]] == ORL_TOK_NONE)  // RecordRunning keeps the first;
                running_tok[key[k]] = tok[idx[k]];                              // one lane per activation
        }
    }
}

__global__ __launch_bounds__(kT) void k_wq_app_offsets(uint32_t n_act, const uint32_t* __restrict__ boff,
                                                       const uint32_t* __restrict__ pre, const uint32_t* __restrict__ old_off,
                                                       uint32_t* __restrict__ new_off, uint64_t* __restrict__ waiting_n) {
    const uint32_t a = blockIdx.x * kT + threadIdx.x;
    if (a > n_act) return;
    const uint32_t v = old_off[a] + pre[boff[a]];  // boff[a] <= n, pre[n] = all ENQUEUEs
    new_off[a] = v;
    if (a == n_act) *waiting_n = v;
}

// Records [0, old_off[n_act]) of the old buffer; the grid covers the host's bound of that length.
__global__ __launch_bounds__(kT) void k_wq_app_move(uint32_t n_act, const uint32_t* __restrict__ old_off,
                                                    const uint32_t* __restrict__ new_off, const uint32_t* __restrict__ old_tok,
                                                    const uint32_t* __restrict__ old_act, const uint8_t* __restrict__ old_mflags,
                                                    uint32_t* __restrict__ new_tok, uint32_t* __restrict__ new_act,
                                                    uint8_t* __restrict__ new_mflags) {
    const size_t i0 = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kI;
    const size_t len = old_off[n_act];
    if (i0 >= len) return;
    uint32_t t[kI], a[kI], f[kI];
    stream_words(old_tok + i0, t);
    stream_words(old_act + i0, a);
    stream_bytes(old_mflags + i0, f);
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        if (i0 + k < len) {
            const size_t dst = i0 + k + (new_off[a[k]] - old_off[a[k]]);  // + E(a)
            new_tok[dst] = t[k];
            new_act[dst] = a[k];
            new_mflags[dst] = (uint8_t)f[k];
        }
    }
}

// ---- complete --------------------------------------------------------------------------------------------------------
// counts (when given): [0] completions, [1] pump requests, [2] drain requests, [3] records with a handle >= n_act.
__global__ __launch_bounds__(kT) void k_wq_mark(const uint32_t* __restrict__ cact, const uint32_t* __restrict__ ctok, size_t m,
                                                uint32_t n_act, const uint32_t* __restrict__ running_tok,
                                                uint32_t* __restrict__ mark, uint32_t* __restrict__ nonc,
                                                uint64_t* __restrict__ counts) {
    __shared__ uint32_t cnt_lds[4];
    if (threadIdx.x < 4) cnt_lds[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * kScanTile + threadIdx.x;
    uint32_t kind[kI];
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        const size_t j = base + (size_t)k * kT;
        kind[k] = 0xFFu;
        if (j < m) {
            const uint32_t a = __builtin_nontemporal_load(cact + j), t = __builtin_nontemporal_load(ctok + j);
            if (a >= n_act) {
                kind[k] = 3;
            } else if (t == ORL_TOK_NONE) {
                kind[k] = 1;
                atomicOr(&mark[a], kMarkPump);
                atomicAdd(&nonc[a], 1u);
            } else if (t == ORL_TOK_DRAIN) {
                kind[k] = 2;
                atomicOr(&mark[a], kMarkDrain);
                atomicAdd(&nonc[a], 1u);
            } else {
                kind[k] = 0;
                if (running_tok[a] == t) atomicOr(&mark[a], kMarkR);
            }
        }
    }
    if (counts) ballot_counts<4>(kind, cnt_lds, counts);  // uniform; every lane of the wave reaches the ballots
}

// An activation's state after steps 1-2 (all its completions applied), from its entry, marks and bucket.
struct Applied {
    uint32_t state, flags, num_running, in_flight, waiting;
    bool underflow;
};

__device__ __forceinline__ Applied apply_completions(const orl_act_state* __restrict__ e, uint32_t mk, uint32_t k) {
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(e);
    const uint32_t w0 = sw[0];
    Applied s;
    s.state = w0 & 0xFFu;
    s.flags = (w0 >> 8) & 0xFFu;
    s.underflow = k > sw[1] || k > sw[2];
    s.num_running = sw[1] > k ? sw[1] - k : 0u;  // ResetRunning per completion, saturating
    s.in_flight = sw[2] > k ? sw[2] - k : 0u;    // InvokeWorkItem.cs:70,79
    s.waiting = sw[3];
    if (mk & kMarkR) s.flags &= ~(ORL_ACTF_RUNNING_SET | ORL_ACTF_RUNNING_RO);  // ActivationData.cs:438-441
    return s;
}

// Records [0, off[n_act]); the grid covers the host's bound of that length.  Consecutive records read equal or
// consecutive entries of every per-activation array.
__global__ __launch_bounds__(kT) void k_wq_cmp_classify(uint32_t n_act, const uint32_t* __restrict__ off,
                                                        const uint32_t* __restrict__ act, const uint8_t* __restrict__ mflags,
                                                        const uint32_t* __restrict__ cboff, const uint32_t* __restrict__ mark,
                                                        const uint32_t* __restrict__ nonc,
                                                        const orl_act_state* __restrict__ state,
                                                        uint8_t* __restrict__ cls_out, SegAgg* __restrict__ agg) {
    __shared__ Seg lds[2 * kT];
    const size_t i0 = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kI;
    const size_t len = off[n_act];
    uint32_t a[kI], f[kI], cls[kI];
    stream_words(act + i0, a);
    stream_bytes(mflags + i0, f);
    Seg sum{0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        uint32_t c = kCmpFail | kCmpHead;  // past the end: a segment of its own that gives nothing
        if (i0 + k < len) {
            const uint32_t h = a[k], o = off[h];
            const uint32_t nrec = cboff[h + 1] - cboff[h];
            bool ok = false, drained = false;
            const bool head = i0 + k == o;
            if (nrec) {
                const uint32_t mk = mark[h];
                if (mk & kMarkDrain) {
                    ok = drained = true;  // DequeueAllWaitingMessages
                } else {
                    const Applied s = apply_completions(state + h, mk, nrec - nonc[h]);
                    if (s.state == ORL_ACT_VALID) {  // Dispatcher.cs:669; then :316-338 per record
                        const bool set = (s.flags & ORL_ACTF_RUNNING_SET) != 0, reent = (s.flags & ORL_ACTF_REENTRANT) != 0;
                        const bool ai = (f[k] & ORL_MF_ALWAYS_INTERLEAVE) != 0, ro = (f[k] & ORL_MF_READ_ONLY) != 0;
                        if (head) {
                            ok = s.num_running == 0 || reent || ai || !set || ((s.flags & ORL_ACTF_RUNNING_RO) && ro);
                        } else {  // behind a taken head Running is set: the state's, or the head itself
                            const bool rro = set ? (s.flags & ORL_ACTF_RUNNING_RO) != 0 : (mflags[o] & ORL_MF_READ_ONLY) != 0;
                            ok = reent || ai || (rro && ro);
                        }
                    }
                }
            }
            c = (ok ? 0u : kCmpFail) | (head ? kCmpHead : 0u) | (drained ? kCmpDrained : 0u);
        }
        cls[k] = c;
        sum = OpOut::op(sum, seg_out(c));
    }
    store_bytes(cls_out + i0, cls);
    Seg total;
    (void)block_exclusive<Seg, OpOut, kT>(sum, lds, &total);
    if (threadIdx.x == 0) agg[blockIdx.x] = SegAgg(total);
}

__global__ __launch_bounds__(kT) void k_wq_cmp_resolve(uint32_t n_act, const uint32_t* __restrict__ off,
                                                       const uint32_t* __restrict__ tok, const uint32_t* __restrict__ act,
                                                       const uint8_t* __restrict__ mflags, const uint8_t* __restrict__ cls_in,
                                                       const SegAgg* __restrict__ carry, uint32_t* __restrict__ new_tok,
                                                       uint32_t* __restrict__ new_act, uint8_t* __restrict__ new_mflags,
                                                       uint32_t* __restrict__ out_tok, uint32_t* __restrict__ out_act,
                                                       uint8_t* __restrict__ out_mflags, uint8_t* __restrict__ out_kind,
                                                       uint32_t* __restrict__ pre) {
    __shared__ Seg lds[2 * kT];
    const size_t i0 = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kI;
    const size_t len = off[n_act];
    uint32_t t[kI], a[kI], f[kI], cls[kI];
    stream_words(tok + i0, t);
    stream_words(act + i0, a);
    stream_bytes(mflags + i0, f);
    load_bytes(cls_in + i0, cls);
    Seg sum{0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) sum = OpOut::op(sum, seg_out(cls[k]));
    Seg total;
    const Seg ex = block_exclusive<Seg, OpOut, kT>(sum, lds, &total);
    const SegAgg cin = carry[blockIdx.x];
    const Seg p = OpOut::op(Seg(cin), ex);
    uint32_t cnt = p.a + p.b;  // nothing is carried into record 0
    bool failed = (p.f & 2u) != 0;
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        const uint32_t c = cls[k];
        if (c & kCmpHead) failed = false;
        failed = failed || (c & kCmpFail);
        const size_t i = i0 + k;
        if (i < len) {
            pre[i] = cnt;
            if (!failed) {
                out_tok[cnt] = t[k];
                out_act[cnt] = a[k];
                out_mflags[cnt] = (uint8_t)f[k];
                out_kind[cnt] = (c & kCmpDrained) ? ORL_WQ_DRAINED : ORL_WQ_RUN;
                cnt += 1;
            } else {
                const size_t dst = i - cnt;
                new_tok[dst] = t[k];
                new_act[dst] = a[k];
                new_mflags[dst] = (uint8_t)f[k];
            }
            if (i + 1 == len) pre[len] = cnt;
        }
    }
}

// One lane per activation (and one for off[n_act]).  scanned = 0: the store is empty by the host's bound and pre was not
// written.  counts (when given): [4] underflowing activations, [5] records run, [6] records drained, [7] still waiting.
__global__ __launch_bounds__(kT) void k_wq_cmp_finish(uint32_t n_act, int scanned, const uint32_t* __restrict__ off,
                                                      uint32_t* __restrict__ new_off, const uint32_t* __restrict__ pre,
                                                      const uint32_t* __restrict__ cboff, const uint32_t* __restrict__ mark,
                                                      const uint32_t* __restrict__ nonc, const uint32_t* __restrict__ tok,
                                                      const uint8_t* __restrict__ mflags, orl_act_state* __restrict__ state,
                                                      uint32_t* __restrict__ running_tok, uint64_t* __restrict__ out_n,
                                                      uint64_t* __restrict__ waiting_n, uint64_t* __restrict__ counts) {
    __shared__ uint32_t cnt_lds[3];
    if (threadIdx.x < 3) cnt_lds[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t a = blockIdx.x * kT + threadIdx.x;
    if (a <= n_act) {
        const bool have = scanned && off[n_act] != 0;
        const uint32_t o = off[a], before = have ? pre[o] : 0u;
        new_off[a] = o - before;
        if (a == n_act) {
            *out_n = before;
            *waiting_n = o - before;
            if (counts) counts[7] = o - before;
        } else {
            const uint32_t nrec = cboff[a + 1] - cboff[a];
            if (nrec) {
                const uint32_t mk = mark[a];
                Applied s = apply_completions(state + a, mk, nrec - nonc[a]);
                const uint32_t o1 = off[a + 1], taken = (have ? pre[o1] : 0u) - before;
                uint32_t rt = (mk & kMarkR) ? ORL_TOK_NONE : running_tok[a];
                if (mk & kMarkDrain) {
                    s.waiting = 0;
                    if (taken) atomicAdd(&cnt_lds[2], taken);
                } else if (taken) {  // HandleIncomingRequest per record taken
                    s.waiting -= taken;
                    s.num_running += taken;
                    s.in_flight += taken;
                    if (!(s.flags & ORL_ACTF_RUNNING_SET)) {  // RecordRunning: the head
                        s.flags = (s.flags & ~ORL_ACTF_RUNNING_RO) | ORL_ACTF_RUNNING_SET |
                                  ((mflags[o] & ORL_MF_READ_ONLY) ? ORL_ACTF_RUNNING_RO : 0u);
                        rt = tok[o];
                    }
                    atomicAdd(&cnt_lds[1], taken);
                }
                if (s.underflow) atomicAdd(&cnt_lds[0], 1u);
                uint32_t* sw = reinterpret_cast<uint32_t*>(state + a);
                sw[0] = (sw[0] & 0xFFFF00FFu) | (s.flags << 8);
                sw[1] = s.num_running;
                sw[2] = s.in_flight;
                sw[3] = s.waiting;
                running_tok[a] = rt;
            }
        }
    }
    if (counts) {
        __syncthreads();
        flush_counts<3>(cnt_lds, counts + 4);
    }
}

// m == 0: an empty out list; nothing else changes.
__global__ void k_wq_cmp_empty(uint32_t n_act, const uint32_t* __restrict__ off, uint64_t* __restrict__ out_n,
                               uint64_t* __restrict__ counts) {
    *out_n = 0;
    if (counts) counts[7] = off[n_act];
}

}  // namespace

int waitq_alloc(orl_waitq** out, uint32_t n_act, uint64_t capacity, uint64_t max_batch) {
    *out = nullptr;
    const uint64_t cap = pad_to(capacity ? capacity : 1, kScanTile), batch = pad_to(max_batch ? max_batch : 1, kScanTile);
    const uint64_t big = cap > batch ? cap : batch, tiles = big / kScanTile;
    const uint64_t b_off = pad_to(((uint64_t)n_act + 1) * 4, 256), b_w = cap * 4, b_b = cap, b_act = pad_to((uint64_t)n_act * 4, 256);
    const uint64_t b_key = batch * 4, b_cls = big, b_pre = pad_to((big + 1) * 4, 256), b_agg = pad_to(tiles * sizeof(SegAgg), 256);
    const uint64_t total = 2 * (b_off + 2 * b_w + b_b) + b_act + (2 * b_w + 2 * b_b) + 256 + b_key + b_cls + b_pre +
                           2 * b_act + b_agg;
    void* base = nullptr;
    hipError_t e = hipMalloc(&base, total);
    if (e != hipSuccess) return (int)e;
    orl_waitq* q = new orl_waitq();
    Carve c(base);
    q->base = base;
    q->capacity = capacity;
    q->max_batch = max_batch;
    q->n_act = n_act;
    for (int i = 0; i < 2; ++i) {
        q->off[i] = c.take<uint32_t>(b_off);
        q->tok[i] = c.take<uint32_t>(b_w);
        q->act[i] = c.take<uint32_t>(b_w);
        q->mflags[i] = c.take(b_b);
    }
    q->running_tok = c.take<uint32_t>(b_act);
    q->out_tok = c.take<uint32_t>(b_w);
    q->out_act = c.take<uint32_t>(b_w);
    q->out_mflags = c.take(b_b);
    q->out_kind = c.take(b_b);
    q->out_n = c.take<uint64_t>(256);
    q->waiting_n = q->out_n + 1;
    q->key = c.take<uint32_t>(b_key);
    q->cls = c.take(b_cls);
    q->pre = c.take<uint32_t>(b_pre);
    q->mark = c.take<uint32_t>(b_act);  // mark and nonc are cleared together
    q->nonc = c.take<uint32_t>(b_act);
    q->agg = c.take<SegAgg>(b_agg);
    e = hipMemset(base, 0, total);
    if (e == hipSuccess) e = hipMemset(q->running_tok, 0xFF, b_act);
    // the fills run on the null stream and need not have finished; the first call may come on a non-blocking stream
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        waitq_free(q);
        return (int)e;
    }
    *out = q;
    return 0;
}

void waitq_free(orl_waitq* q) {
    if (!q) return;
    if (q->base) (void)hipFree(q->base);
    delete q;
}

int launch_waitq_append(const orl_waitq& q, uint64_t old_bound, const uint32_t* d_tok, const uint8_t* d_mflags, size_t n,
                        const uint32_t* d_order, const uint32_t* d_boff, const uint8_t* d_disp, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t c = q.cur, o = c ^ 1u;
    const uint32_t tiles = (uint32_t)((n + kScanTile - 1) / kScanTile);
    const bool order_vec = ((uintptr_t)d_order & 15u) == 0;
    hipLaunchKernelGGL(k_wq_app_classify, dim3(tiles), dim3(kT), 0, st, d_disp, n, q.n_act, d_order, order_vec, d_boff,
                       q.key, q.cls, q.agg);
    hipLaunchKernelGGL(k_wq_tilescan<OpApp>, dim3(1), dim3(kScanThreads), 0, st, q.agg, tiles);
    hipLaunchKernelGGL(k_wq_app_scatter, dim3(tiles), dim3(kT), 0, st, d_tok, d_mflags, n, d_order, order_vec, q.key, q.cls,
                       q.agg, q.off[c], q.tok[o], q.act[o], q.mflags[o], q.running_tok, q.pre);
    hipLaunchKernelGGL(k_wq_app_offsets, dim3(q.n_act / kT + 1), dim3(kT), 0, st, q.n_act, d_boff, q.pre, q.off[c], q.off[o],
                       q.waiting_n);
    if (old_bound) {
        const uint32_t rtiles = (uint32_t)((old_bound + kScanTile - 1) / kScanTile);
        hipLaunchKernelGGL(k_wq_app_move, dim3(rtiles), dim3(kT), 0, st, q.n_act, q.off[c], q.off[o], q.tok[c], q.act[c],
                           q.mflags[c], q.tok[o], q.act[o], q.mflags[o]);
    }
    return (int)hipGetLastError();
}

int launch_waitq_complete(const orl_waitq& q, const uint32_t* d_cact, const uint32_t* d_ctok, size_t m,
                          const uint32_t* d_cboff, orl_act_state* d_state, uint64_t* d_counts, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t c = q.cur, o = c ^ 1u;
    if (d_counts) {
        hipError_t e = hipMemsetAsync(d_counts, 0, 8 * sizeof(uint64_t), st);
        if (e != hipSuccess) return (int)e;
    }
    if (m == 0) {
        hipLaunchKernelGGL(k_wq_cmp_empty, dim3(1), dim3(1), 0, st, q.n_act, q.off[c], q.out_n, d_counts);
        return (int)hipGetLastError();
    }
    hipError_t e = hipMemsetAsync(q.mark, 0, (size_t)((uint8_t*)q.agg - (uint8_t*)q.mark), st);  // mark and nonc
    if (e != hipSuccess) return (int)e;
    const uint32_t mtiles = (uint32_t)((m + kScanTile - 1) / kScanTile);
    hipLaunchKernelGGL(k_wq_mark, dim3(mtiles), dim3(kT), 0, st, d_cact, d_ctok, m, q.n_act, q.running_tok, q.mark, q.nonc,
                       d_counts);
    const uint32_t rtiles = (uint32_t)((q.bound + kScanTile - 1) / kScanTile);
    if (rtiles) {
        hipLaunchKernelGGL(k_wq_cmp_classify, dim3(rtiles), dim3(kT), 0, st, q.n_act, q.off[c], q.act[c], q.mflags[c], d_cboff,
                           q.mark, q.nonc, d_state, q.cls, q.agg);
        hipLaunchKernelGGL(k_wq_tilescan<OpOut>, dim3(1), dim3(kScanThreads), 0, st, q.agg, rtiles);
        hipLaunchKernelGGL(k_wq_cmp_resolve, dim3(rtiles), dim3(kT), 0, st, q.n_act, q.off[c], q.tok[c], q.act[c], q.mflags[c],
                           q.cls, q.agg, q.tok[o], q.act[o], q.mflags[o], q.out_tok, q.out_act, q.out_mflags, q.out_kind,
                           q.pre);
    }
    hipLaunchKernelGGL(k_wq_cmp_finish, dim3(q.n_act / kT + 1), dim3(kT), 0, st, q.n_act, rtiles ? 1 : 0, q.off[c], q.off[o],
                       q.pre, d_cboff, q.mark, q.nonc, q.tok[c], q.mflags[c], d_state, q.running_tok, q.out_n, q.waiting_n,
                       d_counts);
    return (int)hipGetLastError();
}

}  // namespace orl
