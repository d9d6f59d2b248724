// collect.hip — the idle-activation collector on the device (gfx950): collection tickets, idleness, ScanStale / ScanAll.
//
// The reference keeps a ConcurrentDictionary of buckets keyed by ticket (ActivationCollector.cs); every message arrival
// (Catalog.GetOrCreateActivation, Catalog.cs:427) and every ResetRunning that reaches zero (ActivationData.cs:427-435)
// moves the activation's ticket, and a timer dequeues the due buckets (ScanStale, ActivationCollector.cs:226-284) or walks
// all of them (ScanAll, :291-345).  Here the buckets are not stored: ticket[a] and the cancelled bit carry everything the
// reference reads from them, because nextTicket only grows.  The model and its citations are at orl_collector in
// include/orleans_route.h and in DESIGN §18.
//
// Touch.
//   k_col_touch_mark   per message (message order, d_act / d_disp streamed): ORs "certain" / "overloaded seen" into mark[a]
//   k_col_touch_apply  per activation: decides the overloaded-only buckets from the state after admission, reschedules,
//                      clears the mark
// On-complete.
//   k_col_cmp_mark     per record: counts the ordinary-token records of an activation in mark[a]
//   k_col_cmp_apply    per activation: k >= 1 && k >= num_running -> became_idle = now, reschedule; clears the mark
// Scans (stream compaction over n_act, reduce-then-scan over tiles of 2048 = 256 x 8):
//   k_col_scan<.., false>  streams ticket[], decides each candidate, counts the condemned of the tile; writes nothing else
//   k_col_tilescan         exclusive scan of the tile counts (one workgroup); the total is the list's length
//   k_col_scan<.., true>   decides again from the same (unchanged) inputs, scans inside the tile, writes the collector
//                          arrays, orl_act_state.state and the condemned handles
// No workgroup waits for another, no lane walks a segment, every loop is bounded by a count.  Every array entry is written
// by one lane in one pass per call; the only atomics are the marks and the d_counts sums.  Times are 64-bit throughout.

#include <hip/hip_runtime.h>

#include "collect.h"
#include "tile_scan_dev.h"

namespace orl {

namespace {

constexpr uint32_t kT = kTileThreads, kI = kTileItems;

constexpr uint32_t kMarkCertain = 0x1, kMarkOverloaded = 0x2;

struct Cols {
    int64_t* ticket;
    int64_t* became_idle;
    int64_t* keep_alive_until;
    int64_t* age_limit;
    uint8_t* cflags;
};

Cols cols_of(const orl_collector& c) { return Cols{c.ticket, c.became_idle, c.keep_alive_until, c.age_limit, c.cflags}; }

// MakeTicketFromDateTime (ActivationCollector.cs:391-400): t rounded up to a multiple of the quantum; t > 0.
__device__ __forceinline__ int64_t make_ticket(int64_t t, int64_t quantum) { return ((t - 1) / quantum + 1) * quantum; }

// TryRescheduleCollection (ActivationCollector.cs:148-184) of entry a.  -> 0 nothing (exempt, or no ticket), else the
// d_counts slot of what happened: 1 moved, 2 same ticket, 3 expired ticket dropped, 4 cancelled ticket dropped, 5 bad
// timeout (MakeTicketFromTimeSpan would throw, :402-410: left unchanged).
constexpr uint32_t kRsMoved = 1, kRsSame = 2, kRsExpired = 3, kRsCancelled = 4, kRsBadTimeout = 5;

__device__ __forceinline__ uint32_t reschedule(const Cols& c, uint32_t a, int64_t now, int64_t quantum, int64_t next_ticket) {
    const uint32_t fl = c.cflags[a];
    if (fl & ORL_COLF_EXEMPT) return 0;
    const int64_t tk = c.ticket[a];
    if (tk == 0) return 0;
    if (tk < next_ticket) {  // IsExpired :386-389; _Impl fails, ResetCollectionTicket :156
        c.ticket[a] = 0;
        return kRsExpired;
    }
    const int64_t age = c.age_limit[a];
    if (age < quantum) return kRsBadTimeout;
    const int64_t nw = make_ticket(now + age, quantum);
    if (nw == tk) return kRsSame;  // :171, the cancelled flag stays
    if (fl & ORL_COLF_CANCELLED) {  // Bucket.TryRemove fails :457-474, then :156
        c.ticket[a] = 0;
        return kRsCancelled;
    }
    c.ticket[a] = nw;  // TryRemove sets the flag, Add clears it (:412-424)
    return kRsMoved;
}

// ---- schedule / cancel lists -------------------------------------------------------------------------------------------
// counts: [0] scheduled, [1] exempt, [2] age limit 0, [3] bad timeout, [4] already ticketed, [5] handles >= n_act.
__global__ __launch_bounds__(kT) void k_col_schedule(Cols c, const uint32_t* __restrict__ handles, size_t m, uint32_t n_act,
                                                     int64_t now, int64_t quantum, uint64_t* __restrict__ counts) {
    __shared__ uint32_t cnt[8];
    BlockCounts bc;
    bc.init(cnt);
    const size_t j = (size_t)blockIdx.x * kT + threadIdx.x;
    if (j < m) {
        const uint32_t a = handles[j];
        if (a >= n_act) {
            bc.add(5);
        } else {
            const uint32_t fl = c.cflags[a];
            const int64_t age = c.age_limit[a];
            if (fl & ORL_COLF_EXEMPT) bc.add(1);
            else if (age == 0) bc.add(2);
            else if (age < quantum) bc.add(3);
            else if (c.ticket[a] != 0) bc.add(4);
            else {
                c.ticket[a] = make_ticket(now + age, quantum);
                if (fl & ORL_COLF_CANCELLED) c.cflags[a] = (uint8_t)(fl & ~ORL_COLF_CANCELLED);
                bc.add(0);
            }
        }
    }
    bc.flush(counts);
}

// counts: [0] cancelled, [1] exempt, [2] no ticket, [3] expired ticket, [4] already cancelled, [5] handles >= n_act.
__global__ __launch_bounds__(kT) void k_col_cancel(Cols c, const uint32_t* __restrict__ handles, size_t m, uint32_t n_act,
                                                   int64_t next_ticket, uint64_t* __restrict__ counts) {
    __shared__ uint32_t cnt[8];
    BlockCounts bc;
    bc.init(cnt);
    const size_t j = (size_t)blockIdx.x * kT + threadIdx.x;
    if (j < m) {
        const uint32_t a = handles[j];
        if (a >= n_act) {
            bc.add(5);
        } else {
            const uint32_t fl = c.cflags[a];
            const int64_t tk = c.ticket[a];
            if (fl & ORL_COLF_EXEMPT) bc.add(1);
            else if (tk == 0) bc.add(2);
            else if (tk < next_ticket) bc.add(3);
            else if (fl & ORL_COLF_CANCELLED) bc.add(4);
            else {
                c.cflags[a] = (uint8_t)(fl | ORL_COLF_CANCELLED);
                bc.add(0);
            }
        }
    }
    bc.flush(counts);
}

// ---- touch -------------------------------------------------------------------------------------------------------------
// A set bit is not set again: the read may be stale, the OR is monotone.
__global__ __launch_bounds__(kT) void k_col_touch_mark(const uint32_t* __restrict__ act, const uint8_t* __restrict__ disp,
                                                       size_t n, uint32_t n_act, uint32_t* __restrict__ mark) {
    const size_t base = (size_t)blockIdx.x * kScanTile + threadIdx.x;
    uint32_t a[kI], d[kI];
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        const size_t i = base + (size_t)k * kT;
        a[k] = i < n ? __builtin_nontemporal_load(act + i) : 0xFFFFFFFFu;
        d[k] = i < n ? (uint32_t)__builtin_nontemporal_load(disp + i) : (uint32_t)ORL_ADM_UNRESOLVED;
    }
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        if (a[k] >= n_act) continue;
        uint32_t bit = 0;
        if (d[k] == ORL_ADM_RUN || d[k] == ORL_ADM_ENQUEUE || d[k] == ORL_ADM_RESPONSE || d[k] == ORL_ADM_INVALID) bit = kMarkCertain;
        else if (d[k] == ORL_ADM_OVERLOADED) bit = kMarkOverloaded;
        if (bit && !(mark[a[k]] & bit)) atomicOr(&mark[a[k]], bit);
    }
}

// counts: [0] activations touched, [1]-[5] reschedule's, [6] rule-1-only buckets (not touched), [7] rule-7-only buckets.
__global__ __launch_bounds__(kT) void k_col_touch_apply(Cols c, uint32_t n_act, uint32_t* __restrict__ mark,
                                                        const orl_act_state* __restrict__ state, int32_t hard,
                                                        int32_t hard_stateless, int64_t now, int64_t quantum,
                                                        int64_t next_ticket, uint64_t* __restrict__ counts) {
    __shared__ uint32_t cnt[8];
    BlockCounts bc;
    bc.init(cnt);
    const uint32_t a = blockIdx.x * kT + threadIdx.x;
    const uint32_t mk = a < n_act ? mark[a] : 0u;
    if (mk) {
        mark[a] = 0;
        bool touched = (mk & kMarkCertain) != 0;
        if (!touched) {  // OVERLOADED only: rule 1 (before the dispatcher) or rule 7 (after the lookup), DESIGN §18
            const uint32_t* sw = reinterpret_cast<const uint32_t*>(state + a);
            const uint32_t w0 = sw[0];
            const int64_t lim = ((w0 >> 8) & ORL_ACTF_STATELESS) ? hard_stateless : hard;
            const bool rule1 = (w0 & 0xFFu) == ORL_ACT_VALID && lim > 0 && (int64_t)sw[2] + (int64_t)sw[3] > lim;
            touched = !rule1;
            bc.add(rule1 ? 6 : 7);
        }
        if (touched) {
            bc.add(0);
            const uint32_t r = reschedule(c, a, now, quantum, next_ticket);
            if (r) bc.add(r);
        }
    }
    bc.flush(counts);
}

// ---- on-complete -------------------------------------------------------------------------------------------------------
// counts: [6] records with a handle >= n_act, [7] ordinary-token records.
__global__ __launch_bounds__(kT) void k_col_cmp_mark(const uint32_t* __restrict__ cact, const uint32_t* __restrict__ ctok,
                                                     size_t m, uint32_t n_act, uint32_t* __restrict__ mark,
                                                     uint64_t* __restrict__ counts) {
    __shared__ uint32_t cnt[8];
    BlockCounts bc;
    bc.init(cnt);
    const size_t base = (size_t)blockIdx.x * kScanTile + threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        const size_t j = base + (size_t)k * kT;
        if (j < m) {
            const uint32_t a = __builtin_nontemporal_load(cact + j), t = __builtin_nontemporal_load(ctok + j);
            if (a >= n_act) {
                bc.add(6);
            } else if (t != ORL_TOK_NONE && t != ORL_TOK_DRAIN) {
                atomicAdd(&mark[a], 1u);
                bc.add(7);
            }
        }
    }
    bc.flush(counts);
}

// counts: [0] activations that became idle, [1]-[5] reschedule's.
__global__ __launch_bounds__(kT) void k_col_cmp_apply(Cols c, uint32_t n_act, uint32_t* __restrict__ mark,
                                                      const orl_act_state* __restrict__ state, int64_t now, int64_t quantum,
                                                      int64_t next_ticket, uint64_t* __restrict__ counts) {
    __shared__ uint32_t cnt[8];
    BlockCounts bc;
    bc.init(cnt);
    const uint32_t a = blockIdx.x * kT + threadIdx.x;
    const uint32_t k = a < n_act ? mark[a] : 0u;
    if (k) {
        mark[a] = 0;
        if (k >= state[a].num_running) {  // numRunning reaches 0 (ActivationData.cs:427-435)
            c.became_idle[a] = now;
            bc.add(0);
            const uint32_t r = reschedule(c, a, now, quantum, next_ticket);
            if (r) bc.add(r);
        }
    }
    bc.flush(counts);
}

// ---- scans -------------------------------------------------------------------------------------------------------------
// What a scan does with entry a: 0 not a candidate, else the d_counts slot.
constexpr uint32_t kScBadState = 1, kScKeptAlive = 2, kScActive = 3, kScYoung = 4, kScCondemned = 5, kScCancelled = 6;

struct ScanArgs {
    int64_t now, quantum, new_next, age_limit;  // new_next: ScanStale's; age_limit: ScanAll's
};

template <bool kAll>
__device__ __forceinline__ uint32_t scan_decide(const Cols& c, const orl_act_state* __restrict__ state, uint32_t a, int64_t tk,
                                                const ScanArgs& g, uint32_t* fl_out) {
    if (tk == 0 || (!kAll && tk >= g.new_next)) return 0;
    const uint32_t fl = c.cflags[a];
    *fl_out = fl;
    if (fl & ORL_COLF_CANCELLED) return kScCancelled;  // CancelAll skips it (:476-494); ScanAll finds a nulled item
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(state + a);
    if ((sw[0] & 0xFFu) != ORL_ACT_VALID) return kScBadState;
    if (c.keep_alive_until[a] >= g.now) return kScKeptAlive;  // ShouldBeKeptAlive
    if (sw[1] > 0 || sw[3] > 0) return kScActive;             // !IsInactive
    if (g.now - c.became_idle[a] < (kAll ? g.age_limit : c.age_limit[a])) return kScYoung;
    return kScCondemned;
}

// kPlace = false: agg[tile] = the tile's condemned.  kPlace = true: carry[tile] condemned precede the tile; everything is
// written.  counts, ScanStale: [0] candidates, [1] bad state, [2] kept alive, [3] active, [4] not stale, [5] condemned,
// [6] cancelled items skipped, [7] candidates that ScheduleCollection left without a ticket; ScanAll: the same, [7] = 0.
template <bool kAll, bool kPlace>
__global__ __launch_bounds__(kT) void k_col_scan(Cols c, orl_act_state* __restrict__ state, ScanArgs g, uint32_t* __restrict__ agg,
                                                 uint32_t* __restrict__ out_act, uint64_t* __restrict__ counts) {
    __shared__ uint32_t lds[2 * kT];
    __shared__ uint32_t cnt[8];
    BlockCounts bc;
    if (kPlace) bc.init(cnt);
    const uint32_t a0 = blockIdx.x * kScanTile + threadIdx.x * kI;
    int64_t tk[kI];
    stream_i64(c.ticket + a0, tk);  // ticket[a0 .. a0 + 8)
    uint32_t what[kI], fl[kI], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        fl[k] = 0;
        what[k] = scan_decide<kAll>(c, state, a0 + k, tk[k], g, &fl[k]);
        mine += what[k] == kScCondemned;
    }
    uint32_t total;
    const uint32_t ex = block_exclusive<uint32_t, OpAdd, kT>(mine, lds, &total);
    if (!kPlace) {
        if (threadIdx.x == 0) agg[blockIdx.x] = total;
        return;
    }
    uint32_t pos = agg[blockIdx.x] + ex;
#pragma unroll
    for (uint32_t k = 0; k < kI; ++k) {
        const uint32_t w = what[k], a = a0 + k;
        if (!w) continue;
        if (w == kScCancelled) {
            bc.add(6);
            continue;
        }
        bc.add(0);
        bc.add(w);
        if (w == kScCondemned) {  // PrepareForDeactivation (ActivationData.cs:337-341)
            reinterpret_cast<uint8_t*>(state + a)[0] = (uint8_t)ORL_ACT_DEACTIVATING;
            out_act[pos++] = a;
        }
        if (kAll) {
            if (w == kScCondemned) c.cflags[a] = (uint8_t)(fl[k] | ORL_COLF_CANCELLED);  // Bucket.TryCancel; the ticket stays
        } else {
            // CancelAll set the flag, ResetCollectionTicket; ScheduleCollection (:103-128) for the three deferred kinds
            int64_t nt = 0;
            if (w == kScKeptAlive || w == kScActive || w == kScYoung) {
                const int64_t age = c.age_limit[a];
                if (!(fl[k] & ORL_COLF_EXEMPT) && age >= g.quantum) nt = make_ticket(g.now + age, g.quantum);
                if (!nt) bc.add(7);
            }
            c.ticket[a] = nt;
            if (!nt) c.cflags[a] = (uint8_t)(fl[k] | ORL_COLF_CANCELLED);  // Add clears it, and it was clear
        }
    }
    bc.flush(counts);
}

// In place: agg[i] = agg[0] + .. + agg[i - 1] (tile_scan_body); *total = the sum.
__global__ __launch_bounds__(kScanThreads) void k_col_tilescan(uint32_t* __restrict__ agg, uint32_t ntiles,
                                                               uint64_t* __restrict__ total) {
    __shared__ uint32_t lds[2 * kScanThreads];
    uint32_t sum;
    tile_scan_body<uint32_t, uint32_t, OpAdd>(agg, ntiles, lds, &sum);
    if (threadIdx.x == 0) *total = sum;
}

int zero_counts(uint64_t* d_counts, hipStream_t st) {
    if (!d_counts) return 0;
    return (int)hipMemsetAsync(d_counts, 0, 8 * sizeof(uint64_t), st);
}

template <bool kAll>
int launch_scan(const orl_collector& c, orl_act_state* d_state, const ScanArgs& g, uint64_t* d_counts, hipStream_t st) {
    const uint32_t tiles = (uint32_t)(pad_to(c.n_act, kScanTile) / kScanTile);
    const Cols cols = cols_of(c);
    hipLaunchKernelGGL((k_col_scan<kAll, false>), dim3(tiles), dim3(kT), 0, st, cols, d_state, g, c.agg, c.out_act, d_counts);
    hipLaunchKernelGGL(k_col_tilescan, dim3(1), dim3(kScanThreads), 0, st, c.agg, tiles, c.out_n);
    hipLaunchKernelGGL((k_col_scan<kAll, true>), dim3(tiles), dim3(kT), 0, st, cols, d_state, g, c.agg, c.out_act, d_counts);
    return (int)hipGetLastError();
}

}  // namespace

int collector_alloc(orl_collector** out, uint32_t n_act, uint64_t max_batch, int64_t quantum, int64_t next_ticket) {
    *out = nullptr;
    const uint64_t np = pad_to(n_act, kScanTile), tiles = np / kScanTile;
    const uint64_t b_i64 = np * 8, b_u8 = np, b_u32 = np * 4, b_agg = pad_to(tiles * 4, 256);
    const uint64_t total = 4 * b_i64 + b_u8 + 2 * b_u32 + 256 + b_agg;
    void* base = nullptr;
    hipError_t e = hipMalloc(&base, total);
    if (e != hipSuccess) return (int)e;
    e = hipMemset(base, 0, total);
    // the fill runs on the null stream and need not have finished; the first call may come on a non-blocking stream
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipFree(base);
        return (int)e;
    }
    orl_collector* c = new orl_collector();
    Carve cv(base);
    c->base = base;
    c->n_act = n_act;
    c->max_batch = max_batch;
    c->quantum = quantum;
    c->next_ticket = next_ticket;
    c->ticket = cv.take<int64_t>(b_i64);
    c->became_idle = cv.take<int64_t>(b_i64);
    c->keep_alive_until = cv.take<int64_t>(b_i64);
    c->age_limit = cv.take<int64_t>(b_i64);
    c->cflags = cv.take(b_u8);
    c->out_act = cv.take<uint32_t>(b_u32);
    c->mark = cv.take<uint32_t>(b_u32);
    c->out_n = cv.take<uint64_t>(256);
    c->agg = cv.take<uint32_t>(b_agg);
    *out = c;
    return 0;
}

void collector_free(orl_collector* c) {
    if (!c) return;
    if (c->base) (void)hipFree(c->base);
    delete c;
}

int launch_collect_schedule(const orl_collector& c, const uint32_t* d_handles, size_t m, int64_t now, uint64_t* d_counts,
                            void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int e = zero_counts(d_counts, st)) return e;
    if (m == 0) return 0;
    hipLaunchKernelGGL(k_col_schedule, dim3((uint32_t)((m + kT - 1) / kT)), dim3(kT), 0, st, cols_of(c), d_handles, m, c.n_act,
                       now, c.quantum, d_counts);
    return (int)hipGetLastError();
}

int launch_collect_cancel(const orl_collector& c, const uint32_t* d_handles, size_t m, uint64_t* d_counts, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int e = zero_counts(d_counts, st)) return e;
    if (m == 0) return 0;
    hipLaunchKernelGGL(k_col_cancel, dim3((uint32_t)((m + kT - 1) / kT)), dim3(kT), 0, st, cols_of(c), d_handles, m, c.n_act,
                       c.next_ticket, d_counts);
    return (int)hipGetLastError();
}

int launch_collect_touch(const orl_collector& c, const uint32_t* d_act, const uint8_t* d_disp, size_t n,
                         const orl_act_state* d_state, orl_admit_limits limits, int64_t now, uint64_t* d_counts,
                         void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int e = zero_counts(d_counts, st)) return e;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_col_touch_mark, dim3((uint32_t)((n + kScanTile - 1) / kScanTile)), dim3(kT), 0, st, d_act, d_disp, n,
                       c.n_act, c.mark);
    hipLaunchKernelGGL(k_col_touch_apply, dim3((c.n_act + kT - 1) / kT), dim3(kT), 0, st, cols_of(c), c.n_act, c.mark, d_state,
                       limits.hard, limits.hard_stateless, now, c.quantum, c.next_ticket, d_counts);
    return (int)hipGetLastError();
}

int launch_collect_on_complete(const orl_collector& c, const uint32_t* d_cact, const uint32_t* d_ctok, size_t m,
                               const orl_act_state* d_state, int64_t now, uint64_t* d_counts, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int e = zero_counts(d_counts, st)) return e;
    if (m == 0) return 0;
    hipLaunchKernelGGL(k_col_cmp_mark, dim3((uint32_t)((m + kScanTile - 1) / kScanTile)), dim3(kT), 0, st, d_cact, d_ctok, m,
                       c.n_act, c.mark, d_counts);
    hipLaunchKernelGGL(k_col_cmp_apply, dim3((c.n_act + kT - 1) / kT), dim3(kT), 0, st, cols_of(c), c.n_act, c.mark, d_state,
                       now, c.quantum, c.next_ticket, d_counts);
    return (int)hipGetLastError();
}

int launch_collect_scan_stale(const orl_collector& c, orl_act_state* d_state, int64_t now, int64_t old_next,
                              int64_t new_next, uint64_t* d_counts, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int e = zero_counts(d_counts, st)) return e;
    if (new_next == old_next) return (int)hipMemsetAsync(c.out_n, 0, sizeof(uint64_t), st);
    return launch_scan<false>(c, d_state, ScanArgs{now, c.quantum, new_next, 0}, d_counts, st);
}

int launch_collect_scan_all(const orl_collector& c, orl_act_state* d_state, int64_t age_limit, int64_t now,
                            uint64_t* d_counts, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int e = zero_counts(d_counts, st)) return e;
    return launch_scan<true>(c, d_state, ScanArgs{now, c.quantum, 0, age_limit}, d_counts, st);
}

}  // namespace orl
