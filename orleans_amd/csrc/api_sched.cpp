// api_sched.cpp — the scheduler's device calls: admission (admit.hip), the waiting queues (waitq.hip) and the
// idle-activation collector (collect.hip).
#include <hip/hip_runtime.h>

#include "orl_ctx.h"
#include "admit.h"
#include "waitq.h"
#include "collect.h"

namespace {

// The checks every collector call shares; `count` is its m or n.
int collect_check(orl_ctx* c, orl_collector* col, size_t count, bool null_buffer, int64_t now) {
    if (!c) return ORL_E_INVALID;
    if (int r = need_device(c)) return r;
    if (!col) return fail(c, ORL_E_INVALID, "null collector");
    if (now <= 0) return fail(c, ORL_E_INVALID, "collector: now must be positive");
    if (count && null_buffer) return fail(c, ORL_E_INVALID, "null device buffer");
    return check_batch(c, count);
}

}  // namespace

extern "C" {

int orl_admit_device(orl_ctx* c, const uint32_t* d_act, const uint8_t* d_mflags, size_t n, const uint32_t* d_order,
                     const uint32_t* d_off, orl_act_state* d_state, const orl_admit_limits* limits, uint8_t* d_disp,
                     uint64_t* d_counts, void* stream) {
    if (!c) return ORL_E_INVALID;
    if (int r = need_device(c)) return r;
    if (!limits) return fail(c, ORL_E_INVALID, "null limits");
    if (n && (!d_act || !d_mflags || !d_order || !d_off || !d_state || !d_disp)) return fail(c, ORL_E_INVALID, "null device buffer");
    if (int r = check_batch(c, n)) return r;
    if (!c->adm.base) {  // a synchronising allocation, once
        ORL_HIP(c, hipSetDevice(c->cfg.device));
        if (int e = admit_alloc(&c->adm, c->s.max_batch)) return hipfail(c, (hipError_t)e, "admission scratch");
    }
    int e = launch_admit(d_mflags, n, c->cfg.n_act, d_order, d_off, d_state, *limits, d_disp, d_counts, c->adm,
                         stream_of(c, stream));
    if (e) return hipfail(c, (hipError_t)e, "admission launch");
    return ORL_OK;
}

// ---- waiting queues (waitq.hip) ---------------------------------------------------------------------------
int orl_waitq_create(orl_ctx* c, uint64_t capacity, orl_waitq** out) {
    if (!c || !out) return ORL_E_INVALID;
    *out = nullptr;
    if (int r = need_device(c)) return r;
    if (capacity == 0 || capacity >= 0xFFFFFFFFull) return fail(c, ORL_E_INVALID, "waiting queue capacity must be in 1 .. 2^32 - 2");
    ORL_HIP(c, hipSetDevice(c->cfg.device));
    if (int e = waitq_alloc(out, c->cfg.n_act, capacity, c->s.max_batch))
        return fail(c, ORL_E_NOMEM, "waiting queue of %llu records: %s", (unsigned long long)capacity,
                    hipGetErrorString((hipError_t)e));
    return ORL_OK;
}

int orl_waitq_destroy(orl_ctx* c, orl_waitq* q) {
    if (!c) return ORL_E_INVALID;
    if (!q) return ORL_OK;
    ORL_HIP(c, hipSetDevice(c->cfg.device));
    waitq_free(q);
    return ORL_OK;
}

int orl_waitq_view_get(orl_ctx* c, orl_waitq* q, orl_waitq_view* out) {
    if (!c || !q || !out) return ORL_E_INVALID;
    const uint32_t b = q->cur;
    *out = orl_waitq_view{q->off[b], q->tok[b], q->act[b], q->mflags[b], q->running_tok, q->out_tok,
                          q->out_act, q->out_mflags, q->out_kind, q->out_n, q->waiting_n};
    return ORL_OK;
}

int orl_waitq_append_device(orl_ctx* c, orl_waitq* q, const uint32_t* d_tok, const uint8_t* d_mflags, size_t n,
                            const uint32_t* d_order, const uint32_t* d_off, const uint8_t* d_disp, void* stream) {
    if (!c) return ORL_E_INVALID;
    if (int r = need_device(c)) return r;
    if (!q) return fail(c, ORL_E_INVALID, "null waiting queue");
    if (n && (!d_tok || !d_mflags || !d_order || !d_off || !d_disp)) return fail(c, ORL_E_INVALID, "null device buffer");
    if (int r = check_batch(c, n)) return r;
    if (n == 0) return ORL_OK;
    hipStream_t st = stream_of(c, stream);
    if (q->bound + n > q->capacity) {  // the bound may overstate: ask the device for the true length, on this path only
        uint64_t len = 0;
        ORL_HIP(c, hipMemcpyAsync(&len, q->waiting_n, sizeof(len), hipMemcpyDeviceToHost, st));
        ORL_HIP(c, hipStreamSynchronize(st));
        q->bound = len;
        if (q->bound + n > q->capacity)
            return fail(c, ORL_E_CAPACITY, "waiting queue: %llu records + a batch of %zu > capacity %llu",
                        (unsigned long long)len, n, (unsigned long long)q->capacity);
    }
    int e = launch_waitq_append(*q, q->bound, d_tok, d_mflags, n, d_order, d_off, d_disp, st);
    if (e) return hipfail(c, (hipError_t)e, "waiting queue append launch");
    q->bound += n;
    q->cur ^= 1u;
    return ORL_OK;
}

int orl_complete_device(orl_ctx* c, orl_waitq* q, const uint32_t* d_cact, const uint32_t* d_ctok, size_t m,
                        const uint32_t* d_corder, const uint32_t* d_coff, orl_act_state* d_state, uint64_t* d_counts,
                        void* stream) {
    if (!c) return ORL_E_INVALID;
    if (int r = need_device(c)) return r;
    if (!q) return fail(c, ORL_E_INVALID, "null waiting queue");
    if (m && (!d_cact || !d_ctok || !d_corder || !d_coff || !d_state)) return fail(c, ORL_E_INVALID, "null device buffer");
    if (int r = check_batch(c, m)) return r;
    int e = launch_waitq_complete(*q, d_cact, d_ctok, m, d_coff, d_state, d_counts, stream_of(c, stream));
    if (e) return hipfail(c, (hipError_t)e, "completion launch");
    if (m) q->cur ^= 1u;
    return ORL_OK;
}

// ---- the idle-activation collector (collect.hip) -------------------------------------------------------------
int orl_collector_create(orl_ctx* c, int64_t quantum, int64_t now0, orl_collector** out) {
    if (!c || !out) return ORL_E_INVALID;
    *out = nullptr;
    if (int r = need_device(c)) return r;
    if (quantum <= 0 || now0 <= 0) return fail(c, ORL_E_INVALID, "collector: quantum and now0 must be positive");
    if (c->cfg.n_act > 0x80000000u) return fail(c, ORL_E_INVALID, "collector: n_act above 2^31");
    ORL_HIP(c, hipSetDevice(c->cfg.device));
    const int64_t next = ((now0 - 1) / quantum + 1) * quantum;  // MakeTicketFromDateTime (ActivationCollector.cs:391-400)
    if (int e = collector_alloc(out, c->cfg.n_act, c->s.max_batch, quantum, next))
        return fail(c, ORL_E_NOMEM, "collector of %u activations: %s", c->cfg.n_act, hipGetErrorString((hipError_t)e));
    return ORL_OK;
}

int orl_collector_destroy(orl_ctx* c, orl_collector* col) {
    if (!c) return ORL_E_INVALID;
    if (!col) return ORL_OK;
    ORL_HIP(c, hipSetDevice(c->cfg.device));
    collector_free(col);
    return ORL_OK;
}

int orl_collector_view_get(orl_ctx* c, orl_collector* col, orl_collector_view* out) {
    if (!c || !col || !out) return ORL_E_INVALID;
    *out = orl_collector_view{col->ticket, col->became_idle, col->keep_alive_until, col->age_limit, col->cflags,
                              col->out_act, col->out_n, col->quantum, col->next_ticket};
    return ORL_OK;
}

int orl_collect_schedule_device(orl_ctx* c, orl_collector* col, const uint32_t* d_handles, size_t m, int64_t now,
                                uint64_t* d_counts, void* stream) {
    if (int rc = collect_check(c, col, m, !d_handles, now)) return rc;
    int e = launch_collect_schedule(*col, d_handles, m, now, d_counts, stream_of(c, stream));
    if (e) return hipfail(c, (hipError_t)e, "collector schedule launch");
    return ORL_OK;
}

int orl_collect_cancel_device(orl_ctx* c, orl_collector* col, const uint32_t* d_handles, size_t m, uint64_t* d_counts,
                              void* stream) {
    if (int rc = collect_check(c, col, m, !d_handles, 1)) return rc;
    int e = launch_collect_cancel(*col, d_handles, m, d_counts, stream_of(c, stream));
    if (e) return hipfail(c, (hipError_t)e, "collector cancel launch");
    return ORL_OK;
}

int orl_collect_touch_device(orl_ctx* c, orl_collector* col, const uint32_t* d_act, const uint8_t* d_disp, size_t n,
                             const orl_act_state* d_state, const orl_admit_limits* limits, int64_t now, uint64_t* d_counts,
                             void* stream) {
    if (int rc = collect_check(c, col, n, !d_act || !d_disp || !d_state, now)) return rc;
    if (!limits) return fail(c, ORL_E_INVALID, "null limits");
    int e = launch_collect_touch(*col, d_act, d_disp, n, d_state, *limits, now, d_counts, stream_of(c, stream));
    if (e) return hipfail(c, (hipError_t)e, "collector touch launch");
    return ORL_OK;
}

int orl_collect_on_complete_device(orl_ctx* c, orl_collector* col, const uint32_t* d_cact, const uint32_t* d_ctok, size_t m,
                                   const orl_act_state* d_state, int64_t now, uint64_t* d_counts, void* stream) {
    if (int rc = collect_check(c, col, m, !d_cact || !d_ctok || !d_state, now)) return rc;
    int e = launch_collect_on_complete(*col, d_cact, d_ctok, m, d_state, now, d_counts, stream_of(c, stream));
    if (e) return hipfail(c, (hipError_t)e, "collector on-complete launch");
    return ORL_OK;
}

int orl_collect_scan_stale_device(orl_ctx* c, orl_collector* col, orl_act_state* d_state, int64_t now, uint64_t* d_counts,
                                  void* stream) {
    if (int rc = collect_check(c, col, 1, !d_state, now)) return rc;
    const int64_t old_next = col->next_ticket;
    int64_t next = old_next;  // DequeueQuantum while nextTicket <= now (ActivationCollector.cs:186-210)
    if (next <= now) next += ((now - next) / col->quantum + 1) * col->quantum;
    int e = launch_collect_scan_stale(*col, d_state, now, old_next, next, d_counts, stream_of(c, stream));
    if (e) return hipfail(c, (hipError_t)e, "collector ScanStale launch");
    col->next_ticket = next;
    return ORL_OK;
}

int orl_collect_scan_all_device(orl_ctx* c, orl_collector* col, orl_act_state* d_state, int64_t age_limit, int64_t now,
                                uint64_t* d_counts, void* stream) {
    if (int rc = collect_check(c, col, 1, !d_state, now)) return rc;
    int e = launch_collect_scan_all(*col, d_state, age_limit, now, d_counts, stream_of(c, stream));
    if (e) return hipfail(c, (hipError_t)e, "collector ScanAll launch");
    return ORL_OK;
}

}  // extern "C"
