// waitq.h — the per-activation waiting queues on the device (waitq.hip), as orl_api.cpp calls them.  Only the name
// orl_waitq is part of the public ABI (an opaque handle).
#pragma once

#include "orl_internal.h"

// One queue object: the store (double-buffered CSR), running_tok, the out list and the scratch of its calls, all carved
// from one device allocation (`base`).  Per-record arrays are padded to whole tiles.
struct orl_waitq {
    void* base = nullptr;
    uint64_t capacity = 0;   // records
    uint64_t max_batch = 0;  // the context's
    uint32_t n_act = 0;
    uint32_t cur = 0;    // the current buffer of the store; every mutating call writes the other and flips
    uint64_t bound = 0;  // host-side upper bound of the store's length (include/orleans_route.h)
    uint32_t* off[2] = {nullptr, nullptr};  // [n_act + 1]
    uint32_t* tok[2] = {nullptr, nullptr};  // [capacity]
    uint32_t* act[2] = {nullptr, nullptr};
    uint8_t* mflags[2] = {nullptr, nullptr};
    uint32_t* running_tok = nullptr;  // [n_act]
    uint32_t* out_tok = nullptr;      // [capacity] the out list of the last complete
    uint32_t* out_act = nullptr;
    uint8_t* out_mflags = nullptr;
    uint8_t* out_kind = nullptr;
    uint64_t* out_n = nullptr;      // [1]
    uint64_t* waiting_n = nullptr;  // [1] the store's true length
    // scratch
    uint32_t* key = nullptr;   // [max_batch] append: the bucket of a position
    uint8_t* cls = nullptr;    // [max(max_batch, capacity)] append: a position's class; complete: a record's
    uint32_t* pre = nullptr;   // [max(max_batch, capacity) + 1] exclusive count before a position / record, and the total
    uint32_t* mark = nullptr;  // [n_act] complete: kWqMark* of the activation's records
    uint32_t* nonc = nullptr;  // [n_act] complete: its pump and drain records (k = its bucket's length - nonc)
    orl::SegAgg* agg = nullptr;  // [tiles] per-tile aggregates, then their exclusive scan
};

namespace orl {

// hipError_t as int (0 = ok).  waitq_alloc leaves an empty store, running_tok all ORL_TOK_NONE, an empty out list.
int waitq_alloc(orl_waitq** out, uint32_t n_act, uint64_t capacity, uint64_t max_batch);
void waitq_free(orl_waitq* q);

// orl_waitq_append_device's kernels, stream-ordered; n > 0; the caller has checked old_bound + n <= capacity and flips
// q->cur afterwards.  old_bound >= the store's length before the call.
int launch_waitq_append(const orl_waitq& q, uint64_t old_bound, const uint32_t* d_tok, const uint8_t* d_mflags, size_t n,
                        const uint32_t* d_order, const uint32_t* d_boff, const uint8_t* d_disp, void* stream);

// orl_complete_device's kernels, stream-ordered; m == 0 writes an empty out list and d_counts only (no flip), else the
// caller flips q->cur afterwards.  d_counts optional (zeroed here).
int launch_waitq_complete(const orl_waitq& q, const uint32_t* d_cact, const uint32_t* d_ctok, size_t m,
                          const uint32_t* d_cboff, orl_act_state* d_state, uint64_t* d_counts, void* stream);

}  // namespace orl
