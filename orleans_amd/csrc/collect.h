// collect.h — the idle-activation collector on the device (collect.hip), as orl_api.cpp calls it.  Only the name
// orl_collector is part of the public ABI (an opaque handle).
#pragma once

#include "orl_internal.h"

// One collector: the five per-activation arrays, the condemned list of the last scan and the scratch of its calls, all
// carved from one device allocation (`base`), zero-filled.  Per-activation arrays are padded to whole tiles; a padding
// entry keeps ticket == 0 and so is never a candidate of a scan.
struct orl_collector {
    void* base = nullptr;
    uint32_t n_act = 0;
    uint64_t max_batch = 0;    // the context's
    int64_t quantum = 0;       // ticks, > 0
    int64_t next_ticket = 0;   // ActivationCollector.nextTicket; only grows (orl_collect_scan_stale_device)
    int64_t* ticket = nullptr;            // [n_act] CollectionTicket, 0 = none
    int64_t* became_idle = nullptr;       // [n_act]
    int64_t* keep_alive_until = nullptr;  // [n_act]
    int64_t* age_limit = nullptr;         // [n_act]
    uint8_t* cflags = nullptr;            // [n_act] ORL_COLF_*
    uint32_t* out_act = nullptr;          // [n_act] the condemned list of the last scan, ascending
    uint64_t* out_n = nullptr;            // [1] its length
    // scratch
    uint32_t* mark = nullptr;  // [n_act] touch: the two bits of an activation's bucket; on-complete: its completions.  Zero
                               // between calls (the dense pass clears what the message pass set)
    uint32_t* agg = nullptr;   // [tiles] condemned per tile, then their exclusive scan
};

namespace orl {

// hipError_t as int (0 = ok).
int collector_alloc(orl_collector** out, uint32_t n_act, uint64_t max_batch, int64_t quantum, int64_t next_ticket);
void collector_free(orl_collector* c);

// The kernels of the six calls, stream-ordered; d_counts optional (zeroed here).  m, n may be 0.
int launch_collect_schedule(const orl_collector& c, const uint32_t* d_handles, size_t m, int64_t now, uint64_t* d_counts,
                            void* stream);
int launch_collect_cancel(const orl_collector& c, const uint32_t* d_handles, size_t m, uint64_t* d_counts, void* stream);
int launch_collect_touch(const orl_collector& c, const uint32_t* d_act, const uint8_t* d_disp, size_t n,
                         const orl_act_state* d_state, orl_admit_limits limits, int64_t now, uint64_t* d_counts,
                         void* stream);
int launch_collect_on_complete(const orl_collector& c, const uint32_t* d_cact, const uint32_t* d_ctok, size_t m,
                               const orl_act_state* d_state, int64_t now, uint64_t* d_counts, void* stream);
// new_next == old_next: nothing was dequeued; the list's length (0) and d_counts are written and nothing else.
int launch_collect_scan_stale(const orl_collector& c, orl_act_state* d_state, int64_t now, int64_t old_next,
                              int64_t new_next, uint64_t* d_counts, void* stream);
int launch_collect_scan_all(const orl_collector& c, orl_act_state* d_state, int64_t age_limit, int64_t now,
                            uint64_t* d_counts, void* stream);

}  // namespace orl
