// admit.h — admission of a bucketed batch on the device (admit.hip), as orl_api.cpp calls it.  Nothing here is part of the
// public ABI.
#pragma once

#include "orl_internal.h"

namespace orl {

// Scratch of one context's admission calls, allocated once (on the first call), sized by max_batch: one device
// allocation (`base`) carved into the arrays below.  The per-position arrays are padded to whole tiles.
struct AdmitScratch {
    void* base = nullptr;
    uint64_t cap = 0;          // positions (max_batch)
    uint32_t* key = nullptr;   // [cap, padded] min(act[order[p]], n_act)
    uint8_t* cls = nullptr;    // [cap, padded] the message's class, then its provisional disposition
    SegAgg* agg1 = nullptr;    // [tiles] per-tile aggregates of the first scan, then their exclusive scan
    SegAgg* agg2 = nullptr;    // [tiles] the same of the second scan
};

// hipError_t as int (0 = ok).
int admit_alloc(AdmitScratch* s, uint64_t max_batch);
void admit_free(AdmitScratch* s);

// orl_admit_device's kernels over n messages, stream-ordered (include/orleans_route.h has the model).  d_counts optional
// (zeroed here).  The handles themselves are not an argument: a position's bucket is found in d_off.
int launch_admit(const uint8_t* d_mflags, size_t n, uint32_t n_act, const uint32_t* d_order,
                 const uint32_t* d_off, orl_act_state* d_state, orl_admit_limits lim, uint8_t* d_disp, uint64_t* d_counts,
                 const AdmitScratch& s, void* stream);

}  // namespace orl
