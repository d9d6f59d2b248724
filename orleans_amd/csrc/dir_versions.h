// dir_versions.h — the directory partition's per-entry version tags (GrainInfo.VersionTag) and the owner's side of the
// cache refresh, RemoteGrainDirectory.LookUpMany, on the device (dir_versions.hip), as orl_api.cpp calls them.  Nothing
// here is part of the public ABI.
#pragma once

#include "orl_internal.h"

namespace orl {

// RemoteGrainDirectory.LookUpMany (RemoteGrainDirectory.cs:349-380) over n (grain, etag) requests: one lane per request
// walks the 32-B partition read-only, reads the matching slot's tag from d_tags (one int32 per slot) and applies the
// functional mask of d_params (LookUpGrain's IsValidSilo filter, GrainDirectoryPartition.cs:326-344).  d_counts
// (optional, u64[5]) is zeroed and then receives the number of requests per ORL_LUM_* kind.  Stream-ordered; launched in
// chunks when n exceeds one grid.  hipError_t as int (0 = ok).
int launch_lookup_many(const RouteParams* d_params, const DirSlot* d_dir, uint64_t mask, const int32_t* d_tags,
                       const orl_grain_key* d_keys, const int32_t* d_etags, size_t n, uint8_t* d_kind, int32_t* d_etag_out,
                       uint32_t* d_act, uint8_t* d_silo, uint64_t* d_counts, void* stream);

// Host-changed slots of a versioned partition (beside launch_dir_patch): d_tags[idx[k]] = tags[k].
int launch_tag_patch(const uint32_t* d_idx, const int32_t* d_new, uint32_t n, int32_t* d_tags, void* stream);

}  // namespace orl
