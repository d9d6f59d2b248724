// orl_ctx.h — the context of liborleans_route.so and the host helpers that more than one host unit calls.  Included by
// orl_api.cpp and the api_*.cpp files only: no .hip file includes it, and orl_node.cpp reaches the context through
// orl_internal.h's orl::ctx_* accessors.  Nothing here is part of the public ABI.  DESIGN §20 has the cut of the host units.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "orl_internal.h"
#include "admit.h"
#include "cache_adaptive.h"
#include "cache_evict.h"

namespace orl {
namespace host {

// orl_route_batch: chunks per host-array batch (and the smallest chunk)
constexpr size_t kHostChunks = 8;
constexpr size_t kHostChunk = 1u << 20;

}  // namespace host
}  // namespace orl

// The host units name orl_internal.h's layouts and the helpers below without a prefix, and so does the struct.
using namespace orl;
using namespace orl::host;

// ---------------------------------------------------------------------------------------------------
struct orl_ctx {
    orl_config cfg{};
    bool device_mode = false;
    std::string err;
    // silos (LocalGrainDirectory membership view)
    uint32_t n_silos = 0;
    std::vector<uint8_t> running, functional, local;
    uint32_t seed = ORL_NULL_SILO;
    std::vector<std::pair<int32_t, uint8_t>> ring;  // membershipRingList (signed hash, silo)
    // directory partition mirror
    std::vector<DirSlot> table;
    uint64_t mask = 0, count = 0, tombs = 0;
    bool dir_dirty = true;           // the whole table must be uploaded (and the probe tables rebuilt)
    std::vector<uint32_t> dirty_slots;  // else: host-changed slots since the last upload, patched in place
    std::vector<uint8_t> slot_marked;   // dirty_slots membership (one byte per slot, allocated on first use)
    void* d_patch_data = nullptr;       // device staging of a slot patch (grows to the largest patch)
    size_t patch_cap = 0;
    uint64_t n_full_uploads = 0, n_patches = 0;
    // follower graph of orl_csr_set (host-array fan-out)
    uint64_t* d_csr_off = nullptr;
    uint32_t* d_csr_tgt = nullptr;
    size_t csr_nodes = 0;
    std::vector<uint64_t> h_csr_off;
    bool mirror_stale = false;       // device mutations since the mirror was last downloaded
    uint64_t count_ub = 0, tombs_ub = 0;  // upper bounds while the mirror is stale (capacity checks without a sync)
    // version tags (orl_dir_versions_enable; GrainInfo.VersionTag): one int32 per slot beside the mirror and beside the
    // device table; they follow the slots through the upload, the slot patches, the mirror download and the compaction
    bool versions = false;
    std::vector<int32_t> vtag;
    int32_t* d_vtag = nullptr;
    // device state
    DirSlot* d_table = nullptr;
    ProbeSlot* d_probe = nullptr;    // compact probe table of d_table (ProbeSlot, orl_internal.h)
    bool probe_valid = false;        // d_probe mirrors d_table (set by the host upload, cleared by device mutations)
    bool probe_off = false;          // ORL_NO_PROBE16=1: always probe the 32-B table (A/B measurements)
    bool probe_dev = false;          // d_probe was built on the device: validity in *d_probe_bad
    uint2* d_probe8 = nullptr;       // 8-B form of the probe table (one type, 32-bit N1, 24-bit handles)
    bool probe8_valid = false;       // d_probe8 mirrors d_table (host upload only)
    bool probe8_off = false;         // ORL_NO_PROBE8=1: never the 8-B form (A/B measurements)
    bool probe_dev_stale = false;    // device mutations since: rebuild before the next route launch
    uint32_t* d_probe_bad = nullptr;
    uint32_t* d_claim = nullptr;     // per-slot claim word of the device insert/remove kernels (0xFFFFFFFF at rest)
    uint64_t* d_dirstate = nullptr;  // {entries, tombstones, error flag}
    uint32_t* d_dslot = nullptr;     // per-message slot of a device directory batch
    uint8_t* d_dflag = nullptr;      // per-message flag of a device cache batch
    // KeyExt grains (round 5): host table + extension blob, uploaded whole when changed.  Round 6: registrations on the
    // device (orl_dir_insert_keyext_device) make the device table the newer one (ext_dev_newer): the host functions first
    // download it (ext_sync_host).  ext_dirty (host newer) and ext_dev_newer never hold together.
    std::vector<ExtSlot> ext_table;
    std::vector<uint8_t> ext_blob;
    uint64_t ext_count = 0, ext_tombs = 0;
    bool ext_dirty = false;
    bool ext_dev_newer = false;
    uint64_t ext_count_ub = 0, ext_tombs_ub = 0, ext_blob_ub = 0;  // upper bounds while the device is newer
    uint64_t ext_blob_min_cap = 0;   // the device string store's capacity at the next upload (room for a device batch)
    ExtSlot* d_ext_table = nullptr;
    uint8_t* d_ext_blob = nullptr;
    size_t d_ext_table_cap = 0, d_ext_blob_cap = 0;
    uint32_t* d_ext_claim = nullptr;  // per-slot claim words of the device registration (0xFFFFFFFF at rest)
    size_t d_ext_claim_cap = 0;
    uint64_t* d_ext_state = nullptr;  // {string bytes used, entries, tombstones, error}
    // directory cache (AdaptiveGrainDirectoryCache, f4): device table of remote-owned grains
    DirSlot* d_cache = nullptr;
    uint32_t* d_cclaim = nullptr;
    uint64_t* d_cstate = nullptr;    // {entries, tombstones, error word, cumulative device evictions}
    DirSlot* d_cache2 = nullptr;     // the second table a tombstone compaction rebuilds into (then the two swap)
    CacheEvictScratch cev;           // scratch of the device eviction (cache_evict.hip), sized by orl_cache_config
    uint32_t cache_mode = ORL_CACHE_EVICT_DEVICE;
    uint64_t cache_host_evictions = 0, cache_evict_batches = 0, cache_rebuilds = 0, cache_host_fallbacks = 0;
    uint64_t cache_slots = 0, cache_ub = 0, cache_tombs_ub = 0;
    uint64_t cache_cap = 0;       // LRU.MaximumSize (orl_cache_config's capacity)
    uint64_t cache_gen_free = 0;  // LRU.generationToFree: the generation of the last entry evicted
    // adaptive mode (orl_cache_config_adaptive): both tables carry the per-slot state (orl_internal.h CacheAdaptive)
    bool cache_adaptive = false;
    int64_t cache_initial_ttl = 0, cache_max_ttl = 0;  // initialExpirationTimer, maxExpirationTimer (.NET ticks)
    double cache_growth = 0;                           // exponentialTimerGrowth
    int64_t cache_now = 0;                             // the last now_ticks a call gave (the plain add's DateTime.UtcNow)
    AdmitScratch adm;                                  // orl_admit_device's scratch (admit.hip), allocated by its first call
    CacheSweepScratch csw;                             // the maintainer's scratch and output (cache_adaptive.hip)
    // stateless-worker grains (StatelessWorkerDirector.cs:35-80): the listed types with their MaxLocal, and the local
    // catalog's host mirror (SwSlot), uploaded whole when the host changed it (sw_dirty).  orl_sw_set_busy_device makes
    // the device table the newer one (sw_dev_newer): the host calls first read it back (sw_sync_host).  The two flags
    // never hold together.
    uint32_t sw_n = 0;
    uint64_t sw_tcd[ORL_MAX_SW_TYPES] = {};
    uint8_t sw_max[ORL_MAX_SW_TYPES] = {};
    std::vector<SwSlot> sw_table;
    uint64_t sw_mask = 0, sw_count = 0, sw_tombs = 0;
    bool sw_dirty = false;
    bool sw_dev_newer = false;
    hipStream_t sw_dev_stream = nullptr;  // the stream of the last orl_sw_set_busy_device
    SwSlot* d_sw = nullptr;
    size_t d_sw_slots = 0;
    RouteParams hp{};
    RouteParams* d_params = nullptr;
    bool params_dirty = true;
    uint8_t* d_rank_of_silo = nullptr;
    uint8_t h_rank_of_silo[256] = {};  // last uploaded rank_of_silo (uploads only on change: no per-batch sync)
    bool ros_valid = false;
    Scratch s{};
    hipStream_t stream = nullptr;
    // host-buffer staging (orl_route_batch / orl_hash_batch) and its copy streams / per-chunk events
    uint8_t* st_in = nullptr; size_t st_in_cap = 0;
    hipStream_t hstream[2] = {nullptr, nullptr};
    hipEvent_t hev[2 * (kHostChunks + 1)] = {};
    uint32_t* st_out = nullptr; size_t st_out_cap = 0;
    uint32_t* st_off = nullptr;
    // silo consistent hashes (SiloAddress.GetConsistentHashCode) for outbound sender queues
    int32_t silo_hash[256] = {};
    uint8_t silo_known[256] = {};
    bool silo_hash_dirty = true;
    int32_t* d_silo_hash = nullptr;
    uint8_t* d_silo_known = nullptr;
    // stream / reminder virtual-bucket ring (VirtualBucketsRingProvider.bucketsMap)
    uint32_t vr_nb = 30;
    std::map<uint32_t, uint8_t> vr_map;                // bucket hash → silo
    std::map<uint8_t, std::vector<uint32_t>> vr_hashes;  // silo → its GetUniformHashCodes
    std::map<uint8_t, int32_t> vr_gen;
    bool vr_dirty = false;
    uint32_t vr_n_dev = 0;
    uint32_t* d_vr_hash = nullptr;
    uint8_t* d_vr_silo = nullptr;
    // f2: serialized SiloAddress -> silo index for the wire decoder
    uint32_t silo_addr[256][6] = {};
    uint8_t silo_addr_known[256] = {};
    bool silo_addr_dirty = true;
    SiloAddrEntry* d_silo_tab = nullptr;
    uint32_t* d_decode_flag = nullptr;
    uint32_t* d_silo_words = nullptr;  // [256][6] serialized SiloAddress by silo index (stamp)
    // f2 emit: grain class names by type code, and the stamp's scratch
    std::map<int32_t, std::string> grain_types;
    bool gt_dirty = true;
    GrainTypeEntry* d_gt = nullptr;
    uint8_t* d_gt_blob = nullptr;
    uint64_t* d_stamp_sizes = nullptr;
    void* d_stamp_temp = nullptr;
    size_t stamp_cap = 0, stamp_temp_bytes = 0;
    // timing: 4 events per recorded batch (call begin, route begin, route end, call end)
    bool timing = false;
    std::vector<hipEvent_t> tev;
    uint32_t tcount = 0;
};

namespace orl {
namespace host {

// orl_api.cpp: the error string of a refusal, and the upload of every host-side change before a launch
int fail(orl_ctx* c, int code, const char* fmt, ...);
int hipfail(orl_ctx* c, hipError_t e, const char* what);
int sync_device_state(orl_ctx* c);

#define ORL_HIP(c, call)                                           \
    do {                                                           \
        hipError_t _e = (call);                                    \
        if (_e != hipSuccess) return hipfail((c), _e, #call);      \
    } while (0)

inline uint64_t next_pow2(uint64_t v) {
    uint64_t p = 16;
    while (p < v) p <<= 1;
    return p;
}

// The refusals most device entries share, typed once: ORL_OK, or the error code with the message set.
inline int need_device(orl_ctx* c) {
    return c->device_mode ? ORL_OK : fail(c, ORL_E_STATE, "context was created without a device (device < 0)");
}
inline int check_batch(orl_ctx* c, size_t n) {
    return n <= c->s.max_batch ? ORL_OK : fail(c, ORL_E_CAPACITY, "batch %zu > max_batch %llu", n, (unsigned long long)c->s.max_batch);
}
// The caller's stream, or the context's when the caller gave none.
inline hipStream_t stream_of(const orl_ctx* c, void* stream) { return stream ? (hipStream_t)stream : c->stream; }

}  // namespace host
}  // namespace orl
