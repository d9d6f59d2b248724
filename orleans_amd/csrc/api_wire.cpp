// api_wire.cpp — the wire codec's host side (f2): the wire types, the serialized silo addresses, the grain class names,
// and the decode and stamp entries (wire_codec.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "orl_ctx.h"

extern "C" {

int orl_wire_types_set(orl_ctx* c, uint32_t n, const uint64_t* tcd) {
    if (!c) return ORL_E_INVALID;
    if (n > ORL_MAX_WIRE_TYPES || (n && !tcd)) return fail(c, ORL_E_INVALID, "wire types: n = %u (at most %u)", n, ORL_MAX_WIRE_TYPES);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < i; ++j)
            if (tcd[i] == tcd[j]) return fail(c, ORL_E_INVALID, "wire types: entry %u repeats entry %u", i, j);
    RouteParams& P = c->hp;
    std::memset(P.wire_tcd, 0, sizeof P.wire_tcd);
    if (n) std::memcpy(P.wire_tcd, tcd, n * sizeof(uint64_t));
    P.n_wire_types = n;
    uint64_t h = 0xCBF29CE484222325ull;  // FNV-1a over the count and the values, little-endian bytes
    auto mix = [&](uint64_t v) {
        for (int b = 0; b < 8; ++b) { h ^= (v >> (8 * b)) & 0xFFu; h *= 0x100000001B3ull; }
    };
    mix(n);
    for (uint32_t i = 0; i < n; ++i) mix(tcd[i]);
    P.wire_digest = n ? h : 0;
    c->params_dirty = true;
    return ORL_OK;
}

int orl_silo_address_set(orl_ctx* c, uint32_t silo, const uint8_t* ip16, int32_t port, int32_t generation) {
    if (!c) return ORL_E_INVALID;
    if (silo >= 255) return fail(c, ORL_E_INVALID, "silo index %u out of range (< 255)", silo);
    if (!ip16) {
        c->silo_addr_known[silo] = 0;
        c->silo_addr_dirty = true;
        return ORL_OK;
    }
    if (port < 0 || port > 65535) return fail(c, ORL_E_INVALID, "port %d out of range", port);
    uint32_t w[6];
    std::memcpy(w, ip16, 16);
    w[4] = (uint32_t)port;
    w[5] = (uint32_t)generation;
    for (uint32_t s = 0; s < 255; ++s)
        if (s != silo && c->silo_addr_known[s] && std::memcmp(c->silo_addr[s], w, sizeof w) == 0)
            return fail(c, ORL_E_INVALID, "address already belongs to silo %u", s);
    std::memcpy(c->silo_addr[silo], w, sizeof w);
    c->silo_addr_known[silo] = 1;
    c->silo_addr_dirty = true;
    return ORL_OK;
}

int orl_decode_frames_device(orl_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_frame_offsets, size_t n,
                             uint32_t sender_override, orl_msg_hdr* d_out, uint8_t* d_status, uint32_t* d_n_bad, void* stream) {
    if (!c) return ORL_E_INVALID;
    if (n && (!d_bytes || !d_frame_offsets || !d_out || !d_status)) return fail(c, ORL_E_INVALID, "null device buffer");
    if ((uintptr_t)d_bytes & 3u) return fail(c, ORL_E_INVALID, "frame buffer must be 4-byte aligned");
    if (sender_override > ORL_SENDER_FROM_HEADER) return fail(c, ORL_E_INVALID, "sender_override must be < 255 or 0xFF");
    if (n > 0xFFFFFFFFull) return fail(c, ORL_E_CAPACITY, "batch too large");
    if (int r = sync_device_state(c)) return r;
    int e = launch_decode_frames(d_bytes, nbytes, d_frame_offsets, n, sender_override, c->d_silo_tab, d_out, d_status,
                                 d_n_bad, c->d_decode_flag, stream_of(c, stream));
    if (e) return hipfail(c, (hipError_t)e, "decode frames launch");
    return ORL_OK;
}

int orl_grain_type_set(orl_ctx* c, int32_t type_code, const char* utf8, size_t len) {
    if (!c) return ORL_E_INVALID;
    if (len == 0 || !utf8) {
        c->grain_types.erase(type_code);
        c->gt_dirty = true;
        return ORL_OK;
    }
    size_t total = len;
    for (const auto& kv : c->grain_types)
        if (kv.first != type_code) total += kv.second.size();
    if (total > kGrainTypeBlob) return fail(c, ORL_E_CAPACITY, "grain type names exceed %u bytes", kGrainTypeBlob);
    if (c->grain_types.size() >= kGrainTypeSlots / 2 && !c->grain_types.count(type_code))
        return fail(c, ORL_E_CAPACITY, "more than %u grain types", kGrainTypeSlots / 2);
    c->grain_types[type_code] = std::string(utf8, len);
    c->gt_dirty = true;
    return ORL_OK;
}

int orl_stamp_frames_device(orl_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_frame_offsets, size_t n,
                            const uint32_t* d_route, const uint32_t* d_act, const orl_grain_key* d_act_keys, uint32_t n_act_keys,
                            const orl_grain_key* d_new_act_keys, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_offsets,
                            uint64_t* d_out_total, uint8_t* d_status, void* stream) {
    if (!c) return ORL_E_INVALID;
    if (!d_out_total) return fail(c, ORL_E_INVALID, "null total pointer");
    if (n && (!d_bytes || !d_frame_offsets || !d_route || !d_act || !d_out || !d_out_offsets || !d_status))
        return fail(c, ORL_E_INVALID, "null device buffer");
    if (n_act_keys && !d_act_keys) return fail(c, ORL_E_INVALID, "null activation key table");
    if (((uintptr_t)d_bytes & 3u) || ((uintptr_t)d_out & 3u)) return fail(c, ORL_E_INVALID, "frame buffers must be 4-byte aligned");
    if (n > 0xFFFFFFFFull) return fail(c, ORL_E_CAPACITY, "batch too large");
    if (int r = sync_device_state(c)) return r;
    if (n > c->stamp_cap) {  // scratch grows to the largest batch seen (a synchronising allocation, once)
        if (c->d_stamp_sizes) (void)hipFree(c->d_stamp_sizes);
        if (c->d_stamp_temp) (void)hipFree(c->d_stamp_temp);
        c->d_stamp_sizes = nullptr;
        c->d_stamp_temp = nullptr;
        c->stamp_cap = 0;
        const size_t tb = stamp_scan_temp_bytes(n);
        ORL_HIP(c, hipMalloc((void**)&c->d_stamp_sizes, (n + 1) * sizeof(uint64_t)));  // + the deferral flag
        ORL_HIP(c, hipMalloc(&c->d_stamp_temp, std::max<size_t>(tb, 16)));
        c->stamp_cap = n;
        c->stamp_temp_bytes = std::max<size_t>(tb, 16);
    }
    int e = launch_stamp_frames(d_bytes, nbytes, d_frame_offsets, n, d_route, d_act, d_act_keys, n_act_keys, d_new_act_keys,
                                c->d_gt, c->d_gt_blob, c->d_silo_words, c->d_stamp_sizes, c->d_stamp_temp, c->stamp_temp_bytes,
                                d_out, out_cap, d_out_offsets, d_out_total, d_status, stream_of(c, stream));
    if (e) return hipfail(c, (hipError_t)e, "stamp frames launch");
    return ORL_OK;
}

}  // extern "C"
