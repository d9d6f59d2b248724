// api_sw.cpp — stateless-worker grains: the listed types and the local catalog's host mirror, everything orl_sw_*.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "orl_ctx.h"

namespace {

// The mirror after orl_sw_set_busy_device: wait for that stream, then read the table back (only busy bits can differ).
int sw_sync_host(orl_ctx* c) {
    if (!c->sw_dev_newer) return ORL_OK;
    ORL_HIP(c, hipSetDevice(c->cfg.device));
    ORL_HIP(c, hipStreamSynchronize(c->sw_dev_stream));
    if (c->d_sw && c->d_sw_slots == c->sw_table.size())
        ORL_HIP(c, hipMemcpy(c->sw_table.data(), c->d_sw, c->sw_table.size() * sizeof(SwSlot), hipMemcpyDeviceToHost));
    c->sw_dev_newer = false;
    return ORL_OK;
}

void sw_clear(orl_ctx* c, uint64_t slots) {
    c->sw_table.assign(slots, SwSlot{});
    c->sw_mask = slots ? slots - 1 : 0;
    c->sw_count = c->sw_tombs = 0;
    c->sw_dirty = true;
    c->sw_dev_newer = false;
}

int sw_type_index(const orl_ctx* c, uint64_t tcd) {
    for (uint32_t i = 0; i < c->sw_n; ++i)
        if (c->sw_tcd[i] == tcd) return (int)i;
    return -1;
}

// Slot of (key, silo) in the mirror, or -1; *free_slot = the first reusable slot (tombstone or chain end) of the chain.
int64_t sw_find(const orl_ctx* c, const orl_grain_key& k, uint32_t silo, int64_t* free_slot) {
    int64_t fr = -1;
    if (!c->sw_table.empty()) {
        uint64_t i = sw_start(jenkins3(k.type_code_data, k.n0, k.n1), silo, c->sw_mask);
        for (uint64_t step = 0; step <= c->sw_mask; ++step) {
            const SwSlot& s = c->sw_table[i];
            if (s.state == SLOT_EMPTY) { if (fr < 0) fr = (int64_t)i; break; }
            if (s.state == SLOT_TOMB) { if (fr < 0) fr = (int64_t)i; }
            else if (s.silo == silo && s.tcd == k.type_code_data && s.n0 == k.n0 && s.n1 == k.n1) {
                if (free_slot) *free_slot = fr;
                return (int64_t)i;
            }
            i = (i + 1) & c->sw_mask;
        }
    }
    if (free_slot) *free_slot = fr;
    return -1;
}

int sw_pos(const SwSlot& s, uint32_t act) {
    for (uint32_t p = 0; p < s.count; ++p)
        if (s.act[p] == act) return (int)p;
    return -1;
}

// Rebuild the mirror without tombstones (same slot count).
void sw_rehash(orl_ctx* c) {
    std::vector<SwSlot> old;
    old.swap(c->sw_table);
    c->sw_table.assign(old.size(), SwSlot{});
    c->sw_tombs = 0;
    for (const SwSlot& s : old) {
        if (s.state != SLOT_FULL) continue;
        uint64_t i = sw_start(jenkins3(s.tcd, s.n0, s.n1), s.silo, c->sw_mask);
        while (c->sw_table[i].state != SLOT_EMPTY) i = (i + 1) & c->sw_mask;
        c->sw_table[i] = s;
    }
    c->sw_dirty = true;
}

bool sw_item_ok(const orl_ctx* c, const orl_grain_key& k, uint32_t act, uint32_t silo) {
    return sw_type_index(c, k.type_code_data) >= 0 && act < c->cfg.n_act && silo < c->n_silos;
}

}  // namespace

extern "C" {

int orl_sw_types_set(orl_ctx* c, const uint64_t* tcd, const uint8_t* max_local, uint32_t n) {
    if (!c) return ORL_E_INVALID;
    if (n > ORL_MAX_SW_TYPES) return fail(c, ORL_E_INVALID, "stateless-worker types: n = %u (at most %u)", n, ORL_MAX_SW_TYPES);
    if (n && (!tcd || !max_local)) return fail(c, ORL_E_INVALID, "null type or MaxLocal array");
    for (uint32_t i = 0; i < n; ++i) {
        if ((uint32_t)(tcd[i] >> 56) != ORL_CAT_GRAIN)  // GrainTypeData describes grain classes (GrainTypeData.cs:43-50)
            return fail(c, ORL_E_INVALID, "stateless-worker type %u: category %u is not ORL_CAT_GRAIN", i, (uint32_t)(tcd[i] >> 56));
        if (max_local[i] < 1 || max_local[i] > ORL_SW_MAX_LOCAL)
            return fail(c, ORL_E_INVALID, "stateless-worker type %u: MaxLocal %u outside 1..%u", i, max_local[i], ORL_SW_MAX_LOCAL);
        for (uint32_t j = 0; j < i; ++j)
            if (tcd[i] == tcd[j]) return fail(c, ORL_E_INVALID, "stateless-worker types: entry %u repeats entry %u", i, j);
    }
    c->sw_n = n;
    std::memset(c->sw_tcd, 0, sizeof c->sw_tcd);
    std::memset(c->sw_max, 0, sizeof c->sw_max);
    for (uint32_t i = 0; i < n; ++i) {
        c->sw_tcd[i] = tcd[i];
        c->sw_max[i] = max_local[i];
    }
    // the lists were kept under the old types' MaxLocal: start over (a first set sizes the catalog for 1024 entries)
    sw_clear(c, n && c->sw_table.empty() ? next_pow2(2 * 1024) : c->sw_table.size());
    return ORL_OK;
}

int orl_sw_config(orl_ctx* c, uint64_t capacity) {
    if (!c) return ORL_E_INVALID;
    if (capacity > (1ull << 30)) return fail(c, ORL_E_INVALID, "catalog capacity %llu too large", (unsigned long long)capacity);
    sw_clear(c, next_pow2(2 * std::max<uint64_t>(capacity, 1)));
    return ORL_OK;
}

int orl_sw_add(orl_ctx* c, const orl_grain_key* keys, const uint32_t* acts, const uint8_t* silos, size_t n, uint8_t* status) {
    if (!c) return ORL_E_INVALID;
    if (n && (!keys || !acts || !silos || !status)) return fail(c, ORL_E_INVALID, "null array");
    if (int r = sw_sync_host(c)) return r;
    // entries this batch can create: the distinct (grain, silo) pairs of supported items that have no entry yet
    std::vector<std::pair<orl_grain_key, uint32_t>> fresh;
    for (size_t i = 0; i < n; ++i) {
        if (!sw_item_ok(c, keys[i], acts[i], silos[i]) || sw_find(c, keys[i], silos[i], nullptr) >= 0) continue;
        bool seen = false;
        for (const auto& f : fresh)
            seen = seen || (f.second == silos[i] && f.first.type_code_data == keys[i].type_code_data && f.first.n0 == keys[i].n0 &&
                            f.first.n1 == keys[i].n1);
        if (!seen) fresh.push_back({keys[i], silos[i]});
        if (fresh.size() > c->sw_table.size()) break;  // already past any capacity
    }
    if ((c->sw_count + fresh.size()) * 2 > c->sw_table.size())
        return fail(c, ORL_E_CAPACITY, "stateless-worker catalog full: %llu + %zu entries, %zu slots (orl_sw_config)",
                    (unsigned long long)c->sw_count, fresh.size(), c->sw_table.size());
    if ((c->sw_count + c->sw_tombs + fresh.size()) * 2 > c->sw_table.size()) sw_rehash(c);
    for (size_t i = 0; i < n; ++i) {
        const int t = sw_type_index(c, keys[i].type_code_data);
        if (!sw_item_ok(c, keys[i], acts[i], silos[i])) { status[i] = ORL_SW_UNSUPPORTED; continue; }
        int64_t fr = -1;
        const int64_t at = sw_find(c, keys[i], silos[i], &fr);
        if (at >= 0) {
            SwSlot& s = c->sw_table[at];
            if (sw_pos(s, acts[i]) >= 0) { status[i] = ORL_SW_UNSUPPORTED; continue; }
            if (s.count >= s.max_local) { status[i] = ORL_SW_DUPLICATE; continue; }  // Catalog.cs:1176-1180
            s.act[s.count++] = acts[i];  // appended, idle (its busy bit is clear: removal keeps the bits above count zero)
        } else {
            SwSlot& s = c->sw_table[fr];
            if (s.state == SLOT_TOMB) --c->sw_tombs;
            s = SwSlot{};
            s.tcd = keys[i].type_code_data; s.n0 = keys[i].n0; s.n1 = keys[i].n1;
            s.silo = silos[i];
            s.count = 1;
            s.state = SLOT_FULL;
            s.max_local = c->sw_max[t];
            s.act[0] = acts[i];
            ++c->sw_count;
        }
        status[i] = ORL_SW_ADDED;
        c->sw_dirty = true;
    }
    return ORL_OK;
}

int orl_sw_remove(orl_ctx* c, const orl_grain_key* keys, const uint32_t* acts, const uint8_t* silos, size_t n, uint8_t* removed) {
    if (!c) return ORL_E_INVALID;
    if (n && (!keys || !acts || !silos)) return fail(c, ORL_E_INVALID, "null array");
    if (int r = sw_sync_host(c)) return r;
    for (size_t i = 0; i < n; ++i) {
        const int64_t at = sw_find(c, keys[i], silos[i], nullptr);
        const int p = at >= 0 ? sw_pos(c->sw_table[at], acts[i]) : -1;
        if (removed) removed[i] = p >= 0 ? 1 : 0;
        if (p < 0) continue;
        SwSlot& s = c->sw_table[at];
        for (uint32_t q = (uint32_t)p; q + 1 < s.count; ++q) s.act[q] = s.act[q + 1];  // List.Remove: the order stays
        s.act[--s.count] = 0;
        s.busy = (uint8_t)((s.busy & ((1u << p) - 1u)) | ((s.busy >> (p + 1)) << p));
        if (s.count == 0) {  // an emptied list frees its entry
            s = SwSlot{};
            s.state = SLOT_TOMB;
            --c->sw_count;
            ++c->sw_tombs;
        }
        c->sw_dirty = true;
    }
    return ORL_OK;
}

int orl_sw_set_busy(orl_ctx* c, const orl_grain_key* keys, const uint32_t* acts, const uint8_t* silos, const uint8_t* busy,
                    size_t n, uint8_t* found) {
    if (!c) return ORL_E_INVALID;
    if (n && (!keys || !acts || !silos || !busy)) return fail(c, ORL_E_INVALID, "null array");
    if (int r = sw_sync_host(c)) return r;
    for (size_t i = 0; i < n; ++i) {
        const int64_t at = sw_find(c, keys[i], silos[i], nullptr);
        const int p = at >= 0 ? sw_pos(c->sw_table[at], acts[i]) : -1;
        if (found) found[i] = p >= 0 ? 1 : 0;
        if (p < 0) continue;
        SwSlot& s = c->sw_table[at];
        const uint8_t b = busy[i] ? (uint8_t)(s.busy | (1u << p)) : (uint8_t)(s.busy & ~(1u << p));
        if (b != s.busy) {
            s.busy = b;
            c->sw_dirty = true;
        }
    }
    return ORL_OK;
}

int orl_sw_set_busy_device(orl_ctx* c, const orl_grain_key* d_keys, const uint32_t* d_acts, const uint8_t* d_silos,
                           const uint8_t* d_busy, size_t n, uint8_t* d_found, void* stream) {
    if (!c) return ORL_E_INVALID;
    if (n && (!d_keys || !d_acts || !d_silos || !d_busy)) return fail(c, ORL_E_INVALID, "null device buffer");
    if (n > 0xFFFFFFFFull) return fail(c, ORL_E_CAPACITY, "batch too large");
    if (c->sw_n == 0) return fail(c, ORL_E_STATE, "no stateless-worker types set (orl_sw_types_set)");
    if (int r = sync_device_state(c)) return r;  // host changes first (refuses a host-only context)
    if (!c->d_sw) return fail(c, ORL_E_STATE, "no stateless-worker catalog on the device");
    hipStream_t st = stream_of(c, stream);
    int e = launch_sw_set_busy(c->d_sw, c->sw_mask, d_keys, d_acts, d_silos, d_busy, n, d_found, st);
    if (e) return hipfail(c, (hipError_t)e, "busy-bit launch");
    if (n) {
        c->sw_dev_newer = true;
        c->sw_dev_stream = st;
    }
    return ORL_OK;
}

int orl_sw_lookup_host(orl_ctx* c, const orl_grain_key* keys, const uint8_t* silos, size_t n, uint8_t* count, uint32_t* acts,
                       uint8_t* busy_mask) {
    if (!c) return ORL_E_INVALID;
    if (n && (!keys || !silos || !count || !acts || !busy_mask)) return fail(c, ORL_E_INVALID, "null array");
    if (int r = sw_sync_host(c)) return r;
    for (size_t i = 0; i < n; ++i) {
        const int64_t at = sw_find(c, keys[i], silos[i], nullptr);
        count[i] = at >= 0 ? c->sw_table[at].count : 0;
        busy_mask[i] = at >= 0 ? c->sw_table[at].busy : 0;
        for (uint32_t p = 0; p < ORL_SW_MAX_LOCAL; ++p)
            acts[i * ORL_SW_MAX_LOCAL + p] = (at >= 0 && p < c->sw_table[at].count) ? c->sw_table[at].act[p] : ORL_NO_ACT;
    }
    return ORL_OK;
}

int orl_sw_count(orl_ctx* c, uint64_t* n) {
    if (!c || !n) return ORL_E_INVALID;
    *n = c->sw_count;
    return ORL_OK;
}

}  // extern "C"
