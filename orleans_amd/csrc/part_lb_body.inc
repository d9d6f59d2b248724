// The body of k_part_lb and k_part_lb_sw (route_kernels.hip includes it inside each of the two kernels, after defining
// kSw and swp).  As a shared __forceinline__ function the plain k_part_lb forms compiled differently (kernel_resources.py:
// seven of the eight changed their VGPR count, <32, false, false> from 128 to 137 and from 4 to 3 waves per SIMD);
// included as text they compile exactly as they did before the SW forms existed.
//   kSw (constexpr bool): stateless-worker types set: destinations by dest_rank<true> / dest_rank_cached<true>, which
//   keep a listed type's messages in the self segment.  swp (const SwView*): the types (nullptr when !kSw).
    static_assert(!KX || FMT == 32, "KeyExt strings travel beside 32-B records only");
    __shared__ PartLbSmem sm;
    const uint32_t rflags = rank_flags();
    stage_params(&sm.P, gp);
    sm.rank_of_silo[threadIdx.x] = ros[threadIdx.x];
    if (threadIdx.x < kWaves * 8) (&sm.lb.cnt[0][0])[threadIdx.x] = 0;
    if (threadIdx.x == 0) sm.lb.tile = atomicAdd(&state[0], 1u) - tbase;  // the ticket counter runs on across launches
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t t = sm.lb.tile;
    const uint32_t wbase = t * kPartTile + w * (kPartItems * 64u);
    u32x4 h0[kPartItems], h1[kPartItems];
    uint32_t dig[kPartItems], rank[kPartItems];
    uint2 nrec[kPartItems];  // FMT 8: the records, encoded before the ranking so the 32-B headers leave the registers
    uint32_t cact[CACHE ? kPartItems : 1];  // CACHE: the cached handle of each message (ORL_NO_ACT: not cached)
    uint32_t bad = 0, ncached = 0;
    // FMT 8 loads and encodes the tile's headers in kPartGroups groups (a scheduling barrier keeps a group's loads from
    // being hoisted above the previous group's encoding), so only one group's 32-B headers are live at a time: fewer
    // VGPRs, more tiles resident per CU to cover the look-back's device round trips.  Wider records keep the headers.
    constexpr uint32_t G = FMT == 8 ? kPartGroups : 1u, GI = kPartItems / G;
#pragma unroll
    for (uint32_t gq = 0; gq < G; ++gq) {
#pragma unroll
        for (uint32_t jj = 0; jj < GI; ++jj) {  // unconditional (clamped) loads: the group's in flight together
            const uint32_t j = gq * GI + jj, e = wbase + j * 64u + lane;
            const u32x4* sp = reinterpret_cast<const u32x4*>(in + (e < n ? e : n - 1));
            h0[j] = __builtin_nontemporal_load(sp);
            h1[j] = __builtin_nontemporal_load(sp + 1);
        }
#pragma unroll
        for (uint32_t jj = 0; jj < GI; ++jj) {
            const uint32_t j = gq * GI + jj;
            dig[j] = 0;
            if (CACHE) cact[j] = ORL_NO_ACT;
            if (wbase + j * 64u + lane < n) {
                Msg m;
                m.tcd = (uint64_t)h0[j].x | ((uint64_t)h0[j].y << 32);
                m.n0 = (uint64_t)h0[j].z | ((uint64_t)h0[j].w << 32);
                m.n1 = (uint64_t)h1[j].x | ((uint64_t)h1[j].y << 32);
                m.meta = h1[j].z;
                m.aux = h1[j].w;
                if (KX && (uint32_t)(m.tcd >> 56) == ORL_CAT_KEYEXT_GRAIN &&
                    !(((m.meta >> 16) & 0xFFu) & (ORL_HDR_HASH_VALID | ORL_HDR_ADDRESS_COMPLETE))) {
                    const orl_ext_ref x = kx.in[wbase + j * 64u + lane];
                    if ((uint64_t)x.off + x.len <= kx.blob_bytes) {  // the KeyExt hash from the bytes, carried by the record
                        m.aux = keyext_hash_dev(m.n0, m.n1, m.tcd, kx.blob + x.off, x.len);
                        m.meta |= ORL_HDR_HASH_VALID << 16;
                        h1[j].z = m.meta;
                        h1[j].w = m.aux;
                    }
                }
                if (CACHE) {
                    uint32_t chost;
                    dig[j] = dest_rank_cached<kSw>(sm.P, sm.rank_of_silo, cache, cmask, m, excl != 0, my_rank, cact[j], chost,
                                                  wbase + j * 64u + lane, swp);
                    if (cact[j] != ORL_NO_ACT) {  // addressed: TargetSilo = the cached silo (Message.SetTargetPlacement)
                        h1[j].z = (h1[j].z & 0x00FFFFFFu) | (chost << 24);
                        ++ncached;
                    }
                } else {
                    dig[j] = dest_rank<kSw>(sm.P, sm.rank_of_silo, m, excl != 0, my_rank, swp);
                }
                if (FMT == 8) {
                    u32x4 wr;
                    bad |= (encode_wire(h0[j], h1[j], wr) ? 0u : 1u) | (encode_narrow(sm.P, h0[j], h1[j], nrec[j]) ? 0u : 2u);
                }
            }
        }
        if (G > 1 && gq + 1 < G) __builtin_amdgcn_sched_barrier(0);
    }
    if (FMT == 8 && bad) atomicOr(wire_status, bad);
    if (CACHE && __ballot(ncached != 0u) && lane == 0) atomicOr(wire_status, ORL_PART_CACHED);
    rank_steps<3, false, kPartItems, kPartRm>(&sm.lb.cnt[w][0], dig, n > wbase ? n - wbase : 0u, rank, rflags);
    __syncthreads();
    lookback_ranks(sm.lb, state, nranks, ntiles, counts, nullptr, epoch, wire_status);
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kPartItems; ++j) {
        const uint32_t e = wbase + j * 64u + lane;
        if (e < n) {
            const uint32_t d = dig[j];
            const uint64_t g = (uint64_t)d * stride + sm.lb.base[d] + sm.lb.cnt[w][d] + rank[j];
            if (FMT == 16) {
                u32x4 wr;
                if (!encode_wire(h0[j], h1[j], wr)) atomicOr(wire_status, 1u);
                reinterpret_cast<u32x4*>(out)[g] = wr;
            } else if (FMT == 8) {
                reinterpret_cast<uint2*>(out)[g] = nrec[j];
            } else {
                u32x4* dp = reinterpret_cast<u32x4*>(static_cast<orl_msg_hdr*>(out) + g);
                dp[0] = h0[j];
                dp[1] = h1[j];
            }
            if (src_index) src_index[g] = e;
            if (CACHE) act_out[g] = cact[j];
            if (KX) {
                orl_ext_ref r{0xFFFFFFFFu, 0xFFFFFFFFu};
                const uint32_t hf = (h1[j].z >> 16) & 0xFFu;
                if ((h0[j].y >> 24) == ORL_CAT_KEYEXT_GRAIN && !(hf & ORL_HDR_ADDRESS_COMPLETE)) {
                    const orl_ext_ref x = kx.in[e];
                    if ((uint64_t)x.off + x.len <= kx.blob_bytes) {
                        const uint32_t o = atomicAdd(&kx.cur[d], x.len);
                        if ((uint64_t)o + x.len <= kx.blob_cap) {
                            uint8_t* dst = kx.blob_out + (uint64_t)d * kx.blob_cap + o;
                            for (uint32_t b = 0; b < x.len; ++b) dst[b] = kx.blob[x.off + b];
                            r = orl_ext_ref{o, x.len};
                            atomicOr(wire_status, ORL_PART_KEYEXT);
                        } else {
                            atomicOr(wire_status, ORL_PART_EXT_FULL);
                        }
                    }
                }
                kx.out[g] = r;
            }
        }
    }
