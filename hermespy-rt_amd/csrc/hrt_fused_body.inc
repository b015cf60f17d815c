// Body of one macro-chunk of launch b: included (textually) by hrt_fused_kernel -- the workgroup's one chunk -- and by
// hrt_chain_kernel inside its loops (hrt_kernels.hip).  Textual, not a function: compiled inside the kernel the
// launch-0 instance keeps its 32 bytes of scratch at 72 registers; as an inlined __device__ function the same
// text came out with 112 (measured: launch 0 +7 %).
// In scope: P, b, lds; constexpr TRI_IN_LDS, VARIANT, FIRST, K, CHAIN, TXCELL; CHAIN: chunk_c, n_in_c, Ke_c, n_chunks_c
// (the macro-chunk the loop hands out), sc1_in (the live list was written inside this kernel).  `return` leaves the KERNEL: in the chain only a void step does that.
    constexpr int AUX = CHAIN ? 16 : 0;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t *counts = reinterpret_cast<uint32_t *>(P.ws + P.off_counts);
    if (!CHAIN && FIRST && blockIdx.x >= gridDim.x - P.los_blocks) {   // the LoS pass rides along (src/compute_paths.c:515-577)
        los_pairs(P, blockIdx.x - (gridDim.x - P.los_blocks));
        return;
    }
    // (one kernel per launch: the workgroup's macro-chunk is its index; the chain kernel hands them out)
    const uint32_t n_in = CHAIN ? n_in_c : (FIRST ? P.n0 : counts[b]);
    if (!CHAIN && !FIRST && (counts[P.num_bounces + 1] & kErrVoid)) return;   // an earlier fused launch of this trace timed out
    // A SHORT list is bound by the latency of one workgroup, not by throughput: then a workgroup takes
    // one packet per wave (macro-chunk = 256 entries), which spreads the list over K times as many CUs
    // (the grid covers ceil(cap / (256 K)) macro-chunks, so this needs n_in <= grid * 256).
    const uint32_t n_grid = gridDim.x - (FIRST ? P.los_blocks : 0u);
    const uint32_t Ke = CHAIN ? Ke_c : ((K > 1 && n_in <= kShortList && (uint64_t)n_grid * HRT_BLOCK >= n_in) ? 1u : (uint32_t)K);
    const uint32_t MC = Ke * HRT_BLOCK;          // entries per macro-chunk
    const uint32_t n_chunks = CHAIN ? n_chunks_c : (n_in + MC - 1u) / MC;
    const uint32_t chunk = CHAIN ? chunk_c : blockIdx.x;
    if (!CHAIN && chunk >= n_chunks) return;
    const bool do_trace = FIRST || (b < P.num_bounces);

    const uint32_t T = P.num_tri;
    const uint32_t cap4 = (uint32_t)P.cap * 4u;
    const float4 *g_tri = reinterpret_cast<const float4 *>(P.tri);
    const float2 *g_tg = reinterpret_cast<const float2 *>(P.acc.tg);
    const float4 *g_leaf = reinterpret_cast<const float4 *>(P.acc.leaf);
    const uint32_t n_leaf = P.acc.num_leaf;
    const FusedLds L = [&]() {
        if constexpr (TXCELL) return fused0_lds(lds, T, P.num_tx);
        else return fused_lds<TRI_IN_LDS, (VARIANT == 9), FIRST>(lds, T, n_leaf, P.num_rx, wave);
    }();
#ifdef HRT_PHASE_STATS
    // (make EXTRA=-DHRT_PHASE_STATS) time stamps of a workgroup's life (thread 0, 100 MHz wall clock):
    // g_phase[chunk] = {start, loads + staging done, traces + publish done, records done, prefix
    // known, stores issued}; launch HRT_PHASE_BOUNCE only (hrt_hip_read_stats dumps them to HRT_PHASE_FILE)
    int ph_i = 0;
#define HRT_PHASE(col)                                                                           \
    do {                                                                                         \
        if (tid == 0 && b == P.phase_bounce && chunk < 65536u) g_phase[chunk][ph_i++] = wall_clock64(); \
    } while (0)
    HRT_PHASE(0);
#else
#define HRT_PHASE(col) do { } while (0)
#endif

    // ---- (1) ray state of the K entries: requested before the table staging, so that both are in flight ----
    // (FIRST: htri[k] holds the entry's TX; origin and launch Doppler term are formed where they are
    // used -- the origin from the TX positions in LDS -- instead of being held in registers)
    uint32_t ray[K], htri[K];
    float theta[K], fs0[K], tau[K], a0[K], a1[K], a2[K], a3[K];
    F3 o[K], d[K];
    bool valid[K];
    // src/compute_paths.c:452-455: ray i of the launch set, lane i = the i-th ray of the coherent order
    auto launch_entry = [&](int k) {
        const uint32_t i = chunk * MC + (uint32_t)k * HRT_BLOCK + tid;
        const uint32_t tx = (P.num_tx == 1u) ? 0u : i / P.num_local;
        const uint32_t pos = i - tx * P.num_local;
        const uint32_t il = P.order ? P.order[pos] : pos;
        ray[k] = tx * P.num_local + il;
        htri[k] = tx;
        const uint64_t row = P.dirs_in_launch_order ? pos : il;
        d[k] = {P.dirs[3 * row], P.dirs[3 * row + 1], P.dirs[3 * row + 2]};
    };
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t i = chunk * MC + (uint32_t)k * HRT_BLOCK + tid;
        const uint32_t i4 = i * 4u;
        valid[k] = (uint32_t)k < Ke && i < n_in;
        ray[k] = 0u; htri[k] = 0u;
        theta[k] = 0.f; fs0[k] = 0.f; tau[k] = 0.f;
        a0[k] = 1.f; a1[k] = 0.f; a2[k] = 1.f; a3[k] = 0.f;
        o[k] = {0.f, 0.f, 0.f};
        d[k] = {0.f, 0.f, 1.f};
        if (valid[k]) {
            if (FIRST) {
                launch_entry(k);
            } else {
                const Rsrc in = hit_blk(P, b - 1);
                // (chain: the list of the chain's first launch was written by an earlier kernel -- ordinary loads;
                // the later ones by other workgroups of THIS kernel -- sc1)
                if (!CHAIN || sc1_in) {
                    ray[k] = ldu_x<AUX>(in, H_RAY * cap4, i4);
                    htri[k] = ldu_x<AUX>(in, H_TRI * cap4, i4);
                    theta[k] = ldf_x<AUX>(in, H_THETA * cap4, i4);
                    fs0[k] = ldf_x<AUX>(in, H_FS0 * cap4, i4);
                    o[k] = {ldf_x<AUX>(in, H_OX * cap4, i4), ldf_x<AUX>(in, H_OY * cap4, i4), ldf_x<AUX>(in, H_OZ * cap4, i4)};
                    d[k] = {ldf_x<AUX>(in, H_DX * cap4, i4), ldf_x<AUX>(in, H_DY * cap4, i4), ldf_x<AUX>(in, H_DZ * cap4, i4)};
                    a0[k] = ldf_x<AUX>(in, H_A0 * cap4, i4);
                    a1[k] = ldf_x<AUX>(in, H_A1 * cap4, i4);
                    a2[k] = ldf_x<AUX>(in, H_A2 * cap4, i4);
                    a3[k] = ldf_x<AUX>(in, H_A3 * cap4, i4);
                    tau[k] = ldf_x<AUX>(in, H_TAU * cap4, i4);
                } else {
                    ray[k] = ldu_x<0>(in, H_RAY * cap4, i4);
                    htri[k] = ldu_x<0>(in, H_TRI * cap4, i4);
                    theta[k] = ldf_x<0>(in, H_THETA * cap4, i4);
                    fs0[k] = ldf_x<0>(in, H_FS0 * cap4, i4);
                    o[k] = {ldf_x<0>(in, H_OX * cap4, i4), ldf_x<0>(in, H_OY * cap4, i4), ldf_x<0>(in, H_OZ * cap4, i4)};
                    d[k] = {ldf_x<0>(in, H_DX * cap4, i4), ldf_x<0>(in, H_DY * cap4, i4), ldf_x<0>(in, H_DZ * cap4, i4)};
                    a0[k] = ldf_x<0>(in, H_A0 * cap4, i4);
                    a1[k] = ldf_x<0>(in, H_A1 * cap4, i4);
                    a2[k] = ldf_x<0>(in, H_A2 * cap4, i4);
                    a3[k] = ldf_x<0>(in, H_A3 * cap4, i4);
                    tau[k] = ldf_x<0>(in, H_TAU * cap4, i4);
                }
            }
        }
    }
    // origin of launch ray k (FIRST)
    auto tx_origin = [&](int k) -> F3 {
        const uint32_t tx = htri[k];
        if (tx < kLdsTx) {
            const float4 q = L.tx[tx];
            return {q.x, q.y, q.z};
        }
        return {P.tx_pos[3 * tx], P.tx_pos[3 * tx + 1], P.tx_pos[3 * tx + 2]};
    };

    [[maybe_unused]] uint32_t matw_row = 0u;   // TXCELL: the material word of row tid, in flight until the traces' barrier
    if constexpr (CHAIN) __syncthreads();   // (the previous chunk's readers of L.wcnt are done)
    if constexpr (!CHAIN) {
        // (the tables behind the state in one flight: a load -> store -> load chain costs a round trip per 4 KB)
        if constexpr (TXCELL) fused0_stage(P, L, T, tid, matw_row);
        else fused_stage<TRI_IN_LDS, (VARIANT >= 4), FIRST>(P, L, T, n_leaf, tid);
        __syncthreads();
    }
    auto tri = [&]() {
        if constexpr (TRI_IN_LDS) return (const float4 *)L.tri;
        else return g_tri;
    }();
    auto tg = [&]() {
        if constexpr (TRI_IN_LDS) return (const float2 *)L.tg;
        else return g_tg;
    }();
    auto leaf = [&]() {
        if constexpr (TRI_IN_LDS) return (const float4 *)L.leaf;
        else return g_leaf;
    }();
    const Rsrc mesh_r = make_rsrc(reinterpret_cast<const uint8_t *>(P.mesh));
    HRT_PHASE(9);

    // (tables of <= 64 triangles: apex-bound traces go through the per-cell candidate masks)
    const bool masked = VARIANT == 2 && P.rxt.cell_mask != nullptr;
    // ---- (2) the bounce traces (src/compute_paths.c:615), survivors counted per (sub-chunk, wave) ----
    Hit h[K];
    unsigned long long hm[K];
    const LbWords W = lb_words(P, b);
    uint32_t c_total = 0u;
    if (do_trace) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            F3 apex = {0.f, 0.f, 0.f};
            uint32_t apex_k = P.num_rx;
            if (FIRST && P.rxt.num_txt != 0u) {   // the TX's direction table serves the launch packet
                uint32_t tx = 0u;
                if (P.num_tx != 1u) {
                    tx = (uint32_t)__builtin_amdgcn_readfirstlane(
                        (int)((chunk * MC + (uint32_t)k * HRT_BLOCK + (tid & ~63u)) / P.num_local));
                    tx = min(tx, P.num_tx - 1u);
                }
                apex = {P.tx_pos[3 * tx], P.tx_pos[3 * tx + 1], P.tx_pos[3 * tx + 2]};
                apex_k = P.num_rx + tx;
            }
            if ((uint32_t)k >= Ke) {   // (short list: one packet per wave)
                h[k] = {HRT_NO_HIT, 1e9f};
                hm[k] = 0ull;
                if (lane == 0) L.wcnt[16 + k * 4 + (int)wave] = 0u;
                continue;
            }
            const F3 ok = FIRST ? tx_origin(k) : o[k];
            if constexpr (TXCELL) {
                const OrigWords ow = {lds_addr(L.orig), P.acc.orig, P.fused0_words != 0u};
                h[k] = closest_hit_txcell((const float4 *)L.tri, ow, P.patch, htri[k], T, ok, d[k], valid[k], lane);
            } else if (FIRST && masked) {
                h[k] = closest_hit_masked(tri, P.acc.orig, P.rxt, P.num_rx + htri[k], T, ok, d[k], valid[k], lane, 0);
            } else if (FIRST && VARIANT == 2 && P.patch.txcell != nullptr) {
                // (never taken since the plan sends these problems to the TXCELL instantiation: kept so that the
                // shared instantiation, C4's launch 0, compiles to what it did)
                if constexpr (FIRST && VARIANT == 2) h[k] = closest_hit_txcell(tri, P.acc.orig, P.patch, htri[k], T, ok, d[k], valid[k], lane);
            } else {
                Ball ball = {{0.f, 0.f, 0.f}, 0.f, false};
                if constexpr (VARIANT >= 2 && VARIANT != 6) ball = origin_ball(ok, valid[k]);
                h[k] = closest_hit<VARIANT>(tri, tg, leaf, P.acc, P.rxt, apex_k, P.acc.orig, T, ok, d[k], valid[k], lane,
                                            ball, false, apex, L.mask, L.wleaf, FIRST ? 0 : 1);
            }
            hm[k] = HRT_BALLOT(valid[k] && h[k].tri != HRT_NO_HIT);
            if (lane == 0) L.wcnt[16 + k * 4 + (int)wave] = (uint32_t)__popcll(hm[k]);
        }
        if constexpr (TXCELL) if (P.fused0_words && tid < T) L.matw[tid] = matw_row;   // (requested at staging)
        __syncthreads();
        // (L.wcnt[16 ..]: K x 4 counts, sub-chunk-major = entry order)
#pragma unroll
        for (int q = 0; q < 4 * K; ++q) c_total += L.wcnt[16 + q];
        if (tid == 0) lb_store(W.chunk + chunk, kLbDone | c_total);
    }
    HRT_PHASE(10);

    // ---- (3) scatter records of bounce b-1: shadow ray to every RX, in order (unless hrt_records_kernel's) ----
    if constexpr (!FIRST) if (!P.records_done) {
        const uint32_t pb = b - 1;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t i = chunk * MC + (uint32_t)k * HRT_BLOCK + tid;
            const uint32_t i4 = i * 4u;
            if (HRT_BALLOT(valid[k]) == 0ull) continue;   // wave-uniform: past the end of the list
            const Ball ball = (VARIANT >= 2 && VARIANT != 6 && !masked) ? origin_ball(o[k], valid[k])
                                                                       : Ball{{0.f, 0.f, 0.f}, 0.f, false};
            F3 n = {0.f, 0.f, 1.f}, mvel = {0.f, 0.f, 0.f};
            float mat_s = 0.f, mat_alpha = 1.f, th = theta[k];
            if (valid[k]) {
                uint32_t ht = htri[k];
                if (ht >= T) {   // cannot happen; never fault
                    atomicOr(&counts[P.num_bounces + 1], 4u);
                    ht = 0u;
                }
                const float4 q2 = tri[HRT_ROW * ht + 2];
                n = {q2.y, q2.z, q2.w};
                const uint32_t mesh = __float_as_uint(tri[HRT_ROW * ht + 4].w);
                const float4 mm = gather4(mesh_r, HRT_MESH_FLOATS * 4u, mesh, 0u);
                mvel = {mm.x, mm.y, mm.z};
                const float4 m3 = L.mat[4u * __float_as_uint(mm.w) + 3u];
                mat_s = m3.x;
                mat_alpha = m3.y;
            }
            for (uint32_t rx = 0; rx < P.num_rx; ++rx) {
                const float4 rp = L.rx[rx];
                const F3 apex = {rp.x, rp.y, rp.z};
                float d2rx;
                F3 w = shadow_dir(o[k], apex, d2rx);
                if (!valid[k]) w = {0.f, 0.f, 1.f};
                const Hit sh = masked ? closest_hit_masked<true>(tri, P.acc.orig, P.rxt, rx, T, o[k], w, valid[k], lane, 2)
                                      : closest_hit<VARIANT>(tri, tg, leaf, P.acc, P.rxt, rx, P.acc.orig, T, o[k], w, valid[k],
                                                             lane, ball, true, apex, L.mask, L.wleaf, 2);
                bool unblocked = false;
                if (valid[k]) {
                    const Rsrc rec = rec_blk(P, pb, rx);
                    if (sh.tri != HRT_NO_HIT) {
                        const float4 s2 = tri[HRT_ROW * sh.tri + 2];
                        th = incidence_angle({s2.y, s2.z, s2.w}, w);
                    }
                    if (sh.tri != HRT_NO_HIT && sh.t <= 1.f) {
                        stf(rec, R_A0 * cap4, i4, 0.f);
                        stf(rec, R_A1 * cap4, i4, 0.f);
                        stf(rec, R_A2 * cap4, i4, 0.f);
                        stf(rec, R_A3 * cap4, i4, 0.f);
                        stf(rec, R_TAU * cap4, i4, 0.f);
                    } else {
                        unblocked = true;
                        const float th_s = acos_f_ool(dot3(w, n));
                        const float4 S = scatter_pattern(mat_s, mat_alpha, th_s, th, lds_addr(L.mat + kMatItems));
                        float o0 = a0[k] * S.x - a1[k] * S.y;
                        float o1 = a0[k] * S.y + a1[k] * S.x;
                        float o2 = a2[k] * S.z - a3[k] * S.w;
                        float o3 = a2[k] * S.w + a3[k] * S.z;
                        float f2 = P.fsl_mult * d2rx;
                        f2 *= f2;
                        if (f2 > 1.f) { o0 /= f2; o1 /= f2; o2 /= f2; o3 /= f2; }
                        stf(rec, R_A0 * cap4, i4, o0);
                        stf(rec, R_A1 * cap4, i4, o1);
                        stf(rec, R_A2 * cap4, i4, o2);
                        stf(rec, R_A3 * cap4, i4, o3);
                        stf(rec, R_TAU * cap4, i4, tau[k] + div_c(d2rx));
                        stf(rec, R_DX * cap4, i4, -w.x);
                        stf(rec, R_DY * cap4, i4, -w.y);
                        stf(rec, R_DZ * cap4, i4, -w.z);
                        stf(rec, R_DFS * cap4, i4, dot3(sub3(w, d[k]), mvel) * P.dop_mult);
                    }
                }
                const unsigned long long um = HRT_BALLOT(unblocked);
                if (lane == 0 && valid[k]) mask_words(P, pb, rx)[i >> 6] = um;
            }
        }
    }

    HRT_PHASE(11);
    // ---- (4) survivors of all earlier macro-chunks, (5) the bounce itself (:616-659) and the stores ----
    if (do_trace) {
        // Later launches: what the shading reads from memory -- the hit triangle's normal and material --
        // is requested HERE, in front of the wait, so that the shading loop behind it has no load in
        // front of its stores (C4 launch 1: 0.345 -> 0.329 ms).  Launch 0 keeps its registers instead
        // (7 waves per SIMD): it reads the launch ray AGAIN inside the loop (id and direction were not
        // kept through the traces; the lines were touched a few us ago: L2 / MALL hits) -- hoisting
        // those K * 12 registers in front of the wait spills and costs more than it hides (0.309 -> 0.355).
        F3 nk[K];
        uint32_t matk[K];
        if constexpr (!FIRST) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                nk[k] = {0.f, 0.f, 1.f};
                matk[k] = 0u;
                if (valid[k] && h[k].tri != HRT_NO_HIT) bounce_fetch(tri, mesh_r, h[k].tri, nk[k], matk[k]);
            }
        }
        // A chunk without survivors stores nothing: it needs its prefix only if somebody else needs
        // something FROM it -- it closes a group / supergroup (their totals), or it is the last chunk (the
        // list's length).  Half of C4's launch-0 chunks (the upper hemisphere) and nearly all of its
        // launch-1 chunks leave here without waiting for the chunks in front of them (C4 0.725 -> 0.68 ms).
        // (Requesting the words before the first packet is shaded and looking at them after it -- the
        // packet's result waiting in registers -- was measured too: spills at 7 waves, 0.265 -> 0.29 ms.)
        const bool need_prefix = c_total != 0u || (chunk & 63u) == 63u || chunk + 1u == n_chunks;
        if (need_prefix) {   // (uniform over the workgroup)
            if (tid < 64u) {   // wave 0
                const uint32_t excl = lb_exclusive(W, chunk, c_total, lane, &counts[P.num_bounces + 1], P.host_flag, P.tune.lb_max_polls,
                                                   CHAIN ? kErrChainTimeout : kErrFuseTimeout);
                if (lane == 0) {
                    L.wcnt[8] = excl;
                    if (excl != kLbAbort && chunk + 1u == n_chunks) {   // the next live list's length
                        if constexpr (CHAIN) lb_store(&counts[b + 1], excl + c_total);
                        else counts[b + 1] = excl + c_total;
                    }
                }
            }
            __syncthreads();
            if (L.wcnt[8] == kLbAbort) return;   // (uniform) the launch is void: see lb_exclusive
        }
        HRT_PHASE(12);
        uint32_t pos = L.wcnt[8];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            // survivors of this wave's k-th packet start behind those of (k, earlier waves)
            uint32_t before = 0u, sub = 0u;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t cw = L.wcnt[16 + k * 4 + w];
                before += ((uint32_t)w < wave) ? cw : 0u;
                sub += cw;
            }
            const bool hit = valid[k] && h[k].tri != HRT_NO_HIT;
            if (hit) {
                float nth = 0.f;
                if constexpr (FIRST) {   // src/compute_paths.c:460-466 state init, :494-500 the launch Doppler term
                    // (issuing these loads one packet ahead of the stores -- loads and stores share vmcnt --
                    // was measured too: 12 more registers, spills at 7 waves, 0.309 -> 0.34 ms on C4)
                    launch_entry(k);
                    const uint32_t tx = htri[k];
                    o[k] = tx_origin(k);
                    const F3 tv = {P.tx_vel[3 * tx], P.tx_vel[3 * tx + 1], P.tx_vel[3 * tx + 2]};
                    fs0[k] = dot3(tv, d[k]) * P.dop_mult;
                    if constexpr (TXCELL) bounce_fetch0(L.tri, L.matw, P.fused0_words != 0u, mesh_r, h[k].tri, nk[k], matk[k]);
                    else bounce_fetch(tri, mesh_r, h[k].tri, nk[k], matk[k]);
                }
                bounce_apply<(FIRST && HRT_FUSED_INLINE0)>(L.mat, P.fsl_mult, nk[k], matk[k], h[k].t, o[k], d[k], a0[k], a1[k], a2[k], a3[k], tau[k], nth);
                const uint32_t k4 = (pos + before + lane_prefix(hm[k])) * 4u;
                store_survivor<AUX>(hit_out(P, b), cap4, k4, ray[k], h[k].tri, nth, fs0[k], o[k], d[k], a0[k], a1[k], a2[k],
                               a3[k], tau[k]);
            }
            pos += sub;
        }
        HRT_PHASE(13);
    }
#undef HRT_PHASE
