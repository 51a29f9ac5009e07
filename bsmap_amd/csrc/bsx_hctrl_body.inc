// bsx_hctrl_body.inc — the body of the heavy pipeline's control kernel, included by bsx_align.hip once for k_hctrl (BSX_HCTRL_AH 0) and once for its
// emitting twin k_hctrl_ah (BSX_HCTRL_AH 1: the all-hits emission behind unit_finish, argument X_).  One text, so the two cannot drift; and k_hctrl is, token
// for token, the kernel it was before the twin existed.
    __shared__ BlockLds BL;
    __shared__ WaveLds<PE> WL[4];
    __shared__ u64 SORTBUF[4][BSX_LDS_SORT];
    // The helpers called from here (scan, replay, prepare / finish, state save / restore) are real calls that take the arguments,
    // the cursor, the counters and the slab pointers by reference: as private objects they would live in scratch memory — 256 bytes
    // and four cache lines per scalar access, in a kernel that is one chain of dependent accesses.  All of them are wave-uniform:
    // one copy per block (arguments) or per wave in LDS instead.
    __shared__ AlignArgs As;
    __shared__ HeavyArgs Hs;
    __shared__ HCursor KS[4];
    __shared__ Counters CS[4];
    __shared__ UnitSlabs US[4];
    __shared__ uint32_t PEND[4][32];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < sizeof(AlignArgs) / 4; i += 256) ((uint32_t *)&As)[i] = ((const uint32_t *)&A_)[i];
    for (uint32_t i = threadIdx.x; i < sizeof(HeavyArgs) / 4; i += 256) ((uint32_t *)&Hs)[i] = ((const uint32_t *)&H_)[i];
    __syncthreads();
    const AlignArgs &A = As;
    const HeavyArgs &H = Hs;
    init_block_lds(A.P, BL, threadIdx.x, 256);
    __syncthreads();
    MateLds &LA = WL[wv].mate[0];
    MateLds &LB = WL[wv].mate[PE ? 1 : 0];
    Counters Cflush = {0, 0, 0, 0};
    u64 n_units_done = 0, n_aligned = 0, n_aligned_pairs = 0;
    const uint32_t n_active_in = H.fresh ? H.n_active_in : rfl(*H.n_active_in_ptr);  // later passes: count left by the previous pass
    // One word takes ~88 atomics per microsecond and an RRBS pass visits 10^5 units: a wave takes queue entries in chunks (one while units are few: the pass
    // then ends with its longest visit, not with a wave's leftover chunk) and hands in the units it leaves active 32 at a time (PEND).
#ifndef BSX_QCHUNK_DIV
#define BSX_QCHUNK_DIV 128u
#endif
    const uint32_t q_chunk = BSX_HCTRL_BATCH ? max(1u, min(16u, n_active_in / (gridDim.x * BSX_QCHUNK_DIV))) : 1u;   // (RRBS: 175 short visits per wave and pass, chunks of 5; C5: 25 long ones, one at a time)
    uint32_t q_next = 0, q_end = 0, n_pend = 0;
    uint32_t *const pend = PEND[wv];
#define HCTRL_PEND_FLUSH() do { if (n_pend) { uint32_t b_ = 0; if (lane == 0) b_ = atomicAdd(H.n_active_out, n_pend); b_ = rfl(b_); if ((uint32_t)lane < n_pend) H.active_out[b_ + (uint32_t)lane] = pend[lane]; n_pend = 0; wave_fence(); } } while (0)
#define HCTRL_PEND_PUSH(x) do { if (lane == 0) pend[n_pend] = (x); n_pend++; wave_fence(); if (n_pend == (BSX_HCTRL_BATCH ? 32u : 1u)) HCTRL_PEND_FLUSH(); } while (0)
    for (;;) {
        if (q_next == q_end) {
            uint32_t i0 = 0;
            if (lane == 0) i0 = atomicAdd(H.queue, q_chunk);
            q_next = rfl(i0); q_end = min(q_next + q_chunk, n_active_in);
            if (q_next >= n_active_in) break;
        }
        const uint32_t i = q_next++;
        // (later passes take the list back to front: a unit whose visit ended last in the previous pass — a long visit — was appended
        //  last; starting those first keeps the pass from waiting for one long visit that began when all the others were done)
        const uint32_t hidx = H.fresh ? H.hidx_base + i : rfl(H.active_in[n_active_in - 1u - i]);
        const uint32_t unit = rfl(A.heavy_list[H.list_base + hidx]);
        HState *S = &H.state[hidx];
        if (!H.fresh) {
            // a unit whose last request was refused stays parked (no state restore / save) while the pool cannot take it:
            // n_tasks only grows during a pass, so the reservation below would be refused again
            const uint32_t want = rfl(S->want);
            if (want && rfl(__hip_atomic_load(H.n_tasks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) + want > H.task_cap) {
                HCTRL_PEND_PUSH(hidx);
                continue;
            }
        }
        // (the slabs of deferred units carry the ordinary, small duplicate set even where the main kernel's are large — single-end
        //  RRBS —: there are too many deferred units for 4 MB each; a unit that overflows it is redone by the main kernel, below)
        uint8_t *slab = A.debug ? A.scratch + (size_t)unit * A.slab_bytes : H.slabs + (size_t)hidx * A.hslab_bytes;
        UnitSlabs &U = US[wv];
        U = A.debug ? carve_slab(slab, (uint32_t)A.P.max_snp_num + 1, A.rowcap, PE, A.kcap, A.hbits)
                    : carve_slab(slab, (uint32_t)A.P.max_snp_num + 1, A.rowcap, PE, A.hkcap, A.hhbits);
        Mate MA, MB;
        MA.u = lds_mate(&LA.u); MB.u = PE ? lds_mate(&LB.u) : lds_mate(&LA.u2);
        Counters &C = CS[wv];
        C.n_lookup = 0; C.n_cand = 0; C.sum_w = 0; C.n_orient = 0;
        HCursor &K = KS[wv];
        K.n_active = n_active_in; K.want = 0;
        for (int k_ = 0; k_ < 8; k_++) { K.vc[k_] = 0; K.vn[k_] = 0; }
        uint32_t pcnt_reg = 0;
        const u64 cat_prep0 = A.dbg_cat ? __builtin_readcyclecounter() : 0;
        if (H.fresh) {
            unit_prepare<PE, true>(A, BL, LA, LB, MA, MB, unit, lane, C);
            K.level = 0; K.sub = 0; K.paired = 0;
            for (int m_ = 0; m_ < 2; m_++) { K.orient[m_] = 0; K.have[2 * m_] = 0; K.have[2 * m_ + 1] = 0; K.c[m_] = 0; K.W[m_] = HS_WIN0; }
        } else {
            load_mate(S->mate[0], MA, LA, lane);
            if (PE) load_mate(S->mate[1], MB, LB, lane); else MB = MA;
            C = S->C;
            C.n_lookup = (u64)rfl((uint32_t)(C.n_lookup >> 32)) << 32 | rfl((uint32_t)C.n_lookup); C.n_cand = (u64)rfl((uint32_t)(C.n_cand >> 32)) << 32 | rfl((uint32_t)C.n_cand);
            C.sum_w = (u64)rfl((uint32_t)(C.sum_w >> 32)) << 32 | rfl((uint32_t)C.sum_w); C.n_orient = (u64)rfl((uint32_t)(C.n_orient >> 32)) << 32 | rfl((uint32_t)C.n_orient);
            pcnt_reg = S->pcnt_reg[lane];
            K.level = (int)rfl((uint32_t)S->level); K.sub = (int)rfl((uint32_t)S->sub); K.paired = (int)rfl((uint32_t)S->paired);
            for (int m_ = 0; m_ < 2; m_++) {
                K.orient[m_] = (int)rfl((uint32_t)S->orient[m_]); K.have[2 * m_] = (int)rfl((uint32_t)S->have[2 * m_]); K.have[2 * m_ + 1] = (int)rfl((uint32_t)S->have[2 * m_ + 1]); K.c[m_] = rfl(S->c[m_]); K.W[m_] = rfl(S->W[m_]);
            }
        }
        if (A.dbg_cat && lane == 0) { const u64 d_ = (u64)__builtin_readcyclecounter() - cat_prep0; atomicAdd((u64 *)&A.dbg_cat[0], d_); atomicMax((u64 *)&A.dbg_cat[8], d_); }
        const u64 cat_adv0 = A.dbg_cat ? __builtin_readcyclecounter() : 0;
        const bool done = heavy_advance<PE>(A, H, S, hidx, BL, LA, LB, MA, MB, U, pcnt_reg, K, lane, C, SORTBUF[threadIdx.x >> 6]);
        if (A.dbg_cat && lane == 0) {
            const u64 d_ = (u64)__builtin_readcyclecounter() - cat_adv0;
            atomicAdd((u64 *)&A.dbg_cat[6], d_);
            if (atomicMax((u64 *)&A.dbg_cat[14], d_) < d_)  // the longest visit so far: leave its break-down (racy, diagnostics only)
                for (int k_ = 0; k_ < 6; k_++) A.dbg_cat[16 + k_] = (K.vc[k_] << 16) | min(K.vn[k_], 0xffffu);
        }
        const u64 cat_fin0 = A.dbg_cat ? __builtin_readcyclecounter() : 0;
        if (done && ((MA.u->flags | (PE ? MB.u->flags : 0u)) & 4u)) {
            // the small duplicate set of this unit's heavy slab overflowed (single-end RRBS: coordinates its fragment filter rejects
            // are remembered too): its records are not written; the main kernel redoes it alone with its large set, undeferred
            forget_keys(MA, U.SA, lane); if (PE) forget_keys(MB, U.SB, lane);
            if (lane == 0) A.redo_list[atomicAdd(A.redo_count, 1u)] = unit;
        } else if (done) {
            unit_finish<PE>(A, LA, LB, MA, MB, U, pcnt_reg, K.paired, unit, lane, n_aligned, n_aligned_pairs);
#if BSX_HCTRL_AH
            unit_all_hits<PE>(A.P, X_, MA, MB, U, pcnt_reg, K.paired, unit, lane);
#endif
            Cflush.n_lookup += C.n_lookup; Cflush.n_cand += C.n_cand; Cflush.sum_w += C.sum_w; Cflush.n_orient += C.n_orient;
            n_units_done++;
        } else {
            save_mate(S->mate[0], MA, LA, lane);
            if (PE) save_mate(S->mate[1], MB, LB, lane);
            S->pcnt_reg[lane] = pcnt_reg;
            if (lane == 0) {
                S->want = K.want; S->C = C; S->level = K.level; S->sub = K.sub; S->paired = K.paired;
                for (int m_ = 0; m_ < 2; m_++) {
                    S->orient[m_] = K.orient[m_]; S->have[2 * m_] = K.have[2 * m_]; S->have[2 * m_ + 1] = K.have[2 * m_ + 1]; S->c[m_] = K.c[m_]; S->W[m_] = K.W[m_];
                }
            }
            HCTRL_PEND_PUSH(hidx);
        }
        if (A.dbg_cat && lane == 0) { const u64 d_ = (u64)__builtin_readcyclecounter() - cat_fin0; atomicAdd((u64 *)&A.dbg_cat[4], d_); atomicMax((u64 *)&A.dbg_cat[12], d_); }
        wave_fence();
    }
    HCTRL_PEND_FLUSH();
#undef HCTRL_PEND_PUSH
#undef HCTRL_PEND_FLUSH
    if (lane == 0) flush_counters(A, Cflush, n_units_done, n_aligned, n_aligned_pairs);
