// ntt16_kernel_body.inc -- the body of the 16-coefficient transform kernels of ntt16_kernel.h, included into each of them (a kernel
// that called it as a function would not compile to the listing it had): expects LOGNS, INV, LIFT, TENSOR, FD and the argument `a`.
    typedef Geo<LOGNS> G;
    constexpr u32 NS = G::NS, T = G::T, R = G::R, LOGR = G::LOGR, CPT = G::CPT, TWK_PER_SLICE = G::TWK_PER_SLICE;
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const u32 tau = threadIdx.x;
    const u32 w = __builtin_amdgcn_readfirstlane(tau >> 6), l = tau & 63;
    const u32 la = l >> 2, lc = l & 3;
    // element -> image position, per layout (phi(e) = e + 2 (e >> 5)):
    //   pass 1: e = 1024 r + 2 tau          -> p1 + 1088 r            p1 = phi(2 tau)
    //   pass 2: e = 1024 w + 64 k + l       -> p2 + 68 k              p2 = phi(1024 w + l)
    //   pass 3: e = 1024 w + 64 a + 4 k + c -> p3 + 4 k + 2 (k >> 3)  p3 = 1088 w + 68 a + c
    //   pass 4: e = 1024 w + 16 l + k       -> p4 + k                 p4 = phi(1024 w + 16 l)
    u64 *const p1 = lds + phi(CPT * tau);
    u64 *const p2 = lds + phi(1024 * w + l);
    u64 *const p3 = lds + 1088 * w + 68 * la + lc;
    u64 *const p4 = lds + phi(1024 * w + 16 * l);

    u64 x[16];
    // item -> (limb, slice of the limb); forward launches may enumerate [nb][4][skip_M] without the Q limbs of slots 0, 1
    auto limb_of = [&](u32 it) -> u32 {
        u32 lb = it >> a.s0;
        if (!INV && a.skip_L) {
            const u32 P = a.skip_M - a.skip_L, per = 2 * P + 2 * a.skip_M;
            const u32 cb = lb / per, r = lb % per;
            lb = cb * 4 * a.skip_M + (r < 2 * P ? (r / P) * a.skip_M + a.skip_L + r % P : 2 * a.skip_M + (r - 2 * P));
        }
        return lb;
    };
    for (u32 item = blockIdx.x; item < a.nitems; item += gridDim.x) {
        // The lane offsets are made opaque once per item: as loop invariants the compiler widens them to 64-bit pairs, adds the
        // table bases it can hoist, keeps all of that alive across the loop -- and, at this kernel's register budget, spills it.
        // Only the thread index itself is carried from item to item; the four offsets are a handful of instructions per slice.
        u32 tau_ = tau;
        asm volatile("" : "+v"(tau_));
        const u32 voffb = 16 * tau_;       // lane offset (in bytes) of the lane-ordered pairs 2 (T j + tau)
        const u32 coffb = 8 * CPT * tau_;  // ... and of the row accesses 1024 r + CPT tau (pass 1)
        const u32 lab = 4 * (tau_ & 60), lb = 16 * (tau_ & 63);  // ... and into the kernel-ordered twiddle tables of passes 3 (16 la) and 4 (16 l)
        const bool lift = LIFT && !INV && item >= a.lift_first;
        // The G = lift_L * 2^s0 digit items of one (ciphertext, source limb) read the same source limb.  Consecutive workgroups sit
        // on consecutive XCDs, each with its own L2: dealt in order, every XCD fetches every source limb from HBM.  Transposing each
        // block of 8 G items (8 x G) hands the items that share a source to workgroups 8 apart -- one XCD, one fetch, G - 1 L2 hits.
        u32 item_l = item;
        if (lift) {
            item_l = item - a.lift_first;
#if NTT16_LIFT_XCD
            const u32 G = a.lift_L << a.s0, blk8 = 8 * G, within = item_l % blk8;
            if (item_l - within + blk8 <= a.nitems - a.lift_first) item_l = item_l - within + (within & 7) * G + (within >> 3);
#endif
        }
        // TENSOR: the three items d = 0, 1, 2 of one (row, limb, slice) read the same four operand slices (a0 b0 | a0 b1 a1 b0 | a1 b1).
        // Enumerated with d innermost and dealt like the digit items above (blocks of 8 x 3), they run in workgroups 8 apart in the
        // same round: one XCD, each operand slice fetched once.  (The persistent grid strides by gridDim.x = 16 mod 24 or 8 mod 24
        // on 256 CUs: a workgroup's items cycle through d, none collects the twice as long d = 1 items.)
        // With tq_L the triples are those of the P limbs only (their last, incomplete block of 24 in natural order, as before); the Q limbs'
        // d2 items share their operands with nobody and follow in natural order -- the shortest items, at the launch's tail.
        u32 t_d = 0, t_row = 0, t_blk = 0, t_limb = 0;
        if (TENSOR) {
            const u32 M_ = a.mod_count, TL = a.tq_L, TM = M_ - TL;  // TM: limbs with triples
            if (item < a.tq_first) {
#if NTT16_TENSOR_XCD
                u32 il = item;
                const u32 within = il % 24;
                if (il - within + 24 <= a.tq_first) il = il - within + (within & 7) * 3 + (within >> 3);
                const u32 u = il / 3, lm = u >> a.s0;
                t_d = il % 3, t_blk = u & ((1u << a.s0) - 1), t_row = lm / TM;
                t_limb = (t_row * 3 + t_d) * M_ + TL + lm % TM;
#else
                const u32 lm = item >> a.s0;
                t_blk = item & ((1u << a.s0) - 1);
                t_row = lm / (3 * TM), t_d = (lm / TM) % 3;
                t_limb = (t_row * 3 + t_d) * M_ + TL + lm % TM;
#endif
            } else {
                const u32 v = item - a.tq_first, lm = v >> a.s0;
                t_d = 2, t_blk = v & ((1u << a.s0) - 1), t_row = lm / TL;
                t_limb = (t_row * 3 + 2) * M_ + lm % TL;
            }
            t_d = __builtin_amdgcn_readfirstlane(t_d), t_row = __builtin_amdgcn_readfirstlane(t_row);
            t_blk = __builtin_amdgcn_readfirstlane(t_blk), t_limb = __builtin_amdgcn_readfirstlane(t_limb);
        }
        const u32 blk = TENSOR ? t_blk : item_l & ((1u << a.s0) - 1);
        const u32 limb = TENSOR ? t_limb : lift ? item_l >> a.s0 : limb_of(item);
        // (uniform; laundered through a scalar register pair so that the slice's addresses stay "scalar base + lane offset": left to
        // itself the compiler hoists a.data + lane offset out of the item loop as a 64-bit vector base, which the inverse kernel
        // -- at its 128-register budget -- spilled to scratch, and a scratch reload is a vector-memory operation: the
        // s_waitcnt vmcnt(0) in front of its use drained the previous slice's stores and this slice's twiddle loads before the
        // first data load was even issued)
        u64 *g = (lift ? a.data2 : a.data) + (((size_t)limb << a.s0) + blk) * NS;
        asm("" : "+s"(g));
        const u32 mod = __builtin_amdgcn_readfirstlane(a.mod_base + limb % a.mod_count);
        const DcS dcs = (DcS)(u64)a.dc;
        const u64 q = dcs->mod[mod].q;
        const u64 q2 = 2 * q, q4 = 4 * q;
        ModC mc;
        mc.nql = (u32)(0 - q), mc.nqh = (u32)((0 - q) >> 32), mc.nq4 = 0 - q4, mc.q4 = q4;
        const TwS tw = (TwS)(u64)(a.twp + ((size_t)mod * 2 + (INV ? 1 : 0)) * a.N);
        const u64x2 *__restrict__ twk = a.twk + (((size_t)mod * 2 + (INV ? 1 : 0)) << a.s0) * TWK_PER_SLICE + (size_t)blk * TWK_PER_SLICE;
        const u64x2 *__restrict__ tw3 = twk + (size_t)w * 15 * 16;                 // [slot 0..14][16 a]
        const u64x2 *__restrict__ tw4 = twk + G::W * 15 * 16 + (size_t)w * 12 * 64;   // [slot 0..11][64 l]
        // per-lane twiddles of passes 3 and 4, loaded one stage ahead of their use (named by stage: 7, 8, 9, 10, 11, 12)
        u64x2 t7[1], t8[2], t9[4], t10[8], t11[4], t12[8];
#define NTT16_LOAD3(dst, sc)                                                       \
    _Pragma("unroll") for (int j_ = 0; j_ < (1 << (sc)); j_++) dst[j_] = *at_bytes(tw3 + 16 * ((1 << (sc)) - 1 + j_), lab)
#define NTT16_LOAD3H(dst, sc, from)                                                \
    _Pragma("unroll") for (int j_ = (from); j_ < (from) + 4; j_++) dst[j_] = *at_bytes(tw3 + 16 * ((1 << (sc)) - 1 + j_), lab)
#define NTT16_LOAD4(dst, first, n)                                                 \
    _Pragma("unroll") for (int j_ = 0; j_ < (n); j_++) dst[j_] = *at_bytes(tw4 + 64 * ((first) + j_), lb)

        if (!INV) {
            NTT16_STAMP(0);
            NTT16_PRIO_F(0);
            // ---- pass 1: rows r = 0..7 (bits 12..10) of the column pair -------------------------------------------------
            if (lift) {
                // Centred lift of a residue v of q_i into q_j for equal-width primes (q_i < 2 q_j for every pair: the host checks):
                // the centred representative v - [v > q_i / 2] q_i lies in (-q_j, q_j), so its residue mod q_j is v itself for
                // v <= floor(q_i / 2) and v + (q_j - q_i) above -- one masked 64-bit add, canonical result (five instructions; the
                // formulation it replaces reduced v mod q_j first and corrected by q_i mod q_j with a sign fix-up: fourteen).
                const u32 LL = a.lift_L, li = __builtin_amdgcn_readfirstlane((limb / LL) % LL), lj = __builtin_amdgcn_readfirstlane(limb % LL);
                const u64 *src = a.lift_src + (size_t)(limb / (LL * LL)) * a.lift_stride + (size_t)li * a.N;
                const u64 qi = dcs->mod[li].q;
                const u64 nqh1 = 0 - (qi / 2 + 1), dq = q - qi;
                auto lift1 = [&](u64 v) -> u64 {
                    u64 r;
                    asm("v_lshl_add_u64 v[126:127], %[v], 0, %[nqh1]\n\t"   // v - (floor(q_i / 2) + 1): negative iff v <= floor(q_i / 2)
                        "v_ashrrev_i32 v125, 31, v127\n\t"
                        "v_bfi_b32 v126, v125, 0, %[dql]\n\t"               // q_j - q_i where v is above the half, 0 otherwise
                        "v_bfi_b32 v127, v125, 0, %[dqh]\n\t"
                        "v_lshl_add_u64 %[r], %[v], 0, v[126:127]"
                        : [r] "=v"(r)
                        : [v] "v"(v), [nqh1] "s"(nqh1), [dql] "s"((u32)dq), [dqh] "s"((u32)(dq >> 32))
                        : "v125", "v126", "v127");
                    return r;
                };
                if (a.s0 == 1) {
                    // two folded slices per limb: the outermost stage (u, v) -> (u + v psi^{N/2}, u - v psi^{N/2}) is one more
                    // butterfly, and this slice keeps its half (kernels_pie.hip fold_store does the same for the other kernels)
                    u64x2 fw;
                    fw.x = dcs->fold_w[lj];
                    fw.y = dcs->fold_w_sh[lj] >> 1;
                    const Tw t = make_tw(fw);
                    u64 y[16];  // the other half of the limb
#pragma unroll
                    for (int r = 0; r < (int)R; r++) {
                        row_get_global<CPT>(x, r, at_bytes(src + 1024 * r, coffb));
                        row_get_global<CPT>(y, r, at_bytes(src + NS + 1024 * r, coffb));
                    }
#pragma unroll
                    for (int k = 0; k < 16; k++) {
                        u64 u0 = lift1(x[k]), v0 = lift1(y[k]);
                        bfly<false, true>(u0, v0, t, mc);
                        x[k] = blk ? v0 : u0;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < (int)R; r++) row_get_global<CPT>(x, r, at_bytes(src + 1024 * r, coffb));
#pragma unroll
                    for (int k = 0; k < 16; k++) x[k] = lift1(x[k]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < (int)R; r++) row_get_global<CPT>(x, r, at_bytes(g + 1024 * r, coffb));
            }
            NTT16_PRIO_F(1);
#pragma unroll
            for (int s = 0; s < (int)LOGR; s++) {
                const int d = (int)(R >> 1) >> s;
#pragma unroll
                for (int r = 0; r < (int)R; r++) {
                    if (r & d) continue;
                    const Tw t = make_tw(NTT16_TWL(1u << s, (u32)r >> (LOGR - s)));
#pragma unroll
                    for (int c = 0; c < (int)CPT; c++) bfly<false, true>(x[CPT * r + c], x[CPT * (r + d) + c], t, mc);
                }
            }
            NTT16_STAMP(1);
            __syncthreads();  // every wave has finished the previous slice's LDS reads
            NTT16_STAMP(2);
#pragma unroll
            for (int r = 0; r < (int)R; r++) row_put<CPT>(x, r, p1 + 1088 * r);
            NTT16_STAMP(3);
            __syncthreads();
            NTT16_STAMP(4);
            // ---- pass 2: e = 1024 w + 64 k + l, stages 3..6 -----------------------------------------------------------------
            NTT16_PRIO_F(2);
#pragma unroll
            for (int k = 0; k < 16; k++) x[k] = p2[68 * k];
#pragma unroll
            for (int sb = 0; sb < 4; sb++) {
                const int d = 8 >> sb;
#pragma unroll
                for (int mm = 0; mm < 8; mm += 2) {
                    const int k0 = bfly_lo(mm, d), k1 = bfly_lo(mm + 1, d);
                    const Tw t0 = make_tw(NTT16_TWL(G::W << sb, (w << sb) + ((u32)k0 >> (4 - sb))));
                    const Tw t1 = make_tw(NTT16_TWL(G::W << sb, (w << sb) + ((u32)k1 >> (4 - sb))));
                    bfly2<false, true>(x[k0], x[k0 + d], t0, x[k1], x[k1 + d], t1, mc);
                }
            }
            // per-lane twiddles from here on, each stage's loaded one stage ahead (the last stages' eight in two halves: with the
            // next slice in flight the register budget is x 32 + y 32 + twiddles <= 48)
            NTT16_LOAD3(t7, 0);
            NTT16_LOAD3(t8, 1);
#pragma unroll
            for (int k = 0; k < 16; k++) p2[68 * k] = x[k];
            NTT16_STAMP(5);
            wave_sync();
            // ---- pass 3: e = 1024 w + 64 a + 4 k + c, stages 7..10 -------------------------------------------------------
            NTT16_PRIO_F(3);
#pragma unroll
            for (int k = 0; k < 16; k++) x[k] = p3[4 * k + 2 * (k >> 3)];
            NTT16_LOAD3(t9, 2);
            NTT16_FENCE();
            {
                const Tw t = make_tw(t7[0]);
#pragma unroll
                for (int k = 0; k < 8; k += 2) bfly2<false, false, true>(x[k], x[k + 8], t, x[k + 1], x[k + 9], t, mc);
            }
            NTT16_LOAD3H(t10, 3, 0);
            NTT16_FENCE();
#pragma unroll
            for (int mm = 0; mm < 8; mm += 2) {
                const int k0 = bfly_lo(mm, 4), k1 = bfly_lo(mm + 1, 4);
                bfly2<false, false, true>(x[k0], x[k0 + 4], make_tw(t8[k0 >> 3]), x[k1], x[k1 + 4], make_tw(t8[k1 >> 3]), mc);
            }
            NTT16_LOAD3H(t10, 3, 4);
            NTT16_FENCE();
#pragma unroll
            for (int mm = 0; mm < 8; mm += 2) {
                const int k0 = bfly_lo(mm, 2), k1 = bfly_lo(mm + 1, 2);
                bfly2<false, false>(x[k0], x[k0 + 2], make_tw(t9[k0 >> 2]), x[k1], x[k1 + 2], make_tw(t9[k1 >> 2]), mc);
            }
            NTT16_LOAD4(t11, 0, 4);
            NTT16_FENCE();
#pragma unroll
            for (int k = 0; k < 16; k += 4)
                bfly2<false, false>(x[k], x[k + 1], make_tw(t10[k >> 1]), x[k + 2], x[k + 3], make_tw(t10[(k >> 1) + 1]), mc);
#pragma unroll
            for (int k = 0; k < 16; k++) p3[4 * k + 2 * (k >> 3)] = x[k];
            NTT16_STAMP(6);
            wave_sync();
            // ---- pass 4: e = 1024 w + 16 l + k, stages 11, 12 ---------------------------------------------------------------
            NTT16_PRIO_F(4);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const u64x2 v = *reinterpret_cast<const u64x2 *>(p4 + 2 * j);
                x[2 * j] = v.x;
                x[2 * j + 1] = v.y;
            }
            NTT16_LOAD4(t12, 4, 4);
            NTT16_FENCE();
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {  // stage 11: both butterflies of a group of four share its twiddle
                const Tw t = make_tw(t11[g4]);
                bfly2<false, false>(x[4 * g4], x[4 * g4 + 2], t, x[4 * g4 + 1], x[4 * g4 + 3], t, mc);
                if (g4 == 1) {
                    NTT16_FENCE();
                    _Pragma("unroll") for (int j_ = 4; j_ < 8; j_++) t12[j_] = *at_bytes(tw4 + 64 * (4 + j_), lb);
                    NTT16_FENCE();
                }
            }
            NTT16_FENCE();
#pragma unroll
            for (int k = 0; k < 16; k += 4)  // stage 12
                bfly2<false, false>(x[k], x[k + 1], make_tw(t12[k >> 1]), x[k + 2], x[k + 3], make_tw(t12[(k >> 1) + 1]), mc);
            NTT16_STAMP(7);
            // ---- lane-ordered store -------------------------------------------------------------------------------------------
            const bool lazy = (a.flags & F_LAZY_OUT) != 0 && !lift;  // the key-switch MAC splits canonical digits into 30-bit halves
            if (!lazy) {
#pragma unroll
                for (int k = 0; k < 16; k++) x[k] = csub_neg(csub_neg(csub_neg(x[k], 0 - q4), 0 - q2), 0 - q);
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                u64x2 v;
                v.x = x[2 * j], v.y = x[2 * j + 1];
                pair_put_global(v, at_bytes(g + 2 * T * j, voffb));
            }
            NTT16_STAMP(8);
        } else {
            // ---- input: 16 contiguous coefficients per thread -------------------------------------------------------------
            NTT16_STAMP(0);
            NTT16_PRIO_I(0);
            NTT16_LOAD4(t12, 4, 4);   // (the other four behind the data loads: the register budget is x 32 + twiddles)
            // operand-0 polynomials of a standard-order launch: their lane-ordered EVALUATION form lives in the Q limbs of the QP
            // operand array -- written there by this launch (copy) or already by stage A (F_X_LANE_IN: read from there)
            const bool is_x = !TENSOR && (a.flags & F_STD_IN) && a.copy_out && (limb / (2 * a.copy_L)) % a.copy_K == 0;
            u64 *co = nullptr;
            if (is_x) {
                const u32 bin = limb / (2 * a.copy_L * a.copy_K), cc = (limb / a.copy_L) & 1, i = limb % a.copy_L;
                co = a.copy_out + (((((size_t)bin * 4 + cc) * a.copy_M + i) << a.s0) + blk) * NS;
                asm("" : "+s"(co));
            }
            const bool x_in = is_x && (a.flags & F_X_LANE_IN);
            if (!TENSOR && (a.flags & F_STD_IN) && !x_in) {
                // Standard order in.  A wave's pass-4' elements are the 1024 contiguous coefficients of its own block: it loads
                // exactly those (coalesced: pair 64 j + l of the block per lane and instruction), drops them into its own region of
                // the image and picks up its 16 contiguous coefficients -- a hand-off inside the wave.  (Until r04 the slice
                // came in as the rows of pass 1 -- columns across all waves -- which took a second workgroup barrier.)
                u64 yv[16];
                const u64 *gw = g + 1024 * w;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const u64x2 v = pair_get_global(at_bytes(gw + 128 * j, lb));
                    yv[2 * j] = v.x, yv[2 * j + 1] = v.y;
                }
                // (the image is free: every wave passed the barrier behind the previous slice's pass-1' reads)
                {
                    // element 1024 w + 128 j + 2 l at phi(.): phi is additive over multiples of 32, 128 j -> 136 j
                    u64 *const pw = lds + phi(1024 * w + 2 * l);
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        u64x2 v;
                        v.x = yv[2 * j], v.y = yv[2 * j + 1];
                        *reinterpret_cast<u64x2 *>(pw + 136 * j) = v;
                    }
                }
                wave_sync();
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const u64x2 v = *reinterpret_cast<const u64x2 *>(p4 + 2 * j);
                    x[2 * j] = v.x;
                    x[2 * j + 1] = v.y;
                }
                if (is_x) {
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        u64x2 v;
                        v.x = x[2 * j], v.y = x[2 * j + 1];
                        pair_put_global(v, at_bytes(co + 2 * T * j, voffb));
                    }
                }
            } else if (TENSOR) {
                const u32 M_ = a.mod_count;
                const size_t ss = ((size_t)M_ << a.s0) * NS;  // one operand polynomial
                const u64 *e0 = a.tsrc + ((((size_t)t_row * 4 * M_ + limb % M_) << a.s0) + blk) * NS;
                const u64 *pa = e0 + (t_d == 2 ? ss : 0), *pb = e0 + (t_d == 0 ? 2 : 3) * ss, *pc = e0 + ss, *pd = e0 + 2 * ss;
                asm("" : "+s"(pa), "+s"(pb), "+s"(pc), "+s"(pd));
                const u64 mu = FD ? 0 : (dcs->mod[mod].r1 << 59) | (dcs->mod[mod].r0 >> 5);  // floor(2^123 / q)
                if (t_d == 1)
                    tensor_load<T, true, FD>(x, pa, pb, pc, pd, voffb, q, mu);
                else
                    tensor_load<T, false, FD>(x, pa, pb, pc, pd, voffb, q, mu);
            } else {
                const u64 *src = x_in ? co : g;
                asm("" : "+s"(src));
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const u64x2 v = pair_get_global(at_bytes(src + 2 * T * j, voffb));
                    x[2 * j] = v.x, x[2 * j + 1] = v.y;
                }
            }
            NTT16_FENCE();
            _Pragma("unroll") for (int j_ = 4; j_ < 8; j_++) t12[j_] = *at_bytes(tw4 + 64 * (4 + j_), lb);
            NTT16_FENCE();
            NTT16_PRIO_I(1);
            // ---- pass 4': stages 12, 11 ----------------------------------------------------------------------------------------
#pragma unroll
            for (int k = 0; k < 16; k += 4) {  // stage 12
                bfly2<true, false>(x[k], x[k + 1], make_tw(t12[k >> 1]), x[k + 2], x[k + 3], make_tw(t12[(k >> 1) + 1]), mc);
                if (k == 4) {   // the first half of this stage's twiddles is dead: the next stage's take their registers
                    NTT16_FENCE();
                    NTT16_LOAD4(t11, 0, 4);
                    NTT16_FENCE();
                }
            }
            NTT16_LOAD3(t10, 3);
            NTT16_FENCE();
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {  // stage 11
                const Tw t = make_tw(t11[g4]);
                bfly2<true, false>(x[4 * g4], x[4 * g4 + 2], t, x[4 * g4 + 1], x[4 * g4 + 3], t, mc);
            }
            NTT16_STAMP(1);
            // (the stores below overwrite the image the other waves read in pass 1' of the previous slice: they are behind the
            // barrier that follows those reads)
            NTT16_STAMP(2);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                u64x2 v;
                v.x = x[2 * j];
                v.y = x[2 * j + 1];
                *reinterpret_cast<u64x2 *>(p4 + 2 * j) = v;
            }
            wave_sync();
            NTT16_STAMP(3);
            // ---- pass 3': stages 10..7 -----------------------------------------------------------------------------------------
            NTT16_PRIO_I(2);
#pragma unroll
            for (int k = 0; k < 16; k++) x[k] = p3[4 * k + 2 * (k >> 3)];
            NTT16_LOAD3(t9, 2);
            NTT16_FENCE();
#pragma unroll
            for (int k = 0; k < 16; k += 4)
                bfly2<true, false>(x[k], x[k + 1], make_tw(t10[k >> 1]), x[k + 2], x[k + 3], make_tw(t10[(k >> 1) + 1]), mc);
            NTT16_LOAD3(t8, 1);
            NTT16_LOAD3(t7, 0);
            NTT16_FENCE();
#pragma unroll
            for (int mm = 0; mm < 8; mm += 2) {
                const int k0 = bfly_lo(mm, 2), k1 = bfly_lo(mm + 1, 2);
                bfly2<true, false>(x[k0], x[k0 + 2], make_tw(t9[k0 >> 2]), x[k1], x[k1 + 2], make_tw(t9[k1 >> 2]), mc);
            }
            NTT16_FENCE();
#pragma unroll
            for (int mm = 0; mm < 8; mm += 2) {
                const int k0 = bfly_lo(mm, 4), k1 = bfly_lo(mm + 1, 4);
                bfly2<true, false>(x[k0], x[k0 + 4], make_tw(t8[k0 >> 3]), x[k1], x[k1 + 4], make_tw(t8[k1 >> 3]), mc);
            }
            {
                const Tw t = make_tw(t7[0]);
#pragma unroll
                for (int k = 0; k < 8; k += 2) bfly2<true, false>(x[k], x[k + 8], t, x[k + 1], x[k + 9], t, mc);
            }
#pragma unroll
            for (int k = 0; k < 16; k++) p3[4 * k + 2 * (k >> 3)] = x[k];
            wave_sync();
            NTT16_STAMP(4);
            // ---- pass 2': stages 6..3 ------------------------------------------------------------------------------------------
            NTT16_PRIO_I(3);
#pragma unroll
            for (int k = 0; k < 16; k++) x[k] = p2[68 * k];
#pragma unroll
            for (int sb = 3; sb >= 0; sb--) {
                const int d = 8 >> sb;
#pragma unroll
                for (int mm = 0; mm < 8; mm += 2) {
                    const int k0 = bfly_lo(mm, d), k1 = bfly_lo(mm + 1, d);
                    const Tw t0 = make_tw(NTT16_TWL(G::W << sb, (w << sb) + ((u32)k0 >> (4 - sb))));
                    const Tw t1 = make_tw(NTT16_TWL(G::W << sb, (w << sb) + ((u32)k1 >> (4 - sb))));
                    bfly2<true, true>(x[k0], x[k0 + d], t0, x[k1], x[k1 + d], t1, mc);
                }
            }
#pragma unroll
            for (int k = 0; k < 16; k++) p2[68 * k] = x[k];
            NTT16_STAMP(5);
            __syncthreads();
            NTT16_STAMP(6);
            // ---- pass 1': the top LOGR stages, stored straight to HBM ------------------------------------------------------------------
            NTT16_PRIO_I(4);
#pragma unroll
            for (int r = 0; r < (int)R; r++) row_get<CPT>(x, r, p1 + 1088 * r);
            // The image is free from here on.  This is where the workgroup waits for "everybody has read it", not in front of the
            // next slice's first stores: the waves come out of the barrier above together and read eight rows each, so nobody
            // waits here -- behind pass 4' of the next slice the older half of the waves stood 9 000 of a slice's 42 000 cycles
            // waiting for the younger half (equal priorities: the arbiter serves the oldest wave first;
            // profiles/r04/ntt16_lab_cycle_stamps_inverse.txt).
            __syncthreads();
#pragma unroll
            for (int s = (int)LOGR - 1; s >= 0; s--) {
                const int d = (int)(R >> 1) >> s;
#pragma unroll
                for (int r = 0; r < (int)R; r++) {
                    if (r & d) continue;
                    const Tw t = make_tw(NTT16_TWL(1u << s, (u32)r >> (LOGR - s)));
#pragma unroll
                    for (int c = 0; c < (int)CPT; c++) bfly<true, true>(x[CPT * r + c], x[CPT * (r + d) + c], t, mc);
                }
            }
            NTT16_STAMP(7);
            const u64 n_inv = dcs->mod[mod].n_inv, n_inv_sh = dcs->mod[mod].n_inv_sh;
            if (!(a.flags & F_FOLDED)) {
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    if (a.s0 == 0)
                        x[k] = csub_neg(mul_shoup_lazy(x[k], n_inv, n_inv_sh, q), 0 - q);
                    else  // split transform: the global-memory stages expect canonical residues
                        x[k] = csub_neg(csub_neg(x[k], 0 - q2), 0 - q);
                }
            }
#pragma unroll
            for (int r = 0; r < (int)R; r++) row_put_global<CPT>(x, r, at_bytes(g + 1024 * r, coffb));
            NTT16_STAMP(8);
        }
    }
