// attention_hd128.h — the INFERENCE half of attention at head dim 128 (Stable Audio Open Small style DiTs): plane preparation and the
// flash-style forward, fp32 (two bf16 planes, three MFMAs per product) and bf16.  Included by attention.hip, whose helpers (staging,
// fragments, packing, buffer loads, the deferred-max constants) it shares; the head dim 64 kernels there are not touched.  There is no
// backward at head dim 128: sat_attention_bwd refuses it (the two-plane dK / dV tile already needs TQ = 32 to fit LDS at D = 64).
//
// The forward is sat_attn_fwd_kernel<T, NP> with the head dim doubled: one wave owns 32 queries, 64-key tiles go through LDS, the
// products are swapped (S^T = K Q^T, O^T += V^T P^T) so that a softmax row is lane-local, the scores leave the matrix pipe in the exp2
// domain with the running max entering through the C operand, and the rescale is deferred (SAT_ATT_DEFER / SAT_ATT_SUMLIM).  What D
// changes: eight 16-wide k-steps for Q (qf[8][NP]), four 32-row blocks of O^T (oacc[4]: 64 accumulator registers), a K tile of
// [64][128 + 8] and a V^T tile of [128][64 + 8] per plane and buffer — 35 840 B.  Per 64-key tile a wave issues 32 MFMAs (x3 in the
// two-plane mode) for the same 64 x 32 scores' worth of softmax as D = 64 does for 16.
//
// LDS / occupancy, as chosen:
//   NP = 1 (bf16):  double-buffered, 71 680 B per workgroup, 256 registers per lane (amdgpu_waves_per_eu(2)): two waves per SIMD, which
//                   the softmax of one wave needs to run under the MFMAs of another.  Two shapes: NW = 4 waves per workgroup (128
//                   queries; two workgroups share a CU when the grid is that large) and NW = 8 (256 queries: the two waves of a SIMD
//                   belong to ONE workgroup and share its K / V^T tiles, half the staging per MFMA) — sat_attention_fwd picks 8 when
//                   256-query workgroups still give every CU one.
//   NP = 2 (fp32):  NW = 4, double-buffered as well, 143 360 B (inside the 160 KB gemm.hip relies on): ONE workgroup per CU, one wave per SIMD,
//                   with the whole 512-register file for qf (64) + oacc (64) + scores (32) + the tile in flight (64).  Single-buffering
//                   would allow two workgroups per CU only below 256 registers, which this instantiation cannot meet without spilling,
//                   and a single-buffered lone workgroup would expose every tile's global-load latency; this is the 1e-3 parity mode,
//                   so it keeps the simple pipeline of the D = 64 kernel instead.
#pragma once

#define SAT_ATT_D2 128
#define SAT_ATT_KROW2 (SAT_ATT_D2 + 8)      // bf16 per LDS row of the K tile: 272 B stride, conflict-free ds_read_b128

// ---------------------------------------------------------------------------------------------
// prepare: strided (b,h,n,128) -> bf16 planes, the contract of sat_attn_prepare_kernel
// ---------------------------------------------------------------------------------------------
// One 64 (n) x 128 (d) tile per workgroup; a thread converts 8 consecutive d of one row (16-byte loads where the strides allow, 16-byte
// plane stores), the transposed planes go through an LDS tile and are written 8 consecutive n at a time.
template <typename T>
__global__ void __launch_bounds__(256) sat_attn_prepare128_kernel(SatPrepParams p) {
    __shared__ __attribute__((aligned(16))) short t_hi[SAT_ATT_T][SAT_ATT_KROW2];   // [n][d]
    __shared__ __attribute__((aligned(16))) short t_lo[SAT_ATT_T][SAT_ATT_KROW2];
    constexpr int PARTS = SAT_ATT_D2 / 8;
    const int n0 = blockIdx.x * SAT_ATT_T, h = blockIdx.y, b = blockIdx.z;
    const long long base = (long long)b * p.sb + (long long)h * p.sh;
    const size_t plane = ((size_t)b * p.H + h) * (size_t)p.Np * SAT_ATT_D2;
    const bool want_tr = p.tr_hi != nullptr || p.tr_lo != nullptr;
    const bool vec_src = ((p.sn & 7) == 0) && ((p.sb & 7) == 0) && ((p.sh & 7) == 0) &&
                         (((uintptr_t)p.src & 15) == 0);                              // 16-byte loads allowed
    for (int i = threadIdx.x; i < SAT_ATT_T * PARTS; i += 256) {
        const int r = i / PARTS, d0 = (i % PARTS) * 8;
        const int n = n0 + r;                                                         // < Np: the grid covers Np / 64 tiles
        float x[8];
        if (n < p.N) {
            const long long off = base + (long long)n * p.sn + d0;
            if (vec_src) {
                if (sizeof(T) == 2) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>((const short*)p.src + off);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        x[2 * j] = __builtin_bit_cast(float, v[j] << 16);
                        x[2 * j + 1] = __builtin_bit_cast(float, v[j] & 0xffff0000u);
                    }
                } else {
                    const f32x4 v0 = *reinterpret_cast<const f32x4*>((const float*)p.src + off);
                    const f32x4 v1 = *reinterpret_cast<const f32x4*>((const float*)p.src + off + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { x[j] = v0[j]; x[4 + j] = v1[j]; }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = SatSrc<T>::at(p.src, off + j);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = 0.0f;
        }
        uint32_t wh[4], wl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) sat_split2_pk(x[2 * j], x[2 * j + 1], &wh[j], &wl[j]);
        const u32x4 vh{wh[0], wh[1], wh[2], wh[3]}, vl{wl[0], wl[1], wl[2], wl[3]};
        const size_t o = plane + (size_t)n * SAT_ATT_D2 + d0;
        if (p.rm_hi) *reinterpret_cast<u32x4*>(p.rm_hi + o) = vh;
        if (p.rm_lo) *reinterpret_cast<u32x4*>(p.rm_lo + o) = vl;
        if (want_tr) {
            *reinterpret_cast<u32x4*>(&t_hi[r][d0]) = vh;
            *reinterpret_cast<u32x4*>(&t_lo[r][d0]) = vl;
        }
    }
    if (!want_tr) return;   // block-uniform
    __syncthreads();
    for (int i = threadIdx.x; i < SAT_ATT_D2 * (SAT_ATT_T / 8); i += 256) {
        const int d = i >> 3, r0 = (i & 7) * 8;
        bf16x8 vh, vl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            vh[j] = t_hi[r0 + j][d];
            vl[j] = t_lo[r0 + j][d];
        }
        const size_t o = plane + (size_t)d * p.Np + n0 + r0;
        if (p.tr_hi) *reinterpret_cast<bf16x8*>(p.tr_hi + o) = vh;
        if (p.tr_lo) *reinterpret_cast<bf16x8*>(p.tr_lo + o) = vl;
    }
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
// one 64-key tile (NKB = 2) or its first 32 keys (NKB = 1) — sat_attn_fwd_tile with 8 k-steps in QK^T and 4 row blocks in P V
template <int NP, int NKB, bool MASK, bool FIRST, bool DOT2>
SAT_DEVICE void sat_attn_fwd128_tile(short (*k_lds)[SAT_ATT_T][SAT_ATT_KROW2], short (*v_lds)[SAT_ATT_D2][SAT_ATT_ROW], const bf16x8 (&qf)[8][NP],
                                     f32x16 (&oacc)[4], f32x16& negm, float& mb, float& l_run, int l31, int hi, int kperm, int nvalid) {
    f32x16 sacc[NKB];
    auto qk = [&]() {
        SAT_SETPRIO(1);
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            if (FIRST) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[kb][r] = 0.0f;
            }
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                bf16x8 ka[NP];
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) ka[pl] = sat_att_frag_rm(k_lds[pl], kb * 32 + kperm, 16 * s + 8 * hi);
                sacc[kb] = sat_att_mma<NP>(ka, qf[s], (!FIRST && s == 0) ? negm : sacc[kb]);      // -mb enters through the C operand
            }
        }
        SAT_SETPRIO(0);
    };
    auto rowmax = [&]() {
        float tmax = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kb * 32 + (r & 7) + 8 * hi + 16 * (r >> 3);
                if (!MASK || key < nvalid) tmax = fmaxf(tmax, sacc[kb][r]);      // only the last tile holds padded keys (block-uniform)
            }
        return sat_att_halfmax(tmax);
    };
    static_assert(!DOT2 || NP == 1, "the packed row sum needs single-plane (bf16) probabilities");
    float ps0 = 0.0f, ps1 = 0.0f;
    bf16x8 pbs[DOT2 ? NKB : 1][2];      // DOT2: the tile's packed probabilities (the B operands of the P V MFMAs)
    auto expsum = [&]() {
        ps0 = 0.0f;
        ps1 = 0.0f;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float a = sat_exp2(sacc[kb][2 * j]), c = sat_exp2(sacc[kb][2 * j + 1]);
                if (MASK) {
                    const int key = kb * 32 + ((2 * j) & 7) + 8 * hi + 16 * ((2 * j) >> 3);
                    if (key >= nvalid) a = 0.0f;
                    if (key + 1 >= nvalid) c = 0.0f;
                }
                if (!DOT2) {
                    ps0 += a;
                    ps1 += c;
                }
                sacc[kb][2 * j] = a;
                sacc[kb][2 * j + 1] = c;
            }
        if (DOT2) {
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    bf16x8 one[NP];
                    sat_att_pack<NP>(sacc[kb], u, one);
                    pbs[DOT2 ? kb : 0][u] = one[0];
                    const u32x4 w = __builtin_bit_cast(u32x4, one[0]);
                    ps0 = sat_att_sum2(w[0], ps0);
                    ps1 = sat_att_sum2(w[1], ps1);
                    ps0 = sat_att_sum2(w[2], ps0);
                    ps1 = sat_att_sum2(w[3], ps1);
                }
        }
    };
    qk();
    if (FIRST) {
        const float tmax = rowmax();
        mb = tmax;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[kb][r] -= tmax;
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[r] = -mb;
    }
    expsum();
    if (!FIRST) {
        if (sat_wave_any(!(ps0 + ps1 <= SAT_ATT_SUMLIM))) {      // stale running max in some row of the wave (rare): redo with the true one
            qk();
            const float d = fmaxf(rowmax(), 0.0f), alpha = sat_exp2(-d);
            mb += d;
            l_run *= alpha;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[kb][r] -= d;
#pragma unroll
            for (int r = 0; r < 16; ++r) negm[r] = -mb;
            expsum();
        }
    }
    l_run += ps0 + ps1;
    SAT_SETPRIO(1);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            bf16x8 pb[NP];
            if (DOT2) pb[0] = pbs[DOT2 ? kb : 0][u];
            else sat_att_pack<NP>(sacc[kb], u, pb);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                bf16x8 va[NP];
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) va[pl] = sat_att_frag_rm(v_lds[pl], t * 32 + l31, kb * 32 + 16 * u + 8 * hi);
                oacc[t] = sat_att_mma<NP>(va, pb, oacc[t]);
            }
        }
    SAT_SETPRIO(0);
}

template <typename T, int NP, int NW>
__global__ void __launch_bounds__(64 * NW)
#if !defined(SAT_HIPEMU)
__attribute__((amdgpu_waves_per_eu(NP == 1 ? 2 : 1)))      // registers for two (bf16) / one (fp32) waves per SIMD: the LDS bound above
#endif
sat_attn_fwd128_kernel(SatAttnParams p) {
    constexpr int THREADS = 64 * NW, QWG = 32 * NW;      // NW waves of 32 queries each
    constexpr int PIECES = 1024 / THREADS;               // 16-byte pieces of a K / V^T tile per thread and plane
    // K / V^T tiles double-buffered in LDS; tile k+1 travels through registers while tile k is consumed: one barrier per tile
    __shared__ __attribute__((aligned(16))) short k_lds2[2][NP][SAT_ATT_T][SAT_ATT_KROW2];   // [buffer][plane][key][d]
    __shared__ __attribute__((aligned(16))) short v_lds2[2][NP][SAT_ATT_D2][SAT_ATT_ROW];    // [buffer][plane][d][key]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int kperm = sat_att_kperm(l31);
    const int b = blockIdx.z, h = blockIdx.y;
    const int hk = h / (p.H / p.Hkv);
    const int qrow = blockIdx.x * QWG + wave * 32 + l31;     // < Nqp when q_in: Nqp is a multiple of 64, the grid covers Nq in steps of QWG
    const bool q_in = qrow < p.Nqp;
    const bool q_ok = qrow < p.Nq;
    const bool w_ok = blockIdx.x * QWG + wave * 32 < p.Nq;   // wave-uniform: this wave owns a valid query
    const size_t qplane = ((size_t)b * p.H + h) * (size_t)p.Nqp * SAT_ATT_D2;
    const size_t kplane = ((size_t)b * p.Hkv + hk) * (size_t)p.Nkp * SAT_ATT_D2;
    const float sl2 = p.scale * 1.4426950408889634f;

    bf16x8 qf[8][NP];   // B operand of x = K (Q c)^T: lane (q = l31, hi) holds d = 16 s + 8 hi + e, pre-scaled by c = scale * log2(e)
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        u32x4 w[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
            if (q_in) w[pl] = *reinterpret_cast<const u32x4*>(p.q_rm[pl] + qplane + (size_t)qrow * SAT_ATT_D2 + 16 * s + 8 * hi);
            else w[pl] = u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {       // two bf16 per word: element 2j in the low half
            float e0 = __builtin_bit_cast(float, w[0][j] << 16), e1 = __builtin_bit_cast(float, w[0][j] & 0xffff0000u);
            if (NP == 2) {
                e0 += __builtin_bit_cast(float, w[NP - 1][j] << 16);
                e1 += __builtin_bit_cast(float, w[NP - 1][j] & 0xffff0000u);
                uint32_t wh, wl;
                sat_split2_pk(e0 * sl2, e1 * sl2, &wh, &wl);
                w[0][j] = wh;
                w[NP - 1][j] = wl;
            } else {
                w[0][j] = sat_cvt2_pk(e0 * sl2, e1 * sl2);
            }
        }
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) qf[s][pl] = __builtin_bit_cast(bf16x8, w[pl]);
    }

    f32x16 oacc[4], negm;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int t = 0; t < 4; ++t) oacc[t][r] = 0.0f;
        negm[r] = 0.0f;
    }
    float mb = 0.0f, l_run = 0.0f;      // running row max (exp2 domain) and row sum

    // K tile 64 x 128 and V^T tile 128 x 64 bf16 = 1024 16-byte pieces each = PIECES per thread and plane: LDS (row, part) and the byte
    // offsets from the tile's uniform base
    int krow[PIECES], kpart[PIECES], vrow[PIECES], vpart[PIECES];
    unsigned kob[PIECES], vob[PIECES];
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
        const int c = threadIdx.x + j * THREADS;
        krow[j] = c >> 4;       // < 64
        kpart[j] = c & 15;
        vrow[j] = c >> 3;       // < 128
        vpart[j] = c & 7;
        kob[j] = (unsigned)(krow[j] * SAT_ATT_D2 + kpart[j] * 8) * 2u;
        vob[j] = ((unsigned)vrow[j] * (unsigned)p.Nkp + (unsigned)vpart[j] * 8u) * 2u;      // < 128 * Nkp * 2 bytes: Nkp < 2^23 (sat_attention_fwd)
    }
    const SatBuf kbuf0 = sat_buf_make(p.k_rm[0] + kplane), vbuf0 = sat_buf_make(p.v_tr[0] + kplane);
    const SatBuf kbuf1 = sat_buf_make(p.k_rm[NP - 1] + kplane), vbuf1 = sat_buf_make(p.v_tr[NP - 1] + kplane);
    bf16x8 kreg[NP][PIECES], vreg[NP][PIECES];
    auto tile_load = [&](int k0) {      // k0 + 64 <= Nkp: every 16-byte piece lies inside this (batch item, kv head)'s planes
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
#pragma unroll
            for (int j = 0; j < PIECES; ++j) {
                kreg[pl][j] = sat_buf_load16(pl == 0 ? kbuf0 : kbuf1, kob[j], (unsigned)k0 * (SAT_ATT_D2 * 2));
                vreg[pl][j] = sat_buf_load16(pl == 0 ? vbuf0 : vbuf1, vob[j], (unsigned)k0 * 2u);
            }
    };
    auto tile_store = [&](int buf) {
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
#pragma unroll
            for (int j = 0; j < PIECES; ++j) {
                *reinterpret_cast<bf16x8*>(&k_lds2[buf][pl][krow[j]][kpart[j] * 8]) = kreg[pl][j];
                *reinterpret_cast<bf16x8*>(&v_lds2[buf][pl][vrow[j]][vpart[j] * 8]) = vreg[pl][j];
            }
    };
    tile_load(0);
    tile_store(0);
    if (SAT_ATT_T < p.Nk) tile_load(SAT_ATT_T);
    __syncthreads();
    int buf = 0, k0 = 0;
    if (p.Nk >= SAT_ATT_T) {      // the first full tile, peeled: it establishes the running max
        if (SAT_ATT_T < p.Nk) {
            tile_store(1);
            if (2 * SAT_ATT_T < p.Nk) tile_load(2 * SAT_ATT_T);
        }
        if (w_ok) sat_attn_fwd128_tile<NP, 2, false, true, NP == 1>(k_lds2[0], v_lds2[0], qf, oacc, negm, mb, l_run, l31, hi, kperm, SAT_ATT_T);
        __syncthreads();
        k0 = SAT_ATT_T;
        buf = 1;
    }
    // full tiles: ONE straight-line body, so that the accumulators keep their registers around the loop; the ragged last tile is peeled
    for (; k0 + SAT_ATT_T <= p.Nk; k0 += SAT_ATT_T, buf ^= 1) {
        if (k0 + SAT_ATT_T < p.Nk) {
            tile_store(buf ^ 1);                                         // tile k+1: registers -> the other buffer
            if (k0 + 2 * SAT_ATT_T < p.Nk) tile_load(k0 + 2 * SAT_ATT_T);   // tile k+2 -> registers (lands during this tile's math)
        }
        if (w_ok) sat_attn_fwd128_tile<NP, 2, false, false, NP == 1>(k_lds2[buf], v_lds2[buf], qf, oacc, negm, mb, l_run, l31, hi, kperm, SAT_ATT_T);
        __syncthreads();
    }
    if (k0 < p.Nk && w_ok) {
        const int rem = p.Nk - k0;
        if (k0 == 0) {            // fewer than 64 keys in all: the ragged tile is also the first
            if (rem > 32) sat_attn_fwd128_tile<NP, 2, true, true, NP == 1>(k_lds2[buf], v_lds2[buf], qf, oacc, negm, mb, l_run, l31, hi, kperm, rem);
            else sat_attn_fwd128_tile<NP, 1, true, true, NP == 1>(k_lds2[buf], v_lds2[buf], qf, oacc, negm, mb, l_run, l31, hi, kperm, rem);
        } else if (rem > 32) {
            sat_attn_fwd128_tile<NP, 2, true, false, NP == 1>(k_lds2[buf], v_lds2[buf], qf, oacc, negm, mb, l_run, l31, hi, kperm, rem);
        } else {
            sat_attn_fwd128_tile<NP, 1, true, false, NP == 1>(k_lds2[buf], v_lds2[buf], qf, oacc, negm, mb, l_run, l31, hi, kperm, rem);
        }
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv_l = 1.0f / l_tot;
    if (q_ok) {
        // lane (q, hi) holds d = 32 t + 8 g + 4 hi + {0..3} in registers 4 g + {0..3}: 8-byte (bf16) / 16-byte (fp32) stores
        const long long obase = ((long long)b * p.Nq + qrow) * ((long long)p.H * SAT_ATT_D2) + (long long)h * SAT_ATT_D2;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 v = {oacc[t][4 * g] * inv_l, oacc[t][4 * g + 1] * inv_l, oacc[t][4 * g + 2] * inv_l, oacc[t][4 * g + 3] * inv_l};
                const long long idx = obase + t * 32 + 8 * g + 4 * hi;
                if (sizeof(T) == 4) *(f32x4*)((float*)p.o + idx) = v;
                else *(u32x2*)((short*)p.o + idx) = u32x2{sat_cvt2_pk(v[0], v[1]), sat_cvt2_pk(v[2], v[3])};
            }
        // natural-log LSE of the scaled scores: (mb + log2 l) ln 2   (mb lives in the exp2 domain)
        if (p.lse && hi == 0) p.lse[((long long)b * p.H + h) * p.Nq + qrow] = (mb + log2f(l_tot)) * 0.6931471805599453f;
    }
}
