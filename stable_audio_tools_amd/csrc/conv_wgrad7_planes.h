// conv_wgrad7_planes.h — weight gradient of the k = 7 stride-1 (dilated) convs from pre-split bf16 PLANES.  Included by
// conv_wgrad_bf16x3.hip, beside conv_wgrad7_bf16x3_pipe.h (which stays: the fallback and the second implementation).
//
//   dW[co][ci][tap] = sum_b sum_t  dy[b][co][t] * act[b][ci][t + tap*dil - pad]
//
// The pipelined kernel loads fp32 dy / x, re-evaluates SnakeBeta, splits hi / lo and stores to LDS through registers — half of every
// launch (profiles/r06_experiments/wgrad7_ablation/).  Both operands already exist in HBM as the planes of conv1d_planes.h
// ([B][C/8][rows][8 channels], row = 32 + t, zero rows around the sequence): dy for the k7q data-gradient that follows, act as what the
// forward k7q conv read.  Here a stage is LDS-DMA only and the fragments are transposed reads:
//   * tile 128 (co) x 64 (ci) x 7 taps, eight waves (wave w: co rows 32 (w & 3), ci columns 32 (w >> 2)), 7 accumulator tiles per wave,
//     split-K over (b, t) in 64-step stages — the decomposition, slab layout and nsplit rule of the pipelined kernel.
//   * a stage = 16 dy chunk images (64 rows x 16 B) + 8 act chunk images (128 rows: 64 steps + the 6 dil halo, rows from t0 - pad) per
//     plane = 64 lane-linear 1-KiB LDS-DMA pieces, 8 per wave.  No edge path: the planes' zero rows are the padding.
//   * the planes are channel-minor, the MFMA operands time-major (k = time): sat_lds_read_tr16_b64 (ds_read_b64_tr_b16) hands lane
//     (channel c, time half h) steps 8h .. 8h+3 of its channel; two reads per plane and operand.  A tap is a row offset tap * dil * 16 B
//     (an immediate): no v_alignbit, no chunk overrun.  Bank conflicts: a 32-lane half reads 4 rows x 16 B of four consecutive chunk
//     images; images are 64 B apart modulo the 256-B bank row (chunk strides 1088 / 2112 B), so the four land on different quarter rows.
//   * two stages in LDS (134 KiB), one barrier per stage: [vmcnt(0), barrier, issue stage c+1, 128 reads + 84 MFMAs of stage c].
//   * M16: v_mfma_f32_16x16x32_bf16 instead of 32x32x16 (the chip holds a higher clock on that shape: MI355X_MICROARCH.md, DVFS give-back
//     item 7).  A k-step is 32 time steps; lane l holds A[row l & 15][k = 8 (l >> 4) + j], so the 16-lane group l >> 4 is now the k-GROUP
//     (time rows 8 (l >> 4) .. + 7 of the k-step) and the 16-channel block a property of the fragment (+ 2 chunk images, an immediate).
//     Lane 4q + pp of a group still supplies time row q, channel quad pp, and a lane's eight steps are still two reads 64 B apart.  The
//     wave's 32 x 32 x 7 output is 28 tiles of 16 x 16 (the same 112 accumulator registers), hi.hi, lo.hi, hi.lo per tile and k-step: each
//     element sums its products in 32-step instead of 16-step groups, so the result differs from 32x32x16's in the last bits.
//     Banks: a group reads 4 rows x 16 B of two consecutive chunk images = 2 x 64 B, 64 B apart modulo 256 (above): one 128-B half of the
//     bank row.  The 32-lane half's second group reads the k-group 8 rows = 128 B further in the same images: the other half of the bank
//     row.  Conflict-free, like the 32x32x16 map (whose second group is the next 16-channel block: + 2 images = + 128 B modulo 256).
//     A stage is then 128 reads + 168 MFMAs.  Shipped (sat_conv_wgrad7_planes_v: variant 2; 0 = the 32x32x16 form, kept as the A/B arm).
//   * tried on top and not shipped: the next stage's eight pieces issued one by one between the MFMAs instead of in front of the first
//     fragment read — 5-9 % per launch in isolation beside M16, 0.3 ms of the 120 ms step, inside its spread
//     (profiles/wgrad7_planes_variants/README.md).
#pragma once

#define SAT_WQ_NT 512
#define SAT_WQ_NI 64                                         // input channels per workgroup
#define SAT_WQ_LEAD 32                                       // zero rows before t = 0 in a plane (SAT_K7P_LEAD of conv1d_planes.h)
#define SAT_WQ_DY_CH (64 * 16 + 64)                          // bytes between dy chunk images
#define SAT_WQ_ACT_CH (128 * 16 + 64)                        // bytes between act chunk images
#define SAT_WQ_DY_PLANE (16 * SAT_WQ_DY_CH)
#define SAT_WQ_ACT_PLANE (8 * SAT_WQ_ACT_CH)
#define SAT_WQ_ACT_OFF (2 * SAT_WQ_DY_PLANE)
#define SAT_WQ_STAGE (SAT_WQ_ACT_OFF + 2 * SAT_WQ_ACT_PLANE) // 68608

struct SatWgPlParams {
    const short* dy_hi;  // [B][ceil(M/8)][rows_dy][8]
    const short* dy_lo;
    const short* act_hi; // [B][ceil(N/8)][rows_act][8]
    const short* act_lo;
    float* out;          // partial slabs [nsplit][M*N*7] addressed by so_*
    long long so_split, so_m, so_n, so_k;
    int B, M, N, T, pad, rows_dy, rows_act, c8_dy, c8_act;
    int chunks_per_split, nchunks, nT;
};

template <int DIL, bool M16>
__global__ void __launch_bounds__(SAT_WQ_NT) sat_wgrad7_planes_kernel(SatWgPlParams p) {
    static_assert(64 + 6 * DIL <= 128, "a stage's activation rows fit two pieces");
    // ONE LDS object (conv1d_bf16x3_k7q.h)
    __shared__ __attribute__((aligned(1024))) char lds[2 * SAT_WQ_STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = SAT_UNIFORM(tid >> 6);
    int mn_tile, split;
    sat_xcd_tile(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), gridDim.x * gridDim.y, gridDim.z, &mn_tile, &split);
    const int m0 = (mn_tile % (int)gridDim.x) * SAT_CO_T, n0 = (mn_tile / (int)gridDim.x) * SAT_WQ_NI;
    const int m_w = (wave & 3) * 32, n_w = (wave >> 2) * 32;

    // accumulators: 7 tiles of 32 x 32 (acc[tap]), or 28 of 16 x 16 (acc16[tap][co block][ci block]) — 112 registers either way
    f32x16 acc[M16 ? 1 : 7];
    f32x4 acc16[M16 ? 7 : 1][2][2];
    if constexpr (M16) {
#pragma unroll
        for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc16[k][t >> 1][t & 1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    } else {
#pragma unroll
        for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[k][r] = 0.0f;
    }

    const int c_begin = split * p.chunks_per_split;
    int c_end = c_begin + p.chunks_per_split;
    if (c_end > p.nchunks) c_end = p.nchunks;
    const int nst = c_end - c_begin;                                 // stages of this workgroup (>= 1)

    // ---- LDS-DMA of a stage: wave w issues dy pieces w, w + 8, w + 16, w + 24 of [plane][16 chunks] and act pieces of the same
    //      numbers of [plane][8 chunks][2 x 64 rows]; every source is a wave-uniform base + lane * 16 bytes ----
    const unsigned lane8 = (unsigned)lane * 8u;                      // (shorts)
    auto issue = [&](int c, int st) {
        const int ch = c_begin + c;
        const int b = ch / p.nT;
        const int tt0 = (ch - b * p.nT) * SAT_WB_TT;
        char* sb = lds + st * SAT_WQ_STAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = wave + 8 * i, pl = d >> 4, g = d & 15;
            int c8 = (m0 >> 3) + g;
            c8 = c8 < p.c8_dy ? c8 : p.c8_dy - 1;                    // rows past M: any finite data (never stored)
            const short* src = (pl ? p.dy_lo : p.dy_hi) + (((size_t)b * p.c8_dy + c8) * p.rows_dy + SAT_WQ_LEAD + tt0) * 8;
            sat_glds16_raw(src + lane8, sb + pl * SAT_WQ_DY_PLANE + g * SAT_WQ_DY_CH);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int a = wave + 8 * i, pl = a >> 4, g = (a >> 1) & 7, part = a & 1;
            int c8 = (n0 >> 3) + g;
            c8 = c8 < p.c8_act ? c8 : p.c8_act - 1;
            const short* src = (pl ? p.act_lo : p.act_hi) +
                               (((size_t)b * p.c8_act + c8) * p.rows_act + SAT_WQ_LEAD + tt0 - p.pad + part * 64) * 8;
            sat_glds16_raw(src + lane8, sb + SAT_WQ_ACT_OFF + pl * SAT_WQ_ACT_PLANE + g * SAT_WQ_ACT_CH + part * 1024);
        }
    };

    // ---- fragment addresses: lane 4q + pp of the 16-lane group gq = lane >> 4 supplies row (time) q, channels 4pp .. 4pp+3 = chunk (pp >> 1),
    //      bytes 8 (pp & 1).  32x32x16: the group reads the 16-channel block (gq & 1) of the wave's 32 channels at time half gq >> 1 of the
    //      16-step k-step.  16x16x32: the group reads time rows 8 gq .. 8 gq + 7 of the 32-step k-step; the channel block comes from the caller ----
    const int gq = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const unsigned row_off = (unsigned)((8 * (M16 ? gq : gq >> 1) + q) * 16 + 8 * (pp & 1));
    const unsigned a_off = (unsigned)(((m_w >> 3) + (M16 ? 0 : 2 * (gq & 1)) + (pp >> 1)) * SAT_WQ_DY_CH) + row_off;
    const unsigned b_off = (unsigned)(SAT_WQ_ACT_OFF + ((n_w >> 3) + (M16 ? 0 : 2 * (gq & 1)) + (pp >> 1)) * SAT_WQ_ACT_CH) + row_off;
    auto frag = [&](const char* at) {                               // steps 0..3 and 4..7 of this lane's eight time steps
        const bf16x4 v0 = sat_lds_read_tr16_b64(at), v1 = sat_lds_read_tr16_b64(at + 64);
        return bf16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    };
    auto compute = [&](int st) {
        const char* pa = lds + st * SAT_WQ_STAGE + a_off;
        const char* pb = lds + st * SAT_WQ_STAGE + b_off;
        SAT_MFMA_PRIO(1);
        if constexpr (M16) {
#pragma unroll
            for (int ks = 0; ks < SAT_WB_TT / 32; ++ks) {
                bf16x8 a_hi[2], a_lo[2];
#pragma unroll
                for (int ab = 0; ab < 2; ++ab) {
                    a_hi[ab] = frag(pa + ks * 512 + ab * 2 * SAT_WQ_DY_CH);
                    a_lo[ab] = frag(pa + SAT_WQ_DY_PLANE + ks * 512 + ab * 2 * SAT_WQ_DY_CH);
                }
#pragma unroll
                for (int k = 0; k < 7; ++k)
#pragma unroll
                    for (int bb = 0; bb < 2; ++bb) {
                        const char* at = pb + ks * 512 + k * DIL * 16 + bb * 2 * SAT_WQ_ACT_CH;
                        const bf16x8 b_hi = frag(at), b_lo = frag(at + SAT_WQ_ACT_PLANE);
#pragma unroll
                        for (int ab = 0; ab < 2; ++ab) {
                            acc16[k][ab][bb] = sat_mfma_16x16x32_bf16(a_hi[ab], b_hi, acc16[k][ab][bb]);
                            acc16[k][ab][bb] = sat_mfma_16x16x32_bf16(a_lo[ab], b_hi, acc16[k][ab][bb]);
                            acc16[k][ab][bb] = sat_mfma_16x16x32_bf16(a_hi[ab], b_lo, acc16[k][ab][bb]);
                        }
                    }
                SAT_SCHED_FENCE();                                   // without it hipcc hoists the next k-step's reads until registers spill (dilation 9)
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < SAT_WB_TT / 16; ++ks) {
                const bf16x8 a_hi = frag(pa + ks * 256), a_lo = frag(pa + SAT_WQ_DY_PLANE + ks * 256);
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    const bf16x8 b_hi = frag(pb + ks * 256 + k * DIL * 16), b_lo = frag(pb + SAT_WQ_ACT_PLANE + ks * 256 + k * DIL * 16);
                    acc[k] = sat_mfma_32x32x16_bf16(a_hi, b_hi, acc[k]);
                    acc[k] = sat_mfma_32x32x16_bf16(a_lo, b_hi, acc[k]);
                    acc[k] = sat_mfma_32x32x16_bf16(a_hi, b_lo, acc[k]);
                }
            }
        }
        SAT_MFMA_PRIO(0);
    };

    issue(0, 0);
    for (int c = 0; c < nst; ++c) {
        SAT_WAIT_VMCNT(0);                                           // this wave's pieces of stage c have landed ...
        SAT_RAW_BARRIER();                                           // ... and everybody's; every wave is done reading stage c - 1
        SAT_SCHED_FENCE();
        if (c + 1 < nst) issue(c + 1, (c + 1) & 1);                  // (block-uniform) into the buffer stage c - 1 has left
        compute(c & 1);
    }

    if (m0 + m_w < p.M) {
        float* ob = p.out + (size_t)split * p.so_split;
        if constexpr (M16) {                                         // C/D of 16x16x32: row 4 (lane >> 4) + reg, column lane & 15
#pragma unroll
            for (int k = 0; k < 7; ++k)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int m = m0 + m_w + 16 * (t >> 1) + 4 * gq + r, n = n0 + n_w + 16 * (t & 1) + (lane & 15);
                        if (m < p.M && n < p.N) ob[(size_t)m * p.so_m + (size_t)n * p.so_n + (size_t)k * p.so_k] = acc16[k][t >> 1][t & 1][r];
                    }
        } else {
            const int n = n0 + n_w + (lane & 31);
#pragma unroll
            for (int k = 0; k < 7; ++k)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + m_w + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (m < p.M && n < p.N) ob[(size_t)m * p.so_m + (size_t)n * p.so_n + (size_t)k * p.so_k] = acc[k][r];
                }
        }
    }
}
