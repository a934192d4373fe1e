// conv_epilogue.h — the output epilogue of the three bf16x3 matrix conv kernels (conv1d_bf16x3.hip: generic; conv1d_bf16x3_k7.h: direct;
// conv1d_bf16x3_k7q.h: planes), one copy.  Included by conv1d_bf16x3.hip (SAT_K7P_LEAD_ROWS, conv_common.h).  Every kernel hands over its
// 2 x 2 32x32 accumulators per wave (a wave owns 64 output channels x 64 time steps of a 128-channel tile, TW waves along time), its per-channel
// table ep_lds (rows: bias | e^alpha2 | e^beta2 | emission a | emission 1/b) and red_lds, the per-wave-column sums of a data-gradient.
#pragma once

// What the epilogue reads of a launch and the tile's place in it, BY VALUE: scalars read through a pointer to the whole launch inside the
// unrolled row loops were spilled and re-read per row.  Plain output addressing only: `cout` is Cout = the virtual channel count.
struct SatConvEpArgs {
    float* y;                      // output (B, cout, Tout)
    const float* res;              // residual, same shape (null: none)
    const float* x2;               // dsnake input, same shape (null: not a data-gradient)
    float* part_da;                // data-gradient: [cout][B * t_tiles] partial sums of d log-alpha2 / d log-beta2
    float* part_db;
    short* em_hi;                  // plane emission (null: none): [B][em_c8][em_rows][8] bf16
    short* em_lo;
    bool em_act;                   // the planes hold snake(y) with ep_lds rows 3 / 4 (false: y itself)
    int em_c8, em_rows;
    int B, cout, Tout;
    bool tanh_out;
    int b, co0, t0, t_tile, t_tiles;   // batch item, first channel, first time step, time tile and their count
};
// `ea` points to the launch (SatConvBfLaunch) in whatever address space the kernel reads it from
template <class Launch>
SAT_DEVICE SatConvEpArgs sat_conv_ep_args(Launch ea, float* y, const float* res, bool emit, int b, int co0, int t0, int t_tile, int t_tiles) {
    return SatConvEpArgs{y, res, ea->p.x2, ea->p.part_da, ea->p.part_db, emit ? ea->em_hi : nullptr, emit ? ea->em_lo : nullptr,
                         ea->em_a != nullptr, ea->em_c8, ea->em_rows, ea->p.B, ea->cout_v, ea->p.Tout, ea->p.tanh_out != 0,
                         b, co0, t0, t_tile, t_tiles};
}

// One output element: bias, then (data-gradients) the SnakeBeta derivative at x2, then the residual, then tanh.  The element's terms of the
// d log-alpha2 / d log-beta2 sums are ACCUMULATED into pda / pdb inside the branch (a returned term would reach its sum through a phi and
// lose the fused multiply-add every site had).
SAT_DEVICE float sat_conv_finish(float acc, float bias, bool bwd, float x2, float a2, float b2, float res, bool tanh_out, float& pda, float& pdb) {
    float v = acc + bias;
    if (bwd) {
        const SatSnakeGrad g = sat_snake_grad(x2, a2, b2);
        pda += v * g.dla;
        pdb += v * g.dlb;
        v *= g.dx;
    }
    v += res;
    if (tanh_out) v = tanhf(v);
    return v;
}

// 16-byte epilogue (plain output addressing, Tout % 4 == 0, 16-byte aligned tensors): each wave transposes its accumulators through its
// 32 x 68 LDS tile (memory the K loop is done with) so that a lane owns 4 consecutive time steps of a row; the x2 / res loads of a 32-row
// half are all issued before use.  em_hi / em_lo (null: none): plane EMISSION — act(y) as the bf16 hi / lo planes the next k7 conv reads.
// A tile fully inside the tensor takes its loads without per-row range checks.
template <int TW>
SAT_DEVICE void sat_conv_epilogue16(const SatConvEpArgs& ta, f32x16 (&acc)[2][2], float (*tile)[68], float (*red_lds)[TW][SAT_CO_T],
                                    float (*ep_lds)[SAT_CO_T], int lane, int wave) {
    const bool bwd = ta.x2 != nullptr;
    const int b = ta.b, co0 = ta.co0, t0 = ta.t0;
    const int l31 = lane & 31, hi = lane >> 5;
    const int co_w = (wave / TW) * 64, t_w = (wave % TW) * 64;
    const bool wave_on = (co0 + co_w) < ta.cout;
    const bool mi1_on = (co0 + co_w + 32) < ta.cout;
    if (!bwd) __syncthreads();                          // the K loop's memory is free (bwd: synchronised when red_lds was cleared)
    const int lr = lane >> 4, t4 = (lane & 15) * 4;    // this lane's row within a group of 4, its 4 time steps
    // (this lane's first cell as accumulator owner and as row owner: every other one is a compile-time offset from it, not an address register each)
    float* const t_acc = &tile[4 * hi][l31];
    float* const t_row = &tile[lr][t4];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const bool half_on = wave_on && (mi == 0 || mi1_on);
        if (mi == 1) __syncthreads();                   // every wave is done reading its first half
        if (half_on) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) t_acc[((r & 3) + 8 * (r >> 2)) * 68 + ni * 32] = acc[mi][ni][r];
        }
        __syncthreads();                                // (a wave only reads its own tile: this orders its own lanes)
        if (half_on) {
            const int tg = t0 + t_w + t4;
            f32x4 xv[8], rv[8];
            if (co0 + SAT_CO_T <= ta.cout && t0 + TW * 64 <= ta.Tout) {
                // (block-uniform) the loads go out back to back, none wrapped in its own branch
                const size_t o0 = ((size_t)b * ta.cout + co0 + co_w + mi * 32 + lr) * ta.Tout + tg;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    xv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    rv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (bwd) xv[j] = *reinterpret_cast<const f32x4*>(ta.x2 + o0 + (size_t)(j * 4) * ta.Tout);
                    if (ta.res) rv[j] = *reinterpret_cast<const f32x4*>(ta.res + o0 + (size_t)(j * 4) * ta.Tout);
                }
            } else
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int co = co0 + co_w + mi * 32 + j * 4 + lr;
                const bool ok = co < ta.cout && tg < ta.Tout;
                const size_t o = ((size_t)b * ta.cout + (ok ? co : 0)) * ta.Tout + (ok ? tg : 0);
                xv[j] = (bwd && ok) ? *reinterpret_cast<const f32x4*>(ta.x2 + o) : f32x4{0.f, 0.f, 0.f, 0.f};
                rv[j] = (ta.res && ok) ? *reinterpret_cast<const f32x4*>(ta.res + o) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int row = j * 4 + lr;
                const int col = co_w + mi * 32 + row;
                const int co = co0 + col;
                const bool ok = co < ta.cout && tg < ta.Tout;
                const f32x4 av = *reinterpret_cast<const f32x4*>(t_row + j * 4 * 68);
                const float bias = ep_lds[0][col];
                const float a2 = ep_lds[1][col], b2 = ep_lds[2][col];
                float pda = 0.f, pdb = 0.f;
                f32x4 ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) ov[e] = sat_conv_finish(av[e], bias, bwd, xv[j][e], a2, b2, rv[j][e], ta.tanh_out, pda, pdb);
                if (ok) *reinterpret_cast<f32x4*>(ta.y + ((size_t)b * ta.cout + co) * ta.Tout + tg) = ov;
                if (ta.em_hi) {
                    // emission, step 1: the consumer's activation of the finished values (em_a null: the values themselves, for a data-gradient
                    // consumer) goes back into this lane's own cell of the transposition tile (rows past Cout hold act(0) = 0)
                    f32x4 ev = ov;
                    if (ta.em_act) {
                        const float sa = ep_lds[3][col], sib = ep_lds[4][col];
#pragma unroll
                        for (int e = 0; e < 4; ++e) ev[e] = sat_snake(ov[e], sa, sib);
                    }
                    if (!ok) ev = f32x4{0.f, 0.f, 0.f, 0.f};
                    *reinterpret_cast<f32x4*>(t_row + j * 4 * 68) = ev;
                }
                if (bwd) {
                    if (!ok) { pda = 0.f; pdb = 0.f; }
#pragma unroll
                    for (int m = 8; m >= 1; m >>= 1) {     // sum over the 16 lanes that share this row
                        pda += __shfl_xor(pda, m);
                        pdb += __shfl_xor(pdb, m);
                    }
                    if ((lane & 15) == 0) {
                        red_lds[0][wave % TW][col] = pda;
                        red_lds[1][wave % TW][col] = pdb;
                    }
                }
            }
            if (ta.em_hi) {
                // step 2: read the tile COLUMN-wise — an item is 8 consecutive channels of one time step = one 16-byte plane row
                // ([B][em_c8][em_rows][8], row = 32 + t; the zero rows around the sequence belong to the caller) — split and store:
                // 64 lanes write 1 KiB of each plane contiguously (the wave's LDS ops execute in order)
                sat_wave_sync();
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c8i = ((co0 + co_w + mi * 32) >> 3) + g;
                    const int tq = t0 + t_w + lane;
                    float v8[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v8[e] = tile[g * 8 + e][lane];
                    uint32_t eh[4], el[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) sat_split2_pk(v8[2 * e], v8[2 * e + 1], &eh[e], &el[e]);
                    if (c8i < ta.em_c8 && tq < ta.Tout) {
                        const size_t o = (((size_t)b * ta.em_c8 + c8i) * ta.em_rows + SAT_K7P_LEAD_ROWS + tq) * 8;
                        *reinterpret_cast<u32x4*>(ta.em_hi + o) = u32x4{eh[0], eh[1], eh[2], eh[3]};
                        *reinterpret_cast<u32x4*>(ta.em_lo + o) = u32x4{el[0], el[1], el[2], el[3]};
                    }
                }
            }
        }
    }
}

// The whole epilogue of a 128-channel x (TW x 64)-step tile of a kernel of NT threads whose output is plainly addressed (the direct and the
// planes kernel): the 16-byte path above or, for Tout % 4 != 0 or a misaligned tensor, 4 bytes at a time; then the tile's row
// b * ta.t_tiles + t_tile of part_da / part_db.
template <int TW, int NT>
SAT_DEVICE void sat_conv_epilogue_plain(const SatConvEpArgs& ta, f32x16 (&acc)[2][2], float (*tile)[68], float (*red_lds)[TW][SAT_CO_T],
                                        float (*ep_lds)[SAT_CO_T], int tid, int lane, int wave) {
    const bool bwd = ta.x2 != nullptr;
    const int b = ta.b, co0 = ta.co0, t0 = ta.t0;
    if (bwd) {
        __syncthreads();
        for (int i = tid; i < 2 * TW * SAT_CO_T; i += NT) (&red_lds[0][0][0])[i] = 0.0f;
        __syncthreads();
    }
    const int l31 = lane & 31, hi = lane >> 5;
    const int co_w = (wave / TW) * 64, t_w = (wave % TW) * 64;
    const bool vec4 = (ta.Tout & 3) == 0 && (((uintptr_t)ta.y | (uintptr_t)ta.x2 | (uintptr_t)ta.res) & 15) == 0;
    if (vec4) {
        sat_conv_epilogue16<TW>(ta, acc, tile, red_lds, ep_lds, lane, wave);
    } else
    if ((co0 + co_w) < ta.cout) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            if (mi == 1 && (co0 + co_w + 32) >= ta.cout) break;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = co_w + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                const int co = co0 + col;
                const bool co_ok = co < ta.cout;
                const float bias = ep_lds[0][col];
                const float a2 = ep_lds[1][col], b2 = ep_lds[2][col];
                float pda = 0.f, pdb = 0.f;
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const int t = t0 + t_w + ni * 32 + l31;
                    if (co_ok && t < ta.Tout) {
                        const size_t o = ((size_t)b * ta.cout + co) * ta.Tout + t;
                        // (no residual: -0, the exact identity of the addition)
                        ta.y[o] = sat_conv_finish(acc[mi][ni][r], bias, bwd, bwd ? ta.x2[o] : 0.0f, a2, b2, ta.res ? ta.res[o] : -0.0f, ta.tanh_out, pda, pdb);
                    }
                }
                if (bwd) {
                    pda = sat_half_sum(pda);
                    pdb = sat_half_sum(pdb);
                    if (l31 == 0) {
                        red_lds[0][wave % TW][col] = pda;
                        red_lds[1][wave % TW][col] = pdb;
                    }
                }
            }
        }
    }
    if (bwd) {
        __syncthreads();
        const int m = co0 + tid;
        if (tid < SAT_CO_T && m < ta.cout) {
            float sa = 0.f, sb = 0.f;
#pragma unroll
            for (int w = 0; w < TW; ++w) {
                sa += red_lds[0][w][tid];
                sb += red_lds[1][w][tid];
            }
            const size_t row = (size_t)b * ta.t_tiles + ta.t_tile;
            const size_t nrows_p = (size_t)ta.B * ta.t_tiles;
            ta.part_da[(size_t)m * nrows_p + row] = sa;
            ta.part_db[(size_t)m * nrows_p + row] = sb;
        }
    }
}
