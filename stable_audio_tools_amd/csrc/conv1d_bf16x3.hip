// conv1d_bf16x3.hip — the k = 5..8, stride-1 (dilated) Oobleck convolutions — 7/8 of the conv
// stack's FLOPs: the k7 convs of every ResidualUnit (autoencoders.py:58-83) and their data-gradients —
// on the bf16 matrix cores at fp32 accuracy.
//
// Why: with fp32 operands the stack is bound by v_mfma_f32_32x32x2_f32 (157 TFLOP/s); the bf16 pipe is
// 16x faster.  Every fp32 value is split as x = hi + lo (two bf16, |x - hi - lo| <= 2^-17 |x|) and each
// product is three MFMAs (hi*hi + hi*lo + lo*hi, fp32 accumulate): error ~2^-16 per product — far
// inside the 1e-3 parity bar — at 1/3 of the bf16 rate = 5.3x the fp32-MFMA rate.
//
// Implicit GEMM, same 128(co) x 128(t) workgroup tile / 2x2 32x32 accumulators per wave / epilogues
// as conv1d.hip.  What differs is the K side (v_mfma_f32_32x32x16_bf16 wants 8 consecutive k per lane):
//   * a K-chunk is 8 input channels x all taps = 8 "groups" of 8 k-values (tap g, 8 channels); group
//     7 is a zero pad when K = 7.  One MFMA k-step (16 k) = groups 2j (lanes 0-31) and 2j+1 (lanes 32-63).
//   * activations are staged TRANSPOSED: LDS rows are time steps holding 8 channels (16 B), so the B
//     fragment of (tap g, time t) is ONE 16-byte read of row t + g*dil — SnakeBeta and the hi/lo
//     split are applied once per element while staging.
//   * weights are pre-split and pre-arranged by sat_pack_weights_bf16x3 as [chunk][co][group][8],
//     so a chunk's slab is a straight 16-byte-per-lane copy into padded LDS rows.
//   * launches of few tiles and many chunks (the bottom of the U: 128 workgroups of 256 chunks, 8 of 128, the planes kernel's 4 of 128) are SPLIT
//     over chunks (SatConvBfLaunch::nsplit / cps / ws, sat_conv_split_rule below): n workgroups per tile run 1 / n of the K loop each and store
//     their raw accumulators to a workspace slab; a second launch of the SAME kernel with an empty chunk range sums a tile's slabs in index
//     order and runs the unchanged epilogue (one copy of it, no atomics, the same bits every run).  730 -> 333 + 27 us, 261 -> 24 + 31 us and
//     278 -> ~24 + 30 us per launch on the flagship step (profiles/conv_split/README.md).
#include "conv_common.h"
#include <type_traits>

#define SAT_K7P_LEAD_ROWS 32  // zero rows before t = 0 in an activation plane (= SAT_K7P_LEAD of conv1d_planes.h)
#define SAT_BF_AROWS1 192  // CS == 1: max staged time rows: 128 + (K-1)*dil <= 128 + 7*9 = 191
#define SAT_BF_AROWSN 136  // CS  > 1: 128 + (taps-1) rows, taps <= 4, dil = 1

struct SatConvBfLaunch {
    SatConvParams p;       // REAL tensor dims (Cin, Tin, Cout, Tout); p.K / p.dil / p.pad describe the VIRTUAL stride-1 conv;
                           // p.w unused; p.alpha / p.beta hold PRE-EXPONENTIATED snake constants: a = e^alpha, ib = 1/(e^beta+1e-9)
    const short* w_hi;     // [nchunks][cout_pad][NG][8]
    const short* w_lo;
    int cout_pad;          // virtual output channels rounded up to the 128 tile
    int cin_v, cout_v;     // virtual channel counts: Cin << sin_log2, Cout << sout_log2
    int sin_log2;          // space-to-depth of the input:  x'[ci*S + r][q] = x[ci][q*S + r - in_shift]   (strided conv)
    int sout_log2;         // depth-to-space of the output: y[co][q*S + r - out_shift] = y'[co*S + r][q]  (transposed conv)
    int in_shift, out_shift;
    int nq;                // virtual output positions
    // conv1d_planes.h: the activation as pre-split planes [B][xp_c8][xp_rows][8] (null: convert from p.x while staging)
    const short* xp_hi = nullptr;
    const short* xp_lo = nullptr;
    int xp_rows = 0, xp_c8 = 0;
    int wq = 0;            // conv1d_bf16x3_k7q.h: the weight planes are in sat_pack_weights_k7q layout ([chunk16][tap][group][co][8])
    int stagger = 0;       // conv1d_bf16x3_k7q.h: start delay units (x ~4 us x (0..7)) that de-phase the CUs' epilogue bursts
    int persist = 0;       // conv1d_bf16x3_k7q.h: one workgroup per CU walks the tiles, the next tile's first chunk requested before the epilogue
    int dma_in_mfma = 0;   // conv1d_bf16x3_k7q.h VARIANT 3: the next chunk's LDS-DMA issued inside the MFMA sections
    // plane EMISSION (generic kernel, 16-byte epilogue): besides y the kernel writes act(y) as the bf16 hi / lo planes the next k7
    // conv reads ([B][em_c8][em_rows][8], row = 32 + t; the zero rows around the sequence belong to the caller) — the consumer's
    // sat_k7_planes_kernel pre-pass (one read + one write of the tensor) disappears.  em_a / em_ib: pre-exponentiated SnakeBeta
    // constants of the CONSUMER's activation (null: planes of y itself, for a data-gradient consumer).
    short* em_hi = nullptr;
    short* em_lo = nullptr;
    const float* em_a = nullptr;
    const float* em_ib = nullptr;
    int em_rows = 0, em_c8 = 0;
    // fused ResidualUnit forward (conv1d_bf16x3_k7q.h, FUSED): the 1x1 conv's weights in sat_pack_weights_k7q layout (K = 1), its bias,
    // the second SnakeBeta's pre-exponentiated constants, and where the intermediate h goes (fp32 (B, C, T), or null: not kept)
    const short* ru_w1_hi = nullptr;
    const short* ru_w1_lo = nullptr;
    const float* ru_bias2 = nullptr;
    const float* ru_a2 = nullptr;
    const float* ru_ib2 = nullptr;
    float* ru_h = nullptr;
    // split over input-channel chunks ("split-K", sat_conv_split_rule): launches whose tiles leave most CUs idle under a long K loop.
    //   split launch  (nsplit >= 2, cps > 0):  nsplit workgroups per tile; workgroup (tile, z) runs the K loop over chunks [z * cps, min((z + 1) * cps,
    //                 nchunks)), stores its RAW accumulators to slab (tile, z) of `ws` and returns — no epilogue;
    //   finish launch (nsplit >= 2, cps == 0): one workgroup per tile, EMPTY chunk range: the accumulators start as slab 0 + slab 1 + ... (index
    //                 order: the same bits every run) and fall through into the ordinary epilogue.
    // nsplit <= 1: the plain launch.
    int nsplit = 0;
    int cps = 0;           // chunks per split
    float* ws = nullptr;   // tiles x nsplit slabs of SAT_SPLIT_SLAB(waves) floats, 16-byte aligned
};

// A slab holds one workgroup's accumulators as [wave][mi][ni][quad][lane] float4 (quad q = accumulator registers 4q .. 4q + 3): every store and
// load instruction of a wave moves 1 KiB of consecutive addresses, and a lane of the finish launch reads back exactly what the lane of the same
// index wrote (the layout is private to these two functions).  Waves / accumulator rows that multiply nothing (channels past Cout) are skipped
// on both sides by the same tile-derived flags.
#define SAT_SPLIT_SLAB(nwaves) ((nwaves) * 4 * 16 * 64)
template <int NW>
SAT_DEVICE f32x4* sat_split_slab(float* ws, int tile, int z, int nsplit, int wave, int lane) {
    return reinterpret_cast<f32x4*>(ws + ((size_t)tile * nsplit + z) * SAT_SPLIT_SLAB(NW) + (size_t)wave * (4 * 16 * 64)) + lane;
}
template <int NW>
SAT_DEVICE void sat_split_store(float* ws, int tile, int z, int nsplit, int wave, int lane, const f32x16 (&acc)[2][2], bool mi1_on) {
    f32x4* s = sat_split_slab<NW>(ws, tile, z, nsplit, wave, lane);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        if (mi == 1 && !mi1_on) break;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                s[((mi * 2 + ni) * 4 + q) * 64] = f32x4{acc[mi][ni][4 * q], acc[mi][ni][4 * q + 1], acc[mi][ni][4 * q + 2], acc[mi][ni][4 * q + 3]};
    }
}
template <int NW>
SAT_DEVICE void sat_split_sum(const float* ws, int tile, int nsplit, int wave, int lane, f32x16 (&acc)[2][2], bool mi1_on) {
    for (int z = 0; z < nsplit; ++z) {                    // (acc is zero on entry; index order: the sum's bits do not depend on which split finished first)
        const f32x4* s = sat_split_slab<NW>(const_cast<float*>(ws), tile, z, nsplit, wave, lane);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            if (mi == 1 && !mi1_on) break;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = s[((mi * 2 + ni) * 4 + q) * 64];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[mi][ni][4 * q + j] += v[j];
                }
        }
    }
}

#include "conv_epilogue.h"        // the output epilogue of this file's kernel and of the k7 / k7q ones

SAT_DEVICE void sat_split2(float x, short* hi, short* lo) {
    const short h = sat_f32_to_bf16(x);
    *hi = h;
    *lo = sat_f32_to_bf16(x - sat_bf16_to_f32(h));
}

// NG = k-groups (8 values each) per K-chunk, CS = 8-channel sub-blocks per chunk; taps per sub-block KT = NG / CS.
// group g of a chunk = (sub-block g / KT, tap g % KT).  GATHER: the input is read space-to-depth (sin_log2 > 0).
//
// Activation staging is the VALU-heavy part (SnakeBeta + hi/lo split per element), so it is laid out to keep every
// channel index wave-uniform (scalar address arithmetic, s_load for the snake constants): a wave owns one sub-block
// (CS > 1) and its lanes are time rows; the (K'-1) halo rows of a CS > 1 chunk are staged one ELEMENT per lane.
template <int NG, int CS, bool GATHER>
__global__ void __launch_bounds__(256)
#if !defined(SAT_HIPEMU)
// the k = 1 plan (NG = 4) is bound by bytes in flight (3 streams of 4*C*T bytes, 48 MFMAs per wave and tile-chunk): three workgroups per CU
__attribute__((amdgpu_waves_per_eu(NG == 4 ? 3 : 2)))
#endif
sat_conv1d_bf16x3_kernel(SatConvBfLaunch a) {
    constexpr int KT = NG / CS;
    constexpr int KROW = NG * 8 + 8;                      // bf16 per weight row in LDS (+8 pad: conflict-free b128 reads)
    constexpr int AROWS = (CS == 1) ? SAT_BF_AROWS1 : SAT_BF_AROWSN;
    constexpr int WPS = 4 / CS;                           // waves per sub-block
    constexpr int NU = (CS == 1) ? 1 : 128 / (64 * WPS);  // main staging items (one time row x 8 channels) per thread
    const SatConvParams& p = a.p;
    // one LDS pool: the weight slab and the activation slab of the K loop, reused by the epilogue as the per-wave
    // transposition tiles (4 waves x 32 rows x 68 floats)
    constexpr int W_BYTES = 2 * SAT_CO_T * KROW * 2, A_BYTES = 2 * CS * AROWS * 8 * 2, T_BYTES = 4 * 32 * 68 * 4;
    constexpr int POOL = (W_BYTES + A_BYTES) > T_BYTES ? (W_BYTES + A_BYTES) : T_BYTES;
    __shared__ __attribute__((aligned(16))) char lds_pool[POOL];
    short (*w_lds)[SAT_CO_T][KROW] = reinterpret_cast<short (*)[SAT_CO_T][KROW]>(lds_pool);                 // [plane][co][g*8+e]
    short (*a_lds)[CS][AROWS][8] = reinterpret_cast<short (*)[CS][AROWS][8]>(lds_pool + W_BYTES);           // [plane][sub-block][time row][8 ci]
    __shared__ float red_lds[2][2][SAT_CO_T];
    __shared__ float ep_lds[5][SAT_CO_T];
    // the input's SnakeBeta constants (pre-exponentiated), ALL channels, staged once (round 6).  They used to be read per chunk inside
    // write_lds: the channel is wave-uniform, but hipcc cannot prove the arrays unclobbered and emits sixteen VECTOR loads from a uniform
    // address behind the chunk's barrier — an L2 round trip on the critical path of every chunk, and a vmcnt(0) that also drains whatever
    // was prefetched further ahead.  (k = 1 plan: 1024 channels = 8 KB, still three workgroups per CU; the others 2048 = 16 KB, two.)
    constexpr int SN_MAX = (NG == 4) ? 1024 : 2048;
    __shared__ float sn_lds[2][SN_MAX];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    // grid = (time tiles, channel tiles, B): the channel tiles of one activation window share an XCD (sat_xcd_tile)
    // (split launch: grid z = B x nsplit — split z_s of every tile, then split z_s + 1 of every tile)
    int co_tile, win;
    int tile_lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const bool split_on = a.nsplit > 1;                   // block-uniform (kernel argument)
    const bool split_fin = split_on && a.cps == 0;
    int z_s = 0;
    if (split_on) {
        const int tiles = (int)(gridDim.x * gridDim.y) * p.B;
        z_s = tile_lin / tiles;
        tile_lin -= z_s * tiles;
    }
    sat_xcd_tile(tile_lin, gridDim.y, (int)gridDim.x * p.B, &co_tile, &win);
    const int b = win / (int)gridDim.x, t_tile = win - b * (int)gridDim.x;
    const int t0 = t_tile * SAT_T_T;
    const int co0 = co_tile * SAT_CO_T;
    const int co_w = (wave >> 1) * 64, t_w = (wave & 1) * 64;
    const int K = p.K, dil = p.dil;
    const int nrows = SAT_T_T + (K - 1) * dil;
    const int q_in0 = t0 - p.pad;
    const int si = GATHER ? a.sin_log2 : 0, so = a.sout_log2;
    const int smask_i = (1 << si) - 1, smask_o = (1 << so) - 1;
    const float* xb = p.x + (size_t)b * p.Cin * p.Tin;
    const bool wave_on = (co0 + co_w) < a.cout_v;
    const bool mi1_on = (co0 + co_w + 32) < a.cout_v;
    const bool has_snake = p.alpha != nullptr;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    if (tid < SAT_CO_T) {
        const int m = co0 + tid;
        const bool ok = m < a.cout_v;
        const int co = m >> so;
        ep_lds[0][tid] = (ok && p.bias) ? p.bias[co] : 0.0f;
        ep_lds[1][tid] = (ok && p.x2) ? expf(p.alpha2[co]) : 1.0f;
        ep_lds[2][tid] = (ok && p.x2) ? expf(p.beta2[co]) : 1.0f;
        ep_lds[3][tid] = (ok && a.em_a) ? a.em_a[co] : 0.0f;
        ep_lds[4][tid] = (ok && a.em_a) ? a.em_ib[co] : 0.0f;
    }
    if (has_snake) {
        const int nsn = p.Cin < SN_MAX ? p.Cin : SN_MAX;
        for (int i = tid; i < nsn; i += 256) {
            sn_lds[0][i] = p.alpha[i];
            sn_lds[1][i] = p.beta[i];
        }
    }
    __syncthreads();                                       // (the first write_lds reads the table)

    const int nchunks = (a.cin_v + 8 * CS - 1) / (8 * CS);
    // this workgroup's chunk range [c_lo, c_hi): everything (plain launch), split z_s's share, or nothing (finish launch: the slabs' sum instead).
    // No chunk at or past c_hi is ever requested.
    const int c_lo = split_on ? z_s * a.cps : 0;
    const int c_hi = split_on ? (c_lo + a.cps < nchunks ? c_lo + a.cps : nchunks) : nchunks;
    if (split_fin && wave_on) sat_split_sum<4>(a.ws, tile_lin, a.nsplit, wave, lane, acc, mi1_on);
    // Register-staged software pipeline: the global loads of chunk c+1 are issued right after the barrier that
    // publishes chunk c, so their HBM/L2 latency runs under chunk c's MFMA phase; they are converted and written
    // to LDS after the phase's closing barrier.
    const int cs_w = SAT_UNIFORM(wave / WPS);             // this wave's sub-block
    const int row0 = (wave % WPS) * 64 + lane;            // its first time row; item u is row0 + u * 64 * WPS
    // halo rows (CS > 1 only): row 128 + lane/8, element lane%8, staged by the first wave of each sub-block
    const int nhalo = (CS > 1) ? (nrows - SAT_T_T) * 8 : 0;
    const bool halo_on = (CS > 1) && (wave % WPS) == 0 && lane < nhalo;
    const int h_row = SAT_T_T + (lane >> 3), h_e = lane & 7;
    // DEEP (round 6, the strided / transposed plans <8, 4>): TWO staging register sets — chunk c + 2 is requested while chunk c multiplies and
    // is converted after chunk c + 1's MFMA phase, two phases of latency cover instead of one (these launches sat at 0.22 matrix-busy and
    // 0.8-1.1 TB/s: two workgroups of four waves per CU, each stalled on a single chunk of 4-byte loads per phase).  The k = 1 plan keeps one
    // set (three workgroups per CU at 164 registers).
    constexpr bool DEEP = (NG == 8 && CS == 4);
    constexpr int NSET = DEEP ? 2 : 1;
    float av[NSET][NU][8];
    float hv[NSET];
    bf16x8 wv[NG];                                        // the weight slab (L2-resident) stays one chunk ahead in ONE set
#pragma unroll
    for (int s_ = 0; s_ < NSET; ++s_) hv[s_] = 0.0f;
    // element (virtual channel v, time row) -> real input: channel v >> si at time ((q_in0 + row) << si) + (v & mask) - in_shift;
    // channels past the end are clamped (their weights are zero), times outside [0, Tin) read as 0 (= snake(0)).
    // The value comes back RAW (from a clamped address) with its in-range flag beside it: `ok ? val : 0` right behind the load makes hipcc wait
    // for every load of a chunk before the MFMA phase they were issued in front of (round 6: the ISA of rounds 1-5 shows vmcnt(15) ... vmcnt(0)
    // between the loads and the first MFMA — the "register-staged software pipeline" never overlapped anything).  The flags travel as one
    // bit mask per staging set and are applied when the set is converted (write_lds).
    auto load_elem = [&](int v, int row, bool* okp) -> float {
        int ch = v >> si;
        ch = ch < p.Cin ? ch : p.Cin - 1;
        const int tin = ((q_in0 + row) << si) + (v & smask_i) - (GATHER ? a.in_shift : 0);
        const bool ok = (unsigned)tin < (unsigned)p.Tin;
        *okp = ok;
        return xb[(size_t)ch * p.Tin + (ok ? tin : 0)];
    };
    unsigned okm[NSET];
#pragma unroll
    for (int s_ = 0; s_ < NSET; ++s_) okm[s_] = 0u;
    auto issue_loads = [&](int c, auto set_c) {
        constexpr int ST = decltype(set_c)::value;
        const int v0 = (c * CS + cs_w) * 8;
        unsigned m = 0u;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int row = row0 + u * 64 * WPS;
            if (CS == 1 && row >= nrows) continue;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                bool ok;
                av[ST][u][e] = load_elem(v0 + e, row, &ok);
                m |= ok ? (1u << (u * 8 + e)) : 0u;
            }
        }
        static_assert(NU * 8 < 31, "the in-range flags of a staging set are one 32-bit mask (bit 31: the halo element)");
        if (CS > 1 && halo_on) {
            bool ok;
            hv[ST] = load_elem(v0 + h_e, h_row, &ok);
            m |= ok ? (1u << 31) : 0u;
        }
        okm[ST] = m;
    };
    auto issue_w = [&](int c) {
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const int idx = tid + u * 256;                 // part = idx % NG, co = (idx / NG) & 127, plane = idx / (NG * 128)
            const int part = idx % NG, co = (idx / NG) & 127, pl = idx / (NG * 128);
            const short* src = (pl ? a.w_lo : a.w_hi) + (((size_t)c * a.cout_pad + co0 + co) * NG + part) * 8;
            wv[u] = *reinterpret_cast<const bf16x8*>(src);
        }
    };
    auto write_lds = [&](int c, auto set_c) {
        constexpr int ST = decltype(set_c)::value;
        const int v0 = (c * CS + cs_w) * 8;
        float sa[8], sib[8];
        if (has_snake) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {                  // wave-uniform channel: LDS broadcast reads of the staged (pre-exponentiated) constants
                int ch = (v0 + e) >> si;
                ch = ch < p.Cin ? ch : p.Cin - 1;
                sa[e] = sn_lds[0][ch];                     // (Cin <= SN_MAX: the host entry points check)
                sib[e] = sn_lds[1][ch];
            }
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int row = row0 + u * 64 * WPS;
            if (CS == 1 && row >= nrows) continue;
            uint32_t ph[4], pl[4];
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                float o0 = (okm[ST] >> (u * 8 + e)) & 1u ? av[ST][u][e] : 0.0f, o1 = (okm[ST] >> (u * 8 + e + 1)) & 1u ? av[ST][u][e + 1] : 0.0f;
                if (has_snake) {
                    o0 = sat_snake(o0, sa[e], sib[e]);
                    o1 = sat_snake(o1, sa[e + 1], sib[e + 1]);
                }
                sat_split2_pk(o0, o1, &ph[e >> 1], &pl[e >> 1]);
            }
            *reinterpret_cast<u32x4*>(&a_lds[0][cs_w][row][0]) = u32x4{ph[0], ph[1], ph[2], ph[3]};
            *reinterpret_cast<u32x4*>(&a_lds[1][cs_w][row][0]) = u32x4{pl[0], pl[1], pl[2], pl[3]};
        }
        if (CS > 1 && halo_on) {
            float o = (okm[ST] >> 31) & 1u ? hv[ST] : 0.0f;
            if (has_snake) {
                int ch = (v0 + h_e) >> si;
                ch = ch < p.Cin ? ch : p.Cin - 1;
                o = sat_snake(o, sn_lds[0][ch], sn_lds[1][ch]);
            }
            short h, l;
            sat_split2(o, &h, &l);
            a_lds[0][cs_w][h_row][h_e] = h;
            a_lds[1][cs_w][h_row][h_e] = l;
        }
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const int idx = tid + u * 256;
            const int part = idx % NG, co = (idx / NG) & 127, pl = idx / (NG * 128);
            *reinterpret_cast<bf16x8*>(&w_lds[pl][co][part * 8]) = wv[u];
        }
    };
    auto mfma_chunk = [&]() {
        if (wave_on) {
            SAT_MFMA_PRIO(1);
#pragma unroll
            for (int ks = 0; ks < NG / 2; ++ks) {
                const int g = 2 * ks + hi;                 // k-slots 0-7 <- group 2ks (lanes 0-31), 8-15 <- group 2ks+1
                const int cs = g / KT;
                int tap = g - cs * KT;
                if (tap >= K) tap = K - 1;                 // taps >= K are zero-weight pads; keep the row in range
                bf16x8 wa[2][2], xa[2][2];                 // [mi|ni][plane]
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    wa[0][pl] = *reinterpret_cast<const bf16x8*>(&w_lds[pl][co_w + l31][g * 8]);
                    wa[1][pl] = *reinterpret_cast<const bf16x8*>(&w_lds[pl][co_w + 32 + l31][g * 8]);
                    xa[0][pl] = *reinterpret_cast<const bf16x8*>(&a_lds[pl][cs][t_w + l31 + tap * dil][0]);
                    xa[1][pl] = *reinterpret_cast<const bf16x8*>(&a_lds[pl][cs][t_w + 32 + l31 + tap * dil][0]);
                }
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    if (mi == 1 && !mi1_on) break;
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) {
                        acc[mi][ni] = sat_mfma_32x32x16_bf16(wa[mi][0], xa[ni][0], acc[mi][ni]);
                        acc[mi][ni] = sat_mfma_32x32x16_bf16(wa[mi][0], xa[ni][1], acc[mi][ni]);
                        acc[mi][ni] = sat_mfma_32x32x16_bf16(wa[mi][1], xa[ni][0], acc[mi][ni]);
                    }
                }
            }
            SAT_MFMA_PRIO(0);
        }
    };
    using SatSet0 = std::integral_constant<int, 0>;
    using SatSet1 = std::integral_constant<int, NSET - 1>;
    if (c_lo < c_hi) {
        issue_loads(c_lo, SatSet0{});
        issue_w(c_lo);
    }
    if constexpr (DEEP) {
        if (c_lo + 1 < c_hi) issue_loads(c_lo + 1, SatSet1{});
        for (int c = c_lo; c < c_hi; c += 2) {
            write_lds(c, SatSet0{});
            __syncthreads();
            // (oldest first: vmcnt retires in order — the weights of chunk c + 1 are needed one phase before the activations of c + 2)
            if (c + 1 < c_hi) issue_w(c + 1);
            SAT_SCHED_FENCE();                             // (the scheduler would otherwise mix the two groups: program order IS the retire order)
            if (c + 2 < c_hi) issue_loads(c + 2, SatSet0{});
            SAT_SCHED_FENCE();
            mfma_chunk();
            __syncthreads();
            if (c + 1 < c_hi) {                         // (block-uniform)
                write_lds(c + 1, SatSet1{});
                __syncthreads();
                if (c + 2 < c_hi) issue_w(c + 2);
                SAT_SCHED_FENCE();
                if (c + 3 < c_hi) issue_loads(c + 3, SatSet1{});
                SAT_SCHED_FENCE();
                mfma_chunk();
                __syncthreads();
            }
        }
    } else {
        for (int c = c_lo; c < c_hi; ++c) {
            write_lds(c, SatSet0{});
            __syncthreads();
            if (c + 1 < c_hi) {
                issue_loads(c + 1, SatSet0{});
                issue_w(c + 1);
            }
            mfma_chunk();
            __syncthreads();
        }
    }

    if (split_on && !split_fin) {                          // split launch: the raw accumulators to this split's slab, no epilogue
        if (wave_on) sat_split_store<4>(a.ws, tile_lin, z_s, a.nsplit, wave, lane, acc, mi1_on);
        return;
    }

    // ------------- epilogue (as conv1d.hip; virtual channel m = co*S + r lands on y[co][q*S + r - out_shift]) -------------
    const bool bwd = (p.x2 != nullptr);
    if (bwd) {
        for (int i = tid; i < 2 * 2 * SAT_CO_T; i += 256) (&red_lds[0][0][0])[i] = 0.0f;
        __syncthreads();
    }
    const bool vec4 = so == 0 && a.out_shift == 0 && (p.Tout & 3) == 0 &&
                      (((uintptr_t)p.y | (uintptr_t)p.x2 | (uintptr_t)p.res) & 15) == 0;
    if (vec4) {
        // plain output addressing: the 16-byte epilogue (conv_epilogue.h), with plane emission
        const SatConvEpArgs ta = sat_conv_ep_args(&a, p.y, p.res, true, b, co0, t0, t_tile, (int)gridDim.x);
        sat_conv_epilogue16<2>(ta, acc, reinterpret_cast<float (*)[68]>(lds_pool) + wave * 32, red_lds, ep_lds, lane, wave);
    } else
    if (wave_on && so >= 1 && ((t0 << so) - a.out_shift) >= 0 && (((t0 + SAT_T_T - 1) << so) + smask_o - a.out_shift) < p.Tout) {
        // depth-to-space epilogue of an INTERIOR tile (round 6): the four consecutive accumulator rows of a lane are four consecutive TIME steps
        // of one real channel (S >= 4) or two pairs (S = 2): x2 / res / y move as 16- / 8-byte accesses at dword alignment, a quarter /
        // half of the memory instructions of the element-wise path below (which keeps the first and the last tile of an item).
        auto ep_vec = [&](auto lg_c) {
            constexpr int GL = 1 << decltype(lg_c)::value, NGP = 4 / GL;      // group length, groups per accumulator quad
            typedef float vecu __attribute__((ext_vector_type(GL), aligned(4)));
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                if (mi == 1 && !mi1_on) break;
                vecu xv[4][NGP][2], rv[4][NGP][2];
#pragma unroll
                for (int rg = 0; rg < 4; ++rg)
#pragma unroll
                    for (int gp = 0; gp < NGP; ++gp) {
                        const int m = co0 + co_w + mi * 32 + 8 * rg + 4 * hi + gp * GL;
                        const bool m_ok = m < a.cout_v;
                        const int co = m_ok ? m >> so : 0;
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) {
                            const int q = t0 + t_w + ni * 32 + l31;
                            const size_t o = ((size_t)b * p.Cout + co) * p.Tout + ((q << so) + (m & smask_o) - a.out_shift);
#pragma unroll
                            for (int e = 0; e < GL; ++e) { xv[rg][gp][ni][e] = 0.0f; rv[rg][gp][ni][e] = 0.0f; }
                            if (bwd) xv[rg][gp][ni] = *reinterpret_cast<const vecu*>(p.x2 + o);
                            if (p.res) rv[rg][gp][ni] = *reinterpret_cast<const vecu*>(p.res + o);
                        }
                    }
#pragma unroll
                for (int rg = 0; rg < 4; ++rg)
#pragma unroll
                    for (int gp = 0; gp < NGP; ++gp) {
                        const int col0 = co_w + mi * 32 + 8 * rg + 4 * hi + gp * GL;
                        const int m = co0 + col0;
                        const bool m_ok = m < a.cout_v;
                        const int co = m_ok ? m >> so : 0;
                        float pda[GL], pdb[GL];
#pragma unroll
                        for (int e = 0; e < GL; ++e) { pda[e] = 0.f; pdb[e] = 0.f; }
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) {
                            const int q = t0 + t_w + ni * 32 + l31;
                            vecu ov;
#pragma unroll
                            for (int e = 0; e < GL; ++e) {
                                const int col = col0 + e;
                                ov[e] = sat_conv_finish(acc[mi][ni][rg * 4 + gp * GL + e], ep_lds[0][col], bwd, xv[rg][gp][ni][e], ep_lds[1][col], ep_lds[2][col],
                                                        rv[rg][gp][ni][e], p.tanh_out, pda[e], pdb[e]);
                            }
                            if (m_ok) *reinterpret_cast<vecu*>(p.y + ((size_t)b * p.Cout + co) * p.Tout + ((q << so) + (m & smask_o) - a.out_shift)) = ov;
                        }
                        if (bwd) {
#pragma unroll
                            for (int e = 0; e < GL; ++e) {
                                const float sa_ = sat_half_sum(m_ok ? pda[e] : 0.f), sb_ = sat_half_sum(m_ok ? pdb[e] : 0.f);
                                if (l31 == 0) {
                                    red_lds[0][wave & 1][col0 + e] = sa_;
                                    red_lds[1][wave & 1][col0 + e] = sb_;
                                }
                            }
                        }
                    }
            }
        };
        if (so >= 2) ep_vec(std::integral_constant<int, 2>{});
        else ep_vec(std::integral_constant<int, 1>{});
    } else
    if (wave_on) {
        // 4-byte epilogue (depth-to-space outputs: transposed convs and the data-gradients of strided convs).  Round 6: the x2 / res loads of
        // a 32-row half are ALL issued (from clamped addresses, no branch around them) before the first is used — they used to sit inside
        // the per-element `if (in range)` block, one dependent load per element: 64 serialised HBM latencies per thread and tile in the
        // strided convs' data-gradients.
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            if (mi == 1 && !mi1_on) break;
            float xv[16][2], rv[16][2];
            unsigned okb = 0u;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = co_w + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                const int m = co0 + col;
                const bool m_ok = m < a.cout_v;
                const int co = m >> so;
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const int q = t0 + t_w + ni * 32 + l31;
                    const int t = (q << so) + (m & smask_o) - a.out_shift;
                    const bool ok = m_ok && t >= 0 && t < p.Tout;
                    okb |= ok ? (1u << (2 * r + ni)) : 0u;
                    const size_t o = ((size_t)b * p.Cout + (ok ? co : 0)) * p.Tout + (ok ? t : 0);
                    xv[r][ni] = bwd ? p.x2[o] : 0.0f;
                    rv[r][ni] = p.res ? p.res[o] : 0.0f;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = co_w + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                const int m = co0 + col;
                const int co = m >> so;
                const float bias = ep_lds[0][col];
                const float a2 = ep_lds[1][col], b2 = ep_lds[2][col];
                float pda = 0.f, pdb = 0.f;
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const int q = t0 + t_w + ni * 32 + l31;
                    const int t = (q << so) + (m & smask_o) - a.out_shift;
                    const bool ok = (okb >> (2 * r + ni)) & 1u;
                    float da = 0.f, db = 0.f;                  // (an element outside the tensor came from a clamped address: its terms are dropped)
                    const float v = sat_conv_finish(acc[mi][ni][r], bias, bwd, xv[r][ni], a2, b2, rv[r][ni], p.tanh_out, da, db);
                    pda += ok ? da : 0.0f;
                    pdb += ok ? db : 0.0f;
                    if (ok) p.y[((size_t)b * p.Cout + co) * p.Tout + t] = v;
                }
                if (bwd) {
                    pda = sat_half_sum(pda);
                    pdb = sat_half_sum(pdb);
                    if (l31 == 0) {
                        red_lds[0][wave & 1][col] = pda;
                        red_lds[1][wave & 1][col] = pdb;
                    }
                }
            }
        }
    }
    if (bwd) {
        __syncthreads();
        const int m = co0 + tid;
        if (tid < SAT_CO_T && (tid & smask_o) == 0 && m < a.cout_v) {      // one thread per REAL channel: sum its S phases
            float sa = 0.f, sb = 0.f;
            for (int r = 0; r <= smask_o; ++r) {
                sa += red_lds[0][0][tid + r] + red_lds[0][1][tid + r];
                sb += red_lds[1][0][tid + r] + red_lds[1][1][tid + r];
            }
            const size_t row = (size_t)b * gridDim.x + t_tile;
            const size_t nrows_p = (size_t)p.B * gridDim.x;
            p.part_da[(size_t)(m >> so) * nrows_p + row] = sa;
            p.part_db[(size_t)(m >> so) * nrows_p + row] = sb;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Plans.  Every conv of the stack is a stride-1 implicit GEMM over virtual channels:
//   conv, stride 1:            K' = K,  plain channels
//   conv, stride S, K = 2S:    K' = 2,  in-channels (ci, r):   x'[(ci,r)][q] = x[ci][q*S + r - pad],   W'[co][(ci,r)][j] = w[co][ci][j*S + r]
//   conv_transpose, K = 2S:    K' = 2,  out-channels (co, r):  y[co][q*S + r - pad] = y'[(co,r)][q],
//                              y'[(co,r)][q] = sum_ci W[ci][co][r+S] x[ci][q-1] + W[ci][co][r] x[ci][q]
// ------------------------------------------------------------------------------------------------
struct SatBfPlan { int ng, cs, kv; };     // groups per chunk, sub-blocks per chunk, virtual taps
static bool sat_bf_plan(int K, int stride, int mode, SatBfPlan* pl) {
    if (mode == 2 || stride > 1) {
        if (K != 2 * stride || (stride & (stride - 1)) || stride > 64) return false;
        *pl = SatBfPlan{8, 4, 2};
        return true;
    }
    if (stride != 1 || K < 1 || K > 8) return false;
    if (K == 1) *pl = SatBfPlan{4, 4, 1};
    else if (K == 2) *pl = SatBfPlan{8, 4, K};
    else if (K <= 4) *pl = SatBfPlan{8, 2, K};
    else *pl = SatBfPlan{8, 1, K};
    return true;
}
static int sat_log2i(int s) { int l = 0; while ((1 << l) < s) ++l; return l; }

// ------------------------------------------------------------------------------------------------
// weight preparation: torch weight w[D0][D1][K] (fp32) -> hi/lo bf16 planes [chunk][m (padded to 128)][group g][e]
// holding W'[m][v][tap] with v = (chunk*CS + g/KT)*8 + e, tap = g % KT (0 where tap/m/v are out of range):
//   mode 0 (conv, w = [out][in][K]):            stride 1: W' = w[m][v][tap];   stride S: W' = w[m][v/S][tap*S + v%S]
//   mode 1 (data-gradient of a stride-1 conv):  W'[m][v][tap] = w[v][m][K-1-tap]
//   mode 2 (conv_transpose, w = [in][out][K]):  W'[m][v][0] = w[v][m/S][m%S + S],  W'[m][v][1] = w[v][m/S][m%S]
// ------------------------------------------------------------------------------------------------
struct SatPackBfParams {
    const float* w;
    short* hi;
    short* lo;
    int D0, D1, K, S, mode, ng, cs, kv, m_v, v_v, out_pad;
    long long total;
};
__global__ void __launch_bounds__(256) sat_pack_bf16x3_kernel(SatPackBfParams p) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= p.total) return;
    const int e = (int)(o & 7);
    long long q = o >> 3;
    const int g = (int)(q % p.ng);
    q /= p.ng;
    const int m = (int)(q % p.out_pad), chunk = (int)(q / p.out_pad);
    const int kt = p.ng / p.cs;
    const int v = (chunk * p.cs + g / kt) * 8 + e, tap = g % kt;
    float val = 0.0f;
    if (tap < p.kv && m < p.m_v && v < p.v_v) {
        if (p.mode == 0) val = p.w[((size_t)m * p.D1 + v / p.S) * p.K + tap * p.S + v % p.S];
        else if (p.mode == 1) val = p.w[((size_t)v * p.D1 + m) * p.K + (p.K - 1 - tap)];
        else val = p.w[((size_t)v * p.D1 + m / p.S) * p.K + (m % p.S) + (tap == 0 ? p.S : 0)];
    }
    short h, l;
    sat_split2(val, &h, &l);
    p.hi[o] = h;
    p.lo[o] = l;
}

static bool sat_pack_bf_geometry(int D0, int D1, int K, int stride, int mode, SatPackBfParams* p) {
    SatBfPlan pl;
    if (mode < 0 || mode > 2 || D0 <= 0 || D1 <= 0 || !sat_bf_plan(K, stride, mode, &pl)) return false;
    if (mode == 1 && stride != 1) return false;
    p->D0 = D0; p->D1 = D1; p->K = K; p->S = stride; p->mode = mode;
    p->ng = pl.ng; p->cs = pl.cs; p->kv = pl.kv;
    if (mode == 0) { p->m_v = D0; p->v_v = D1 * stride; }
    else if (mode == 1) { p->m_v = D1; p->v_v = D0; }
    else { p->m_v = D1 * stride; p->v_v = D0; }
    p->out_pad = sat_cdiv(p->m_v, SAT_CO_T) * SAT_CO_T;
    p->total = (long long)sat_cdiv(p->v_v, 8 * pl.cs) * p->out_pad * pl.ng * 8;
    return true;
}
extern "C" long long sat_pack_weights_bf16x3_size(int D0, int D1, int K, int stride, int mode) {
    SatPackBfParams p{};
    return sat_pack_bf_geometry(D0, D1, K, stride, mode, &p) ? p.total : -1;
}
extern "C" int sat_pack_weights_bf16x3(const float* w, short* hi, short* lo, int D0, int D1, int K, int stride, int mode, void* stream) {
    SatPackBfParams p{};
    if (!sat_pack_bf_geometry(D0, D1, K, stride, mode, &p)) {
        sat_set_error("sat_pack_weights_bf16x3: needs stride 1 with K <= 8, or K == 2*stride with a power-of-two stride; mode 0|1|2");
        return 1;
    }
    p.w = w; p.hi = hi; p.lo = lo;
    SAT_LAUNCH(sat_pack_bf16x3_kernel, dim3((unsigned)sat_cdivll(p.total, 256)), dim3(256), stream, p);
    return sat_check_launch("sat_pack_weights_bf16x3");
}

// snake constants: a = e^alpha, ib = 1 / (e^beta + 1e-9)
struct SatSnakeConstParams { const float* alpha; const float* beta; float* a; float* ib; int C; };
__global__ void __launch_bounds__(256) sat_snake_consts_kernel(SatSnakeConstParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.C) return;
    p.a[i] = expf(p.alpha[i]);
    p.ib[i] = 1.0f / (expf(p.beta[i]) + 1e-9f);
}
extern "C" int sat_snake_consts(const float* alpha, const float* beta, float* a, float* ib, int C, void* stream) {
    if (C <= 0) { sat_set_error("sat_snake_consts: empty"); return 1; }
    SatSnakeConstParams p{alpha, beta, a, ib, C};
    SAT_LAUNCH(sat_snake_consts_kernel, dim3(sat_cdiv(C, 256)), dim3(256), stream, p);
    return sat_check_launch("sat_snake_consts");
}

#include "conv1d_bf16x3_k7.h"     // the pipelined kernel of the (8, 1) plan
#include "conv1d_planes.h"        // activation planes [B][Cin/8][rows][8] (pre-pass kernel; layout constants)
#include "conv1d_bf16x3_k7q.h"    // planes, 16-channel chunks (one tap per MFMA k-step), two wave rows one barrier apart

// ------------------------------------------------------------------------------------------------
// Split over input-channel chunks.  A launch of few tiles and a long K loop runs on a small part of the chip (the bottom of the U at T = 1024: a
// 1024 -> 2048 stride-8 conv is 128 workgroups of 256 chunks each on 256 CUs; the 2048 -> 64 k7 data-gradient is FOUR workgroups of 128 chunks).
// THE RULE (one function, no per-shape table): as many splits as there are free workgroup slots per tile, while every split keeps at least
// SAT_SPLIT_MINC chunks — below that its prologue (the first chunk's latency, uncovered) and the round trip of its slab are not amortised:
//     nsplit = min(slots / tiles, nchunks / SAT_SPLIT_MINC),   slots = CUs x resident workgroups per CU of the plan,
// evened out so that no split is empty (chunks per split = ceil(nchunks / nsplit), nsplit = ceil(nchunks / cps)); 1 = do not split.
// ------------------------------------------------------------------------------------------------
#define SAT_SPLIT_MINC 8
#define SAT_SPLIT_MAX 64
extern "C" int sat_conv_split_rule(int tiles, int nchunks, int resident, int cus) {
    if (tiles <= 0 || nchunks <= 0 || resident <= 0 || cus <= 0) return 1;
    const long long by_slots = (long long)cus * resident / tiles;
    long long n = nchunks / SAT_SPLIT_MINC;
    if (by_slots < n) n = by_slots;
    if (n > SAT_SPLIT_MAX) n = SAT_SPLIT_MAX;
    if (n < 2) return 1;
    const int cps = sat_cdiv(nchunks, (int)n);
    return sat_cdiv(nchunks, cps);
}

// ---- activation planes of the k = 5..7 stride-1 convs (conv1d_planes.h, conv1d_bf16x3_k7q.h) ----
// rows of one (batch, 8-channel chunk) plane: 32 zero rows, the sequence, zero rows up to the last window's halo
extern "C" int sat_conv1d_k7_plane_rows(int Tin, int Tout, int pad) {
    if (Tin <= 0 || Tout <= 0 || pad < 0 || pad > SAT_K7P_LEAD) return -1;
    const int need = sat_cdiv(Tout, SAT_K7_T) * SAT_K7_T - pad + SAT_K7_AROWS;   // last window: rows [t0 - pad, t0 - pad + 320)
    const int body = need > Tin ? need : Tin;
    return SAT_K7P_LEAD + sat_cdiv(body, 64) * 64;
}
// x (B, Cin, Tin) fp32 -> act(x) as bf16 hi / lo planes [B][ceil(Cin/8)][rows][8]  (act = SnakeBeta with pre-exponentiated constants, or none)
extern "C" int sat_conv1d_k7_planes(const float* x, const float* snake_a, const float* snake_ib, short* xp_hi, short* xp_lo, int B,
                                    int Cin, int Tin, int rows, void* stream) {
    if (B <= 0 || Cin <= 0 || Tin <= 0 || rows < SAT_K7P_LEAD + Tin) { sat_set_error("sat_conv1d_k7_planes: bad shape"); return 1; }
    if ((snake_a == nullptr) != (snake_ib == nullptr)) { sat_set_error("sat_conv1d_k7_planes: snake constants must both be given"); return 1; }
    SatK7PlaneParams p{x, snake_a, snake_ib, xp_hi, xp_lo, B, Cin, Tin, rows, sat_cdiv(Cin, 8)};
    SAT_LAUNCH(sat_k7_planes_kernel, dim3(sat_cdiv(rows, 256), p.c8, B), dim3(256), stream, p);
    return sat_check_launch("sat_conv1d_k7_planes");
}

// ------------------------------------------------------------------------------------------------
// One launch = a SHAPE (integers), the KERNEL that serves it and its OPERANDS (pointers).  Every launching entry point fills a shape and an
// operand record and calls sat_bf_run: sat_bf_geometry (every shape check; the virtual stride-1 conv of "Plans" above) -> sat_bf_kernel ->
// sat_bf_bind (every pointer check) -> sat_bf_split_decide -> the launch, or the split and the finish launch.  The host-only queries
// (sat_conv_bf16x3_split, *_partial_rows) stop after sat_bf_kernel.
// ------------------------------------------------------------------------------------------------
enum SatBfKind { SAT_BF_CONV = 0, SAT_BF_CONVTR = 1, SAT_BF_PLANES = 2, SAT_BF_UNIT = 3 };      // 0 .. 2: the `kind` of sat_conv_bf16x3_split
struct SatBfShape {
    int kind, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, tanh_out;
    int rows;              // SAT_BF_PLANES / _UNIT: rows of an input plane
    int flags;             // SAT_BF_PLANES: bit 0: one workgroup per tile (round 5's launch; A/B runs and the tests' second arm); bit 1: persistent at
                           // any size (the tests: small shapes); bit 2: VARIANT 3 of the k7q kernel
};
struct SatBfInput { const float* x; const float* snake_a; const float* snake_ib; };     // fp32 input, its pre-exponentiated SnakeBeta constants or null
struct SatBfPlanesIn { const short* hi; const short* lo; };                             // SAT_BF_PLANES / _UNIT: the (activated) input as planes
struct SatBfOutput { const float* bias; const float* res; float* y; };
struct SatBfDgrad { const float* x2; const float* alpha2; const float* beta2; float* part_da; float* part_db; };      // data-gradient epilogue: all five or none
struct SatBfEmit { short* hi; short* lo; const float* a; const float* ib; int rows; };  // plane emission (hi null: none)
struct SatBfUnit { const short* w1_hi; const short* w1_lo; const float* bias2; const float* a2; const float* ib2; float* h; };   // fused unit: its second conv
struct SatBfOperands {
    SatBfInput in;
    SatBfPlanesIn xp;
    const short* w_hi;
    const short* w_lo;
    SatBfOutput out;
    SatBfDgrad dg;
    SatBfEmit em;
    SatBfUnit ru;
};

// WHICH KERNEL SERVES A LAUNCH — asked here and nowhere else — and what the host needs to know of that kernel.
enum SatBfKernelId { SAT_BF_K7, SAT_BF_K7Q, SAT_BF_K7Q_FUSED, SAT_BF_GENERIC };       // direct k7, planes k7q, the fused unit, sat_conv1d_bf16x3_kernel
struct SatBfKernel {
    SatBfKernelId id;
    int ng, cs;            // SAT_BF_GENERIC: the instantiation <ng, cs, strided>
    bool strided;
    int co_t, t_t;         // output tile: channels x time steps
    int chunk;             // input channels per step of the K loop
    int resident;          // workgroups per CU
    int slab;              // floats of a workgroup's accumulators in the split workspace; 0: the kernel does not split
    bool emits;            // its epilogue can write the consumer's planes
};
static SatBfKernel sat_bf_kernel(int kind, const SatBfPlan& pl, const SatConvBfLaunch& a) {
    if (pl.ng == 8 && pl.cs == 1 && a.sin_log2 == 0 && a.sout_log2 == 0) {       // 5 <= K <= 8 at stride 1: the 128 x 256 tile, 512 threads
        const SatBfKernelId id = kind == SAT_BF_UNIT ? SAT_BF_K7Q_FUSED : kind == SAT_BF_PLANES ? SAT_BF_K7Q : SAT_BF_K7;
        return SatBfKernel{id, 8, 1, false, SAT_K7_CO, SAT_K7_T, id == SAT_BF_K7 ? 8 : 16, 1, id == SAT_BF_K7Q ? SAT_SPLIT_SLAB(SAT_K7_NT / 64) : 0,
                           id == SAT_BF_K7Q_FUSED};
    }
    return SatBfKernel{SAT_BF_GENERIC, pl.ng, pl.cs, a.sin_log2 > 0, SAT_CO_T, SAT_T_T, 8 * pl.cs, pl.ng == 4 ? 3 : 2, SAT_SPLIT_SLAB(4), true};
}

static int sat_bf_fail(const char* who, const char* msg) {
    char buf[512];
    snprintf(buf, sizeof(buf), "%s: %s", who, msg);
    sat_set_error(buf);
    return 1;
}

// shape -> plan + launch with every non-pointer field set; 1 and sat_last_error() where the family does not serve the shape
static int sat_bf_geometry(const char* who, const SatBfShape& s, SatBfPlan* pl, SatConvBfLaunch* out) {
    const bool unit = s.kind == SAT_BF_UNIT;
    if (s.B <= 0 || s.Cin <= 0 || s.Cout <= 0 || s.Tin <= 0 || s.Tout <= 0) return sat_bf_fail(who, unit ? "needs 1 <= C <= 128" : "empty shape");
    SatConvBfLaunch a{};
    a.cin_v = s.Cin;
    a.cout_v = s.Cout;
    a.nq = s.Tout;
    int vdil = s.dil, vpad = s.pad;                           // of the virtual stride-1 conv
    if (s.kind == SAT_BF_CONV) {
        if (!sat_bf_plan(s.K, s.stride, 0, pl) || s.dil < 1 || (s.stride > 1 && s.dil != 1))
            return sat_bf_fail(who, "needs stride 1 with K <= 8, or K == 2*stride (power-of-two stride, dilation 1)");
        if ((pl->kv - 1) * s.dil > (pl->cs == 1 ? 62 : SAT_BF_AROWSN - SAT_T_T)) return sat_bf_fail(who, "receptive field too large for the LDS slab");
        a.cin_v = s.Cin * s.stride;
        a.sin_log2 = sat_log2i(s.stride);
        if (s.stride > 1) { a.in_shift = s.pad; vpad = 0; }
    } else if (s.kind == SAT_BF_CONVTR) {
        if (!sat_bf_plan(s.K, s.stride, 2, pl) || s.pad < 0) return sat_bf_fail(who, "needs K == 2*stride with a power-of-two stride");
        a.cout_v = s.Cout * s.stride;
        a.sout_log2 = sat_log2i(s.stride);
        a.out_shift = s.pad;
        a.nq = sat_cdiv(s.Tout + s.pad, s.stride);
        vdil = vpad = 1;
    } else {
        if (unit && s.Cout > SAT_K7_CO) return sat_bf_fail(who, "needs 1 <= C <= 128");
        if (s.K < 5 || s.K > SAT_K7Q_TAPS || s.dil < 1 || (s.K - 1) * s.dil > 62 || (unit && 2 * s.pad != (s.K - 1) * s.dil))
            return sat_bf_fail(who, unit ? "needs 5 <= K <= 7, (K-1)*dil <= 62, 'same' padding" : "needs stride 1, 5 <= K <= 7, (K-1)*dil <= 62");
        if (s.rows < sat_conv1d_k7_plane_rows(s.Tin, s.Tout, s.pad))
            return sat_bf_fail(who, unit ? "rows must be >= sat_conv1d_k7_plane_rows(T, T, pad)" : "rows must be >= sat_conv1d_k7_plane_rows(Tin, Tout, pad)");
        *pl = SatBfPlan{8, 1, s.K};
        a.xp_rows = s.rows;
        a.xp_c8 = sat_cdiv(s.Cin, 8);
        a.wq = 1;
        if (!unit) {
            a.dma_in_mfma = (s.flags & 4) ? 1 : 0;
            a.persist = (s.flags & 1) ? 0 : ((s.flags & 2) ? 2 : 1);
        }
    }
    a.cout_pad = sat_cdiv(a.cout_v, SAT_CO_T) * SAT_CO_T;
    a.p.B = s.B; a.p.Cin = s.Cin; a.p.Cout = s.Cout; a.p.Tin = s.Tin; a.p.Tout = s.Tout;
    a.p.K = pl->kv; a.p.stride = 1; a.p.dil = vdil; a.p.pad = vpad; a.p.tanh_out = s.tanh_out;
    *out = a;
    return 0;
}

// the pointer-dependent checks, once, then the pointers into the launch
static int sat_bf_bind(const char* who, const SatBfKernel& k, const SatBfOperands& o, SatConvBfLaunch* a) {
    const bool fused = k.id == SAT_BF_K7Q_FUSED;
    if ((o.in.snake_a == nullptr) != (o.in.snake_ib == nullptr)) return sat_bf_fail(who, "snake constants must both be given");
    if (o.dg.x2 && (!o.dg.alpha2 || !o.dg.beta2 || !o.dg.part_da || !o.dg.part_db)) return sat_bf_fail(who, "backward epilogue needs alpha2/beta2/partials");
    if (k.id == SAT_BF_K7Q && (!o.xp.hi || !o.xp.lo)) return sat_bf_fail(who, "activation planes missing");
    if (fused && (!o.xp.hi || !o.xp.lo || !o.w_hi || !o.w_lo || !o.ru.w1_hi || !o.ru.w1_lo || !o.ru.a2 || !o.ru.ib2 || !o.out.res || !o.out.y))
        return sat_bf_fail(who, "missing operand");
    const bool vec4 = (a->p.Tout & 3) == 0 && (((uintptr_t)o.out.y | (uintptr_t)o.dg.x2 | (uintptr_t)o.out.res) & 15) == 0;       // the 16-byte epilogue
    if (fused && !vec4) return sat_bf_fail(who, "T % 4 == 0 and 16-byte aligned x / y");
    if (o.em.hi) {
        if (!k.emits || !vec4 || !o.em.lo || (o.em.a == nullptr) != (o.em.ib == nullptr) || o.em.rows < SAT_K7P_LEAD_ROWS + a->p.Tout ||
            (((uintptr_t)o.em.hi | (uintptr_t)o.em.lo) & 15))
            return sat_bf_fail(who, fused ? "bad emission planes"
                                          : "emission needs K <= 4 or a strided conv, Tout % 4 == 0, 16-byte aligned tensors, rows >= 32 + Tout");
        a->em_hi = o.em.hi; a->em_lo = o.em.lo; a->em_a = o.em.a; a->em_ib = o.em.ib; a->em_rows = o.em.rows; a->em_c8 = sat_cdiv(a->p.Cout, 8);
    }
    a->p.x = o.in.x; a->p.alpha = o.in.snake_a; a->p.beta = o.in.snake_ib;
    a->xp_hi = o.xp.hi; a->xp_lo = o.xp.lo;
    a->w_hi = o.w_hi; a->w_lo = o.w_lo;
    a->p.bias = o.out.bias; a->p.res = o.out.res; a->p.y = o.out.y;
    a->p.x2 = o.dg.x2; a->p.alpha2 = o.dg.alpha2; a->p.beta2 = o.dg.beta2; a->p.part_da = o.dg.part_da; a->p.part_db = o.dg.part_db;
    a->ru_w1_hi = o.ru.w1_hi; a->ru_w1_lo = o.ru.w1_lo; a->ru_bias2 = o.ru.bias2; a->ru_a2 = o.ru.a2; a->ru_ib2 = o.ru.ib2; a->ru_h = o.ru.h;
    return 0;
}

// want: < 0 the rule, 0 no split, n >= 2 exactly n splits.  Returns the split count (1: none), or -1 for a forced count the launch cannot have
// (a kernel that does not split, more splits than chunks, or a count that would leave a split without chunks).  *ws_floats: the slabs' size.
static int sat_bf_split_decide(const SatConvBfLaunch& a, const SatBfKernel& k, int want, int cus, int* cps, long long* ws_floats) {
    const int tiles = k.slab ? (a.cout_pad / k.co_t) * sat_cdiv(a.nq, k.t_t) * a.p.B : 0, nchunks = sat_cdiv(a.cin_v, k.chunk);
    int n = 1;
    *cps = 0;
    *ws_floats = 0;
    if (want == 0 || want == 1) return 1;
    if (want < 0) {
        if (tiles == 0) return 1;
        n = sat_conv_split_rule(tiles, nchunks, k.resident, cus > 0 ? cus : sat_cu_count());
        if (n < 2) return 1;
    } else {
        if (tiles == 0 || want > SAT_SPLIT_MAX || want > nchunks) return -1;
        if (sat_cdiv(nchunks, sat_cdiv(nchunks, want)) != want) return -1;
        n = want;
    }
    *cps = sat_cdiv(nchunks, n);
    *ws_floats = (long long)tiles * n * k.slab;
    return n;
}

static int sat_bf_launch_one(const char* who, SatConvBfLaunch& a, const SatBfKernel& k, void* stream) {
    const unsigned zmul = (a.nsplit > 1 && a.cps > 0) ? (unsigned)a.nsplit : 1u;      // workgroups per tile
    if (k.id != SAT_BF_GENERIC) {
        if (k.id == SAT_BF_K7) sat_bf_launch_k7(a, stream);
        else sat_bf_launch_k7q(a, stream, zmul);
        return sat_check_launch(who);
    }
    // the generic kernel stages the input's SnakeBeta constants of ALL channels in LDS: 1024 channels on the k = 1 plan (4, 4), 2048 on the others
    // (every Oobleck level: channels 128 x c_mults <= 16)
    if (a.p.alpha && a.p.Cin > ((k.ng == 4) ? 1024 : 2048))
        return sat_bf_fail(who, "an activated input of more than 2048 channels (1024 for K <= 4 at stride 1) is not served by the bf16x3 kernels (ops.use_bf16x3 = False takes the fp32-MFMA ones)");
    dim3 grid(sat_cdiv(a.nq, k.t_t), a.cout_pad / k.co_t, a.p.B * zmul);
    if (k.strided) { SAT_LAUNCH((sat_conv1d_bf16x3_kernel<8, 4, true>), grid, dim3(256), stream, a); }     // strided: always plan (8, 4)
    else if (k.ng == 8 && k.cs == 1) { SAT_LAUNCH((sat_conv1d_bf16x3_kernel<8, 1, false>), grid, dim3(256), stream, a); }
    else if (k.ng == 8 && k.cs == 2) { SAT_LAUNCH((sat_conv1d_bf16x3_kernel<8, 2, false>), grid, dim3(256), stream, a); }
    else if (k.ng == 8 && k.cs == 4) { SAT_LAUNCH((sat_conv1d_bf16x3_kernel<8, 4, false>), grid, dim3(256), stream, a); }
    else { SAT_LAUNCH((sat_conv1d_bf16x3_kernel<4, 4, false>), grid, dim3(256), stream, a); }
    return sat_check_launch(who);
}

// the split state of one call through a _ws entry point; the plain entry points pass SAT_NO_SPLIT: no workspace, no split
struct SatSplitWs { float* ws; long long ws_floats; int want; int cus; };
static const SatSplitWs SAT_NO_SPLIT{nullptr, 0, 0, 0};

static int sat_bf_run(const char* who, const SatBfShape& s, const SatBfOperands& o, const SatSplitWs& sw, void* stream) {
    SatBfPlan pl;
    SatConvBfLaunch a;
    if (sat_bf_geometry(who, s, &pl, &a)) return 1;
    const SatBfKernel k = sat_bf_kernel(s.kind, pl, a);
    if (sat_bf_bind(who, k, o, &a)) return 1;
    int cps;
    long long need;
    const int n = sat_bf_split_decide(a, k, sw.want, sw.cus, &cps, &need);
    if (n < 0) return sat_bf_fail(who, "this launch cannot be split that many ways (2 <= n <= chunks, every split at least one chunk; the direct k7 kernel and the fused unit do not split)");
    if (n < 2) return sat_bf_launch_one(who, a, k, stream);
    if (!sw.ws || sw.ws_floats < need || ((uintptr_t)sw.ws & 15)) return sat_bf_fail(who, "the split workspace is missing, misaligned or smaller than sat_conv_bf16x3_split asks for");
    a.ws = sw.ws;
    a.nsplit = n;
    a.cps = cps;                                           // split launch: n workgroups per tile
    if (const int st = sat_bf_launch_one(who, a, k, stream)) return st;
    a.cps = 0;                                             // finish launch: the slabs' sum and the epilogue
    return sat_bf_launch_one(who, a, k, stream);
}

// Same contract as sat_conv1d (y[co][t] = sum W[co][ci][k] act(x)[ci][t*stride + k*dil - pad]), with the weights given
// as sat_pack_weights_bf16x3 planes (mode 0, or mode 1 for a stride-1 data-gradient) and the SnakeBeta constants given
// pre-exponentiated (sat_snake_consts), or NULL for no activation.  stride 1: K <= 8; stride S: K == 2S, S a power of two.
extern "C" int sat_conv1d_bf16x3(const float* x, const short* w_hi, const short* w_lo, const float* bias,
                                 const float* snake_a, const float* snake_ib, const float* res, float* y,
                                 const float* x2, const float* alpha2, const float* beta2, float* part_da,
                                 float* part_db, int B, int Cin, int Cout, int Tin, int Tout, int K, int stride, int dil,
                                 int pad, int tanh_out, void* stream) {
    const SatBfShape s{SAT_BF_CONV, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, tanh_out, 0, 0};
    const SatBfOperands o{{x, snake_a, snake_ib}, {}, w_hi, w_lo, {bias, res, y}, {x2, alpha2, beta2, part_da, part_db}, {}, {}};
    return sat_bf_run("sat_conv1d_bf16x3", s, o, SAT_NO_SPLIT, stream);
}
// sat_conv1d_bf16x3 that ALSO writes act(y) as the activation planes of the k7 conv that consumes y next (sat_conv1d_bf16x3_planesq):
// em_hi / em_lo [B][ceil(Cout/8)][em_rows][8] bf16 (row 32 + t; the caller keeps the rows around the sequence zero),
// em_a / em_ib the consumer's pre-exponentiated SnakeBeta constants (sat_snake_consts) or NULL for planes of y itself.  The k = 1 /
// K <= 4 / strided plans only (the producers of a ResidualUnit's input), Tout % 4 == 0.
extern "C" int sat_conv1d_bf16x3_emit(const float* x, const short* w_hi, const short* w_lo, const float* bias,
                                      const float* snake_a, const float* snake_ib, const float* res, float* y,
                                      const float* x2, const float* alpha2, const float* beta2, float* part_da,
                                      float* part_db, int B, int Cin, int Cout, int Tin, int Tout, int K, int stride, int dil,
                                      int pad, int tanh_out, void* em_hi, void* em_lo, const float* em_a, const float* em_ib, int em_rows,
                                      void* stream) {
    if (!em_hi) return sat_bf_fail("sat_conv1d_bf16x3_emit", "planes missing");
    const SatBfShape s{SAT_BF_CONV, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, tanh_out, 0, 0};
    const SatBfOperands o{{x, snake_a, snake_ib}, {}, w_hi, w_lo, {bias, res, y}, {x2, alpha2, beta2, part_da, part_db},
                          {(short*)em_hi, (short*)em_lo, em_a, em_ib, em_rows}, {}};
    return sat_bf_run("sat_conv1d_bf16x3_emit", s, o, SAT_NO_SPLIT, stream);
}
// sat_conv1d_bf16x3 / _emit (em_hi NULL: no emission) that may SPLIT its launch over input-channel chunks (sat_conv_split_rule): ws = a workspace of
// ws_floats floats, at least what sat_conv_bf16x3_split(0, ...) reports for the same `split` (-1: the rule, 0: off, n >= 2: exactly n — status 1
// and no launch where the launch cannot be split that way).  The workspace is written by the first launch and read by the second.
extern "C" int sat_conv1d_bf16x3_ws(const float* x, const short* w_hi, const short* w_lo, const float* bias,
                                    const float* snake_a, const float* snake_ib, const float* res, float* y,
                                    const float* x2, const float* alpha2, const float* beta2, float* part_da,
                                    float* part_db, int B, int Cin, int Cout, int Tin, int Tout, int K, int stride, int dil,
                                    int pad, int tanh_out, void* em_hi, void* em_lo, const float* em_a, const float* em_ib, int em_rows,
                                    float* ws, long long ws_floats, int split, void* stream) {
    const SatBfShape s{SAT_BF_CONV, B, Cin, Cout, Tin, Tout, K, stride, dil, pad, tanh_out, 0, 0};
    const SatBfOperands o{{x, snake_a, snake_ib}, {}, w_hi, w_lo, {bias, res, y}, {x2, alpha2, beta2, part_da, part_db},
                          {(short*)em_hi, (short*)em_lo, em_a, em_ib, em_rows}, {}};
    return sat_bf_run("sat_conv1d_bf16x3_ws", s, o, SatSplitWs{ws, ws_floats, split, 0}, stream);
}

// sat_conv1d_bf16x3 for stride 1, 5 <= K <= 7, with the (activated) input given as planes (sat_conv1d_k7_planes or a producer's emission)
// and the weights packed by sat_pack_weights_k7q (mode 0, or mode 1 for a data-gradient): conv1d_bf16x3_k7q.h.
extern "C" int sat_conv1d_bf16x3_planesq(const short* xp_hi, const short* xp_lo, int rows, const short* w_hi, const short* w_lo,
                                         const float* bias, const float* res, float* y, const float* x2, const float* alpha2,
                                         const float* beta2, float* part_da, float* part_db, int B, int Cin, int Cout, int Tin, int Tout,
                                         int K, int dil, int pad, int tanh_out, int flags, void* stream) {
    const SatBfShape s{SAT_BF_PLANES, B, Cin, Cout, Tin, Tout, K, 1, dil, pad, tanh_out, rows, flags};
    const SatBfOperands o{{}, {xp_hi, xp_lo}, w_hi, w_lo, {bias, res, y}, {x2, alpha2, beta2, part_da, part_db}, {}, {}};
    return sat_bf_run("sat_conv1d_bf16x3_planesq", s, o, SAT_NO_SPLIT, stream);
}
// sat_conv1d_bf16x3_planesq that may split its launch: ws / ws_floats / split as sat_conv1d_bf16x3_ws (sat_conv_bf16x3_split(2, ...)).  A split launch
// is one workgroup per (tile, split), whatever the persistence flags say.
extern "C" int sat_conv1d_bf16x3_planesq_ws(const short* xp_hi, const short* xp_lo, int rows, const short* w_hi, const short* w_lo,
                                            const float* bias, const float* res, float* y, const float* x2, const float* alpha2,
                                            const float* beta2, float* part_da, float* part_db, int B, int Cin, int Cout, int Tin, int Tout,
                                            int K, int dil, int pad, int tanh_out, int flags, float* ws, long long ws_floats, int split, void* stream) {
    const SatBfShape s{SAT_BF_PLANES, B, Cin, Cout, Tin, Tout, K, 1, dil, pad, tanh_out, rows, flags};
    const SatBfOperands o{{}, {xp_hi, xp_lo}, w_hi, w_lo, {bias, res, y}, {x2, alpha2, beta2, part_da, part_db}, {}, {}};
    return sat_bf_run("sat_conv1d_bf16x3_planesq_ws", s, o, SatSplitWs{ws, ws_floats, split, 0}, stream);
}

// The whole ResidualUnit forward in one launch (autoencoders.py:58-83), C <= 128 channels:
//   h = conv7(planes of snake1(x)) + bias1          (stored to `h` if given: the backward needs it)
//   y = x + conv1(snake2(h)) + bias2                 (+ optionally written as the NEXT unit's activation planes: em_*)
// xp_hi / xp_lo: activation planes of snake1(x) (sat_conv1d_k7_planes or a producer's emission); w7_*: sat_pack_weights_k7q(K, mode 0);
// w1_*: sat_pack_weights_k7q of the (C, C, 1) weight (K = 1, mode 0); a2 / ib2: sat_snake_consts of the second activation.
extern "C" int sat_residual_unit_fwd(const short* xp_hi, const short* xp_lo, int rows, const short* w7_hi, const short* w7_lo,
                                     const float* bias1, const float* a2, const float* ib2, const short* w1_hi, const short* w1_lo,
                                     const float* bias2, const float* x, float* h, float* y, int B, int C, int T, int K, int dil, int pad,
                                     void* em_hi, void* em_lo, const float* em_a, const float* em_ib, int em_rows, void* stream) {
    const SatBfShape s{SAT_BF_UNIT, B, C, C, T, T, K, 1, dil, pad, 0, rows, 0};
    const SatBfOperands o{{}, {xp_hi, xp_lo}, w7_hi, w7_lo, {bias1, x, y}, {}, {(short*)em_hi, (short*)em_lo, em_a, em_ib, em_rows},
                          {w1_hi, w1_lo, bias2, a2, ib2, h}};
    return sat_bf_run("sat_residual_unit_fwd", s, o, SAT_NO_SPLIT, stream);
}

// Same contract as sat_convtr1d (y[co][q*stride + k - pad] += W[ci][co][k] act(x)[ci][q], K == 2*stride, power-of-two
// stride), weights as sat_pack_weights_bf16x3 planes (mode 2).
extern "C" int sat_convtr1d_bf16x3(const float* x, const short* w_hi, const short* w_lo, const float* bias,
                                   const float* snake_a, const float* snake_ib, const float* res, float* y,
                                   const float* x2, const float* alpha2, const float* beta2, float* part_da,
                                   float* part_db, int B, int Cin, int Cout, int Tin, int Tout, int K, int stride,
                                   int pad, int tanh_out, void* stream) {
    const SatBfShape s{SAT_BF_CONVTR, B, Cin, Cout, Tin, Tout, K, stride, 1, pad, tanh_out, 0, 0};
    const SatBfOperands o{{x, snake_a, snake_ib}, {}, w_hi, w_lo, {bias, res, y}, {x2, alpha2, beta2, part_da, part_db}, {}, {}};
    return sat_bf_run("sat_convtr1d_bf16x3", s, o, SAT_NO_SPLIT, stream);
}
// sat_convtr1d_bf16x3 that may split its launch: ws / ws_floats / split as sat_conv1d_bf16x3_ws (sat_conv_bf16x3_split(1, ...))
extern "C" int sat_convtr1d_bf16x3_ws(const float* x, const short* w_hi, const short* w_lo, const float* bias,
                                      const float* snake_a, const float* snake_ib, const float* res, float* y,
                                      const float* x2, const float* alpha2, const float* beta2, float* part_da,
                                      float* part_db, int B, int Cin, int Cout, int Tin, int Tout, int K, int stride,
                                      int pad, int tanh_out, float* ws, long long ws_floats, int split, void* stream) {
    const SatBfShape s{SAT_BF_CONVTR, B, Cin, Cout, Tin, Tout, K, stride, 1, pad, tanh_out, 0, 0};
    const SatBfOperands o{{x, snake_a, snake_ib}, {}, w_hi, w_lo, {bias, res, y}, {x2, alpha2, beta2, part_da, part_db}, {}, {}};
    return sat_bf_run("sat_convtr1d_bf16x3_ws", s, o, SatSplitWs{ws, ws_floats, split, 0}, stream);
}

// How many ways the launch of a conv splits, and the workspace that takes: kind 0 = sat_conv1d_bf16x3, 1 = sat_convtr1d_bf16x3, 2 =
// sat_conv1d_bf16x3_planesq (stride ignored); the count does not depend on Tin.  split: -1 the rule (sat_conv_split_rule), 0 off,
// n >= 2 forced; cus: the CU count the rule assumes (<= 0: this device's).  Returns the split count (1: a plain launch), -1 where the shape is not
// served or a forced count is not possible; *ws_floats (may be NULL): floats of workspace the _ws entry point needs.  Host code only.
extern "C" int sat_conv_bf16x3_split(int kind, int B, int Cin, int Cout, int Tout, int K, int stride, int dil, int pad, int split, int cus,
                                     long long* ws_floats) {
    if (ws_floats) *ws_floats = 0;
    if (kind < SAT_BF_CONV || kind > SAT_BF_PLANES) { sat_set_error("sat_conv_bf16x3_split: kind 0 | 1 | 2"); return -1; }
    const SatBfShape s{kind, B, Cin, Cout, Tout, Tout, K, stride, dil, pad, 0, kind == SAT_BF_PLANES ? sat_conv1d_k7_plane_rows(Tout, Tout, pad) : 0, 0};
    SatBfPlan pl;
    SatConvBfLaunch a;
    if (sat_bf_geometry("sat_conv_bf16x3_split", s, &pl, &a)) return -1;
    int cps;
    long long need;
    const int n = sat_bf_split_decide(a, sat_bf_kernel(kind, pl, a), split, cus, &cps, &need);
    if (n < 0) { sat_set_error("sat_conv_bf16x3_split: this launch cannot be split that many ways"); return -1; }
    if (ws_floats) *ws_floats = need;
    return n;
}
// rows of the snake-gradient partial-sum planes written by sat_conv1d_bf16x3 (one per batch item and time tile of the launch's kernel)
extern "C" int sat_conv1d_bf16x3_partial_rows(int B, int Tout, int K, int stride) {
    const SatBfShape s{SAT_BF_CONV, B, 1, 1, Tout, Tout, K, stride, 1, 0, 0, 0, 0};
    SatBfPlan pl;
    SatConvBfLaunch a;
    if (sat_bf_geometry("sat_conv1d_bf16x3_partial_rows", s, &pl, &a)) return -1;
    return B * sat_cdiv(a.nq, sat_bf_kernel(s.kind, pl, a).t_t);
}
// (answers for any stride >= 1, as it always has: the transposed plan's kernel is the generic one at every stride)
extern "C" int sat_convtr1d_bf16x3_partial_rows(int B, int Tout, int stride, int pad) {
    if (B <= 0 || Tout <= 0 || stride < 1 || pad < 0) return -1;
    return B * sat_cdiv(sat_cdiv(Tout + pad, stride), sat_bf_kernel(SAT_BF_CONVTR, SatBfPlan{8, 4, 2}, SatConvBfLaunch{}).t_t);
}
