// layout.hip — the junction between the conv stack's (B, C, T) fp32 layout and the transformer's (B, N, D) token layout
// (TAAEBlock's Transpose modules, models/autoencoders.py:85-89, :101, :117): sat_ct_to_tokens and sat_tokens_to_ct.
//
// Both are one batched matrix transpose, (B, R, Cc) -> (B, Cc, R), with an optional bf16 rounding on the way out (round to nearest
// even: sat_cvt2_pk / sat_f32_to_bf16, the rounding of sat_cast_bf16) or a bf16 widening on the way in.  One launch, no workspace, one
// workgroup of 256 threads per 64 x 64 tile, tiles numbered along blockIdx.x only (the tile count of one dim passes 65535 at the
// Oobleck item length); every element offset is 64-bit.
//
// Global side: a lane moves one 16-byte chunk (4 fp32 or 8 bf16) of a row, on both sides, when the vector path applies: both bases
// 16-byte aligned, the source's contiguous dim a multiple of its chunk and the destination's contiguous dim a multiple of its chunk
// (for ct_to_tokens to bf16: T % 4 == 0, C % 8 == 0).  A chunk is then wholly inside the matrix or wholly outside.  Everything else
// takes the scalar edge path: the same tile walk with per-element bounds checks.
//
// LDS side: the tile is fp32, tile[r][c] with a row stride of 65 words, moved with 4-byte LDS accesses (ds_write_b32 / ds_read_b32:
// banked by (byte / 4) mod 32 and served per 32-lane half; an odd stride rules 16-byte LDS accesses out, and a stride that is a
// multiple of 4 words puts a column walk on 8 banks).  65 mod 32 = 1, so word (r, c) lies on bank (r + c) mod 32.  With W the chunk
// width in elements, a 32-lane half holds 32 / W chunks of one row segment times W consecutive rows:
//   write of element e: lanes at (row r0 + j, column W * i + e), j < W, i < 32 / W  -> banks W * i + j + const: 32 distinct banks;
//   read  of element e: lanes at (row W * i + e, column c0 + j)                       -> the same set: 32 distinct banks.
// Expected conflict degree: 1 (conflict-free) on both sides, for W = 4 and W = 8.  The two halves of a wave cover the two halves of
// the same 64-element row segments, so a wave's global access is W rows x 256 B (fp32) or W rows x 128 B (bf16).
// The kernel is bound by HBM: 32 KiB of traffic per tile against ~400 LDS cycles.
#include "sat_device.h"

struct SatLayoutParams {
    const void* src;
    void* dst;
    long long R, Cc;                // source matrix: R rows of Cc contiguous elements; destination: Cc rows of R
    long long tiles_r, tiles_c;     // ceil(R / 64), ceil(Cc / 64)
    int vec;                        // 16-byte global accesses on both sides
};

// lane -> (chunk of the 64-element row segment, row among the W rows a half-wave covers)
template <int W>
SAT_DEVICE void sat_layout_lane(int lane, int* chunk, int* row) {
    constexpr int HALF = 32 / W;                       // chunks per half row segment
    *chunk = (lane & 31) % HALF + HALF * (lane >> 5);
    *row = (lane & 31) / HALF;
}

template <bool SRC_BF16, bool DST_BF16>
__global__ void __launch_bounds__(256) sat_layout_transpose_kernel(SatLayoutParams p) {
    constexpr int WS = SRC_BF16 ? 8 : 4, WD = DST_BF16 ? 8 : 4;
    __shared__ float tile[64][65];
    const long long L = blockIdx.x;
    const long long tcx = L % p.tiles_c, rest = L / p.tiles_c;
    const long long trx = rest % p.tiles_r, b = rest / p.tiles_r;
    const long long r0 = trx * 64, c0 = tcx * 64;
    const long long plane = p.R * p.Cc;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    {   // ---- source rows -> tile[r][c]
        int ch, rw;
        sat_layout_lane<WS>(lane, &ch, &rw);
        for (int pass = 0; pass < 64 / (4 * WS); ++pass) {
            const int rr = pass * 4 * WS + wave * WS + rw;
            const long long r = r0 + rr, c = c0 + ch * WS;
            float v[WS];
            for (int e = 0; e < WS; ++e) v[e] = 0.f;
            if (r < p.R && c < p.Cc) {
                const long long off = b * plane + r * p.Cc + c;
                if (p.vec) {
                    if constexpr (SRC_BF16) {
                        const u32x4 q = *(const u32x4*)((const short*)p.src + off);
                        for (int e = 0; e < 4; ++e) {
                            v[2 * e] = sat_bf16_to_f32((short)(q[e] & 0xffffu));
                            v[2 * e + 1] = sat_bf16_to_f32((short)(q[e] >> 16));
                        }
                    } else {
                        const f32x4 q = *(const f32x4*)((const float*)p.src + off);
                        for (int e = 0; e < 4; ++e) v[e] = q[e];
                    }
                } else {
                    for (int e = 0; e < WS; ++e) {
                        if (c + e >= p.Cc) break;
                        if constexpr (SRC_BF16) v[e] = sat_bf16_to_f32(((const short*)p.src)[off + e]);
                        else v[e] = ((const float*)p.src)[off + e];
                    }
                }
            }
            for (int e = 0; e < WS; ++e) tile[rr][ch * WS + e] = v[e];
        }
    }
    __syncthreads();
    {   // ---- tile columns -> destination rows
        int ch, rw;
        sat_layout_lane<WD>(lane, &ch, &rw);
        for (int pass = 0; pass < 64 / (4 * WD); ++pass) {
            const int cc = pass * 4 * WD + wave * WD + rw;          // destination row inside the tile = source column
            const long long c = c0 + cc, r = r0 + ch * WD;          // destination row, first destination column
            if (c >= p.Cc || r >= p.R) continue;
            float v[WD];
            for (int e = 0; e < WD; ++e) v[e] = tile[ch * WD + e][cc];
            const long long off = b * plane + c * p.R + r;
            if (p.vec) {
                if constexpr (DST_BF16) {
                    u32x4 q;
                    for (int e = 0; e < 4; ++e) q[e] = sat_cvt2_pk(v[2 * e], v[2 * e + 1]);
                    *(u32x4*)((short*)p.dst + off) = q;
                } else {
                    f32x4 q;
                    for (int e = 0; e < 4; ++e) q[e] = v[e];
                    *(f32x4*)((float*)p.dst + off) = q;
                }
            } else {
                for (int e = 0; e < WD; ++e) {
                    if (r + e >= p.R) break;
                    if constexpr (DST_BF16) ((short*)p.dst)[off + e] = sat_f32_to_bf16(v[e]);
                    else ((float*)p.dst)[off + e] = v[e];
                }
            }
        }
    }
}

// (B, R, Cc) -> (B, Cc, R); fp32 -> fp32 | bf16, or bf16 -> fp32
static int sat_layout_transpose(const char* who, const void* src, void* dst, int B, long long R, long long Cc, int src_bf16, int dst_bf16,
                                void* stream) {
    if (!src || !dst || B <= 0 || R <= 0 || Cc <= 0) { sat_set_error("sat_ct_to_tokens / sat_tokens_to_ct: bad arguments (B, C, T >= 1)"); return 1; }
    const long long tiles_r = sat_cdivll(R, 64), tiles_c = sat_cdivll(Cc, 64);
    const long long tiles = (long long)B * tiles_r * tiles_c;
    if (tiles > 0x7fffffffLL) { sat_set_error("sat_ct_to_tokens / sat_tokens_to_ct: more than 2^31 - 1 tiles of 64 x 64"); return 1; }
    const int ws = src_bf16 ? 8 : 4, wd = dst_bf16 ? 8 : 4;
    const bool vec = ((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0) && (Cc % ws == 0) && (R % wd == 0);
    SatLayoutParams p{src, dst, R, Cc, tiles_r, tiles_c, vec ? 1 : 0};
    const dim3 grid((unsigned)tiles), block(256);
    if (src_bf16) { SAT_LAUNCH((sat_layout_transpose_kernel<true, false>), grid, block, stream, p); }
    else if (dst_bf16) { SAT_LAUNCH((sat_layout_transpose_kernel<false, true>), grid, block, stream, p); }
    else { SAT_LAUNCH((sat_layout_transpose_kernel<false, false>), grid, block, stream, p); }
    return sat_check_launch(who);
}

extern "C" int sat_ct_to_tokens(const float* x, void* y, int B, int C, int T, int out_bf16, void* stream) {
    return sat_layout_transpose("sat_ct_to_tokens", x, y, B, C, T, 0, out_bf16 ? 1 : 0, stream);
}

extern "C" int sat_tokens_to_ct(const void* x, float* y, int B, int C, int T, int in_bf16, void* stream) {
    return sat_layout_transpose("sat_tokens_to_ct", x, y, B, T, C, in_bf16 ? 1 : 0, 0, stream);
}
