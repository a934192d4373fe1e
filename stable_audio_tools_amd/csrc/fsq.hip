// fsq.hip — the eval-mode quantiser of the dithered finite-scalar-quantisation bottleneck (models/fsq.py:64-107, models/bottleneck.py:426-484):
// sat_fsq_encode (latents -> codes and token ids) and sat_fsq_decode_tokens (token ids -> codes), one launch each, straight on the conv
// stack's (B, C, T) layout.  The reference transposes to (B, T, C), runs ~10 elementwise torch ops and a reduction over the digits, and
// transposes back.
//
// With levels L_0 .. L_{D-1}, Q codebooks and C = D * Q, channel q * D + d is digit d of codebook q.  Per element, in fp32 as torch does it:
//     z = tanh(x);  li = (z + 1) / half_l[d];  r = round-half-to-even(li);  code = r * half_l[d] - 1;  index = sum_d r_d * basis[d]
// half_l[d] = 2 / (L_d - 1) and table[d][r] = r * half_l[d] - 1 come from the HOST, computed by torch: the code is a table lookup, so it is
// the reference's two-rounding value (hipcc would contract r * h - 1 into one fma), and the only device arithmetic is tanhf, one add, one
// correctly rounded division (the compiler default: no fast-math flag on this file's build line, no reciprocal) and rintf (roundf rounds
// halves away from zero: x = 0 is an exact tie for every even L).  levels / half_l / basis / table ride in the kernel's by-value
// parameter struct (as sat_multi_copy's table): no device upload, no workspace, nothing a HIP-graph capture could trip over.
//
// One thread per (b, q, t), lanes along t: the D reads x[b, q * D + d, t] and the D writes codes[b, q * D + d, t] of a wave are 256-byte row
// segments; indices[b, t, q] (encode) / tokens[b, t, q] (decode) is one 8-byte access per thread.  256 threads per block, blocks numbered
// along blockIdx.x alone, every element offset 64-bit.  The loops over d hold no per-thread array (the next digit's x is prefetched into a
// scalar), so nothing lands in scratch; the table lookup is a per-lane load from the argument segment (2 KiB: L1-resident).
// Both kernels are bound by HBM and, at codec sizes, by the launch itself.
#include "sat_device.h"

#define SAT_FSQ_MAXD 16
#define SAT_FSQ_MAXTAB 512

struct SatFsqParams {
    const void* in;                 // encode: x fp32 (B, C, T); decode: tokens int64 (B, T, Q)
    float* codes;                   // (B, C, T)
    long long* indices;             // encode only: (B, T, Q)
    long long T, total;             // total = B * Q * T threads
    int D, Q;
    int levels[SAT_FSQ_MAXD];
    int off[SAT_FSQ_MAXD];          // first entry of digit d's table
    float half_l[SAT_FSQ_MAXD];
    long long basis[SAT_FSQ_MAXD];  // cumprod([1] + levels[:-1])
    float table[SAT_FSQ_MAXTAB];
};
static_assert(sizeof(SatFsqParams) <= 4096, "kernel arguments are limited to 4 KiB");

// thread n -> (b, q, t), t fastest; *row = first element of channel q * D of batch item b at time t, *tok = element (b, t, q)
SAT_DEVICE bool sat_fsq_thread(const SatFsqParams& p, long long* row, long long* tok) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= p.total) return false;
    const long long t = n % p.T, bq = n / p.T;
    const long long q = bq % p.Q, b = bq / p.Q;
    *row = bq * p.D * p.T + t;                      // (b * C + q * D) * T + t, C = D * Q
    *tok = (b * p.T + t) * p.Q + q;
    return true;
}

__global__ void __launch_bounds__(256) sat_fsq_encode_kernel(SatFsqParams p) {
    long long row, tok;
    if (!sat_fsq_thread(p, &row, &tok)) return;
    const float* x = (const float*)p.in + row;
    float* codes = p.codes + row;
    long long index = 0;
    float xv = x[0];
    for (int d = 0; d < SAT_FSQ_MAXD; ++d) {
        if (d >= p.D) break;
        const float xn = d + 1 < p.D ? x[(long long)(d + 1) * p.T] : 0.f;      // in flight under this digit's tanh
        const int top = p.levels[d] - 1;
        const float li = (tanhf(xv) + 1.0f) / p.half_l[d];
        // clamped as a float first: fmaxf(NaN, 0) = 0, so a NaN input reads table entry 0 and nothing is converted out of range
        const int r = (int)fminf(fmaxf(rintf(li), 0.f), (float)top);
        codes[(long long)d * p.T] = p.table[p.off[d] + r];
        index += (long long)r * p.basis[d];
        xv = xn;
    }
    p.indices[tok] = index;
}

__global__ void __launch_bounds__(256) sat_fsq_decode_kernel(SatFsqParams p) {
    long long row, tok;
    if (!sat_fsq_thread(p, &row, &tok)) return;
    float* codes = p.codes + row;
    // digit d = floor(token / basis[d]) mod L_d, floor division and a non-negative remainder as torch's // and % on int64; with
    // basis[d + 1] = basis[d] * L_d the quotients chain: floor(token / basis[d + 1]) = floor(floor(token / basis[d]) / L_d)
    long long cur = ((const long long*)p.in)[tok];
    for (int d = 0; d < SAT_FSQ_MAXD; ++d) {
        if (d >= p.D) break;
        const long long L = p.levels[d];
        long long nxt = cur / L, rem = cur % L;     // C++ truncates: move a negative remainder up by L, the quotient down by one
        if (rem < 0) { rem += L; --nxt; }
        const int r = (int)rem;                     // in [0, L)
        codes[(long long)d * p.T] = p.table[p.off[d] + r];
        cur = nxt;
    }
}

// fills everything but the pointers; 0 on success
static int sat_fsq_params(SatFsqParams* p, int B, int C, int T, int D, int Q, const int* levels, const float* half_l,
                          const float* table) {
    if (!levels || !table || B <= 0 || C <= 0 || T <= 0) { sat_set_error("sat_fsq_encode / sat_fsq_decode_tokens: bad arguments (B, C, T >= 1)"); return 1; }
    if (D < 1 || D > SAT_FSQ_MAXD) { sat_set_error("sat_fsq_encode / sat_fsq_decode_tokens: 1 <= D <= 16 levels"); return 1; }
    if (Q < 1 || (long long)D * Q != C) { sat_set_error("sat_fsq_encode / sat_fsq_decode_tokens: C == D * Q"); return 1; }
    int sum = 0;
    long long prod = 1;
    for (int d = 0; d < D; ++d) {
        const int L = levels[d];
        if (L < 2) { sat_set_error("sat_fsq_encode / sat_fsq_decode_tokens: every level count is >= 2"); return 1; }
        if (L > SAT_FSQ_MAXTAB || sum + L > SAT_FSQ_MAXTAB) { sat_set_error("sat_fsq_encode / sat_fsq_decode_tokens: sum of the levels <= 512"); return 1; }
        if (prod > 0x7fffffffffffffffLL / L) { sat_set_error("sat_fsq_encode / sat_fsq_decode_tokens: codebook size (product of the levels) <= 2^63 - 1"); return 1; }
        p->levels[d] = L;
        p->off[d] = sum;
        p->half_l[d] = half_l ? half_l[d] : 0.f;
        p->basis[d] = prod;
        sum += L;
        prod *= L;
    }
    for (int d = D; d < SAT_FSQ_MAXD; ++d) { p->levels[d] = 2; p->off[d] = 0; p->half_l[d] = 2.f; p->basis[d] = 0; }
    for (int i = 0; i < SAT_FSQ_MAXTAB; ++i) p->table[i] = i < sum ? table[i] : 0.f;
    p->T = T;
    p->total = (long long)B * Q * T;
    p->D = D;
    p->Q = Q;
    if (sat_cdivll(p->total, 256) > 0x7fffffffLL) { sat_set_error("sat_fsq_encode / sat_fsq_decode_tokens: more than 2^31 - 1 blocks of 256 (b, t, q)"); return 1; }
    return 0;
}

extern "C" int sat_fsq_encode(const float* x, float* codes, long long* indices, int B, int C, int T, int D, int Q, const int* levels,
                              const float* half_l, const float* table, void* stream) {
    SatFsqParams p;
    if (!half_l) { sat_set_error("sat_fsq_encode: no half_l"); return 1; }
    if (int rc = sat_fsq_params(&p, B, C, T, D, Q, levels, half_l, table)) return rc;
    if (!x || !codes || !indices) { sat_set_error("sat_fsq_encode: null tensor"); return 1; }
    p.in = x;
    p.codes = codes;
    p.indices = indices;
    SAT_LAUNCH(sat_fsq_encode_kernel, dim3((unsigned)sat_cdivll(p.total, 256)), dim3(256), stream, p);
    return sat_check_launch("sat_fsq_encode");
}

extern "C" int sat_fsq_decode_tokens(const long long* tokens, float* codes, int B, int C, int T, int D, int Q, const int* levels,
                                     const float* table, void* stream) {
    SatFsqParams p;
    if (int rc = sat_fsq_params(&p, B, C, T, D, Q, levels, nullptr, table)) return rc;
    if (!tokens || !codes) { sat_set_error("sat_fsq_decode_tokens: null tensor"); return 1; }
    p.in = tokens;
    p.codes = codes;
    p.indices = nullptr;
    SAT_LAUNCH(sat_fsq_decode_kernel, dim3((unsigned)sat_cdivll(p.total, 256)), dim3(256), stream, p);
    return sat_check_launch("sat_fsq_decode_tokens");
}
