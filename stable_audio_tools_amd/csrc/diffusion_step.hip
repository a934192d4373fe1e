// diffusion_step.hip — the front and the tail of the DiT optimisation step (training.DiTTrainStep, restating
// DiffusionCondTrainingWrapper.training_step, training/diffusion.py:332-487):
//   sat_diffusion_noise   alphas / sigmas of the drawn timesteps, noised = x*alpha + noise*sigma and the v / rectified-flow targets
//                         (:377-379, :406-420) in one pass over x and noise
//   sat_diffusion_noise_inpaint  the same, plus the inpainting conditioning of :429-438 (models/inpainting.py:11-97) from a device
//                         table of masked intervals: the mask channel and the masked, scaled latent, in the same pass
//   sat_masked_mse_fwd    MSELoss with mask_key="padding_mask" (training/losses/losses.py:76-89): the mean of (out - targets)^2 over the
//                         SELECTED elements, without the host sync of the reference's boolean indexing
//   sat_masked_mse_bwd    its gradient, zero at masked positions
// No atomics: every reduction is a set of write-once partials summed in a fixed order, so a step is bit-reproducible run to run, and
// nothing here reads the device from the host, so the step stays capturable.  dtype: 0 = fp32, 1 = bf16 `out` / `dout` (math in fp32).
#include <cstdio>
#include "sat_device.h"

template <typename T> struct SatStepIO;
template <> struct SatStepIO<float> {
    static SAT_DEVICE float ld(const void* p, long long i) { return ((const float*)p)[i]; }
    static SAT_DEVICE void st(void* p, long long i, float v) { ((float*)p)[i] = v; }
};
template <> struct SatStepIO<short> {
    static SAT_DEVICE float ld(const void* p, long long i) { return sat_bf16_to_f32(((const short*)p)[i]); }
    static SAT_DEVICE void st(void* p, long long i, float v) { ((short*)p)[i] = sat_f32_to_bf16(v); }
};

// ------------------------------------------------------------------------------------------------
// noising + targets.  grid (chunks of a row, B): a workgroup stays inside one batch row, so alpha / sigma are evaluated ONCE per
// workgroup (accurate cosf / sinf: two transcendental expansions per ELEMENT would make this memory-bound pass VALU-bound).
// ------------------------------------------------------------------------------------------------
struct SatNoiseParams {
    const float* x;       // (B, per)
    const float* noise;   // (B, per)
    const float* t;       // (B)
    float* noised;        // (B, per)
    float* targets;       // (B, per)
    long long per;        // C * T
    float inv_scale;      // 1 / latent scale, applied to x first
    int objective;        // 0: v, 1: rectified flow
};

SAT_DEVICE void sat_noise_one(float xv, float nz, float alpha, float sigma, float inv_scale, int objective, float* noised, float* target) {
    const float xs = xv * inv_scale;
    *noised = xs * alpha + nz * sigma;
    *target = objective == 0 ? nz * alpha - xs * sigma : nz - xs;
}

// alpha / sigma of batch row b into ab[0], ab[1] (thread 0); the caller's __syncthreads() publishes them
SAT_DEVICE void sat_noise_alpha_sigma(const float* t, int b, int objective, float* ab) {
    if (threadIdx.x == 0) {
        const float tb = t[b];
        if (objective == 0) {
            const float ang = tb * 1.57079632679489662f;       // t * pi / 2
            ab[0] = cosf(ang);
            ab[1] = sinf(ang);
        } else {
            ab[0] = 1.0f - tb;
            ab[1] = tb;
        }
    }
}

__global__ void __launch_bounds__(256) sat_diffusion_noise_kernel(SatNoiseParams p) {
    __shared__ float ab[2];
    const int b = blockIdx.y;
    sat_noise_alpha_sigma(p.t, b, p.objective, ab);
    __syncthreads();
    const float alpha = ab[0], sigma = ab[1];
    const long long off = (long long)b * p.per;
    const float* x = p.x + off;
    const float* nz = p.noise + off;
    float* noised = p.noised + off;
    float* targets = p.targets + off;
    // 16-byte accesses where the row offset allows: the four rows must sit at the same offset inside a 16-byte line (they do whenever the
    // tensors' bases are aligned alike); `head` scalar elements lead up to the first aligned one, < 4 trail the last whole vector
    const unsigned mis = (unsigned)((uintptr_t)x & 15);
    const bool same = (mis & 3) == 0 && ((uintptr_t)nz & 15) == mis && ((uintptr_t)noised & 15) == mis && ((uintptr_t)targets & 15) == mis;
    long long head = same ? (long long)(((16u - mis) & 15u) >> 2) : p.per;
    if (head > p.per) head = p.per;
    const long long nvec = (p.per - head) >> 2;
    const long long tail0 = head + 4 * nvec;
    const long long stride = (long long)gridDim.x * 256;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
        const long long i = head + 4 * v;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i);
        const f32x4 nv = *reinterpret_cast<const f32x4*>(nz + i);
        f32x4 o, g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a, c;
            sat_noise_one(xv[e], nv[e], alpha, sigma, p.inv_scale, p.objective, &a, &c);
            o[e] = a;
            g[e] = c;
        }
        *reinterpret_cast<f32x4*>(noised + i) = o;
        *reinterpret_cast<f32x4*>(targets + i) = g;
    }
    const long long nscalar = head + (p.per - tail0);
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < nscalar; k += stride) {
        const long long i = k < head ? k : tail0 + (k - head);
        float a, c;
        sat_noise_one(x[i], nz[i], alpha, sigma, p.inv_scale, p.objective, &a, &c);
        noised[i] = a;
        targets[i] = c;
    }
}

extern "C" int sat_diffusion_noise(const float* x, const float* noise, const float* t, float* noised, float* targets, int B, int C, int T,
                                   int objective, float inv_scale, void* stream) {
    if (B <= 0 || C <= 0 || T <= 0) { sat_set_error("sat_diffusion_noise: empty shape"); return 1; }
    if (B > 65535) { sat_set_error("sat_diffusion_noise: B > 65535"); return 1; }
    if (objective != 0 && objective != 1) { sat_set_error("sat_diffusion_noise: objective must be 0 (v) or 1 (rectified flow)"); return 1; }
    if (!x || !noise || !t || !noised || !targets) { sat_set_error("sat_diffusion_noise: null tensor"); return 1; }
    SatNoiseParams p{x, noise, t, noised, targets, (long long)C * T, inv_scale, objective};
    long long nx = sat_cdivll(p.per, 4096);            // 16 elements per thread and pass
    if (nx > 1024) nx = 1024;
    SAT_LAUNCH(sat_diffusion_noise_kernel, dim3((unsigned)nx, (unsigned)B), dim3(256), stream, p);
    return sat_check_launch("sat_diffusion_noise");
}

// ------------------------------------------------------------------------------------------------
// noising + targets + inpainting conditioning.  Same grid, same arithmetic for noised / targets (sat_noise_one, sat_noise_alpha_sigma:
// bit-equal to sat_diffusion_noise).  Item b's S intervals [start, end) are loaded into LDS once per workgroup; every lane reads the same
// interval at the same time (an LDS broadcast).  An element's time index is its position modulo T inside its row of C*T.  The masked
// latent is a SELECT between x * inv_scale and +0: an inf / nan inside an inpainted interval does not reach the conditioning.  A batch
// row of `concat` is (1 + C) * T floats, so its masked-latent block may sit at another offset inside a 16-byte line than the row of x:
// it is then written with scalar stores from the same registers.  The intervals are only compared with, never indexed by.
// ------------------------------------------------------------------------------------------------
#define SAT_INPAINT_MAX_SEGS 256

struct SatInpaintParams {
    SatNoiseParams n;
    const int* segments;  // (B, S, 2)
    float* mask;          // mask channel of batch row 0: (B, T) with row stride crow
    float* masked;        // masked latent of batch row 0: (B, C * T) with row stride crow
    long long crow;       // (1 + C) * T
    int T, S;
};

SAT_DEVICE bool sat_inpaint_keep(const int* seg, int S, int tt) {
    bool hit = false;
    for (int s = 0; s < S; ++s) hit |= tt >= seg[2 * s] && tt < seg[2 * s + 1];
    return !hit;
}

__global__ void __launch_bounds__(256) sat_diffusion_noise_inpaint_kernel(SatInpaintParams q) {
    __shared__ float ab[2];
    __shared__ int seg[2 * SAT_INPAINT_MAX_SEGS];
    const SatNoiseParams& p = q.n;
    const int b = blockIdx.y;
    sat_noise_alpha_sigma(p.t, b, p.objective, ab);
    for (int k = threadIdx.x; k < 2 * q.S; k += 256) seg[k] = q.segments[(long long)b * 2 * q.S + k];
    __syncthreads();
    const float alpha = ab[0], sigma = ab[1];
    const long long off = (long long)b * p.per;
    const float* x = p.x + off;
    const float* nz = p.noise + off;
    float* noised = p.noised + off;
    float* targets = p.targets + off;
    float* masked = q.masked + (long long)b * q.crow;
    float* mk = q.mask + (long long)b * q.crow;
    const long long stride = (long long)gridDim.x * 256;
    const long long first = (long long)blockIdx.x * 256 + threadIdx.x;
    // the mask channel: T of the row's (1 + C) * T floats
    for (long long j = first; j < q.T; j += stride) mk[j] = sat_inpaint_keep(seg, q.S, (int)j) ? 1.0f : 0.0f;
    // head / vector body / tail as in sat_diffusion_noise_kernel, decided by the four (B, C, T) tensors
    const unsigned mis = (unsigned)((uintptr_t)x & 15);
    const bool same = (mis & 3) == 0 && ((uintptr_t)nz & 15) == mis && ((uintptr_t)noised & 15) == mis && ((uintptr_t)targets & 15) == mis;
    const bool mvec = ((uintptr_t)masked & 15) == mis;
    long long head = same ? (long long)(((16u - mis) & 15u) >> 2) : p.per;
    if (head > p.per) head = p.per;
    const long long nvec = (p.per - head) >> 2;
    const long long tail0 = head + 4 * nvec;
    for (long long v = first; v < nvec; v += stride) {
        const long long i = head + 4 * v;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i);
        const f32x4 nv = *reinterpret_cast<const f32x4*>(nz + i);
        int tt[4];
        tt[0] = (int)(i % q.T);
#pragma unroll
        for (int e = 1; e < 4; ++e) tt[e] = tt[e - 1] + 1 == q.T ? 0 : tt[e - 1] + 1;
        bool hit[4] = {false, false, false, false};
        for (int s = 0; s < q.S; ++s) {
            const int lo = seg[2 * s], hi = seg[2 * s + 1];
#pragma unroll
            for (int e = 0; e < 4; ++e) hit[e] |= tt[e] >= lo && tt[e] < hi;
        }
        f32x4 o, g, m;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a, c;
            sat_noise_one(xv[e], nv[e], alpha, sigma, p.inv_scale, p.objective, &a, &c);
            o[e] = a;
            g[e] = c;
            m[e] = hit[e] ? 0.0f : xv[e] * p.inv_scale;
        }
        *reinterpret_cast<f32x4*>(noised + i) = o;
        *reinterpret_cast<f32x4*>(targets + i) = g;
        if (mvec) {
            *reinterpret_cast<f32x4*>(masked + i) = m;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) masked[i + e] = m[e];
        }
    }
    const long long nscalar = head + (p.per - tail0);
    for (long long k = first; k < nscalar; k += stride) {
        const long long i = k < head ? k : tail0 + (k - head);
        float a, c;
        sat_noise_one(x[i], nz[i], alpha, sigma, p.inv_scale, p.objective, &a, &c);
        noised[i] = a;
        targets[i] = c;
        masked[i] = sat_inpaint_keep(seg, q.S, (int)(i % q.T)) ? x[i] * p.inv_scale : 0.0f;
    }
}

extern "C" int sat_diffusion_noise_inpaint(const float* x, const float* noise, const float* t, const int* segments, float* noised,
                                           float* targets, float* concat, int B, int C, int T, int S, int objective, float inv_scale,
                                           int mask_first, void* stream) {
    if (B <= 0 || C <= 0 || T <= 0) { sat_set_error("sat_diffusion_noise_inpaint: empty shape"); return 1; }
    if (B > 65535) { sat_set_error("sat_diffusion_noise_inpaint: B > 65535"); return 1; }
    if (S <= 0) { sat_set_error("sat_diffusion_noise_inpaint: S <= 0"); return 1; }
    if (S > SAT_INPAINT_MAX_SEGS) { sat_set_error("sat_diffusion_noise_inpaint: S > 256"); return 1; }
    if (objective != 0 && objective != 1) { sat_set_error("sat_diffusion_noise_inpaint: objective must be 0 (v) or 1 (rectified flow)"); return 1; }
    if (!x || !noise || !t || !segments || !noised || !targets || !concat) { sat_set_error("sat_diffusion_noise_inpaint: null tensor"); return 1; }
    SatInpaintParams q{};
    q.n = SatNoiseParams{x, noise, t, noised, targets, (long long)C * T, inv_scale, objective};
    q.segments = segments;
    q.mask = mask_first ? concat : concat + q.n.per;
    q.masked = mask_first ? concat + T : concat;
    q.crow = q.n.per + T;
    q.T = T;
    q.S = S;
    long long nx = sat_cdivll(q.n.per, 4096);
    if (nx > 1024) nx = 1024;
    SAT_LAUNCH(sat_diffusion_noise_inpaint_kernel, dim3((unsigned)nx, (unsigned)B), dim3(256), stream, q);
    return sat_check_launch("sat_diffusion_noise_inpaint");
}

// ------------------------------------------------------------------------------------------------
// masked MSE.  A work item is 1024 consecutive time steps of one (b, c) row; workgroup g takes items g, g + G, ... and leaves one partial
// sum and one integer count; a second one-workgroup launch adds the partials in index order and writes (loss, count).  Masked elements are
// SKIPPED (never multiplied by zero): an inf / nan there does not reach the loss.
// ------------------------------------------------------------------------------------------------
#define SAT_MSE_CHUNK 1024
#define SAT_MSE_MAX_BLOCKS 1024

struct SatMseParams {
    const void* out;            // (B, C, T) fp32 | bf16
    const float* targets;       // (B, C, T)
    const unsigned char* mask;  // (B, T) bytes, non-zero = selected; NULL: every element
    float* psum;                // [nblocks] fwd partial sums
    int* pcnt;                  // [nblocks] fwd partial counts
    float* res;                 // fwd out / bwd in: (loss, count)
    const float* gloss;         // bwd: dL/dloss, device scalar
    void* dout;                 // bwd out, dtype of `out`
    long long items;            // B * C * chunks
    int nblocks;
    int B, C, T, chunks;        // chunks = ceil(T / 1024)
};

SAT_DEVICE float sat_step_block_sum(float s, float* red) {
    s = sat_wave_sum(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

template <typename T>
__global__ void __launch_bounds__(256) sat_masked_mse_fwd_kernel(SatMseParams p) {
    __shared__ float red[4];
    __shared__ int cnts[256];
    float s = 0.f;
    int n = 0;
    for (long long w = blockIdx.x; w < p.items; w += gridDim.x) {
        const long long row = w / p.chunks;                    // b * C + c
        const int t0 = (int)(w - row * p.chunks) * SAT_MSE_CHUNK;
        const long long base = row * p.T;
        const unsigned char* m = p.mask ? p.mask + (row / p.C) * p.T : nullptr;
#pragma unroll
        for (int k = 0; k < SAT_MSE_CHUNK / 256; ++k) {
            const int t = t0 + k * 256 + (int)threadIdx.x;
            if (t < p.T && (m == nullptr || m[t] != 0)) {
                const float d = SatStepIO<T>::ld(p.out, base + t) - p.targets[base + t];
                s += d * d;
                ++n;
            }
        }
    }
    s = sat_step_block_sum(s, red);
    cnts[threadIdx.x] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int i = 0; i < 256; ++i) c += cnts[i];
        p.psum[blockIdx.x] = s;
        p.pcnt[blockIdx.x] = c;
    }
}

// one workgroup: loss = sum(psum) / sum(pcnt); an empty selection gives 0 / 0 = NaN, as the reference's mean of nothing
__global__ void __launch_bounds__(256) sat_masked_mse_finish_kernel(SatMseParams p) {
    __shared__ float red[4];
    __shared__ long long cnts[256];
    float s = 0.f;
    long long n = 0;
    for (int i = threadIdx.x; i < p.nblocks; i += 256) {
        s += p.psum[i];
        n += p.pcnt[i];
    }
    s = sat_step_block_sum(s, red);
    cnts[threadIdx.x] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long c = 0;
        for (int i = 0; i < 256; ++i) c += cnts[i];
        const float cf = (float)c;
        p.res[0] = s / cf;
        p.res[1] = cf;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) sat_masked_mse_bwd_kernel(SatMseParams p) {
    const float coef = 2.0f * p.gloss[0] / p.res[1];
    for (long long w = blockIdx.x; w < p.items; w += gridDim.x) {
        const long long row = w / p.chunks;
        const int t0 = (int)(w - row * p.chunks) * SAT_MSE_CHUNK;
        const long long base = row * p.T;
        const unsigned char* m = p.mask ? p.mask + (row / p.C) * p.T : nullptr;
#pragma unroll
        for (int k = 0; k < SAT_MSE_CHUNK / 256; ++k) {
            const int t = t0 + k * 256 + (int)threadIdx.x;
            if (t >= p.T) continue;
            float g = 0.f;                                     // masked: exactly 0, whatever coef is (count 0 makes it inf / nan)
            if (m == nullptr || m[t] != 0) g = (SatStepIO<T>::ld(p.out, base + t) - p.targets[base + t]) * coef;
            SatStepIO<T>::st(p.dout, base + t, g);
        }
    }
}

static int sat_mse_check(const char* who, const void* out, const float* targets, const void* other, int B, int C, int T, int dtype) {
    char buf[160];
    const char* why = nullptr;
    if (B <= 0 || C <= 0 || T <= 0) why = "empty shape";
    else if (dtype != 0 && dtype != 1) why = "dtype must be 0 (f32) or 1 (bf16)";
    else if (!out || !targets || !other) why = "null tensor";
    if (!why) return 0;
    snprintf(buf, sizeof(buf), "%s: %s", who, why);
    sat_set_error(buf);
    return 1;
}
static SatMseParams sat_mse_params(int B, int C, int T) {
    SatMseParams p{};
    p.B = B; p.C = C; p.T = T;
    p.chunks = sat_cdiv(T, SAT_MSE_CHUNK);
    p.items = (long long)B * C * p.chunks;
    p.nblocks = (int)(p.items < SAT_MSE_MAX_BLOCKS ? p.items : SAT_MSE_MAX_BLOCKS);
    return p;
}

extern "C" int sat_masked_mse_nblocks(int B, int C, int T) {
    if (B <= 0 || C <= 0 || T <= 0) return -1;
    return sat_mse_params(B, C, T).nblocks;
}

extern "C" int sat_masked_mse_fwd(const void* out, const float* targets, const unsigned char* mask, float* work, float* res, int B, int C,
                                  int T, int dtype, void* stream) {
    if (sat_mse_check("sat_masked_mse_fwd", out, targets, res, B, C, T, dtype)) return 1;
    if (!work) { sat_set_error("sat_masked_mse_fwd: null workspace (2 * sat_masked_mse_nblocks words)"); return 1; }
    SatMseParams p = sat_mse_params(B, C, T);
    p.out = out; p.targets = targets; p.mask = mask; p.res = res;
    p.psum = work;
    p.pcnt = reinterpret_cast<int*>(work + p.nblocks);
    if (dtype == 0) SAT_LAUNCH(sat_masked_mse_fwd_kernel<float>, dim3(p.nblocks), dim3(256), stream, p);
    else SAT_LAUNCH(sat_masked_mse_fwd_kernel<short>, dim3(p.nblocks), dim3(256), stream, p);
    if (sat_check_launch("sat_masked_mse_fwd")) return 2;
    SAT_LAUNCH(sat_masked_mse_finish_kernel, dim3(1), dim3(256), stream, p);
    return sat_check_launch("sat_masked_mse_fwd (finish)");
}

extern "C" int sat_masked_mse_bwd(const void* out, const float* targets, const unsigned char* mask, const float* res, const float* gloss,
                                  void* dout, int B, int C, int T, int dtype, void* stream) {
    if (sat_mse_check("sat_masked_mse_bwd", out, targets, dout, B, C, T, dtype)) return 1;
    if (!res || !gloss) { sat_set_error("sat_masked_mse_bwd: null result / gloss"); return 1; }
    SatMseParams p = sat_mse_params(B, C, T);
    p.out = out; p.targets = targets; p.mask = mask; p.res = const_cast<float*>(res); p.gloss = gloss; p.dout = dout;
    if (dtype == 0) SAT_LAUNCH(sat_masked_mse_bwd_kernel<float>, dim3(p.nblocks), dim3(256), stream, p);
    else SAT_LAUNCH(sat_masked_mse_bwd_kernel<short>, dim3(p.nblocks), dim3(256), stream, p);
    return sat_check_launch("sat_masked_mse_bwd");
}
