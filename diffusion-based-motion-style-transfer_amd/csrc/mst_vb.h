// The variational-bound evaluation (reference diffusion/gaussian_diffusion.py:1281-1314 `_vb_terms_bpd`, :1529-1545 `_prior_bpd`,
// :1547-1602 `calc_bpd_loop`; diffusion/losses.py:12-77) on timestep-batched ROWS.
//
// A row r is one pair (clip[r], t[r]): the loop's T timesteps are independent, so (clip, timestep) pairs are packed into full model
// batches in any order.  x_start / mask / motion are per CLIP ([N, F, 1, T], gathered by clip[r]); x_t, the model output, a noise
// buffer and the stored x0-hat are per ROW ([R, F, 1, T]).
//
//   k_vb_diffuse   x_t[r] = sqrt_ac[t] x0[clip] + sqrt_1m_ac[t] z (1 - m[clip]): k_q_sample's expression on gathered operands.
//   k_vb_terms     out[r] = (vb term in bits, mean (x0hat - x0)^2, mean (eps - z)^2, rms x0hat); x0-hat optionally stored.
//   k_vb_prior     out[n] = mean_flat(normal_kl(sqrt_ac[T-1] x0, log(1 - ac[T-1]), 0, 0)) / ln 2.
//
// z is read from a buffer [R, ...] or drawn here: element (f, l) of row r is component l & 3 of philox_normal4(l >> 2, f, clip[r], t[r]),
// i.e. mst_philox_normal(N, F, T, seed, step = t[r])[clip[r]] -- the noise of a (clip, timestep) pair does not depend on the packing.
//
// Reductions: every thread adds its elements in index order into doubles, a wave folds them with a fixed shuffle tree, thread 0 adds the
// waves' sums in wave order.  No atomics, one workgroup per row: a row's numbers are the same bits wherever the row sits in the launch.
// Every access is base + i with i < per_clip (element loops) or a guarded frame index (quad loops): nothing reads or writes past a row at
// per_clip not a multiple of 4 or of the workgroup size.
#pragma once

namespace mst {

constexpr int VB_THREADS = 1024;          // one workgroup per row; 16 waves keep enough loads in flight for a 263 x 196 row (docs/LAB_NOTES.md)
constexpr double VB_LN2 = 0.69314718055994530942;

// x_t of rows from a noise buffer: the loop, expression and rounding order of k_q_sample with x0 / mask gathered by clip.
__global__ void k_vb_diffuse(const float* __restrict__ tab, int nsteps, const float* __restrict__ x0, const float* __restrict__ noise,
                             const float* __restrict__ mask, const long long* __restrict__ clip, const long long* __restrict__ t,
                             long long per_clip, float* __restrict__ out) {
    const int row = blockIdx.y;
    const int tt = (int)t[row];
    const float a = tab[TAB_SQRT_AC * nsteps + tt], b = tab[TAB_SQRT_1M_AC * nsteps + tt];
    const size_t base = (size_t)row * per_clip, cbase = (size_t)clip[row] * per_clip;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < per_clip; i += (long long)gridDim.x * blockDim.x) {
        float n = noise[base + i];
        if (mask) n = n * (1.0f - mask[cbase + i]);
        out[base + i] = a * x0[cbase + i] + b * n;
    }
}

// the same with z drawn: one thread per quad of frames (k_philox_normal's mapping and counter)
__global__ void k_vb_diffuse_draw(const float* __restrict__ tab, int nsteps, const float* __restrict__ x0, const float* __restrict__ mask,
                                  const long long* __restrict__ clip, const long long* __restrict__ t, int F, int T,
                                  unsigned long long seed, float* __restrict__ out) {
    const int row = blockIdx.y;
    const int tt = (int)t[row];
    const long long c = clip[row];
    const float a = tab[TAB_SQRT_AC * nsteps + tt], b = tab[TAB_SQRT_1M_AC * nsteps + tt];
    const size_t base = (size_t)row * F * T, cbase = (size_t)c * F * T;
    const int TQ = (T + 3) >> 2;
    const long long quads = (long long)F * TQ;          // (a 64-bit index: i + the grid's stride may pass 2^31 on the last trip)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < quads; i += (long long)gridDim.x * blockDim.x) {
        const int f = (int)(i / TQ), tq = (int)(i - (long long)f * TQ);
        float z[4];
        philox_normal4((unsigned)tq, (unsigned)f, (unsigned)c, (unsigned)tt, seed, z);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int l = tq * 4 + j;
            if (l < T) {
                const size_t e = (size_t)f * T + l;
                float n = z[j];
                if (mask) n = n * (1.0f - mask[cbase + e]);
                out[base + e] = a * x0[cbase + e] + b * n;
            }
        }
    }
}

// K sums of a workgroup in a fixed order: lanes by the xor tree, then waves 0, 1, ... in wave order.  Valid in thread 0 on return.
template <int K>
__device__ __forceinline__ void vb_block_sum(double (&s)[K]) {
    __shared__ double part[VB_THREADS / 64][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) part[wave][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = blockDim.x >> 6;
#pragma unroll
        for (int k = 0; k < K; k++) {
            double a = part[0][k];
            for (int w = 1; w < nw; w++) a += part[w][k];
            s[k] = a;
        }
    }
}

// approx_standard_normal_cdf (losses.py:42-47) in double
__device__ __forceinline__ double vb_cdf(double x) {
    return 0.5 * (1.0 + tanh(0.79788456080286535588 * (x + 0.044715 * (x * x * x))));
}
// minus discretized_gaussian_log_likelihood (losses.py:50-77) of one element, in double: cdf_plus - cdf_min cancels in fp32
__device__ __forceinline__ double vb_decoder_nll(float x, double mean, double log_scale) {
    const double centered = (double)x - mean;
    const double inv_stdv = exp(-log_scale);
    const double cdf_plus = vb_cdf(inv_stdv * (centered + 1.0 / 255.0));
    const double cdf_min = vb_cdf(inv_stdv * (centered - 1.0 / 255.0));
    double lp;
    if (x < -0.999f) lp = log(fmax(cdf_plus, 1e-12));
    else if (x > 0.999f) lp = log(fmax(1.0 - cdf_min, 1e-12));
    else lp = log(fmax(cdf_plus - cdf_min, 1e-12));
    return -lp;
}

struct VbRow {          // per-row scalars
    StepCoef sc;
    bool first;         // t == 0: the decoder NLL instead of the KL
    double c1, c2;      // posterior_mean_coef1/2 (t == 0 branch, in double)
    double log_scale;   // 0.5 * model log-variance
};

// One element: x0-hat (blend on the raw output, conversion, clip: step_pred), the three squares, and the bound's per-element term --
// t != 0: the squared difference of the two posterior means (the row's KL is affine in its mean, see k_vb_terms); t == 0: the NLL.
template <int MEAN>
__device__ __forceinline__ float vb_element(const VbRow& vr, float x0, float xt, float mo, float z, bool blend, float m, float mot,
                                            bool clip, double (&s)[4]) {
    float raw = mo;
    if (blend) raw = raw * (1.0f - m) + mot * m;
    const float pred = step_pred<MEAN>(vr.sc, mo, xt, blend, m, mot, clip);
    const float dx = pred - x0;
    const float eps = (vr.sc.srac * xt - pred) / vr.sc.srm1ac;
    const float de = eps - z;
    if (vr.first) {
        const double mean = MEAN == 2 ? (double)raw : vr.c1 * (double)pred + vr.c2 * (double)xt;
        s[0] += vb_decoder_nll(x0, mean, vr.log_scale);
    } else {
        // mean types 0 and 1: true_mean - model_mean = coef1 (x0 - x0hat), the coef2 x_t terms cancel exactly
        const float dm = MEAN == 2 ? (vr.sc.c1 * x0 + vr.sc.c2 * xt) - raw : vr.sc.c1 * (x0 - pred);
        s[0] += (double)(dm * dm);
    }
    s[1] += (double)(dx * dx);
    s[2] += (double)(de * de);
    s[3] += (double)(pred * pred);
    return pred;
}

// DRAW: z from the counter (one thread per quad of frames); otherwise from `noise` [R, per_clip] (one thread per element).
template <int MEAN, bool DRAW>
__global__ __launch_bounds__(VB_THREADS) void k_vb_terms(const float* __restrict__ tab, const float* __restrict__ true_logvar, int nsteps,
                                                         const float* __restrict__ x_start, const float* __restrict__ x_t,
                                                         const float* __restrict__ model_out, const float* __restrict__ noise,
                                                         const float* __restrict__ mask, const float* __restrict__ motion,
                                                         const long long* __restrict__ clip, const long long* __restrict__ t,
                                                         long long per_clip, int F, int T, unsigned long long seed, int clip_denoised,
                                                         float* __restrict__ out, float* __restrict__ xstart) {
    const int row = blockIdx.x;
    const int tt = (int)t[row];
    const long long c = clip[row];
    VbRow vr;
    vr.sc = step_coef_plms(tab, nsteps, tt);            // c1, c2, srac, srm1ac at t (the sampler-specific fields are not read)
    vr.first = tt == 0;
    vr.c1 = (double)vr.sc.c1;
    vr.c2 = (double)vr.sc.c2;
    const double lv2 = (double)tab[TAB_LOGVAR * nsteps + tt], lv1 = (double)true_logvar[tt];
    vr.log_scale = 0.5 * lv2;
    const bool blend = mask != nullptr && motion != nullptr;
    const size_t base = (size_t)row * per_clip, cbase = (size_t)c * per_clip;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (DRAW) {
        const int TQ = (T + 3) >> 2;
        const long long quads = (long long)F * TQ;
        for (long long i = threadIdx.x; i < quads; i += VB_THREADS) {
            const int f = (int)(i / TQ), tq = (int)(i - (long long)f * TQ);
            float z[4];
            philox_normal4((unsigned)tq, (unsigned)f, (unsigned)c, (unsigned)tt, seed, z);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int l = tq * 4 + j;
                if (l < T) {
                    const size_t e = (size_t)f * T + l;
                    const float pred = vb_element<MEAN>(vr, x_start[cbase + e], x_t[base + e], model_out[base + e], z[j], blend,
                                                        blend ? mask[cbase + e] : 0.f, blend ? motion[cbase + e] : 0.f, clip_denoised, s);
                    if (xstart) xstart[base + e] = pred;
                }
            }
        }
    } else {
        for (long long i = threadIdx.x; i < per_clip; i += VB_THREADS) {
            const float pred = vb_element<MEAN>(vr, x_start[cbase + i], x_t[base + i], model_out[base + i], noise[base + i], blend,
                                                blend ? mask[cbase + i] : 0.f, blend ? motion[cbase + i] : 0.f, clip_denoised, s);
            if (xstart) xstart[base + i] = pred;
        }
    }
    vb_block_sum<4>(s);
    if (threadIdx.x == 0) {
        const double n = (double)per_clip;
        double vb;
        if (vr.first) vb = s[0] / n;
        else          // mean_flat(normal_kl): 0.5 (-1 + lv2 - lv1 + exp(lv1 - lv2) + mean((m1 - m2)^2) exp(-lv2)), the row's scalars in double
            vb = 0.5 * (-1.0 + lv2 - lv1 + exp(lv1 - lv2) + (s[0] / n) * exp(-lv2));
        out[(size_t)row * 4 + 0] = (float)(vb / VB_LN2);
        out[(size_t)row * 4 + 1] = (float)(s[1] / n);
        out[(size_t)row * 4 + 2] = (float)(s[2] / n);
        out[(size_t)row * 4 + 3] = (float)sqrt(s[3] / n);
    }
}

// _prior_bpd: normal_kl(mean1 = sqrt_ac x0, logvar1 = lv, 0, 0) = 0.5 (-1 - lv + exp(lv) + mean1^2); one workgroup per clip.
__global__ __launch_bounds__(VB_THREADS) void k_vb_prior(const float* __restrict__ x_start, long long per_clip, float sqrt_ac, float lv,
                                                         float* __restrict__ out) {
    const int n = blockIdx.x;
    const size_t base = (size_t)n * per_clip;
    double s[1] = {0.0};
    for (long long i = threadIdx.x; i < per_clip; i += VB_THREADS) {
        const float m = sqrt_ac * x_start[base + i];
        s[0] += (double)(m * m);
    }
    vb_block_sum<1>(s);
    if (threadIdx.x == 0) {
        const double l = (double)lv;
        out[n] = (float)(0.5 * (-1.0 - l + exp(l) + s[0] / (double)per_clip) / VB_LN2);
    }
}

}  // namespace mst
