// The T2M evaluators and their statistics, all in fp32 (the covariance in double): the evaluator is the instrument that measures the
// sampler, so nothing here rounds to f16.  Reference: data_loaders/humanml/networks/modules.py (MovementConvEncoder,
// MotionEncoderBiGRUCo, TextEncoderBiGRUCo) and data_loaders/humanml/utils/metrics.py.
//
//   k_gemm_f32     C = epi(gather(A) W^T + bias [+ add]) on v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain per output, two chains per
//                  output (even / odd k-steps) joined once.  gather: plain rows, or the four input frames 2t-1 .. 2t+2 of a
//                  Conv1d(C, N, 4, 2, 1) read where they lie (rows [B][T][ld] or the samplers' [B][F][1][T]), with a per-feature affine.
//   k_gru_step     one time step of both directions of torch's GRU (gates r, z, n): W_hh[slice] h for 16 units x 3 gates x 16 clips a
//                  workgroup, the gate arithmetic fused, h double-buffered in global memory by the host loop.
//   k_ln_leaky     LayerNorm (two-pass, biased variance) + LeakyReLU, one wave a row.
//   k_dist_rank    sqrt(-2 a.b + |a|^2 + |b|^2) and per row the number of entries strictly below the diagonal one.  Only a radicand
//                  below zero (rounding) is clamped to 0: NaN and +inf pass through the root, so a non-finite embedding row gives a
//                  non-finite row of distances, never 0.  A row whose diagonal distance is not finite gets rank n2: it is in no top-k.
//   k_col_mean_f64 / k_cov_f64   np.cov(rowvar=False) of fp32 rows in double.
//   k_pair_norms   |A[i_k] - B[j_k]|, summed in fp32.
// No atomics; every result is a fixed-order sum, so a row's value does not depend on what else is in the batch.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mst_common.h"

enum { kEvalPlain = 0, kEvalConvRows = 1, kEvalConvSample = 2 };
#define EVAL_BM 64
#define EVAL_BN 64
#define EVAL_BK 32
#define EVAL_GRU_CLIPS 16
#define EVAL_GRU_UNITS 16
#define EVAL_DIST_MAX_D 8192

struct EvalGemmArgs {
    const float* a;          // plain: [M][lda]; conv rows: [B][Tin][ldx]; conv sample: [B][ldx = F][Tin]
    const float* w;          // [N][K]; conv: K index = tap * C + channel
    const float* bias;       // [N] or null
    const float* add;        // [M][ldadd] or null: added before the activation
    const float* scale;      // [C] or null: x * scale + shift on every value read (the zero padding stays zero)
    const float* shift;
    float* c;                // [M][ldc]
    int M, N, K, mode, leaky;
    int Tin, Tout, C;
    int64_t lda, ldc, ldadd, ldx, sb;
};

__device__ __forceinline__ float eval_a(const EvalGemmArgs& p, int m, int k) {
    if (m >= p.M || k >= p.K) return 0.f;
    if (p.mode == kEvalPlain) return p.a[(int64_t)m * p.lda + k];
    const int b = m / p.Tout, t = m - b * p.Tout;
    const int tap = k / p.C, ch = k - tap * p.C;
    const int f = 2 * t - 1 + tap;
    if (f < 0 || f >= p.Tin) return 0.f;
    float v = p.mode == kEvalConvRows ? p.a[b * p.sb + (int64_t)f * p.ldx + ch] : p.a[b * p.sb + (int64_t)ch * p.Tin + f];
    if (p.scale) v = v * p.scale[ch] + p.shift[ch];
    return v;
}

__global__ __launch_bounds__(256) void k_gemm_f32(const EvalGemmArgs p) {
    __shared__ float As[EVAL_BM][EVAL_BK + 1];
    __shared__ float Ws[EVAL_BN][EVAL_BK + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * EVAL_BN, m0 = blockIdx.y * EVAL_BM;
    const int lr = tid >> 2, lk = (tid & 3) * 8;             // this thread stages 8 consecutive k of one row of each operand
    f32x4 acc[2][4];
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int ct = 0; ct < 4; ct++) acc[h][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < p.K; k0 += EVAL_BK) {
        float ra[8], rw[8];
        const int n = n0 + lr;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int k = k0 + lk + e;
            ra[e] = eval_a(p, m0 + lr, k);
            rw[e] = (n < p.N && k < p.K) ? p.w[(int64_t)n * p.K + k] : 0.f;
        }
        __syncthreads();                                     // the previous tile's reads are done
#pragma unroll
        for (int e = 0; e < 8; e++) {
            As[lr][lk + e] = ra[e];
            Ws[lr][lk + e] = rw[e];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < EVAL_BK / 4; ks++) {
            const float a = As[wave * 16 + (lane & 15)][ks * 4 + (lane >> 4)];
#pragma unroll
            for (int ct = 0; ct < 4; ct++) {
                const float b = Ws[ct * 16 + (lane & 15)][ks * 4 + (lane >> 4)];
                acc[ks & 1][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[ks & 1][ct], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ct++) {
        const int col = n0 + ct * 16 + (lane & 15);
        if (col >= p.N) continue;
        const float bv = p.bias ? p.bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = m0 + wave * 16 + (lane >> 4) * 4 + r;
            if (row >= p.M) continue;
            float v = (acc[0][ct][r] + acc[1][ct][r]) + bv;
            if (p.add) v += p.add[(int64_t)row * p.ldadd + col];
            if (p.leaky) v = v > 0.f ? v : 0.2f * v;
            p.c[(int64_t)row * p.ldc + col] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------ the recurrence
struct EvalGruArgs {
    const float* xproj;      // [B][Tm][2][3][H]: W_ih x + b_ih of every position, both directions
    const float* w_hh;       // [2][3 H][H]
    const float* b_hh;       // [2][3 H]
    const int32_t* steps;    // [B]: clip b takes part in steps 0 .. steps[b] - 1
    int B, Tm, H;
};

__global__ void k_gru_init(const float* __restrict__ hidden, float* __restrict__ h, int B, int H) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)B * 2 * H) h[i] = hidden[i % (2 * H)];            // h: [B][2][H], hidden: [2][1][H]
}

__global__ __launch_bounds__(256) void k_gru_step(const EvalGruArgs p, const float* __restrict__ h_in, float* __restrict__ h_out, int s) {
    __shared__ float red[4][3][EVAL_GRU_CLIPS][EVAL_GRU_UNITS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = p.H, ntile = H / EVAL_GRU_UNITS;
    const int u0 = ((int)blockIdx.x % ntile) * EVAL_GRU_UNITS, c0 = ((int)blockIdx.x / ntile) * EVAL_GRU_CLIPS;
    const int dir = blockIdx.y;
    {
        const int i = lane & 15, q = lane >> 4;
        const bool live = c0 + i < p.B;
        const float* hrow = h_in + ((int64_t)(live ? c0 + i : 0) * 2 + dir) * H;
        const float* wrow = p.w_hh + ((int64_t)dir * 3 * H + u0 + i) * H;
        f32x4 acc[3][2];
#pragma unroll
        for (int g = 0; g < 3; g++) acc[g][0] = acc[g][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kq = H / 4;                                // a wave sums a quarter of k; H is a multiple of 64
        for (int kb = wave * kq; kb < (wave + 1) * kq; kb += 16) {
            // a lane holds k = kb + 4 q .. + 3 of its clip row and of its unit row: MFMA e of the four sums over k = kb + 4 q' + e
            f32x4 a = *reinterpret_cast<const f32x4*>(hrow + kb + 4 * q);
            if (!live) a = f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 b[3];
#pragma unroll
            for (int g = 0; g < 3; g++) b[g] = *reinterpret_cast<const f32x4*>(wrow + (int64_t)g * H * H + kb + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int g = 0; g < 3; g++) acc[g][e & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[g][e], acc[g][e & 1], 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 3; g++)
#pragma unroll
            for (int r = 0; r < 4; r++) red[wave][g][q * 4 + r][i] = acc[g][0][r] + acc[g][1][r];
    }
    __syncthreads();
    const int unit = u0 + (tid & 15), cl = tid >> 4, clip = c0 + cl;
    if (clip >= p.B) return;
    const int64_t hoff = ((int64_t)clip * 2 + dir) * H + unit;
    const float hprev = h_in[hoff];
    int st = p.steps[clip];
    st = st < 0 ? 0 : (st > p.Tm ? p.Tm : st);
    if (s >= st) {                                           // finished: carried unchanged
        h_out[hoff] = hprev;
        return;
    }
    float hg[3];
#pragma unroll
    for (int g = 0; g < 3; g++)
        hg[g] = ((red[0][g][cl][tid & 15] + red[1][g][cl][tid & 15]) + (red[2][g][cl][tid & 15] + red[3][g][cl][tid & 15])) +
                p.b_hh[(dir * 3 + g) * H + unit];
    const int pos = dir == 0 ? s : st - 1 - s;
    const float* x = p.xproj + (((int64_t)clip * p.Tm + pos) * 2 + dir) * 3 * H + unit;
    const float r = 1.f / (1.f + expf(-(x[0] + hg[0])));
    const float z = 1.f / (1.f + expf(-(x[H] + hg[1])));
    const float n = tanhf(x[2 * H] + r * hg[2]);
    h_out[hoff] = (1.f - z) * n + z * hprev;
}

// ------------------------------------------------------------------------------------------ LayerNorm + LeakyReLU(0.2)
__device__ __forceinline__ float eval_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(64) void k_ln_leaky(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                 float* __restrict__ y, int width, float eps, int leaky) {
    const float* row = x + (int64_t)blockIdx.x * width;
    float* out = y + (int64_t)blockIdx.x * width;
    const int lane = threadIdx.x;
    float s = 0.f;
    for (int i = lane; i < width; i += 64) s += row[i];
    const float mean = eval_wave_sum(s) / (float)width;
    float q = 0.f;
    for (int i = lane; i < width; i += 64) {
        const float d = row[i] - mean;
        q += d * d;
    }
    const float inv = 1.f / sqrtf(eval_wave_sum(q) / (float)width + eps);
    for (int i = lane; i < width; i += 64) {
        float v = (row[i] - mean) * inv * gamma[i] + beta[i];
        if (leaky) v = v > 0.f ? v : 0.2f * v;
        out[i] = v;
    }
}

// ------------------------------------------------------------------------------------------ statistics
// One workgroup a row i of E1 (kept in LDS); a wave takes every fourth row j of E2, its lanes the features.
__global__ __launch_bounds__(256) void k_dist_rank(const float* __restrict__ e1, const float* __restrict__ e2, int n1, int n2, int d,
                                                   float* __restrict__ dist, int32_t* __restrict__ rank) {
    extern __shared__ float a_row[];                         // [d]
    __shared__ float a_sq;
    __shared__ int cnt[4];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < d; k += 256) a_row[k] = e1[(int64_t)i * d + k];
    __syncthreads();
    if (wave == 0) {
        float s = 0.f;
        for (int k = lane; k < d; k += 64) s += a_row[k] * a_row[k];
        s = eval_wave_sum(s);
        if (lane == 0) a_sq = s;
    }
    __syncthreads();
    const float asq = a_sq;
    for (int j = wave; j < n2; j += 4) {
        const float* b = e2 + (int64_t)j * d;
        float dot = 0.f, bsq = 0.f;
        for (int k = lane; k < d; k += 64) {
            const float bv = b[k];
            dot = fmaf(a_row[k], bv, dot);
            bsq = fmaf(bv, bv, bsq);
        }
        dot = eval_wave_sum(dot);
        bsq = eval_wave_sum(bsq);
        if (lane == 0) {
            const float rad = (-2.f * dot + asq) + bsq;      // the reference's order: d1 + d2, then + d3
            dist[(int64_t)i * n2 + j] = sqrtf(rad < 0.f ? 0.f : rad);       // NaN is not below zero: it goes through the root, as +inf does
        }
    }
    if (!rank) return;
    __syncthreads();                                         // the row of distances is written (workgroup scope)
    int c = 0;
    bool ranked = false;
    if (i < n2) {
        const float diag = dist[(int64_t)i * n2 + i];
        ranked = fabsf(diag) <= FLT_MAX;                     // false for NaN and inf
        for (int j = tid; j < n2; j += 256) c += dist[(int64_t)i * n2 + j] < diag ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) cnt[wave] = c;
    __syncthreads();
    if (tid == 0) rank[i] = i < n2 ? (ranked ? cnt[0] + cnt[1] + cnt[2] + cnt[3] : n2) : -1;
}

__global__ void k_col_mean_f64(const float* __restrict__ a, int n, int d, double* __restrict__ mean) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (int r = 0; r < n; r++) s += (double)a[(int64_t)r * d + c];
    mean[c] = s / (double)n;
}

// cov[i][j] = sum_r (a[r][i] - mean[i]) (a[r][j] - mean[j]) / (n - 1): 16 x 16 outputs a workgroup, the mean subtracted before the product
__global__ __launch_bounds__(256) void k_cov_f64(const float* __restrict__ a, const double* __restrict__ mean, int n, int d,
                                                 double* __restrict__ cov) {
    __shared__ double xi[16][17], xj[16][17];
    const int tid = threadIdx.x, tc = tid & 15, tr = tid >> 4;
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
    const int ci = i0 + tc, cj = j0 + tc;
    const double mi = ci < d ? mean[ci] : 0.0, mj = cj < d ? mean[cj] : 0.0;
    double acc = 0.0;
    for (int r0 = 0; r0 < n; r0 += 16) {
        const int r = r0 + tr;
        __syncthreads();
        xi[tr][tc] = (r < n && ci < d) ? (double)a[(int64_t)r * d + ci] - mi : 0.0;
        xj[tr][tc] = (r < n && cj < d) ? (double)a[(int64_t)r * d + cj] - mj : 0.0;
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 16; rr++) acc = fma(xi[rr][tr], xj[rr][tc], acc);
    }
    const int oi = i0 + tr, oj = j0 + tc;
    if (oi < d && oj < d) cov[(int64_t)oi * d + oj] = acc / (double)(n - 1);
}

// One wave a pair.  An index outside its matrix gives NaN and reads nothing.
__global__ __launch_bounds__(256) void k_pair_norms(const float* __restrict__ a, const float* __restrict__ b, const int32_t* __restrict__ ia,
                                                    const int32_t* __restrict__ ib, int pairs, int na, int nb, int d, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= pairs) return;
    const int i = ia[k], j = ib[k];
    if (i < 0 || i >= na || j < 0 || j >= nb) {
        if (lane == 0) out[k] = __builtin_nanf("");
        return;
    }
    const float* x = a + (int64_t)i * d;
    const float* y = b + (int64_t)j * d;
    float s = 0.f;
    for (int c = lane; c < d; c += 64) {
        const float v = x[c] - y[c];
        s = fmaf(v, v, s);
    }
    s = eval_wave_sum(s);
    if (lane == 0) out[k] = sqrtf(s);
}
