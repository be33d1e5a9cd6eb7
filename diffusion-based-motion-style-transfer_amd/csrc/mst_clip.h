// CLIP's text tower (width 512, 8 heads of 64, FFN 2048 with QuickGELU, causal attention over at most 77 tokens) over PACKED rows:
// only rows 0 .. e of a prompt (e = its end-of-text position) are ever computed, and the live rows of all prompts form one row range
// [0, M), prompt b at rows offs[b] .. offs[b] + lens[b] - 1.  The residual stream x stays fp32 from the embedding to the output; GEMM
// operands are f16 on v_mfma_f32_16x16x32_f16 with fp32 accumulation; LayerNorm statistics (two-pass), softmax and QuickGELU are fp32.
//
//   k_clip_pack      a row-major [N][K] matrix (f32 or f16) -> the B-fragment order of the 16x16x32 MFMA: fragment (n / 16, k / 32) is
//                    64 lanes x 8 halves, lane l holding W[16 nt + (l & 15)][32 ks + 8 (l >> 4) + 0..7]; fragments of one nt are
//                    contiguous along k, so a wave streams 1 KB per k-step.
//   k_clip_embed     x = tok_emb[id] + pos_emb[i] and h = LN1 of layer 0, one wave a row.
//   k_clip_gemm<E>   32 rows x 512 columns a workgroup, 8 waves of 32 x 64 (2 x 4 MFMA tiles); operands go global -> registers (the
//                    weight fragments are lane-linear, the activation fragment is 16 contiguous bytes of a row), no LDS in the loop.
//                    E = store:  out = f16(acc + bias)                           (QKV)
//                    E = gelu:   out = f16(u sigmoid(1.702 u)), u = acc + bias   (FFN1)
//                    E = resid:  x += acc + bias, then h = f16(LN(x; g, b)) of the NEXT LayerNorm (out-proj -> LN2, FFN2 -> next
//                                layer's LN1; no LayerNorm after the last layer), both written from the accumulators.
//   k_clip_attn      one workgroup per (head, prompt): K and V of the pair in LDS, a wave per query row, scores over j <= i only.
//   k_clip_final     per prompt: LN(x[e]; gf, bf) @ P, the LayerNorm output kept fp32.
//
// No atomics and no split-K.  Every output element is one fixed-order sum: the k-loop of a GEMM runs 0 .. K in 32-steps whatever M is,
// the tile is 32 x 512 whatever M is, a LayerNorm row is summed over (4 tiles in a lane) -> (16 lanes, xor butterfly) -> (8 waves in
// order), and attention sums keys 0 .. i in order.  None of this depends on the batch size, on M or on where a prompt's rows lie.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mst_common.h"

namespace mst {

#define CLIP_D 512
#define CLIP_H 8
#define CLIP_HD 64
#define CLIP_FF 2048
#define CLIP_CTX 77
#define CLIP_BM 32
#define CLIP_BN 512
#define CLIP_KSTRIDE 66      // halves a K row in LDS: 33 dwords, so 64 lanes reading 64 rows at one column hit 32 banks twice, not one 64 times
#define CLIP_LN_EPS 1e-5f

typedef f16 clip_f16x2 __attribute__((ext_vector_type(2)));

enum { kClipStore = 0, kClipGelu = 1, kClipResid = 2 };

template <typename T>
__global__ __launch_bounds__(256) void k_clip_pack(const T* __restrict__ src, f16* __restrict__ dst, int N, int K) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one (fragment, lane)
    if (idx >= (int64_t)N * K / 8) return;
    const int lane = (int)(idx & 63);
    const int64_t frag = idx >> 6;
    const int KS = K / 32;
    const int nt = (int)(frag / KS), ks = (int)(frag % KS);
    const T* s = src + (size_t)(nt * 16 + (lane & 15)) * K + ks * 32 + 8 * (lane >> 4);
    f16x8 v;
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = (f16)s[j];
    *(f16x8*)(dst + idx * 8) = v;
}

__device__ __forceinline__ float clip_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float clip_wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float clip_row16_sum(float v) {        // across the 16 lanes that hold one accumulator row
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

struct ClipEmbedArgs {
    const int32_t* ids;      // [B][stride]
    const int32_t* lens;     // [B] live rows of a prompt
    const int32_t* offs;     // [B] first packed row
    const f16* tok;          // [vocab][512]
    const f16* pos;          // [context][512]
    const float* g;          // LN1 of layer 0
    const float* b;
    float* x;                // [M][512]
    f16* h;                  // [M][512]
    int stride, vocab, context, M;
};

__global__ __launch_bounds__(256) void k_clip_embed(ClipEmbedArgs p) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int len = min(min(p.lens[b], p.stride), p.context), off = p.offs[b];
    const int c0 = lane * 8;
    for (int i = wave; i < len; i += 4) {
        const int row = off + i;
        if (row < 0 || row >= p.M) continue;                       // a plan that does not match the lengths writes nothing out of range
        const int id = min(max(p.ids[(size_t)b * p.stride + i], 0), p.vocab - 1);
        const f16x8 t = *(const f16x8*)(p.tok + (size_t)id * CLIP_D + c0);
        const f16x8 e = *(const f16x8*)(p.pos + (size_t)i * CLIP_D + c0);
        float v[8];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            v[j] = (float)t[j] + (float)e[j];
            s += v[j];
        }
        const float mean = clip_wave_sum(s) * (1.0f / CLIP_D);
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 8; j++) q += (v[j] - mean) * (v[j] - mean);
        const float rstd = 1.0f / sqrtf(clip_wave_sum(q) * (1.0f / CLIP_D) + CLIP_LN_EPS);
        float* xr = p.x + (size_t)row * CLIP_D + c0;
        *(f32x4*)xr = f32x4{v[0], v[1], v[2], v[3]};
        *(f32x4*)(xr + 4) = f32x4{v[4], v[5], v[6], v[7]};
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = (f16)((v[j] - mean) * rstd * p.g[c0 + j] + p.b[c0 + j]);
        *(f16x8*)(p.h + (size_t)row * CLIP_D + c0) = o;
    }
}

struct ClipGemmArgs {
    const f16* a;            // [M][K]
    const f16* w;            // [N][K] in fragment order (k_clip_pack)
    const float* bias;       // [N]
    float* x;                // resid: the fp32 stream [M][512], read and written
    const float* g;          // resid: the next LayerNorm, or null after the last layer
    const float* b;
    f16* out;                // store / gelu: [M][N]; resid: the LayerNorm output [M][512]
    int M, N, K;
};

template <int EPI>
__global__ __launch_bounds__(512) void k_clip_gemm(ClipGemmArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.x * CLIP_BM, n0 = blockIdx.y * CLIP_BN + wave * 64;
    const int KS = p.K / 32;
    // rows past M read row M - 1 (their results are never stored)
    const int ra = min(m0 + (lane & 15), p.M - 1), rb = min(m0 + 16 + (lane & 15), p.M - 1);
    const f16x8* a0 = (const f16x8*)(p.a + (size_t)ra * p.K + 8 * (lane >> 4));
    const f16x8* a1 = (const f16x8*)(p.a + (size_t)rb * p.K + 8 * (lane >> 4));
    const f16x8* wp = (const f16x8*)p.w + (size_t)(n0 / 16) * KS * 64 + lane;
    const size_t wstep = (size_t)KS * 64;                          // fragments of the next 16 columns
    f32x4 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int t = 0; t < 4; t++) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < KS; k0 += 4) {                           // K is 512 or 2048: four k-steps a trip, their loads issued together
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            const int ks = k0 + kk;
            const f16x8 fa0 = a0[ks * 4], fa1 = a1[ks * 4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const f16x8 fb = wp[t * wstep + (size_t)ks * 64];
                acc[0][t] = mfma16(fa0, fb, acc[0][t]);
                acc[1][t] = mfma16(fa1, fb, acc[1][t]);
            }
        }
    }
    // accumulator element (m, t, r): row m0 + 16 m + 4 (lane >> 4) + r, column n0 + 16 t + (lane & 15)
    const int col0 = n0 + (lane & 15), rbase = m0 + 4 * (lane >> 4);
    if constexpr (EPI != kClipResid) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int col = col0 + 16 * t;
            const float bias = p.bias[col];
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = rbase + 16 * m + r;
                    float u = acc[m][t][r] + bias;
                    if constexpr (EPI == kClipGelu) u = u / (1.0f + expf(-1.702f * u));
                    if (row < p.M) p.out[(size_t)row * p.N + col] = (f16)u;
                }
        }
    } else {
        __shared__ float red[2][8][CLIP_BM];
        float v[2][4][4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int col = col0 + 16 * t;
            const float bias = p.bias[col];
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = rbase + 16 * m + r;
                    float* xp = p.x + (size_t)min(row, p.M - 1) * CLIP_D + col;
                    const float y = *xp + (acc[m][t][r] + bias);
                    v[m][t][r] = y;
                    if (row < p.M) *xp = y;
                }
        }
        if (p.g != nullptr) {                                      // uniform over the launch
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float s = clip_row16_sum((v[m][0][r] + v[m][1][r]) + (v[m][2][r] + v[m][3][r]));
                    if ((lane & 15) == 0) red[0][wave][16 * m + 4 * (lane >> 4) + r] = s;
                }
            __syncthreads();
            float mean[2][4];
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int slot = 16 * m + 4 * (lane >> 4) + r;
                    float s = red[0][0][slot];
#pragma unroll
                    for (int w = 1; w < 8; w++) s += red[0][w][slot];
                    mean[m][r] = s * (1.0f / CLIP_D);
                }
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float q[4];
#pragma unroll
                    for (int t = 0; t < 4; t++) q[t] = (v[m][t][r] - mean[m][r]) * (v[m][t][r] - mean[m][r]);
                    const float s = clip_row16_sum((q[0] + q[1]) + (q[2] + q[3]));
                    if ((lane & 15) == 0) red[1][wave][16 * m + 4 * (lane >> 4) + r] = s;
                }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < 2; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int slot = 16 * m + 4 * (lane >> 4) + r, row = rbase + 16 * m + r;
                    float s = red[1][0][slot];
#pragma unroll
                    for (int w = 1; w < 8; w++) s += red[1][w][slot];
                    const float rstd = 1.0f / sqrtf(s * (1.0f / CLIP_D) + CLIP_LN_EPS);
                    if (row < p.M) {
#pragma unroll
                        for (int t = 0; t < 4; t++) {
                            const int col = col0 + 16 * t;
                            p.out[(size_t)row * CLIP_D + col] = (f16)((v[m][t][r] - mean[m][r]) * rstd * p.g[col] + p.b[col]);
                        }
                    }
                }
        }
    }
}

struct ClipAttnArgs {
    const f16* qkv;          // [M][1536]: q | k | v, head h at columns 64 h .. 64 h + 63 of each
    const int32_t* lens;
    const int32_t* offs;
    f16* out;                // [M][512]
    int M;
};

__global__ __launch_bounds__(256) void k_clip_attn(ClipAttnArgs p) {
    __shared__ __attribute__((aligned(16))) f16 ks[CLIP_CTX * CLIP_KSTRIDE];
    __shared__ __attribute__((aligned(16))) f16 vs[CLIP_CTX * CLIP_HD];
    __shared__ float qs[4][CLIP_HD];
    __shared__ float ps[4][128];
    const int head = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int off = p.offs[b];
    int len = min(p.lens[b], CLIP_CTX);
    if (off < 0 || off + len > p.M) len = 0;                       // uniform: a plan that does not match the lengths computes nothing
    const f16* base = p.qkv + (size_t)max(off, 0) * (3 * CLIP_D) + head * CLIP_HD;
    for (int idx = threadIdx.x; idx < len * 8; idx += 256) {
        const int j = idx >> 3, c = idx & 7;
        const uint4 kk = *(const uint4*)(base + (size_t)j * (3 * CLIP_D) + CLIP_D + c * 8);
        const uint4 vv = *(const uint4*)(base + (size_t)j * (3 * CLIP_D) + 2 * CLIP_D + c * 8);
        unsigned* kd = (unsigned*)(ks + j * CLIP_KSTRIDE + c * 8);  // 4-byte aligned only (row stride 132 bytes)
        kd[0] = kk.x; kd[1] = kk.y; kd[2] = kk.z; kd[3] = kk.w;
        *(uint4*)(vs + j * CLIP_HD + c * 8) = vv;
    }
    __syncthreads();
    for (int i0 = 0; i0 < len; i0 += 4) {                          // uniform trip count: the barriers below are reached by every wave
        const int i = i0 + wave;
        const bool live = i < len;
        if (live) qs[wave][lane] = (float)base[(size_t)i * (3 * CLIP_D) + lane];
        __syncthreads();
        float s0 = -INFINITY, s1 = -INFINITY;
        if (live) {
            const int j0 = lane, j1 = lane + 64;
            if (j0 <= i) {
                float s = 0.f;
#pragma unroll 8
                for (int d = 0; d < CLIP_HD; d += 2) {
                    const clip_f16x2 k2 = *(const clip_f16x2*)(ks + j0 * CLIP_KSTRIDE + d);
                    s = fmaf(qs[wave][d], (float)k2[0], s);
                    s = fmaf(qs[wave][d + 1], (float)k2[1], s);
                }
                s0 = s * 0.125f;
            }
            if (j1 <= i) {
                float s = 0.f;
#pragma unroll 8
                for (int d = 0; d < CLIP_HD; d += 2) {
                    const clip_f16x2 k2 = *(const clip_f16x2*)(ks + j1 * CLIP_KSTRIDE + d);
                    s = fmaf(qs[wave][d], (float)k2[0], s);
                    s = fmaf(qs[wave][d + 1], (float)k2[1], s);
                }
                s1 = s * 0.125f;
            }
        }
        const float mx = clip_wave_max(fmaxf(s0, s1));             // key 0 is always live: finite for a live row
        const float p0 = live && lane <= i ? expf(s0 - mx) : 0.f;
        const float p1 = live && lane + 64 <= i ? expf(s1 - mx) : 0.f;
        const float den = clip_wave_sum(p0 + p1);
        ps[wave][lane] = p0;
        ps[wave][lane + 64] = p1;
        __syncthreads();
        if (live) {
            float o = 0.f;
            for (int j = 0; j <= i; j++) o = fmaf(ps[wave][j], (float)vs[j * CLIP_HD + lane], o);
            p.out[(size_t)(off + i) * CLIP_D + head * CLIP_HD + lane] = (f16)(o / den);
        }
        __syncthreads();
    }
}

struct ClipFinalArgs {
    const float* x;          // [M][512]
    const int32_t* lens;
    const int32_t* offs;
    const float* g;          // ln_final
    const float* b;
    const f16* proj;         // text_projection [512 in][512 out], row-major
    float* out;              // [B][512]
    int M;
};

__global__ __launch_bounds__(512) void k_clip_final(ClipFinalArgs p) {
    __shared__ float hs[CLIP_D];
    __shared__ float red[2][8];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = min(max(p.offs[b] + min(p.lens[b], CLIP_CTX) - 1, 0), p.M - 1);
    const float v = p.x[(size_t)row * CLIP_D + tid];
    const float s = clip_wave_sum(v);
    if (lane == 0) red[0][wave] = s;
    __syncthreads();
    float tot = red[0][0];
#pragma unroll
    for (int w = 1; w < 8; w++) tot += red[0][w];
    const float mean = tot * (1.0f / CLIP_D);
    const float q = clip_wave_sum((v - mean) * (v - mean));
    if (lane == 0) red[1][wave] = q;
    __syncthreads();
    tot = red[1][0];
#pragma unroll
    for (int w = 1; w < 8; w++) tot += red[1][w];
    const float rstd = 1.0f / sqrtf(tot * (1.0f / CLIP_D) + CLIP_LN_EPS);
    hs[tid] = (v - mean) * rstd * p.g[tid] + p.b[tid];
    __syncthreads();
    float o = 0.f;
#pragma unroll 8
    for (int k = 0; k < CLIP_D; k++) o = fmaf(hs[k], (float)p.proj[(size_t)k * CLIP_D + tid], o);
    p.out[(size_t)b * CLIP_D + tid] = o;
}

}  // namespace mst
