// The SMPLify-3D fitting objective and its gradient in fp32, one launch for every frame of a clip: what the reference's closure computes
// with a full smplx forward pass, visualize/joints2smpl/src/customloss.py:6-21, :128-226, prior.py:180-195 and an autograd backward pass
// (smplify.py:168-181, :218-235).  The posed joints of SMPL do not depend on the pose blend shapes, so no vertex is formed:
// J = J0 + Jdirs beta, the rigid chain over `parents`, and the loss reads the joints alone.  The reverse pass is written by hand.
//
//   k_smplify_pack  the symmetric precisions [8][69][69], the means [8][69] and -log(nll_weights) [8] -> one operand image: the
//                   precisions in MFMA fragment order (below), the means padded to 72, the 8 constants.  Once per prior.
//   k_smplify       one wave per tile of 16 frames.
//                   Prior (body stage), all 64 lanes, v_mfma_f32_16x16x4_f32 (an exact fp32 fmaf chain per output): for each of the 8
//                   components Y_m = P_m d_m, d_m = body_pose - mean_m, as a [69 -> 80] x [72] x [16 frames] product: five 16-row
//                   output tiles, K = 69 padded to 72 with zeros in 18 steps of ascending k.  The C/D map leaves a lane with frame
//                   (lane & 15) and rows 16 tile + 4 (lane >> 4) + r; its share of d_m^T Y_m is summed in that order and the four
//                   shares of a frame are added in ascending lane order.  value_m = 1/2 d_m^T Y_m - log nll_weight_m; the smallest
//                   wins, ties to the lowest index, and its Y IS the gradient (P is packed as its symmetric part).
//                   Chain, lanes 0 .. 15, one lane per frame: the 24 Rodrigues matrices (smplx's batch_rodrigues form, below), the
//                   chain, the joint / angle / shape / keep terms or the camera term, then the reverse walk from joint 23 to the root
//                   and through each Rodrigues form.  Its body-pose gradient crosses to the prior's lanes through LDS.
//   k_smplify_sum   the total: the per-frame losses added in double in ascending frame order by one lane, rounded once.
// No atomics and no split-K.  Every output of a frame is a fixed-order sum of that frame's own operands: the same bits alone, anywhere
// in a batch and on any stream, whatever other frames hold (an MFMA column reads its own frame's operand only).
//
// The Rodrigues form (fit_rodrigues), RECALLED from smplx.lbs.batch_rodrigues and not verified against it (smplx is not installed
// where this was written): a = |theta + 1e-8| with the 1e-8 added to every component, d = theta / a, K = skew(d),
// R = I + sin a K + (1 - cos a) K K.  Its derivative (fit_rodrigues_bwd) is that of this exact form: da/dtheta_i = (theta_i + 1e-8) / a,
// so theta = 0 is an ordinary point (a = sqrt(3) 1e-8, dR/dtheta_i the i-th generator).
//
// The packed precisions: [m 8][tile 5][pair 9][lane 64][2] floats; entry (.., lane, e) is P_m[16 tile + (lane & 15)][4 (2 pair + e) +
// (lane >> 4)], zero where a row or column is 69 or more.  A lane reads two K steps with one 8-byte load, the wave 512 consecutive bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mst_common.h"

namespace mst {

constexpr int kFitJoints = 24;
constexpr int kFitBetas = 10;
constexpr int kFitPose = 69;                               // the body pose: 23 axis-angles
constexpr int kFitK = 72;                                  // 69 padded to 18 steps of 4
constexpr int kFitComp = 8;                                // Gaussians of the mixture
constexpr int kFitTiles = 5;                               // 16-row output tiles: 80 >= 69
constexpr int kFitPairs = kFitK / 8;                       // 9 pairs of K steps
constexpr int kFitMatFloats = kFitComp * kFitTiles * kFitPairs * 64 * 2;       // 46080
constexpr int kFitMeanFloats = kFitComp * kFitK;                                // 576
constexpr int kFitPackedFloats = kFitMatFloats + kFitMeanFloats + kFitComp;    // 46664
constexpr int kFitFrames = 16;                             // frames a wave owns
enum { kFitCamera = 0, kFitBody = 1 };

__global__ void k_smplify_pack(const float* __restrict__ prec, const float* __restrict__ means, const float* __restrict__ neglog,
                               float* __restrict__ packed) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= kFitPackedFloats) return;
    float val = 0.f;
    if (idx < kFitMatFloats) {
        const int e = idx & 1, lane = (idx >> 1) & 63;
        int rest = idx >> 7;
        const int pair = rest % kFitPairs;
        rest /= kFitPairs;
        const int tile = rest % kFitTiles, m = rest / kFitTiles;
        const int k = 4 * (2 * pair + e) + (lane >> 4), i = 16 * tile + (lane & 15);
        if (i < kFitPose && k < kFitPose) val = prec[((size_t)m * kFitPose + i) * kFitPose + k];
    } else if (idx < kFitMatFloats + kFitMeanFloats) {
        const int r = idx - kFitMatFloats, m = r / kFitK, k = r - m * kFitK;
        if (k < kFitPose) val = means[m * kFitPose + k];
    } else {
        val = neglog[idx - kFitMatFloats - kFitMeanFloats];
    }
    packed[idx] = val;
}

struct FitArgs {
    int stage, nj, N;
    const float* pose;                       // [N][69]
    const float* orient;                     // [N][3]
    const float* betas;                      // [N][10]
    const float* cam;                        // [N][3]
    const float* target;                     // [N][nj][3]
    const float* conf;                       // [nj] (body stage)
    const float* preserve;                   // [N][69] (body stage)
    const float* cam_est;                    // [N][3] (camera stage)
    const float* J0;                         // [24][3]
    const float* Jdirs;                      // [24][3][10]
    const float* packed;                     // k_smplify_pack's image (body stage)
    signed char parents[kFitJoints];
    int sel[4];                              // camera stage: the torso joints
    float sigma, w_joint, w_prior, w_angle, w_shape, w_keep, w_depth;
    float* per_frame;                        // [N]
    float* joints;                           // [N][24][3]: the posed joints, no camera translation
    float* g_pose;                           // [N][69] or null
    float* g_orient;                         // [N][3] or null
    float* g_betas;                          // [N][10] or null
    float* g_cam;                            // [N][3] or null
    float* rot;                              // [N][24][9] or null
};

// smplx's batch_rodrigues as recalled (see the head of this file): the ONE place that states the form
__device__ __forceinline__ void fit_rodrigues(const float* th, float* R) {
    const float e0 = th[0] + 1e-8f, e1 = th[1] + 1e-8f, e2 = th[2] + 1e-8f;
    const float a = sqrtf((e0 * e0 + e1 * e1) + e2 * e2);
    const float x = th[0] / a, y = th[1] / a, z = th[2] / a;
    const float s = sinf(a), c1 = 1.f - cosf(a);
    R[0] = 1.f - c1 * (y * y + z * z);
    R[1] = c1 * (x * y) - s * z;
    R[2] = c1 * (x * z) + s * y;
    R[3] = c1 * (x * y) + s * z;
    R[4] = 1.f - c1 * (x * x + z * z);
    R[5] = c1 * (y * z) - s * x;
    R[6] = c1 * (x * z) - s * y;
    R[7] = c1 * (y * z) + s * x;
    R[8] = 1.f - c1 * (x * x + y * y);
}
// g = dL/dR -> dL/dtheta of the form above
__device__ __forceinline__ void fit_rodrigues_bwd(const float* th, const float* g, float* gth) {
    const float e0 = th[0] + 1e-8f, e1 = th[1] + 1e-8f, e2 = th[2] + 1e-8f;
    const float a = sqrtf((e0 * e0 + e1 * e1) + e2 * e2);
    const float x = th[0] / a, y = th[1] / a, z = th[2] / a;
    const float s = sinf(a), c = cosf(a), c1 = 1.f - c;
    // dL/ds over K, dL/dc1 over K K
    const float gs = (x * (g[7] - g[5]) + y * (g[2] - g[6])) + z * (g[3] - g[1]);
    const float gc1 = ((x * y) * (g[1] + g[3]) + (x * z) * (g[2] + g[6]) + (y * z) * (g[5] + g[7])) -
                      ((y * y + z * z) * g[0] + (x * x + z * z) * g[4] + (x * x + y * y) * g[8]);
    const float gx = s * (g[7] - g[5]) + c1 * ((y * (g[1] + g[3]) + z * (g[2] + g[6])) - 2.f * x * (g[4] + g[8]));
    const float gy = s * (g[2] - g[6]) + c1 * ((x * (g[1] + g[3]) + z * (g[5] + g[7])) - 2.f * y * (g[0] + g[8]));
    const float gz = s * (g[3] - g[1]) + c1 * ((x * (g[2] + g[6]) + y * (g[5] + g[7])) - 2.f * z * (g[0] + g[4]));
    const float ga = gs * c + gc1 * s;
    // d = theta / a: dd_k/dtheta_i = delta_ki / a - theta_k / a^2 da/dtheta_i, da/dtheta_i = (theta_i + 1e-8) / a
    const float t = (ga - ((gx * x + gy * y) + gz * z) / a) / a;
    gth[0] = gx / a + t * e0;
    gth[1] = gy / a + t * e1;
    gth[2] = gz / a + t * e2;
}

__global__ __launch_bounds__(64) void k_smplify(const FitArgs p) {
    __shared__ float gl[kFitFrames][kFitK];  // the chain lanes' share of the body-pose gradient
    const int lane = threadIdx.x, col = lane & 15, g = lane >> 4;
    const int n = blockIdx.x * kFitFrames + col;
    const bool live = n < p.N, body = p.stage == kFitBody;
    const int nc = live ? n : p.N - 1;       // a column past the clip reads the last frame's operands; nothing of it is stored
    float vbest = 0.f;
    f32x4 ybest[kFitTiles];
#pragma unroll
    for (int t = 0; t < kFitTiles; t++) ybest[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---------------------------------------------------------------- the mixture prior: Y_m = P_m (pose - mean_m), all lanes
    if (body) {
        const float* pr = p.pose + (size_t)nc * kFitPose;
        float xb[2 * kFitPairs], xo[kFitTiles][4];
#pragma unroll
        for (int s = 0; s < 2 * kFitPairs; s++) xb[s] = 4 * s + g < kFitPose ? pr[4 * s + g] : 0.f;
#pragma unroll
        for (int t = 0; t < kFitTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) xo[t][r] = 16 * t + 4 * g + r < kFitPose ? pr[16 * t + 4 * g + r] : 0.f;
        const float2* mat = (const float2*)p.packed;
        const float* means = p.packed + kFitMatFloats;
        const float* neglog = means + kFitMeanFloats;
#pragma unroll 1
        for (int m = 0; m < kFitComp; m++) {
            const float* mean = means + m * kFitK;
            f32x4 acc[kFitTiles];
#pragma unroll
            for (int t = 0; t < kFitTiles; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < kFitPairs; q++) {
                const float b0 = xb[2 * q] - mean[8 * q + g], b1 = xb[2 * q + 1] - mean[8 * q + 4 + g];
#pragma unroll
                for (int t = 0; t < kFitTiles; t++) {
                    const float2 a = mat[((m * kFitTiles + t) * kFitPairs + q) * 64 + lane];
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1, acc[t], 0, 0, 0);
                }
            }
            float part = 0.f;
#pragma unroll
            for (int t = 0; t < kFitTiles; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int i = 16 * t + 4 * g + r;
                    part = fmaf(i < kFitPose ? xo[t][r] - mean[i] : 0.f, acc[t][r], part);
                }
            const float q0 = __shfl(part, col), q1 = __shfl(part, col + 16), q2 = __shfl(part, col + 32), q3 = __shfl(part, col + 48);
            const float v = 0.5f * (((q0 + q1) + q2) + q3) + neglog[m];
            if (m == 0 || v < vbest) {       // the smallest; a tie keeps the lower index
                vbest = v;
#pragma unroll
                for (int t = 0; t < kFitTiles; t++) ybest[t] = acc[t];
            }
        }
    }

    // ---------------------------------------------------------------- the chain, forward and reverse: one lane per frame
    if (lane < kFitFrames && live) {
        float th[kFitJoints][3], beta[kFitBetas], cam[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            th[0][c] = p.orient[(size_t)n * 3 + c];
            cam[c] = p.cam[(size_t)n * 3 + c];
        }
        for (int i = 0; i < kFitPose; i++) th[1 + i / 3][i % 3] = p.pose[(size_t)n * kFitPose + i];
#pragma unroll
        for (int i = 0; i < kFitBetas; i++) beta[i] = p.betas[(size_t)n * kFitBetas + i];
        float J[kFitJoints][3], R[kFitJoints][9], GR[kFitJoints][9], Gt[kFitJoints][3];
        for (int j = 0; j < kFitJoints; j++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float s = p.J0[j * 3 + c];
#pragma unroll
                for (int i = 0; i < kFitBetas; i++) s = fmaf(p.Jdirs[(j * 3 + c) * kFitBetas + i], beta[i], s);
                J[j][c] = s;
            }
            float Rj[9];
            fit_rodrigues(th[j], Rj);
#pragma unroll
            for (int k = 0; k < 9; k++) R[j][k] = Rj[k];
            if (p.rot) {
#pragma unroll
                for (int k = 0; k < 9; k++) p.rot[((size_t)n * kFitJoints + j) * 9 + k] = Rj[k];
            }
            if (j == 0) {
#pragma unroll
                for (int k = 0; k < 9; k++) GR[0][k] = Rj[k];
#pragma unroll
                for (int c = 0; c < 3; c++) Gt[0][c] = J[0][c];
            } else {
                const int a = p.parents[j];
                float Ga[9], rel[3];
#pragma unroll
                for (int k = 0; k < 9; k++) Ga[k] = GR[a][k];
#pragma unroll
                for (int c = 0; c < 3; c++) rel[c] = J[j][c] - J[a][c];
#pragma unroll
                for (int r = 0; r < 3; r++) {
#pragma unroll
                    for (int c = 0; c < 3; c++) GR[j][3 * r + c] = fmaf(Ga[3 * r], Rj[c], fmaf(Ga[3 * r + 1], Rj[3 + c], Ga[3 * r + 2] * Rj[6 + c]));
                    Gt[j][r] = fmaf(Ga[3 * r], rel[0], fmaf(Ga[3 * r + 1], rel[1], Ga[3 * r + 2] * rel[2])) + Gt[a][r];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) p.joints[((size_t)n * kFitJoints + j) * 3 + c] = Gt[j][c];
        }

        // the loss of this frame and dL/d(posed joint)
        float gGt[kFitJoints][3], gcam[3] = {0.f, 0.f, 0.f}, gbeta[kFitBetas], loss;
        for (int j = 0; j < kFitJoints; j++)
#pragma unroll
            for (int c = 0; c < 3; c++) gGt[j][c] = 0.f;
#pragma unroll
        for (int i = 0; i < kFitBetas; i++) gbeta[i] = 0.f;
        if (body) {
            const float s2 = p.sigma * p.sigma, wj2 = p.w_joint * p.w_joint, wa2 = p.w_angle * p.w_angle, ws2 = p.w_shape * p.w_shape,
                        wk2 = p.w_keep * p.w_keep;
            float lj = 0.f;
            for (int j = 0; j < p.nj; j++) {
                const float cf = p.conf[j], c2 = cf * cf;
                float e = 0.f;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float r = (Gt[j][c] + cam[c]) - p.target[((size_t)n * p.nj + j) * 3 + c];
                    const float x2 = r * r, den = s2 + x2;
                    e += (s2 * x2) / den;
                    const float gq = (wj2 * c2) * ((2.f * r) * ((s2 / den) * (s2 / den)));
                    gGt[j][c] = gq;
                    gcam[c] += gq;
                }
                lj = fmaf(c2, e, lj);
            }
            // angle prior: entries 52, 55, 9, 12 of the body pose, signs +, -, -, -
            const int ai[4] = {52, 55, 9, 12};
            const float as[4] = {1.f, -1.f, -1.f, -1.f};
            float la = 0.f, ga[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float ex = expf(as[k] * th[1 + ai[k] / 3][ai[k] % 3]);
                la += ex * ex;
                ga[k] = wa2 * (2.f * as[k]) * (ex * ex);
            }
            float ls = 0.f, lk = 0.f;
#pragma unroll
            for (int i = 0; i < kFitBetas; i++) {
                ls = fmaf(beta[i], beta[i], ls);
                gbeta[i] = ws2 * (2.f * beta[i]);
            }
            for (int i = 0; i < kFitPose; i++) {
                const float d = th[1 + i / 3][i % 3] - p.preserve[(size_t)n * kFitPose + i];
                lk = fmaf(d, d, lk);
                float gi = wk2 * (2.f * d);
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (i == ai[k]) gi += ga[k];
                gl[col][i] = gi;
            }
            loss = (((wj2 * lj + (p.w_prior * p.w_prior) * vbest) + wa2 * la) + ws2 * ls) + wk2 * lk;
        } else {
            const float wd2 = p.w_depth * p.w_depth;
            float le = 0.f, ld = 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = p.sel[k];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float e = p.target[((size_t)n * p.nj + j) * 3 + c] - (Gt[j][c] + cam[c]);
                    le = fmaf(e, e, le);
                    gGt[j][c] += -2.f * e;
                    gcam[c] += -2.f * e;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float d = cam[c] - p.cam_est[(size_t)n * 3 + c];
                ld = fmaf(d, d, ld);
                gcam[c] += wd2 * (2.f * d);
            }
            loss = le + wd2 * ld;
        }
        p.per_frame[n] = loss;
        if (p.g_cam) {
#pragma unroll
            for (int c = 0; c < 3; c++) p.g_cam[(size_t)n * 3 + c] = gcam[c];
        }

        // the reverse walk: children before parents, joint 23 down to the root
        if (p.g_pose || p.g_orient || p.g_betas) {
            float gGR[kFitJoints][9], gJ[kFitJoints][3];
            for (int j = 0; j < kFitJoints; j++) {
#pragma unroll
                for (int k = 0; k < 9; k++) gGR[j][k] = 0.f;
#pragma unroll
                for (int c = 0; c < 3; c++) gJ[j][c] = 0.f;
            }
            for (int j = kFitJoints - 1; j >= 0; j--) {
                float gR[9], gt[3], gr[9], gth[3];
#pragma unroll
                for (int c = 0; c < 3; c++) gt[c] = gGt[j][c];
#pragma unroll
                for (int k = 0; k < 9; k++) gr[k] = gGR[j][k];
                if (j == 0) {
#pragma unroll
                    for (int k = 0; k < 9; k++) gR[k] = gr[k];
#pragma unroll
                    for (int c = 0; c < 3; c++) gJ[0][c] += gt[c];
                } else {
                    const int a = p.parents[j];
                    float Ga[9], Rj[9], rel[3];
#pragma unroll
                    for (int k = 0; k < 9; k++) {
                        Ga[k] = GR[a][k];
                        Rj[k] = R[j][k];
                    }
#pragma unroll
                    for (int c = 0; c < 3; c++) rel[c] = J[j][c] - J[a][c];
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        gGt[a][r] += gt[r];
                        // Gt[j] = GR[a] rel + Gt[a];  GR[j] = GR[a] R[j]
                        const float grel = fmaf(Ga[r], gt[0], fmaf(Ga[3 + r], gt[1], Ga[6 + r] * gt[2]));
                        gJ[j][r] += grel;
                        gJ[a][r] -= grel;
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            gGR[a][3 * r + c] += fmaf(gt[r], rel[c], fmaf(gr[3 * r], Rj[3 * c], fmaf(gr[3 * r + 1], Rj[3 * c + 1], gr[3 * r + 2] * Rj[3 * c + 2])));
                            gR[3 * r + c] = fmaf(Ga[r], gr[c], fmaf(Ga[3 + r], gr[3 + c], Ga[6 + r] * gr[6 + c]));
                        }
                    }
                }
                fit_rodrigues_bwd(th[j], gR, gth);
                if (j == 0) {
                    if (p.g_orient) {
#pragma unroll
                        for (int c = 0; c < 3; c++) p.g_orient[(size_t)n * 3 + c] = gth[c];
                    }
                } else if (body) {
#pragma unroll
                    for (int c = 0; c < 3; c++) gl[col][3 * (j - 1) + c] += gth[c];
                }
            }
            if (p.g_betas) {
                for (int j = 0; j < kFitJoints; j++)
#pragma unroll
                    for (int c = 0; c < 3; c++)
#pragma unroll
                        for (int i = 0; i < kFitBetas; i++) gbeta[i] = fmaf(gJ[j][c], p.Jdirs[(j * 3 + c) * kFitBetas + i], gbeta[i]);
#pragma unroll
                for (int i = 0; i < kFitBetas; i++) p.g_betas[(size_t)n * kFitBetas + i] = gbeta[i];
            }
        }
    }
    __syncthreads();

    // ---------------------------------------------------------------- the body-pose gradient: the chain's share plus w_prior^2 Y
    if (body && live && p.g_pose) {
        const float wp2 = p.w_prior * p.w_prior;
#pragma unroll
        for (int t = 0; t < kFitTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = 16 * t + 4 * g + r;
                if (i < kFitPose) p.g_pose[(size_t)n * kFitPose + i] = fmaf(wp2, ybest[t][r], gl[col][i]);
            }
    }
}

__global__ __launch_bounds__(256) void k_smplify_sum(const float* __restrict__ per_frame, int N, float* __restrict__ total) {
    __shared__ float buf[256];
    double s = 0.0;
    for (int base = 0; base < N; base += 256) {
        const int idx = base + threadIdx.x;
        buf[threadIdx.x] = idx < N ? per_frame[idx] : 0.f;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = min(256, N - base);
            for (int i = 0; i < cnt; i++) s += (double)buf[i];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = (float)s;
}

}  // namespace mst
