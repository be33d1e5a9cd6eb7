// The SMPL body on the GPU in fp32: what smplx.SMPLLayer's `lbs` computes under the reference's model/smpl.py:86-97 and
// model/rotation2xyz.py:17-92, for every live frame of a batch of clips at once.  No backward pass.
//
//   k_smpl_pack    posedirs [207][3 V] and shapedirs [V][3][10] -> one operand image per tile of 32 vertices, in the order k_smpl_skin's
//                  lanes read it (below).  Once per body.
//   k_smpl_pose    one lane per live frame.  Reads the sample where it lies (x[b, j, f, t] through four strides), converts the 24
//                  rotations (rot6d / rotmat / rotquat / rotvec, the reference's own formulas, utils/rotation_conversions.py:38-66,
//                  :448-478, :536-551), J = J0 + Jdirs beta (J0, Jdirs formed by the host in double), the rigid chain over `parents`
//                  (G[j] = G[parent] [R[j] | J[j] - J[parent]]), and writes A [N][24][12] (A[j] = [G_R | G_t - G_R J[j]]), the operand
//                  row [N][224] (207 values of R[1:] - I, the 10 betas, 7 zeros) and the posed joints [N][24][3].  jointstype 'smpl' ends
//                  here: the root-relative joints go straight into the caller's [B][24][3][T].
//   k_smpl_skin    the hot kernel, v_mfma_f32_16x16x4_f32 throughout (an exact fp32 fmaf chain per output).  A workgroup owns 32 vertices;
//                  their 96 columns x 224 rows of [posedirs; shapedirs; 0] (84 KB) stay in LDS while its 8 waves walk the frame tiles of 16
//                  frames, so the body leaves HBM once.  Per tile a wave forms, for its two 16-vertex halves,
//                    off[v][c]  = sum_k row[n][k] P[k][3 v + c]       3 tiles a half (x, y, z), K = 224 in ascending k: the pose blend shapes
//                                                                     for k < 207, then shapedirs beta
//                    T[v][e]    = sum_j W[v][j] A[n][j][e]            12 tiles a half, K = 24 in ascending j: the DENSE sum over all joints
//                  so a lane ends with frame (lane & 15) and vertices 4 (lane >> 4) + r of both halves -- the C/D map puts the frame on
//                  the low lane bits, which is the contiguous axis of the [B][V][3][T] store.  Epilogue: v_posed = v_template + off,
//                  vertex = T [v_posed; 1], + (trans[t] - trans[0]) when asked for, one store.
//   k_smpl_regress one workgroup per live frame, for the joint lists that need vertices ('vibe', 'a2m', 'a2mpl'): the 9 rows of
//                  J_regressor_extra over the frame's vertices summed in double in a fixed order, the `vertex_ids` gather, the root
//                  subtracted, the translation added.
// No atomics and no split-K; every output is one fixed-order sum of operands that belong to its own frame, so a frame's bits depend on
// neither the batch, its position in it, other clips' lengths nor the stream.  Frames a mask rules out are never read.
//
// The operand row's storage order.  A lane of the 16x16x4 form supplies k = 4 s + (lane >> 4) of step s.  A lane reads four steps with
// one 16-byte load at float 16 q + 4 (lane >> 4) of the row, so storage slot 16 q + 4 g + i holds k = 16 q + 4 i + g (smpl_slot): the
// chain then runs in ascending k.  The packed body image is [tile][q 14][half 2][c 3][lane 64][i 4] floats, k the same function of
// (q, lane >> 4, i), vertex = 32 tile + 16 half + (lane & 15): the fill of LDS is a straight copy and every ds_read is 16 bytes a
// lane at consecutive addresses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mst_common.h"
#include "mst_rotdec.h"      // rot_cross, rot_dot, rot_matrix (the same 6D form), rot_mul, rot_mv

namespace mst {

constexpr int kSmplJoints = 24;
constexpr int kSmplBetas = 10;
constexpr int kSmplPoseK = 9 * (kSmplJoints - 1);          // 207
constexpr int kSmplK = 224;                                // 207 + 10 betas, padded to 14 x 16
constexpr int kSmplQ = kSmplK / 16;
constexpr int kSmplTileV = 32;                             // vertices a workgroup owns
constexpr int kSmplTileFloats = kSmplK * 3 * kSmplTileV;   // 21504 floats = 86016 bytes of LDS
constexpr int kSmplSkinThreads = 512;
constexpr int kSmplAllJoints = 54;                         // 24 posed + 21 vertex ids + 9 regressed
constexpr int kSmplVertexIds = 21;
constexpr int kSmplExtra = 9;
enum { kSmplRot6d = 0, kSmplRotmat = 1, kSmplRotquat = 2, kSmplRotvec = 3 };

__host__ __device__ inline int smpl_slot(int k) { return (k & ~15) + 4 * (k & 3) + ((k & 15) >> 2); }

// the workspace of one call: A | rows | posed joints | vertices (only when a joint list needs them), each 256-byte aligned
struct SmplWorkspace {
    float* A;        // [N][24][12]
    float* rows;     // [N][224]
    float* posed;    // [N][24][3]
    float* verts;    // [N][V][3]
    int64_t bytes;
};
inline SmplWorkspace smpl_carve(void* base, int64_t N, int64_t V, bool verts) {
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    const int64_t a = up(N * kSmplJoints * 12 * 4), r = up(N * kSmplK * 4), p = up(N * kSmplJoints * 3 * 4), v = verts ? up(N * V * 3 * 4) : 0;
    char* c = (char*)base;
    return SmplWorkspace{(float*)c, (float*)(c + a), (float*)(c + a + r), verts ? (float*)(c + a + r + p) : nullptr, a + r + p + v};
}

// ------------------------------------------------------------------------------------------ packing
__global__ void k_smpl_pack(const float* __restrict__ posedirs, const float* __restrict__ shapedirs, float* __restrict__ packed, int V, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int i = idx & 3, lane = (idx >> 2) & 63;
    int64_t rest = idx >> 8;
    const int c = rest % 3;
    rest /= 3;
    const int half = rest & 1;
    rest >>= 1;
    const int q = rest % kSmplQ;
    const int64_t tile = rest / kSmplQ;
    const int k = 16 * q + 4 * i + (lane >> 4);
    const int64_t v = tile * kSmplTileV + 16 * half + (lane & 15);
    float val = 0.f;
    if (v < V) {
        if (k < kSmplPoseK) val = posedirs[(int64_t)k * 3 * V + 3 * v + c];
        else if (k < kSmplPoseK + kSmplBetas) val = shapedirs[(v * 3 + c) * kSmplBetas + (k - kSmplPoseK)];
    }
    packed[idx] = val;
}

// ------------------------------------------------------------------------------------------ rotations and the chain
struct SmplPoseArgs {
    const float* x;                          // element (b, j, f, t) at x[b * sb + j * sj + f * sf + t * st]
    long long sb, sj, sf, st;
    const int* frame_ids;                    // [N]: b * T + t of every live frame, or null (frame n is clip 0's frame n)
    int N, B, T, rep, glob;
    float glob_rot[3];                       // glob == 0: the one axis-angle of every frame
    const float* betas;                      // [N][10] or null: (0, beta, 0, ...)
    float beta;
    const float* J0;                         // [24][3]
    const float* Jdirs;                      // [24][3][10]
    signed char parents[kSmplJoints];
    int trans_joint;                         // >= 0: the sample row that carries the translation, added as trans[t] - trans[0]
    float* A;
    float* rows;
    float* posed;
    float* rot;                              // [N][24][9] or null
    float* out;                              // [B][24][3][T] or null: posed joints minus the root's
};

// quaternion_to_matrix (utils/rotation_conversions.py:38-66): two_s = 2 / |q|^2, q as it comes
__device__ __forceinline__ void smpl_quat_matrix(const float* q, float* M) {
#pragma clang fp contract(off)
    const float r = q[0], i = q[1], j = q[2], k = q[3];
    const float s = 2.0f / (((r * r + i * i) + j * j) + k * k);
    M[0] = 1.f - s * (j * j + k * k);
    M[1] = s * (i * j - k * r);
    M[2] = s * (i * k + j * r);
    M[3] = s * (i * j + k * r);
    M[4] = 1.f - s * (i * i + k * k);
    M[5] = s * (j * k - i * r);
    M[6] = s * (i * k - j * r);
    M[7] = s * (j * k + i * r);
    M[8] = 1.f - s * (i * i + j * j);
}
// axis_angle_to_quaternion (:448-478), its small-angle branch at 1e-6, then quaternion_to_matrix
__device__ __forceinline__ void smpl_rotvec_matrix(const float* a, float* M) {
#pragma clang fp contract(off)
    const float ang = sqrtf(rot_dot(a, a)), half = 0.5f * ang;
    const float s = fabsf(ang) < 1e-6f ? 0.5f - (ang * ang) / 48.f : sinf(half) / ang;
    const float q[4] = {cosf(half), a[0] * s, a[1] * s, a[2] * s};
    smpl_quat_matrix(q, M);
}

__device__ __forceinline__ void smpl_rotation(const SmplPoseArgs& p, int b, int t, int r, float* M) {
    if (!p.glob && r == 0) {
        smpl_rotvec_matrix(p.glob_rot, M);
        return;
    }
    const float* src = p.x + (long long)b * p.sb + (long long)(p.glob ? r : r - 1) * p.sj + (long long)t * p.st;
    float f[9];
    const int nf = p.rep == kSmplRot6d ? 6 : p.rep == kSmplRotmat ? 9 : p.rep == kSmplRotquat ? 4 : 3;
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = k < nf ? src[k * p.sf] : 0.f;
    if (p.rep == kSmplRot6d) rot_matrix(f, M);
    else if (p.rep == kSmplRotquat) smpl_quat_matrix(f, M);
    else if (p.rep == kSmplRotvec) smpl_rotvec_matrix(f, M);
    else {
#pragma unroll
        for (int k = 0; k < 9; k++) M[k] = f[k];
    }
}

__global__ __launch_bounds__(64) void k_smpl_pose(const SmplPoseArgs p) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= p.N) return;
    int fid = p.frame_ids ? p.frame_ids[n] : n;
    fid = min(max(fid, 0), p.B * p.T - 1);               // no access leaves the sample, whatever the caller wrote
    const int b = fid / p.T, t = fid - b * p.T;
    float beta[kSmplBetas];
#pragma unroll
    for (int i = 0; i < kSmplBetas; i++) beta[i] = p.betas ? p.betas[(size_t)n * kSmplBetas + i] : (i == 1 ? p.beta : 0.f);
    // the chain state of a lane: 24 x (rotation 9, translation 3) and the rest joints; indexed by `parents`, so it lives in scratch
    // memory, as k_rot_decode's does
    float G[kSmplJoints][12], J[kSmplJoints][3];
    float* A = p.A + (size_t)n * kSmplJoints * 12;
    float* row = p.rows + (size_t)n * kSmplK;
    for (int j = 0; j < kSmplJoints; j++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float s = p.J0[j * 3 + c];
#pragma unroll
            for (int i = 0; i < kSmplBetas; i++) s = fmaf(p.Jdirs[(j * 3 + c) * kSmplBetas + i], beta[i], s);
            J[j][c] = s;
        }
        float R[9];
        smpl_rotation(p, b, t, j, R);
        if (p.rot) {
#pragma unroll
            for (int k = 0; k < 9; k++) p.rot[((size_t)n * kSmplJoints + j) * 9 + k] = R[k];
        }
        if (j == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) G[0][k] = R[k];
#pragma unroll
            for (int c = 0; c < 3; c++) G[0][9 + c] = J[0][c];
        } else {
#pragma unroll
            for (int k = 0; k < 9; k++) row[smpl_slot(9 * (j - 1) + k)] = R[k] - ((k & 3) == 0 ? 1.f : 0.f);
            const int a = p.parents[j];
            float Ga[12], Gn[9], rel[3], o[3];
#pragma unroll
            for (int k = 0; k < 12; k++) Ga[k] = G[a][k];
#pragma unroll
            for (int c = 0; c < 3; c++) rel[c] = J[j][c] - J[a][c];
            rot_mul(Ga, R, Gn);
            rot_mv(Ga, rel, o);
#pragma unroll
            for (int k = 0; k < 9; k++) G[j][k] = Gn[k];
#pragma unroll
            for (int c = 0; c < 3; c++) G[j][9 + c] = o[c] + Ga[9 + c];
        }
        float gj[12], jj[3], gr[3];
#pragma unroll
        for (int k = 0; k < 12; k++) gj[k] = G[j][k];
#pragma unroll
        for (int c = 0; c < 3; c++) jj[c] = J[j][c];
        rot_mv(gj, jj, gr);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            A[j * 12 + 4 * c] = gj[3 * c];
            A[j * 12 + 4 * c + 1] = gj[3 * c + 1];
            A[j * 12 + 4 * c + 2] = gj[3 * c + 2];
            A[j * 12 + 4 * c + 3] = gj[9 + c] - gr[c];
            p.posed[((size_t)n * kSmplJoints + j) * 3 + c] = gj[9 + c];
        }
    }
#pragma unroll
    for (int i = 0; i < kSmplBetas; i++) row[smpl_slot(kSmplPoseK + i)] = beta[i];
    for (int k = kSmplPoseK + kSmplBetas; k < kSmplK; k++) row[smpl_slot(k)] = 0.f;
    if (p.out) {
        float d[3] = {0.f, 0.f, 0.f};
        if (p.trans_joint >= 0) {
            const float* tr = p.x + (long long)b * p.sb + (long long)p.trans_joint * p.sj;
#pragma unroll
            for (int c = 0; c < 3; c++) d[c] = tr[c * p.sf + (long long)t * p.st] - tr[c * p.sf];
        }
        for (int j = 0; j < kSmplJoints; j++) {
#pragma unroll
            for (int c = 0; c < 3; c++)
                p.out[(((size_t)b * kSmplJoints + j) * 3 + c) * p.T + t] = (G[j][9 + c] - G[0][9 + c]) + d[c];
        }
    }
}

// ------------------------------------------------------------------------------------------ skinning
struct SmplSkinArgs {
    const float* packed;                     // [tiles][kSmplTileFloats]
    const float* v_template;                 // [V][3]
    const float* weights;                    // [V][24]
    const float* A;
    const float* rows;
    const int* frame_ids;                    // [N] or null: frame n is (b 0, t n)
    int N, V, T, B;
    const float* trans;                      // element (b, c, t) at trans[b * tb + c * tc + t * tt], or null
    long long tb, tc, tt;
    float* out;                              // element (b, t, v, c) at out[b * ob + t * ot + v * ov + c * oc]
    long long ob, ot, ov, oc;
};

__global__ __launch_bounds__(kSmplSkinThreads) void k_smpl_skin(const SmplSkinArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smpl_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, col = lane & 15;
    const int v0 = blockIdx.x * kSmplTileV;
    {
        const f32x4* src = (const f32x4*)(p.packed + (size_t)blockIdx.x * kSmplTileFloats);
        f32x4* dst = (f32x4*)smpl_lds;
        for (int i = tid; i < kSmplTileFloats / 4; i += kSmplSkinThreads) dst[i] = src[i];
    }
    // what a lane keeps for the whole walk: its skinning weights as A operands (vertex v0 + 16 h + col, joint 4 s + g) and the rest
    // positions of the vertices it ends with (v0 + 16 h + 4 g + r).  A vertex past V reads the last one's; it is never stored.
    float wf[2][6], vt[2][4][3];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int va = min(v0 + 16 * h + col, p.V - 1);
#pragma unroll
        for (int s = 0; s < 6; s++) wf[h][s] = p.weights[(size_t)va * kSmplJoints + 4 * s + g];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int vo = min(v0 + 16 * h + 4 * g + r, p.V - 1);
#pragma unroll
            for (int c = 0; c < 3; c++) vt[h][r][c] = p.v_template[(size_t)vo * 3 + c];
        }
    }
    __syncthreads();
    const f32x4* lds4 = (const f32x4*)smpl_lds;
    const int ntiles = (p.N + 15) / 16, stride = gridDim.y * (kSmplSkinThreads / 64);
    for (int ft = blockIdx.y * (kSmplSkinThreads / 64) + wave; ft < ntiles; ft += stride) {
        const int n = ft * 16 + col;
        const bool live = n < p.N;
        const int nc = live ? n : p.N - 1;
        const f32x4* row = (const f32x4*)(p.rows + (size_t)nc * kSmplK) + g;
        const f32x4* Ar = (const f32x4*)(p.A + (size_t)nc * kSmplJoints * 12);
        f32x4 off[2][3];
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int c = 0; c < 3; c++) off[h][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int q = 0; q < kSmplQ; q++) {
            const f32x4 bq = row[4 * q];
            f32x4 aq[2][3];
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int c = 0; c < 3; c++) aq[h][c] = lds4[((q * 2 + h) * 3 + c) * 64 + lane];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int h = 0; h < 2; h++)
#pragma unroll
                    for (int c = 0; c < 3; c++) off[h][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[h][c][i], bq[i], off[h][c], 0, 0, 0);
        }
        f32x4 tr[2][12];
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int e = 0; e < 12; e++) tr[h][e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 6; s++) {
            const f32x4 a0 = Ar[(4 * s + g) * 3], a1 = Ar[(4 * s + g) * 3 + 1], a2 = Ar[(4 * s + g) * 3 + 2];
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    tr[h][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[h][s], a0[e], tr[h][e], 0, 0, 0);
                    tr[h][4 + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[h][s], a1[e], tr[h][4 + e], 0, 0, 0);
                    tr[h][8 + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[h][s], a2[e], tr[h][8 + e], 0, 0, 0);
                }
        }
        if (!live) continue;
        int b = 0, t = n;
        if (p.frame_ids) {
            const int fid = min(max(p.frame_ids[n], 0), p.B * p.T - 1);
            b = fid / p.T;
            t = fid - b * p.T;
        }
        float d[3] = {0.f, 0.f, 0.f};
        if (p.trans) {
#pragma unroll
            for (int c = 0; c < 3; c++) d[c] = p.trans[b * p.tb + c * p.tc + t * p.tt] - p.trans[b * p.tb + c * p.tc];
        }
        float* o = p.out + b * p.ob + t * p.ot;
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int v = v0 + 16 * h + 4 * g + r;
                if (v >= p.V) continue;
                const float x = vt[h][r][0] + off[h][0][r], y = vt[h][r][1] + off[h][1][r], z = vt[h][r][2] + off[h][2][r];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float s = fmaf(tr[h][4 * c][r], x, fmaf(tr[h][4 * c + 1][r], y, fmaf(tr[h][4 * c + 2][r], z, tr[h][4 * c + 3][r])));
                    o[v * p.ov + c * p.oc] = s + d[c];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------ the joint lists over vertices
struct SmplRegressArgs {
    const float* verts;                      // [N][V][3]
    const float* posed;                      // [N][24][3]
    const float* extra;                      // [9][V]
    int vertex_ids[kSmplVertexIds];
    const int* frame_ids;
    int N, V, T, B;
    int map[kSmplAllJoints];                 // output joint i is entry map[i] of (24 posed | 21 vertex ids | 9 regressed)
    int map_len, root;                       // root: the OUTPUT index whose joint is subtracted, -1: none
    const float* trans;
    long long tb, tc, tt;
    float* out;                              // [B][map_len][3][T]
};

__global__ __launch_bounds__(256) void k_smpl_regress(const SmplRegressArgs p) {
    __shared__ double part[256];
    __shared__ float all[kSmplAllJoints][3];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* vx = p.verts + (size_t)n * p.V * 3;
    for (int i = tid; i < kSmplJoints * 3; i += 256) all[i / 3][i % 3] = p.posed[(size_t)n * kSmplJoints * 3 + i];
    for (int i = tid; i < kSmplVertexIds * 3; i += 256) all[kSmplJoints + i / 3][i % 3] = vx[(size_t)p.vertex_ids[i / 3] * 3 + i % 3];
    // 27 sums over the vertices: a thread's own vertices in ascending order, then a tree over the 256 partial sums
    for (int e = 0; e < kSmplExtra; e++) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int v = tid; v < p.V; v += 256) {
            const double w = (double)p.extra[(size_t)e * p.V + v];
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] += w * (double)vx[(size_t)v * 3 + c];
        }
        for (int c = 0; c < 3; c++) {
            __syncthreads();
            part[tid] = s[c];
            __syncthreads();
            for (int w = 128; w > 0; w >>= 1) {
                if (tid < w) part[tid] += part[tid + w];
                __syncthreads();
            }
            if (tid == 0) all[kSmplJoints + kSmplVertexIds + e][c] = (float)part[0];
        }
    }
    __syncthreads();
    int b = 0, t = n;
    if (p.frame_ids) {
        const int fid = min(max(p.frame_ids[n], 0), p.B * p.T - 1);
        b = fid / p.T;
        t = fid - b * p.T;
    }
    for (int i = tid; i < p.map_len * 3; i += 256) {
        const int j = i / 3, c = i - 3 * j;
        float d = 0.f;
        if (p.trans) d = p.trans[b * p.tb + c * p.tc + t * p.tt] - p.trans[b * p.tb + c * p.tc];
        const float rv = p.root >= 0 ? all[p.map[p.root]][c] : 0.f;
        p.out[(((size_t)b * p.map_len + j) * 3 + c) * p.T + t] = (all[p.map[j]][c] - rv) + d;
    }
}

}  // namespace mst
