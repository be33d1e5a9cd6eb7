// A sample's rotation channels decoded on the GPU, one launch per batch: the reference's `recover_root_rot_pos`
// (data_loaders/humanml/common/bvh_utils.py:1299-1318) followed by one of three routes.
//
//   kRotHml    the 12 J - 1 HumanML row (263 features at 22 joints).  `output_bvh` (:1382-1441): the J - 1 6D blocks at feature
//              4 + 3 (J - 1) through `cont6d2q` (common/rotation.py:744-776, :453-474, :209-232), world quaternions chain by chain with
//              `qmultipy` (:110-128) -- EVERY chain restarts from r_rot_quat, also one that begins at a non-root joint -- the gather
//              onto the expanded skeleton (a host table, `expand_chains`) and qinv(world[parent]) (x) world[i].  `recover_from_rot`
//              (:1321-1335): `forward_kinematics_cont6d` (common/skeleton.py:177-198), the root's 6D the first two columns of
//              `q2rotm(r_rot_quat)` (rotation.py:139-160, :766-769).
//   kRotPosIk  the same 12 J - 1 row, read for its POSITIONS.  `output_bvh_with_pos` (:1444-1511): `recover_from_ric` (:1348-1363), then
//              `Skeleton.inverse_kinematics_np(smooth_forward=True)` (common/skeleton.py:55-103) -- the forward direction of every frame
//              (two fp32 rows in LDS, written in a first walk over the clip), smoothed by scipy's gaussian_filter1d(sigma 20): 161 taps
//              from the host in double, summed in double, index clamped into the clip, exactly as k_encode states it; the root quaternion
//              qbetween((0,0,1), forward), identity at frame 0; the chain IK, every chain restarting from that quaternion.  The IK's root
//              is dropped and its local quaternions go through the same chain products (restarting from r_rot_quat) and the same
//              expanded skeleton as kRotHml.  The joints output is recover_from_ric's.
//   kRotReal   the 9 J + 1 position-rotation row (181 / 190 features).  `output_bvh_from_real_rot` (:1538-1563): J 6D blocks through
//              `cont6d2q`, the root's multiplied from the left by r_rot_quat; the quaternions are local already.
//              `recover_from_real_rot` (:1337-1345): `forward_kinematics_real_cont6d` (skeleton.py:200-222).
//              `process_pos_from_real_rot` (:1366-1378): those positions minus the root's x and z, rotated by qinv(r_rot_quat)
//              (root-relative: a stated deviation from what the reference's aliased in-place subtraction returns, see the store).
//
// One workgroup per clip, lanes walk the frames of the clip's own length in rounds of the workgroup's width.  No atomics; every store is
// an ordinary vector store.  Rows at or past a clip's length are exact zeros in every output.
//
// The root.  The angle is the exclusive prefix sum of feature 0, root x and z the inclusive prefix sums of
// qrot(r_rot_quat[t], (v_x[t-1], 0, v_z[t-1])) -- this fork rotates by r_rot_quat, not by its inverse.  torch.cumsum on a CPU keeps ONE
// running sum, left to right, in double, and rounds every output to fp32.  Here the sums are in double too and rounded once per frame, but
// associated differently: a Hillis-Steele tree inside each wave of 64 frames, ((carry of earlier rounds + totals of earlier waves, in
// order) + the lane's in-wave prefix).  In double the two associations differ by about T * 2^-53 relative to the largest partial sum
// (5e-13 at 4096 frames), far below the final fp32 rounding, so almost every output is the same fp32 number.
//
// Per frame the lane keeps the chain state -- world quaternion or global matrix, and position, of every joint -- in a private array
// (16 J floats a lane, 1.5 KB at the cap; scratch memory, as k_ik_solve's chain state).  Nothing a frame needs is kept in LDS.
// Not reproduced: rotm2axangle's SVD branch for an angle that is an exact multiple of pi, as in k_ik_solve.
#pragma once
#include <hip/hip_runtime.h>

namespace mst {

constexpr int kRotMaxJoints = 24;            // the caps of mst_fit_joints and mst_encode_motion: every skeleton those take
constexpr int kRotMaxOut = 2 * kRotMaxJoints;    // expanded joints: one duplicate per chain, at most J - 1 chains
constexpr int kRotMaxFrames = 4096;          // what the windowed loops return (kWinMaxFrames); the bound is time, not memory
constexpr int kRotThreads = 256;
constexpr int kRotWaves = kRotThreads / 64;
// LDS: three scans x kRotWaves wave totals in double = 96 bytes, whatever the clip length or the joint count; kRotPosIk adds the forward
// direction, two fp32 rows of `frames` entries: 32 KB at the cap, below the 64 KB a launch gets without an opt-in.
constexpr int kRotHml = 0, kRotReal = 1, kRotPosIk = 2;
constexpr int kRotRadius = 80;               // int(4 * 20 + 0.5): scipy's truncate = 4 at sigma 20 (twin: kEncRadius)

struct RotArgs {
    const float* data;                       // element (b, t, f) at data[b * sb + t * st + f * sf]
    long long sb, st, sf;
    const float* mean;                       // [feats] or null
    const float* stdv;
    const int* lengths;                      // [B] or null
    int B, T, J, mode, Jx;                   // Jx: joints of the quaternion output (kRotReal: J)
    int n_links;                             // the chains link by link in the reference's order; every joint 1 .. J - 1 is a child once
    signed char link_child[kRotMaxJoints], link_parent[kRotMaxJoints], link_first[kRotMaxJoints];
    signed char src[kRotMaxOut];             // kRotHml: expanded joint -> the joint whose world quaternion it carries, -1: identity
    signed char xparent[kRotMaxOut];         // kRotHml: expanded joint -> its expanded parent (0: -1)
    float off[kRotMaxJoints][3];
    int face[4];                             // kRotPosIk: r_hip, l_hip, sdr_r, sdr_l
    float raw[kRotMaxJoints][3];             // kRotPosIk: the unit bone directions
    double taps[kRotRadius + 1];             // kRotPosIk: taps[|k|], normalised
    float* quats;                            // [B][T][Jx][4] or null
    float* root_pos;                         // [B][T][3] or null
    float* joints;                           // [B][T][J][3] or null
    float* local;                            // [B][T][3 (J - 1)] or null (kRotReal)
};

__device__ __forceinline__ float rot_value(const RotArgs& p, int b, int t, int f) {
#pragma clang fp contract(off)
    const float v = p.data[(long long)b * p.sb + (long long)t * p.st + (long long)f * p.sf];
    return p.mean ? v * p.stdv[f] + p.mean[f] : v;
}

// ---- restated device functions; mst_encode.h and mst_ik.h are pinned bit for bit by their own tests and stay untouched.  No contraction
// into fused multiply-adds: q (x) (1, 0, 0, 0) = q and the vector part of qinv(q) (x) q = 0 then hold exactly.
__device__ __forceinline__ void rot_cross(const float* a, const float* b, float* o) {          // twin: enc_cross / ik_cross
#pragma clang fp contract(off)
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float rot_dot(const float* a, const float* b) {
#pragma clang fp contract(off)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
__device__ __forceinline__ void rot_qrot(const float* q, const float* v, float* o) {            // twin: enc_qrot (rotation.py:47-56)
#pragma clang fp contract(off)
    float uv[3], uuv[3];
    rot_cross(q + 1, v, uv);
    rot_cross(q + 1, uv, uuv);
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = v[k] + 2.f * (q[0] * uv[k] + uuv[k]);
}
__device__ __forceinline__ void rot_qmultipy(const float* a, const float* b, float* o) {       // rotation.py:110-128; twin: k_ik_solve's tail
#pragma clang fp contract(off)
    float v[3];
    rot_cross(a + 1, b + 1, v);
    o[0] = a[0] * b[0] - rot_dot(a + 1, b + 1);
#pragma unroll
    for (int k = 0; k < 3; k++) o[1 + k] = (a[0] * b[1 + k] + b[0] * a[1 + k]) + v[k];
}
__device__ __forceinline__ void rot_mul(const float* A, const float* B, float* C) {            // C = A B, row-major; twin: ik_mul
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ void rot_mv(const float* A, const float* v, float* o) {             // twin: ik_mv
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = A[3 * r] * v[0] + A[3 * r + 1] * v[1] + A[3 * r + 2] * v[2];
}
// cont6d_to_matrix / cont6d2matrix (quaternion.py:347-363, rotation.py:744-760): x, y, z as columns; twin: ik_matrix
__device__ __forceinline__ void rot_matrix(const float* c, float* M) {
#pragma clang fp contract(off)
    float x[3], zr[3], z[3], y[3];
    const float n = sqrtf(rot_dot(c, c));
#pragma unroll
    for (int k = 0; k < 3; k++) x[k] = c[k] / n;
    rot_cross(x, c + 3, zr);
    const float nz = sqrtf(rot_dot(zr, zr));
#pragma unroll
    for (int k = 0; k < 3; k++) z[k] = zr[k] / nz;
    rot_cross(z, x, y);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        M[3 * k] = x[k];
        M[3 * k + 1] = y[k];
        M[3 * k + 2] = z[k];
    }
}
// rotm2axangle (rotation.py:453-474) then axangle2q (:209-232), with the reference's rule for an angle of exactly 0: theta = 0.1, so the
// axis is 0 / (2 sin 0.1) = 0 and the quaternion exactly (1, 0, 0, 0).  twin: k_ik_solve's tail
__device__ __forceinline__ void rot_matrix_to_quat(const float* M, float* o) {
#pragma clang fp contract(off)
    float ac = (M[0] + M[4] + M[8] - 1.f) / 2.f;
    ac = fminf(fmaxf(ac, -1.f), 1.f);
    float th = acosf(ac);
    if (th == 0.f) th = 0.1f;
    const float den = 2.f * sinf(th);
    const float aa[3] = {(M[7] - M[5]) / den * th, (M[2] - M[6]) / den * th, (M[3] - M[1]) / den * th};
    const float th2 = sqrtf(rot_dot(aa, aa)), th1 = th2 == 0.f ? 0.1f : th2;
    const float sh = sinf(th2 / 2.f);
    o[0] = cosf(th2 / 2.f);
#pragma unroll
    for (int k = 0; k < 3; k++) o[1 + k] = aa[k] / th1 * sh;
}
// quaternion_to_matrix (quaternion.py:300-327): q normalised, then 2 / |q_n|^2; twin: ik_quat_matrix
__device__ __forceinline__ void rot_quat_matrix(const float* q, float* Y) {
#pragma clang fp contract(off)
    const float nq = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float r = q[0] / nq, i = q[1] / nq, j = q[2] / nq, k = q[3] / nq;
    const float t = 2.f / (r * r + i * i + j * j + k * k);
    Y[0] = 1.f - t * (j * j + k * k);
    Y[1] = t * (i * j - k * r);
    Y[2] = t * (i * k + j * r);
    Y[3] = t * (i * j + k * r);
    Y[4] = 1.f - t * (i * i + k * k);
    Y[5] = t * (j * k - i * r);
    Y[6] = t * (i * k - j * r);
    Y[7] = t * (j * k + i * r);
    Y[8] = 1.f - t * (i * i + j * j);
}

__device__ __forceinline__ void rot_qmul(const float* a, const float* b, float* o) {           // quaternion.py:33-51; twin: enc_qmul
#pragma clang fp contract(off)
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
__device__ __forceinline__ void rot_qbetween(const float* v0, const float* v1, float* q) {     // quaternion.py:421-431; twin: enc_qbetween
#pragma clang fp contract(off)
    rot_cross(v0, v1, q + 1);
    q[0] = sqrtf(rot_dot(v0, v0) * rot_dot(v1, v1)) + rot_dot(v0, v1);
    const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] /= n;
}
// recover_from_ric (bvh_utils.py:1348-1363): joint j of frame t from the position channels, the root from r_pos
__device__ __forceinline__ void rot_ric_pos(const RotArgs& p, int b, int t, int j, const float* r, const float* rp, float* o) {
#pragma clang fp contract(off)
    if (j == 0) {
        o[0] = rp[0];
        o[1] = rp[1];
        o[2] = rp[2];
        return;
    }
    const int f = 4 + 3 * (j - 1);
    const float v[3] = {rot_value(p, b, t, f), rot_value(p, b, t, f + 1), rot_value(p, b, t, f + 2)};
    rot_qrot(r, v, o);
    o[0] += rp[0];
    o[2] += rp[2];
}

// inclusive prefix sum over the wave's 64 lanes, Hillis-Steele
__device__ __forceinline__ double rot_wave_scan(double x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(x, d, 64);
        if (lane >= d) x += o;
    }
    return x;
}

__global__ __launch_bounds__(kRotThreads) void k_rot_decode(RotArgs p) {
#pragma clang fp contract(off)
    extern __shared__ float rot_fw[];        // kRotPosIk: fwd_x[T], fwd_z[T]
    __shared__ double wtot[3][kRotWaves];    // per scan: every wave's total of the round
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = p.T, J = p.J, Jx = p.Jx;
    int len = p.lengths ? p.lengths[b] : T;
    len = min(max(len, 1), T);               // no access leaves the clip, whatever the caller wrote
    const int R0 = 4 + 3 * (J - 1);
    // offsets inside a clip fit an int (at the caps: 4096 frames x 48 joints x 4 floats); only the clip's bases are 64-bit
    float* quats = p.quats ? p.quats + (size_t)b * T * Jx * 4 : nullptr;
    float* root_pos = p.root_pos ? p.root_pos + (size_t)b * T * 3 : nullptr;
    float* joints = p.joints ? p.joints + (size_t)b * T * J * 3 : nullptr;
    float* local = p.local ? p.local + (size_t)b * T * (J - 1) * 3 : nullptr;
    float* fwx = rot_fw;
    float* fwz = rot_fw + T;

    // kRotPosIk walks the clip twice: the first walk (pass 0) leaves every frame's forward direction in LDS, which the second smooths over
    // +-80 frames.  Both walks form the same scans from the same operands.
    for (int pass = p.mode == kRotPosIk ? 0 : 1; pass < 2; pass++) {
    double carry_a = 0.0, carry_x = 0.0, carry_z = 0.0;      // the sums of all earlier rounds: every lane forms the same three numbers
    for (int base = 0; base < len; base += kRotThreads) {
        const int t = base + tid;
        const bool live = t < len;
        // ---- the angle: exclusive prefix sum of feature 0
        const double a_in = rot_wave_scan(live ? (double)rot_value(p, b, t, 0) : 0.0, lane);
        double a_ex = __shfl_up(a_in, 1, 64);
        if (lane == 0) a_ex = 0.0;
        if (lane == 63) wtot[0][wave] = a_in;
        __syncthreads();
        double before = carry_a;
        for (int w = 0; w < kRotWaves; w++) {
            if (w == wave) before = carry_a;
            carry_a += wtot[0][w];
        }
        const float ang = (float)(before + a_ex);
        // ---- r_rot_quat = (cos, 0, sin, 0) of the angle, not of its half; the rotated velocity of the frame before
        const float cs = cosf(ang), sn = sinf(ang);
        float sx = 0.f, sz = 0.f;
        if (live && t > 0) {
            const float vx = rot_value(p, b, t - 1, 1), vz = rot_value(p, b, t - 1, 2);
            const float uvx = sn * vz, uvz = -(sn * vx);     // u x v with u = (0, sn, 0), then u x (u x v)
            const float uuvx = sn * uvz, uuvz = -(sn * uvx);
            sx = vx + 2.f * (cs * uvx + uuvx);
            sz = vz + 2.f * (cs * uvz + uuvz);
        }
        const double x_in = rot_wave_scan((double)sx, lane), z_in = rot_wave_scan((double)sz, lane);
        if (lane == 63) {
            wtot[1][wave] = x_in;
            wtot[2][wave] = z_in;
        }
        __syncthreads();                     // wtot[0] is written again only behind this barrier, wtot[1..2] only behind the next round's first
        double bx = carry_x, bz = carry_z;
        for (int w = 0; w < kRotWaves; w++) {
            if (w == wave) {
                bx = carry_x;
                bz = carry_z;
            }
            carry_x += wtot[1][w];
            carry_z += wtot[2][w];
        }
        if (!live) continue;                 // no barrier below in this round
        const float r[4] = {cs, 0.f, sn, 0.f};
        const float rp[3] = {(float)(bx + x_in), rot_value(p, b, t, 3), (float)(bz + z_in)};
        if (pass == 0) {                     // (0,1,0) x normalize(across): (across_z, 0, -across_x) / |across|; twin: enc_forward
            float g[4][3], ac[3];
#pragma unroll
            for (int a = 0; a < 4; a++) rot_ric_pos(p, b, t, p.face[a], r, rp, g[a]);
#pragma unroll
            for (int k = 0; k < 3; k++) ac[k] = (g[0][k] - g[1][k]) + (g[2][k] - g[3][k]);
            const float n = sqrtf(rot_dot(ac, ac));
            fwx[t] = ac[2] / n;
            fwz[t] = -(ac[0] / n);
            continue;
        }
        if (root_pos) {
#pragma unroll
            for (int k = 0; k < 3; k++) root_pos[t * 3 + k] = rp[k];
        }
        float S[kRotMaxJoints][16];          // per joint: kRotHml the world quaternion (4), kRotReal the global matrix (9); then the position at 12
        if (p.mode != kRotReal) {
#pragma unroll
            for (int k = 0; k < 4; k++) S[0][k] = r[k];
#pragma unroll
            for (int k = 0; k < 3; k++) S[0][12 + k] = rp[k];
            if (p.mode == kRotPosIk) {
                for (int j = 1; j < J; j++) {
                    float o[3];
                    rot_ric_pos(p, b, t, j, r, rp, o);
#pragma unroll
                    for (int k = 0; k < 3; k++) S[j][12 + k] = o[k];
                }
                // the 161 taps, index clamped into the clip, summed in double, rounded to fp32 where qbetween_np casts; twin: k_encode
                double sx2 = p.taps[0] * (double)fwx[t], sz2 = p.taps[0] * (double)fwz[t];
                for (int k = 1; k <= kRotRadius; k++) {
                    const int lo = max(t - k, 0), hi = min(t + k, len - 1);
                    sx2 += p.taps[k] * ((double)fwx[lo] + (double)fwx[hi]);
                    sz2 += p.taps[k] * ((double)fwz[lo] + (double)fwz[hi]);
                }
                float f[3] = {(float)sx2, 0.f, (float)sz2};
                const float nf = sqrtf(rot_dot(f, f));
                f[0] /= nf;
                f[2] /= nf;
                const float zax[3] = {0.f, 0.f, 1.f};
                float rq[4];
                rot_qbetween(zax, f, rq);
                if (t == 0) {
                    rq[0] = 1.f;
                    rq[1] = rq[2] = rq[3] = 0.f;
                }
                // the chain IK (skeleton.py:88-103), every chain restarting from rq; its local quaternions into world ones from r
                float Rk[4], Rw[4];
                for (int l = 0; l < p.n_links; l++) {
                    if (p.link_first[l]) {
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            Rk[k] = rq[k];
                            Rw[k] = r[k];
                        }
                    }
                    const int c = p.link_child[l], a = p.link_parent[l];
                    float v[3], quv[4], loc[4], Rn[4], Rwn[4];
#pragma unroll
                    for (int k = 0; k < 3; k++) v[k] = S[c][12 + k] - S[a][12 + k];
                    const float nv = sqrtf(rot_dot(v, v));
#pragma unroll
                    for (int k = 0; k < 3; k++) v[k] /= nv;
                    const float u[3] = {p.raw[c][0], p.raw[c][1], p.raw[c][2]};
                    rot_qbetween(u, v, quv);
                    const float Ri[4] = {Rk[0], -Rk[1], -Rk[2], -Rk[3]};
                    rot_qmul(Ri, quv, loc);
                    rot_qmul(Rk, loc, Rn);
                    rot_qmultipy(Rw, loc, Rwn);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        Rk[k] = Rn[k];
                        S[c][k] = Rw[k] = Rwn[k];
                    }
                }
            } else {
            // world quaternions and forward_kinematics_cont6d in one walk over the links
            float M0[9];
            {
                // q2cont6d: the first two columns of q2rotm(r), then cont6d_to_matrix of them
                const float q0 = r[0], q1 = r[1], q2 = r[2], q3 = r[3];
                const float c6[6] = {1.f - 2.f * (q2 * q2) - 2.f * (q3 * q3), 2.f * q1 * q2 + 2.f * q0 * q3, 2.f * q1 * q3 - 2.f * q0 * q2,
                                     2.f * q1 * q2 - 2.f * q0 * q3, 1.f - 2.f * (q1 * q1) - 2.f * (q3 * q3), 2.f * q2 * q3 + 2.f * q0 * q1};
                rot_matrix(c6, M0);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) S[0][k] = r[k];
#pragma unroll
            for (int k = 0; k < 3; k++) S[0][12 + k] = rp[k];
            float R[4], G[9];
            for (int l = 0; l < p.n_links; l++) {
                if (p.link_first[l]) {
#pragma unroll
                    for (int k = 0; k < 4; k++) R[k] = r[k];
#pragma unroll
                    for (int k = 0; k < 9; k++) G[k] = M0[k];
                }
                const int c = p.link_child[l], a = p.link_parent[l];
                float c6[6], M[9], q[4], Rn[4], Gn[9], o[3];
#pragma unroll
                for (int k = 0; k < 6; k++) c6[k] = rot_value(p, b, t, R0 + 6 * (c - 1) + k);
                rot_matrix(c6, M);
                rot_matrix_to_quat(M, q);
                rot_qmultipy(R, q, Rn);
                rot_mul(G, M, Gn);
#pragma unroll
                for (int k = 0; k < 4; k++) S[c][k] = R[k] = Rn[k];
#pragma unroll
                for (int k = 0; k < 9; k++) G[k] = Gn[k];
                const float off[3] = {p.off[c][0], p.off[c][1], p.off[c][2]};
                rot_mv(G, off, o);
#pragma unroll
                for (int k = 0; k < 3; k++) S[c][12 + k] = o[k] + S[a][12 + k];
            }
            }
            if (quats) {
                for (int i = 0; i < Jx; i++) {
                    const int s = p.src[i];
                    float w[4] = {1.f, 0.f, 0.f, 0.f}, q[4];
                    if (s >= 0) {
#pragma unroll
                        for (int k = 0; k < 4; k++) w[k] = S[s][k];
                    }
                    if (i == 0) {
#pragma unroll
                        for (int k = 0; k < 4; k++) q[k] = w[k];
                    } else {
                        const int sa = p.src[p.xparent[i]];
                        float wa[4] = {1.f, 0.f, 0.f, 0.f};
                        if (sa >= 0) {
#pragma unroll
                            for (int k = 0; k < 4; k++) wa[k] = S[sa][k];
                        }
                        const float wi[4] = {wa[0], -wa[1], -wa[2], -wa[3]};
                        rot_qmultipy(wi, w, q);
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++) quats[(t * Jx + i) * 4 + k] = q[k];
                }
            }
        } else {
            // forward_kinematics_real_cont6d in link order (a joint's parent is placed before it), cont6d2q on the way
            for (int l = -1; l < p.n_links; l++) {
                const int c = l < 0 ? 0 : p.link_child[l], a = l < 0 ? 0 : p.link_parent[l];
                float c6[6], M[9], q[4];
#pragma unroll
                for (int k = 0; k < 6; k++) c6[k] = rot_value(p, b, t, R0 + 6 * c + k);
                rot_matrix(c6, M);
                rot_matrix_to_quat(M, q);
                if (l < 0) {
                    float Y[9], G[9], q0[4];
                    rot_quat_matrix(r, Y);
                    rot_mul(Y, M, G);
#pragma unroll
                    for (int k = 0; k < 9; k++) S[0][k] = G[k];
#pragma unroll
                    for (int k = 0; k < 3; k++) S[0][12 + k] = rp[k];
                    rot_qmultipy(r, q, q0);
#pragma unroll
                    for (int k = 0; k < 4; k++) q[k] = q0[k];
                } else {
                    float Ga[9], G[9], o[3];
#pragma unroll
                    for (int k = 0; k < 9; k++) Ga[k] = S[a][k];
                    const float off[3] = {p.off[c][0], p.off[c][1], p.off[c][2]};
                    rot_mv(Ga, off, o);
#pragma unroll
                    for (int k = 0; k < 3; k++) S[c][12 + k] = o[k] + S[a][12 + k];
                    rot_mul(Ga, M, G);
#pragma unroll
                    for (int k = 0; k < 9; k++) S[c][k] = G[k];
                }
                if (quats) {
#pragma unroll
                    for (int k = 0; k < 4; k++) quats[(t * Jx + c) * 4 + k] = q[k];
                }
            }
            if (local) {
                const float ri[4] = {r[0], -r[1], -r[2], -r[3]};
                for (int j = 1; j < J; j++) {
                    // Stated deviation: the reference's `pos[..., 0] -= pos[..., 0:1, 0]` subtracts in place from the storage it reads, so
                    // what it returns depends on how torch splits the loop (a short clip loses the subtraction altogether).  Here the
                    // rows are root-relative, which is what the function is for.
                    const float d[3] = {S[j][12] - S[0][12], S[j][13], S[j][14] - S[0][14]};
                    float o[3];
                    rot_qrot(ri, d, o);
#pragma unroll
                    for (int k = 0; k < 3; k++) local[(t * (J - 1) + (j - 1)) * 3 + k] = o[k];
                }
            }
        }
        if (joints) {
            for (int j = 0; j < J; j++) {
#pragma unroll
                for (int k = 0; k < 3; k++) joints[(t * J + j) * 3 + k] = S[j][12 + k];
            }
        }
    }
    __syncthreads();                         // pass 0's forward rows are complete; wtot is free for the second walk
    }
    // ---- frames at or past the clip's length: exact zeros
    if (quats)
        for (int i = tid + len * Jx * 4; i < T * Jx * 4; i += kRotThreads) quats[i] = 0.f;
    if (root_pos)
        for (int i = tid + len * 3; i < T * 3; i += kRotThreads) root_pos[i] = 0.f;
    if (joints)
        for (int i = tid + len * J * 3; i < T * J * 3; i += kRotThreads) joints[i] = 0.f;
    if (local)
        for (int i = tid + len * (J - 1) * 3; i < T * (J - 1) * 3; i += kRotThreads) local[i] = 0.f;
}

}  // namespace mst
