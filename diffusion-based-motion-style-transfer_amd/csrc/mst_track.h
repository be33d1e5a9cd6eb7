// Pose tracks on the GPU: what the reference does frame by frame around a video pose estimator's output (utils/process_smpl_from_hybrik.py)
// and in the fractional branch of its BVH reader (data_loaders/humanml/common/bvh_utils.py:251-287).
//
//   k_track_resample   `downsample` / `joints_downsample` (process_smpl_from_hybrik.py:56-87) for a rational rate up / down: `qslerp`
//                      (common/quaternion.py:403-418 over `qpow`, :371-398) on quaternion tracks of any joint count, `lerp` (:446-457) on
//                      point tracks.  The reference forms all (T - 1) * up up-sampled frames and keeps every down-th; here output frame k
//                      is computed alone from its source interval i = (k * down) / up and t = ((k * down) % up) / up.
//   k_track_joints     `amass_to_pose` (:89-180) after the file is read: rotation matrices -> quaternions (the closed form of `rotm2q`'s
//                      dominant eigenvector, utils/rotation.py:163-206), the resampling above, `q2axangle` (:234-250), the body model's
//                      joints (Rodrigues, J = J0 + Jdirs beta, the rigid chain over the first 22 joints), the translation, the re-axing
//                      (x and z swapped, y negated), and the estimator's own joint track through the same lerp and re-axing.
//
// No atomics; every store is an ordinary vector store.  One thread (k_track_resample: per clip, output frame and joint or point;
// k_track_joints: per clip and output frame) computes its output from the two source frames of its own interval, which lie inside the
// clip's own length, in one fixed order: a clip's bits depend on neither the batch, its place in it, the stream, nor on what other clips
// or the rows behind its length hold.  Output rows at and behind a clip's output length are exact zeros.
//
// Arithmetic: rotations in float32 as the reference's (its `t` is float64 and so are theta = t * theta0 and the sin / cos of it; here t
// is formed in double, rounded once and everything after is float32).  Points and translations in double, rounded once on the store (the
// reference keeps the translation float64).  No contraction into fused multiply-adds in the quaternion products: for equal ends the
// relative quaternion's vector part then cancels to exact zeros and `qpow`'s 10e-10 guard gives the end itself.
#pragma once
#include <hip/hip_runtime.h>

#include "mst_rotdec.h"      // rot_qmul, rot_mul, rot_mv
#include "mst_smplify.h"     // fit_rodrigues: the one place that states the Rodrigues form

namespace mst {

constexpr int kTrackChain = 22;              // joints the chain walks: what the reference keeps (`[..., :22, :]`)
constexpr int kTrackBetas = 10;
constexpr int kTrackMaxJoints = 4096;        // k_track_resample keeps no table: the bound is only a sanity check on the argument
constexpr int kTrackMaxFrames = 16384;       // source frames of a clip, as mst_bvh_max_frames
constexpr int kTrackMaxRate = 100000;        // up and down, each; (frames - 1) * up stays far inside an int
constexpr int kTrackThreads = 64;

__device__ __forceinline__ void track_qnormalize(const float* q, float* o) {
#pragma clang fp contract(off)
    const float n = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = q[k] / n;
}

// qslerp(q0, q1, t) = qmul(qpow(qmul(q1, qinv(q0)), t), q0), both ends normalised first.  shortest: the relative quaternion is negated
// when its w is negative, so the arc is the shorter one whatever the sign of either end.
__device__ __forceinline__ void track_qslerp(const float* q0, const float* q1, float t, bool shortest, float* o) {
#pragma clang fp contract(off)
    float a[4], b[4], rel[4];
    track_qnormalize(q0, a);
    track_qnormalize(q1, b);
    const float ai[4] = {a[0], -a[1], -a[2], -a[3]};
    rot_qmul(b, ai, rel);
    if (shortest && rel[0] < 0.f) {
#pragma unroll
        for (int k = 0; k < 4; k++) rel[k] = -rel[k];
    }
    float r[4];
    track_qnormalize(rel, r);                // qpow's own qnormalize
    float theta0 = acosf(r[0]);
    if (theta0 <= 10e-10f && theta0 >= -10e-10f) theta0 = 10e-10f;
    const float s0 = sinf(theta0), theta = t * theta0, s = sinf(theta);
    const float p[4] = {cosf(theta), (r[1] / s0) * s, (r[2] / s0) * s, (r[3] / s0) * s};
    rot_qmul(p, a, o);
}

// The quaternion of a rotation matrix (row-major): the dominant eigenvector of rotm2q's K matrix in closed form, on the largest of the
// four diagonal combinations so that the square root's argument is at least 1.  Its sign is this form's, not LAPACK's.
__device__ __forceinline__ void track_rotm2q(const float* M, float* q) {
#pragma clang fp contract(off)
    const float dx = (M[0] - M[4]) - M[8], dy = (M[4] - M[0]) - M[8], dz = (M[8] - M[0]) - M[4], dw = (M[0] + M[4]) + M[8];
    if (dw >= dx && dw >= dy && dw >= dz) {
        const float s = 2.f * sqrtf(1.f + dw);
        q[0] = 0.25f * s;
        q[1] = (M[7] - M[5]) / s;
        q[2] = (M[2] - M[6]) / s;
        q[3] = (M[3] - M[1]) / s;
    } else if (dx >= dy && dx >= dz) {
        const float s = 2.f * sqrtf(1.f + dx);
        q[0] = (M[7] - M[5]) / s;
        q[1] = 0.25f * s;
        q[2] = (M[1] + M[3]) / s;
        q[3] = (M[2] + M[6]) / s;
    } else if (dy >= dz) {
        const float s = 2.f * sqrtf(1.f + dy);
        q[0] = (M[2] - M[6]) / s;
        q[1] = (M[1] + M[3]) / s;
        q[2] = 0.25f * s;
        q[3] = (M[5] + M[7]) / s;
    } else {
        const float s = 2.f * sqrtf(1.f + dz);
        q[0] = (M[3] - M[1]) / s;
        q[1] = (M[2] + M[6]) / s;
        q[2] = (M[5] + M[7]) / s;
        q[3] = 0.25f * s;
    }
}

// q2axangle: the quaternion normalised, theta = 2 acos(w), xyz / sin(theta / 2) * theta, the sine replaced by 0.1 where it is 0
__device__ __forceinline__ void track_q2axangle(const float* q, float* a) {
#pragma clang fp contract(off)
    float n[4];
    track_qnormalize(q, n);
    const float theta = acosf(n[0]) * 2.f;
    float s = sinf(theta / 2.f);
    if (s == 0.f) s = 0.1f;
#pragma unroll
    for (int k = 0; k < 3; k++) a[k] = (n[1 + k] / s) * theta;
}

// The interval and parameter of output frame k: false when the frame does not exist for a clip of `len` source frames.
__device__ __forceinline__ bool track_frame(int k, int len, int up, int down, int& i, double& td) {
    const long long pos = (long long)k * down;
    if (pos >= (long long)(len - 1) * up) return false;
    i = (int)(pos / up);
    td = (double)(pos % up) / (double)up;
    return true;
}

// ------------------------------------------------------------------------------------------ tracks of any joint count
struct TrackResampleArgs {
    const float* quats;                      // [B][T][J][4] or null
    const float* points;                     // [B][T][P][3] or null
    const int* lengths;                      // [B] or null
    int B, T, J, P, Tout, up, down, shortest;
    float* quats_out;                        // [B][Tout][J][4]
    float* points_out;                       // [B][Tout][P][3]
};

__global__ __launch_bounds__(256) void k_track_resample(TrackResampleArgs p) {
    const int E = p.J + p.P;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)p.B * p.Tout * E) return;
    const int e = (int)(idx % E);
    const long long bk = idx / E;
    const int k = (int)(bk % p.Tout), b = (int)(bk / p.Tout);
    int len = p.lengths ? p.lengths[b] : p.T;
    len = min(max(len, 1), p.T);             // no access leaves the clip, whatever the caller wrote
    int i = 0;
    double td = 0.0;
    const bool live = track_frame(k, len, p.up, p.down, i, td);
    if (e < p.J) {
        float* o = p.quats_out + (((size_t)b * p.Tout + k) * p.J + e) * 4;
        float q[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            const float* s = p.quats + (((size_t)b * p.T + i) * p.J + e) * 4;
            const float q0[4] = {s[0], s[1], s[2], s[3]};
            const float* s1 = s + (size_t)p.J * 4;
            const float q1[4] = {s1[0], s1[1], s1[2], s1[3]};
            track_qslerp(q0, q1, (float)td, p.shortest != 0, q);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) o[c] = q[c];
    } else {
        const int pt = e - p.J;
        float* o = p.points_out + (((size_t)b * p.Tout + k) * p.P + pt) * 3;
        float v[3] = {0.f, 0.f, 0.f};
        if (live) {
            const float* s = p.points + (((size_t)b * p.T + i) * p.P + pt) * 3;
            const float* s1 = s + (size_t)p.P * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double p0 = (double)s[c], p1 = (double)s1[c];
                v[c] = (float)(p0 + td * (p1 - p0));
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) o[c] = v[c];
    }
}

// ------------------------------------------------------------------------------------------ the fused video path
struct TrackJointsArgs {
    const float* rot;                        // [B][T][Jr][4] (w first) or [B][T][Jr][3][3]
    int rot_mat, Jr;
    const float* transl;                     // [B][T][3] or null
    const float* betas;                      // [B][10]
    const float* extra;                      // [B][T][Je][3] or null: the estimator's own joints
    int Je;
    const int* lengths;                      // [B] or null
    int B, T, Tout, up, down, shortest, with_trans;
    const float* J0;                         // [22][3]
    const float* Jdirs;                      // [22][3][10]
    signed char parents[kTrackChain];
    float* out;                              // [B][Tout][22][3]
    float* extra_out;                        // [B][Tout][22][3] or null
};

__device__ __forceinline__ void track_load_quat(const TrackJointsArgs& p, size_t frame, int j, float* q) {
    if (p.rot_mat) {
        const float* s = p.rot + (frame * p.Jr + j) * 9;
        float M[9];
#pragma unroll
        for (int k = 0; k < 9; k++) M[k] = s[k];
        track_rotm2q(M, q);
    } else {
        const float* s = p.rot + (frame * p.Jr + j) * 4;
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = s[k];
    }
}

__global__ __launch_bounds__(kTrackThreads) void k_track_joints(const TrackJointsArgs p) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, k = blockIdx.x * kTrackThreads + threadIdx.x;
    if (k >= p.Tout) return;
    int len = p.lengths ? p.lengths[b] : p.T;
    len = min(max(len, 1), p.T);
    float* out = p.out + ((size_t)b * p.Tout + k) * kTrackChain * 3;
    float* eout = p.extra_out ? p.extra_out + ((size_t)b * p.Tout + k) * kTrackChain * 3 : nullptr;
    int i = 0;
    double td = 0.0;
    if (!track_frame(k, len, p.up, p.down, i, td)) {
        for (int e = 0; e < kTrackChain * 3; e++) {
            out[e] = 0.f;
            if (eout) eout[e] = 0.f;
        }
        return;
    }
    const float tf = (float)td;
    const size_t f0 = (size_t)b * p.T + i;   // the interval's first frame; the second, f0 + 1, lies inside the clip's length
    double tr[3] = {0.0, 0.0, 0.0};
    if (p.transl && p.with_trans) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double t0 = (double)p.transl[f0 * 3 + c], t1 = (double)p.transl[(f0 + 1) * 3 + c];
            tr[c] = t0 + td * (t1 - t0);
        }
    }
    float beta[kTrackBetas];
#pragma unroll
    for (int n = 0; n < kTrackBetas; n++) beta[n] = p.betas[(size_t)b * kTrackBetas + n];
    // the chain state of a lane, indexed by `parents`: it lives in scratch memory, as k_smpl_pose's does
    float G[kTrackChain][12], J[kTrackChain][3];
    for (int j = 0; j < kTrackChain; j++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float s = p.J0[j * 3 + c];
#pragma unroll
            for (int n = 0; n < kTrackBetas; n++) s = fmaf(p.Jdirs[(j * 3 + c) * kTrackBetas + n], beta[n], s);
            J[j][c] = s;
        }
        float q0[4], q1[4], q[4], aa[3], R[9];
        track_load_quat(p, f0, j, q0);
        track_load_quat(p, f0 + 1, j, q1);
        track_qslerp(q0, q1, tf, p.shortest != 0 || p.rot_mat != 0, q);
        track_q2axangle(q, aa);
        fit_rodrigues(aa, R);
        if (j == 0) {
#pragma unroll
            for (int e = 0; e < 9; e++) G[0][e] = R[e];
#pragma unroll
            for (int c = 0; c < 3; c++) G[0][9 + c] = J[0][c];
        } else {
            const int a = p.parents[j];
            float Ga[12], Gn[9], rel[3], o[3];
#pragma unroll
            for (int e = 0; e < 12; e++) Ga[e] = G[a][e];
#pragma unroll
            for (int c = 0; c < 3; c++) rel[c] = J[j][c] - J[a][c];
            rot_mul(Ga, R, Gn);
            rot_mv(Ga, rel, o);
#pragma unroll
            for (int e = 0; e < 9; e++) G[j][e] = Gn[e];
#pragma unroll
            for (int c = 0; c < 3; c++) G[j][9 + c] = o[c] + Ga[9 + c];
        }
        // the translation joins in double and the sum is rounded once; then x and z swap and y is negated
        const double x = (double)G[j][9] + tr[0], y = (double)G[j][10] + tr[1], z = (double)G[j][11] + tr[2];
        out[3 * j] = (float)z;
        out[3 * j + 1] = (float)-y;
        out[3 * j + 2] = (float)x;
        if (eout) {
            const float* e0 = p.extra + (f0 * p.Je + j) * 3;
            const float* e1 = e0 + (size_t)p.Je * 3;
            double v[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double a0 = (double)e0[c], a1 = (double)e1[c];
                v[c] = (a0 + td * (a1 - a0)) + tr[c];
            }
            eout[3 * j] = (float)v[2];
            eout[3 * j + 1] = (float)-v[1];
            eout[3 * j + 2] = (float)v[0];
        }
    }
}

}  // namespace mst
