// Joint positions (and rotations) encoded into the model's feature rows on the GPU: the reference's `process_file_with_rotation`
// (data_loaders/humanml/common/bvh_utils.py:1091-1287, the 9 J + 1 "posrot" layout mst_fit_joints reads) and `process_file`
// (:898-1088, the 12 J - 1 HumanML layout), followed by the z-normalisation and zero padding of `process_np_motion`
// (data_loaders/humanml/data/dataset.py:484-519), one launch.
//
// One workgroup per clip, lanes walk frames, every stage over the clip's own length `len` (clamped into 2 .. frames), never the padded
// frame count.  No atomics; every store is an ordinary vector store.
//
//   floor        the minimum of y over all frames and joints (a tree through LDS), subtracted
//   origin       frame 0's root x and z, subtracted from every joint
//   facing       across = (r_hip - l_hip) + (sdr_r - sdr_l) of frame 0, forward_init = normalize((0,1,0) x normalize(across)),
//                q_init = quatbetween(forward_init, (0,0,1)) (common/rotation.py:97-108); every position is rotated by it (these are the
//                `global_positions`), and in POSROT the root rotation becomes q_init (x) rot
//   root         Skeleton.inverse_kinematics_np(smooth_forward=True) (common/skeleton.py:55-86): forward = (0,1,0) x normalize(across)
//                per frame -- its y is exactly zero, so x and z alone are kept, two fp32 rows in LDS -- smoothed by scipy's
//                gaussian_filter1d(sigma 20): 161 normalised taps, mode 'nearest' = index clamped into [0, len - 1].  The taps come
//                from the host in double and the sum is taken in double (the reference filters float64), then rounded to fp32 where
//                the reference's qbetween_np casts.  r_rot = qbetween((0,0,1), forward) (common/quaternion.py:421-431), identity at
//                frame 0; one quaternion a frame in LDS, because frame t also reads r_rot[t + 1].
//   row t        (t < len - 1) [arcsin(clamped y of r_rot[t+1] (x) r_rot[t]^-1), x and z of qinv(r_rot[t+1]) applied to root[t+1] - root[t],
//                root height], the J - 1 local positions (root x, z subtracted, rotated by qinv(r_rot[t])), the rotations -- POSROT:
//                6D of all J given quaternions (quaternion_to_matrix, common/quaternion.py:300-327), the root one multiplied from the left
//                by qinv(r_rot[t]); HML: the chain IK (skeleton.py:88-103), every chain restarting from the frame's root quaternion, 6D of
//                q2rotm (common/rotation.py:139-160) for joints 1 .. J - 1 -- and in HML the J local velocities and four foot contacts.
//
// The global positions of frame t + 1 (root velocity, local velocities, contacts) are recomputed from the input by the lane of frame t:
// the same instructions on the same operands, so they are the values the lane of frame t + 1 forms, and LDS holds 24 bytes a frame
// whatever the joint count.
// Stated deviation: the arcsin argument is clamped into [-1, 1] (the reference returns NaN past 1).  Not imitated or hidden: a
// zero-length bone in HML mode divides by zero in the chain IK, here as in the reference (NaN in that joint's rotation columns).
#pragma once
#include <hip/hip_runtime.h>

namespace mst {

constexpr int kEncMaxJoints = 24;
constexpr int kEncMaxFrames = 2048;          // LDS: forward x, forward z (fp32) and r_rot (4 fp32) per frame, 24 bytes: 48 KB at the cap
constexpr int kEncRadius = 80;               // int(4 * 20 + 0.5): scipy's truncate = 4 at sigma 20
constexpr int kEncThreads = 256;
constexpr int kEncPosRot = 0, kEncHml = 1;

struct EncArgs {
    const float* pos;                        // [B][T][J][3]
    const float* rot;                        // [B][T][J][4] or null (HML)
    const int* lengths;                      // [B] or null
    const float* mean;                       // [feats] or null
    const float* stdv;
    int B, T, J, mode, frames_out, feats;
    float feet_thre;
    int face[4];                             // r_hip, l_hip, sdr_r, sdr_l
    int fid[4];                              // fid_l[0..1], fid_r[0..1]
    int n_links;                             // HML: the chains, link by link in the reference's order
    int link_child[kEncMaxJoints], link_parent[kEncMaxJoints], link_first[kEncMaxJoints];   // first: R restarts from the root quaternion
    int named[kEncMaxJoints];                // a joint no chain names keeps the reference's all-zero quaternion
    float raw[kEncMaxJoints][3];
    double taps[kEncRadius + 1];             // taps[|k|], normalised
    float* sample;                           // [B][feats][1][frames_out]
    int* out_len;                            // [B]
    float* glob;                             // [B][T][J][3] or null
    float* local;                            // [B][T][J][3] or null
    float* lvel;                             // [B][T-1][2] or null
};

__device__ __forceinline__ void enc_cross(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float enc_dot(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void enc_qrot(const float* q, const float* v, float* o) {          // quaternion.py:88-99
    float uv[3], uuv[3];
    enc_cross(q + 1, v, uv);
    enc_cross(q + 1, uv, uuv);
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = v[k] + 2.f * (q[0] * uv[k] + uuv[k]);
}
__device__ __forceinline__ void enc_qinv(const float* q, float* o) {
    o[0] = q[0];
    o[1] = -q[1];
    o[2] = -q[2];
    o[3] = -q[3];
}
__device__ __forceinline__ void enc_qmul(const float* a, const float* b, float* o) {           // a (x) b
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
__device__ __forceinline__ void enc_qbetween(const float* v0, const float* v1, float* q) {     // quaternion.py:421-431
    enc_cross(v0, v1, q + 1);
    q[0] = sqrtf(enc_dot(v0, v0) * enc_dot(v1, v1)) + enc_dot(v0, v1);
    const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] /= n;
}
// the first two columns of q2rotm (rotation.py:139-160; q as it is): M00, M10, M20, M01, M11, M21
__device__ __forceinline__ void enc_cont6d(const float* q, float two, float* c) {
    const float r = q[0], i = q[1], j = q[2], k = q[3];
    c[0] = 1.f - two * (j * j + k * k);
    c[1] = two * (i * j + k * r);
    c[2] = two * (i * k - j * r);
    c[3] = two * (i * j - k * r);
    c[4] = 1.f - two * (i * i + k * k);
    c[5] = two * (j * k + i * r);
}

struct EncClip {                             // what turns an input position into a global one
    const float* in;
    float floor, ox, oz, qi[4];
    int J;
};
__device__ __forceinline__ void enc_global(const EncClip& c, int t, int j, float* g) {
    const float* s = c.in + ((size_t)t * c.J + j) * 3;
    const float v[3] = {s[0] - c.ox, s[1] - c.floor, s[2] - c.oz};
    enc_qrot(c.qi, v, g);
}
// (0,1,0) x normalize(across): (across_z, 0, -across_x) / |across|
__device__ __forceinline__ void enc_forward(const float* a, const float* b, const float* c, const float* d, float& fx, float& fz) {
    float ac[3];
#pragma unroll
    for (int k = 0; k < 3; k++) ac[k] = (a[k] - b[k]) + (c[k] - d[k]);
    const float n = sqrtf(enc_dot(ac, ac));
    fx = ac[2] / n;
    fz = -(ac[0] / n);
}

__global__ __launch_bounds__(kEncThreads) void k_encode(EncArgs p) {
    extern __shared__ float enc_rows[];      // fwd_x[T], fwd_z[T], r_rot[T][4]
    __shared__ float red[kEncThreads];
    const int b = blockIdx.x, tid = threadIdx.x, T = p.T, J = p.J, F = p.feats, fo = p.frames_out;
    int len = p.lengths ? p.lengths[b] : T;
    len = min(max(len, 2), T);               // no access leaves the clip, whatever the caller wrote
    const int rows = min(len - 1, fo);
    float* fwx = enc_rows;
    float* fwz = enc_rows + T;
    float* rq = enc_rows + 2 * T;
    EncClip c;
    c.in = p.pos + (size_t)b * T * J * 3;
    c.J = J;

    // ---- floor
    float m = INFINITY;
    for (int i = tid; i < len * J; i += kEncThreads) m = fminf(m, c.in[(size_t)i * 3 + 1]);
    red[tid] = m;
    __syncthreads();
    for (int s = kEncThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fminf(red[tid], red[tid + s]);
        __syncthreads();
    }
    c.floor = red[0];
    c.ox = c.in[0];
    c.oz = c.in[2];
    // ---- initial facing: frame 0 before the origin shift (a difference of joints; y carries the floor shift as in the reference)
    {
        float q[4][3];
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const float* s = c.in + (size_t)p.face[a] * 3;
            q[a][0] = s[0];
            q[a][1] = s[1] - c.floor;
            q[a][2] = s[2];
        }
        float f[3] = {0.f, 0.f, 0.f};
        enc_forward(q[0], q[1], q[2], q[3], f[0], f[2]);
        const float n = sqrtf(enc_dot(f, f));
        f[0] /= n;
        f[2] /= n;
        const float z[3] = {0.f, 0.f, 1.f};
        enc_qbetween(f, z, c.qi);
    }
    // ---- forward per frame, from the rotated positions
    for (int t = tid; t < len; t += kEncThreads) {
        float g[4][3];
#pragma unroll
        for (int a = 0; a < 4; a++) enc_global(c, t, p.face[a], g[a]);
        enc_forward(g[0], g[1], g[2], g[3], fwx[t], fwz[t]);
    }
    __syncthreads();
    // ---- the 161 taps, index clamped into the clip; r_rot
    for (int t = tid; t < len; t += kEncThreads) {
        double sx = p.taps[0] * (double)fwx[t], sz = p.taps[0] * (double)fwz[t];
        for (int k = 1; k <= kEncRadius; k++) {
            const int lo = max(t - k, 0), hi = min(t + k, len - 1);
            sx += p.taps[k] * ((double)fwx[lo] + (double)fwx[hi]);
            sz += p.taps[k] * ((double)fwz[lo] + (double)fwz[hi]);
        }
        float f[3] = {(float)sx, 0.f, (float)sz};
        const float n = sqrtf(enc_dot(f, f));
        f[0] /= n;
        f[2] /= n;
        const float z[3] = {0.f, 0.f, 1.f};
        float q[4];
        enc_qbetween(z, f, q);
        if (t == 0) {
            q[0] = 1.f;
            q[1] = q[2] = q[3] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) rq[4 * t + k] = q[k];
    }
    __syncthreads();

    // ---- rows
    float* out = p.sample + (size_t)b * F * fo;
    const int R0 = 4 + 3 * (J - 1);
    for (int t = tid; t < len; t += kEncThreads) {
        const bool write = t < rows, next = t + 1 < len;
        auto put = [&](int f, float v) {
            if (write) out[(size_t)f * fo + t] = p.mean ? (v - p.mean[f]) / p.stdv[f] : v;
        };
        float r[4], ri[4], r1[4], root[3];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            r[k] = rq[4 * t + k];
            r1[k] = rq[4 * (next ? t + 1 : t) + k];
        }
        enc_qinv(r, ri);
        enc_global(c, t, 0, root);
        if (next) {
            float root1[3], r1i[4], d[3], v[3], q[4];
            enc_global(c, t + 1, 0, root1);
#pragma unroll
            for (int k = 0; k < 3; k++) d[k] = root1[k] - root[k];
            enc_qinv(r1, r1i);
            enc_qrot(r1i, d, v);
            enc_qmul(r1, ri, q);
            put(0, asinf(fminf(fmaxf(q[2], -1.f), 1.f)));
            put(1, v[0]);
            put(2, v[2]);
            if (p.lvel) {
                float* lv = p.lvel + ((size_t)b * (T - 1) + t) * 2;
                lv[0] = v[0];
                lv[1] = v[2];
            }
        }
        for (int j = 0; j < J; j++) {
            float g[3], l[3];
            enc_global(c, t, j, g);
            const float s[3] = {g[0] - root[0], g[1], g[2] - root[2]};
            enc_qrot(ri, s, l);
            const size_t o = (((size_t)b * T + t) * J + j) * 3;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (p.glob) p.glob[o + k] = g[k];
                if (p.local) p.local[o + k] = l[k];
            }
            if (j == 0) {
                put(3, l[1]);
            } else {
#pragma unroll
                for (int k = 0; k < 3; k++) put(4 + 3 * (j - 1) + k, l[k]);
            }
        }
        if (!write) continue;
        if (p.mode == kEncPosRot) {
            const float* rot = p.rot + ((size_t)b * T + t) * J * 4;
            for (int j = 0; j < J; j++) {
                float q[4] = {rot[4 * j], rot[4 * j + 1], rot[4 * j + 2], rot[4 * j + 3]}, c6[6];
                if (j == 0) {
                    float a[4];
                    enc_qmul(c.qi, q, a);
                    enc_qmul(ri, a, q);
                }
                // quaternion_to_matrix: q normalised, then 2 / |q_n|^2
                const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
                for (int k = 0; k < 4; k++) q[k] /= n;
                enc_cont6d(q, 2.f / (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), c6);
#pragma unroll
                for (int k = 0; k < 6; k++) put(R0 + 6 * j + k, c6[k]);
            }
        } else {
            for (int j = 1; j < J; j++)
                if (!p.named[j]) {            // q2rotm of the all-zero quaternion
#pragma unroll
                    for (int k = 0; k < 6; k++) put(R0 + 6 * (j - 1) + k, k == 0 || k == 4 ? 1.f : 0.f);
                }
            float R[4] = {r[0], r[1], r[2], r[3]};
            for (int l = 0; l < p.n_links; l++) {
                if (p.link_first[l]) {
#pragma unroll
                    for (int k = 0; k < 4; k++) R[k] = r[k];
                }
                const int ch = p.link_child[l];
                float gc[3], gp[3], v[3], quv[4], Ri[4], loc[4], Rn[4], c6[6];
                enc_global(c, t, ch, gc);
                enc_global(c, t, p.link_parent[l], gp);
#pragma unroll
                for (int k = 0; k < 3; k++) v[k] = gc[k] - gp[k];
                const float n = sqrtf(enc_dot(v, v));
#pragma unroll
                for (int k = 0; k < 3; k++) v[k] /= n;
                const float u[3] = {p.raw[ch][0], p.raw[ch][1], p.raw[ch][2]};
                enc_qbetween(u, v, quv);
                enc_qinv(R, Ri);
                enc_qmul(Ri, quv, loc);
                enc_qmul(R, loc, Rn);
#pragma unroll
                for (int k = 0; k < 4; k++) R[k] = Rn[k];
                enc_cont6d(loc, 2.f, c6);
#pragma unroll
                for (int k = 0; k < 6; k++) put(R0 + 6 * (ch - 1) + k, c6[k]);
            }
            const int V0 = R0 + 6 * (J - 1), C0 = V0 + 3 * J;
            for (int j = 0; j < J; j++) {
                float g0[3], g1[3], d[3], v[3];
                enc_global(c, t, j, g0);
                enc_global(c, t + 1, j, g1);
#pragma unroll
                for (int k = 0; k < 3; k++) d[k] = g1[k] - g0[k];
                enc_qrot(ri, d, v);
#pragma unroll
                for (int k = 0; k < 3; k++) put(V0 + 3 * j + k, v[k]);
            }
#pragma unroll
            for (int a = 0; a < 4; a++) {
                float g0[3], g1[3];
                enc_global(c, t, p.fid[a], g0);
                enc_global(c, t + 1, p.fid[a], g1);
                const float dx = g1[0] - g0[0], dy = g1[1] - g0[1], dz = g1[2] - g0[2];
                put(C0 + a, (dx * dx + dy * dy) + dz * dz < p.feet_thre ? 1.f : 0.f);
            }
        }
    }
    // ---- padding: exact zeros from the clip's last row on (the reference pads after normalising); optional outputs past the clip
    const int pad = fo - rows;
    for (int i = tid; i < F * pad; i += kEncThreads) {
        const int f = i / pad;
        out[(size_t)f * fo + rows + (i - f * pad)] = 0.f;
    }
    for (int i = tid + len * J * 3; i < T * J * 3; i += kEncThreads) {
        if (p.glob) p.glob[(size_t)b * T * J * 3 + i] = 0.f;
        if (p.local) p.local[(size_t)b * T * J * 3 + i] = 0.f;
    }
    if (p.lvel)
        for (int i = tid + (len - 1) * 2; i < (T - 1) * 2; i += kEncThreads) p.lvel[(size_t)b * (T - 1) * 2 + i] = 0.f;
    if (tid == 0) p.out_len[b] = rows;
}

}  // namespace mst
