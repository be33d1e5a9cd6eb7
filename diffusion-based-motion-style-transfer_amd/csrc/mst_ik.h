// Joint rotations fitted to joint positions on the GPU: the optimisation inside the reference's `fit_joints_bvh`
// (data_loaders/humanml/common/bvh_utils.py:1811-1846) -- `InverseKinematics_hmlvec` (common/Kinematics.py:30-91) stepping torch's Adam
// through `Skeleton.forward_kinematics_real_cont6d` (common/skeleton.py:200-222) -- and that function's conversion to quaternions
// (common/rotation.py:744-776), two launches per call.
//
// The loss is a sum over frames, every parameter belongs to one frame and Adam is elementwise: each frame is an optimisation of its
// own with 6 J + 7 parameters (J 6D rotations, r_pos, r_rot_quat).
//
//   k_ik_init    one workgroup per clip: the starting point of Kinematics.py:8-44.  a_t = sum_{s<t} data[s][0];
//                r_rot_quat = (cos a, 0, sin a, 0) -- of the angle, not of its half; r_pos = running sum of qrot(r_rot_quat_t,
//                (data[t-1][1], 0, data[t-1][2])) (rotation.py:47-56, no inverse), its y replaced by data[t][3]; cont6d = the last 6 J
//                features.  `data` is read through element strides with an optional mean / std, so the samplers' normalised
//                [B][F][1][T] output needs no torch op in front.  The three running sums are serial, in double, rounded per frame, as
//                torch.cumsum forms them on a CPU.
//   k_ik_solve   one lane per (clip, frame), 64-lane workgroups, no barrier and no atomic: all iterations of a frame run in its lane.
//                Parameters, both Adam moments and the frame's target sit in LDS as [slot][lane] (a lane's column is its own; 21 J + 21
//                floats a lane, 123 KB at J = 22).  The chain state -- G_j and p_j on the way down, the gradients on the way up, 12 J
//                floats a lane -- is a per-lane private array: with it in LDS as well a 64-lane workgroup would need 174 KB at J = 22,
//                more than a CU has, so it lives in scratch memory, which stays in the cache hierarchy (1 KB a lane).
//                Nothing else is written between iterations.  The tail converts to quaternions and runs the final forward kinematics.
//
// The reverse pass works in joint-local frames, which is what lets G and the gradients share storage: with H_j = G_j^T dL/dG_j and
// l_j = G_j^T dL/dp_j (G_j is a rotation),
//     dL/dM_j = M_j H_j          H_parent += M_j H_j M_j^T + (M_j l_j) (x) offset_j          l_parent += M_j l_j
// A leaf has H = 0 exactly, so dL/dM and its 6D gradient are exact zeros and Adam never moves it, as in the reference.
//
// The quirk (measured on the reference): forward_kinematics_real_cont6d builds `lpos` in the storage autograd saved
// as x_raw for the backward of x = x_raw / |x_raw|, so the reference's gradient is
//     dL/dx_raw = g / n - s (g . s) / n^3,   s_j = offset_j (j >= 1), s_0 = the frame's current r_pos
// where the true gradient has x_raw for s.  true_gradient = 0 reproduces the reference; everything else is the true gradient either way.
// Not reproduced: rotm2axangle's SVD branch for an angle that is an exact multiple of pi.
#pragma once
#include <hip/hip_runtime.h>

namespace mst {

constexpr int kIkMaxJoints = 24;             // LDS: (21 J + 21) * 256 bytes = 134 400 at the cap; scratch: 12 J floats a lane
constexpr int kIkMaxFrames = 4096;           // k_ik_init keeps three fp32 rows of `frames` entries in LDS (48 KB at the cap)
constexpr int kIkLanes = 64;

struct IkArgs {
    const float* data;                       // element (b, t, f) at data[b * sb + t * st + f * sf]
    long long sb, st, sf;
    const float* mean;                       // [feats] or null
    const float* stdv;                       // [feats] or null
    const float* target;                     // [B][T][J][3]
    const int* lengths;                      // [B] or null
    int B, T, J, iters, true_gradient;
    int parents[kIkMaxJoints];
    int leaf[kIkMaxJoints];
    float off[kIkMaxJoints][3];              // row 0 unused (the reference overwrites it with r_pos)
    float* cont6d;                           // [B][T][J][6]   in: the starting point; out: the fit
    float* r_pos;                            // [B][T][3]
    float* r_rot;                            // [B][T][4]
    float* positions;                        // [B][T][J][3]
    float* quats;                            // [B][T][J][4]
    float* frame_loss;                       // [B][T][2] or null
    float* grad;                             // [B][T][6 J + 7] or null
};

__device__ __forceinline__ float ik_value(const IkArgs& p, int b, int t, int f) {
#pragma clang fp contract(off)
    const float v = p.data[(long long)b * p.sb + (long long)t * p.st + (long long)f * p.sf];
    return p.mean ? v * p.stdv[f] + p.mean[f] : v;
}

__global__ __launch_bounds__(256) void k_ik_init(IkArgs p) {
#pragma clang fp contract(off)
    extern __shared__ float ik_rows[];                       // ang[T], sx[T], sz[T]
    const int T = p.T, J = p.J, b = blockIdx.x, tid = threadIdx.x;
    float* ang = ik_rows;
    float* sx = ik_rows + T;
    float* sz = ik_rows + 2 * T;
    for (int t = tid; t < T; t += 256) ang[t] = ik_value(p, b, t, 0);
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int t = 0; t < T; t++) {
            const float v = ang[t];
            ang[t] = (float)acc;
            acc += (double)v;
        }
    }
    __syncthreads();
    for (int t = tid; t < T; t += 256) {
        const float cs = cosf(ang[t]), sn = sinf(ang[t]);
        const float vx = t ? ik_value(p, b, t - 1, 1) : 0.f, vz = t ? ik_value(p, b, t - 1, 2) : 0.f;
        const float uvx = sn * vz, uvz = -(sn * vx);         // u x v with u = (0, sn, 0), then u x (u x v)
        const float uuvx = sn * uvz, uuvz = -(sn * uvx);
        sx[t] = vx + 2.f * (cs * uvx + uuvx);
        sz[t] = vz + 2.f * (cs * uvz + uuvz);
        float* q = p.r_rot + ((size_t)b * T + t) * 4;
        q[0] = cs;
        q[1] = 0.f;
        q[2] = sn;
        q[3] = 0.f;
        p.r_pos[((size_t)b * T + t) * 3 + 1] = ik_value(p, b, t, 3);
    }
    __syncthreads();
    if (tid < 2) {
        const float* s = tid ? sz : sx;
        double acc = 0.0;
        for (int t = 0; t < T; t++) {
            acc += (double)s[t];
            p.r_pos[((size_t)b * T + t) * 3 + 2 * tid] = (float)acc;
        }
    }
    const int first = 4 + 3 * (J - 1), n6 = 6 * J;
    for (int i = tid; i < T * n6; i += 256) {
        const int t = i / n6, k = i - t * n6;
        p.cont6d[(size_t)b * T * n6 + i] = ik_value(p, b, t, first + k);
    }
}

// ------------------------------------------------------------------------------------------ 3 x 3 helpers, row-major
__device__ __forceinline__ void ik_mul(const float* A, const float* B, float* C) {            // C = A B
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ void ik_mul_t(const float* A, const float* B, float* C) {          // C = A B^T
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1] + A[3 * r + 2] * B[3 * c + 2];
}
__device__ __forceinline__ void ik_mv(const float* A, const float* v, float* o) {             // o = A v
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = A[3 * r] * v[0] + A[3 * r + 1] * v[1] + A[3 * r + 2] * v[2];
}
__device__ __forceinline__ void ik_tv(const float* A, const float* v, float* o) {             // o = A^T v
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = A[c] * v[0] + A[3 + c] * v[1] + A[6 + c] * v[2];
}
__device__ __forceinline__ void ik_cross(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float ik_dot(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

struct IkFrame {                             // cont6d_to_matrix (quaternion.py:347-363) and what its backward needs
    float xr[3], yr[3], x[3], z[3], n, nz;
};
__device__ __forceinline__ void ik_matrix(const float* c, IkFrame& f, float* M) {
    float zr[3], y[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        f.xr[k] = c[k];
        f.yr[k] = c[3 + k];
    }
    f.n = sqrtf(ik_dot(f.xr, f.xr));
#pragma unroll
    for (int k = 0; k < 3; k++) f.x[k] = f.xr[k] / f.n;
    ik_cross(f.x, f.yr, zr);
    f.nz = sqrtf(ik_dot(zr, zr));
#pragma unroll
    for (int k = 0; k < 3; k++) f.z[k] = zr[k] / f.nz;
    ik_cross(f.z, f.x, y);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        M[3 * k] = f.x[k];
        M[3 * k + 1] = y[k];
        M[3 * k + 2] = f.z[k];
    }
}
// dL/dM -> dL/d(x_raw, y_raw).  s: what the backward of x_raw / |x_raw| reads as x_raw (the quirk), or x_raw itself.
__device__ __forceinline__ void ik_matrix_backward(const float* gM, const IkFrame& f, const float* s, float* g) {
    float gx[3], gy[3], gz[3], t[3], gzr[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        gx[k] = gM[3 * k];
        gy[k] = gM[3 * k + 1];
        gz[k] = gM[3 * k + 2];
    }
    ik_cross(f.x, gy, t);                                   // y = z x x
#pragma unroll
    for (int k = 0; k < 3; k++) gz[k] += t[k];
    ik_cross(gy, f.z, t);
#pragma unroll
    for (int k = 0; k < 3; k++) gx[k] += t[k];
    const float dz = ik_dot(f.z, gz);                        // z = z_raw / |z_raw|
#pragma unroll
    for (int k = 0; k < 3; k++) gzr[k] = (gz[k] - f.z[k] * dz) / f.nz;
    ik_cross(f.yr, gzr, t);                                 // z_raw = x x y_raw
#pragma unroll
    for (int k = 0; k < 3; k++) gx[k] += t[k];
    ik_cross(gzr, f.x, g + 3);
    float sn[3];
#pragma unroll
    for (int k = 0; k < 3; k++) sn[k] = s[k] / f.n;
    const float ds = ik_dot(gx, sn) / f.n;
#pragma unroll
    for (int k = 0; k < 3; k++) g[k] = gx[k] / f.n - sn[k] * ds;
}

struct IkQuat {                              // quaternion_to_matrix (quaternion.py:300-327): q normalised, then 2 / |q_n|^2
    float qn[4], nq, ss, t;
};
__device__ __forceinline__ void ik_quat_matrix(const float* q, IkQuat& w, float* Y) {
    w.nq = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; k++) w.qn[k] = q[k] / w.nq;
    const float r = w.qn[0], i = w.qn[1], j = w.qn[2], k = w.qn[3];
    w.ss = r * r + i * i + j * j + k * k;
    const float t = w.t = 2.f / w.ss;
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
__device__ __forceinline__ void ik_quat_backward(const float* A, const float* q, const IkQuat& w, float* gq) {
    const float r = w.qn[0], i = w.qn[1], j = w.qn[2], k = w.qn[3], t = w.t;
    const float gt = -A[0] * (j * j + k * k) + A[1] * (i * j - k * r) + A[2] * (i * k + j * r) + A[3] * (i * j + k * r) -
                     A[4] * (i * i + k * k) + A[5] * (j * k - i * r) + A[6] * (i * k - j * r) + A[7] * (j * k + i * r) - A[8] * (i * i + j * j);
    float g[4];
    g[0] = t * (-A[1] * k + A[2] * j + A[3] * k - A[5] * i - A[6] * j + A[7] * i);
    g[1] = t * (A[1] * j + A[2] * k + A[3] * j - 2.f * A[4] * i - A[5] * r + A[6] * k + A[7] * r - 2.f * A[8] * i);
    g[2] = t * (-2.f * A[0] * j + A[1] * i + A[2] * r + A[3] * i + A[5] * k - A[6] * r + A[7] * k - 2.f * A[8] * j);
    g[3] = t * (-2.f * A[0] * k - A[1] * r + A[2] * i + A[3] * r - 2.f * A[4] * k + A[5] * j + A[6] * i + A[7] * j);
    const float gss = -4.f * gt / (w.ss * w.ss);              // t = 2 / ss, ss = q_n . q_n
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        g[c] += gss * w.qn[c];
        d += g[c] * w.qn[c];
    }
#pragma unroll
    for (int c = 0; c < 4; c++) gq[c] = (g[c] - w.qn[c] * d) / w.nq;
    (void)q;
}

struct IkAdam {                              // torch/optim/adam.py, _single_tensor_adam: the scalars of one step, formed in double
    float w1, b2, w2, bc2_sqrt, eps, neg_step;
};
__device__ __forceinline__ void ik_adam(float* p, float* m, float* v, float g, const IkAdam& a) {
    const float mm = fmaf(a.w1, g - *m, *m);                  // lerp_(grad, 1 - beta1)
    const float vv = fmaf(a.w2 * g, g, *v * a.b2);            // mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float denom = sqrtf(vv) / a.bc2_sqrt + a.eps;
    *m = mm;
    *v = vv;
    *p += (a.neg_step * mm) / denom;                          // addcdiv_(exp_avg, denom, value = -step_size)
}

__device__ __forceinline__ float ik_gmof(const float* d, float* gd) {          // Kinematics.py:57-63 at sigma 100, and its derivative
    const float s2 = 10000.f;
    float loss = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float x2 = d[k] * d[k], den = s2 + x2;
        loss += (s2 * x2) / den;
        gd[k] = 2.f * s2 * s2 * d[k] / (den * den);
    }
    return loss;
}

// Forward kinematics of the lane's parameters (LDS columns): S[12 j ..] = G_j (9), p_j (3).
__device__ __forceinline__ void ik_forward(const IkArgs& p, const float* par, int J, float* S) {
    float c[6], q[4], M[9], Y[9];
    IkFrame f;
    IkQuat w;
#pragma unroll
    for (int k = 0; k < 6; k++) c[k] = par[k * kIkLanes];
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = par[(6 * J + 3 + k) * kIkLanes];
    ik_matrix(c, f, M);
    ik_quat_matrix(q, w, Y);
    ik_mul(Y, M, S);
#pragma unroll
    for (int k = 0; k < 3; k++) S[9 + k] = par[(6 * J + k) * kIkLanes];
    for (int j = 1; j < J; j++) {
        const float* Sa = S + 12 * p.parents[j];
        float Ga[9], o[3];
#pragma unroll
        for (int k = 0; k < 9; k++) Ga[k] = Sa[k];
#pragma unroll
        for (int k = 0; k < 6; k++) c[k] = par[(6 * j + k) * kIkLanes];
        ik_matrix(c, f, M);
        const float off[3] = {p.off[j][0], p.off[j][1], p.off[j][2]};
        ik_mv(Ga, off, o);
#pragma unroll
        for (int k = 0; k < 3; k++) S[12 * j + 9 + k] = o[k] + Sa[9 + k];
        ik_mul(Ga, M, S + 12 * j);
    }
}

__global__ __launch_bounds__(kIkLanes) void k_ik_solve(IkArgs p) {
    extern __shared__ float ik_lds[];                        // [21 J + 21][64]: parameters, m, v (6 J + 7 each), target (3 J)
    const int J = p.J, T = p.T, NP = 6 * J + 7, lane = threadIdx.x;
    const long long frame = (long long)blockIdx.x * kIkLanes + lane;
    if (frame >= (long long)p.B * T) return;                 // no barrier anywhere below: a lane touches its own LDS column only
    const int b = (int)(frame / T), t = (int)(frame - (long long)b * T);
    const int len = p.lengths ? p.lengths[b] : T;
    const bool run = t < len;
    float* par = ik_lds + lane;
    float* mom = par + NP * kIkLanes;
    float* var = mom + NP * kIkLanes;
    float* tgt = var + NP * kIkLanes;
    float* c_out = p.cont6d + (size_t)frame * 6 * J;
    float* rp_out = p.r_pos + (size_t)frame * 3;
    float* q_out = p.r_rot + (size_t)frame * 4;
    for (int k = 0; k < 6 * J; k++) par[k * kIkLanes] = c_out[k];
    for (int k = 0; k < 3; k++) par[(6 * J + k) * kIkLanes] = rp_out[k];
    for (int k = 0; k < 4; k++) par[(6 * J + 3 + k) * kIkLanes] = q_out[k];
    for (int k = 0; k < NP; k++) {
        mom[k * kIkLanes] = 0.f;
        var[k * kIkLanes] = 0.f;
    }
    for (int k = 0; k < 3 * J; k++) tgt[k * kIkLanes] = p.target[(size_t)frame * 3 * J + k];

    float S[12 * kIkMaxJoints];
    float* grad_out = p.grad ? p.grad + (size_t)frame * NP : nullptr;
    float loss_first = 0.f, loss_last = 0.f;
    if (run) {
        for (int it = 1; it <= p.iters; it++) {
            IkAdam a;
            {
                const double bc1 = 1.0 - pow(0.9, (double)it), bc2 = 1.0 - pow(0.999, (double)it);
                a.w1 = (float)(1.0 - 0.9);
                a.b2 = (float)0.999;
                a.w2 = (float)(1.0 - 0.999);
                a.bc2_sqrt = (float)sqrt(bc2);
                a.eps = 1e-8f;
                a.neg_step = (float)(-(1e-3 / bc1));
            }
            const bool last = it == p.iters;
            ik_forward(p, par, J, S);
            // the loss, and every joint's own position gradient turned into its local frame; G_j makes room for H_j = 0
            float loss = 0.f;
            for (int j = 0; j < J; j++) {
                float* Sj = S + 12 * j;
                float d[3], gd[3], l[3];
#pragma unroll
                for (int k = 0; k < 3; k++) d[k] = Sj[9 + k] - tgt[(3 * j + k) * kIkLanes];
                loss += ik_gmof(d, gd);
                ik_tv(Sj, gd, l);
#pragma unroll
                for (int k = 0; k < 3; k++) Sj[9 + k] = l[k];
#pragma unroll
                for (int k = 0; k < 9; k++) Sj[k] = 0.f;
            }
            if (it == 1) loss_first = loss;
            loss_last = loss;
            // children to parents
            for (int j = J - 1; j >= 0; j--) {
                float* Sj = S + 12 * j;
                float c[6], M[9], l[3], tl[3], g[6];
                IkFrame f;
#pragma unroll
                for (int k = 0; k < 6; k++) c[k] = par[(6 * j + k) * kIkLanes];
#pragma unroll
                for (int k = 0; k < 3; k++) l[k] = Sj[9 + k];
                ik_matrix(c, f, M);
                ik_mv(M, l, tl);
                const bool leaf = p.leaf[j] != 0;
                float gM[9], W[9];
                if (!leaf) {
                    float H[9];
#pragma unroll
                    for (int k = 0; k < 9; k++) H[k] = Sj[k];
                    ik_mul(M, H, gM);
                    ik_mul_t(gM, M, W);
                }
                if (j > 0) {
                    float* Sa = S + 12 * p.parents[j];
                    const float off[3] = {p.off[j][0], p.off[j][1], p.off[j][2]};
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        Sa[9 + r] += tl[r];
#pragma unroll
                        for (int k = 0; k < 3; k++) Sa[3 * r + k] += (leaf ? 0.f : W[3 * r + k]) + tl[r] * off[k];
                    }
                    if (leaf) {                              // dL/dM = 0 exactly: nothing moves, the gradient is zero
                        if (last && grad_out)
                            for (int k = 0; k < 6; k++) grad_out[6 * j + k] = 0.f;
                        continue;
                    }
                    ik_matrix_backward(gM, f, p.true_gradient ? f.xr : off, g);
                } else {
                    // the root: G_0 = Y M_0, so dL/dY = Y (M_0 H_0 M_0^T) and dL/dr_pos = Y (M_0 l_0)
                    float q[4], rp[3], Y[9], gY[9], grp[3], gq[4];
                    IkQuat w;
#pragma unroll
                    for (int k = 0; k < 3; k++) rp[k] = par[(6 * J + k) * kIkLanes];
#pragma unroll
                    for (int k = 0; k < 4; k++) q[k] = par[(6 * J + 3 + k) * kIkLanes];
                    ik_quat_matrix(q, w, Y);
                    if (leaf) {                              // a skeleton of one joint is refused on the host; kept total all the same
#pragma unroll
                        for (int k = 0; k < 9; k++) gM[k] = W[k] = 0.f;
                    }
                    ik_mul(Y, W, gY);
                    ik_mv(Y, tl, grp);
                    ik_quat_backward(gY, q, w, gq);
                    ik_matrix_backward(gM, f, p.true_gradient ? f.xr : rp, g);
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        if (last && grad_out) grad_out[6 * J + k] = grp[k];
                        ik_adam(par + (6 * J + k) * kIkLanes, mom + (6 * J + k) * kIkLanes, var + (6 * J + k) * kIkLanes, grp[k], a);
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (last && grad_out) grad_out[6 * J + 3 + k] = gq[k];
                        ik_adam(par + (6 * J + 3 + k) * kIkLanes, mom + (6 * J + 3 + k) * kIkLanes, var + (6 * J + 3 + k) * kIkLanes, gq[k], a);
                    }
                }
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    if (last && grad_out) grad_out[6 * j + k] = g[k];
                    ik_adam(par + (6 * j + k) * kIkLanes, mom + (6 * j + k) * kIkLanes, var + (6 * j + k) * kIkLanes, g[k], a);
                }
            }
        }
    } else if (grad_out) {
        for (int k = 0; k < NP; k++) grad_out[k] = 0.f;
    }
    if (p.frame_loss) {
        p.frame_loss[(size_t)frame * 2] = loss_first;
        p.frame_loss[(size_t)frame * 2 + 1] = loss_last;
    }

    // ---- the fit, its forward kinematics, and bvh_utils.py:1833-1835: cont6d2q, the root times the normalised r_rot_quat
    ik_forward(p, par, J, S);
    float qr[4];
    {
        float nq = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            qr[k] = par[(6 * J + 3 + k) * kIkLanes];
            q_out[k] = qr[k];
            nq += qr[k] * qr[k];
        }
        nq = sqrtf(nq);
#pragma unroll
        for (int k = 0; k < 4; k++) qr[k] /= nq;
#pragma unroll
        for (int k = 0; k < 3; k++) rp_out[k] = par[(6 * J + k) * kIkLanes];
    }
    for (int j = 0; j < J; j++) {
        float c[6], M[9];
        IkFrame f;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            c[k] = par[(6 * j + k) * kIkLanes];
            c_out[6 * j + k] = c[k];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) p.positions[((size_t)frame * J + j) * 3 + k] = S[12 * j + 9 + k];
        ik_matrix(c, f, M);
        // rotm2axangle (rotation.py:453-474) then axangle2q (:209-232)
        float ac = (M[0] + M[4] + M[8] - 1.f) / 2.f;
        ac = fminf(fmaxf(ac, -1.f), 1.f);
        float th = acosf(ac);
        if (th == 0.f) th = 0.1f;
        const float den = 2.f * sinf(th);
        float aa[3] = {(M[7] - M[5]) / den * th, (M[2] - M[6]) / den * th, (M[3] - M[1]) / den * th};
        const float th2 = sqrtf(ik_dot(aa, aa)), th1 = th2 == 0.f ? 0.1f : th2;
        const float sh = sinf(th2 / 2.f);
        float o[4] = {cosf(th2 / 2.f), aa[0] / th1 * sh, aa[1] / th1 * sh, aa[2] / th1 * sh};
        if (j == 0) {                                        // qmultipy (rotation.py:110-128)
            float v[3];
            ik_cross(qr + 1, o + 1, v);
            const float w0 = qr[0] * o[0] - ik_dot(qr + 1, o + 1);
#pragma unroll
            for (int k = 0; k < 3; k++) v[k] += qr[0] * o[1 + k] + o[0] * qr[1 + k];
            o[0] = w0;
            o[1] = v[0];
            o[2] = v[1];
            o[3] = v[2];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) p.quats[((size_t)frame * J + j) * 4 + k] = o[k];
    }
}

}  // namespace mst
