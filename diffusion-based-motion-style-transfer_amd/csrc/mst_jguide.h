// Joint-space guidance, one launch per batch: the Gaussian log-likelihood of world-space joint positions of a denoised clip and its
// gradient with respect to the clip's normalised feature rows.
//
//   p       = recover_from_ric(x0 * std + mean, J)          data_loaders/humanml/scripts/motion_process.py:389-410, :444-461
//   logp[b] = -1/2 scale[b] sum_{t < len_b, j, c} w (p - y)^2
//   grad    = d logp / d x0                                   [B][F][1][T], the std[f] factor included
//
// Forward: k_recover_from_ric's map (mst_elem.h) -- the yaw quaternion is (cos a, 0, sin a, 0) with the FULL angle a, the exclusive
// running sum of feature 0; root x / z the inclusive running sums of the yaw-rotated features 1 / 2 of the frame before; joint j > 0
// the yaw-rotated features 4 + 3 (j - 1) .. moved to the root's x and z; feature 3 the root's height.  With that quaternion qrot turns
// (x, z) by 2a:  rx = cos 2a x + sin 2a z,  rz = -sin 2a x + cos 2a z,  so d rx / da = 2 rz and d rz / da = -2 rx.
//
// Reverse, by hand in the same launch.  With g = -scale w (p - y) the gradient at a position:
//   frame t, all joints in the order 0 .. J - 1 (one lane, one running sum each):
//       Gx[t], Gz[t] = sum_j g_x, g_z                           d / d (root x, z at t)
//       A[t]         = sum_{j > 0} 2 (g_x rz - g_z rx)          d / d ang[t] through the local positions
//       features 4 ..: the residual turned back (qrot with -sin a), feature 3: g_y of the root
//   velocity frame u (its rotated velocity enters root x / z at every frame > u, turned by ang[u + 1]):
//       E[u]   = sum_{t > u} (Gx, Gz)[t]                        exclusive suffix sums
//       features 1, 2 at u = E[u] turned back by ang[u + 1];    C[u] = 2 (E_x rvz - E_z rvx), its share of d / d ang[u + 1]
//       feature 0 at u = sum_{s > u} (A[s] + C[s]) + C[u]       ang[s] holds the yaw velocity of every frame < s
// which are the suffix sums over t >= s of the root gradients and the exclusive suffix sum of d / d ang of the usual statement, written so
// that every lane stores to its own frame.  The three suffix sums and the three prefix sums of the forward map are workgroup scans in
// double -- a Hillis-Steele tree inside each wave of 64 frames, wave totals and the carry of other rounds added in a fixed order
// (mst_rotdec.h's pattern) -- and rounded to fp32 once per frame.  No atomics; the result of a clip depends on nothing but the clip:
// the same bits alone, anywhere in a batch and from run to run.  Frames at or past the clip's length contribute nothing and receive
// exact zeros, as do the channels the map does not read; both maps are causal, so what such frames hold reaches no output.
//
// One workgroup per clip, one lane per frame in rounds of 256.  LDS per frame: Gx, Gz, A in double and cos / sin of the angle in fp32,
// 32 bytes -- kJgMaxFrames frames fit the 64 KB a launch gets without an opt-in, beside the scans' wave totals.
#pragma once
#include <hip/hip_runtime.h>

namespace mst {

constexpr int kJgThreads = 256;
constexpr int kJgWaves = kJgThreads / 64;
constexpr int kJgFrameBytes = 3 * (int)sizeof(double) + 2 * (int)sizeof(float);
constexpr int kJgMaxFrames = 2040;           // 2040 x 32 B + 128 B of wave totals <= 64 KB; the training node takes 223 frames

struct JGuideArgs {
    const float* x0;                         // [B][F][1][T], normalised
    const float* mean;                       // [F]
    const float* stdv;
    const float* target;                     // [B][T][J][3]
    const float* weight;                     // [B][T][J][3], >= 0
    const float* scale;                      // [B]
    const int* lengths;                      // [B] or null
    int F, T, J;
    float* logp;                             // [B]
    float* grad;                             // [B][F][1][T]
    float* pos;                              // [B][T][J][3] or null
};

// qrot by (c, 0, s, 0) restricted to x and z (quaternion.py:88-99); twin: yaw_rot (mst_elem.h), without contraction
__device__ __forceinline__ void jg_yaw(float c, float s, float vx, float vz, float& ox, float& oz) {
#pragma clang fp contract(off)
    const float uvx = s * vz, uvz = -(s * vx);
    const float uuvx = s * uvz, uuvz = -(s * uvx);
    ox = vx + 2.f * (c * uvx + uuvx);
    oz = vz + 2.f * (c * uvz + uuvz);
}

// inclusive prefix / suffix sum over the wave's 64 lanes, Hillis-Steele
__device__ __forceinline__ double jg_scan_up(double x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(x, d, 64);
        if (lane >= d) x += o;
    }
    return x;
}
__device__ __forceinline__ double jg_scan_down(double x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_down(x, d, 64);
        if (lane + d < 64) x += o;
    }
    return x;
}

__global__ __launch_bounds__(kJgThreads) void k_joint_guide(JGuideArgs p) {
#pragma clang fp contract(off)
    extern __shared__ double jg_rows[];      // Gx[T], Gz[T], A[T] in double, then cs[T], sn[T] in fp32
    __shared__ double wtot[3][kJgWaves];     // per scan: every wave's total of the round
    __shared__ double wsum[kJgWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = p.T, F = p.F, J = p.J;
    int len = p.lengths ? p.lengths[b] : T;
    len = min(max(len, 0), T);               // no access leaves the clip, whatever the caller wrote
    const int R0 = 4 + 3 * (J - 1);          // the channels the map reads: 0 .. R0 - 1
    double* Gx = jg_rows;
    double* Gz = Gx + T;
    double* Ga = Gz + T;
    float* cs = (float*)(Ga + T);
    float* sn = cs + T;
    // offsets inside a clip fit an int (F x T and T x J x 3 at the caps); only the clip's bases are 64-bit
    const float* xb = p.x0 + (size_t)b * F * T;
    float* gb = p.grad + (size_t)b * F * T;
    const float* yb = p.target + (size_t)b * T * J * 3;
    const float* wb = p.weight + (size_t)b * T * J * 3;
    float* pb = p.pos ? p.pos + (size_t)b * T * J * 3 : nullptr;
    const float sc = p.scale[b];
    auto den = [&](int f, int t) { return xb[f * T + t] * p.stdv[f] + p.mean[f]; };

    // ---- forward, frames ascending: angle and root by prefix scans, then the frame's joints, residuals and per-frame gradient sums
    double lp = 0.0;                                         // this lane's share of sum w (p - y)^2
    double carry_a = 0.0, carry_x = 0.0, carry_z = 0.0;      // the sums of all earlier rounds: every lane forms the same three numbers
    for (int base = 0; base < len; base += kJgThreads) {
        const int t = base + tid;
        const bool live = t < len;
        const double a_in = jg_scan_up(live ? (double)den(0, t) : 0.0, lane);
        double a_ex = __shfl_up(a_in, 1, 64);
        if (lane == 0) a_ex = 0.0;
        if (lane == 63) wtot[0][wave] = a_in;
        __syncthreads();
        double before = carry_a;
        for (int w = 0; w < kJgWaves; w++) {
            if (w == wave) before = carry_a;
            carry_a += wtot[0][w];
        }
        const float ang = (float)(before + a_ex);
        float s_, c_;
        sincosf(ang, &s_, &c_);
        float sx = 0.f, sz = 0.f;
        if (live && t > 0) jg_yaw(c_, s_, den(1, t - 1), den(2, t - 1), sx, sz);
        const double x_in = jg_scan_up((double)sx, lane), z_in = jg_scan_up((double)sz, lane);
        if (lane == 63) {
            wtot[1][wave] = x_in;
            wtot[2][wave] = z_in;
        }
        __syncthreads();                     // wtot[0] is written again only behind this barrier, wtot[1..2] only behind the next round's first
        double bx = carry_x, bz = carry_z;
        for (int w = 0; w < kJgWaves; w++) {
            if (w == wave) {
                bx = carry_x;
                bz = carry_z;
            }
            carry_x += wtot[1][w];
            carry_z += wtot[2][w];
        }
        if (!live) continue;                 // no barrier below in this round
        const float px = (float)(bx + x_in), pz = (float)(bz + z_in);
        double gx = 0.0, gz = 0.0, ga = 0.0;
        for (int j = 0; j < J; j++) {        // the joints in their order: one running sum each
            float q[3], rx = 0.f, rz = 0.f;
            const int f = j == 0 ? 3 : 4 + 3 * (j - 1);
            if (j == 0) {
                q[0] = px;
                q[1] = den(3, t);
                q[2] = pz;
            } else {
                jg_yaw(c_, s_, den(f, t), den(f + 2, t), rx, rz);
                q[0] = rx + px;
                q[1] = den(f + 1, t);
                q[2] = rz + pz;
            }
            const int o = (t * J + j) * 3;
            float g[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (pb) pb[o + k] = q[k];
                const float w = wb[o + k];
                const float d = q[k] - yb[o + k];
                const float wd = w != 0.f ? w * d : 0.f;     // weight 0: unconstrained, whatever the target holds
                lp += (double)wd * (double)d;
                g[k] = -(sc * wd);
            }
            gx += (double)g[0];
            gz += (double)g[2];
            if (j == 0) {
                gb[3 * T + t] = g[1] * p.stdv[3];
            } else {
                ga += (double)(2.f * (g[0] * rz - g[2] * rx));
                float hx, hz;
                jg_yaw(c_, -s_, g[0], g[2], hx, hz);
                gb[f * T + t] = hx * p.stdv[f];
                gb[(f + 1) * T + t] = g[1] * p.stdv[f + 1];
                gb[(f + 2) * T + t] = hz * p.stdv[f + 2];
            }
        }
        Gx[t] = gx;
        Gz[t] = gz;
        Ga[t] = ga;
        cs[t] = c_;
        sn[t] = s_;
    }

    // ---- logp: the lanes' shares down a fixed tree, the waves' in order
    {
        double s = lp;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
        if (lane == 0) wsum[wave] = s;
    }
    __syncthreads();                         // the rows are complete; wtot is free for the reverse walk
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < kJgWaves; w++) s += wsum[w];
        p.logp[b] = (float)(-0.5 * (double)sc * s);
    }

    // ---- reverse, frames descending: suffix scans of the root gradients, then of d / d ang
    double carry_gx = 0.0, carry_gz = 0.0, carry_h = 0.0;    // the sums of all later rounds
    for (int base = ((len - 1) / kJgThreads) * kJgThreads; len > 0 && base >= 0; base -= kJgThreads) {
        const int t = base + tid;
        const bool live = t < len;
        const double x_in = jg_scan_down(live ? Gx[t] : 0.0, lane), z_in = jg_scan_down(live ? Gz[t] : 0.0, lane);
        double x_ex = __shfl_down(x_in, 1, 64), z_ex = __shfl_down(z_in, 1, 64);
        if (lane == 63) x_ex = z_ex = 0.0;
        if (lane == 0) {
            wtot[0][wave] = x_in;
            wtot[1][wave] = z_in;
        }
        __syncthreads();
        double ax = carry_gx, az = carry_gz;
        for (int w = kJgWaves - 1; w >= 0; w--) {
            if (w == wave) {
                ax = carry_gx;
                az = carry_gz;
            }
            carry_gx += wtot[0][w];
            carry_gz += wtot[1][w];
        }
        // E[t]: what the frames behind t ask of the root; it reaches this frame's velocity turned by the NEXT frame's angle
        float hx = 0.f, hz = 0.f, cn = 0.f;
        if (live && t + 1 < len) {
            const float ex = (float)(ax + x_ex), ez = (float)(az + z_ex);
            const float c1 = cs[t + 1], s1 = sn[t + 1];
            float rvx, rvz;
            jg_yaw(c1, s1, den(1, t), den(2, t), rvx, rvz);
            jg_yaw(c1, -s1, ex, ez, hx, hz);
            cn = 2.f * (ex * rvz - ez * rvx);
        }
        const double h_in = jg_scan_down(live ? Ga[t] + (double)cn : 0.0, lane);
        double h_ex = __shfl_down(h_in, 1, 64);
        if (lane == 63) h_ex = 0.0;
        if (lane == 0) wtot[2][wave] = h_in;
        __syncthreads();                     // wtot[0..1] are written again only behind this barrier, wtot[2] only behind the next round's first
        double ah = carry_h;
        for (int w = kJgWaves - 1; w >= 0; w--) {
            if (w == wave) ah = carry_h;
            carry_h += wtot[2][w];
        }
        if (!live) continue;
        gb[t] = (float)((ah + h_ex) + (double)cn) * p.stdv[0];
        gb[T + t] = hx * p.stdv[1];
        gb[2 * T + t] = hz * p.stdv[2];
    }

    // ---- exact zeros: the channels the map does not read, and in the others the frames at or past the clip's length
    for (int i = R0 * T + tid; i < F * T; i += kJgThreads) gb[i] = 0.f;
    const int pad = T - len;
    for (int i = tid; i < R0 * pad; i += kJgThreads) {
        const int f = i / pad;
        gb[f * T + len + (i - f * pad)] = 0.f;
    }
    if (pb)
        for (int i = len * J * 3 + tid; i < T * J * 3; i += kJgThreads) pb[i] = 0.f;
}

}  // namespace mst
