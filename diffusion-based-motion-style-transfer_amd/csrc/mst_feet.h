// Foot-skate cleanup of finished joint clips on the GPU: the reference's `remove_fs`
// (data_loaders/humanml/common/bvh_utils.py:1685-1809) with its two contact detectors (`get_foot_contact_by_vel_acc` :1591-1639,
// `get_foot_contact_by_vel3` :1642-1682) and its forward-backward `Butterworth` low-pass (:1872-1916), one launch per call.
//
// One workgroup per clip [T][J][3] fp32 (what k_recover_from_ric writes).  The stages run in the reference's order, each behind a
// workgroup barrier, on the clip's own rows of `out`:
//   contacts   from the reference motion as it was on entry (null: the clip itself, read before anything is written), kept as two
//              byte maps [4][T] in dynamic LDS -- the detector's own bits and, under use_window, the refined ones
//   filter     (use_butterworth) cut-off 3 over every joint coordinate
//   floor      y -= min y over all joints and valid frames
//   runs       the thread at the first frame of a maximal contact run sums the run serially in fp32, in frame order, as the
//              reference's `avg +=` does, divides by the count and writes the mean to every frame of the run
//   blend      one thread per (foot, non-contact frame): nearest contact frame within interp_length on either side, alpha(t) =
//              2t^3 - 3t^2 + 1 evaluated in double (the reference's Python floats) and rounded to fp32 where numpy rounds it
//   filter     (after_butterworth) cut-off 2.5
// Every stage sees frames 0 .. len-1 only; frames from len on are copied through.  The four feet are distinct joints (the host
// refuses duplicates), so the reference's loop over feet carries no dependence and the feet run side by side.
//
// Every function here switches floating-point contraction off: the reference's expressions round after every operation (numpy and
// Python floats have no fused multiply-add), and the run means, the blend and the filter recursion follow them operation by operation.
#pragma once
#include <hip/hip_runtime.h>

namespace mst {

constexpr int kFeetMaxFrames = 4096;         // two byte maps of 4 * frames entries in LDS: 32 KB at the cap, below the 64 KB opt-in
constexpr int kFeetWindow = 3;               // use_window: bvh_utils.py:1628
constexpr float kFeetWindowHeight = 0.006f;  // :1636

struct FeetArgs {
    const float* in;          // [B][T][J][3]
    float* out;               // [B][T][J][3], may be `in`; null: contacts and velocities only
    const float* ref;         // [B or 1][T][J][3] or null (the clip itself as it was on entry)
    long long ref_stride;     // T * J * 3, or 0 when one reference serves every clip
    const int* lengths;       // [B] or null (every clip T frames)
    int T, J;
    int fid[4];
    int vel3, use_window, force_on_floor, interp_length, filter_before, filter_after;
    float thr;
    double kb[5], ka[5];      // a, b, c, d, e of the recursion for cut-off 3 and 2.5
    double* ws;               // [B][T-1][J*3] forward result of the filter (only read when a filter is on)
    int* contacts;            // [B][T][4] or null
    float* foot_vels;         // [B][T-1][4] or null
};

// Butterworth over the columns x[0..n-1][col] of one clip, in place; y is this clip's [n-1][C] workspace.  One lane per column:
// the recursion is 2 (n - 1) dependent steps in double.  The reference pads two samples on each side (Dat2 = x0 x0 x0 .. x_{n-1} x_{n-1}),
// runs s = 2 .. n forwards (so x_{n-1} never enters), repeats the last forward value twice, runs backwards to 0 and copies n - 1
// values back: the last frame keeps its unfiltered value.  Loads are issued eight steps ahead of the chain that consumes them.
__device__ __forceinline__ void feet_butterworth(float* x, double* y, int n, int C, double a, double b, double c, double d, double e) {
#pragma clang fp contract(off)
    for (int col = threadIdx.x; col < C; col += blockDim.x) {
        const double x0 = (double)x[col];
        double x1 = x0, x2 = x0, y1 = x0, y2 = x0;
        for (int r0 = 0; r0 < n - 1; r0 += 8) {
            double xs[8];
#pragma unroll
            for (int u = 0; u < 8; u++) xs[u] = (double)x[(size_t)min(r0 + u, n - 2) * C + col];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (r0 + u < n - 1) {
                    const double yy = a * xs[u] + b * x1 + c * x2 + d * y1 + e * y2;
                    y[(size_t)(r0 + u) * C + col] = yy;
                    x2 = x1; x1 = xs[u]; y2 = y1; y1 = yy;
                }
            }
        }
        double yb = y1, yc = y1, z1 = y1, z2 = y1;
        for (int i0 = n - 2; i0 >= 0; i0 -= 8) {
            double ys[8];
#pragma unroll
            for (int u = 0; u < 8; u++) ys[u] = y[(size_t)max(i0 - u, 0) * C + col];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (i0 - u >= 0) {
                    const double z = a * ys[u] + b * yb + c * yc + d * z1 + e * z2;
                    x[(size_t)(i0 - u) * C + col] = (float)z;
                    yc = yb; yb = ys[u]; z2 = z1; z1 = z;
                }
            }
        }
    }
}

__device__ __forceinline__ float feet_lerp(double a, float l, float r) {       // (1 - a) * l + a * r with a a Python float:
#pragma clang fp contract(off)                                                  // numpy rounds both factors to fp32 first
    const float c1 = (float)(1.0 - a), c2 = (float)a;
    return c1 * l + c2 * r;
}

__device__ __forceinline__ double feet_alpha(double t) {
#pragma clang fp contract(off)
    return 2.0 * t * t * t - 3.0 * t * t + 1;
}

__device__ __forceinline__ void feet_sync() {
    __threadfence_block();       // the stages hand rows of `out` from one thread to another through global memory
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_remove_fs(FeetArgs p) {
#pragma clang fp contract(off)
    extern __shared__ unsigned char feet_lds[];              // raw[4][T], then refined[4][T]
    __shared__ float wave_min[4];
    const int T = p.T, J = p.J, C = 3 * J, b = blockIdx.x, tid = threadIdx.x;
    int n = p.lengths ? p.lengths[b] : T;
    n = min(max(n, 2), T);                                   // the caller checks 2 <= len <= T; nothing here indexes outside the clip
    const size_t clip = (size_t)T * C;
    const float* in = p.in + (size_t)b * clip;
    float* out = p.out ? p.out + (size_t)b * clip : nullptr;
    const float* ref = p.ref ? p.ref + (size_t)b * p.ref_stride : in;
    unsigned char* raw = feet_lds;
    unsigned char* fixed = p.use_window && !p.vel3 ? feet_lds + 4 * T : feet_lds;

    // ---- contacts (and the velocities the detector compared), from the reference motion
    for (int i = tid; i < 4 * T; i += 256) {
        const int t = i >> 2, f = i & 3;
        const float* q = ref + (size_t)t * C + 3 * p.fid[f];
        float vel = 0.f;
        bool hit = false;
        if (t < n - 1) {
            if (p.vel3) {
                const float dx = q[C] - q[0], dy = q[C + 1] - q[1], dz = q[C + 2] - q[2];
                vel = sqrtf(dx * dx + dy * dy + dz * dz);
                hit = vel < p.thr;
            } else {
                vel = q[C + 1] - q[1];                       // v[t]; the frame's contact compares v[t-1] and v[t]
                if (t >= 1) {
                    const float vp = q[1] - q[1 - C];
                    hit = (fabsf(vp) < p.thr && vel - vp > 0.f) || (vp < 0.f && vel > 0.f);
                }
            }
        }
        raw[f * T + t] = hit;
        if (p.foot_vels && t < T - 1) p.foot_vels[((size_t)b * (T - 1) + t) * 4 + f] = vel;
    }
    __syncthreads();
    if (fixed != raw) {
        // use_window: a contact frame rewrites frames f-3 .. f+3 with |y - y_f| < 0.006, later frames over earlier ones -- so frame k
        // takes the verdict of the LAST contact frame within its window, and keeps its own bit (0) when there is none
        for (int i = tid; i < 4 * T; i += 256) {
            const int k = i >> 2, f = i & 3;
            bool hit = false;
            if (k < n) {
                const float* yk = ref + 3 * p.fid[f] + 1;
                for (int g = min(k + kFeetWindow, n - 1); g >= max(k - kFeetWindow, 0); g--)
                    if (raw[f * T + g]) {
                        hit = fabsf(yk[(size_t)k * C] - yk[(size_t)g * C]) < kFeetWindowHeight;
                        break;
                    }
            }
            fixed[f * T + k] = hit;
        }
        __syncthreads();
    }
    if (p.contacts)
        for (int i = tid; i < 4 * T; i += 256) p.contacts[(size_t)b * 4 * T + i] = fixed[(i & 3) * T + (i >> 2)];

    if (!p.out) return;                                       // contacts alone were asked for

    // ---- the clip itself: every frame is copied, frames from len on stay as they are
    if (out != in) {
        for (size_t i = tid; i < clip; i += 256) out[i] = in[i];
        feet_sync();
    }
    double* ws = p.ws ? p.ws + (size_t)b * (size_t)(T - 1) * C : nullptr;
    if (p.filter_before) {
        feet_butterworth(out, ws, n, C, p.kb[0], p.kb[1], p.kb[2], p.kb[3], p.kb[4]);
        feet_sync();
    }

    // ---- floor
    float lo = INFINITY;
    for (int i = tid; i < n * J; i += 256) lo = fminf(lo, out[(size_t)i * 3 + 1]);
    for (int o = 32; o > 0; o >>= 1) lo = fminf(lo, __shfl_xor(lo, o, 64));
    if ((tid & 63) == 0) wave_min[tid >> 6] = lo;
    __syncthreads();
    lo = fminf(fminf(wave_min[0], wave_min[1]), fminf(wave_min[2], wave_min[3]));
    for (int i = tid; i < n * J; i += 256) out[(size_t)i * 3 + 1] -= lo;
    feet_sync();

    // ---- runs: the mean of each maximal contact run, written to every frame of the run
    for (int i = tid; i < 4 * n; i += 256) {
        const int s = i >> 2, f = i & 3;
        const unsigned char* fx = fixed + f * T;
        if (!fx[s] || (s > 0 && fx[s - 1])) continue;
        float* q = out + 3 * p.fid[f];
        float ax = q[(size_t)s * C], ay = q[(size_t)s * C + 1], az = q[(size_t)s * C + 2];
        int t = s;
        while (t + 1 < n && fx[t + 1]) {
            t++;
            ax += q[(size_t)t * C];
            ay += q[(size_t)t * C + 1];
            az += q[(size_t)t * C + 2];
        }
        const float cnt = (float)(t - s + 1);
        ax /= cnt;
        ay /= cnt;
        az /= cnt;
        if (p.force_on_floor) ay = 0.f;
        for (int j = s; j <= t; j++) {
            q[(size_t)j * C] = ax;
            q[(size_t)j * C + 1] = ay;
            q[(size_t)j * C + 2] = az;
        }
    }
    feet_sync();

    // ---- blend: reads the frame itself and contact frames, writes the frame itself
    const int L = p.interp_length;
    for (int i = tid; i < 4 * n; i += 256) {
        const int s = i >> 2, f = i & 3;
        const unsigned char* fx = fixed + f * T;
        if (fx[s]) continue;
        int l = -1, r = -1;
        for (int k = 0; k < L && s - k - 1 >= 0; k++)
            if (fx[s - k - 1]) { l = s - k - 1; break; }
        for (int k = 0; k < L && s + k + 1 < n; k++)
            if (fx[s + k + 1]) { r = s + k + 1; break; }
        if (l < 0 && r < 0) continue;
        float* q = out + 3 * p.fid[f];
        const double al = l >= 0 ? feet_alpha(1.0 * (s - l + 1) / (L + 1)) : 0.0;
        const double ar = r >= 0 ? feet_alpha(1.0 * (r - s + 1) / (L + 1)) : 0.0;
        const double am = l >= 0 && r >= 0 ? feet_alpha(1.0 * (s - l + 1) / (r - l + 1)) : 0.0;
        for (int c = 0; c < 3; c++) {
            const float v = q[(size_t)s * C + c];
            float res;
            if (l >= 0 && r >= 0) {
                const float litp = feet_lerp(al, v, q[(size_t)l * C + c]);
                const float ritp = feet_lerp(ar, v, q[(size_t)r * C + c]);
                res = feet_lerp(am, ritp, litp);
            } else if (l >= 0) {
                res = feet_lerp(al, v, q[(size_t)l * C + c]);
            } else {
                res = feet_lerp(ar, v, q[(size_t)r * C + c]);
            }
            q[(size_t)s * C + c] = res;
        }
    }
    if (p.filter_after) {
        feet_sync();
        feet_butterworth(out, ws, n, C, p.ka[0], p.ka[1], p.ka[2], p.ka[3], p.ka[4]);
    }
}

}  // namespace mst
