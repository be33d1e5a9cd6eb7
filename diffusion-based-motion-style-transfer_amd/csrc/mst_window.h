// Overlapping windows of long clips (mst_window_plan): the glue that lets the sampler, whose clips are at most max_frames long, follow
// the stages around it to 4096 frames.  A long clip [C,F,1,L] is cut into windows [N,F,1,W] of the model's own length (unfold), all
// windows of all clips are sampled as one batch, and after every diffusion step the frames that two or more windows share are replaced,
// in all of them, by one weighted mean (stitch; MultiDiffusion / DoubleTake-style synchronisation).  The last stitch of a loop also
// writes the long clip (fold).
//
// The feature rows are frame-local (the root enters as velocities, everything else is relative to the root), so rows [s, s + W) of a
// long clip ARE the rows of the sub-clip: no value is re-expressed on the way in or out.
//
// Covering windows.  A clip's window starts are strictly ascending and every window is W long, so the windows that cover long frame f
// are a contiguous run of the clip's windows; the host (mst_window_plan_create) writes that run per (clip, long frame) as
// {first window, count}, count 0 from the clip's length on.  The kernels never search.
//
// k_window_stitch: one thread owns one (clip, feature, long frame) and is the only one that reads or writes that element of any
// window, so there are no atomics and no ordering between threads.  With K the covering windows in ascending order:
//   |K| == 1                    the element is not touched;
//   all of K hold the same bits they keep them (an inpainted row stays bit-exact: every window blends the same content value);
//   otherwise                   v = (sum_K h x) / (sum_K h), h(i) = min(i + 1, W - i) at the window's local frame i, every product and sum
//                               rounded to fp32 on its own in ascending window order (contraction is off: the NumPy statement in
//                               tests/window_fixture.py rounds the same way), and v is stored into every window of K.
// Lanes walk long frames, so a wavefront reads and writes 64 consecutive floats of each covering window and of the long row.  Window
// starts are arbitrary: a 16-byte access along frames would be legal only where start, W and L are all multiples of 4, which the last
// window of a clip (start = len - W) almost never is; the kernels are dword-per-lane at every shape instead of carrying two paths.
//
// k_window_noise: the noise of a stochastic step (ancestral, or DDIM at eta != 0) in LONG-clip coordinates.  The step kernels' own draw
// is keyed by (frame quad, feature, batch clip, step) of the WINDOW, so two windows would draw different numbers for a long frame they
// share and the stitch's mean would shrink the noise variance there.  Here entry j of the buffer is unfold(Z_j), Z_j [C,F,1,L] =
// mst_philox_normal(C, F, L, seed, step0 + j): element (c, f, l) is component l & 3 of philox_normal4(l >> 2, f, c, step0 + j, seed),
// the code the in-kernel draw shares.  Every window that covers a long frame receives the same bits for it, x_{t-1} stays linear in
// (x_t, x0-hat, noise), and the stitch stays the exact bookkeeping it is for eta == 0.  One thread owns one long quad of one step: it
// draws once and scatters the four normals to the covering windows through the cover table, a dword at a time.
#pragma once
#include <hip/hip_runtime.h>
#include "mst_common.h"

namespace mst {

constexpr int kWinMaxFrames = 4096;          // longest long clip: what the stages around the sampler take (mst_recover_from_ric, mst_remove_fs, mst_fit_joints)
constexpr int kWinThreads = 256;

struct WinCover { int first, count; };       // windows first .. first + count - 1 cover this long frame

// long [C,F,1,L] -> windows [N,F,1,W]; window frames at or past the clip's length are 0.0
__global__ void __launch_bounds__(kWinThreads)
k_window_unfold(const float* __restrict__ lng, const int* __restrict__ clip_len, const int* __restrict__ win_clip,
                const int* __restrict__ win_start, int N, int F, int W, int L, float* __restrict__ win) {
    const size_t idx = (size_t)blockIdx.x * kWinThreads + threadIdx.x;
    if (idx >= (size_t)N * F * W) return;
    const int i = (int)(idx % W);
    const size_t row = idx / W;              // n * F + feat
    const int feat = (int)(row % F), n = (int)(row / F);
    const int c = win_clip[n], f = win_start[n] + i;
    win[idx] = f < clip_len[c] ? lng[((size_t)c * F + feat) * L + f] : 0.0f;
}

// windows [N,F,1,W] stitched in place; lng != nullptr: also the fold, long [C,F,1,L] (exactly 0.0 from the clip's length on)
__global__ void __launch_bounds__(kWinThreads)
k_window_stitch(float* __restrict__ win, const WinCover* __restrict__ cover, const int* __restrict__ win_start, int C, int F, int W, int L,
                float* __restrict__ lng) {
    const size_t idx = (size_t)blockIdx.x * kWinThreads + threadIdx.x;
    if (idx >= (size_t)C * F * L) return;
    const int f = (int)(idx % L);
    const size_t row = idx / L;              // c * F + feat
    const int feat = (int)(row % F), c = (int)(row / F);
    const WinCover k = cover[(size_t)c * L + f];
    if (k.count == 0) {
        if (lng) lng[idx] = 0.0f;
        return;
    }
    const size_t wrow = (size_t)F * W;       // elements per window
    float* const base = win + (size_t)k.first * wrow + (size_t)feat * W;
    const int i0 = f - win_start[k.first];
    const float x0 = base[i0];
    float v = x0;
    if (k.count > 1) {
        bool same = true;
        float num = 0.0f;
        int den = 0;
        for (int j = 0; j < k.count; j++) {
#pragma clang fp contract(off)      // h x and the sum round separately, as the NumPy statement's do (the compiler would fuse them otherwise)
            const int i = f - win_start[k.first + j];
            const float x = base[(size_t)j * wrow + i];
            const int h = min(i + 1, W - i);
            same = same && __float_as_uint(x) == __float_as_uint(x0);
            num = num + (float)h * x;
            den += h;
        }
        if (!same) {
            v = num / (float)den;           // (sum of h <= W^2 / 2: exact in fp32; the division is correctly rounded)
            for (int j = 0; j < k.count; j++) base[(size_t)j * wrow + (f - win_start[k.first + j])] = v;
        }
    }
    if (lng) lng[idx] = v;
}

// noise [nsteps,N,F,1,W] <- unfold of the long draws Z_j [C,F,1,L], j = 0 .. nsteps - 1; EVERY element is written (the buffer may be
// uninitialised): window frames at or past the clip's length get 0.0.  Such frames exist only in the single window, at start 0, of a clip
// shorter than W, and W may exceed L, so a row is walked in Q = ceil(max(L, W) / 4) quads: frames from L on have no long element and
// are padding.  A quad at or past the clip's length draws nothing.
__global__ void __launch_bounds__(kWinThreads)
k_window_noise(const WinCover* __restrict__ cover, const int* __restrict__ clip_len, const int* __restrict__ win_start, int C, int N, int F,
               int W, int L, int Q, int nsteps, unsigned long long seed, unsigned step0, float* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * kWinThreads + threadIdx.x;
    if (idx >= (size_t)nsteps * C * F * Q) return;
    const int q = (int)(idx % Q);
    size_t row = idx / Q;                    // (j * C + c) * F + feat
    const int feat = (int)(row % F);
    row /= F;
    const int c = (int)(row % C), j = (int)(row / C);
    const int len = clip_len[c];
    float* const step = out + (size_t)j * N * F * W;
    const WinCover* const cov = cover + (size_t)c * L;
    float n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (4 * q < len) philox_normal4((unsigned)q, (unsigned)feat, (unsigned)c, step0 + (unsigned)j, seed, n);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int l = 4 * q + k;
        if (l < len) {                       // (len <= L: the cover entry exists; its windows hold l at local frame l - start, in [0, W))
            const WinCover kc = cov[l];
            for (int w = 0; w < kc.count; w++)
                step[((size_t)(kc.first + w) * F + feat) * W + (l - win_start[kc.first + w])] = n[k];
        } else if (l < W && len < W) {       // padding of the clip's only window (frame 0 is always covered, by the clip's first window)
            step[((size_t)cov[0].first * F + feat) * W + l] = 0.0f;
        }
    }
}

}  // namespace mst
