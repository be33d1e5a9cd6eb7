// Clips to video frames on the GPU: the scene of the reference's `explicit_plot_3d_motion` (data_loaders/humanml/utils/plot_script.py:
// 168-311) -- the stick figure's first five kinematic chains over the ground quad, re-centred on the root frame by frame, with the root
// or joint traces the inpainting mask names -- drawn by rules of our own (include/mst_engine.h states them in full), not by matplotlib.
//
//   k_render_bounds   `MINS` / `MAXS` (:221-225) of scale * joints over a clip's live frames, both skeletons: one workgroup a clip.
//   k_render_frames   `update(index)` (:257-305): one workgroup per (clip, frame, 32 x 32 pixel tile), four pixels of a row a lane.
//
// A layer is the quad or one polyline (a chain, a trace).  A polyline's points are projected into LDS, at most kRenderChunk at a time
// (a trace at frame t has up to t + 1 points and clips go to 4096 frames; consecutive chunks share one point, so no segment is lost).
// Each wave then compacts the segments of its own 64-groups that can reach the tile into its own list with one ballot a group -- no
// atomics and no prefix across waves -- and every pixel takes the minimum squared distance over the four lists.  A segment is dropped
// only when its bounding box misses the tile's pixel centres by the layer's reach w/2 + 0.5 plus a margin far above the arithmetic's
// error, so its coverage at every pixel of the tile is exactly 0 and the minimum over the survivors gives the same bits as the minimum
// over all: the cull changes no bit.  The minimum is order-free and sqrt is monotone, so one square root a layer serves.
//
// No atomics; every store is an ordinary vector store.  A workgroup reads its own clip's live frames and the clip's bounds, nothing
// else: a clip's frames are the same bits alone, anywhere in a batch, on any stream, for any frame sub-range, whatever other clips or
// the frames behind its length hold.  Frames at and behind a clip's length are exact zeros.
//
// Arithmetic: float32, no contraction into fused multiply-adds, division and square root correctly rounded: operation by operation
// what tests/render_fixture.py states in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mst {

constexpr int kRenderMaxFrames = 4096;       // frames of a clip: a trace's points
constexpr int kRenderMaxJoints = 64;
constexpr int kRenderChains = 5;             // chains drawn: the reference's zip with a five-colour palette stops there
constexpr int kRenderMaxChains = 16;         // chains taken and checked
constexpr int kRenderMaxChainPoints = 128;   // over the chains drawn, one skeleton
constexpr int kRenderMaxTraces = 8;
constexpr int kRenderMinSide = 16, kRenderMaxSide = 1024;
constexpr int kRenderTile = 32;              // pixels a side: 256 lanes x 4 pixels of a row
constexpr int kRenderThreads = 256;
constexpr int kRenderChunk = 512;            // polyline points in LDS at a time: 4 KiB of coordinates, 1 KiB of lists
constexpr int kRenderList = kRenderChunk / 4;        // a wave's own survivors: its 64-groups hold a quarter of a chunk's segments
constexpr int kRenderPalettes = 4;           // blue, orange, purple, upper_body

// the reference's hex values (:226-230), row = palette, column = chain
__constant__ unsigned char kRenderPalette[kRenderPalettes][kRenderChains][3] = {
    {{0x4D, 0x84, 0xAA}, {0x5B, 0x99, 0x65}, {0x61, 0xCE, 0xB9}, {0x34, 0xC1, 0xE2}, {0x80, 0xB7, 0x9A}},
    {{0xDD, 0x5A, 0x37}, {0xD6, 0x9E, 0x00}, {0xB7, 0x5A, 0x39}, {0xFF, 0x6D, 0x00}, {0xDD, 0xB5, 0x0E}},
    {{0x6B, 0x31, 0xDB}, {0xAD, 0x40, 0xA8}, {0xAF, 0x2B, 0x79}, {0x9B, 0x00, 0xFF}, {0xD8, 0x36, 0xC1}},
    {{0x4D, 0x84, 0xAA}, {0x5B, 0x99, 0x65}, {0xB7, 0x5A, 0x39}, {0xFF, 0x6D, 0x00}, {0xDD, 0xB5, 0x0E}}};

struct RenderArgs {
    const float* joints;                     // element (b, t, j, c) at b * sB + t * sT + j * sJ + c * sC
    const float* joints2;                    // the second skeleton, same strides, or null
    long long sB, sT, sJ, sC;
    const int* lengths;                      // [B] or null
    const float* bounds;                     // [B][8]: MINS xyz, MAXS xyz, two zeros (k_render_bounds)
    int B, T, J;
    float scale;
    int n_chains;                            // chains drawn, <= kRenderChains
    unsigned char chain_off[kRenderChains + 1];
    unsigned char chain_joint[kRenderMaxChainPoints];
    int n_traces;
    unsigned char trace_kind[kRenderMaxTraces];      // 0 root_horizontal, 1 root, 2 a joint
    unsigned char trace_joint[kRenderMaxTraces];
    const int* palette;                      // [B][T] or null (orange)
    float M[12];                             // rows x, y and w of the projective matrix
    float A[6];                              // pixels = A (x / w, y / w, 1)
    int W, H;
    float reach_chain, reach_trace;          // w / 2 + 0.5 in pixels
    const unsigned char* overlay;            // [overlay_batch][H][W] or null
    int overlay_batch;
    int t0, frames_out;
    unsigned char* out;                      // [B][frames_out][H][W][3]
    float* outf;                             // the same before quantisation, or null
};

__device__ __forceinline__ int render_len(const RenderArgs& p, int b) {
    const int len = p.lengths ? p.lengths[b] : p.T;
    return min(max(len, 1), p.T);            // no access leaves the clip, whatever the caller wrote
}

// ------------------------------------------------------------------------------------------ MINS / MAXS
// the workgroup's minimum and maximum of three coordinates -> out[8]: MINS xyz, MAXS xyz, two zeros (shared with mst_mesh.h)
__device__ __forceinline__ void render_bounds_reduce(float* mn, float* mx, float (*s_red)[6], float* __restrict__ out) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        for (int o = 32; o > 0; o >>= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], o));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o));
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            s_red[tid >> 6][c] = mn[c];
            s_red[tid >> 6][3 + c] = mx[c];
        }
    }
    __syncthreads();
    if (tid < 8) {
        float v = 0.f;
        if (tid < 6) {
            v = s_red[0][tid];
            for (int w = 1; w < kRenderThreads / 64; w++) v = tid < 3 ? fminf(v, s_red[w][tid]) : fmaxf(v, s_red[w][tid]);
        }
        out[tid] = v;
    }
}

__global__ __launch_bounds__(kRenderThreads) void k_render_bounds(const RenderArgs p, float* __restrict__ bounds) {
#pragma clang fp contract(off)
    __shared__ float s_red[kRenderThreads / 64][6];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = render_len(p, b) * p.J, total = p.joints2 ? 2 * n : n;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < total; i += kRenderThreads) {
        const int r = i < n ? i : i - n, k = r / p.J, j = r - k * p.J;
        const float* s = (i < n ? p.joints : p.joints2) + (long long)b * p.sB + (long long)k * p.sT + (long long)j * p.sJ;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float v = p.scale * s[c * p.sC];
            mn[c] = fminf(mn[c], v);         // NaN is passed over, as numpy's fmin / fmax do
            mx[c] = fmaxf(mx[c], v);
        }
    }
    render_bounds_reduce(mn, mx, s_red, bounds + (size_t)b * 8);
}

// ------------------------------------------------------------------------------------------ frames
// (x, y, z) -> pixels; NaN for a point that is not drawn: a non-finite coordinate, a projective w that is not positive and finite
__device__ __forceinline__ void render_project(const RenderArgs& p, float x, float y, float z, float& px, float& py) {
#pragma clang fp contract(off)
    const float X = ((p.M[0] * x + p.M[1] * y) + p.M[2] * z) + p.M[3];
    const float Y = ((p.M[4] * x + p.M[5] * y) + p.M[6] * z) + p.M[7];
    const float Wc = ((p.M[8] * x + p.M[9] * y) + p.M[10] * z) + p.M[11];
    const float xn = X / Wc, yn = Y / Wc;
    const float qx = (p.A[0] * xn + p.A[1] * yn) + p.A[2];
    const float qy = (p.A[3] * xn + p.A[4] * yn) + p.A[5];
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && isfinite(Wc) && Wc > 0.f && isfinite(qx) && isfinite(qy);
    px = ok ? qx : NAN;
    py = ok ? qy : NAN;
}

// joint j of frame k of a skeleton, as frame t sees it: W[k, j] - (traj[t].x, 0, traj[t].z), W = scale * joints with y -= MINS.y
__device__ __forceinline__ void render_point(const RenderArgs& p, const float* clip, int k, int j, float tx, float miny, float tz,
                                             bool flat, float& px, float& py) {
#pragma clang fp contract(off)
    const float* s = clip + (long long)k * p.sT + (long long)j * p.sJ;
    const float x = p.scale * s[0] - tx;
    const float y = flat ? 0.f : p.scale * s[p.sC] - miny;
    const float z = p.scale * s[2 * p.sC] - tz;
    render_project(p, x, y, z, px, py);
}

struct RenderTile {
    float x0, x1, y0, y1;                    // the tile's pixel centres
};

// Each wave compacts the segments of its own 64-groups that can reach the tile into its own list.  A segment with an end that is
// not drawn (NaN) is skipped here, which is where the rule "a segment with a non-finite end is skipped" is carried out.
__device__ __forceinline__ void render_cull(const float* s_px, const float* s_py, int npts, float reach, const RenderTile& tb,
                                            unsigned short* my_list, int* s_cnt) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int cnt = 0;                             // wave-uniform
    for (int s0 = wv * 64; s0 < npts - 1; s0 += kRenderThreads) {
        const int s = s0 + lane;
        bool keep = false;
        if (s < npts - 1) {
            const float ax = s_px[s], ay = s_py[s], bx = s_px[s + 1], by = s_py[s + 1];
            // the margin: 1 pixel and 1e-4 of the coordinates' size, against an error of a few float32 roundings of that size
            const float g = reach + (1.f + 1e-4f * (fabsf(ax) + fabsf(ay) + fabsf(bx) + fabsf(by)));
            const bool drawn = (ax == ax) && (bx == bx);                     // x and y are NaN together
            const bool out = fmaxf(ax, bx) < tb.x0 - g || fminf(ax, bx) > tb.x1 + g || fmaxf(ay, by) < tb.y0 - g || fminf(ay, by) > tb.y1 + g;
            keep = drawn && !out;
        }
        const unsigned long long m = __ballot(keep);
        if (keep) my_list[cnt + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)s;
        cnt += __popcll(m);
    }
    if (lane == 0) s_cnt[wv] = cnt;
}

// min over the surviving segments of the squared distance from each of the lane's four pixel centres
__device__ __forceinline__ void render_accumulate(const float* s_px, const float* s_py, const unsigned short (*s_list)[kRenderList],
                                                  const int* s_cnt, float cx0, float cy, float* d2) {
#pragma clang fp contract(off)
    for (int v = 0; v < kRenderThreads / 64; v++) {
        const int n = s_cnt[v];
        for (int i = 0; i < n; i++) {
            const int s = s_list[v][i];
            const float ax = s_px[s], ay = s_py[s];
            const float dx = s_px[s + 1] - ax, dy = s_py[s + 1] - ay;
            const float l2 = dx * dx + dy * dy;
            const float ey = cy - ay;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float ex = (cx0 + (float)q) - ax;
                float u = 0.f;               // a zero-length segment is a point
                if (l2 > 0.f) u = fminf(fmaxf((ex * dx + ey * dy) / l2, 0.f), 1.f);
                const float rx = ex - u * dx, ry = ey - u * dy;
                d2[q] = fminf(d2[q], rx * rx + ry * ry);
            }
        }
    }
}

__device__ __forceinline__ void render_blend(float* c, const float* col, float a) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = c[k] * (1.f - a) + col[k] * a;
}

__device__ __forceinline__ void render_line_layer(float (*c)[3], float* d2, float reach, const float* col) {
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float cov = fminf(fmaxf(reach - sqrtf(d2[q]), 0.f), 1.f);
        render_blend(c[q], col, cov);
        d2[q] = INFINITY;
    }
}

__global__ __launch_bounds__(kRenderThreads) void k_render_frames(const RenderArgs p) {
#pragma clang fp contract(off)
    __shared__ float s_px[kRenderChunk], s_py[kRenderChunk];
    __shared__ unsigned short s_list[kRenderThreads / 64][kRenderList];
    __shared__ int s_cnt[kRenderThreads / 64];
    __shared__ float s_quad[8];
    const int tid = threadIdx.x, wv = tid >> 6;
    const int tiles_x = (p.W + kRenderTile - 1) / kRenderTile;
    const int tx0 = ((int)blockIdx.x % tiles_x) * kRenderTile, ty0 = ((int)blockIdx.x / tiles_x) * kRenderTile;
    const int fi = blockIdx.y, t = p.t0 + fi, b = blockIdx.z;
    const int col0 = tx0 + (tid & 7) * 4, row = ty0 + (tid >> 3);
    const bool live = t < render_len(p, b);                                  // uniform over the workgroup
    float c[4][3];
#pragma unroll
    for (int q = 0; q < 4; q++) c[q][0] = c[q][1] = c[q][2] = live ? 1.f : 0.f;

    if (live) {
        // pixel (row, col) has its centre at (col + 0.5, H - row - 0.5): y up, as matplotlib's pixel frame
        const float cx0 = (float)col0 + 0.5f, cy = (float)(p.H - row) - 0.5f;
        RenderTile tb;
        tb.x0 = (float)tx0 + 0.5f;
        tb.x1 = (float)min(tx0 + kRenderTile, p.W) - 0.5f;
        tb.y0 = (float)(p.H - min(ty0 + kRenderTile, p.H)) + 0.5f;
        tb.y1 = (float)(p.H - ty0) - 0.5f;
        const float* bd = p.bounds + (size_t)b * 8;
        const float minx = bd[0], miny = bd[1], minz = bd[2], maxx = bd[3], maxz = bd[5];
        const float* clip = p.joints + (long long)b * p.sB;
        const float* clip2 = p.joints2 ? p.joints2 + (long long)b * p.sB : nullptr;
        const float* root = clip + (long long)t * p.sT;
        const float tx = p.scale * root[0], tz = p.scale * root[2 * p.sC];  // traj[t]
        int pal = p.palette ? p.palette[(size_t)b * p.T + t] : 1;
        pal = min(max(pal, 0), kRenderPalettes - 1);
        const int P = p.chain_off[p.n_chains];                               // chain points of one skeleton

        // the quad's corners in the reference's order, and every chain point of the frame
        if (tid < 4) {
            const float qx = (tid < 2 ? minx : maxx) - tx, qz = (tid == 0 || tid == 3 ? minz : maxz) - tz;
            render_project(p, qx, 0.f, qz, s_quad[2 * tid], s_quad[2 * tid + 1]);
        }
        for (int i = tid; i < (clip2 ? 2 * P : P); i += kRenderThreads) {
            const int e = i < P ? i : i - P;
            render_point(p, i < P ? clip : clip2, t, p.chain_joint[e], tx, miny, tz, false, s_px[i], s_py[i]);
        }
        __syncthreads();

        // ---- the ground quad: 0.5 grey at alpha 0.5, coverage from the signed distance to the nearest edge
        {
            float qx[4], qy[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                qx[k] = s_quad[2 * k];
                qy[k] = s_quad[2 * k + 1];
            }
            float area2 = 0.f;               // twice the signed area
#pragma unroll
            for (int k = 0; k < 4; k++) area2 = area2 + (qx[k] * qy[(k + 1) & 3] - qx[(k + 1) & 3] * qy[k]);
            const float area = 0.5f * area2;
            if (fabsf(area) >= 1e-12f) {     // false for NaN: a corner that is not drawn draws no quad
                const float sgn = area > 0.f ? 1.f : -1.f;
                float dmin[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float ex = qx[(k + 1) & 3] - qx[k], ey = qy[(k + 1) & 3] - qy[k];
                    const float el = sqrtf(ex * ex + ey * ey);
                    if (el > 0.f) {          // an edge of no length bounds nothing
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const float fx = (cx0 + (float)q) - qx[k], fy = cy - qy[k];
                            dmin[q] = fminf(dmin[q], sgn * ((ex * fy - ey * fx) / el));
                        }
                    }
                }
                const float grey[3] = {0.5f, 0.5f, 0.5f};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float cov = dmin[q] < INFINITY ? fminf(fmaxf(0.5f + dmin[q], 0.f), 1.f) : 0.f;
                    render_blend(c[q], grey, 0.5f * cov);
                }
            }
        }

        float d2[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
        // ---- chains in order, the second skeleton's right after the first's same chain
        for (int ch = 0; ch < p.n_chains; ch++) {
            const int o = p.chain_off[ch], n = p.chain_off[ch + 1] - o;
            float col[3];
#pragma unroll
            for (int k = 0; k < 3; k++) col[k] = (float)kRenderPalette[pal][ch][k] / 255.f;
            for (int sk = 0; sk < (clip2 ? 2 : 1); sk++) {
                if (n < 2) continue;
                const float* bx = s_px + o + sk * P;
                const float* by = s_py + o + sk * P;
                __syncthreads();             // the lists' readers of the layer before
                render_cull(bx, by, n, p.reach_chain, tb, s_list[wv], s_cnt);
                __syncthreads();
                render_accumulate(bx, by, s_list, s_cnt, cx0, cy, d2);
                render_line_layer(c, d2, p.reach_chain, col);
            }
        }

        // ---- traces in order, each in the frame's palette colour 0, a chunk of points at a time
        float tcol[3];
#pragma unroll
        for (int k = 0; k < 3; k++) tcol[k] = (float)kRenderPalette[pal][0][k] / 255.f;
        for (int tr = 0; tr < p.n_traces; tr++) {
            const int kind = p.trace_kind[tr], j = kind == 2 ? p.trace_joint[tr] : 0;
            const int n = kind == 2 ? t + 1 : t;                             // root traces stop before the frame, a joint's includes it
            if (n < 2) continue;             // fewer than 2 points draw nothing
            for (int c0 = 0; c0 < n - 1; c0 += kRenderChunk - 1) {
                const int m = min(kRenderChunk, n - c0);
                __syncthreads();             // the points' and lists' readers of the chunk or layer before
                for (int i = tid; i < m; i += kRenderThreads) render_point(p, clip, c0 + i, j, tx, miny, tz, kind == 0, s_px[i], s_py[i]);
                __syncthreads();
                render_cull(s_px, s_py, m, p.reach_trace, tb, s_list[wv], s_cnt);
                __syncthreads();
                render_accumulate(s_px, s_py, s_list, s_cnt, cx0, cy, d2);
            }
            render_line_layer(c, d2, p.reach_trace, tcol);
        }

        // ---- the overlay: coverage in black
        if (p.overlay && row < p.H) {
            const unsigned char* ov = p.overlay + ((size_t)(p.overlay_batch == 1 ? 0 : b) * p.H + row) * p.W;
            const float black[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (col0 + q < p.W) render_blend(c[q], black, (float)ov[col0 + q] / 255.f);
            }
        }
    }

    if (row >= p.H || col0 >= p.W) return;
    const size_t pix = (((size_t)b * p.frames_out + fi) * p.H + row) * p.W + col0;
    unsigned char u[12];
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int k = 0; k < 3; k++) u[3 * q + k] = (unsigned char)(int)floorf(255.f * c[q][k] + 0.5f);
    }
    if ((p.W & 3) == 0 && ((uintptr_t)p.out & 3) == 0) {
        // a row's bytes and col0 * 3 are multiples of 4 and the four pixels lie inside the row: three packed words
        uint32_t* o = reinterpret_cast<uint32_t*>(p.out + pix * 3);
#pragma unroll
        for (int k = 0; k < 3; k++)
            o[k] = (uint32_t)u[4 * k] | ((uint32_t)u[4 * k + 1] << 8) | ((uint32_t)u[4 * k + 2] << 16) | ((uint32_t)u[4 * k + 3] << 24);
    } else {
        const int nq = min(4, p.W - col0);
        for (int e = 0; e < 3 * nq; e++) p.out[pix * 3 + e] = u[e];
    }
    if (p.outf) {
        const int nq = min(4, p.W - col0);
        for (int q = 0; q < nq; q++) {
#pragma unroll
            for (int k = 0; k < 3; k++) p.outf[(pix + q) * 3 + k] = c[q][k];
        }
    }
}

}  // namespace mst
