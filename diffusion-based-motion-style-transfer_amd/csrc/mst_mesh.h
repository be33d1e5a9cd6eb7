// SMPL meshes to video frames on the GPU: the scene of the reference's visualize/render_final.py `render` (:79-89, :169-251) -- the
// posed body, one colour a frame, over a translucent background, seen by a perspective camera above and in front of the clip --
// drawn by a triangle rasteriser with a depth test and rules of our own (include/mst_engine.h states them in full), not by pyrender.
//
//   k_mesh_bounds     `MINS` / `MAXS` (:79-80) of the vertices over a clip's live frames: one workgroup a clip.
//   k_mesh_vertices   one lane per (clip, output frame, vertex): vertex normal, shade, projection -> (px, py, depth, 1/w, shade) in the
//                     caller's workspace, and every workgroup's pixel bounding box of the vertices it drew.
//   k_mesh_frames     one workgroup per (clip, output frame, 32 x 32 pixel tile), four pixels of a row a lane, samples^2 points a pixel.
//
// A tile that the frame's bounding box misses writes background and leaves.  Otherwise the faces are streamed kMeshChunk at a time:
// each wave compacts the faces of its own 64-groups whose pixel bounding box can reach the tile into its own LDS list with one ballot
// a group (the scheme of mst_render.h: no atomics, no prefix across waves), their three vertices sorted by index beside them, and
// every sample point takes the minimum of (depth, face index) over the four lists.  A sample is covered only inside the face's own
// bounding box, which float32 comparisons decide exactly, so a face is dropped only where it covers no sample of the tile and the
// minimum over the survivors is the minimum over all: the cull changes no bit.  The margin of one pixel on top is far above any error
// (there is none to cover).  The winner's shade is formed once, after the last chunk, from the same edge functions.
//
// No atomics; every store is an ordinary vector store.  A workgroup reads its own clip's live frames and nothing else: a clip's frames
// are the same bits alone, anywhere in a batch, on any stream, for any frame sub-range, whatever other clips or the frames behind its
// length hold.  Frames at and behind a clip's length are exact zeros (the face-index image: -1).  There is no near-plane clipping.
//
// Arithmetic: float32, no contraction into fused multiply-adds, division and square root correctly rounded: operation by operation
// what tests/mesh_fixture.py states in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mst_render.h"

namespace mst {

constexpr int kMeshMaxFrames = 65535;        // frames of a clip: a grid dimension
constexpr int kMeshMaxVertices = 32768;
constexpr int kMeshMaxFaces = 65536;         // a face index fits 16 bits of a list entry
constexpr int kMeshMinSide = 16, kMeshMaxSide = 1024;
constexpr int kMeshMaxSamples = 4;           // sample points a side of a pixel
constexpr int kMeshTile = 32;                // pixels a side: 256 lanes x 4 pixels of a row
constexpr int kMeshThreads = 256;
constexpr int kMeshChunk = 1024;             // faces culled at a time: their survivors' 40 KiB of vertices and ids in LDS
constexpr int kMeshList = kMeshChunk / 4;    // a wave's own survivors: its 64-groups hold a quarter of a chunk's faces
constexpr int kMeshVertexFloats = 5;         // px, py | depth, 1 / w, shade

struct MeshArgs {
    const float* verts;                      // element (b, t, v, c) at b * sB + t * sT + v * sV + c * sC
    long long sB, sT, sV, sC;
    const int* lengths;                      // [B] or null
    int B, T, V, F;
    const int* faces;                        // [F][3]
    const int* adj_off;                      // [V + 1]: vertex -> its faces, ascending
    const int* adj_face;                     // [3 F]
    const float* proj;                       // [proj_batch][16]: rows x, y, depth, w
    int proj_batch;                          // 1 or B
    float A[6];                              // pixels = A (x / w, y / w, 1)
    int W, H;
    float light[3], ambient;
    const float* colors;                     // [B][T][4] or null (the reference's ramp)
    float bg[4];
    int t0, frames_out;
    int ids_sample;                          // the sub-sample the face-index image reports
    float* ws;                               // [B][frames_out][5 V + 4 ceil(V / 256)]
    unsigned char* out;                      // [B][frames_out][H][W][4]
    float* outf;                             // the same before quantisation, or null
    int* ids;                                // [B][frames_out][H][W], or null
};

__host__ __device__ __forceinline__ int mesh_blocks(int V) { return (V + kMeshThreads - 1) / kMeshThreads; }
__host__ __device__ __forceinline__ size_t mesh_frame_floats(int V) { return (size_t)kMeshVertexFloats * V + 4 * (size_t)mesh_blocks(V); }

__device__ __forceinline__ int mesh_len(const MeshArgs& p, int b) {
    const int len = p.lengths ? p.lengths[b] : p.T;
    return min(max(len, 1), p.T);            // no access leaves the clip, whatever the caller wrote
}

// ------------------------------------------------------------------------------------------ MINS / MAXS
__global__ __launch_bounds__(kMeshThreads) void k_mesh_bounds(const MeshArgs p, float* __restrict__ bounds) {
#pragma clang fp contract(off)
    __shared__ float s_red[kMeshThreads / 64][6];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long total = (long long)mesh_len(p, b) * p.V;
    const float* clip = p.verts + (long long)b * p.sB;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = tid; i < total; i += kMeshThreads) {
        const long long k = i / p.V, v = i - k * p.V;
        const float* s = clip + k * p.sT + v * p.sV;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float x = s[c * p.sC];
            mn[c] = fminf(mn[c], x);         // NaN is passed over, as numpy's fmin / fmax do
            mx[c] = fmaxf(mx[c], x);
        }
    }
    render_bounds_reduce(mn, mx, s_red, bounds + (size_t)b * 8);
}

// ------------------------------------------------------------------------------------------ vertices
__global__ __launch_bounds__(kMeshThreads) void k_mesh_vertices(const MeshArgs p) {
#pragma clang fp contract(off)
    __shared__ float s_red[kMeshThreads / 64][4];
    const int tid = threadIdx.x, v = blockIdx.x * kMeshThreads + tid;
    const int fi = blockIdx.y, t = p.t0 + fi, b = blockIdx.z;
    if (t >= mesh_len(p, b)) return;         // uniform over the workgroup; a dead frame's workspace is never read
    float* fr = p.ws + ((size_t)b * p.frames_out + fi) * mesh_frame_floats(p.V);
    float px = NAN, py = NAN;
    if (v < p.V) {
        const float* frame = p.verts + (long long)b * p.sB + (long long)t * p.sT;
        const float* s = frame + (long long)v * p.sV;
        const float x = s[0], y = s[p.sC], z = s[2 * p.sC];
        // the normal: the sum of cross(p1 - p0, p2 - p0) over the vertex's faces in ascending face order, normalised
        float nx = 0.f, ny = 0.f, nz = 0.f;
        const int k1 = p.adj_off[v + 1];
        for (int k = p.adj_off[v]; k < k1; k++) {
            const int* f = p.faces + 3 * (size_t)p.adj_face[k];
            const float* a = frame + (long long)f[0] * p.sV;
            const float* c1 = frame + (long long)f[1] * p.sV;
            const float* c2 = frame + (long long)f[2] * p.sV;
            const float ax = a[0], ay = a[p.sC], az = a[2 * p.sC];
            const float ux = c1[0] - ax, uy = c1[p.sC] - ay, uz = c1[2 * p.sC] - az;
            const float wx = c2[0] - ax, wy = c2[p.sC] - ay, wz = c2[2 * p.sC] - az;
            nx = nx + (uy * wz - uz * wy);
            ny = ny + (uz * wx - ux * wz);
            nz = nz + (ux * wy - uy * wx);
        }
        const float l = sqrtf((nx * nx + ny * ny) + nz * nz);
        if (l > 0.f && l < INFINITY) {
            nx = nx / l;
            ny = ny / l;
            nz = nz / l;
        } else {
            nx = ny = nz = 0.f;              // a zero or non-finite sum
        }
        const float d = (nx * p.light[0] + ny * p.light[1]) + nz * p.light[2];
        const float shade = p.ambient + (1.f - p.ambient) * fmaxf(d, 0.f);
        // projection, as render_project, with the depth row and 1 / w kept
        const float* M = p.proj + (p.proj_batch == 1 ? 0 : (size_t)b * 16);
        const float X = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
        const float Y = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
        const float Z = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
        const float Wc = ((M[12] * x + M[13] * y) + M[14] * z) + M[15];
        const float xn = X / Wc, yn = Y / Wc, dep = Z / Wc, iw = 1.f / Wc;
        const float qx = (p.A[0] * xn + p.A[1] * yn) + p.A[2];
        const float qy = (p.A[3] * xn + p.A[4] * yn) + p.A[5];
        const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && isfinite(Wc) && Wc > 0.f && isfinite(qx) && isfinite(qy) &&
                        isfinite(dep) && isfinite(iw);
        px = ok ? qx : NAN;
        py = ok ? qy : NAN;
        fr[2 * v] = px;
        fr[2 * v + 1] = py;
        float* r = fr + 2 * (size_t)p.V + 3 * (size_t)v;
        r[0] = ok ? dep : NAN;
        r[1] = ok ? iw : NAN;
        r[2] = ok ? shade : NAN;
    }
    // this workgroup's pixel bounding box of the vertices it drew (NaN is passed over)
    float bb[4] = {px, py, px, py};
    for (int o = 32; o > 0; o >>= 1) {
        bb[0] = fminf(bb[0], __shfl_xor(bb[0], o));
        bb[1] = fminf(bb[1], __shfl_xor(bb[1], o));
        bb[2] = fmaxf(bb[2], __shfl_xor(bb[2], o));
        bb[3] = fmaxf(bb[3], __shfl_xor(bb[3], o));
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 4; c++) s_red[tid >> 6][c] = bb[c];
    }
    __syncthreads();
    if (tid < 4) {
        float r = s_red[0][tid];
        for (int w = 1; w < kMeshThreads / 64; w++) r = tid < 2 ? fminf(r, s_red[w][tid]) : fmaxf(r, s_red[w][tid]);
        // no vertex drawn: (+inf, +inf, -inf, -inf), which no tile meets
        if (!(r == r)) r = tid < 2 ? INFINITY : -INFINITY;
        fr[(size_t)kMeshVertexFloats * p.V + 4 * (size_t)blockIdx.x + tid] = r;
    }
}

// ------------------------------------------------------------------------------------------ frames
struct MeshFace {
    float x[3], y[3];                        // pixels of the vertices in ascending vertex index: L, M, H
    int v[3];
};

// face f of a frame's workspace with its vertices sorted by index -> true when it may be drawn: every vertex drawn, the doubled
// area (M - L) x (H - L) finite and not zero
__device__ __forceinline__ bool mesh_face(const MeshArgs& p, const float* fr, int f, MeshFace& o) {
#pragma clang fp contract(off)
    const int* idx = p.faces + 3 * (size_t)f;
    int a = idx[0], b = idx[1], c = idx[2], s;
    if (a > b) { s = a; a = b; b = s; }
    if (b > c) { s = b; b = c; c = s; }
    if (a > b) { s = a; a = b; b = s; }
    o.v[0] = a; o.v[1] = b; o.v[2] = c;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        o.x[k] = fr[2 * o.v[k]];
        o.y[k] = fr[2 * o.v[k] + 1];
    }
    const float area2 = (o.x[1] - o.x[0]) * (o.y[2] - o.y[0]) - (o.y[1] - o.y[0]) * (o.x[2] - o.x[0]);
    const bool drawn = (o.x[0] == o.x[0]) && (o.x[1] == o.x[1]) && (o.x[2] == o.x[2]);        // a vertex's values are NaN together
    return drawn && area2 != 0.f && fabsf(area2) < INFINITY;
}

// The three edge functions at (sx, sy), each formed from its edge's lower-index end so that two faces sharing an edge form the same
// number: wl belongs to vertex L (edge M -> H), wm to M (edge L -> H, negated), wh to H (edge L -> M).
// -> covered: inside the face's bounding box, all three >= 0 or all three <= 0, and their sum not zero.
__device__ __forceinline__ bool mesh_weights(const float* x, const float* y, float sx, float sy, float& wl, float& wm, float& wh, float& sum) {
#pragma clang fp contract(off)
    const float bx0 = fminf(fminf(x[0], x[1]), x[2]), bx1 = fmaxf(fmaxf(x[0], x[1]), x[2]);
    const float by0 = fminf(fminf(y[0], y[1]), y[2]), by1 = fmaxf(fmaxf(y[0], y[1]), y[2]);
    const float qlx = sx - x[0], qly = sy - y[0], qmx = sx - x[1], qmy = sy - y[1];
    wh = (x[1] - x[0]) * qly - (y[1] - y[0]) * qlx;
    wm = -((x[2] - x[0]) * qly - (y[2] - y[0]) * qlx);
    wl = (x[2] - x[1]) * qmy - (y[2] - y[1]) * qmx;
    sum = (wl + wm) + wh;
    const bool inbox = sx >= bx0 && sx <= bx1 && sy >= by0 && sy <= by1;
    const bool same = (wl >= 0.f && wm >= 0.f && wh >= 0.f) || (wl <= 0.f && wm <= 0.f && wh <= 0.f);
    return inbox && same && sum != 0.f;
}

template <int S>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_frames(const MeshArgs p) {
#pragma clang fp contract(off)
    constexpr int NS = S * S, NW = kMeshThreads / 64;
    __shared__ float s_f[NW][9][kMeshList];                  // a wave's survivors: x, y of L, M, H and their depths
    __shared__ int s_id[NW][kMeshList];
    __shared__ int s_cnt[NW];
    __shared__ float s_box[NW][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tiles_x = (p.W + kMeshTile - 1) / kMeshTile;
    const int tx0 = ((int)blockIdx.x % tiles_x) * kMeshTile, ty0 = ((int)blockIdx.x / tiles_x) * kMeshTile;
    const int fi = blockIdx.y, t = p.t0 + fi, b = blockIdx.z;
    const int col0 = tx0 + (tid & 7) * 4, row = ty0 + (tid >> 3);
    const bool live = t < mesh_len(p, b);                                    // uniform over the workgroup
    const float* fr = p.ws + ((size_t)b * p.frames_out + fi) * mesh_frame_floats(p.V);

    // sample (q, j, i) of the lane: pixel col0 + q, sub-sample row j, column i; y up, as in mst_render.h
    float sx[4][S], sy[S];
#pragma unroll
    for (int i = 0; i < S; i++) {
#pragma unroll
        for (int q = 0; q < 4; q++) sx[q][i] = (float)(col0 + q) + ((float)i + 0.5f) / (float)S;
        sy[i] = (float)(p.H - row) - ((float)i + 0.5f) / (float)S;
    }
    float bestd[4][NS];
    int bestf[4][NS];
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int k = 0; k < NS; k++) {
            bestd[q][k] = INFINITY;
            bestf[q][k] = -1;
        }
    }

    bool hit = false;
    if (live) {
        // the frame's bounding box: the minimum and maximum over k_mesh_vertices' workgroups
        const float* boxes = fr + (size_t)kMeshVertexFloats * p.V;
        float bb[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};
        for (int i = tid; i < mesh_blocks(p.V); i += kMeshThreads) {
            bb[0] = fminf(bb[0], boxes[4 * i]);
            bb[1] = fminf(bb[1], boxes[4 * i + 1]);
            bb[2] = fmaxf(bb[2], boxes[4 * i + 2]);
            bb[3] = fmaxf(bb[3], boxes[4 * i + 3]);
        }
        for (int o = 32; o > 0; o >>= 1) {
            bb[0] = fminf(bb[0], __shfl_xor(bb[0], o));
            bb[1] = fminf(bb[1], __shfl_xor(bb[1], o));
            bb[2] = fmaxf(bb[2], __shfl_xor(bb[2], o));
            bb[3] = fmaxf(bb[3], __shfl_xor(bb[3], o));
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 4; c++) s_box[wv][c] = bb[c];
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NW; w++) {
            bb[0] = fminf(bb[0], s_box[w][0]);
            bb[1] = fminf(bb[1], s_box[w][1]);
            bb[2] = fmaxf(bb[2], s_box[w][2]);
            bb[3] = fmaxf(bb[3], s_box[w][3]);
        }
        // every sample point of the tile lies inside (X0, X1) x (Y0, Y1); one pixel of margin on top
        const float g = 1.f;
        const float X0 = (float)tx0 - g, X1 = (float)min(tx0 + kMeshTile, p.W) + g;
        const float Y0 = (float)(p.H - min(ty0 + kMeshTile, p.H)) - g, Y1 = (float)(p.H - ty0) + g;
        hit = !(bb[2] < X0 || bb[0] > X1 || bb[3] < Y0 || bb[1] > Y1);       // uniform over the workgroup

        if (hit) {
            const float* rest = fr + 2 * (size_t)p.V;
            const float lx0 = (float)col0, lx1 = (float)(col0 + 4), ly0 = (float)(p.H - row - 1), ly1 = (float)(p.H - row);
            for (int c0 = 0; c0 < p.F; c0 += kMeshChunk) {
                const int c1 = min(c0 + kMeshChunk, p.F);
                __syncthreads();             // the lists' readers of the chunk before
                int cnt = 0;                 // wave-uniform
                for (int f0 = c0 + wv * 64; f0 < c1; f0 += kMeshThreads) {
                    const int f = f0 + lane;
                    MeshFace m;
                    bool keep = false;
                    if (f < c1) {
                        keep = mesh_face(p, fr, f, m);
                        const float bx0 = fminf(fminf(m.x[0], m.x[1]), m.x[2]), bx1 = fmaxf(fmaxf(m.x[0], m.x[1]), m.x[2]);
                        const float by0 = fminf(fminf(m.y[0], m.y[1]), m.y[2]), by1 = fmaxf(fmaxf(m.y[0], m.y[1]), m.y[2]);
                        keep = keep && !(bx1 < X0 || bx0 > X1 || by1 < Y0 || by0 > Y1);
                    }
                    const unsigned long long mask = __ballot(keep);
                    if (keep) {
                        const int slot = cnt + __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
                        for (int k = 0; k < 3; k++) {
                            s_f[wv][2 * k][slot] = m.x[k];
                            s_f[wv][2 * k + 1][slot] = m.y[k];
                            s_f[wv][6 + k][slot] = rest[3 * (size_t)m.v[k]];
                        }
                        s_id[wv][slot] = f;
                    }
                    cnt += __popcll(mask);
                }
                if (lane == 0) s_cnt[wv] = cnt;
                __syncthreads();
                for (int w = 0; w < NW; w++) {
                    const int n = s_cnt[w];
                    for (int e = 0; e < n; e++) {
                        float x[3], y[3], z[3];
#pragma unroll
                        for (int k = 0; k < 3; k++) {
                            x[k] = s_f[w][2 * k][e];
                            y[k] = s_f[w][2 * k + 1][e];
                            z[k] = s_f[w][6 + k][e];
                        }
                        // the lane's own sample points all lie in [lx0, lx1] x [ly0, ly1]: outside the face's box none is covered
                        if (fmaxf(fmaxf(x[0], x[1]), x[2]) < lx0 || fminf(fminf(x[0], x[1]), x[2]) > lx1 ||
                            fmaxf(fmaxf(y[0], y[1]), y[2]) < ly0 || fminf(fminf(y[0], y[1]), y[2]) > ly1)
                            continue;
                        const int f = s_id[w][e];
#pragma unroll
                        for (int q = 0; q < 4; q++) {
#pragma unroll
                            for (int k = 0; k < NS; k++) {
                                float wl, wm, wh, sum;
                                if (mesh_weights(x, y, sx[q][k % S], sy[k / S], wl, wm, wh, sum)) {
                                    const float d = ((wl * z[0] + wm * z[1]) + wh * z[2]) / sum;
                                    if (d < bestd[q][k] || (d == bestd[q][k] && f < bestf[q][k])) {      // false for a NaN depth
                                        bestd[q][k] = d;
                                        bestf[q][k] = f;
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }

    if (row >= p.H || col0 >= p.W) return;
    // ---- the winners' shade, compositing over the background, the mean over the sub-samples
    float rgba[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        if (p.colors) {
            const float* c = p.colors + ((size_t)b * p.T + t) * 4;
#pragma unroll
            for (int k = 0; k < 4; k++) rgba[k] = c[k];
        } else {                             // the reference's ramp (:184), each channel clamped to 1
            rgba[0] = 1.f;
            rgba[1] = fminf((145.f + 0.8f * (float)t) / 255.f, 1.f);
            rgba[2] = fminf((33.f + 0.5f * (float)t) / 255.f, 1.f);
            rgba[3] = 0.9f;
        }
    }
    const float al = rgba[3], om = 1.f - al;
    const float cover_a = al + om * p.bg[3];
    float c[4][4];
    int idv[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        idv[q] = -1;
#pragma unroll
        for (int k = 0; k < NS; k++) {
            float s4[4];
            const int f = bestf[q][k];
            if (f >= 0) {
                MeshFace m;
                mesh_face(p, fr, f, m);
                float wl, wm, wh, sum;
                mesh_weights(m.x, m.y, sx[q][k % S], sy[k / S], wl, wm, wh, sum);
                const float* rest = fr + 2 * (size_t)p.V;
                const float al_ = wl * rest[3 * (size_t)m.v[0] + 1], am = wm * rest[3 * (size_t)m.v[1] + 1], ah = wh * rest[3 * (size_t)m.v[2] + 1];
                const float shade = ((al_ * rest[3 * (size_t)m.v[0] + 2] + am * rest[3 * (size_t)m.v[1] + 2]) + ah * rest[3 * (size_t)m.v[2] + 2]) /
                                    ((al_ + am) + ah);
#pragma unroll
                for (int ch = 0; ch < 3; ch++) s4[ch] = al * (rgba[ch] * shade) + om * p.bg[ch];
                s4[3] = cover_a;
            } else {
#pragma unroll
                for (int ch = 0; ch < 4; ch++) s4[ch] = p.bg[ch];
            }
#pragma unroll
            for (int ch = 0; ch < 4; ch++) c[q][ch] = k == 0 ? s4[ch] : c[q][ch] + s4[ch];
            if (k == p.ids_sample) idv[q] = f;
        }
#pragma unroll
        for (int ch = 0; ch < 4; ch++) c[q][ch] = live ? fminf(fmaxf(c[q][ch] / (float)NS, 0.f), 1.f) : 0.f;
    }

    const size_t pix = (((size_t)b * p.frames_out + fi) * p.H + row) * p.W + col0;
    const int nq = min(4, p.W - col0);
    uint32_t u[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        u[q] = 0;
#pragma unroll
        for (int ch = 0; ch < 4; ch++) u[q] |= (uint32_t)(int)floorf(255.f * c[q][ch] + 0.5f) << (8 * ch);
    }
    uint32_t* o = reinterpret_cast<uint32_t*>(p.out) + pix;                  // the ABI takes a 4-byte aligned image
    if ((p.W & 3) == 0 && ((uintptr_t)p.out & 15) == 0) {
        *reinterpret_cast<uint4*>(o) = make_uint4(u[0], u[1], u[2], u[3]);   // col0 and a row's pixels are multiples of 4
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (q < nq) o[q] = u[q];
    }
    if (p.outf) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (q < nq) *reinterpret_cast<float4*>(p.outf + (pix + q) * 4) = make_float4(c[q][0], c[q][1], c[q][2], c[q][3]);
        }
    }
    if (p.ids) {
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (q < nq) p.ids[pix + q] = idv[q];
    }
}

}  // namespace mst
