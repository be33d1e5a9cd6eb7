// Motion files on the GPU: what the reference does clip by clip in Python loops around its BVH reader and writer.
//
//   k_bvh_decode          `read_bvh` after the text is parsed (data_loaders/humanml/common/bvh_utils.py:222-295): Euler degrees ->
//                         radians -> `eul2q` (utils/rotation.py:344-361 over `angle_axis_to_quat`, :327-341), the sign continuity of
//                         `remove_quat_discontinuities` (:666-683), the `[i::k]` sub-sampling, and `quat_fk` (:646-663).
//   k_quats_to_channels   the numbers `save_bvh` formats (bvh_utils.py:588-612): `qnorm`, `q2eul` of order[::-1] (rotation.py:364-382),
//                         degrees, in the writer's joint permutation and channel order.
//   k_retarget            `uniform_skeleton_basic` (data_loaders/humanml/scripts/motion_process.py:12-35): the source offsets of frame 0
//                         (`Skeleton.get_offsets_joints`, common/skeleton.py:43-51), the leg ratio, the chain IK of
//                         `inverse_kinematics_np` (:55-105, smooth_forward=False) and `forward_kinematics_np` (:130-151).
//
// No atomics; every store is an ordinary vector store.
//
// k_bvh_decode: one workgroup per clip, lanes walk the frames of the clip's own length in rounds of the workgroup's width.
//   round, first half   per file joint the raw local quaternion q(e0, axis0) (x) (q(e1, axis1) (x) q(e2, axis2)) of frame t (sinf / cosf)
//                       and of frame t - 1 -- formed by the lane of frame t from the channels, the same instructions on the same operands
//                       as the lane of frame t - 1 uses -- and the flip bit dot(raw[t-1], raw[t]) < 0.  The sign of frame t is the parity of
//                       the flip bits of frames 1 .. t: a wave ballot gives the parity within the wave (kept by the lane as one bit a joint),
//                       the waves' totals go to LDS, the carry of all earlier rounds is one bit a joint in LDS.  A joint without rotation
//                       channels (an End Site) is the identity and never flips.
//   one barrier
//   round, second half  sign = lane bit ^ earlier waves' totals ^ carry; the lane of a frame that is written (t = phase + k * stride) reads
//                       its raw quaternions back from the workspace (same-thread read after write: no barrier), applies the sign, and runs
//                       quat_fk in file order, writing gr / gp of the whole file skeleton to the workspace and reading its own parent's
//                       entries back.  LDS therefore holds the scan alone and the joint cap does not depend on it.
// Stated deviation: for a dot product of exactly 0 the reference resets the sign to the raw quaternion's, the kernel keeps the running one.
// Outputs for the selected joints (or all of them): the local quaternion -- the file's own (signed, not normalised: `Anim.quats`) where the
// nearest selected ancestor is the file parent, qinv(gr[ancestor]) (x) gr[j] otherwise (gr[j] itself with no selected ancestor) -- and
// the global position; optionally the local position (`Anim.pos`) and the global quaternion.  Frames at or past a clip's length: exact zeros.
#pragma once
#include <hip/hip_runtime.h>

#include "mst_encode.h"

namespace mst {

// File joints (End Sites included): the skeleton's tables ride in the kernel arguments -- 28 bytes a joint, 2.7 KB at 96 of the 4 KB
// a launch may pass -- and the lane keeps one scan bit a joint in two 64-bit registers.  Skeletons with fingers (about 60 joints and a
// dozen End Sites) fit.
constexpr int kBvhMaxJoints = 96;
constexpr int kBvhMaxSel = kEncMaxJoints;    // what encode_joints takes
// Frames: nothing a frame needs is kept on chip, so the bound is time, not memory -- a clip is walked by one workgroup, 256 frames a round
// with one barrier each, 64 rounds at the cap (4 x the 4096 of mst_remove_fs_max_frames and mst_fit_joints_max_frames).  Longer files
// are read in pieces (start / end).
constexpr int kBvhMaxFrames = 16384;
constexpr int kBvhThreads = 256;
constexpr int kBvhWaves = kBvhThreads / 64;
constexpr int kBvhWs = 11;                   // workspace floats per frame and file joint: raw local quaternion, gr, gp

struct BvhArgs {
    const float* ch;                         // [B][T][C]
    const int* lengths;                      // [B] or null
    int B, T, C, Jf, nsel, stride, phase, Tout;
    float scale;
    int axis[3];                             // the file's rotation order, 0 / 1 / 2 = x / y / z
    short parent[kBvhMaxJoints];             // -1 for the root
    short rot_col[kBvhMaxJoints];            // first rotation column, -1: none
    short pos_col[kBvhMaxJoints];            // first position column, -1: the offset
    float off[kBvhMaxJoints][3];
    short sel[kBvhMaxSel];                   // file joint of output joint k
    short sel_anc[kBvhMaxSel];               // file joint of its nearest selected ancestor, -1: none
    short sel_direct[kBvhMaxSel];            // that ancestor is the file parent (or the joint is the file's root): the file's own local values
    float* ws;                               // [B][T][Jf][11]
    float* rot;                              // [B][Tout][J][4]
    float* pos;                              // [B][Tout][J][3]
    float* lpos;                             // [B][Tout][J][3] or null
    float* grot;                             // [B][Tout][J][4] or null
};

// eul2q: q(e0, axis0) (x) (q(e1, axis1) (x) q(e2, axis2)), degrees in
__device__ __forceinline__ void bvh_eul2q(const float* e, const int* axis, float* q) {
    float a[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float h = (e[k] * 0.017453292519943295f) / 2.0f;
        const float c = cosf(h), s = sinf(h);
        a[k][0] = c;
        a[k][1] = axis[k] == 0 ? s : 0.f;
        a[k][2] = axis[k] == 1 ? s : 0.f;
        a[k][3] = axis[k] == 2 ? s : 0.f;
    }
    float m[4];
    enc_qmul(a[1], a[2], m);
    enc_qmul(a[0], m, q);
}

__global__ __launch_bounds__(kBvhThreads) void k_bvh_decode(BvhArgs p) {
    __shared__ unsigned char wtot[2][kBvhWaves][kBvhMaxJoints];      // parity of a wave's flip bits, per round parity
    __shared__ unsigned char carry[2][kBvhMaxJoints];                // parity of all earlier rounds
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = p.T, C = p.C, Jf = p.Jf;
    int len = p.lengths ? p.lengths[b] : T;
    len = min(max(len, 1), T);               // no access leaves the clip, whatever the caller wrote
    const int J = p.nsel ? p.nsel : Jf;
    const float* ch = p.ch + (size_t)b * T * C;
    float* ws = p.ws + (size_t)b * T * Jf * kBvhWs;
    // offsets inside a clip fit an int (at the caps: 16384 frames x 96 joints x 11 floats); only the clip's bases are 64-bit
    const size_t ob = (size_t)b * p.Tout * J;
    float* rot = p.rot + ob * 4;
    float* pos = p.pos + ob * 3;
    float* lpos = p.lpos ? p.lpos + ob * 3 : nullptr;
    float* grot = p.grot ? p.grot + ob * 4 : nullptr;
    const unsigned long long below = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);     // lanes 0 .. lane
    if (tid < Jf) carry[0][tid] = 0;
    // the first round's carry is read after that round's barrier

    for (int base = 0, r = 0; base < len; base += kBvhThreads, r ^= 1) {
        const int t = base + tid;
        const bool live = t < len;
        unsigned long long bits_lo = 0, bits_hi = 0;                 // this lane's parity within its wave, one bit a joint
        for (int j = 0; j < Jf; j++) {
            const int rc = p.rot_col[j];
            bool flip = false;
            if (live && rc >= 0) {
                float q[4];
                bvh_eul2q(ch + (t * C + rc), p.axis, q);
                float* w = ws + (t * Jf + j) * kBvhWs;
#pragma unroll
                for (int k = 0; k < 4; k++) w[k] = q[k];
                if (t > 0) {
                    float q0[4];
                    bvh_eul2q(ch + ((t - 1) * C + rc), p.axis, q0);
                    flip = q0[0] * q[0] + q0[1] * q[1] + q0[2] * q[2] + q0[3] * q[3] < 0.f;
                }
            }
            const unsigned long long bal = __ballot(flip);
            const unsigned long long mine = (unsigned long long)(__popcll(bal & below) & 1);
            if (j < 64) bits_lo |= mine << j;
            else bits_hi |= mine << (j - 64);
            if (lane == 0) wtot[r][wave][j] = (unsigned char)(__popcll(bal) & 1);
        }
        __syncthreads();
        if (tid < Jf) {                      // the next round's carry; this round's is read below, the other buffer is written here
            unsigned v = carry[r][tid];
#pragma unroll
            for (int w = 0; w < kBvhWaves; w++) v ^= wtot[r][w][tid];
            carry[r ^ 1][tid] = (unsigned char)v;
        }
        const int k_out = t - p.phase;
        if (!live || k_out < 0 || k_out % p.stride) continue;
        const int to = k_out / p.stride;
        for (int j = 0; j < Jf; j++) {
            unsigned neg = (unsigned)((j < 64 ? bits_lo >> j : bits_hi >> (j - 64)) & 1ull) ^ carry[r][j];
            for (int w = 0; w < wave; w++) neg ^= wtot[r][w][j];
            float* w = ws + (t * Jf + j) * kBvhWs;
            float q[4] = {1.f, 0.f, 0.f, 0.f}, l[3];
            if (p.rot_col[j] >= 0) {
#pragma unroll
                for (int k = 0; k < 4; k++) q[k] = neg ? -w[k] : w[k];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = q[k];                 // Anim.quats
            const int pc = p.pos_col[j];
#pragma unroll
            for (int k = 0; k < 3; k++) l[k] = (pc >= 0 ? ch[t * C + pc + k] : p.off[j][k]) * p.scale;
            // quat_fk: qnorm, then gr = gr[parent] (x) lrot, gp = qrot(gr[parent], lpos) + gp[parent]
            const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            float qn[4], gr[4], gp[3];
#pragma unroll
            for (int k = 0; k < 4; k++) qn[k] = q[k] / n;
            const int par = p.parent[j];
            if (par < 0) {
#pragma unroll
                for (int k = 0; k < 4; k++) gr[k] = qn[k];
#pragma unroll
                for (int k = 0; k < 3; k++) gp[k] = l[k];
            } else {
                const float* wp = ws + (t * Jf + par) * kBvhWs;
                const float pr[4] = {wp[4], wp[5], wp[6], wp[7]};
                float rl[3];
                enc_qrot(pr, l, rl);
#pragma unroll
                for (int k = 0; k < 3; k++) gp[k] = rl[k] + wp[8 + k];
                enc_qmul(pr, qn, gr);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) w[4 + k] = gr[k];
#pragma unroll
            for (int k = 0; k < 3; k++) w[8 + k] = gp[k];
            if (!p.nsel) {
                const int o = to * J + j;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    rot[o * 4 + k] = q[k];
                    if (grot) grot[o * 4 + k] = gr[k];
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    pos[o * 3 + k] = gp[k];
                    if (lpos) lpos[o * 3 + k] = l[k];
                }
            }
        }
        for (int s = 0; s < p.nsel; s++) {   // the lane's own gr / gp of the frame, read back
            const int j = p.sel[s], anc = p.sel_anc[s];
            const float* w = ws + (t * Jf + j) * kBvhWs;
            float q[4], l[3];
            if (p.sel_direct[s]) {
#pragma unroll
                for (int k = 0; k < 4; k++) q[k] = w[k];
                const int pc = p.pos_col[j];
#pragma unroll
                for (int k = 0; k < 3; k++) l[k] = (pc >= 0 ? ch[t * C + pc + k] : p.off[j][k]) * p.scale;
            } else if (anc < 0) {
#pragma unroll
                for (int k = 0; k < 4; k++) q[k] = w[4 + k];
#pragma unroll
                for (int k = 0; k < 3; k++) l[k] = w[8 + k];
            } else {
                const float* wa = ws + (t * Jf + anc) * kBvhWs;
                const float ga[4] = {wa[4], wa[5], wa[6], wa[7]}, gj[4] = {w[4], w[5], w[6], w[7]};
                const float d[3] = {w[8] - wa[8], w[9] - wa[9], w[10] - wa[10]};
                float gi[4];
                enc_qinv(ga, gi);
                enc_qmul(gi, gj, q);
                enc_qrot(gi, d, l);
            }
            const int o = to * J + s;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                rot[o * 4 + k] = q[k];
                if (grot) grot[o * 4 + k] = w[4 + k];
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                pos[o * 3 + k] = w[8 + k];
                if (lpos) lpos[o * 3 + k] = l[k];
            }
        }
    }
    // ---- frames at or past the clip's length: exact zeros
    const int rows = len > p.phase ? (len - p.phase + p.stride - 1) / p.stride : 0;
    for (int i = tid + rows * J; i < p.Tout * J; i += kBvhThreads) {
        const int o = i;                     // an output joint of the clip
#pragma unroll
        for (int k = 0; k < 4; k++) {
            rot[o * 4 + k] = 0.f;
            if (grot) grot[o * 4 + k] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            pos[o * 3 + k] = 0.f;
            if (lpos) lpos[o * 3 + k] = 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------ quaternions -> the writer's channel values
constexpr int kQ2cZyx = 0, kQ2cXzy = 1;      // the file orders whose reverse q2eul has formulas for: 'xyz' and 'yzx'

struct Q2cArgs {
    const float* quats;                      // [B][T][J][4]
    const float* root_pos;                   // [B][T][3]
    const float* positions;                  // [B][T][J][3] or null: a position in front of every joint's angles
    int B, T, J, order;
    short perm[kBvhMaxJoints];               // output slot -> joint (the writer's save_joint_seq)
    float* out;                              // [B][T][3 + 3 J] or [B][T][6 J]
};

__global__ __launch_bounds__(256) void k_quats_to_channels(Q2cArgs p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)p.B * p.T * p.J) return;
    const int s = (int)(i % p.J);
    const long long bt = i / p.J;
    const int j = p.perm[s];
    const float* q = p.quats + ((size_t)bt * p.J + j) * 4;
    const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float q0 = q[0] / n, q1 = q[1] / n, q2 = q[2] / n, q3 = q[3] / n;
    float e[3];                              // by axis: x, y, z
    if (p.order == kQ2cZyx) {                // q2eul 'xyz'
        e[0] = atan2f(2.f * (q0 * q1 + q2 * q3), 1.f - 2.f * (q1 * q1 + q2 * q2));
        e[1] = asinf(fminf(fmaxf(2.f * (q0 * q2 - q3 * q1), -1.f), 1.f));
        e[2] = atan2f(2.f * (q0 * q3 + q1 * q2), 1.f - 2.f * (q2 * q2 + q3 * q3));
    } else {                                 // q2eul 'yzx'
        e[0] = atan2f(2.f * (q1 * q0 - q2 * q3), -q1 * q1 + q2 * q2 - q3 * q3 + q0 * q0);
        e[1] = atan2f(2.f * (q2 * q0 - q1 * q3), q1 * q1 - q2 * q2 - q3 * q3 + q0 * q0);
        e[2] = asinf(fminf(fmaxf(2.f * (q1 * q2 + q3 * q0), -1.f), 1.f));
    }
    const int a0 = p.order == kQ2cZyx ? 2 : 0, a1 = p.order == kQ2cZyx ? 1 : 2, a2 = p.order == kQ2cZyx ? 0 : 1;
    const float deg = 57.29577951308232f;
    const int width = p.positions ? 6 * p.J : 3 + 3 * p.J;
    float* o = p.out + (size_t)bt * width + (p.positions ? 6 * s : 3 + 3 * s);
    if (s == 0 || p.positions) {
        float* op = p.positions ? o : p.out + (size_t)bt * width;
        const float* src = s == 0 ? p.root_pos + (size_t)bt * 3 : p.positions + ((size_t)bt * p.J + j) * 3;
        op[0] = src[0];
        op[1] = src[1];
        op[2] = src[2];
    }
    if (p.positions) o += 3;
    o[0] = e[a0] * deg;
    o[1] = e[a1] * deg;
    o[2] = e[a2] * deg;
}

// ------------------------------------------------------------------------------------------ uniform_skeleton_basic
// The clip length is bounded as the decode's is: nothing a frame needs is kept on chip.
constexpr int kRetMaxFrames = kBvhMaxFrames;

struct RetArgs {
    float tgt[kEncMaxJoints][3];             // the target offsets
    float tgt_leg;                           // max |component| of the target's two leg offsets, summed
    int leg[2], leg_parent[2];               // l_idx and their parents (common/skeleton.py:11-15)
    float* out;                              // [B][T][J][3]
};

// One workgroup per clip, one frame per lane.  `e` carries the clip, the lengths, the face joints, the raw offsets and the chain links
// exactly as k_encode reads them.
__global__ __launch_bounds__(kEncThreads) void k_retarget(EncArgs e, RetArgs x) {
    const int b = blockIdx.x, tid = threadIdx.x, T = e.T, J = e.J;
    int len = e.lengths ? e.lengths[b] : T;
    len = min(max(len, 1), T);
    const float* in = e.pos + (size_t)b * T * J * 3;
    float* out = x.out + (size_t)b * T * J * 3;
    // the leg ratio: the largest absolute component of |bone| * raw of frame 0, not a norm (the reference's quirk, kept)
    float src_leg = 0.f;
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const float* c = in + (size_t)x.leg[a] * 3;
        const float* q = in + (size_t)x.leg_parent[a] * 3;
        const float d[3] = {c[0] - q[0], c[1] - q[1], c[2] - q[2]};
        const float n = sqrtf(enc_dot(d, d));
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) m = fmaxf(m, fabsf(n * e.raw[x.leg[a]][k]));
        src_leg += m;
    }
    const float ratio = x.tgt_leg / src_leg;
    for (int t = tid; t < len; t += kEncThreads) {
        const float* f = in + (size_t)t * J * 3;
        float* o = out + (size_t)t * J * 3;
        for (int j = 0; j < J; j++)
            if (!e.named[j]) {               // np.zeros where no chain places a joint; the root is set below
#pragma unroll
                for (int k = 0; k < 3; k++) o[3 * j + k] = 0.f;
            }
#pragma unroll
        for (int k = 0; k < 3; k++) o[k] = f[k] * ratio;
        float r[4] = {1.f, 0.f, 0.f, 0.f};
        if (t > 0) {
            float fw[3] = {0.f, 0.f, 0.f};
            enc_forward(f + 3 * e.face[0], f + 3 * e.face[1], f + 3 * e.face[2], f + 3 * e.face[3], fw[0], fw[2]);
            const float n = sqrtf(enc_dot(fw, fw));
            fw[0] /= n;
            fw[2] /= n;
            const float z[3] = {0.f, 0.f, 1.f};
            enc_qbetween(z, fw, r);
        }
        float R[4] = {r[0], r[1], r[2], r[3]};
        for (int l = 0; l < e.n_links; l++) {
            if (e.link_first[l]) {
#pragma unroll
                for (int k = 0; k < 4; k++) R[k] = r[k];
            }
            const int c = e.link_child[l], a = e.link_parent[l];
            float v[3], quv[4], Ri[4], loc[4], Rn[4], g[3];
#pragma unroll
            for (int k = 0; k < 3; k++) v[k] = f[3 * c + k] - f[3 * a + k];
            const float n = sqrtf(enc_dot(v, v));
#pragma unroll
            for (int k = 0; k < 3; k++) v[k] /= n;
            const float u[3] = {e.raw[c][0], e.raw[c][1], e.raw[c][2]};
            enc_qbetween(u, v, quv);
            enc_qinv(R, Ri);
            enc_qmul(Ri, quv, loc);
            enc_qmul(R, loc, Rn);            // the IK's running R and the FK's: the same product
#pragma unroll
            for (int k = 0; k < 4; k++) R[k] = Rn[k];
            enc_qrot(R, x.tgt[c], g);
#pragma unroll
            for (int k = 0; k < 3; k++) o[3 * c + k] = g[k] + o[3 * a + k];       // the lane's own store of the chain's previous joint
        }
    }
    for (int i = tid + len * J * 3; i < T * J * 3; i += kEncThreads) out[i] = 0.f;
}

}  // namespace mst
