// The launch plan of the sampling path: which kernels a launch sequence runs, at what tile height, and in how many clip slices a loop
// runs.  Plain C++ for the host (no HIP header, no f16; k_embed_out alone reads the constexpr rules of embed_out_staged): every launcher
// of mst_engine.hip follows it, tests/plan_mirror.py mirrors it, and tests/test_launch_plan_cpu.py compares the two on the CPU through
// a driver that includes only this file.
#pragma once

namespace mst {

// The engine's switches the plan depends on, copied per call (mst_engine.hip: plan_knobs).  Plain ints only: the graph key of a
// sampling loop appends the struct word by word, so a knob added here is part of the key.
struct PlanKnobs {
    int small_m, small_ln, small_ln_m, small_fast, precise, fuse_qkv_attn, fuse_tail, tail_ntb, ln128_min_m, trunk_groups, num_layers, nsplit,
        dbg_stop /* a debug stop is set (mst_debug_stop_after) */;
};
constexpr int PLAN_KNOB_WORDS = sizeof(PlanKnobs) / sizeof(int);

// SMALL_RING: 64 x 128 ring GEMMs + row-wise LayerNorm (split operands when TrunkPlan::precise); SMALL_ROWS: the rows GEMMs of mst_small.h
// instead; SMALL_ROWS_LN: ... with the LayerNorms inside the GEMM behind them; RESIDENT: the whole stack as one launch of resident groups
// (mst_trunk.h); LARGE: large tiles, QKV + attention and then the layer tail per layer
enum TrunkPath { PATH_SMALL_RING = 0, PATH_SMALL_ROWS, PATH_SMALL_ROWS_LN, PATH_RESIDENT, PATH_LARGE };
enum QkvAttn { QA_UNFUSED = 0, QA_STREAMED /* k_qkv_attention2 */, QA_RING /* round 2's k_qkv_attention */ };

struct TrunkPlan {
    int path, precise /* every activation multiplied as hi + lo */, lnf /* path == PATH_SMALL_ROWS_LN */;
    int qkv_attn, fuse_tail, ln128;     // large tiles: QkvAttn; K6 + K7 + K8 as k_layer_tail; else the LayerNorm GEMMs on 128-token tiles
    int tail_ntb, nt16;                 // 16-token blocks per tile of the fused tail; k_qkv_attention2<NT16>
};

// The role-swapped QKV+attention kernel holds K, V and Q images of 16 ceil(S / 16) rows in LDS: up to S = 208 (the model's 196 frames + 1).
inline bool qkv_attn2_fits(int S) { return S <= 208; }

// One launch sequence over `rows` clips of T frames (+ 1 conditioning token) that shares the chip with `slices` - 1 others.
inline TrunkPlan plan_trunk(const PlanKnobs& k, int rows, int T, int slices, int instrumented) {
    const int S = T + 1;
    const long long M = (long long)rows * S;
    TrunkPlan p{};
    const bool small = k.precise || (k.small_m > 0 && M <= k.small_m);
    // Clips of at most 16 frames: so few values are averaged per output that the f16 rounding of the ACTIVATION operands shows at the
    // 1e-3 bar (oracle rounding model, classifier-free guidance: 1.07e-3 mean over seeds at 1 frame, 9.1e-4 at 5 frames, 7.6e-4 at
    // 196).  Those launches -- a handful of tiles, nowhere near a throughput regime -- multiply every activation as hi + lo: 6.5e-4.
    p.precise = k.precise || (small && T <= 16);
    // round 4: without split operands the four GEMMs run as resident-tile / streamed-weight kernels (MST_SMALL_FAST=0: the ring) ...
    const bool fast = small && !p.precise && k.small_fast;
    // ... and the LayerNorms inside the GEMM behind them (MST_SMALL_LN=0: every LayerNorm a launch)
    p.lnf = fast && k.small_ln && !k.dbg_stop && M <= k.small_ln_m;
    const int n16 = (S + 15) / 16;
    // The resident-group trunk: token counts of 13 blocks of 16 (193 .. 208 tokens: the model's 196 frames), the default fused kernels,
    // no debug stop, no instrumented step, at most 8 layers.
    const bool resident = k.trunk_groups && n16 == 13 && k.fuse_qkv_attn == 1 && k.fuse_tail && k.tail_ntb == 0 && !k.dbg_stop && !k.precise &&
                          k.num_layers <= 8 && !instrumented;
    p.path = small ? (p.lnf ? PATH_SMALL_ROWS_LN : fast ? PATH_SMALL_ROWS : PATH_SMALL_RING) : (resident ? PATH_RESIDENT : PATH_LARGE);
    // 1 (default): weights streamed to registers, tokens through the ring; 2: round 2's kernel, which also takes S = 209..224
    p.qkv_attn = !k.fuse_qkv_attn ? QA_UNFUSED : (k.fuse_qkv_attn == 1 && qkv_attn2_fits(S) ? QA_STREAMED : QA_RING);
    p.fuse_tail = k.fuse_tail != 0;
    p.ln128 = M >= k.ln128_min_m;
    // Tile height of the fused tail.  A launch that has the chip to itself and does not fill it runs on more, lower tiles; the clip
    // slices of a sampling loop share the chip (3 x 68 tiles of 64 tokens at the headline batch) and keep the 64-token tile: 48-token
    // tiles measured 99.4 against 105.3 clips/s there, 32-token tiles 88.3 (tools/experiments/r4_ntb_ab.sh).
    int ntb = k.tail_ntb ? k.tail_ntb : 4;
    if (!k.tail_ntb && slices == 1) {
        if ((M + 31) / 32 <= 256) ntb = 2;
        else if ((M + 47) / 48 <= 256) ntb = 3;
    }
    p.tail_ntb = ntb;
    p.nt16 = n16 == 13 ? 13 : (n16 + 1) / 2 * 2;
    return p;
}

// Token blocks of 16 per tile of a rows GEMM (mst_small.h) over M rows: 1 up to ntb1_m rows (a clip or two: a quarter of the DMA burst
// in front of the first MFMA), 2 above ntb2_from, 4 between.  The training path's small launches follow it too.
inline int rows_ntb(int M, int ntb1_m, int ntb2_from) { return M <= ntb1_m ? 1 : (M > ntb2_from ? 2 : 4); }

// How many independent clip slices a loop over `batch` clips of `frames` frames runs as.  Measured, same box, interleaved
// (tools/experiments/streams_ab.sh, streams_ab_configs.sh), round-2 kernels at 196 frames: a batch whose tiles are all resident at
// once on the large-tile path wanted ONE slice (batch 64: 82.0 / 81.6 / 80.6 clips/s at 1 / 2 / 3 slices; batch 32: 43.8 vs 39.7 at 3
// -- slices would drop to the small-tile kernels); more tiles than CUs want one slice per round of tiles (batch 128 = 394 tiles:
// 78.5 / 91.2 / 88.0 at 1 / 2 / 3; CFG at 64 clips: 39.8 / 45.5 / 44.6); the small-tile path (batch 16: 22.1 vs 28.8) up to three.
inline int plan_slices(const PlanKnobs& k, int batch, int cfg, int frames) {
    if (k.dbg_stop) return 1;
    const int rows = (cfg ? 2 : 1) * batch;
    int n = k.nsplit;
    if (n == 0) {
        const int path = plan_trunk(k, rows, frames, 1, 0).path;       // of the whole batch as one launch sequence
        if (path == PATH_RESIDENT) return 1;                           // every clip is a chain of its own inside ONE launch
        const long long M = (long long)rows * (frames + 1);
        const long long tiles = (M + 63) / 64, waves = (tiles + 255) / 256;      // rounds of 64-token tiles over the 256 CUs
        n = path != PATH_LARGE ? 3 : (int)(waves < 3 ? waves : 3);
        // Round 3: a batch that fills most of the chip in ONE round (the headline: 64 clips = 197 tiles) runs every workgroup through the
        // same phase at the same time; three slices of it (each still on the large-tile path) decorrelate them.  Same-box, interleaved,
        // 1 vs 3 slices at 64 clips: 96.9 vs 98.9 clips/s on a slow box (three rounds), 103.2 vs 104.1 on a fast one; at 48 clips
        // (148 tiles) two slices are a wash (84.0 vs 83.7) and three fall to the small-tile kernels.
        if (path == PATH_LARGE && waves == 1 && tiles >= 192) n = 3;
    }
    while (n > 1 && rows / n < 8) n--;                       // at least 8 rows through the transformer per slice
    return n;
}

// ------------------------------------------------------------------------------ the two projections (K3, K9)
// The latency kernels of mst_embed.h work on 64-frame tiles inside this much dynamic LDS (EmbCfg::BT / EmbCfg::SMEM: mst_engine.hip
// asserts that they match).
constexpr int EMBED_BT = 64, EMBED_SMEM = 160 * 1024;

// EMBED_LATENCY: k_embed_in<KS> / k_embed_out<NBW, MODE, NX, KSN> (mst_embed.h); EMBED_RING: the slab ring (launch_gemm_dma), which
// also multiplies split WEIGHTS (precise mode) and a caller's weight (the pose embedding's backward).
enum EmbedKernel { EMBED_LATENCY = 0, EMBED_RING };

// K of the pose-embedding GEMM: whole 32-deep slabs, and at least the 3 slabs the ring keeps in flight.
inline int embed_kin_pad(int feats) { const int k = (feats + 31) / 32 * 32; return k < 96 ? 96 : k; }
// 16-feature blocks per wave of k_embed_out: eight waves own blocks w, w + 8, ...
inline int embed_out_nbw(int feats) { return (feats + 127) / 128; }

struct EmbedInPlan { int kin_pad, ks /* k_embed_in<KS> */, kernel /* EmbedKernel */; };
inline EmbedInPlan plan_embed_in(int feats, int precise, int embed_fast) {
    const int kp = embed_kin_pad(feats);
    return EmbedInPlan{kp, kp / 32, embed_fast && !precise ? EMBED_LATENCY : EMBED_RING};
}

// Can a sampling step's output projection also embed the NEXT step (k_embed_out<.., KSN>)?  The shapes the reference's datasets have
// (150 / 181 / 190 / 263 features: 5 / 6 / 6 / 9 k-steps), frame counts the staged epilogue takes, and the tile plus the two frame
// images must fit the LDS.  Returns KSN, or 0.
inline int embed_next_ksn(int feats, int T, int precise, int embed_fast) {
    const int ks = embed_kin_pad(feats) / 32, nbw = embed_out_nbw(feats);
    if (!embed_fast || precise || (T & 3)) return 0;
    if (!((ks == 5 && nbw == 2) || (ks == 6 && nbw == 2) || (ks == 9 && nbw == 3))) return 0;
    return (long long)feats * (EMBED_BT + 4) * 4 + 16 + 2LL * EMBED_BT * (ks * 64 + 16) <= (long long)EMBED_SMEM ? ks : 0;
}

// Which epilogue k_embed_out<NBW, MODE, ..> runs: the staged one (OutItems) on a diffusion step, up to three blocks per wave (4 blocks =
// 16 items per thread: too many registers), whose frame count is a multiple of 4 (a float4 never straddles a clip); else
// DEpiEmbedOut::finish.  The kernel decides by itself, per launch, from THESE two rules (constexpr: hipcc compiles them for the device
// too; the first is a constant of the instantiation), so the plan below and the kernel cannot drift apart.
constexpr bool embed_out_can_stage(int nbw, int mode) { return mode != 0 && nbw <= 3; }
constexpr bool embed_out_frames_stage(int T) { return (T & 3) == 0; }
constexpr bool embed_out_staged(int nbw, int mode, int T) { return embed_out_can_stage(nbw, mode) && embed_out_frames_stage(T); }

struct EmbedOutPlan {
    int kernel;                 // EmbedKernel
    int nbw, nx, staged;        // EMBED_LATENCY: k_embed_out<NBW, MODE, NX>; `staged`: embed_out_staged, as the kernel will find it
    int ksn;                    // ... and the KSN of the fused next-step embedding a plain loop step may ask for (0: none)
    int ring_bf, ring_xs;       // EMBED_RING: launch_out_nx<MODE, BF, ..> and its XS (2: hi and lo of a k-slab beside one weight slab)
};
// mode: DEpiEmbedOut<MODE> (0 = the model output alone); hi_lo: the stream is a split pair (ws.hx / ws.hl); custom_w: a caller's weight
// or bias (the pose embedding's backward).
inline EmbedOutPlan plan_embed_out(int feats, int T, int cfg, int precise, int embed_fast, int mode, int hi_lo, int custom_w) {
    EmbedOutPlan p{};
    const int nbw = embed_out_nbw(feats);
    p.nx = cfg ? 2 : 1;
    if (embed_fast && !precise && hi_lo && !custom_w && !(cfg && nbw == 4)) {        // (385+ features under CFG: its two accumulator sets spill)
        p.kernel = EMBED_LATENCY;
        p.nbw = nbw;
        p.staged = embed_out_staged(nbw, mode, T);
        p.ksn = mode != 0 && !cfg ? embed_next_ksn(feats, T, precise, embed_fast) : 0;
        return p;
    }
    p.kernel = EMBED_RING;
    p.ring_bf = feats <= 256 ? 256 : feats <= 384 ? 384 : 512;
    p.ring_xs = hi_lo && p.ring_bf <= 384 ? 2 : 1;                 // (512 rows: the ring no longer fits the LDS twice; the K range runs twice)
    return p;
}

// Slice i of `batch` clips in n slices: the last one may be short, and clips <= 0 means the slice is empty.
struct SliceRange { int first, clips; };
inline SliceRange slice_of(int batch, int n, int i) {
    const int per = (batch + n - 1) / n, c0 = i * per;
    return SliceRange{c0, c0 + per <= batch ? per : batch - c0};
}

}  // namespace mst
