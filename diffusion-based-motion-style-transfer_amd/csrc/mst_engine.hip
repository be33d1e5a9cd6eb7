// libmst_engine.so -- host side: engine state, launch sequence, C ABI (include/mst_engine.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/mst_engine.h"
#include "mst_attn.h"
#include "mst_train.h"
#include "mst_common.h"
#include "mst_elem.h"
#include "mst_gemm_dma.h"
#include "mst_tail.h"
#include "mst_trunk.h"
#include "mst_tail_bwd.h"
#ifdef EMB_PROBE            // diagnostic build only (tools/experiments/r4_embed_stamps.py): wave 0..7 of every workgroup stamp the 100 MHz clock at the phase marks
__device__ unsigned long long g_emb_stamp[512][8][8];
#define EMB_MARK(i) if ((threadIdx.x & 63) == 0 && blockIdx.x < 512) g_emb_stamp[blockIdx.x][threadIdx.x >> 6][i] = __builtin_amdgcn_s_memrealtime();
extern "C" int mst_probe_read(void* dst) { return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_emb_stamp), sizeof(g_emb_stamp)) == hipSuccess ? 0 : 1; }
#endif
#include "mst_embed.h"
#include "mst_small.h"
#include "mst_style.h"
#include "mst_feet.h"
#include "mst_ik.h"
#include "mst_encode.h"
#include "mst_bvh.h"
#include "mst_rotdec.h"
#include "mst_jguide.h"
#include "mst_eval.h"
#include "mst_window.h"
#include "mst_plan.h"
#include "mst_vb.h"
#include "mst_clip.h"
#include "mst_smpl.h"
#include "mst_smplify.h"
#include "mst_track.h"
#include "mst_render.h"
#include "mst_mesh.h"

using namespace mst;

// wide (QKV / FFN1) tile: WIDE_BT tokens x 256 features, 8 waves of (WIDE_BT/64) x 2 MFMA tiles
#define WIDE_BT 128   // same-box A/B (round 1, script since removed): 128/3-slot/XCD 52.4 clips/s, 128/4-slot 47.2, 256/4-slot 47.5
#define WIDE_NS 3     // 3 x 24 KB ring: two blocks share a CU
#define FFN1_BF 256   // same-box A/B: 128x512 tiles (one 8-wave block per CU) 40 us vs 35 us for two co-resident 128x256 blocks
#define WIDE_XCD 1
// LayerNorm GEMMs (64 x 512 tiles, one block per CU): slab depth / ring slots.  64-deep slabs move whole
// 128-B cache lines per DMA segment; 32-deep slabs fetch every line twice, one slab apart (gemm_bench: 24.3 -> 19.5 us at K=512).
#define LN_BK 64
#define LN_NS (LN_BK == 64 ? 2 : 4)
// (These are fixed constants, not -D knobs: a stray compile flag must not be able to change what the product library computes or how
// fast -- _native.build_in_place passes no -D but the source hash, and folds its flag list into that hash.)
// launch geometry of a wide GEMM over nx token tiles x ny feature tiles (1-D when XCD-aware)
static dim3 wide_grid(int M, int ny) {
    const int nx = (M + WIDE_BT - 1) / WIDE_BT;
    return WIDE_XCD ? dim3(((nx + 7) / 8) * 8 * ny, 1, 1) : dim3(nx, ny, 1);
}

// dgrad GEMMs that end in the fp32 gradient stream (N = 512): token tile
#define DG_BT 128     // same-box A/B of the backward pass at batch 64: 128 x 256 tiles 2.99 ms, 64 x 256 (394 blocks, two per CU) 3.10 ms
static dim3 dg_grid(int M, int ny) {
    const int nx = (M + DG_BT - 1) / DG_BT;
    return WIDE_XCD ? dim3(((nx + 7) / 8) * 8 * ny, 1, 1) : dim3(nx, ny, 1);
}

// ------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
static int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}
#define HIPCHECK(x)                                                                              \
    do {                                                                                         \
        hipError_t _e = (x);                                                                     \
        if (_e != hipSuccess) return fail("%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#define CHECK(x)                 \
    do {                         \
        int _r = (x);            \
        if (_r) return _r;       \
    } while (0)

extern "C" const char* mst_last_error(void) { return g_err; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a PER-DEVICE opt-in: remember (kernel, device) pairs, so a second
// engine on another GPU of the same process gets its own (a process-wide "done" flag would launch there without it).
static int ensure_dyn_lds(const void* kern, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    HIPCHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({kern, dev})) return 0;
    HIPCHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.insert({kern, dev});
    return 0;
}

// Every ABI entry runs on its engine's / schedule's device and leaves the caller's current device as it found it.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) cur = -1;
        if (cur != dev) {
            ok = hipSetDevice(dev) == hipSuccess;
            prev = cur;
        }
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define ON_DEVICE(dev)                                                    \
    DeviceGuard _dev_guard(dev);                                          \
    if (!_dev_guard.ok) return fail("hipSetDevice(%d) failed (%s:%d)", (int)(dev), __FILE__, __LINE__)
extern "C" int mst_version(void) { return 2; }
#ifndef MST_SRC_HASH
#define MST_SRC_HASH "unhashed"
#endif
extern "C" const char* mst_source_hash(void) { return MST_SRC_HASH; }

// ------------------------------------------------------------------------------------------ state
struct mst_schedule {
    int n = 0, device = 0;
    float* tab = nullptr;          // [NTAB][n] float32
    long long* tmap = nullptr;     // [n] int64 original-process timesteps
    float* var = nullptr;          // [n] float32 variance row (mst_schedule_set_variance; read by the guided ancestral step alone)
};

struct LayerW {
    f16 *w_in = nullptr, *w_out = nullptr, *w1 = nullptr, *w2 = nullptr;
    float *b_in = nullptr, *b_out = nullptr, *b1 = nullptr, *b2 = nullptr;
    float *g1 = nullptr, *be1 = nullptr, *g2 = nullptr, *be2 = nullptr;
    // [in][out] f16 copies: the "weights" operand of the dgrad GEMMs (training path)
    f16 *w_inT = nullptr, *w_outT = nullptr, *w1T = nullptr, *w2T = nullptr;
    f16* wtail = nullptr;           // W_out | W1 | W2 as the fused layer tail's slab stream (mst_tail.h, k_pack_tail)
    f16* wtail_bwd = nullptr;       // W2^T | W1^T | W_out^T as the fused BACKWARD tail's stream (mst_tail_bwd.h, k_pack_tail_bwd): allocated and packed on first use
    bool tailb_dirty = true;
    f16 *w_in_lo = nullptr, *w_out_lo = nullptr, *w1_lo = nullptr, *w2_lo = nullptr;   // f16(w - f16(w)): the weights' lo halves (precise mode)
    bool tail_dirty = true, qkv_dirty = true;   // wtail / wqkv are older than w_out | w1 | w2 / w_in: repacked by ensure_packed() before the next sampling launch
    f16* wqkv = nullptr;            // W_in as the fused QKV+attention kernel's per-(head, wave) fragment streams (mst_attn.h, k_pack_qkv)
    f16 *wsm_in = nullptr, *wsm_out = nullptr, *wsm_1 = nullptr, *wsm_2 = nullptr;   // the four matrices as [16-row block][k-step] fragments: the small-launch GEMMs (mst_small.h)
    bool small_dirty = true;        // ... older than the plain matrices (ensure_packed / the training forward repack them, all stale layers in one launch)
};

// engine-owned scratch of the backward pass, allocated on the first training call
struct TrainWS {
    bool ready = false;
    float *g0 = nullptr, *g1 = nullptr;                 // fp32 gradient stream, ping-pong
    // operands the wgrad stream reads while the dgrad chain moves on: double-buffered by layer parity
    f16 *dbr2[2] = {nullptr, nullptr}, *dbr1[2] = {nullptr, nullptr}, *dpre[2] = {nullptr, nullptr}, *dqkv[2] = {nullptr, nullptr};
    f16* datt = nullptr;
    f16* hidr[2] = {nullptr, nullptr};                  // hid = dropout(GELU(pre)) regenerated by the FFN2 dgrad epilogue: the operand of dW2 (by layer parity)
    hipEvent_t ev_ready = nullptr, ev_side[2] = {nullptr, nullptr};
    hipEvent_t ev_layer[16] = {nullptr};                // recorded when layer l's parameter gradients of the LAST backward call are enqueued
    bool layer_done[16] = {false};
    float* part = nullptr;                              // split-K partial products
    float* ln_part = nullptr;                           // k_ln_bwd's per-block [dgamma | dbeta | dbias] partials (dgrad stream)
    float* ln_part2 = nullptr;                          // ... LayerNorm2's, when both LayerNorms of a layer are finished by one launch (round 6)
    // round 6: a layer's split-K reduces wait for ONE batched launch at the layer's end (train_stack_backward sets red_defer around its layers;
    // each weight gradient then gets a region of `part` of its own).  MST_WGRAD_REDUCE_BATCH=0: a reduce behind every weight gradient.
    RedJobs red_jobs{};
    int n_red = 0;
    bool red_defer = false;
    size_t part_used = 0, part_cap = 0;
    float* cs_part = nullptr;                           // k_colsum_f16's per-row-block bias-gradient partials (wgrad stream)
    float* zeros = nullptr;                             // zero bias
    float* gscale = nullptr;                            // [0] scale applied to the incoming gradient, [1] its inverse
    unsigned* amax = nullptr;
    size_t split_cap = 0;
};

enum Family { FAM_COND = 0, FAM_EMBED_IN, FAM_QKV, FAM_ATTN, FAM_OUTPROJ_LN, FAM_FFN1, FAM_FFN2_LN, FAM_EMBED_OUT, FAM_QKV_ATTN, FAM_TAIL, FAM_WGRAD, FAM_COUNT };
static const char* kFamilyNames[FAM_COUNT] = {"cond_token", "embed_in", "qkv_gemm", "attention", "outproj_ln_gemm",
                                              "ffn1_gelu_gemm", "ffn2_ln_gemm", "embed_out_step", "qkv_attention_fused",
                                              "layer_tail_fused", "wgrad_tr"};

struct ProfPoint { int fam; hipEvent_t a, b; };

// Several styles in one batch (mst_style_slots / mst_set_styles; csrc/mst_style.h).  Where one slice of a call finds its tables inside
// the engine's plan buffer (int offsets; segments per tile height 16, 32, 48, 64 rows).
struct StyleSlice { int rows = 0, off_slot = 0, off_order = 0, off_seg[4] = {0, 0, 0, 0}, nseg[4] = {0, 0, 0, 0}; };

struct mst_engine {
    mst_config cfg;
    int S_max = 0, M_pad = 0, kin_pad = 0, nt_out = 0, fout_pad = 0;
    LayerW L[16];
    f16 *w_pose_in = nullptr, *w_pose_out = nullptr;
    f16 *w_pose_in_lo = nullptr, *w_pose_out_lo = nullptr;      // lo halves (precise mode)
    f16 *w_pose_inT = nullptr, *w_pose_outT = nullptr;   // [fout_pad][512] and [512][kin_pad]: the projections' dgrad operands
    float *b_pose_in = nullptr, *b_pose_out = nullptr;
    f16 *w_pose_in_pk = nullptr, *w_pose_out_pk = nullptr;      // the two projections as per-wave fragment streams (mst_embed.h, k_pack_wave_blocks)
    bool pose_in_dirty = true, pose_out_dirty = true;          // ... older than w_pose_in / w_pose_out: repacked by ensure_packed()
    int small_ln = 1, small_ln_m = 512;   // ... with the LayerNorms inside the consuming GEMMs, up to this many stream rows (MST_SMALL_LN, MST_SMALL_LN_M; tools/experiments/r4_small_sweep.sh: ahead through 2 clips x 197 rows, behind from 4)
    int train_fuse_ln2_bwd = 1;           // ... with LayerNorm2's backward at the head of the same launch (frozen stacks; MST_TRAIN_FUSE_LN2_BWD=0: a launch of its own; LAB_NOTES R6.9)
    int train_fuse_bwd_tail = 1;          // training backward at batch size: FFN2 dgrad + GELU' + FFN1 dgrad + LayerNorm1 backward + out-proj dgrad as k_layer_tail_bwd
                                          // (MST_TRAIN_FUSE_BWD_TAIL: 0 = three dgrad launches, 1 = frozen stacks (no parameter gradients: the motion encoder), 2 = every stack)
    int train_small_ln = 1;               // training at a clip or two: the LayerNorms inside the GEMMs behind them (MST_TRAIN_SMALL_LN=0: k_ln_rows_train launches)
    int train_fuse_tail = 1;              // training forward at batch size: out-proj + LN1 + FFN + LN2 as k_layer_tail_train, writing the tape (MST_TRAIN_FUSE_TAIL=0: three ring GEMMs)
    int fuse_ln_bwd = 1;                  // training at batch size: LayerNorm1's backward in the epilogue of the dgrad GEMM in front of it (MST_FUSE_LN_BWD=0: two launches)
    int small_fast = 1;                   // small launches: the layer GEMMs as the kernels of mst_small.h (MST_SMALL_FAST=0: the slab ring)
    int fuse_embed = 1;                   // a sampling step's output projection also embeds the next step (MST_FUSE_EMBED=0: two launches)
    int embed_fast = 1;                   // K3 / K9 as the latency kernels of mst_embed.h; MST_EMBED_FAST=0: the ring GEMMs of rounds 1-3
    float *w_t0 = nullptr, *b_t0 = nullptr, *w_t2 = nullptr, *b_t2 = nullptr, *w_text = nullptr, *b_text = nullptr;
    float* pe = nullptr;
    // workspace
    f16* hl = nullptr;        // lo half of the stream (hx is the hi half)
    f16 *hx2 = nullptr, *hl2 = nullptr;   // second stream buffer: small launches with the LayerNorms inside the GEMMs (mst_small.h, LnRows)
    f16 *hx = nullptr, *qkv = nullptr, *att = nullptr, *hid = nullptr, *xt = nullptr;
    float* gelu_tab = nullptr;      // Phi(x) interpolation table of the fused layer tail's GELU stage (TailCfg::GELU_N entries {Phi, dPhi})
    f16* xt_lo = nullptr;     // lo half of the frame rows: the pose embedding multiplies x_t as hi + lo (RowsDirect::Xlo)
    float *temb_hid = nullptr, *temb = nullptr, *textproj = nullptr;
    int temb_cap = 0;
    // round 6: the timestep embedding of EVERY timestep (pe_len rows), built once per load of the (frozen) timestep MLP: a training call reads its
    // clips' rows through their timestep indices inside the embedding kernel instead of running the two-layer MLP on them first -- two dependent
    // launches less at the head of every model call, six of the seven per fine-tune iteration on the chained steps' critical path.  MST_TEMB_TABLE=0: off.
    float *temb_table = nullptr, *temb_table_hid = nullptr;
    bool temb_table_valid = false;
    int temb_table_on = 1;
    std::vector<std::string> loaded;
    std::set<std::string> lo_missing;     // GEMM weights uploaded while precise mode was off: their lo halves f16(w - f16(w)) were not written
                                          // (a fine-tune iteration re-uploads all 96 tensors and never reads them); precise mode refuses to run on those
    int text_batch = 0, text_cfg = 0;
    TrainWS tw;
    int dbg_layer = -1, dbg_stage = -1;   // stop the trunk after (layer, stage); -1 = run everything
    int fuse_qkv_attn = 1;                // K4 + K5 as one kernel per (clip, head); MST_FUSE_QKV_ATTN=0 keeps them apart
    int fuse_tail = 1;                    // K6 + K7 + K8 as one kernel per 64-token tile (mst_tail.h); MST_FUSE_TAIL=0 keeps them apart
    int tail_ntb = 0;                     // fused layer tail: 16-token blocks per tile; 0 = per launch (plan_trunk), MST_TAIL_NTB=2..4 fixes it
    int trunk_groups = 0;                 // MST_TRUNK=1: the encoder stack of a sampling step as ONE launch of resident workgroup groups (mst_trunk.h)
    unsigned* trunk_cnt = nullptr;        // [max_rows][32]: a clip's arrival counter (one 128-byte line each); every launch finds it at 0 and leaves it at 0
    unsigned* trunk_err = nullptr;        // pinned host word the kernel sets when a bounded spin gives up (mst_trunk_check)
    bool trunk_used = false;              // a resident-group launch was enqueued since the last check: mst_forward / mst_sample_loop synchronise and read trunk_err
    void* trunk_layers = nullptr;         // TrunkLayer[num_layers] in device memory: the layers' pointers (fixed at creation), uploaded at the first such launch
    int fuse_frames = 1;                  // sampling loop: a step's epilogue writes the next step's f16 frame rows; MST_FUSE_FRAMES=0 runs k_frames_f16 every step
    int precise = 0;                      // mst_set_precise / MST_PRECISE=1: every layer GEMM of the sampling path multiplies its activation as hi + lo (the small-tile
                                          // kernels at any size, ~2x their MFMA work): for checkpoints whose outlier channels put f16 operands above the 1e-3 bar
    int small_m = 1900;                   // launches of at most this many token rows take the small-tile path (MST_SMALL_M, 0 = never).
                                          // Round 4, with 32-token tiles in the fused tail of a lone launch (tools/experiments/r4_batch_sweep.sh, clips/s of a
                                          // 200-step loop, small / large tiles): 4 clips 46.2 / 41.0, 8: 85.6 / 83.2, 12: 105.8 / 125.1, 16: 139.2 / 167.5
                                          // -- hand-over between 9 and 10 clips (it was 16 clips = 3200 rows with 64-token tiles only)
    float* zacc = nullptr;                // fp32 GEMM result feeding k_ln_rows on that path
    int ln128_min_m = 1 << 30;            // MST_LN128_M=n: launches of >= n token rows use 128-token LayerNorm tiles (half the weight
                                          // re-streaming).  Off by default: wins 16-21 % in gemm_bench, nothing in the pipeline (CFG 39.7 vs
                                          // 39.9, batch 128 77.2 vs 77.1 clips/s; forced at batch 64: 58.7 vs 68.3) -- kept, parity-tested
    int wgrad_stream_on = 1;              // training: wgrads on a second stream beside the dgrad chain (MST_WGRAD_STREAM=0: one stream)
    int nsplit = 0;                       // clip slices of a sampling loop on separate streams: 0 = chosen per call (plan_slices), 1..3 = MST_STREAMS
    static constexpr int MAX_SLICES = 8;
    hipStream_t aux_stream[MAX_SLICES - 1] = {nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[MAX_SLICES - 1] = {nullptr};
    // sampling-loop state in device memory + the captured step graph (mst_sample_loop)
    LoopDev* ld_dev = nullptr;
    unsigned char* rowflag = nullptr;     // [max_rows][feats] summary of the loop's inpainting mask (k_mask_rowflags)
    float* plms_out = nullptr;            // [max_rows][feats][max_frames] model output of the PLMS warm-up's two evaluations (first PLMS chain allocates it)
    LoopDev* ld_pin = nullptr;            // pinned staging ring for the per-call upload
    static constexpr int LD_SLOTS = 8;
    hipEvent_t ld_ev[LD_SLOTS] = {nullptr};
    int ld_next = 0;
    int graph_on = 0;                     // MST_GRAPH=1: long loops replay a captured hipGraph of graph_steps steps (host enqueue ~0).
                                          // Off by default: on ROCm 7.2 the replay is not faster than host-enqueued launches
                                          // (same box, batch 64: 73.7 vs 74.1 clips/s; batch 1: 381 vs 367 us per step) -- the loop
                                          // is GPU-bound either way (tools/host_bound.py)
    int graph_steps = 20;                 // denoise steps per captured graph (MST_GRAPH_STEPS)
    hipStream_t loop_stream = nullptr;    // the loop runs on the engine's own streams (a caller's legacy default stream cannot be
    hipEvent_t ev_in = nullptr, ev_out = nullptr;   //  captured); it is ordered behind / before the caller's stream by these two events
    hipGraphExec_t gexec = nullptr;
    std::vector<long long> gkey;          // what the instantiated graph was captured for
    std::vector<long long> warm_key;      // configuration whose kernels have all been launched eagerly once (per-kernel LDS opt-ins done)
    // profiling
    int prof_on = 0, prof_now = 0, prof_period = 16;
    std::vector<ProfPoint> prof_pts;
    size_t prof_used = 0;
    float prof_overhead_us = -1.f;        // median duration an empty event pair reports (calibrated at mst_profile_enable)
    double prof_ms[FAM_COUNT] = {0};
    int prof_n[FAM_COUNT] = {0};
    // several styles (mst_style.h): slot 0 is L[]; slots 1 .. nslots - 1 hold only what sampling reads
    int nslots = 1;
    std::vector<LayerW> slot_w;           // [(slot - 1) * 16 + layer]
    std::vector<char> slot_loaded;        // [slot]: mst_load_layers_slot has filled it (slot 0: mst_weights_complete decides)
    StyleLayer* style_tab = nullptr;      // [nslots][num_layers] in device memory (pointers fixed when the slots are made)
    f16* style_stage = nullptr;           // one layer's plain f16 matrices: mst_load_layers_slot converts into it, then packs
    std::vector<int> styles;              // slot of every clip of the batch mst_set_styles named (empty: off)
    int style_xcd = 1;                    // segments and clips ordered so that one style's workgroups share XCDs (MST_STYLE_XCD=0: plain order;
                                          // same box, 8 styles x 8 HumanML clips: 87.6 against 85.0 clips/s, profiles/style_bank_bench.txt)
    int* plan_dev = nullptr;              // this call's tables (row slots, clip order, segments), ONE upload per call
    size_t plan_cap = 0;
    std::vector<int> plan_host;
    hipEvent_t plan_ev = nullptr;         // recorded behind the upload: plan_host is not rewritten before the copy has read it
    StyleSlice plan_sl[MAX_SLICES];
};

template <class T>
static int dmalloc(T** p, size_t count) {
    HIPCHECK(hipMalloc((void**)p, count * sizeof(T)));
    HIPCHECK(hipMemset(*p, 0, count * sizeof(T)));
    return 0;
}

// ------------------------------------------------------------------------------------------ schedule
extern "C" int mst_schedule_create(int32_t num_steps, const float* tables_host, const int32_t* timestep_map_host,
                                   int32_t device, mst_schedule** out) {
    if (!out || !tables_host || !timestep_map_host || num_steps <= 0) return fail("mst_schedule_create: bad arguments");
    ON_DEVICE(device);
    mst_schedule* s = new mst_schedule();
    s->n = num_steps;
    s->device = device;
    HIPCHECK(hipMalloc((void**)&s->tab, sizeof(float) * NTAB * num_steps));
    HIPCHECK(hipMalloc((void**)&s->tmap, sizeof(long long) * num_steps));
    HIPCHECK(hipMemcpy(s->tab, tables_host, sizeof(float) * NTAB * num_steps, hipMemcpyHostToDevice));
    std::vector<long long> tm(num_steps);
    for (int i = 0; i < num_steps; i++) tm[i] = timestep_map_host[i];
    HIPCHECK(hipMemcpy(s->tmap, tm.data(), sizeof(long long) * num_steps, hipMemcpyHostToDevice));
    *out = s;
    return 0;
}

extern "C" int mst_schedule_set_variance(mst_schedule* s, const float* variance_host) {
    if (!s || !variance_host) return fail("mst_schedule_set_variance: null argument");
    ON_DEVICE(s->device);
    if (!s->var) HIPCHECK(hipMalloc((void**)&s->var, sizeof(float) * s->n));
    HIPCHECK(hipMemcpy(s->var, variance_host, sizeof(float) * s->n, hipMemcpyHostToDevice));
    return 0;
}

extern "C" void mst_schedule_destroy(mst_schedule* s) {
    if (!s) return;
    (void)hipFree(s->var);
    (void)hipFree(s->tab);
    (void)hipFree(s->tmap);
    delete s;
}

// ------------------------------------------------------------------------------------------ engine
extern "C" int mst_engine_create(const mst_config* c, mst_engine** out) {
    if (!c || !out) return fail("mst_engine_create: null argument");
    if (c->latent_dim != MST_D || c->num_heads != MST_H || c->ff_size != MST_FF)
        return fail("mst_engine_create: kernels are built for latent_dim 512 / 4 heads / ff 1024 (got %d/%d/%d)",
                    c->latent_dim, c->num_heads, c->ff_size);
    if (c->num_layers < 1 || c->num_layers > 16) return fail("mst_engine_create: num_layers must be 1..16");
    if (c->feats < 1 || c->feats > 512) return fail("mst_engine_create: feats must be 1..512 (got %d)", c->feats);
    if (c->max_frames < 1 || c->max_frames > 223) return fail("mst_engine_create: max_frames must be 1..223 (got %d)", c->max_frames);
    if (c->max_rows < 1) return fail("mst_engine_create: max_rows must be >= 1");
    if (c->clip_dim < 1 || c->pe_len < c->max_frames + 1) return fail("mst_engine_create: bad clip_dim / pe_len");
    ON_DEVICE(c->device);
    mst_engine* e = new mst_engine();
    e->cfg = *c;
    e->S_max = c->max_frames + 1;
    size_t M = (size_t)c->max_rows * e->S_max;
    // rows of every token-row buffer: whole 256-row tiles plus one spare tile -- a slice starts at an arbitrary row and
    // its last tile may over-READ up to a tile beyond the slice (never write)
    e->M_pad = (int)(((M + 255) / 256) * 256) + 256;
    e->kin_pad = embed_kin_pad(c->feats);               // K of the pose-embedding GEMM (mst_plan.h)
    e->nt_out = (c->feats + 255) / 256;              // output-projection tile = 256 * nt_out features
    e->fout_pad = e->nt_out * 256;
    for (int l = 0; l < c->num_layers; l++) {
        LayerW& w = e->L[l];
        CHECK(dmalloc(&w.w_in, (size_t)3 * MST_D * MST_D));
        CHECK(dmalloc(&w.w_out, (size_t)MST_D * MST_D));
        CHECK(dmalloc(&w.w1, (size_t)MST_FF * MST_D));
        CHECK(dmalloc(&w.w2, (size_t)MST_D * MST_FF));
        CHECK(dmalloc(&w.b_in, 3 * MST_D));
        CHECK(dmalloc(&w.b_out, MST_D));
        CHECK(dmalloc(&w.b1, MST_FF));
        CHECK(dmalloc(&w.b2, MST_D));
        CHECK(dmalloc(&w.g1, MST_D));
        CHECK(dmalloc(&w.be1, MST_D));
        CHECK(dmalloc(&w.g2, MST_D));
        CHECK(dmalloc(&w.be2, MST_D));
        CHECK(dmalloc(&w.w_inT, (size_t)3 * MST_D * MST_D));
        CHECK(dmalloc(&w.w_outT, (size_t)MST_D * MST_D));
        CHECK(dmalloc(&w.w1T, (size_t)MST_FF * MST_D));
        CHECK(dmalloc(&w.w2T, (size_t)MST_D * MST_FF));
        CHECK(dmalloc(&w.wtail, TailCfg::LAYER_BYTES / 2));
        CHECK(dmalloc(&w.wqkv, (size_t)3 * MST_D * MST_D));
        CHECK(dmalloc(&w.wsm_in, (size_t)3 * MST_D * MST_D));
        CHECK(dmalloc(&w.wsm_out, (size_t)MST_D * MST_D));
        CHECK(dmalloc(&w.wsm_1, (size_t)MST_FF * MST_D));
        CHECK(dmalloc(&w.wsm_2, (size_t)MST_D * MST_FF));
        CHECK(dmalloc(&w.w_in_lo, (size_t)3 * MST_D * MST_D));
        CHECK(dmalloc(&w.w_out_lo, (size_t)MST_D * MST_D));
        CHECK(dmalloc(&w.w1_lo, (size_t)MST_FF * MST_D));
        CHECK(dmalloc(&w.w2_lo, (size_t)MST_D * MST_FF));
    }
    CHECK(dmalloc(&e->w_pose_in, (size_t)MST_D * e->kin_pad));
    CHECK(dmalloc(&e->w_pose_in_lo, (size_t)MST_D * e->kin_pad));
    CHECK(dmalloc(&e->w_pose_out_lo, (size_t)e->fout_pad * MST_D));
    CHECK(dmalloc(&e->b_pose_in, MST_D));
    CHECK(dmalloc(&e->w_pose_in_pk, (size_t)8 * 16 * 4 * 512));
    CHECK(dmalloc(&e->w_pose_out_pk, (size_t)8 * 16 * 4 * 512));
    CHECK(dmalloc(&e->w_pose_out, (size_t)e->fout_pad * MST_D));
    CHECK(dmalloc(&e->b_pose_out, e->fout_pad));
    CHECK(dmalloc(&e->w_pose_inT, (size_t)e->fout_pad * MST_D));
    CHECK(dmalloc(&e->w_pose_outT, (size_t)MST_D * e->kin_pad));
    CHECK(dmalloc(&e->w_t0, (size_t)MST_D * MST_D));
    CHECK(dmalloc(&e->b_t0, MST_D));
    CHECK(dmalloc(&e->w_t2, (size_t)MST_D * MST_D));
    CHECK(dmalloc(&e->b_t2, MST_D));
    CHECK(dmalloc(&e->w_text, (size_t)MST_D * c->clip_dim));
    CHECK(dmalloc(&e->b_text, MST_D));
    CHECK(dmalloc(&e->pe, (size_t)c->pe_len * MST_D));
    CHECK(dmalloc(&e->hl, (size_t)e->M_pad * MST_D));
    CHECK(dmalloc(&e->hx, (size_t)e->M_pad * MST_D));
    CHECK(dmalloc(&e->hx2, (size_t)e->M_pad * MST_D));
    CHECK(dmalloc(&e->hl2, (size_t)e->M_pad * MST_D));
    CHECK(dmalloc(&e->qkv, (size_t)e->M_pad * 3 * MST_D));
    CHECK(dmalloc(&e->att, (size_t)e->M_pad * MST_D));
    CHECK(dmalloc(&e->hid, (size_t)e->M_pad * MST_FF));
    CHECK(dmalloc(&e->xt, ((size_t)c->max_rows * c->max_frames + 128) * e->kin_pad));
    CHECK(dmalloc(&e->xt_lo, ((size_t)c->max_rows * c->max_frames + 128) * e->kin_pad));
    {   // Phi in double on the host: entry i = {Phi(x_i), Phi(x_i+1) - Phi(x_i)}, x_i = -6 + i / 128
        std::vector<float> tab(TailCfg::GELU_TAB_BYTES / 4, 0.f);
        auto phi = [](double x) { return 0.5 * std::erfc(-x * 0.70710678118654752440); };
        for (int i = 0; i <= TailCfg::GELU_N; i++) {
            const double x0 = -6.0 + i / 128.0, p0 = phi(x0), p1 = phi(x0 + 1.0 / 128.0);
            tab[2 * i] = (float)p0;
            tab[2 * i + 1] = (float)(p1 - p0);
        }
        CHECK(dmalloc(&e->gelu_tab, tab.size()));
        HIPCHECK(hipMemcpy(e->gelu_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    }
    e->temb_cap = c->max_rows > 1024 ? c->max_rows : 1024;
    CHECK(dmalloc(&e->temb_hid, (size_t)e->temb_cap * MST_D));
    CHECK(dmalloc(&e->temb, (size_t)e->temb_cap * MST_D));
    CHECK(dmalloc(&e->textproj, (size_t)c->max_rows * MST_D));
    HIPCHECK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < mst_engine::MAX_SLICES - 1; i++) {
        HIPCHECK(hipStreamCreateWithFlags(&e->aux_stream[i], hipStreamNonBlocking));
        HIPCHECK(hipEventCreateWithFlags(&e->ev_join[i], hipEventDisableTiming));
    }
    if (const char* v = getenv("MST_STREAMS")) {
        // At most three concurrent slices: ROCm maps streams onto four hardware queues by default and the caller's stream holds
        // one, so a fourth slice stream shares a queue with another and the two serialise (measured: 77.1 clips/s at 3, 40.9 at 4).
        int n = atoi(v);
        e->nsplit = n < 1 ? 1 : (n > mst_engine::MAX_SLICES ? mst_engine::MAX_SLICES : n);
    }
    if (const char* v = getenv("MST_FUSE_QKV_ATTN")) e->fuse_qkv_attn = atoi(v);
    if (const char* v = getenv("MST_FUSE_TAIL")) e->fuse_tail = atoi(v) != 0;
    if (const char* v = getenv("MST_FUSE_FRAMES")) e->fuse_frames = atoi(v) != 0;
    if (const char* v = getenv("MST_EMBED_FAST")) e->embed_fast = atoi(v) != 0;
    if (const char* v = getenv("MST_FUSE_EMBED")) e->fuse_embed = atoi(v) != 0;
    if (const char* v = getenv("MST_SMALL_FAST")) e->small_fast = atoi(v) != 0;
    if (const char* v = getenv("MST_FUSE_LN_BWD")) e->fuse_ln_bwd = atoi(v) != 0;
    if (const char* v = getenv("MST_TRAIN_FUSE_TAIL")) e->train_fuse_tail = atoi(v) != 0;
    if (const char* v = getenv("MST_TRAIN_SMALL_LN")) e->train_small_ln = atoi(v) != 0;
    if (const char* v = getenv("MST_TRAIN_FUSE_BWD_TAIL")) e->train_fuse_bwd_tail = atoi(v);
    if (const char* v = getenv("MST_TRAIN_FUSE_LN2_BWD")) e->train_fuse_ln2_bwd = atoi(v);
    if (const char* v = getenv("MST_TEMB_TABLE")) e->temb_table_on = atoi(v);
    if (const char* v = getenv("MST_SMALL_LN")) e->small_ln = atoi(v) != 0;
    if (const char* v = getenv("MST_SMALL_LN_M")) e->small_ln_m = atoi(v);
    if (const char* v = getenv("MST_TAIL_NTB")) { int n = atoi(v); e->tail_ntb = (n >= 2 && n <= 4) ? n : 0; }
    if (const char* v = getenv("MST_WGRAD_STREAM")) e->wgrad_stream_on = atoi(v) != 0;
    if (const char* v = getenv("MST_SMALL_M")) e->small_m = atoi(v);
    if (const char* v = getenv("MST_PRECISE")) e->precise = atoi(v) != 0;
    if (const char* v = getenv("MST_LN128_M")) e->ln128_min_m = atoi(v);
    if (const char* v = getenv("MST_TRUNK")) e->trunk_groups = atoi(v) != 0;
    if (const char* v = getenv("MST_STYLE_XCD")) e->style_xcd = atoi(v) != 0;
    CHECK(dmalloc(&e->trunk_cnt, (size_t)c->max_rows * 32));
    HIPCHECK(hipHostMalloc((void**)&e->trunk_err, 64, hipHostMallocDefault));
    e->trunk_err[0] = 0;
    CHECK(dmalloc(&e->zacc, (size_t)e->M_pad * MST_D));
    CHECK(dmalloc(&e->ld_dev, 1));
    CHECK(dmalloc(&e->rowflag, (size_t)c->max_rows * c->feats));
    HIPCHECK(hipStreamCreateWithFlags(&e->loop_stream, hipStreamNonBlocking));
    HIPCHECK(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
    HIPCHECK(hipEventCreateWithFlags(&e->ev_out, hipEventDisableTiming));
    HIPCHECK(hipHostMalloc((void**)&e->ld_pin, sizeof(LoopDev) * mst_engine::LD_SLOTS, hipHostMallocDefault));
    for (int i = 0; i < mst_engine::LD_SLOTS; i++) HIPCHECK(hipEventCreateWithFlags(&e->ld_ev[i], hipEventDisableTiming));
    if (const char* v = getenv("MST_GRAPH")) e->graph_on = atoi(v) != 0;
    if (const char* v = getenv("MST_GRAPH_STEPS")) { int n = atoi(v); e->graph_steps = n < 2 ? 2 : (n > 100 ? 100 : n); }
    *out = e;
    return 0;
}

extern "C" void mst_engine_destroy(mst_engine* e) {
    if (!e) return;
    for (int l = 0; l < e->cfg.num_layers; l++) {
        LayerW& w = e->L[l];
        void* p[] = {w.w_in, w.w_out, w.w1, w.w2, w.b_in, w.b_out, w.b1, w.b2, w.g1, w.be1, w.g2, w.be2,
                     w.w_inT, w.w_outT, w.w1T, w.w2T, w.wtail, w.wtail_bwd, w.wqkv, w.w_in_lo, w.w_out_lo, w.w1_lo, w.w2_lo, w.wsm_in, w.wsm_out, w.wsm_1, w.wsm_2};
        for (void* q : p) (void)hipFree(q);
    }
    {
        TrainWS& t = e->tw;
        void* p[] = {t.g0, t.g1, t.dbr2[0], t.dbr2[1], t.dbr1[0], t.dbr1[1], t.dpre[0], t.dpre[1], t.dqkv[0], t.dqkv[1],
                     t.datt, t.part, t.zeros, t.gscale, t.amax, t.ln_part, t.cs_part, t.hidr[0], t.hidr[1], t.ln_part2};
        if (t.ev_ready) (void)hipEventDestroy(t.ev_ready);
        for (int i = 0; i < 16; i++) if (t.ev_layer[i]) (void)hipEventDestroy(t.ev_layer[i]);
        for (int i = 0; i < 2; i++) if (t.ev_side[i]) (void)hipEventDestroy(t.ev_side[i]);
        for (void* q : p) (void)hipFree(q);
    }
    void* p[] = {e->w_pose_in_pk, e->w_pose_out_pk, e->w_pose_in_lo, e->w_pose_out_lo, e->w_pose_in, e->b_pose_in, e->w_pose_out, e->b_pose_out, e->w_pose_inT, e->w_pose_outT, e->w_t0, e->b_t0, e->w_t2, e->b_t2,
                 e->w_text, e->b_text, e->pe, e->hl, e->hx, e->hx2, e->hl2, e->qkv, e->att, e->hid, e->xt, e->xt_lo, e->gelu_tab, e->temb_hid, e->temb, e->textproj, e->zacc, e->temb_table, e->temb_table_hid};
    for (void* q : p) (void)hipFree(q);
    for (int i = 0; i < mst_engine::MAX_SLICES - 1; i++) {
        if (e->aux_stream[i]) (void)hipStreamDestroy(e->aux_stream[i]);
        if (e->ev_join[i]) (void)hipEventDestroy(e->ev_join[i]);
    }
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->trunk_cnt) (void)hipFree(e->trunk_cnt);
    if (e->trunk_layers) (void)hipFree(e->trunk_layers);
    if (e->trunk_err) (void)hipHostFree(e->trunk_err);
    if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
    if (e->loop_stream) (void)hipStreamDestroy(e->loop_stream);
    if (e->ev_in) (void)hipEventDestroy(e->ev_in);
    if (e->ev_out) (void)hipEventDestroy(e->ev_out);
    (void)hipFree(e->ld_dev);
    (void)hipFree(e->rowflag);
    (void)hipFree(e->plms_out);
    if (e->ld_pin) (void)hipHostFree(e->ld_pin);
    for (LayerW& w : e->slot_w) {
        void* q[] = {w.b_in, w.b_out, w.b1, w.b2, w.g1, w.be1, w.g2, w.be2, w.wtail, w.wqkv, w.wsm_in, w.wsm_out, w.wsm_1, w.wsm_2};
        for (void* x : q) (void)hipFree(x);
    }
    (void)hipFree(e->style_tab);
    (void)hipFree(e->style_stage);
    (void)hipFree(e->plan_dev);
    if (e->plan_ev) (void)hipEventDestroy(e->plan_ev);
    for (int i = 0; i < mst_engine::LD_SLOTS; i++) if (e->ld_ev[i]) (void)hipEventDestroy(e->ld_ev[i]);
    for (auto& pp : e->prof_pts) {
        (void)hipEventDestroy(pp.a);
        (void)hipEventDestroy(pp.b);
    }
    delete e;
}

// ------------------------------------------------------------------------------------------ weights
static int put_matrix(const float* src, int N, int K, f16* dst, int Npad, int Kpad, hipStream_t st, f16* dst_lo = nullptr) {
    hipLaunchKernelGGL(k_convert_pad, dim3(1024), dim3(256), 0, st, src, N, K, dst, Npad, Kpad, dst_lo);
    HIPCHECK(hipGetLastError());
    return 0;
}
static int put_matrix_t(const float* src, int N, int K, f16* dst, hipStream_t st) {      // [N][K] f32 -> [K][N] f16
    hipLaunchKernelGGL(k_convert_transpose, dim3((K + 31) / 32, (N + 31) / 32), dim3(256), 0, st, src, N, K, dst, N);
    HIPCHECK(hipGetLastError());
    return 0;
}
static int put_vector(const float* src, int n, float* dst, int npad, hipStream_t st) {
    hipLaunchKernelGGL(k_copy_pad_f32, dim3((npad + 255) / 256), dim3(256), 0, st, src, n, dst, npad);
    HIPCHECK(hipGetLastError());
    return 0;
}
static bool shape_is(const int64_t* s, int nd, int64_t a, int64_t b = -1) {
    if (b < 0) return nd == 1 && s[0] == a;
    return nd == 2 && s[0] == a && s[1] == b;
}

extern "C" int mst_load_weight(mst_engine* e, const char* name, const float* src, const int64_t* shape, int32_t ndim,
                               void* stream) {
    if (!e || !name || !src || !shape) return fail("mst_load_weight: null argument");
    hipStream_t st = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    const int F = e->cfg.feats, C = e->cfg.clip_dim;
    std::string n(name);
    int rc = -1;
    int layer = -1;
    char rest[128] = "";
    if (sscanf(name, "seqTransEncoder.layers.%d.%127s", &layer, rest) == 2) {
        if (layer < 0 || layer >= e->cfg.num_layers) return fail("mst_load_weight: layer %d out of range", layer);
        LayerW& w = e->L[layer];
        std::string r(rest);
#define MAT(key, N_, K_, dst) if (r == key) { if (!shape_is(shape, ndim, N_, K_)) return fail("mst_load_weight: %s: bad shape", name); rc = put_matrix(src, N_, K_, dst, N_, K_, st, e->precise ? dst##_lo : nullptr); if (!rc) rc = put_matrix_t(src, N_, K_, dst##T, st); repack = dst != w.w_in; is_gemm_w = true; }
        bool repack = false, is_gemm_w = false;
#define VEC(key, N_, dst) if (r == key) { if (!shape_is(shape, ndim, N_)) return fail("mst_load_weight: %s: bad shape", name); rc = put_vector(src, N_, dst, N_, st); }
        MAT("self_attn.in_proj_weight", 3 * MST_D, MST_D, w.w_in)
        VEC("self_attn.in_proj_bias", 3 * MST_D, w.b_in)
        MAT("self_attn.out_proj.weight", MST_D, MST_D, w.w_out)
        VEC("self_attn.out_proj.bias", MST_D, w.b_out)
        MAT("linear1.weight", MST_FF, MST_D, w.w1)
        VEC("linear1.bias", MST_FF, w.b1)
        MAT("linear2.weight", MST_D, MST_FF, w.w2)
        VEC("linear2.bias", MST_D, w.b2)
        VEC("norm1.weight", MST_D, w.g1)
        VEC("norm1.bias", MST_D, w.be1)
        VEC("norm2.weight", MST_D, w.g2)
        VEC("norm2.bias", MST_D, w.be2)
#undef MAT
#undef VEC
        // The fused kernels' packed copies (k_pack_qkv, k_pack_tail) are made once per re-upload and layer, and only if a sampling launch
        // follows (ensure_packed): a fine-tune iteration re-uploads all 96 tensors and its training node reads the plain matrices.
        if (rc == 0 && r == "self_attn.in_proj_weight") w.qkv_dirty = true;
        if (rc == 0 && repack) w.tail_dirty = w.tailb_dirty = true;
        if (rc == 0 && is_gemm_w) w.small_dirty = true;
        if (rc == 0 && is_gemm_w) { if (e->precise) e->lo_missing.erase(n); else e->lo_missing.insert(n); }
    } else if (n == "input_process.poseEmbedding.weight") {
        if (!shape_is(shape, ndim, MST_D, F)) return fail("mst_load_weight: %s: bad shape", name);
        rc = put_matrix(src, MST_D, F, e->w_pose_in, MST_D, e->kin_pad, st, e->precise ? e->w_pose_in_lo : nullptr);
        if (!rc) { if (e->precise) e->lo_missing.erase(n); else e->lo_missing.insert(n); e->pose_in_dirty = true; }
        if (!rc) {      // [512][F] -> [F (padded to fout_pad)][512]
            hipLaunchKernelGGL(k_convert_transpose, dim3((F + 31) / 32, (MST_D + 31) / 32), dim3(256), 0, st, src, MST_D, F, e->w_pose_inT, MST_D);
            HIPCHECK(hipGetLastError());
        }
    } else if (n == "input_process.poseEmbedding.bias") {
        if (!shape_is(shape, ndim, MST_D)) return fail("mst_load_weight: %s: bad shape", name);
        rc = put_vector(src, MST_D, e->b_pose_in, MST_D, st);
    } else if (n == "output_process.poseFinal.weight") {
        if (!shape_is(shape, ndim, F, MST_D)) return fail("mst_load_weight: %s: bad shape", name);
        rc = put_matrix(src, F, MST_D, e->w_pose_out, e->fout_pad, MST_D, st, e->precise ? e->w_pose_out_lo : nullptr);
        if (!rc) { if (e->precise) e->lo_missing.erase(n); else e->lo_missing.insert(n); e->pose_out_dirty = true; }
        if (!rc) {      // [F][512] -> [512][F (padded to kin_pad)]
            hipLaunchKernelGGL(k_convert_transpose, dim3((MST_D + 31) / 32, (F + 31) / 32), dim3(256), 0, st, src, F, MST_D, e->w_pose_outT, e->kin_pad);
            HIPCHECK(hipGetLastError());
        }
    } else if (n == "output_process.poseFinal.bias") {
        if (!shape_is(shape, ndim, F)) return fail("mst_load_weight: %s: bad shape", name);
        rc = put_vector(src, F, e->b_pose_out, e->fout_pad, st);
    } else if (n == "embed_timestep.time_embed.0.weight" || n == "embed_timestep.time_embed.2.weight") {
        if (!shape_is(shape, ndim, MST_D, MST_D)) return fail("mst_load_weight: %s: bad shape", name);
        rc = put_vector(src, MST_D * MST_D, n[26] == '0' ? e->w_t0 : e->w_t2, MST_D * MST_D, st);
        e->temb_table_valid = false;
    } else if (n == "embed_timestep.time_embed.0.bias" || n == "embed_timestep.time_embed.2.bias") {
        if (!shape_is(shape, ndim, MST_D)) return fail("mst_load_weight: %s: bad shape", name);
        rc = put_vector(src, MST_D, n[26] == '0' ? e->b_t0 : e->b_t2, MST_D, st);
        e->temb_table_valid = false;
    } else if (n == "embed_text.weight") {
        if (!shape_is(shape, ndim, MST_D, C)) return fail("mst_load_weight: %s: bad shape", name);
        rc = put_vector(src, MST_D * C, e->w_text, MST_D * C, st);
    } else if (n == "embed_text.bias") {
        if (!shape_is(shape, ndim, MST_D)) return fail("mst_load_weight: %s: bad shape", name);
        rc = put_vector(src, MST_D, e->b_text, MST_D, st);
    } else if (n == "sequence_pos_encoder.pe") {
        int64_t rows = ndim == 3 ? shape[0] : (ndim == 2 ? shape[0] : -1);
        int64_t cols = ndim == 3 ? shape[1] * shape[2] : (ndim == 2 ? shape[1] : -1);
        if (cols != MST_D || rows < e->cfg.pe_len) return fail("mst_load_weight: %s: bad shape", name);
        rc = put_vector(src, e->cfg.pe_len * MST_D, e->pe, e->cfg.pe_len * MST_D, st);
        e->temb_table_valid = false;
    }
    if (rc == -1) return fail("mst_load_weight: unknown tensor name '%s'", name);
    if (rc) return rc;
    bool seen = false;
    for (auto& s : e->loaded) seen |= (s == n);
    if (!seen) e->loaded.push_back(n);
    return 0;
}

// All 12 tensors of every encoder layer in one launch per 8 layers (k_upload_layers): what a fine-tune iteration does after every
// optimizer step.  srcs: num_layers x 12 device pointers in the order of mst_load_weight's layer list (in_proj_weight, in_proj_bias,
// out_proj.weight, out_proj.bias, linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm1.weight, norm1.bias, norm2.weight,
// norm2.bias).  Same results as 12 x num_layers mst_load_weight calls (precise mode: use those -- this entry writes no lo halves).
extern "C" int mst_load_layers(mst_engine* e, const float* const* srcs, void* stream) {
    if (!e || !srcs) return fail("mst_load_layers: null argument");
    if (e->precise) return fail("mst_load_layers: precise mode needs the weights' lo halves: upload with mst_load_weight");
    static_assert(MST_D == 512 && MST_FF == 1024, "k_upload_layers' tile map");
    static const char* kNames[12] = {"self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                                     "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias",
                                     "norm2.weight", "norm2.bias"};
    hipStream_t st = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    const int nl = e->cfg.num_layers;
    for (int i = 0; i < 12 * nl; i++) if (!srcs[i]) return fail("mst_load_layers: null tensor %d", i);
    for (int l0 = 0; l0 < nl; l0 += 8) {
        UpArgs a{};
        const int n = nl - l0 < 8 ? nl - l0 : 8;
        for (int j = 0; j < n; j++) {
            LayerW& w = e->L[l0 + j];
            UpLayer& u = a.L[j];
            for (int k = 0; k < 12; k++) u.src[k] = srcs[(l0 + j) * 12 + k];
            u.w[0] = w.w_in; u.w[1] = w.w_out; u.w[2] = w.w1; u.w[3] = w.w2;
            u.wT[0] = w.w_inT; u.wT[1] = w.w_outT; u.wT[2] = w.w1T; u.wT[3] = w.w2T;
            u.v[0] = w.b_in; u.v[1] = w.b_out; u.v[2] = w.b1; u.v[3] = w.b2; u.v[4] = w.g1; u.v[5] = w.be1; u.v[6] = w.g2; u.v[7] = w.be2;
        }
        hipLaunchKernelGGL(k_upload_layers, dim3(2049, n), dim3(256), 0, st, a);
        HIPCHECK(hipGetLastError());
    }
    for (int l = 0; l < nl; l++) {
        e->L[l].qkv_dirty = e->L[l].tail_dirty = e->L[l].tailb_dirty = e->L[l].small_dirty = true;
        for (int k = 0; k < 12; k++) {
            char name[160];
            snprintf(name, sizeof(name), "seqTransEncoder.layers.%d.%s", l, kNames[k]);
            std::string n(name);
            if ((k & 1) == 0 && k < 8) e->lo_missing.insert(n);
            bool seen = false;
            for (auto& s2 : e->loaded) seen |= (s2 == n);
            if (!seen) e->loaded.push_back(n);
        }
    }
    return 0;
}

extern "C" int mst_weights_complete(const mst_engine* e) {
    if (!e) return fail("mst_weights_complete: null engine");
    size_t want = (size_t)e->cfg.num_layers * 12 + 11;
    if (e->loaded.size() != want) return fail("mst_weights_complete: %zu of %zu tensors loaded", e->loaded.size(), want);
    return 0;
}

// ------------------------------------------------------------------------------------------ profiling
extern "C" int mst_profile_enable(mst_engine* e, int32_t on) {
    if (!e) return fail("mst_profile_enable: null engine");
    e->prof_on = on > 0 ? 1 : 0;          // on = N > 0: instrument every N-th step of a loop
    e->prof_period = on > 0 ? on : 16;
    if (e->prof_on && e->prof_pts.empty()) {
        e->prof_pts.resize(8192);
        for (auto& p : e->prof_pts) {
            HIPCHECK(hipEventCreate(&p.a));
            HIPCHECK(hipEventCreate(&p.b));
        }
    }
    e->prof_used = 0;
    for (int i = 0; i < FAM_COUNT; i++) { e->prof_ms[i] = 0; e->prof_n[i] = 0; }
    if (e->prof_on && e->prof_overhead_us < 0.f) {
        // what an event pair measures around NOTHING on an otherwise busy-free stream: the fixed part of every timed launch
        // (rocprofv3's kernel durations are shorter than event-bracketed ones by about this much)
        ON_DEVICE(e->cfg.device);
        float v[16];
        for (int i = 0; i < 16; i++) {
            HIPCHECK(hipEventRecord(e->prof_pts[0].a, e->loop_stream));
            HIPCHECK(hipEventRecord(e->prof_pts[0].b, e->loop_stream));
            HIPCHECK(hipEventSynchronize(e->prof_pts[0].b));
            HIPCHECK(hipEventElapsedTime(&v[i], e->prof_pts[0].a, e->prof_pts[0].b));
        }
        std::sort(v, v + 16);
        e->prof_overhead_us = 1e3f * v[8];
    }
    return 0;
}

extern "C" float mst_profile_event_overhead_us(const mst_engine* e) { return e ? e->prof_overhead_us : -1.f; }

extern "C" int mst_profile_read(mst_engine* e, const char** names, float* total_ms, int32_t* launches, int32_t cap) {
    if (!e) return -1;
    // caller has synchronised the stream
    for (size_t i = 0; i < e->prof_used; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e->prof_pts[i].a, e->prof_pts[i].b) == hipSuccess) {
            e->prof_ms[e->prof_pts[i].fam] += ms;
            e->prof_n[e->prof_pts[i].fam] += 1;
        }
    }
    e->prof_used = 0;
    int n = FAM_COUNT < cap ? FAM_COUNT : cap;
    for (int i = 0; i < n; i++) {
        names[i] = kFamilyNames[i];
        total_ms[i] = (float)e->prof_ms[i];
        launches[i] = e->prof_n[i];
    }
    return n;
}

struct ProfScope {
    mst_engine* e; hipStream_t st; ProfPoint* p = nullptr;
    ProfScope(mst_engine* e_, int fam, hipStream_t st_) : e(e_), st(st_) {
        if (e->prof_on && e->prof_now && e->prof_used < e->prof_pts.size()) {
            p = &e->prof_pts[e->prof_used++];
            p->fam = fam;
            (void)hipEventRecord(p->a, st);
        }
    }
    ~ProfScope() { if (p) (void)hipEventRecord(p->b, st); }
};

// ------------------------------------------------------------------------------------------ launches
template <int BT, int BF, int MT, int NT, int NS, int NX, int BK = 32, int XS = 1, class SRC, class EPI>
static int launch_gemm_dma(dim3 grid, const SRC& xs, const f16* W, int ldw, int K, const EPI& epi, hipStream_t st, int xcd_ny = 0) {
    using TL = DTile<BT, BF, MT, NT, NS, NX, BK, XS>;
    static_assert(EPI::template smem_bytes<BT, BF>() <= TL::SMEM, "epilogue tile must fit the ring");
    static_assert(TL::SMEM <= 163840, "ring exceeds the 160 KiB LDS");
    auto kern = k_gemm_dma<BT, BF, MT, NT, NS, NX, SRC, EPI, BK, XS>;
    if (XS == 2 && !xs.Xlo) return fail("gemm: the split-activation tile needs the lo tensor");
    CHECK(ensure_dyn_lds((const void*)kern, TL::SMEM));
    if (K < BK * (NS - 1) || (K % BK)) return fail("gemm: K=%d unsupported by the %d-slot ring", K, NS);
    hipLaunchKernelGGL(kern, grid, dim3(512), TL::SMEM, st, xs, W, ldw, K, xcd_ny, epi);
    HIPCHECK(hipGetLastError());
    return 0;
}

// Wide (128 x 256) GEMM launch.  Few token rows = few workgroups, each walking the whole K loop alone: the loop is then
// bound by the DMA round trip per slab, not by bandwidth, so small launches use 64-deep slabs (half as many round trips,
// one workgroup per CU is plenty); large launches keep 32-deep slabs and two co-resident workgroups per CU.
#define SMALL_M 2048
#define LN_BWD_WIDE_M 4096        // k_ln_bwd: sixteen waves per block above this many rows (four below: a clip or a few, one row per wave)
template <class SRC, class EPI>
static int launch_wide(int M, int ny, const SRC& xs, const f16* W, int ldw, int K, const EPI& epi, hipStream_t st) {
    if (M <= SMALL_M && (K % 64) == 0 && K >= 128)
        return launch_gemm_dma<WIDE_BT, 256, WIDE_BT / 64, 2, 3, 1, 64>(wide_grid(M, ny), xs, W, ldw, K, epi, st, WIDE_XCD ? ny : 0);
    return launch_gemm_dma<WIDE_BT, 256, WIDE_BT / 64, 2, WIDE_NS, 1>(wide_grid(M, ny), xs, W, ldw, K, epi, st, WIDE_XCD ? ny : 0);
}

// Few token rows (a clip or two): 64 x 128 tiles over a 2-D grid so that tens of workgroups share the weight matrix
// instead of 4-12 of them each streaming all of it; LayerNorm then runs as its own row-wise kernel (k_ln_rows).
template <class SRC, class EPI>
static int launch_small(int M, int N, const SRC& xs, const f16* W, int ldw, int K, const EPI& epi, hipStream_t st) {
    return launch_gemm_dma<64, 128, 1, 1, 3, 1, 64>(dim3((M + 63) / 64, N / 128), xs, W, ldw, K, epi, st, 0);
}

// The small-launch GEMMs of mst_small.h: 64 x 128 tiles, the token tile resident in LDS, the weights streamed as fragments.
static int g_rows_ntb1_m = [] { const char* v = getenv("MST_SMALL_NTB1_M"); return v ? atoi(v) : 800; }();
// (tools/experiments/r4_ntb1_sweep.sh, r4_ntb2_sweep.sh: 16-token tiles ahead through 4 clips x 197 rows, behind at 6; 32-token tiles 4 % ahead at 8 and 9 clips, level at 6, behind at 5)
static int g_rows_ntb2_from = [] { const char* v = getenv("MST_SMALL_NTB2_FROM"); return v ? atoi(v) : 1300; }();
template <int KS, int MODE>
static int launch_rows_gemm(int M, int N, const f16* X, const f16* wpk, const float* bias, void* out, int ldo, hipStream_t st, const LnRows* ln = nullptr,
                            const FfnTrain* ft = nullptr) {
    constexpr int smem = 64 * (KS / 16) * 1024;
#define ROWS_LAUNCH(LNF_, NTB_, ln_)                                                                                                       \
    hipLaunchKernelGGL((k_rows_gemm<KS, MODE, LNF_, NTB_>), dim3((M + 16 * NTB_ - 1) / (16 * NTB_), N / 128), dim3(512), smem * NTB_ / 4, st, X, \
                       wpk, bias, out, ldo, M, ln_, ft ? *ft : FfnTrain{})
    if (ln) {                                                      // the LayerNorm in front: 16-token tiles (mst_small.h)
        if constexpr (KS == 16 && (MODE == 0 || MODE == 1 || MODE == 3)) ROWS_LAUNCH(1, 1, *ln);
        else return fail("rows GEMM: no fused-LayerNorm instantiation for KS %d MODE %d", KS, MODE);
    } else switch (rows_ntb(M, g_rows_ntb1_m, g_rows_ntb2_from)) {
        case 1: ROWS_LAUNCH(0, 1, LnRows{}); break;
        case 2: ROWS_LAUNCH(0, 2, LnRows{}); break;
        default:
            CHECK(ensure_dyn_lds((const void*)k_rows_gemm<KS, MODE>, smem));
            ROWS_LAUNCH(0, 4, LnRows{});
    }
#undef ROWS_LAUNCH
    HIPCHECK(hipGetLastError());
    return 0;
}
template <int NKT>
static int launch_attn_n(const f16* qkv, f16* out, int S, int rows, hipStream_t st, int qsplit, f16* out_lo) {
    auto kern = k_attention<NKT>;
    const int smem = NKT * 32 * 256 * 2;
    CHECK(ensure_dyn_lds((const void*)kern, smem));
    hipLaunchKernelGGL(kern, dim3(rows * MST_H, qsplit ? NKT : 1), dim3(512), smem, st, qkv, out, S, qsplit, out_lo);
    HIPCHECK(hipGetLastError());
    return 0;
}

template <int NKT>
static int launch_qkv_attn_n(const f16* hx, const f16* w_in, const float* b_in, f16* out, int S, int rows, hipStream_t st) {
    auto kern = k_qkv_attention<NKT>;
    constexpr int smem = QATile<NKT>::SMEM;
    static_assert(smem <= 163840, "fused QKV+attention exceeds the 160 KiB LDS");
    CHECK(ensure_dyn_lds((const void*)kern, smem));
    hipLaunchKernelGGL(kern, dim3(rows * MST_H), dim3(512), smem, st, hx, w_in, b_in, out, S);
    HIPCHECK(hipGetLastError());
    return 0;
}

#define NKT_SWITCH(fn, S, ...)                                    \
    switch (((S) + 31) / 32) {                                    \
        case 1: return fn<1>(__VA_ARGS__);                        \
        case 2: return fn<2>(__VA_ARGS__);                        \
        case 3: return fn<3>(__VA_ARGS__);                        \
        case 4: return fn<4>(__VA_ARGS__);                        \
        case 5: return fn<5>(__VA_ARGS__);                        \
        case 6: return fn<6>(__VA_ARGS__);                        \
        case 7: return fn<7>(__VA_ARGS__);                        \
    }                                                             \
    return fail("attention: S=%d unsupported", S);
static int launch_qkv_attn(const f16* hx, const f16* w_in, const float* b_in, f16* out, int S, int rows, hipStream_t st) {
    NKT_SWITCH(launch_qkv_attn_n, S, hx, w_in, b_in, out, S, rows, st)
}

template <int NT16>
static int launch_qkv_attn2_n(const f16* hx, const f16* wq, const float* b_in, f16* out, int S, int rows, hipStream_t st) {
    auto kern = k_qkv_attention2<NT16>;
    constexpr int smem = QA2Tile<NT16>::SMEM;
    CHECK(ensure_dyn_lds((const void*)kern, smem));
    hipLaunchKernelGGL(kern, dim3(rows * MST_H), dim3(512), smem, st, hx, wq, b_in, out, S);
    HIPCHECK(hipGetLastError());
    return 0;
}
// nt16: TrunkPlan::nt16 (mst_plan.h), shared with the style-aware kernel
#define NT16_SWITCH(fn, nt16, S, ...)                             \
    switch (nt16) {                                               \
        case 2: return fn<2>(__VA_ARGS__);                        \
        case 4: return fn<4>(__VA_ARGS__);                        \
        case 6: return fn<6>(__VA_ARGS__);                        \
        case 8: return fn<8>(__VA_ARGS__);                        \
        case 10: return fn<10>(__VA_ARGS__);                      \
        case 12: return fn<12>(__VA_ARGS__);                      \
        case 13: return fn<13>(__VA_ARGS__);                      \
    }                                                             \
    return fail("attention: S=%d unsupported", S);
static int launch_qkv_attn2(const f16* hx, const f16* wq, const float* b_in, f16* out, int S, int rows, int nt16, hipStream_t st) {
    NT16_SWITCH(launch_qkv_attn2_n, nt16, S, hx, wq, b_in, out, S, rows, st)
}

static int launch_attn(const f16* qkv, f16* out, int S, int rows, hipStream_t st, int qsplit = 0, f16* out_lo = nullptr) {
    NKT_SWITCH(launch_attn_n, S, qkv, out, S, rows, st, qsplit, out_lo)
}

static int rowwise_linear(const float* in, int ldin, const long long* gather, const float* rowscale, int rows_zero_from,
                          const float* W, const float* b, int K, int N, int act, float* out, int in_row_mod, int rows,
                          hipStream_t st, int rowscale_is_drop = 0) {
    // a wave per output where the rows are few (64 rows x 128 = 8 K blocks; the hoisted timestep rows of a 1000-step loop keep 16 per row)
    const int gy = rows <= 64 ? (N + 3) / 4 : 16;
    hipLaunchKernelGGL(k_rowwise_linear, dim3(rows, gy), dim3(256), 0, st, in, ldin, gather, rowscale, rows_zero_from, W, b,
                       K, N, act, out, in_row_mod, rowscale_is_drop);
    HIPCHECK(hipGetLastError());
    return 0;
}

// the timestep embedding of every timestep there is (rows of the positional table), once per load of the timestep MLP
static int ensure_temb_table(mst_engine* e, hipStream_t st) {
    if (e->temb_table_valid) return 0;
    const int rows = e->cfg.pe_len;
    if (!e->temb_table) {
        CHECK(dmalloc(&e->temb_table, (size_t)rows * MST_D));
        CHECK(dmalloc(&e->temb_table_hid, (size_t)rows * MST_D));
    }
    CHECK(rowwise_linear(e->pe, MST_D, nullptr, nullptr, rows, e->w_t0, e->b_t0, MST_D, MST_D, 1, e->temb_table_hid, 0, rows, st));
    CHECK(rowwise_linear(e->temb_table_hid, MST_D, nullptr, nullptr, rows, e->w_t2, e->b_t2, MST_D, MST_D, 0, e->temb_table, 0, rows, st));
    e->temb_table_valid = true;
    return 0;
}

// timestep embedding rows: temb[j] = W2 silu(W0 pe[tidx[j]] + b0) + b2   (mdm :415-422)
static int timestep_rows(mst_engine* e, const long long* tidx_dev, int rows, hipStream_t st) {
    if (rows > e->temb_cap) return fail("timestep_rows: %d rows exceed capacity %d", rows, e->temb_cap);
    CHECK(rowwise_linear(e->pe, MST_D, tidx_dev, nullptr, rows, e->w_t0, e->b_t0, MST_D, MST_D, 1, e->temb_hid, 0, rows, st));
    CHECK(rowwise_linear(e->temb_hid, MST_D, nullptr, nullptr, rows, e->w_t2, e->b_t2, MST_D, MST_D, 0, e->temb, 0, rows, st));
    return 0;
}

extern "C" int mst_set_text(mst_engine* e, const float* text_emb, const float* keep, int32_t batch, int32_t cfg, void* stream) {
    if (!e || !text_emb) return fail("mst_set_text: null argument");
    int rows = cfg ? 2 * batch : batch;
    if (batch < 1 || rows > e->cfg.max_rows) return fail("mst_set_text: %d rows exceed max_rows %d", rows, e->cfg.max_rows);
    hipStream_t st = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    CHECK(rowwise_linear(text_emb, e->cfg.clip_dim, nullptr, keep, cfg ? batch : rows, e->w_text, e->b_text, e->cfg.clip_dim,
                         MST_D, 0, e->textproj, batch, rows, st));
    e->text_batch = batch;
    e->text_cfg = cfg ? 1 : 0;
    return 0;
}

extern "C" int mst_set_text_dropped(mst_engine* e, const float* text_emb, const float* drop, int32_t batch, void* stream) {
    if (!e || !text_emb || !drop) return fail("mst_set_text_dropped: null argument");
    if (batch < 1 || batch > e->cfg.max_rows) return fail("mst_set_text_dropped: %d rows exceed max_rows %d", batch, e->cfg.max_rows);
    hipStream_t st = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    CHECK(rowwise_linear(text_emb, e->cfg.clip_dim, nullptr, drop, batch, e->w_text, e->b_text, e->cfg.clip_dim, MST_D, 0, e->textproj, batch, batch, st, 1));
    e->text_batch = batch;
    e->text_cfg = 0;
    return 0;
}

// A slice of the workspace: clips [r0, r0 + n) of the batch get their own rows of every buffer, so slices can
// run concurrently on different streams (tiles may over-READ into a neighbour's rows; they never write them).
struct WS {
    f16 *hl, *hx, *qkv, *att, *hid, *xt; float* textproj; float* zacc; f16* xt_lo; f16 *hx2, *hl2;
};
static WS ws_slice(const mst_engine* e, int r0, int T) {
    const size_t row = (size_t)r0 * (T + 1);
    return WS{e->hl + row * MST_D, e->hx + row * MST_D, e->qkv + row * 3 * MST_D, e->att + row * MST_D, e->hid + row * MST_FF,
              e->xt + (size_t)r0 * T * e->kin_pad, e->textproj + (size_t)r0 * MST_D, e->zacc + row * MST_D,
              e->xt_lo + (size_t)r0 * T * e->kin_pad, e->hx2 + row * MST_D, e->hl2 + row * MST_D};
}

// Packed weight copies of the two fused kernels, refreshed where stale: on the stream the sampling launch is about to use (the caller
// orders that stream behind its weight uploads, as for the plain matrices).
static int embed_out_nbw(const mst_engine* e) { return embed_out_nbw(e->cfg.feats); }     // 16-feature blocks per wave of k_embed_out (mst_plan.h)
static_assert(EMBED_BT == EmbCfg::BT && EMBED_SMEM == EmbCfg::SMEM, "mst_plan.h plans the projections for mst_embed.h's tile and LDS budget");
// (layers = false: the training node's model calls -- they run the two projections' fast kernels but read the layers' plain matrices,
// and every fine-tune iteration re-uploads those: their packed copies are made only when a sampling launch follows)
// (on the stream every slice of a loop forks from: mst_sample_loop packs before the fork, so no slice reads fragments another stream is still writing)
static int ensure_small_packed(mst_engine* e, int l, hipStream_t st) {
    LayerW& w = e->L[l];
    if (!w.small_dirty) return 0;
    hipLaunchKernelGGL(k_pack_blocks, dim3(192), dim3(256), 0, st, w.w_in, MST_D, 3 * MST_D, MST_D, w.wsm_in);
    hipLaunchKernelGGL(k_pack_blocks, dim3(64), dim3(256), 0, st, w.w_out, MST_D, MST_D, MST_D, w.wsm_out);
    hipLaunchKernelGGL(k_pack_blocks, dim3(128), dim3(256), 0, st, w.w1, MST_D, MST_FF, MST_D, w.wsm_1);
    hipLaunchKernelGGL(k_pack_blocks, dim3(128), dim3(256), 0, st, w.w2, MST_FF, MST_D, MST_FF, w.wsm_2);
    HIPCHECK(hipGetLastError());
    w.small_dirty = false;
    return 0;
}

// every stale layer's four matrices in ONE launch (the fine-tune loop re-uploads all of them each iteration)
static int ensure_small_packed_all(mst_engine* e, hipStream_t st) {
    PackJobs jobs{};
    int n = 0;
    for (int l = 0; l < e->cfg.num_layers && l < 8; l++) {
        LayerW& w = e->L[l];
        if (!w.small_dirty) continue;
        jobs.j[n++] = PackJob{w.w_in, w.wsm_in, MST_D, 3 * MST_D, MST_D, 0};
        jobs.j[n++] = PackJob{w.w_out, w.wsm_out, MST_D, MST_D, MST_D, 0};
        jobs.j[n++] = PackJob{w.w1, w.wsm_1, MST_D, MST_FF, MST_D, 0};
        jobs.j[n++] = PackJob{w.w2, w.wsm_2, MST_FF, MST_D, MST_FF, 0};
    }
    if (n) {
        hipLaunchKernelGGL(k_pack_blocks_multi, dim3(48, n), dim3(256), 0, st, jobs);
        HIPCHECK(hipGetLastError());
        for (int l = 0; l < e->cfg.num_layers && l < 8; l++) e->L[l].small_dirty = false;
    }
    for (int l = 8; l < e->cfg.num_layers; l++) CHECK(ensure_small_packed(e, l, st));
    return 0;
}
static int ensure_packed(mst_engine* e, hipStream_t st, bool layers = true) {
    if (e->pose_in_dirty) {
        hipLaunchKernelGGL(k_pack_wave_blocks, dim3(256), dim3(256), 0, st, e->w_pose_in, e->kin_pad, MST_D, e->kin_pad / 32, 4, e->w_pose_in_pk);
        HIPCHECK(hipGetLastError());
        e->pose_in_dirty = false;
    }
    if (e->pose_out_dirty) {
        hipLaunchKernelGGL(k_pack_wave_blocks, dim3(256), dim3(256), 0, st, e->w_pose_out, MST_D, e->fout_pad, MST_D / 32, embed_out_nbw(e), e->w_pose_out_pk);
        HIPCHECK(hipGetLastError());
        e->pose_out_dirty = false;
    }
    if (!layers) return 0;
    for (int l = 0; l < e->cfg.num_layers; l++) {
        LayerW& w = e->L[l];
        if (w.qkv_dirty) {
            hipLaunchKernelGGL(k_pack_qkv, dim3(384), dim3(256), 0, st, w.w_in, w.wqkv);
            HIPCHECK(hipGetLastError());                  // a flag is cleared only behind a launch that was accepted
            w.qkv_dirty = false;
        }
        if (w.tail_dirty) {
            hipLaunchKernelGGL(k_pack_tail, dim3(640), dim3(256), 0, st, w.w_out, w.w1, w.w2, w.wtail);
            HIPCHECK(hipGetLastError());
            w.tail_dirty = false;
        }
    }
    if (e->small_fast && e->small_m > 0) CHECK(ensure_small_packed_all(e, st));
    return 0;
}

// K6 + K7 + K8 of one layer as one launch (mst_tail.h): one workgroup per tile of 16 ntb tokens (TrunkPlan::tail_ntb)
static int launch_tail(const mst_engine* e, const LayerW& w, const WS& ws, int M, int ntb, hipStream_t st) {
    static_assert(TailCfg::SMEM <= 163840, "fused layer tail exceeds the 160 KiB LDS");
    const int grid = (M + 16 * ntb - 1) / (16 * ntb);
#define TAIL_LAUNCH(N_)                                                                                                          \
    do {                                                                                                                         \
        CHECK(ensure_dyn_lds((const void*)k_layer_tail<N_>, TailCfg::SMEM));                                                     \
        hipLaunchKernelGGL(k_layer_tail<N_>, dim3(grid), dim3(512), TailCfg::SMEM, st, ws.att, w.wtail, w.b_out, w.g1, w.be1,     \
                           w.b1, w.b2, w.g2, w.be2, ws.hx, ws.hl, e->gelu_tab, M);                                               \
    } while (0)
    if (ntb == 2) TAIL_LAUNCH(2);
    else if (ntb == 3) TAIL_LAUNCH(3);
    else TAIL_LAUNCH(4);
#undef TAIL_LAUNCH
    HIPCHECK(hipGetLastError());
    return 0;
}

// The whole stack of a sampling step as one launch of resident groups (mst_trunk.h; PATH_RESIDENT in mst_plan.h)
static int launch_trunk_groups(mst_engine* e, const WS& ws, int S, int rows, hipStream_t st) {
    using TT = TrunkTile<13>;
    if (e->trunk_err[0]) return fail("resident-group trunk: a hand-off wait gave up in an earlier launch (results of that loop are invalid)");
    TrunkArgs a{};
    if (!e->trunk_layers) {
        TrunkLayer tab[8];
        for (int l = 0; l < e->cfg.num_layers; l++) {
            const LayerW& w = e->L[l];
            tab[l] = TrunkLayer{w.wqkv, w.b_in, w.wtail, w.b_out, w.g1, w.be1, w.b1, w.b2, w.g2, w.be2};
        }
        HIPCHECK(hipMalloc(&e->trunk_layers, sizeof(tab)));
        HIPCHECK(hipMemcpy(e->trunk_layers, tab, sizeof(tab), hipMemcpyHostToDevice));
    }
    a.L = static_cast<const TrunkLayer*>(e->trunk_layers);
    a.hx = ws.hx; a.hl = ws.hl; a.att = ws.att; a.gelu_tab = e->gelu_tab;
    a.cnt = e->trunk_cnt + (size_t)((ws.hx - e->hx) / ((size_t)S * MST_D)) * 32;       // the slice's first clip
    a.err = e->trunk_err;
    a.S = S; a.nclips = rows; a.nlayers = e->cfg.num_layers;
    const int groups = rows < 64 ? rows : 64;
    CHECK(ensure_dyn_lds((const void*)k_trunk_groups<13>, TT::SMEM));
    hipLaunchKernelGGL(k_trunk_groups<13>, dim3(4 * groups), dim3(512), TT::SMEM, st, a);
    HIPCHECK(hipGetLastError());
    e->trunk_used = true;
    return 0;
}
// The error word is written by the kernel when it RUNS; a loop enqueues hundreds of steps ahead, so reading it at enqueue time is always
// stale.  Every ABI call that may have used the resident launch therefore ends with a synchronisation of its stream and
// this check: a give-up (the four blocks of a group not co-resident -- the launch rests on in-order dispatch of at most 256 one-per-CU
// blocks, which another process or a busy foreign stream on the same GPU can break) is an ERROR of that call, never a wrong sample.
static int trunk_settle(mst_engine* e, hipStream_t st, int rc) {
    if (!e->trunk_used) return rc;
    e->trunk_used = false;
    if (hipStreamSynchronize(st) != hipSuccess) return rc ? rc : fail("resident-group trunk: synchronisation failed");
    if (e->trunk_err[0]) return fail("resident-group trunk: a hand-off wait gave up (groups not co-resident?); the results of this call are invalid -- "
                                     "mst_set_trunk_groups(e, 0) returns to one launch per kernel");
    return rc;
}
extern "C" int mst_trunk_check(mst_engine* e) {          // after a synchronisation: did every hand-off of the resident-group launches arrive?
    if (!e) return fail("mst_trunk_check: null engine");
    if (e->trunk_err[0]) return fail("resident-group trunk: a hand-off wait gave up");
    return 0;
}

// ------------------------------------------------------------------------------------------ several styles (csrc/mst_style.h)
static StyleLayer style_record(const LayerW& w) {
    return StyleLayer{w.wqkv, w.b_in, w.wtail, w.b_out, w.g1, w.be1, w.b1, w.b2, w.g2, w.be2, w.wsm_in, w.wsm_out, w.wsm_1, w.wsm_2};
}
static LayerW& slot_layer(mst_engine* e, int slot, int l) { return slot == 0 ? e->L[l] : e->slot_w[(size_t)(slot - 1) * 16 + l]; }

// Tile heights the stack's launches use (16 NTB rows): the segment tables exist for each of them.
static int style_h_index(int tile_rows) { return tile_rows / 16 - 1; }

static int plan_segments(const int* slot_of_row, int nrows, int S, int tile_rows, StyleSeg* out, int cap) {
    if (!slot_of_row || nrows < 1 || S < 1 || tile_rows < 1 || cap < 0) return -1;
    const int M = nrows * S;
    int n = 0;
    for (int t0 = 0; t0 < M; t0 += tile_rows) {
        const int t1 = t0 + tile_rows < M ? t0 + tile_rows : M;
        int lo = t0;
        while (lo < t1) {
            const int slot = slot_of_row[lo / S];
            int hi = (lo / S + 1) * S;                      // end of this clip
            while (hi < t1 && slot_of_row[hi / S] == slot) hi += S;
            if (hi > t1) hi = t1;
            if (n >= cap) return -1;
            out[n++] = StyleSeg{t0, lo, hi, slot};
            lo = hi;
        }
    }
    return n;
}

extern "C" int32_t mst_plan_style_segments(const int32_t* styles_host, int32_t nclips, int32_t S, int32_t tile_rows, int32_t* out, int32_t cap) {
    if (!styles_host || !out) return (void)fail("mst_plan_style_segments: null argument"), -1;
    if (nclips < 1 || S < 1 || tile_rows < 1 || cap < 0) return (void)fail("mst_plan_style_segments: bad sizes"), -1;
    const int n = plan_segments(styles_host, nclips, S, tile_rows, reinterpret_cast<StyleSeg*>(out), cap);
    if (n < 0) return (void)fail("mst_plan_style_segments: more than %d segments", cap), -1;
    return n;
}

// XCD-affine order: items sorted (stably) by slot fill the block positions of XCD 0 (x, x + 8, ...), then XCD 1, ... (round-robin
// dispatch: block b runs on XCD b % 8), so that one slot's workgroups share as few L2s as possible.  Returns order[position] = item.
static std::vector<int> xcd_order(const std::vector<int>& slot_of_item) {
    const int n = (int)slot_of_item.size();
    std::vector<int> sorted(n), order(n);
    for (int i = 0; i < n; i++) sorted[i] = i;
    std::stable_sort(sorted.begin(), sorted.end(), [&](int a, int b) { return slot_of_item[a] < slot_of_item[b]; });
    int k = 0;
    for (int x = 0; x < 8; x++)
        for (int p = x; p < n; p += 8) order[p] = sorted[k++];
    return order;
}

extern "C" int mst_style_slots(mst_engine* e, int32_t n) {
    if (!e) return fail("mst_style_slots: null engine");
    if (n < 1 || n > 64) return fail("mst_style_slots: %d slots (1..64)", n);
    if (n < e->nslots) return fail("mst_style_slots: the engine already has %d slots", e->nslots);
    ON_DEVICE(e->cfg.device);
    const int nl = e->cfg.num_layers;
    e->slot_w.resize((size_t)(n - 1) * 16);
    for (int s = e->nslots; s < n; s++) {
        for (int l = 0; l < nl; l++) {
            LayerW& w = slot_layer(e, s, l);
            CHECK(dmalloc(&w.b_in, 3 * MST_D));
            CHECK(dmalloc(&w.b_out, MST_D));
            CHECK(dmalloc(&w.b1, MST_FF));
            CHECK(dmalloc(&w.b2, MST_D));
            CHECK(dmalloc(&w.g1, MST_D));
            CHECK(dmalloc(&w.be1, MST_D));
            CHECK(dmalloc(&w.g2, MST_D));
            CHECK(dmalloc(&w.be2, MST_D));
            CHECK(dmalloc(&w.wtail, TailCfg::LAYER_BYTES / 2));
            CHECK(dmalloc(&w.wqkv, (size_t)3 * MST_D * MST_D));
            CHECK(dmalloc(&w.wsm_in, (size_t)3 * MST_D * MST_D));
            CHECK(dmalloc(&w.wsm_out, (size_t)MST_D * MST_D));
            CHECK(dmalloc(&w.wsm_1, (size_t)MST_FF * MST_D));
            CHECK(dmalloc(&w.wsm_2, (size_t)MST_D * MST_FF));
        }
    }
    if (!e->style_stage) CHECK(dmalloc(&e->style_stage, (size_t)(3 * MST_D * MST_D + MST_D * MST_D + 2 * MST_FF * MST_D)));
    std::vector<StyleLayer> tab((size_t)n * nl);
    for (int s = 0; s < n; s++)
        for (int l = 0; l < nl; l++) tab[(size_t)s * nl + l] = style_record(slot_layer(e, s, l));
    (void)hipFree(e->style_tab);
    e->style_tab = nullptr;
    CHECK(dmalloc(&e->style_tab, tab.size()));
    HIPCHECK(hipMemcpy(e->style_tab, tab.data(), tab.size() * sizeof(StyleLayer), hipMemcpyHostToDevice));
    if (!e->plan_dev) {
        // every slice layout of a call: row slots + clip order (2 ints per transformer row) and, per tile height h, at most
        // (rows of the slice) / h + 1 tiles + (clips of the slice) segments of 4 ints; plus alignment slack per table
        const size_t M = (size_t)e->cfg.max_rows * e->S_max, R = (size_t)e->cfg.max_rows, K = mst_engine::MAX_SLICES;
        size_t cap = 2 * R + 8 * K;
        for (int h = 16; h <= 64; h += 16) cap += 4 * (M / h + K + R) + 8 * K;
        CHECK(dmalloc(&e->plan_dev, cap));
        e->plan_cap = cap;
    }
    e->slot_loaded.resize(n, 0);                          // existing slots keep their state
    e->nslots = n;
    return 0;
}

extern "C" int mst_load_layers_slot(mst_engine* e, int32_t slot, const float* const* srcs, void* stream) {
    if (!e || !srcs) return fail("mst_load_layers_slot: null argument");
    if (slot == 0) return mst_load_layers(e, srcs, stream);
    if (slot < 0 || slot >= e->nslots) return fail("mst_load_layers_slot: slot %d outside 0..%d (mst_style_slots)", slot, e->nslots - 1);
    hipStream_t st = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    const int nl = e->cfg.num_layers;
    for (int i = 0; i < 12 * nl; i++) if (!srcs[i]) return fail("mst_load_layers_slot: null tensor %d", i);
    f16* const w_in = e->style_stage;
    f16* const w_out = w_in + 3 * MST_D * MST_D;
    f16* const w1 = w_out + MST_D * MST_D;
    f16* const w2 = w1 + MST_FF * MST_D;
    for (int l = 0; l < nl; l++) {
        LayerW& w = slot_layer(e, slot, l);
        const float* const* s = srcs + 12 * l;
        // the plain f16 matrices go to the staging buffer (stream-ordered: the previous layer's packs have read it), then the packings
        CHECK(put_matrix(s[0], 3 * MST_D, MST_D, w_in, 3 * MST_D, MST_D, st));
        CHECK(put_vector(s[1], 3 * MST_D, w.b_in, 3 * MST_D, st));
        CHECK(put_matrix(s[2], MST_D, MST_D, w_out, MST_D, MST_D, st));
        CHECK(put_vector(s[3], MST_D, w.b_out, MST_D, st));
        CHECK(put_matrix(s[4], MST_FF, MST_D, w1, MST_FF, MST_D, st));
        CHECK(put_vector(s[5], MST_FF, w.b1, MST_FF, st));
        CHECK(put_matrix(s[6], MST_D, MST_FF, w2, MST_D, MST_FF, st));
        CHECK(put_vector(s[7], MST_D, w.b2, MST_D, st));
        CHECK(put_vector(s[8], MST_D, w.g1, MST_D, st));
        CHECK(put_vector(s[9], MST_D, w.be1, MST_D, st));
        CHECK(put_vector(s[10], MST_D, w.g2, MST_D, st));
        CHECK(put_vector(s[11], MST_D, w.be2, MST_D, st));
        hipLaunchKernelGGL(k_pack_qkv, dim3(384), dim3(256), 0, st, w_in, w.wqkv);
        hipLaunchKernelGGL(k_pack_tail, dim3(640), dim3(256), 0, st, w_out, w1, w2, w.wtail);
        hipLaunchKernelGGL(k_pack_blocks, dim3(192), dim3(256), 0, st, w_in, MST_D, 3 * MST_D, MST_D, w.wsm_in);
        hipLaunchKernelGGL(k_pack_blocks, dim3(64), dim3(256), 0, st, w_out, MST_D, MST_D, MST_D, w.wsm_out);
        hipLaunchKernelGGL(k_pack_blocks, dim3(128), dim3(256), 0, st, w1, MST_D, MST_FF, MST_D, w.wsm_1);
        hipLaunchKernelGGL(k_pack_blocks, dim3(128), dim3(256), 0, st, w2, MST_FF, MST_D, MST_FF, w.wsm_2);
        HIPCHECK(hipGetLastError());
    }
    e->slot_loaded[slot] = 1;
    return 0;
}

extern "C" int mst_set_styles(mst_engine* e, const int32_t* styles_host, int32_t batch, void* stream) {
    (void)stream;
    if (!e) return fail("mst_set_styles: null engine");
    if (!styles_host) { e->styles.clear(); return 0; }
    if (batch < 1 || batch > e->cfg.max_rows) return fail("mst_set_styles: batch %d outside 1..%d", batch, e->cfg.max_rows);
    for (int i = 0; i < batch; i++)
        if (styles_host[i] < 0 || styles_host[i] >= e->nslots)
            return fail("mst_set_styles: clip %d has style %d outside [0, %d)", i, styles_host[i], e->nslots);
    for (int i = 0; i < batch; i++) {                        // slot memory is allocated uninitialised: never sample with it
        const int s = styles_host[i];
        if (s == 0 ? mst_weights_complete(e) != 0 : !e->slot_loaded[s])
            return fail("mst_set_styles: clip %d names style slot %d, which was never loaded (mst_load_layers_slot)", i, s);
    }
    e->styles.assign(styles_host, styles_host + batch);
    return 0;
}

static bool styles_on(const mst_engine* e) { return e->nslots > 1 && !e->styles.empty(); }

// The configurations the style-aware kernels cover; everything else is refused by name (never a silent single-style answer).
static int style_check(const mst_engine* e, int batch, int frames) {
    const char* what = nullptr;
    if (e->precise) what = "precise mode (mst_set_precise / MST_PRECISE)";
    else if (e->trunk_groups) what = "the resident trunk (mst_set_trunk_groups / MST_TRUNK)";
    else if (!e->fuse_tail) what = "MST_FUSE_TAIL=0";
    else if (e->fuse_qkv_attn != 1) what = "MST_FUSE_QKV_ATTN other than 1";
    else if (!e->small_fast) what = "MST_SMALL_FAST=0";
    else if (e->dbg_stage >= 0) what = "a debug stop (mst_debug_stop_after)";
    else if (e->graph_on) what = "graph replay (MST_GRAPH)";
    else if (e->prof_on) what = "profiling (mst_profile_enable)";
    else if (frames <= 16) what = "clips of 16 frames or fewer (split-operand kernels)";
    else if (!qkv_attn2_fits(frames + 1)) what = "clips of more than 207 frames";
    if (what) return fail("several styles: %s is not supported with more than one style slot", what);
    if ((int)e->styles.size() != batch) return fail("several styles: mst_set_styles named %zu clips, the call has %d", e->styles.size(), batch);
    return 0;
}

// This call's tables: for each slice (slice_of's split of the batch; cond + uncond twins of a clip share its slot) the slot of every
// transformer row, the clip order of the attention launch and the segments of every tile height -- built once and uploaded in ONE copy.
static int style_plan(mst_engine* e, int batch, int cfg, int frames, int nsl, hipStream_t st) {
    const int S = frames + 1;
    if (!e->plan_ev) HIPCHECK(hipEventCreateWithFlags(&e->plan_ev, hipEventDisableTiming));
    HIPCHECK(hipEventSynchronize(e->plan_ev));
    std::vector<int>& h = e->plan_host;
    h.clear();
    auto align4 = [&]() { while (h.size() & 3) h.push_back(0); };
    for (int sl = 0; sl < nsl; sl++) {
        StyleSlice& ps = e->plan_sl[sl];
        ps = StyleSlice{};
        const int c0 = slice_of(batch, nsl, sl).first, nb = slice_of(batch, nsl, sl).clips;
        if (nb <= 0) continue;
        const int rows = cfg ? 2 * nb : nb;
        std::vector<int> slot(rows);
        for (int r = 0; r < rows; r++) slot[r] = e->styles[c0 + r % nb];
        ps.rows = rows;
        align4();
        ps.off_slot = (int)h.size();
        h.insert(h.end(), slot.begin(), slot.end());
        ps.off_order = (int)h.size();
        if (e->style_xcd) { const std::vector<int> o = xcd_order(slot); h.insert(h.end(), o.begin(), o.end()); }
        else for (int r = 0; r < rows; r++) h.push_back(r);
        for (int hi = 0; hi < 4; hi++) {
            const int tr = 16 * (hi + 1), cap = (rows * S) / tr + 1 + rows;
            std::vector<StyleSeg> seg(cap);
            const int n = plan_segments(slot.data(), rows, S, tr, seg.data(), cap);
            if (n < 0) return fail("several styles: segment table overflow");
            seg.resize(n);
            if (e->style_xcd) {
                std::vector<int> key(n);
                for (int i = 0; i < n; i++) key[i] = seg[i].slot;
                const std::vector<int> o = xcd_order(key);
                std::vector<StyleSeg> re(n);
                for (int i = 0; i < n; i++) re[i] = seg[o[i]];
                seg.swap(re);
            }
            align4();
            ps.off_seg[hi] = (int)h.size();
            ps.nseg[hi] = n;
            for (const StyleSeg& g : seg) { h.push_back(g.row0); h.push_back(g.row_lo); h.push_back(g.row_hi); h.push_back(g.slot); }
        }
    }
    if (h.size() > e->plan_cap) return fail("several styles: plan of %zu ints exceeds %zu", h.size(), e->plan_cap);
    HIPCHECK(hipMemcpyAsync(e->plan_dev, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHECK(hipEventRecord(e->plan_ev, st));
    return 0;
}

template <int KS, int MODE, int LNF, int NTB>
static int launch_rows_seg(mst_engine* e, const StyleSlice& ps, int l, const f16* X, void* out, int ldo, int N, const LnRows& ln, hipStream_t st) {
    constexpr int smem = 64 * (KS / 16) * 1024 / (4 / NTB);
    if constexpr (NTB == 4) CHECK(ensure_dyn_lds((const void*)k_rows_gemm_seg<KS, MODE, LNF, NTB>, smem));
    const int hi = style_h_index(16 * NTB), nl = e->cfg.num_layers;
    const StyleSeg* segs = reinterpret_cast<const StyleSeg*>(e->plan_dev + ps.off_seg[hi]);
    hipLaunchKernelGGL((k_rows_gemm_seg<KS, MODE, LNF, NTB>), dim3(ps.nseg[hi], N / 128), dim3(512), smem, st, X, e->style_tab + l,
                       e->style_tab + (l > 0 ? l - 1 : 0), nl, segs, out, ldo, ln);
    HIPCHECK(hipGetLastError());
    return 0;
}
// launch_rows_gemm's tile heights, per segment table
template <int KS, int MODE>
static int launch_rows_seg_m(mst_engine* e, const StyleSlice& ps, int l, int M, const f16* X, void* out, int ldo, int N, hipStream_t st) {
    const int ntb = rows_ntb(M, g_rows_ntb1_m, g_rows_ntb2_from);
    if (ntb == 1) return launch_rows_seg<KS, MODE, 0, 1>(e, ps, l, X, out, ldo, N, LnRows{}, st);
    if (ntb == 2) return launch_rows_seg<KS, MODE, 0, 2>(e, ps, l, X, out, ldo, N, LnRows{}, st);
    return launch_rows_seg<KS, MODE, 0, 4>(e, ps, l, X, out, ldo, N, LnRows{}, st);
}
static int launch_ln_style(mst_engine* e, const StyleSlice& ps, int l, int which, const float* acc, f16* hi, f16* lo, int M, int S, hipStream_t st,
                           f16* ohi = nullptr, f16* olo = nullptr) {
    hipLaunchKernelGGL(k_ln_rows_style, dim3((M + 3) / 4), dim3(256), 0, st, acc, e->style_tab + l, e->cfg.num_layers, which, e->plan_dev + ps.off_slot,
                       S, hi, lo, M, ohi, olo);
    HIPCHECK(hipGetLastError());
    return 0;
}
template <int NT16>
static int launch_qkv_attn2_style_n(mst_engine* e, const StyleSlice& ps, int l, const WS& ws, int S, int rows, hipStream_t st) {
    auto kern = k_qkv_attention2_style<NT16>;
    constexpr int smem = QA2Tile<NT16>::SMEM;
    CHECK(ensure_dyn_lds((const void*)kern, smem));
    hipLaunchKernelGGL(kern, dim3(rows * MST_H), dim3(512), smem, st, ws.hx, e->style_tab + l, e->cfg.num_layers, e->plan_dev + ps.off_slot,
                       e->plan_dev + ps.off_order, ws.att, S);
    HIPCHECK(hipGetLastError());
    return 0;
}
static int launch_qkv_attn2_style(mst_engine* e, const StyleSlice& ps, int l, const WS& ws, int S, int rows, int nt16, hipStream_t st) {
    NT16_SWITCH(launch_qkv_attn2_style_n, nt16, S, e, ps, l, ws, S, rows, st)
}
static int launch_tail_style(mst_engine* e, const StyleSlice& ps, int l, const WS& ws, int ntb, hipStream_t st) {
    const int hi = style_h_index(16 * ntb), nl = e->cfg.num_layers;
    const StyleSeg* segs = reinterpret_cast<const StyleSeg*>(e->plan_dev + ps.off_seg[hi]);
#define TAIL_SEG(N_)                                                                                                               \
    do {                                                                                                                           \
        CHECK(ensure_dyn_lds((const void*)k_layer_tail_seg<N_>, TailCfg::SMEM));                                                   \
        hipLaunchKernelGGL(k_layer_tail_seg<N_>, dim3(ps.nseg[hi]), dim3(512), TailCfg::SMEM, st, ws.att, e->style_tab + l, nl, segs, \
                           ws.hx, ws.hl, e->gelu_tab);                                                                             \
    } while (0)
    if (ntb == 2) TAIL_SEG(2);
    else if (ntb == 3) TAIL_SEG(3);
    else TAIL_SEG(4);
#undef TAIL_SEG
    HIPCHECK(hipGetLastError());
    return 0;
}

// run_trunk for a batch of several styles: the default fused path (style_check has refused everything else), each launch reading the
// slice's tables.  Same launch sequence and tile heights as the single-style path.
static int run_trunk_style(mst_engine* e, const WS& ws, int rows, int T, hipStream_t st, const StyleSlice& ps, const TrunkPlan& tp) {
    const int S = T + 1, M = rows * S, NL = e->cfg.num_layers;
    if (ps.rows != rows) return fail("several styles: slice of %d rows, plan of %d", rows, ps.rows);
    const bool small = tp.path != PATH_LARGE, lnf = tp.lnf;
    for (int l = 0; small && l < NL; l++) {
        {
            ProfScope pq(e, FAM_QKV, st);
            if (lnf && l > 0) {
                const LnRows ln{ws.zacc, nullptr, nullptr, nullptr, ws.hx2, ws.hl2, ws.hx, ws.hl};
                CHECK((launch_rows_seg<16, 0, 1, 1>(e, ps, l, nullptr, ws.qkv, 3 * MST_D, 3 * MST_D, ln, st)));
            } else CHECK((launch_rows_seg_m<16, 0>(e, ps, l, M, ws.hx, ws.qkv, 3 * MST_D, 3 * MST_D, st)));
        }
        {
            ProfScope pa(e, FAM_ATTN, st);
            CHECK(launch_attn(ws.qkv, ws.att, S, rows, st, 1, nullptr));
        }
        {
            ProfScope po(e, FAM_OUTPROJ_LN, st);
            CHECK((launch_rows_seg_m<16, 2>(e, ps, l, M, ws.att, ws.zacc, MST_D, MST_D, st)));
            if (!lnf) CHECK(launch_ln_style(e, ps, l, 0, ws.zacc, ws.hx, ws.hl, M, S, st));
        }
        {
            ProfScope p1(e, FAM_FFN1, st);
            if (lnf) {
                const LnRows ln{ws.zacc, nullptr, nullptr, nullptr, ws.hx, ws.hl, ws.hx2, ws.hl2};
                CHECK((launch_rows_seg<16, 1, 1, 1>(e, ps, l, nullptr, ws.hid, MST_FF, MST_FF, ln, st)));
            } else CHECK((launch_rows_seg_m<16, 1>(e, ps, l, M, ws.hx, ws.hid, MST_FF, MST_FF, st)));
        }
        {
            ProfScope p2(e, FAM_FFN2_LN, st);
            CHECK((launch_rows_seg_m<32, 2>(e, ps, l, M, ws.hid, ws.zacc, MST_D, MST_D, st)));
            if (!lnf) CHECK(launch_ln_style(e, ps, l, 1, ws.zacc, ws.hx, ws.hl, M, S, st));
            else if (l == NL - 1) CHECK(launch_ln_style(e, ps, l, 1, ws.zacc, ws.hx2, ws.hl2, M, S, st, ws.hx, ws.hl));
        }
    }
    for (int l = 0; !small && l < NL; l++) {
        {
            ProfScope pq(e, FAM_QKV_ATTN, st);
            CHECK(launch_qkv_attn2_style(e, ps, l, ws, S, rows, tp.nt16, st));
        }
        {
            ProfScope pt(e, FAM_TAIL, st);
            CHECK(launch_tail_style(e, ps, l, ws, tp.tail_ntb, st));
        }
    }
    return 0;
}

// K3 .. K8: token stream through the encoder stack.  rows = clips through the transformer.
// K1-K3: conditioning token + pose embedding of the frames -> token stream rows (ws.hx / ws.hl)
struct LoopRef { const LoopDev* ld = nullptr; int joff = 0; unsigned long long eo = 0; bool frames_ready = false; bool stream_ready = false; };   // stream_ready: the previous step's k_embed_out already embedded this step (token stream and conditioning tokens are in ws.hx / ws.hl)   // frames_ready: the previous step's epilogue already wrote ws.xt   // loop mode of a step's kernels (see LoopDev)

template <int KS>
static int launch_embed_in_n(mst_engine* e, const WS& ws, int tot, const DEpiEmbedIn& epi, hipStream_t st) {
    CHECK(ensure_dyn_lds((const void*)k_embed_in<KS>, EmbCfg::SMEM));
    hipLaunchKernelGGL(k_embed_in<KS>, dim3((tot + EmbCfg::BT - 1) / EmbCfg::BT), dim3(512), EmbCfg::SMEM, st, ws.xt, ws.xt_lo, e->kin_pad,
                       e->w_pose_in_pk, epi);
    HIPCHECK(hipGetLastError());
    return 0;
}
static int launch_embed_in(mst_engine* e, const WS& ws, int tot, const DEpiEmbedIn& epi, const EmbedInPlan& ip, hipStream_t st) {
    switch (ip.ks) {
#define EI(K_) case K_: return launch_embed_in_n<K_>(e, ws, tot, epi, st);
        EI(3) EI(4) EI(5) EI(6) EI(7) EI(8) EI(9) EI(10) EI(11) EI(12) EI(13) EI(14) EI(15) EI(16)
#undef EI
    }
    return fail("pose embedding: %d input columns unsupported", e->kin_pad);
}

// the pose embedding's epilogue of a model call / loop step: positional rows, stream rows, conditioning tokens
static DEpiEmbedIn embed_in_epi(const mst_engine* e, const WS& ws, int clips_x, int rows, int T, int temb_uniform_row, int temb_mod, int tp_uncond,
                                const LoopDev* ld, int joff, const long long* tidx_table = nullptr, const Drop* pe_dropout = nullptr) {
    const int S = T + 1, tot = clips_x * T;
    DEpiEmbedIn epi{e->b_pose_in, e->pe, ws.hx, ws.hl, T, S, tot, rows > clips_x ? (size_t)clips_x * S * MST_D : 0};
    epi.ct.temb = e->temb; epi.ct.textproj = ws.textproj; epi.ct.ld = ld;
    epi.ct.uniform_row = temb_uniform_row; epi.ct.temb_mod = temb_mod; epi.ct.joff = joff; epi.ct.rows = rows;
    epi.ct.tp_half = rows > clips_x ? clips_x : 0; epi.ct.tp_uncond = rows > clips_x ? tp_uncond : 0;
    if (tidx_table) { epi.ct.temb = e->temb_table; epi.ct.tidx = tidx_table; }
    if (pe_dropout) epi.pd = *pe_dropout;
    return epi;
}

static int assemble_stream(mst_engine* e, const WS& ws, const float* x, int clips_x, int rows, int T, int temb_uniform_row, int temb_mod,
                           hipStream_t st, int tp_uncond, LoopRef lr = LoopRef(), const long long* tidx_table = nullptr, const Drop* pe_dropout = nullptr) {
    if (lr.stream_ready) return 0;
    const int S = T + 1;
    (void)S;
    // (the conditioning token of every clip -- timestep embedding + text projection + positional row 0, formerly a launch of its
    // own, k_cond_token -- is written by the pose-embedding GEMM's epilogue: CondTok in mst_gemm_dma.h)
    {
        // frames -> f16 rows (transpose + convert), then the pose-embedding GEMM on the DMA ring.  The doubled
        // CFG batch feeds the same x to both halves: embed once, store twice (dup).
        ProfScope ps(e, FAM_EMBED_IN, st);
        const int F = e->cfg.feats, tot = clips_x * T;
        if (!lr.frames_ready) {
            hipLaunchKernelGGL(k_frames_f16, dim3((T + 31) / 32, e->kin_pad / 32, clips_x), dim3(256), 0, st, x, F, T, e->kin_pad, ws.xt, (const float*)nullptr, lr.ld, lr.eo, ws.xt_lo);
            HIPCHECK(hipGetLastError());
        }
        const DEpiEmbedIn epi = embed_in_epi(e, ws, clips_x, rows, T, temb_uniform_row, temb_mod, tp_uncond, lr.ld, lr.joff, tidx_table, pe_dropout);
        const EmbedInPlan ip = plan_embed_in(F, e->precise, e->embed_fast);
        if (ip.kernel == EMBED_LATENCY) return launch_embed_in(e, ws, tot, epi, ip, st);
        // x_t as hi + lo (RowsDirect::Xlo): both halves of a k-slab beside ONE copy of the weight slab
        CHECK((launch_gemm_dma<64, 512, 2, 2, 4, 1, 32, 2>(dim3((tot + 63) / 64, 1), RowsDirect{ws.xt, e->kin_pad, ws.xt_lo, e->precise ? e->w_pose_in_lo : nullptr},
                                                          e->w_pose_in, e->kin_pad, e->kin_pad, epi, st)));
    }
    return 0;
}

// K3 .. K8: token stream through the encoder stack.  rows = clips through the transformer; tp = plan_trunk of this launch sequence
// (mst_plan.h); style = the slice's tables when the batch holds several styles (nullptr: single-style launches).
static int run_trunk(mst_engine* e, const WS& ws, const float* x, int clips_x, int rows, int T, int temb_uniform_row, int temb_mod,
                     hipStream_t st, const TrunkPlan& tp, const StyleSlice* style, int tp_uncond = 0, LoopRef lr = LoopRef()) {
    const int S = T + 1, M = rows * S;
    CHECK(assemble_stream(e, ws, x, clips_x, rows, T, temb_uniform_row, temb_mod, st, tp_uncond, lr));
    if (e->dbg_stage == 0) return 0;
    if (style) return run_trunk_style(e, ws, rows, T, st, *style, tp);
#define DBG_STOP(stage) if (e->dbg_layer == l && e->dbg_stage == stage) return 0;
    const bool small = tp.path <= PATH_SMALL_ROWS_LN, fast = small && tp.path != PATH_SMALL_RING, lnf = tp.lnf;
    // split operands (RowsDirect::Xlo): the lo halves of att and hid borrow the idle hid / qkv buffers
    f16 *const att_lo = tp.precise ? ws.hid : nullptr, *const hid_lo = tp.precise ? ws.qkv : nullptr;
    const f16* const hl_in = tp.precise ? ws.hl : nullptr;
    // lnf (LnRows): LN1 in FFN1, which leaves the stream in (hx2, hl2); LN2 in the next layer's QKV GEMM, which brings it back to
    // (hx, hl); the last LN2 as the rows kernel
    const int NL = e->cfg.num_layers;
    for (int l = 0; small && l < NL; l++) {
        const LayerW& w = e->L[l];
        {
            ProfScope ps(e, FAM_QKV, st);
            if (lnf && l > 0) {
                const LayerW& p = e->L[l - 1];
                const LnRows ln{ws.zacc, p.b2, p.g2, p.be2, ws.hx2, ws.hl2, ws.hx, ws.hl};
                CHECK((launch_rows_gemm<16, 0>(M, 3 * MST_D, nullptr, w.wsm_in, w.b_in, ws.qkv, 3 * MST_D, st, &ln)));
            } else if (fast) CHECK((launch_rows_gemm<16, 0>(M, 3 * MST_D, ws.hx, w.wsm_in, w.b_in, ws.qkv, 3 * MST_D, st)));
            else {
                DEpiBiasF16<false> epi{w.b_in, ws.qkv, 3 * MST_D, M};
                CHECK(launch_small(M, 3 * MST_D, RowsDirect{ws.hx, MST_D, hl_in, e->precise ? w.w_in_lo : nullptr}, w.w_in, MST_D, MST_D, epi, st));
            }
        }
        DBG_STOP(1)
        {
            ProfScope ps(e, FAM_ATTN, st);
            CHECK(launch_attn(ws.qkv, ws.att, S, rows, st, 1, att_lo));
        }
        DBG_STOP(2)
        {
            ProfScope ps(e, FAM_OUTPROJ_LN, st);
            if (fast) CHECK((launch_rows_gemm<16, 2>(M, MST_D, ws.att, w.wsm_out, nullptr, ws.zacc, MST_D, st)));
            else {
                DEpiPlainF32 epi{ws.zacc, MST_D, M};
                CHECK(launch_small(M, MST_D, RowsDirect{ws.att, MST_D, att_lo, e->precise ? w.w_out_lo : nullptr}, w.w_out, MST_D, MST_D, epi, st));
            }
            if (!lnf) hipLaunchKernelGGL(k_ln_rows, dim3((M + 3) / 4), dim3(256), 0, st, ws.zacc, w.b_out, w.g1, w.be1, ws.hx, ws.hl, M, (f16*)nullptr, (f16*)nullptr);
            HIPCHECK(hipGetLastError());
        }
        DBG_STOP(3)
        {
            ProfScope ps(e, FAM_FFN1, st);
            if (lnf) {
                const LnRows ln{ws.zacc, w.b_out, w.g1, w.be1, ws.hx, ws.hl, ws.hx2, ws.hl2};
                CHECK((launch_rows_gemm<16, 1>(M, MST_FF, nullptr, w.wsm_1, w.b1, ws.hid, MST_FF, st, &ln)));
            } else if (fast) CHECK((launch_rows_gemm<16, 1>(M, MST_FF, ws.hx, w.wsm_1, w.b1, ws.hid, MST_FF, st)));
            else {
                DEpiBiasF16<true> epi{w.b1, ws.hid, MST_FF, M, hid_lo};
                CHECK(launch_small(M, MST_FF, RowsDirect{ws.hx, MST_D, hl_in, e->precise ? w.w1_lo : nullptr}, w.w1, MST_D, MST_D, epi, st));
            }
        }
        DBG_STOP(4)
        {
            ProfScope ps(e, FAM_FFN2_LN, st);
            if (fast) CHECK((launch_rows_gemm<32, 2>(M, MST_D, ws.hid, w.wsm_2, nullptr, ws.zacc, MST_D, st)));
            else {
                DEpiPlainF32 epi{ws.zacc, MST_D, M};
                CHECK(launch_small(M, MST_D, RowsDirect{ws.hid, MST_FF, hid_lo, e->precise ? w.w2_lo : nullptr}, w.w2, MST_FF, MST_FF, epi, st));
            }
            if (!lnf) hipLaunchKernelGGL(k_ln_rows, dim3((M + 3) / 4), dim3(256), 0, st, ws.zacc, w.b2, w.g2, w.be2, ws.hx, ws.hl, M, (f16*)nullptr, (f16*)nullptr);
            else if (l == NL - 1) hipLaunchKernelGGL(k_ln_rows, dim3((M + 3) / 4), dim3(256), 0, st, ws.zacc, w.b2, w.g2, w.be2, ws.hx2, ws.hl2, M, ws.hx, ws.hl);
            HIPCHECK(hipGetLastError());
        }
        DBG_STOP(5)
    }
    if (tp.path == PATH_RESIDENT) return launch_trunk_groups(e, ws, S, rows, st);
    for (int l = 0; !small && l < e->cfg.num_layers; l++) {
        const LayerW& w = e->L[l];
        if (tp.qkv_attn != QA_UNFUSED && !(e->dbg_layer == l && e->dbg_stage == 1)) {
            ProfScope ps(e, FAM_QKV_ATTN, st);
            if (tp.qkv_attn == QA_STREAMED) CHECK(launch_qkv_attn2(ws.hx, w.wqkv, w.b_in, ws.att, S, rows, tp.nt16, st));
            else CHECK(launch_qkv_attn(ws.hx, w.w_in, w.b_in, ws.att, S, rows, st));
        } else {
            {
                ProfScope ps(e, FAM_QKV, st);
                DEpiBiasF16<false> epi{w.b_in, ws.qkv, 3 * MST_D, M};
                CHECK((launch_wide(M, 3 * MST_D / 256, RowsDirect{ws.hx, MST_D}, w.w_in, MST_D, MST_D, epi, st)));
            }
            DBG_STOP(1)
            {
                ProfScope ps(e, FAM_ATTN, st);
                CHECK(launch_attn(ws.qkv, ws.att, S, rows, st));
            }
        }
        DBG_STOP(2)
        if (tp.fuse_tail && !(e->dbg_layer == l && (e->dbg_stage == 3 || e->dbg_stage == 4))) {
            ProfScope ps(e, FAM_TAIL, st);
            CHECK(launch_tail(e, w, ws, M, tp.tail_ntb, st));
            DBG_STOP(5)
            continue;
        }
        {
            ProfScope ps(e, FAM_OUTPROJ_LN, st);
            DEpiResidLN epi{w.b_out, w.g1, w.be1, ws.hx, ws.hl, M};
            if (tp.ln128)
                CHECK((launch_gemm_dma<128, 512, 2, 4, 2, 1, 64>(dim3((M + 127) / 128, 1), RowsDirect{ws.att, MST_D}, w.w_out, MST_D, MST_D, epi, st)));
            else
                CHECK((launch_gemm_dma<64, 512, 2, 2, LN_NS, 1, LN_BK>(dim3((M + 63) / 64, 1), RowsDirect{ws.att, MST_D}, w.w_out, MST_D, MST_D, epi, st)));
        }
        DBG_STOP(3)
        {
            ProfScope ps(e, FAM_FFN1, st);
            DEpiBiasF16<true> epi{w.b1, ws.hid, MST_FF, M};
#if FFN1_BF == 512      // 128 x 512 tiles: 198 blocks at batch 64, one per CU, 640 KB staged per block
            const int nx = (M + 127) / 128;
            CHECK((launch_gemm_dma<128, 512, 2, 4, 3, 1>(dim3(((nx + 7) / 8) * 8 * 2, 1, 1), RowsDirect{ws.hx, MST_D}, w.w1, MST_D, MST_D, epi, st, 2)));
#else
            CHECK((launch_wide(M, MST_FF / 256, RowsDirect{ws.hx, MST_D}, w.w1, MST_D, MST_D, epi, st)));
#endif
        }
        DBG_STOP(4)
        {
            ProfScope ps(e, FAM_FFN2_LN, st);
            DEpiResidLN epi{w.b2, w.g2, w.be2, ws.hx, ws.hl, M};
            if (tp.ln128)
                CHECK((launch_gemm_dma<128, 512, 2, 4, 2, 1, 64>(dim3((M + 127) / 128, 1), RowsDirect{ws.hid, MST_FF}, w.w2, MST_FF, MST_FF, epi, st)));
            else
                CHECK((launch_gemm_dma<64, 512, 2, 2, LN_NS, 1, LN_BK>(dim3((M + 63) / 64, 1), RowsDirect{ws.hid, MST_FF}, w.w2, MST_FF, MST_FF, epi, st)));
        }
        DBG_STOP(5)
    }
#undef DBG_STOP
    return 0;
}

// output projection tiles: 64 frames x BF features.  8 waves as 1 x 8 with 2 x NTO MFMA tiles each (BF = 256 NTO), or -- for
// 257..384 features, the HumanML / bandai widths -- as 2 x 4 with 1 x 3 tiles (BF = 384): the 512-row tile streamed and multiplied
// 37 % zero-padding rows per slab.
template <int MODE, int BF, int MT, int NT, int NX, int XS = 1>
static int launch_out(mst_engine* e, const WS& ws, int batch, int T, float* out, const StepArgs& sa, hipStream_t st,
                      const f16* w_override = nullptr, const float* b_override = nullptr, int tok_off = 1, bool frames_next = false,
                      bool hi_lo = false) {
    const int S = T + tok_off;
    RowsFrames xs{ws.hx, MST_D, T, S, batch * T, 64, (size_t)batch * S, tok_off, hi_lo ? ws.hl : nullptr,   // hi_lo: ws.hx / ws.hl are the last stream
                  hi_lo && e->precise && !w_override ? e->w_pose_out_lo : nullptr};
    DEpiEmbedOut<MODE> epi{b_override ? b_override : e->b_pose_out, e->cfg.feats, T, batch * T, out, sa};
    if (frames_next) { epi.xt_next = ws.xt; epi.kpad = e->kin_pad; epi.xt_next_lo = ws.xt_lo; }
    return launch_gemm_dma<64, BF, MT, NT, 4, NX, 32, XS>(dim3((batch * T + 63) / 64, 1), xs, w_override ? w_override : e->w_pose_out, MST_D, MST_D, epi, st);
}
template <int MODE, int BF, int MT, int NT>
static int launch_out_nx(mst_engine* e, const WS& ws, const EmbedOutPlan& op, int batch, int T, float* out, const StepArgs& sa, hipStream_t st,
                         const f16* wo = nullptr, const float* bo = nullptr, int tok_off = 1, bool frames_next = false, bool hi_lo = false) {
    const bool cfg = op.nx == 2;
    // hi + lo stream: both halves of a k-slab beside one copy of the weight slab where that ring fits the LDS (<= 384 rows),
    // otherwise the K range twice (gemm_mainloop_dma)
    if constexpr (BF <= 384) {
        if (op.ring_xs == 2) return cfg ? launch_out<MODE, BF, MT, NT, 2, 2>(e, ws, batch, T, out, sa, st, wo, bo, tok_off, frames_next, true)
                              : launch_out<MODE, BF, MT, NT, 1, 2>(e, ws, batch, T, out, sa, st, wo, bo, tok_off, frames_next, true);
    }
    return cfg ? launch_out<MODE, BF, MT, NT, 2>(e, ws, batch, T, out, sa, st, wo, bo, tok_off, frames_next, hi_lo)
               : launch_out<MODE, BF, MT, NT, 1>(e, ws, batch, T, out, sa, st, wo, bo, tok_off, frames_next, hi_lo);
}
template <int MODE, int NBW, int NX>
static int launch_embed_out_n(mst_engine* e, const RowsFrames& xs, const DEpiEmbedOut<MODE>& epi, int tiles, hipStream_t st) {
    CHECK(ensure_dyn_lds((const void*)k_embed_out<NBW, MODE, NX>, EmbCfg::SMEM));
    hipLaunchKernelGGL((k_embed_out<NBW, MODE, NX>), dim3(tiles), dim3(512), EmbCfg::SMEM, st, xs, e->w_pose_out_pk, epi);
    HIPCHECK(hipGetLastError());
    return 0;
}
// Can a sampling step's output projection also embed the NEXT step (k_embed_out<.., KSN>)?  embed_next_ksn of mst_plan.h.
static bool embed_next_fits(const mst_engine* e, int T) { return embed_next_ksn(e->cfg.feats, T, e->precise, e->embed_fast) != 0; }
template <int MODE, int NBW, int KSN>
static int launch_embed_step_n(mst_engine* e, const RowsFrames& xs, const DEpiEmbedOut<MODE>& epi, const DEpiEmbedIn& next, int tiles, hipStream_t st) {
    CHECK(ensure_dyn_lds((const void*)k_embed_out<NBW, MODE, 1, KSN>, EmbCfg::SMEM));
    hipLaunchKernelGGL((k_embed_out<NBW, MODE, 1, KSN>), dim3(tiles), dim3(512), EmbCfg::SMEM, st, xs, e->w_pose_out_pk, epi, e->w_pose_in_pk, next);
    HIPCHECK(hipGetLastError());
    return 0;
}
template <int MODE>
static int launch_embed_out(mst_engine* e, const WS& ws, const EmbedOutPlan& op, int batch, int T, float* out, const StepArgs& sa, hipStream_t st,
                            int tok_off, bool frames_next, const DEpiEmbedIn* next = nullptr) {
    const int S = T + tok_off, tiles = (batch * T + EmbCfg::BT - 1) / EmbCfg::BT;
    RowsFrames xs{ws.hx, MST_D, T, S, batch * T, EmbCfg::BT, (size_t)batch * S, tok_off, ws.hl, nullptr};
    DEpiEmbedOut<MODE> epi{e->b_pose_out, e->cfg.feats, T, batch * T, out, sa};
    if (frames_next) { epi.xt_next = ws.xt; epi.kpad = e->kin_pad; epi.xt_next_lo = ws.xt_lo; }
    const bool cfg = op.nx == 2;
    if constexpr (MODE != 0) {
        if (next) {                                         // (mst_sample_loop asked embed_next_fits first)
            if (cfg || tok_off != 1) return fail("output projection: the fused next-step embedding is for plain sampling steps");
            epi.xt_next = ws.xt; epi.kpad = e->kin_pad;     // (marks the tile as reusable: OutItems::apply writes x_{t-1} back into it)
            switch (op.ksn) {
                case 5: return launch_embed_step_n<MODE, 2, 5>(e, xs, epi, *next, tiles, st);
                case 6: return launch_embed_step_n<MODE, 2, 6>(e, xs, epi, *next, tiles, st);
                case 9: return launch_embed_step_n<MODE, 3, 9>(e, xs, epi, *next, tiles, st);
            }
            return fail("output projection: no fused instantiation for %d input columns", e->kin_pad);
        }
    }
#define EO(N_) case N_: return cfg ? launch_embed_out_n<MODE, N_, 2>(e, xs, epi, tiles, st) : launch_embed_out_n<MODE, N_, 1>(e, xs, epi, tiles, st);
    switch (op.nbw) { EO(1) EO(2) EO(3) case 4: return launch_embed_out_n<MODE, 4, 1>(e, xs, epi, tiles, st); }
#undef EO
    return fail("output projection: %d features unsupported", e->cfg.feats);
}
template <int MODE>
static int launch_out_nt(mst_engine* e, const WS& ws, int cfg, int batch, int T, float* out, const StepArgs& sa, hipStream_t st,
                         const f16* wo = nullptr, const float* bo = nullptr, int tok_off = 1, bool frames_next = false, bool hi_lo = false,
                         const DEpiEmbedIn* next = nullptr) {
    ProfScope ps(e, FAM_EMBED_OUT, st);
    const EmbedOutPlan op = plan_embed_out(e->cfg.feats, T, cfg, e->precise, e->embed_fast, MODE, hi_lo, wo || bo);
    if (op.kernel == EMBED_LATENCY) return launch_embed_out<MODE>(e, ws, op, batch, T, out, sa, st, tok_off, frames_next, next);
    if (next) return fail("output projection: the fused next-step embedding needs the fast embed kernels");
    // (the ring also runs the pose embedding's backward, with W_in^T)
    if (op.ring_bf == 256) return launch_out_nx<MODE, 256, 2, 1>(e, ws, op, batch, T, out, sa, st, wo, bo, tok_off, frames_next, hi_lo);
    if (op.ring_bf == 384) return launch_out_nx<MODE, 384, 1, 3>(e, ws, op, batch, T, out, sa, st, wo, bo, tok_off, frames_next, hi_lo);
    return launch_out_nx<MODE, 512, 2, 2>(e, ws, op, batch, T, out, sa, st, wo, bo, tok_off, frames_next, hi_lo);
}

// the switches mst_plan.h decides by, as they stand now (mst_set_precise, mst_set_trunk_groups and mst_debug_stop_after change them between calls)
static PlanKnobs plan_knobs(const mst_engine* e) {
    return PlanKnobs{e->small_m, e->small_ln, e->small_ln_m, e->small_fast, e->precise, e->fuse_qkv_attn, e->fuse_tail, e->tail_ntb, e->ln128_min_m,
                     e->trunk_groups, e->cfg.num_layers, e->nsplit, e->dbg_stage >= 0};
}

static int check_ready(mst_engine* e, int batch, int frames, int cfg) {
    if (!e) return fail("null engine");
    CHECK(mst_weights_complete(e));
    if (frames < 1 || frames > e->cfg.max_frames) return fail("frames %d outside 1..%d", frames, e->cfg.max_frames);
    int rows = cfg ? 2 * batch : batch;
    if (batch < 1 || rows > e->cfg.max_rows) return fail("batch %d (rows %d) exceeds max_rows %d", batch, rows, e->cfg.max_rows);
    if (e->precise && !e->lo_missing.empty())
        return fail("precise mode: %zu weight matrices (first: %s) were uploaded while it was off, without their lo halves: upload them again",
                    e->lo_missing.size(), e->lo_missing.begin()->c_str());
    if (e->text_batch != batch || e->text_cfg != (cfg ? 1 : 0))
        return fail("mst_set_text was not called for batch %d cfg %d (have %d/%d)", batch, cfg, e->text_batch, e->text_cfg);
    return 0;
}

extern "C" int mst_forward(mst_engine* e, const float* x, const int64_t* t, const float* scale, int32_t batch, int32_t frames,
                           int32_t cfg, float* out, void* stream) {
    CHECK(check_ready(e, batch, frames, cfg));
    if (!x || !t || !out || (cfg && !scale)) return fail("mst_forward: null argument");
    hipStream_t st = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    e->prof_now = e->prof_on;
    CHECK(ensure_packed(e, st));
    CHECK(timestep_rows(e, (const long long*)t, batch, st));
    const int rows = cfg ? 2 * batch : batch;
    const WS ws = ws_slice(e, 0, frames);
    if (styles_on(e)) {
        CHECK(style_check(e, batch, frames));
        CHECK(style_plan(e, batch, cfg, frames, 1, st));
    }
    CHECK(run_trunk(e, ws, x, batch, rows, frames, -1, batch, st, plan_trunk(plan_knobs(e), rows, frames, 1, e->prof_now),
                    styles_on(e) ? &e->plan_sl[0] : nullptr, batch));
    StepArgs sa{};
    sa.scale = scale;
    return trunk_settle(e, st, launch_out_nt<0>(e, ws, cfg, batch, frames, out, sa, st, nullptr, nullptr, 1, false, true));
}

extern "C" int mst_loop_slices(const mst_engine* e, int32_t batch, int32_t cfg, int32_t frames) {
    return e ? plan_slices(plan_knobs(e), batch, cfg, frames > 0 ? frames : e->cfg.max_frames) : 1;
}

struct LoopPlan {
    const mst_schedule* s; const mst_loop_args* a; int nsl; size_t per_clip, clip_elems;
    hipStream_t streams[mst_engine::MAX_SLICES];
    const mst_guide_args* gd = nullptr;      // mst_sample_loop_guided: the step kernels are the guided MODEs
};
// One slice of a loop's launch sequence: its clips, its rows of the workspace, its stream, its style tables and its trunk plan;
// for_each_slice calls body(SliceCtx) for every non-empty slice of the batch in nsl slices (slice sl on p.streams[sl]).
struct SliceCtx { int c0, nb; size_t eo; WS ws; hipStream_t ss; const StyleSlice* style; TrunkPlan tp; };
template <class Body>
static int for_each_slice(mst_engine* e, const LoopPlan& p, int nsl, const Body& body) {
    const mst_loop_args* a = p.a;
    const PlanKnobs k = plan_knobs(e);
    for (int sl = 0; sl < nsl; sl++) {
        const SliceRange r = slice_of(a->batch, nsl, sl);
        if (r.clips <= 0) continue;
        // workspace rows of the slice: its clips (cond + uncond twins under CFG); text projections are indexed in the full-batch
        // layout [cond 0..B | uncond 0..B].  (Several styles: the tables are planned for p.nsl slices; instrumented steps are refused.)
        WS ws = ws_slice(e, a->cfg ? 2 * r.first : r.first, a->frames);
        ws.textproj = e->textproj + (size_t)r.first * MST_D;
        CHECK(body(SliceCtx{r.first, r.clips, (size_t)r.first * p.per_clip, ws, p.streams[sl], styles_on(e) ? &e->plan_sl[sl] : nullptr,
                            plan_trunk(k, a->cfg ? 2 * r.clips : r.clips, a->frames, nsl, e->prof_now)}));
    }
    return 0;
}
// MODE of a loop step's output projection (DEpiEmbedOut<MODE>; 0 = the model output alone)
static int step_mode(int sampler, bool guided) {
    if (guided) return sampler == MST_SAMPLER_DDPM ? 5 : 6;
    return sampler == MST_SAMPLER_DDPM ? 1 : sampler == MST_SAMPLER_DDIM_REVERSE ? 3 : sampler == MST_SAMPLER_PLMS ? 4 : 2;
}
// One denoise step of every slice, enqueued (or captured); step = *ld.jbase + joff.
// frames_ready / frames_next: the step's frame rows (ws.xt) were written by the previous step's epilogue / this step's epilogue
// writes them for the next one (mst_sample_loop decides; see DEpiEmbedOut::xt_next)
// stream_ready / embed_next: the previous step's output projection embedded this step / this step's embeds the next (k_embed_out<.., KSN>)
static int enqueue_step(mst_engine* e, const LoopPlan& p, int joff, int nsj, bool frames_ready = false, bool frames_next = false,
                        bool stream_ready = false, bool embed_next = false) {
    const mst_loop_args* a = p.a;
    return for_each_slice(e, p, nsj, [&](const SliceCtx& c) -> int {
        const auto& [c0, nb, eo, ws, ss, style, tp] = c;
        LoopRef lr{e->ld_dev, joff, eo, frames_ready, stream_ready};
        CHECK(run_trunk(e, ws, nullptr, nb, a->cfg ? 2 * nb : nb, a->frames, 0, 0, ss, tp, style, a->batch, lr));
        const DEpiEmbedIn next_epi = embed_in_epi(e, ws, nb, nb, a->frames, 0, 0, a->batch, e->ld_dev, joff + 1);
        const DEpiEmbedIn* next = embed_next ? &next_epi : nullptr;
        StepArgs sa{};
        sa.tab = p.s->tab; sa.nsteps = p.s->n;
        // presence flags: the kernel resolves the pointers from *ld (step_resolve)
        const float* const yes = reinterpret_cast<const float*>(1);
        sa.mask = a->inpainting_mask_dev ? yes : nullptr; sa.motion = a->inpainted_motion_dev ? yes : nullptr;
        const bool draws = a->sampler != MST_SAMPLER_DDIM_REVERSE && a->sampler != MST_SAMPLER_PLMS;      // the reverse and PLMS steps have no noise term: noise_mode, seed, noise_dev, mask_noise are not read
        sa.noise = draws && a->noise_mode == MST_NOISE_BUFFER ? yes : nullptr;
        sa.scale = a->scale_dev ? yes : nullptr; sa.xstart = a->xstart_dump_dev ? reinterpret_cast<float*>(1) : nullptr;
        sa.clip0 = (unsigned)c0; sa.mask_noise = draws ? a->mask_noise : 0; sa.clip = a->clip_denoised;
        sa.philox = draws && a->noise_mode == MST_NOISE_PHILOX;
        sa.ld = e->ld_dev; sa.joff = joff; sa.eo = eo; sa.step_stride = p.clip_elems;
        sa.rowflag = (a->inpainting_mask_dev && a->inpainted_motion_dev) ? e->rowflag + (size_t)c0 * e->cfg.feats : nullptr;
        switch (step_mode(a->sampler, p.gd != nullptr)) {
#define OUT(M_) case M_: return launch_out_nt<M_>(e, ws, a->cfg, nb, a->frames, nullptr, sa, ss, nullptr, nullptr, 1, frames_next, true, next);
            OUT(1) OUT(2) OUT(3) OUT(4) OUT(5) OUT(6)
#undef OUT
        }
        return fail("mst_sample_loop: no step kernel for sampler %d", a->sampler);
    });
}
// The step that opens a PLMS chain of order > 1 (Pseudo Improved Euler, gaussian_diffusion.py:1134-1141): once per chain, so not fused.
// Per slice, on its stream: the model at (x, t_start) through the model-output-only projection (MODE 0), k_plms_epilogue's first half
// (x <- x_mid, ring slot 0 <- eps, x0-hat dump entry 0 <- pred, ring slot 1 <- the original x: free until chain step 1 writes it), the
// model at (x_mid, t_start - 1) -- the loop's step 1 as far as the conditioning token is concerned -- and k_plms_euler (x <- the sample).
// Always enqueued from the host; the step behind it starts from x in memory (no chained frame rows, no pre-embedded stream).
static int enqueue_plms_warmup(mst_engine* e, const LoopPlan& p, const mst_plms_args* pl) {
    const mst_loop_args* a = p.a;
    const int gx = (int)((p.per_clip + 255) / 256);
    return for_each_slice(e, p, p.nsl, [&](const SliceCtx& c) -> int {
        const auto& [c0, nb, eo, ws, ss, style, tp] = c;
        float* const out = e->plms_out + eo;
        float* const x = a->x_dev + eo;
        float* const h0 = pl->hist_dev + eo;
        float* const h1 = h0 + p.clip_elems;
        const bool blend = a->inpainting_mask_dev && a->inpainted_motion_dev;
        const float* const mask = blend ? a->inpainting_mask_dev + eo : nullptr;
        const float* const motion = blend ? a->inpainted_motion_dev + eo : nullptr;
        for (int half = 0; half < 2; half++) {
            LoopRef lr{e->ld_dev, half, eo, false, false};
            CHECK(run_trunk(e, ws, nullptr, nb, a->cfg ? 2 * nb : nb, a->frames, 0, 0, ss, tp, style, a->batch, lr));
            StepArgs sa{};
            sa.scale = a->scale_dev ? a->scale_dev + c0 : nullptr;
            CHECK(launch_out_nt<0>(e, ws, a->cfg, nb, a->frames, out, sa, ss, nullptr, nullptr, 1, false, true));
            if (half == 0)
                hipLaunchKernelGGL(k_plms_epilogue<0>, dim3(gx, nb), dim3(256), 0, ss, p.s->tab, p.s->n, out, x, mask, motion, (const long long*)nullptr,
                                   a->t_start, (long long)p.per_clip, a->clip_denoised, 0, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                                   x, a->xstart_dump_dev ? a->xstart_dump_dev + eo : nullptr, h0, h1);
            else
                hipLaunchKernelGGL(k_plms_euler<0>, dim3(gx, nb), dim3(256), 0, ss, p.s->tab, p.s->n, out, x, h1, h0, mask, motion, (const long long*)nullptr,
                                   a->t_start, (long long)p.per_clip, a->clip_denoised, x);
            HIPCHECK(hipGetLastError());
        }
        return 0;
    });
}
static int fork_slices(mst_engine* e, const LoopPlan& p) {
    HIPCHECK(hipEventRecord(e->ev_fork, p.streams[0]));
    for (int i = 1; i < p.nsl; i++) HIPCHECK(hipStreamWaitEvent(p.streams[i], e->ev_fork, 0));
    return 0;
}
static int join_slices(mst_engine* e, const LoopPlan& p) {
    for (int i = 1; i < p.nsl; i++) {
        HIPCHECK(hipEventRecord(e->ev_join[i - 1], p.streams[i]));
        HIPCHECK(hipStreamWaitEvent(p.streams[0], e->ev_join[i - 1], 0));
    }
    return 0;
}

// The reference's per-step Python loop (gaussian_diffusion.py:775-794) as ONE call.  Steps are either enqueued from the host
// (short loops, instrumented runs) or replayed from a captured hipGraph of `graph_steps` steps: every kernel reads its
// tensors and its step index through the LoopDev block in device memory, which a one-thread kernel at the end of the graph
// advances, so the instantiated graph is reused by every replay and by every later call with the same shapes.
// pl: the PLMS chain state (mst_sample_loop_plms; a->sampler is then MST_SAMPLER_PLMS), null for every other sampler.
// gd: the guide (mst_sample_loop_guided, which has checked it; MST_SAMPLER_DDPM / MST_SAMPLER_DDIM only), null for an unguided loop.
// wp: the window plan, null otherwise.  mst_sample_loop_windows (MST_SAMPLER_DDIM at eta 0, no guide) and mst_window_sample_loop
//     (MST_SAMPLER_DDPM, or MST_SAMPLER_DDIM at any eta, with or without gd; a step with a noise term reads buffer noise that
//     mst_window_noise drew in long-clip coordinates) have checked it against the call.
//     Every step is then enqueued from the host and reads x from memory -- no graph, no chained frame rows, no fused embed: each would
//     hand step j + 1 rows that the stitch has since changed -- and behind every step the slices join, k_window_stitch runs on the loop
//     stream and the slices fork again.  With a null plan nothing below differs from what it enqueued before the plan existed.
static int window_stitch_launch(const mst_window_plan* wp, float* win, int feats, float* long_out, hipStream_t st);
static float* window_plan_fold(const mst_window_plan* wp);
static int sample_loop_run(mst_engine* e, const mst_schedule* s, const mst_loop_args* a, const mst_plms_args* pl, void* stream,
                           const mst_guide_args* gd = nullptr, const mst_window_plan* wp = nullptr) {
    if (!s || !a) return fail("mst_sample_loop: null argument");
    CHECK(check_ready(e, a->batch, a->frames, a->cfg));
    if (a->sampler == MST_SAMPLER_PLMS && !pl)
        return fail("mst_sample_loop: bad sampler %d: MST_SAMPLER_PLMS carries a history between steps, call mst_sample_loop_plms", a->sampler);
    if (a->sampler != MST_SAMPLER_DDPM && a->sampler != MST_SAMPLER_DDIM && a->sampler != MST_SAMPLER_DDIM_REVERSE && a->sampler != MST_SAMPLER_PLMS)
        return fail("mst_sample_loop: bad sampler %d", a->sampler);
    const bool up = a->sampler == MST_SAMPLER_DDIM_REVERSE;      // ddim_reverse_sample: ascending indices, no noise term
    if (up) {
        if (a->t_start < 0 || a->t_end >= s->n || a->t_start > a->t_end)
            return fail("mst_sample_loop: bad index range %d..%d for %d steps: the reverse sampler runs upward, 0 <= t_start <= t_end <= %d",
                        a->t_start, a->t_end, s->n, s->n - 1);
        if (a->eta != 0.0f) return fail("mst_sample_loop: Reverse ODE only for deterministic path (eta %g must be 0)", (double)a->eta);
    } else if (a->t_start >= s->n || a->t_end < 0 || a->t_start < a->t_end)
        return fail("mst_sample_loop: bad index range %d..%d for %d steps", a->t_start, a->t_end, s->n);
    if (!a->x_dev || (a->cfg && !a->scale_dev)) return fail("mst_sample_loop: null x / scale");
    if (!up && !pl && a->noise_mode == MST_NOISE_BUFFER && !a->noise_dev) return fail("mst_sample_loop: noise buffer missing");
    if (styles_on(e)) CHECK(style_check(e, a->batch, a->frames));
    hipStream_t caller = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    // a PLMS chain of order > 1 opens with the two-evaluation Euler step (enqueue_plms_warmup)
    const bool warm = pl && pl->steps_done == 0 && pl->order > 1;
    if (warm && !e->plms_out) CHECK(dmalloc(&e->plms_out, (size_t)e->cfg.max_rows * e->cfg.feats * e->cfg.max_frames));
    // The loop runs on engine-owned streams: behind everything the caller has enqueued (ev_in), and the caller's stream
    // continues behind the loop (ev_out).  A captured graph needs that: torch's current stream is normally the legacy
    // default stream, which cannot be captured.
    hipStream_t st = e->loop_stream;
    HIPCHECK(hipEventRecord(e->ev_in, caller));
    HIPCHECK(hipStreamWaitEvent(st, e->ev_in, 0));
    const int nrun = (up ? a->t_end - a->t_start : a->t_start - a->t_end) + 1;
    // K1 hoisted: the timestep MLP for every index this loop visits (row r <-> index min(t_start, t_end) + r: a descending loop's step j
    // reads row nrun - 1 - j, an ascending one row j -- CondTok)
    e->prof_now = 0;
    CHECK(ensure_packed(e, st));
    // (a PLMS warm-up evaluates the model at t_start - 1 as well: a one-step call then hoists two rows)
    const int trows = warm && nrun < 2 ? 2 : nrun;
    CHECK(timestep_rows(e, s->tmap + (up ? a->t_start : a->t_start - trows + 1), trows, st));
    // Clips are independent, so the batch runs as `nsplit` slices on separate streams: one slice's kernels fill
    // the CUs the other leaves idle in its prologues, tails and launch gaps (per-launch time is per-CU bound and
    // flat in the block count at this size).  CFG batches are sliced the same way (cond + uncond twins stay together).
    LoopPlan p{s, a, plan_slices(plan_knobs(e), a->batch, a->cfg, a->frames), (size_t)e->cfg.feats * a->frames, (size_t)a->batch * e->cfg.feats * a->frames,
               {st, e->aux_stream[0], e->aux_stream[1], e->aux_stream[2], e->aux_stream[3], e->aux_stream[4], e->aux_stream[5], e->aux_stream[6]}};
    p.gd = gd;
    if (styles_on(e)) CHECK(style_plan(e, a->batch, a->cfg, a->frames, p.nsl, st));     // before the fork: every slice stream is behind it
    // per-call arguments -> device (pinned staging slot; the slot's previous upload has long completed when it comes round again)
    {
        const int slot = e->ld_next;
        e->ld_next = (slot + 1) % mst_engine::LD_SLOTS;
        HIPCHECK(hipEventSynchronize(e->ld_ev[slot]));
        LoopDev& h = e->ld_pin[slot];
        h = LoopDev{a->x_dev, a->inpainting_mask_dev, a->inpainted_motion_dev, a->noise_dev, a->scale_dev, a->xstart_dump_dev,
                    a->seed, a->eta, a->t_start, trows, 0, up ? 1 : 0,
                    pl ? pl->hist_dev : nullptr, (unsigned long long)p.clip_elems, pl ? pl->order : 0, pl ? pl->steps_done : 0,
                    gd ? gd->kind : 0, gd ? gd->follow_schedule : 0, gd ? gd->grad_dev : nullptr, gd ? gd->target_dev : nullptr,
                    gd ? gd->mask_dev : nullptr, gd ? gd->weight_dev : nullptr, s->var};
        HIPCHECK(hipMemcpyAsync(e->ld_dev, &h, sizeof(LoopDev), hipMemcpyHostToDevice, st));
        HIPCHECK(hipEventRecord(e->ld_ev[slot], st));
    }
    if (a->inpainting_mask_dev && a->inpainted_motion_dev) {      // once per loop: which mask rows the step kernel may skip
        const int rows_m = a->batch * e->cfg.feats;
        hipLaunchKernelGGL(k_mask_rowflags, dim3((rows_m + 3) / 4), dim3(256), 0, st, a->inpainting_mask_dev, rows_m, a->frames, e->rowflag);
        HIPCHECK(hipGetLastError());
    }
    // what a captured graph depends on (everything else reaches the kernels through LoopDev)
    const int U = e->graph_steps;
    std::vector<long long> key = {a->batch, a->frames, a->cfg, a->sampler, a->noise_mode, a->mask_noise, a->clip_denoised,
                                  a->inpainting_mask_dev != nullptr, a->inpainted_motion_dev != nullptr, a->xstart_dump_dev != nullptr,
                                  a->scale_dev != nullptr, p.nsl, U, (long long)(size_t)s->tab, s->n, e->embed_fast, gd != nullptr};
    const PlanKnobs knobs = plan_knobs(e);     // ... and every switch the launch plan reads, word by word: a knob added to PlanKnobs is in the key
    key.insert(key.end(), reinterpret_cast<const int*>(&knobs), reinterpret_cast<const int*>(&knobs) + PLAN_KNOB_WORDS);
    const int j0 = warm ? 1 : 0;                              // the warm-up is the call's step 0
    const bool use_graph = e->graph_on && !wp && !e->prof_on && e->dbg_stage < 0 && nrun - j0 >= 2 * U;
    bool forked = false;
    auto steps = [&]() -> int {
        int j = 0;
        if (warm) {
            if (p.nsl > 1) { CHECK(fork_slices(e, p)); forked = true; }
            CHECK(enqueue_plms_warmup(e, p, pl));
            j = 1;
        }
        if (use_graph) {
            // head of the loop from the host: the remainder, plus one graph's worth of steps the first time a configuration is
            // seen (every kernel's per-device LDS opt-in must have happened before a capture)
            int pre = (nrun - j0) % U;
            if (e->warm_key != key) pre += U;
            pre += j0;
            if (p.nsl > 1 && !forked) { CHECK(fork_slices(e, p)); forked = true; }
            for (; j < pre; j++) CHECK(enqueue_step(e, p, j, p.nsl));
            if (forked) { CHECK(join_slices(e, p)); forked = false; }
            e->warm_key = key;
            if (pre > 0) {
                hipLaunchKernelGGL(k_loop_advance, dim3(1), dim3(1), 0, st, e->ld_dev, pre);
                HIPCHECK(hipGetLastError());
            }
            if (e->gkey != key || !e->gexec) {
                if (e->gexec) { (void)hipGraphExecDestroy(e->gexec); e->gexec = nullptr; }
                e->gkey.clear();
                HIPCHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
                int rc = 0;
                if (p.nsl > 1) rc = fork_slices(e, p);
                for (int k = 0; k < U && !rc; k++) rc = enqueue_step(e, p, k, p.nsl);
                if (!rc && p.nsl > 1) rc = join_slices(e, p);
                if (!rc) {
                    hipLaunchKernelGGL(k_loop_advance, dim3(1), dim3(1), 0, st, e->ld_dev, U);
                    if (hipGetLastError() != hipSuccess) rc = fail("mst_sample_loop: capture of the step-counter kernel failed");
                }
                hipGraph_t graph = nullptr;
                const hipError_t ce = hipStreamEndCapture(st, &graph);          // always end the capture: the stream must come back
                if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
                if (ce != hipSuccess || !graph) return fail("mst_sample_loop: stream capture failed: %s", hipGetErrorString(ce));
                const hipError_t ie = hipGraphInstantiate(&e->gexec, graph, nullptr, nullptr, 0);
                (void)hipGraphDestroy(graph);
                if (ie != hipSuccess) { e->gexec = nullptr; return fail("mst_sample_loop: hipGraphInstantiate failed: %s", hipGetErrorString(ie)); }
                e->gkey = key;
            }
            for (; j < nrun; j += U) HIPCHECK(hipGraphLaunch(e->gexec, st));
            return 0;
        }
        // Host-enqueued steps chain their frame rows: step j's epilogue writes the f16 rows step j + 1 embeds, so only step 0 runs
        // the transpose kernel.  Not under CFG (there a slice's rows sit at 2 x its first clip, which changes when an instrumented
        // step runs as one slice), not for frame counts the epilogue walks element-wise, not in captured graphs (their first
        // step would have to differ from call to call).
        const bool chain = e->fuse_frames && !wp && !a->cfg && (a->frames & 3) == 0 && e->dbg_stage < 0;
        // ... and where the shapes allow, step j's output projection embeds step j + 1 in the same launch (MST_FUSE_EMBED=0: frame rows
        // only).  Instrumented steps and their neighbours keep the two kernels apart, so that the event-timed families stay what they say.
        const bool fuse_embed = chain && e->fuse_embed && embed_next_fits(e, a->frames);
        auto instrumented = [&](int jj) { return e->prof_on && (jj % e->prof_period == 0); };
        bool stream_ready = false;
        for (; j < nrun; j++) {
            e->prof_now = e->prof_on && (j % e->prof_period == 0);
            // instrumented steps run as ONE full-batch slice so the HIP-event durations are those of isolated
            // full-batch launches (the roofline figures); all other steps use the concurrent slices
            const int nsj = e->prof_now ? 1 : p.nsl;
            if (nsj > 1 && !forked) { CHECK(fork_slices(e, p)); forked = true; }
            else if (nsj == 1 && forked) { CHECK(join_slices(e, p)); forked = false; }
            const bool embed_next = fuse_embed && j + 1 < nrun && !instrumented(j) && !instrumented(j + 1);
            CHECK(enqueue_step(e, p, j, nsj, chain && j > j0 && !stream_ready, chain && j + 1 < nrun && !embed_next, stream_ready, embed_next));
            stream_ready = embed_next;
            if (wp) {      // the windows' shared frames -> one value each, on the loop stream behind every slice; the last stitch is the fold
                if (forked) { CHECK(join_slices(e, p)); forked = false; }
                CHECK(window_stitch_launch(wp, a->x_dev, e->cfg.feats, j + 1 == nrun ? window_plan_fold(wp) : nullptr, st));
            }
        }
        return 0;
    };
    const int rc = steps();
    // join the slice streams whatever happened: after an error mid-loop the slices' work is still in flight on the
    // caller's tensors, so the caller's stream must not run ahead of it (best effort: errors here are not reported twice)
    if (forked) {
        for (int i = 1; i < p.nsl; i++) {
            if (hipEventRecord(e->ev_join[i - 1], p.streams[i]) == hipSuccess) (void)hipStreamWaitEvent(st, e->ev_join[i - 1], 0);
        }
    }
    e->prof_now = 0;
    if (hipEventRecord(e->ev_out, st) == hipSuccess) (void)hipStreamWaitEvent(caller, e->ev_out, 0);
    return trunk_settle(e, st, rc);
}

extern "C" int mst_sample_loop(mst_engine* e, const mst_schedule* s, const mst_loop_args* a, void* stream) {
    return sample_loop_run(e, s, a, nullptr, stream);
}

extern "C" int mst_sample_loop_plms(mst_engine* e, const mst_schedule* s, const mst_loop_args* a, const mst_plms_args* pl, void* stream) {
    if (!s || !a || !pl) return fail("mst_sample_loop_plms: null argument");
    if (pl->order < 1 || pl->order > 4) return fail("mst_sample_loop_plms: order %d is invalid (should be int from 1-4)", pl->order);
    if (pl->steps_done < 0) return fail("mst_sample_loop_plms: steps_done %d is negative", pl->steps_done);
    if (pl->order > 1 && !pl->hist_dev) return fail("mst_sample_loop_plms: order %d needs the eps history ring (hist_dev is NULL)", pl->order);
    if (pl->order > 1 && pl->steps_done == 0 && a->t_start == 0)
        return fail("mst_sample_loop_plms: a chain of order %d cannot start at index 0: its first step evaluates the model at index t - 1", pl->order);
    mst_loop_args b = *a;
    b.sampler = MST_SAMPLER_PLMS;
    b.eta = 0.0f;
    b.noise_mode = MST_NOISE_PHILOX;                         // (no noise term: nothing is drawn, no buffer is read)
    b.noise_dev = nullptr;
    b.seed = 0;
    b.mask_noise = 0;
    return sample_loop_run(e, s, &b, pl, stream);
}

static_assert(MST_GUIDE_GRADIENT == GUIDE_GRADIENT && MST_GUIDE_TARGET == GUIDE_TARGET, "the kernels' guide kinds are the ABI's");
static int guide_check(const char* who, const mst_schedule* s, int sampler, const mst_guide_args* g) {
    if (sampler == MST_SAMPLER_DDIM_REVERSE)
        return fail("%s: MST_SAMPLER_DDIM_REVERSE takes no guide: the reference's ddim_reverse_sample has no cond_fn", who);
    if (sampler == MST_SAMPLER_PLMS) return fail("%s: MST_SAMPLER_PLMS takes no guide: guided PLMS is not built", who);
    if (sampler != MST_SAMPLER_DDPM && sampler != MST_SAMPLER_DDIM) return fail("%s: bad sampler %d", who, sampler);
    if (g->kind == MST_GUIDE_GRADIENT) {
        if (!g->grad_dev) return fail("%s: MST_GUIDE_GRADIENT needs grad_dev (NULL)", who);
    } else if (g->kind == MST_GUIDE_TARGET) {
        if (!g->target_dev) return fail("%s: MST_GUIDE_TARGET needs target_dev (NULL)", who);
        if (!g->weight_dev) return fail("%s: MST_GUIDE_TARGET needs weight_dev (NULL)", who);
    } else
        return fail("%s: bad guide kind %d (MST_GUIDE_GRADIENT = 1, MST_GUIDE_TARGET = 2)", who, g->kind);
    if (sampler == MST_SAMPLER_DDPM && !s->var)
        return fail("%s: a guided MST_SAMPLER_DDPM step needs the schedule's variance row: call mst_schedule_set_variance", who);
    return 0;
}

// The guide of a whole loop (mst_sample_loop_guided, mst_window_sample_loop): guide_check, and a caller's gradient belongs to one step.
static int loop_guide_check(const char* who, const mst_schedule* s, const mst_loop_args* a, const mst_guide_args* g) {
    CHECK(guide_check(who, s, a->sampler, g));
    if (g->kind == MST_GUIDE_GRADIENT && a->t_start != a->t_end)
        return fail("%s: MST_GUIDE_GRADIENT carries the gradient of ONE step: t_start %d must equal t_end %d", who, a->t_start, a->t_end);
    return 0;
}

// p_sample_loop / ddim_sample_loop with a cond_fn (gaussian_diffusion.py:644-794 / :948-1082 with :577-580 / :821-824).
extern "C" int mst_sample_loop_guided(mst_engine* e, const mst_schedule* s, const mst_loop_args* a, const mst_guide_args* g, void* stream) {
    if (!s || !a || !g) return fail("mst_sample_loop_guided: null argument");
    CHECK(loop_guide_check("mst_sample_loop_guided", s, a, g));
    return sample_loop_run(e, s, a, nullptr, stream, g);
}

// ------------------------------------------------------------------------------------------ windows ABI (mst_window.h)
// One plan = the cut of `clips` long clips [C,F,1,L] into `windows` windows [N,F,1,W]; the feature count is a call's, not the plan's.
struct mst_window_plan {
    int device = 0, clips = 0, windows = 0, window = 0, long_frames = 0;
    int* dev = nullptr;                      // ONE allocation: clip_len [C] | win_clip [N] | win_start [N] | cover [C * L] {first, count}
    const int *clip_len = nullptr, *win_clip = nullptr, *win_start = nullptr;
    const WinCover* cover = nullptr;
    float* fold_dev = nullptr;               // mst_window_plan_set_fold: where mst_sample_loop_windows' last stitch writes the long clips
};

extern "C" int mst_window_max_frames(void) { return kWinMaxFrames; }

extern "C" int mst_window_plan_create(const int32_t* clip_len, const int32_t* clip_win0, const int32_t* win_start, int32_t clips, int32_t windows,
                                      int32_t window, int32_t long_frames, int32_t device, mst_window_plan** out) {
    const char* who = "mst_window_plan_create";
    if (!clip_len || !clip_win0 || !win_start || !out) return fail("%s: null argument", who);
    if (clips < 1 || windows < clips) return fail("%s: %d windows for %d clips (every clip has at least one window)", who, windows, clips);
    if (window < 1) return fail("%s: window %d must be at least 1 frame", who, window);
    if (long_frames < 1 || long_frames > kWinMaxFrames)
        return fail("%s: long_frames %d outside 1..%d (mst_window_max_frames)", who, long_frames, kWinMaxFrames);
    if (clip_win0[0] != 0 || clip_win0[clips] != windows)
        return fail("%s: clip_win0 must run from 0 to the window count %d (got %d .. %d)", who, windows, clip_win0[0], clip_win0[clips]);
    std::vector<int> host((size_t)clips + 2 * (size_t)windows + 2 * (size_t)clips * long_frames, 0);
    int* const h_len = host.data();
    int* const h_clip = h_len + clips;
    int* const h_start = h_clip + windows;
    WinCover* const h_cov = reinterpret_cast<WinCover*>(h_start + windows);
    for (int c = 0; c < clips; c++) {
        const int len = clip_len[c], n0 = clip_win0[c], n1 = clip_win0[c + 1];
        if (len < 1 || len > long_frames) return fail("%s: clip %d: length %d outside 1..long_frames %d", who, c, len, long_frames);
        if (n1 <= n0 || n1 > windows) return fail("%s: clip %d: clip_win0 %d .. %d names no window (it must ascend, within %d windows)", who, c, n0, n1, windows);
        const int reach = len > window ? len : window;      // a clip no longer than the window: one window at 0, zero padding behind the clip
        int covered = 0;                                    // frames [0, covered) are covered by the windows seen so far
        for (int n = n0; n < n1; n++) {
            const int st = win_start[n];
            if (st < 0) return fail("%s: clip %d: window %d starts at %d (negative)", who, c, n, st);
            if (n > n0 && st <= win_start[n - 1])
                return fail("%s: clip %d: window starts must be strictly ascending (window %d starts at %d behind %d)", who, c, n, st, win_start[n - 1]);
            if ((long long)st + window > reach)
                return fail("%s: clip %d: window %d covers frames %d .. %d past max(length %d, window %d): start + W <= max(len, W)", who, c, n, st,
                            st + window - 1, len, window);
            if (st > covered) return fail("%s: clip %d: uncovered frame %d (window %d starts at %d)", who, c, covered, n, st);
            covered = st + window;
            h_clip[n] = c;
            h_start[n] = st;
        }
        if (covered < len) return fail("%s: clip %d: uncovered frame %d (the last window ends there, the clip is %d frames long)", who, c, covered, len);
        h_len[c] = len;
        // the covering run of every frame below the length: both ends only move forward
        int lo = n0, hi = n0;                               // windows [lo, hi) cover f
        for (int f = 0; f < len; f++) {
            while (hi < n1 && win_start[hi] <= f) hi++;
            while (lo < hi && win_start[lo] + window <= f) lo++;
            h_cov[(size_t)c * long_frames + f] = WinCover{lo, hi - lo};
        }
    }
    ON_DEVICE(device);
    mst_window_plan* p = new mst_window_plan();
    p->device = device; p->clips = clips; p->windows = windows; p->window = window; p->long_frames = long_frames;
    if (hipMalloc(&p->dev, host.size() * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        delete p;
        return fail("%s: out of device memory (%zu bytes) or no device %d", who, host.size() * sizeof(int), device);
    }
    if (hipMemcpy(p->dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {      // the one upload
        (void)hipGetLastError();
        (void)hipFree(p->dev);
        delete p;
        return fail("%s: the upload of the plan failed", who);
    }
    p->clip_len = p->dev;
    p->win_clip = p->dev + clips;
    p->win_start = p->win_clip + windows;
    p->cover = reinterpret_cast<const WinCover*>(p->win_start + windows);
    *out = p;
    return 0;
}

extern "C" void mst_window_plan_destroy(mst_window_plan* p) {
    if (!p) return;
    DeviceGuard g(p->device);
    if (p->dev) (void)hipFree(p->dev);
    delete p;
}

extern "C" int mst_window_plan_set_fold(mst_window_plan* p, float* long_out_dev) {
    if (!p) return fail("mst_window_plan_set_fold: null plan");
    p->fold_dev = long_out_dev;
    return 0;
}
static float* window_plan_fold(const mst_window_plan* wp) { return wp->fold_dev; }

static int window_blocks(const char* who, size_t elems, unsigned* blocks) {
    const size_t b = (elems + kWinThreads - 1) / kWinThreads;
    if (b > 0x7fffffffu) return fail("%s: %zu elements are more than one launch takes", who, elems);
    *blocks = (unsigned)b;
    return 0;
}

extern "C" int mst_window_unfold(const mst_window_plan* p, const float* long_dev, int32_t feats, float* win_dev, void* stream) {
    if (!p || !long_dev || !win_dev) return fail("mst_window_unfold: null argument");
    if (feats < 1) return fail("mst_window_unfold: feats %d must be at least 1", feats);
    unsigned blocks = 0;
    CHECK(window_blocks("mst_window_unfold", (size_t)p->windows * feats * p->window, &blocks));
    ON_DEVICE(p->device);
    hipLaunchKernelGGL(k_window_unfold, dim3(blocks), dim3(kWinThreads), 0, (hipStream_t)stream, long_dev, p->clip_len, p->win_clip, p->win_start,
                       p->windows, feats, p->window, p->long_frames, win_dev);
    HIPCHECK(hipGetLastError());
    return 0;
}

static int window_stitch_launch(const mst_window_plan* p, float* win, int feats, float* long_out, hipStream_t st) {
    unsigned blocks = 0;
    CHECK(window_blocks("mst_window_stitch", (size_t)p->clips * feats * p->long_frames, &blocks));
    hipLaunchKernelGGL(k_window_stitch, dim3(blocks), dim3(kWinThreads), 0, st, win, p->cover, p->win_start, p->clips, feats, p->window,
                       p->long_frames, long_out);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_window_stitch(const mst_window_plan* p, float* win_dev, int32_t feats, float* long_out_dev, void* stream) {
    if (!p || !win_dev) return fail("mst_window_stitch: null argument");
    if (feats < 1) return fail("mst_window_stitch: feats %d must be at least 1", feats);
    ON_DEVICE(p->device);
    return window_stitch_launch(p, win_dev, feats, long_out_dev, (hipStream_t)stream);
}

// What both windowed loops ask of their plan: the loop's batch is the plan's windows, on the engine's device.
static int window_plan_check(const char* who, const mst_engine* e, const mst_loop_args* a, const mst_window_plan* p) {
    if (a->batch != p->windows) return fail("%s: batch %d is not the plan's window count %d", who, a->batch, p->windows);
    if (a->frames != p->window) return fail("%s: frames %d is not the plan's window %d", who, a->frames, p->window);
    if (p->device != e->cfg.device) return fail("%s: the plan lives on device %d, the engine on device %d", who, p->device, e->cfg.device);
    return 0;
}

// ddim_sample_loop over every window of every long clip as ONE batch, stitched behind every step (sample_loop_run with a plan): the
// deterministic subset of mst_window_sample_loop over the same code, with its own two refusals in front.
extern "C" int mst_sample_loop_windows(mst_engine* e, const mst_schedule* s, const mst_loop_args* a, const mst_window_plan* p, void* stream) {
    const char* who = "mst_sample_loop_windows";
    if (!e || !s || !a || !p) return fail("%s: null argument", who);
    if (a->sampler != MST_SAMPLER_DDIM)
        return fail("%s: sampler %d is not MST_SAMPLER_DDIM: only the deterministic DDIM step keeps the windows' shared frames identical", who, a->sampler);
    if (a->eta != 0.0f) return fail("%s: eta %g must be 0: a stochastic step would need per-window noise unfolded from one long draw", who, (double)a->eta);
    CHECK(window_plan_check(who, e, a, p));
    return sample_loop_run(e, s, a, nullptr, stream, nullptr, p);
}

// The noise of stochastic windowed steps, drawn in long-clip coordinates (k_window_noise): out [nsteps,N,F,1,W], entry j =
// unfold(mst_philox_normal(C, F, L, seed, step0 + j)) -- what an MST_NOISE_BUFFER loop of mst_window_sample_loop reads.
extern "C" int mst_window_noise(const mst_window_plan* p, int32_t feats, uint64_t seed, uint32_t step0, int32_t nsteps, float* out_dev,
                                void* stream) {
    const char* who = "mst_window_noise";
    if (feats < 1) return fail("%s: feats %d must be at least 1", who, feats);
    if (nsteps < 1) return fail("%s: nsteps %d must be at least 1", who, nsteps);
    if (!p) return fail("%s: null plan", who);
    if (!out_dev) return fail("%s: null out", who);
    const int quads = ((p->long_frames > p->window ? p->long_frames : p->window) + 3) / 4;
    unsigned blocks = 0;
    CHECK(window_blocks(who, (size_t)nsteps * p->clips * feats * quads, &blocks));
    ON_DEVICE(p->device);
    hipLaunchKernelGGL(k_window_noise, dim3(blocks), dim3(kWinThreads), 0, (hipStream_t)stream, p->cover, p->clip_len, p->win_start, p->clips,
                       p->windows, feats, p->window, p->long_frames, quads, nsteps, (unsigned long long)seed, (unsigned)step0, out_dev);
    HIPCHECK(hipGetLastError());
    return 0;
}

// p_sample_loop / ddim_sample_loop (any eta), with or without a guide, over every window of every long clip as ONE batch, stitched
// behind every step: mst_sample_loop_windows (which stays the deterministic subset, refusals included) extended by the noise term and
// by mst_sample_loop_guided's guide.
extern "C" int mst_window_sample_loop(mst_engine* e, const mst_schedule* s, const mst_loop_args* a, const mst_window_plan* p,
                                      const mst_guide_args* g, void* stream) {
    const char* who = "mst_window_sample_loop";
    if (!e || !s || !a || !p) return fail("%s: null argument", who);
    if (a->sampler != MST_SAMPLER_DDPM && a->sampler != MST_SAMPLER_DDIM)
        return fail("%s: sampler %d is neither MST_SAMPLER_DDPM nor MST_SAMPLER_DDIM: PLMS and the reverse DDIM step over windows are not built",
                    who, a->sampler);
    if (a->sampler == MST_SAMPLER_DDPM || a->eta != 0.0f) {      // the step has a noise term
        if (a->noise_mode == MST_NOISE_PHILOX)
            return fail("%s: MST_NOISE_PHILOX with a noise term: the in-kernel draw is keyed by window, so windows that share a long frame "
                        "would draw different numbers for it; fill a buffer with mst_window_noise and pass MST_NOISE_BUFFER", who);
        if (!a->noise_dev) return fail("%s: noise buffer missing (mst_window_noise fills one)", who);
    }
    CHECK(window_plan_check(who, e, a, p));
    if (g) CHECK(loop_guide_check(who, s, a, g));
    return sample_loop_run(e, s, a, nullptr, stream, g, p);
}

// ------------------------------------------------------------------------------------------ elementwise ABI
extern "C" int mst_q_sample(const mst_schedule* s, const float* x0, const float* noise, const float* mask, const int64_t* t,
                            int32_t batch, int64_t per_clip, float* out, void* stream) {
    if (!s || !x0 || !noise || !t || !out || batch < 1 || per_clip < 1) return fail("mst_q_sample: bad arguments");
    ON_DEVICE(s->device);
    int gx = (int)((per_clip + 255) / 256);
    if (gx > 2048) gx = 2048;
    hipLaunchKernelGGL(k_q_sample, dim3(gx, batch), dim3(256), 0, (hipStream_t)stream, s->tab, s->n, x0, noise, mask,
                       (const long long*)t, (long long)per_clip, out);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_step_epilogue_mt(const mst_schedule* s, const float* model_out, const float* x, const float* noise,
                                    const float* mask, const float* motion, const int64_t* t, int32_t batch, int64_t per_clip,
                                    int32_t sampler, int32_t mean_type, float eta, int32_t mask_noise, int32_t clip_denoised, float* sample,
                                    float* xstart, void* stream) {
    if (!s || !model_out || !x || !t || batch < 1 || per_clip < 1) return fail("mst_step_epilogue: bad arguments");
    if (sampler != MST_SAMPLER_DDPM && sampler != MST_SAMPLER_DDIM && sampler != MST_SAMPLER_DDIM_REVERSE)
        return fail("mst_step_epilogue: bad sampler %d", sampler);
    if (sampler == MST_SAMPLER_DDIM_REVERSE && eta != 0.0f)
        return fail("mst_step_epilogue: Reverse ODE only for deterministic path (eta %g must be 0)", (double)eta);
    if (mean_type < 0 || mean_type > 2) return fail("mst_step_epilogue: bad mean type %d (0 = x_start, 1 = epsilon, 2 = previous x)", mean_type);
    ON_DEVICE(s->device);
    int gx = (int)((per_clip + 255) / 256);
    if (gx > 2048) gx = 2048;
#define STEP_LAUNCH(S_, M_)                                                                                                              \
    hipLaunchKernelGGL((k_step_epilogue<S_, M_>), dim3(gx, batch), dim3(256), 0, (hipStream_t)stream, s->tab, s->n, eta, model_out, x,   \
                       noise, mask, motion, (const long long*)t, (long long)per_clip, mask_noise, clip_denoised, sample, xstart)
    const bool ddim = sampler == MST_SAMPLER_DDIM, rev = sampler == MST_SAMPLER_DDIM_REVERSE;      // (rev: `noise` is never read, may be null)
    switch (mean_type) {
        case 0: if (rev) STEP_LAUNCH(2, 0); else if (ddim) STEP_LAUNCH(1, 0); else STEP_LAUNCH(0, 0); break;
        case 1: if (rev) STEP_LAUNCH(2, 1); else if (ddim) STEP_LAUNCH(1, 1); else STEP_LAUNCH(0, 1); break;
        default: if (rev) STEP_LAUNCH(2, 2); else if (ddim) STEP_LAUNCH(1, 2); else STEP_LAUNCH(0, 2); break;
    }
#undef STEP_LAUNCH
    HIPCHECK(hipGetLastError());
    return 0;
}
extern "C" int mst_step_epilogue(const mst_schedule* s, const float* model_out, const float* x, const float* noise,
                                 const float* mask, const float* motion, const int64_t* t, int32_t batch, int64_t per_clip,
                                 int32_t sampler, float eta, int32_t mask_noise, int32_t clip_denoised, float* sample,
                                 float* xstart, void* stream) {
    return mst_step_epilogue_mt(s, model_out, x, noise, mask, motion, t, batch, per_clip, sampler, 0, eta, mask_noise, clip_denoised, sample,
                                xstart, stream);
}

// p_sample / ddim_sample with a cond_fn given the model output (gaussian_diffusion.py:577-580 / :821-846).
extern "C" int mst_step_epilogue_guided(const mst_schedule* s, const float* model_out, const float* x, const float* noise,
                                        const float* mask, const float* motion, const int64_t* t, int32_t batch, int64_t per_clip,
                                        int32_t sampler, int32_t mean_type, float eta, int32_t mask_noise, int32_t clip_denoised,
                                        const mst_guide_args* g, float* sample, float* xstart, void* stream) {
    if (!s || !model_out || !x || !t || !g || batch < 1 || per_clip < 1) return fail("mst_step_epilogue_guided: bad arguments");
    CHECK(guide_check("mst_step_epilogue_guided", s, sampler, g));
    if (mean_type < 0 || mean_type > 2) return fail("mst_step_epilogue_guided: bad mean type %d (0 = x_start, 1 = epsilon, 2 = previous x)", mean_type);
    ON_DEVICE(s->device);
    int gx = (int)((per_clip + 255) / 256);
    if (gx > 2048) gx = 2048;
#define GSTEP_LAUNCH(S_, M_)                                                                                                             \
    hipLaunchKernelGGL((k_step_epilogue_guided<S_, M_>), dim3(gx, batch), dim3(256), 0, (hipStream_t)stream, s->tab, s->var, s->n, eta,  \
                       model_out, x, noise, mask, motion, (const long long*)t, (long long)per_clip, mask_noise, clip_denoised, g->kind,   \
                       g->grad_dev, g->target_dev, g->mask_dev, g->weight_dev, g->follow_schedule, sample, xstart)
    const bool ddim = sampler == MST_SAMPLER_DDIM;
    switch (mean_type) {
        case 0: if (ddim) GSTEP_LAUNCH(1, 0); else GSTEP_LAUNCH(0, 0); break;
        case 1: if (ddim) GSTEP_LAUNCH(1, 1); else GSTEP_LAUNCH(0, 1); break;
        default: if (ddim) GSTEP_LAUNCH(1, 2); else GSTEP_LAUNCH(0, 2); break;
    }
#undef GSTEP_LAUNCH
    HIPCHECK(hipGetLastError());
    return 0;
}

// plms_sample given the model output (gaussian_diffusion.py:1084-1166).  first_half: the first half of the Euler step instead.
extern "C" int mst_plms_epilogue(const mst_schedule* s, const float* model_out, const float* x, const float* mask, const float* motion,
                                 const int64_t* t, int32_t batch, int64_t per_clip, int32_t mean_type, int32_t clip_denoised, int32_t cur_order,
                                 int32_t first_half, const float* e1, const float* e2, const float* e3, float* sample, float* xstart,
                                 float* eps_out, void* stream) {
    if (!s || !model_out || !x || !t || batch < 1 || per_clip < 1) return fail("mst_plms_epilogue: bad arguments");
    if (mean_type < 0 || mean_type > 2) return fail("mst_plms_epilogue: bad mean type %d (0 = x_start, 1 = epsilon, 2 = previous x)", mean_type);
    if (!first_half) {
        if (cur_order < 1 || cur_order > 4) return fail("mst_plms_epilogue: cur_order %d is invalid (should be int from 1-4)", cur_order);
        if ((cur_order >= 2 && !e1) || (cur_order >= 3 && !e2) || (cur_order >= 4 && !e3))
            return fail("mst_plms_epilogue: cur_order %d needs %d history entries", cur_order, cur_order - 1);
    }
    ON_DEVICE(s->device);
    const int gx = (int)((per_clip + 255) / 256), co = first_half ? 0 : cur_order;
#define PLMS_LAUNCH(M_)                                                                                                                  \
    hipLaunchKernelGGL(k_plms_epilogue<M_>, dim3(gx, batch), dim3(256), 0, (hipStream_t)stream, s->tab, s->n, model_out, x, mask, motion, \
                       (const long long*)t, 0, (long long)per_clip, clip_denoised, co, e1, e2, e3, sample, xstart, eps_out, (float*)nullptr)
    switch (mean_type) { case 0: PLMS_LAUNCH(0); break; case 1: PLMS_LAUNCH(1); break; default: PLMS_LAUNCH(2); break; }
#undef PLMS_LAUNCH
    HIPCHECK(hipGetLastError());
    return 0;
}
// The second half of the Euler step: model_out is the model at (x_mid, t - 1); t holds the step's own indices (every one >= 1).
extern "C" int mst_plms_euler(const mst_schedule* s, const float* model_out, const float* x_mid, const float* x, const float* eps,
                              const float* mask, const float* motion, const int64_t* t, int32_t batch, int64_t per_clip, int32_t mean_type,
                              int32_t clip_denoised, float* sample, void* stream) {
    if (!s || !model_out || !x_mid || !x || !eps || !t || !sample || batch < 1 || per_clip < 1) return fail("mst_plms_euler: bad arguments");
    if (mean_type < 0 || mean_type > 2) return fail("mst_plms_euler: bad mean type %d (0 = x_start, 1 = epsilon, 2 = previous x)", mean_type);
    ON_DEVICE(s->device);
    const int gx = (int)((per_clip + 255) / 256);
#define EULER_LAUNCH(M_)                                                                                                                 \
    hipLaunchKernelGGL(k_plms_euler<M_>, dim3(gx, batch), dim3(256), 0, (hipStream_t)stream, s->tab, s->n, model_out, x_mid, x, eps, mask, \
                       motion, (const long long*)t, 0, (long long)per_clip, clip_denoised, sample)
    switch (mean_type) { case 0: EULER_LAUNCH(0); break; case 1: EULER_LAUNCH(1); break; default: EULER_LAUNCH(2); break; }
#undef EULER_LAUNCH
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_step_backward(const mst_schedule* s, const float* g_sample, const float* g_pred, const float* mask,
                                 int32_t has_blend, const int64_t* t, int32_t batch, int64_t per_clip, int32_t sampler, float eta,
                                 const float* pred_clipped, float* d_model_out, void* stream) {
    if (!s || !t || !d_model_out || batch < 1 || per_clip < 1 || (!g_sample && !g_pred) || (has_blend && !mask))
        return fail("mst_step_backward: bad arguments");
    ON_DEVICE(s->device);
    int gx = (int)((per_clip + 255) / 256);
    if (gx > 2048) gx = 2048;
    if (sampler == MST_SAMPLER_DDPM)
        hipLaunchKernelGGL(k_step_backward<0>, dim3(gx, batch), dim3(256), 0, (hipStream_t)stream, s->tab, s->n, eta, g_sample, g_pred, mask,
                           has_blend, (const long long*)t, (long long)per_clip, pred_clipped, d_model_out);
    else if (sampler == MST_SAMPLER_DDIM)
        hipLaunchKernelGGL(k_step_backward<1>, dim3(gx, batch), dim3(256), 0, (hipStream_t)stream, s->tab, s->n, eta, g_sample, g_pred, mask,
                           has_blend, (const long long*)t, (long long)per_clip, pred_clipped, d_model_out);
    else if (sampler == MST_SAMPLER_DDIM_REVERSE)
        return fail("mst_step_backward: MST_SAMPLER_DDIM_REVERSE has no backward: the reference has no _with_grad form of ddim_reverse_sample");
    else if (sampler == MST_SAMPLER_PLMS)
        return fail("mst_step_backward: MST_SAMPLER_PLMS has no backward: the reference has no _with_grad form of plms_sample");
    else
        return fail("mst_step_backward: bad sampler %d", sampler);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_masked_l2(const float* a, int64_t a_stride, const float* b, const float* mask, int64_t mask_stride, int32_t n,
                             int32_t feats, int32_t frames, const float* g, float* out, void* stream) {
    if (!a || !b || !mask || !out || n < 1 || feats < 1 || frames < 1) return fail("mst_masked_l2: bad arguments");
    if (!g)
        hipLaunchKernelGGL(k_masked_l2_fwd, dim3(n), dim3(1024), 0, (hipStream_t)stream, a, (long long)a_stride, b, mask, (long long)mask_stride,
                           feats, frames, out);
    else {
        int gx = (feats * frames + 255) / 256;
        if (gx > 64) gx = 64;
        hipLaunchKernelGGL(k_masked_l2_bwd, dim3(gx, n), dim3(256), 0, (hipStream_t)stream, a, (long long)a_stride, b, mask,
                           (long long)mask_stride, feats, frames, g, out);
    }
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_text_cosine(const float* f, const float* m, int32_t batch, int32_t dim, const float* g, float* out, void* stream) {
    if (!f || !m || !out || batch < 1 || batch > 1024 || dim < 1) return fail("mst_text_cosine: bad arguments (batch 1..1024)");
    hipLaunchKernelGGL(k_text_cosine, dim3(1), dim3(1024), 0, (hipStream_t)stream, f, m, batch, dim, g ? 1 : 0, g, out);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_philox_normal(float* out, int32_t batch, int32_t feats, int32_t frames, uint64_t seed, uint32_t step,
                                 void* stream) {
    if (!out || batch < 1 || feats < 1 || frames < 1) return fail("mst_philox_normal: bad arguments");
    int n = feats * ((frames + 3) / 4);
    hipLaunchKernelGGL(k_philox_normal, dim3((n + 255) / 256, batch), dim3(256), 0, (hipStream_t)stream, out, feats, frames,
                       (unsigned long long)seed, (unsigned)step);
    HIPCHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ variational bound (mst_vb.h)
// A draw needs the clip's layout (the counter is (frame quad, feature, clip, t)); a buffer does not.
static int vb_draw_check(const char* who, int64_t per_clip, int32_t feats, int32_t frames) {
    if (feats < 1 || frames < 1) return fail("%s: a drawn noise (noise_dev NULL) needs feats and frames (got %d, %d)", who, feats, frames);
    if ((int64_t)feats * frames != per_clip)
        return fail("%s: feats %d x frames %d is not per_clip %lld", who, feats, frames, (long long)per_clip);
    if ((int64_t)feats * ((frames + 3) / 4) > 0x7fffffffLL) return fail("%s: feats x frames too large for a drawn noise", who);
    return 0;
}

// q_sample on rows (clip[r], t[r]) (gaussian_diffusion.py:267-285 as calc_bpd_loop calls it, :1573-1574).
extern "C" int mst_vb_diffuse(const mst_schedule* s, const float* x0, const float* noise, const float* mask, const int64_t* clip,
                              const int64_t* t, int32_t rows, int64_t per_clip, int32_t feats, int32_t frames, uint64_t seed, float* out,
                              void* stream) {
    if (!s || !x0 || !clip || !t || !out) return fail("mst_vb_diffuse: null argument");
    if (rows < 1 || per_clip < 1) return fail("mst_vb_diffuse: rows %d and per_clip %lld must be >= 1", rows, (long long)per_clip);
    if (!noise) CHECK(vb_draw_check("mst_vb_diffuse", per_clip, feats, frames));
    ON_DEVICE(s->device);
    if (noise) {
        int gx = (int)((per_clip + 255) / 256);
        if (gx > 2048) gx = 2048;
        hipLaunchKernelGGL(k_vb_diffuse, dim3(gx, rows), dim3(256), 0, (hipStream_t)stream, s->tab, s->n, x0, noise, mask,
                           (const long long*)clip, (const long long*)t, (long long)per_clip, out);
    } else {
        int gx = (int)(((int64_t)feats * ((frames + 3) / 4) + 255) / 256);
        if (gx > 2048) gx = 2048;
        hipLaunchKernelGGL(k_vb_diffuse_draw, dim3(gx, rows), dim3(256), 0, (hipStream_t)stream, s->tab, s->n, x0, mask,
                           (const long long*)clip, (const long long*)t, feats, frames, (unsigned long long)seed, out);
    }
    HIPCHECK(hipGetLastError());
    return 0;
}

// _vb_terms_bpd given the model output (gaussian_diffusion.py:1281-1314) plus the loop's two MSEs (:1586-1588), one workgroup per row.
extern "C" int mst_vb_terms(const mst_schedule* s, const float* true_logvar, const float* x0, const float* x_t, const float* model_out,
                            const float* noise, const float* mask, const float* motion, const int64_t* clip, const int64_t* t,
                            int32_t rows, int64_t per_clip, int32_t feats, int32_t frames, uint64_t seed, int32_t mean_type,
                            int32_t clip_denoised, float* out, float* xstart, void* stream) {
    if (!s || !true_logvar || !x0 || !x_t || !model_out || !clip || !t || !out) return fail("mst_vb_terms: null argument");
    if (rows < 1 || per_clip < 1) return fail("mst_vb_terms: rows %d and per_clip %lld must be >= 1", rows, (long long)per_clip);
    if (mean_type < 0 || mean_type > 2) return fail("mst_vb_terms: bad mean type %d (0 = x_start, 1 = epsilon, 2 = previous x)", mean_type);
    if ((mask != nullptr) != (motion != nullptr)) return fail("mst_vb_terms: the inpainting pair is mask AND motion, or neither");
    if (!noise) CHECK(vb_draw_check("mst_vb_terms", per_clip, feats, frames));
    ON_DEVICE(s->device);
#define VB_LAUNCH(M_, D_)                                                                                                                \
    hipLaunchKernelGGL((k_vb_terms<M_, D_>), dim3(rows), dim3(VB_THREADS), 0, (hipStream_t)stream, s->tab, true_logvar, s->n, x0, x_t,    \
                       model_out, noise, mask, motion, (const long long*)clip, (const long long*)t, (long long)per_clip, feats, frames,   \
                       (unsigned long long)seed, clip_denoised, out, xstart)
    switch (mean_type) {
        case 0: if (noise) VB_LAUNCH(0, false); else VB_LAUNCH(0, true); break;
        case 1: if (noise) VB_LAUNCH(1, false); else VB_LAUNCH(1, true); break;
        default: if (noise) VB_LAUNCH(2, false); else VB_LAUNCH(2, true); break;
    }
#undef VB_LAUNCH
    HIPCHECK(hipGetLastError());
    return 0;
}

// _prior_bpd (gaussian_diffusion.py:1529-1545): the same reduction over x_start^2, one workgroup per clip.
extern "C" int mst_vb_prior(const mst_schedule* s, const float* x0, int32_t batch, int64_t per_clip, float sqrt_ac_last, float log_1m_ac_last, float* out,
                            void* stream) {
    if (!s || !x0 || !out) return fail("mst_vb_prior: null argument");
    if (batch < 1 || per_clip < 1) return fail("mst_vb_prior: batch %d and per_clip %lld must be >= 1", batch, (long long)per_clip);
    ON_DEVICE(s->device);
    hipLaunchKernelGGL(k_vb_prior, dim3(batch), dim3(VB_THREADS), 0, (hipStream_t)stream, x0, (long long)per_clip, sqrt_ac_last,
                       log_1m_ac_last, out);
    HIPCHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ training ABI
// The trainable encoder stack (seqTransEncoder, mdm_forstyledataset.py:539-546) in training mode.
// Tape: per layer the activations the backward pass needs, in caller-owned memory.
struct TapeL { f16 *qkv, *att, *z1h, *z1l, *x1h, *x1l, *pre, *hid, *z2h, *z2l; float* lse; };
struct Tape { f16* sh[17]; f16* sl[17]; TapeL L[16]; };
static size_t tape_rows(int M) { return ((size_t)(M + 255) / 256) * 256 + 256; }     // whole tiles + one spare (over-read)
static size_t tape_layout(char* base, int nl, size_t Mp, Tape* t) {
    size_t off = 0;
    auto take = [&](size_t width) { f16* p = reinterpret_cast<f16*>(base + off); off += Mp * width * 2; return p; };
    for (int l = 0; l <= nl; l++) { t->sh[l] = take(MST_D); t->sl[l] = take(MST_D); }
    for (int l = 0; l < nl; l++) {
        TapeL& a = t->L[l];
        a.qkv = take(3 * MST_D); a.att = take(MST_D);
        a.z1h = take(MST_D); a.z1l = take(MST_D); a.x1h = take(MST_D); a.x1l = take(MST_D);
        a.pre = take(MST_FF); a.hid = take(MST_FF);
        a.z2h = take(MST_D); a.z2l = take(MST_D);
        a.lse = reinterpret_cast<float*>(take(2 * MST_H));            // softmax row statistics [rows][4][S] (4 floats per token)
    }
    return off;
}

// elem_off: the site's element counter starts there (drop_mul hashes idx * phi + key, so an offset is a shifted key): a forward pass that
// writes clips [clip0, ..) of a LARGER tape draws exactly the masks a backward pass over the whole tape regenerates
// the rows of clips [clip0, ..) inside a tape laid out for more clips (every slot is [rows][width], clip-major)
static void tape_shift(Tape& t, int nl, size_t row0) {
    for (int l = 0; l <= nl; l++) { t.sh[l] += row0 * MST_D; t.sl[l] += row0 * MST_D; }
    for (int l = 0; l < nl; l++) {
        TapeL& a = t.L[l];
        a.qkv += row0 * 3 * MST_D; a.att += row0 * MST_D;
        a.z1h += row0 * MST_D; a.z1l += row0 * MST_D; a.x1h += row0 * MST_D; a.x1l += row0 * MST_D;
        a.pre += row0 * MST_FF; a.hid += row0 * MST_FF;
        a.z2h += row0 * MST_D; a.z2l += row0 * MST_D;
        a.lse += row0 * MST_H;
    }
}

static Drop make_drop(uint64_t seed, int layer, int site, float p, uint32_t elem_off = 0) {
    Drop d{0u, 0u, 1.0f};
    if (p <= 0.f) return d;
    d.key = mix32((uint32_t)seed ^ mix32((uint32_t)(seed >> 32) + 0x9E3779B9u * (uint32_t)(layer * 4 + site + 1))) + elem_off * 0x9E3779B9u;
    const double t = (double)p * 4294967296.0;
    d.thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
    d.inv = 1.0f / (1.0f - p);
    return d;
}

static int train_check(mst_engine* e, int rows, int S, float p) {
    if (!e) return fail("null engine");
    CHECK(mst_weights_complete(e));
    if (S < 2 || S > e->S_max) return fail("train: S=%d outside 2..%d", S, e->S_max);
    if (rows < 1 || (size_t)rows * S > (size_t)e->cfg.max_rows * e->S_max) return fail("train: %d rows x %d tokens exceed the engine capacity", rows, S);
    if (!(p >= 0.f && p < 1.f)) return fail("train: dropout probability %g outside [0, 1)", (double)p);
    if ((size_t)rows * S * MST_FF >= 0xFFFFFFFFull || (size_t)rows * MST_H * S * S >= 0xFFFFFFFFull)
        return fail("train: batch too large for the 32-bit dropout counters");
    return 0;
}
// The training stack reads slot 0's weights only: with several styles set it would compute every clip with slot 0.
static int train_refuse_styles(const mst_engine* e, const char* who) {
    if (styles_on(e)) return fail("%s: styles are set (mst_set_styles / StyleBank); training runs one stack: mst_set_styles(e, nullptr) first", who);
    return 0;
}

extern "C" int64_t mst_train_tape_bytes(const mst_engine* e, int32_t rows, int32_t S) {
    if (!e || rows < 1 || S < 1) return -1;
    Tape t;
    return (int64_t)tape_layout(nullptr, e->cfg.num_layers, tape_rows(rows * S), &t);
}

template <int NKT>
static int launch_attn_train_n(const f16* qkv, f16* out, int S, int rows, Drop d, const unsigned char* keep, int qsplit, float* lse, hipStream_t st) {
    auto kern = k_attention_train<NKT>;
    const int smem = NKT * 32 * 256 * 2 + NKT * 32 * 4;
    CHECK(ensure_dyn_lds((const void*)kern, smem));
    hipLaunchKernelGGL(kern, dim3(rows * MST_H, qsplit ? NKT : 1), dim3(512), smem, st, qkv, out, S, d, keep, qsplit, lse);
    HIPCHECK(hipGetLastError());
    return 0;
}
template <int NKT>
static int launch_attn_bwd_n(const f16* qkv, const f16* att, const f16* datt, f16* dqkv, int S, int rows, Drop d,
                             const unsigned char* keep, const float* lse, int split, hipStream_t st) {
    auto kern = k_attention_bwd<NKT>;
    const int smem = NKT * 32 * 256 * 2 + NKT * 32 * 12;
    CHECK(ensure_dyn_lds((const void*)kern, smem));
    hipLaunchKernelGGL(kern, dim3(rows * MST_H, split ? 2 * NKT : 1), dim3(512), smem, st, qkv, att, datt, dqkv, S, d, keep, lse, split);
    HIPCHECK(hipGetLastError());
    return 0;
}
static int launch_attn_train(const f16* qkv, f16* out, int S, int rows, Drop d, const unsigned char* keep, int qsplit, float* lse, hipStream_t st) {
    NKT_SWITCH(launch_attn_train_n, S, qkv, out, S, rows, d, keep, qsplit, lse, st)
}
static int launch_attn_bwd(const f16* qkv, const f16* att, const f16* datt, f16* dqkv, int S, int rows, Drop d,
                           const unsigned char* keep, const float* lse, int split, hipStream_t st) {
    NKT_SWITCH(launch_attn_bwd_n, S, qkv, att, datt, dqkv, S, rows, d, keep, lse, split, st)
}

// h_in / h_out: [rows][S][512] float32 (clip-major token rows).  mdm_forstyledataset.py:622 `self.seqTransEncoder(xseq)`
// with nn.TransformerEncoderLayer semantics (post-norm, erf GELU, dropout p at the four sites of the layer).
// the eight layers from tape slot 0 to slot num_layers
static int train_stack_forward(mst_engine* e, const Tape& t, int rows, int S, float p_drop, uint64_t seed, const uint8_t* key_keep,
                               hipStream_t st, int clip0 = 0) {
    const int M = rows * S, nl = e->cfg.num_layers;
    // dropout counters of the four sites start at clip `clip0` of the tape (attention probabilities, 512-wide rows, hidden rows)
    const uint32_t o0 = (uint32_t)clip0 * MST_H * S * S, o1 = (uint32_t)clip0 * S * MST_D, o2 = (uint32_t)clip0 * S * MST_FF;
    e->prof_now = 0;
    const bool small = e->small_m > 0 && M <= e->small_m;
    const bool fast = small && e->small_fast;            // the four GEMMs as resident-tile kernels (mst_small.h), as in the sampling path
    if (fast) CHECK(ensure_small_packed_all(e, st));
    // round 6: at a clip or two (the objective's chained single-clip calls) the two LayerNorms of a layer ride in the GEMM behind them
    // (k_rows_gemm LNF = 1 with LnRows' training fields: dropout, z -> tape), as on the sampling path: 16 launches fewer per call.
    // LayerNorm1 in FFN1; LayerNorm2 in the NEXT layer's QKV GEMM, the last one as the rows kernel.  MST_TRAIN_SMALL_LN=0: every LayerNorm a launch.
    const bool lnf = fast && e->train_small_ln && M <= e->small_ln_m;
    for (int l = 0; small && l < nl; l++) {              // few token rows: 64 x 128 tiles, row-wise LayerNorm, query-split attention
        const LayerW& w = e->L[l];
        const TapeL& a = t.L[l];
        if (lnf && l > 0) {
            const LayerW& p = e->L[l - 1];
            const TapeL& pa = t.L[l - 1];
            LnRows ln{e->zacc, p.b2, p.g2, p.be2, pa.x1h, pa.x1l, t.sh[l], t.sl[l]};
            ln.z_hi = pa.z2h; ln.z_lo = pa.z2l; ln.d = make_drop(seed, l - 1, 3, p_drop, o1);
            CHECK((launch_rows_gemm<16, 0>(M, 3 * MST_D, nullptr, w.wsm_in, w.b_in, a.qkv, 3 * MST_D, st, &ln)));
        } else if (fast) CHECK((launch_rows_gemm<16, 0>(M, 3 * MST_D, t.sh[l], w.wsm_in, w.b_in, a.qkv, 3 * MST_D, st)));
        else {
            DEpiBiasF16<false> epi{w.b_in, a.qkv, 3 * MST_D, M};
            CHECK(launch_small(M, 3 * MST_D, RowsDirect{t.sh[l], MST_D}, w.w_in, MST_D, MST_D, epi, st));
        }
        CHECK(launch_attn_train(a.qkv, a.att, S, rows, make_drop(seed, l, 0, p_drop, o0), key_keep, 1, a.lse, st));
        {
            if (fast) CHECK((launch_rows_gemm<16, 2>(M, MST_D, a.att, w.wsm_out, nullptr, e->zacc, MST_D, st)));
            else {
                DEpiPlainF32 epi{e->zacc, MST_D, M};
                CHECK(launch_small(M, MST_D, RowsDirect{a.att, MST_D}, w.w_out, MST_D, MST_D, epi, st));
            }
            if (!lnf) {
                hipLaunchKernelGGL(k_ln_rows_train, dim3((M + 3) / 4), dim3(256), 0, st, e->zacc, w.b_out, w.g1, w.be1, t.sh[l], t.sl[l],
                                   a.z1h, a.z1l, a.x1h, a.x1l, M, make_drop(seed, l, 1, p_drop, o1));
                HIPCHECK(hipGetLastError());
            }
        }
        if (lnf) {
            const FfnTrain ft{a.pre, make_drop(seed, l, 2, p_drop, o2)};
            LnRows ln{e->zacc, w.b_out, w.g1, w.be1, t.sh[l], t.sl[l], a.x1h, a.x1l};
            ln.z_hi = a.z1h; ln.z_lo = a.z1l; ln.d = make_drop(seed, l, 1, p_drop, o1);
            CHECK((launch_rows_gemm<16, 3>(M, MST_FF, nullptr, w.wsm_1, w.b1, a.hid, MST_FF, st, &ln, &ft)));
        } else if (fast) {
            const FfnTrain ft{a.pre, make_drop(seed, l, 2, p_drop, o2)};
            CHECK((launch_rows_gemm<16, 3>(M, MST_FF, a.x1h, w.wsm_1, w.b1, a.hid, MST_FF, st, nullptr, &ft)));
        } else {
            DEpiRowOp<OpFfn1Train> epi{w.b1, M, OpFfn1Train{a.pre, a.hid, MST_FF, make_drop(seed, l, 2, p_drop, o2)}};
            CHECK(launch_small(M, MST_FF, RowsDirect{a.x1h, MST_D}, w.w1, MST_D, MST_D, epi, st));
        }
        {
            if (fast) CHECK((launch_rows_gemm<32, 2>(M, MST_D, a.hid, w.wsm_2, nullptr, e->zacc, MST_D, st)));
            else {
                DEpiPlainF32 epi{e->zacc, MST_D, M};
                CHECK(launch_small(M, MST_D, RowsDirect{a.hid, MST_FF}, w.w2, MST_FF, MST_FF, epi, st));
            }
            if (!lnf || l == nl - 1) {
                hipLaunchKernelGGL(k_ln_rows_train, dim3((M + 3) / 4), dim3(256), 0, st, e->zacc, w.b2, w.g2, w.be2, a.x1h, a.x1l,
                                   a.z2h, a.z2l, t.sh[l + 1], t.sl[l + 1], M, make_drop(seed, l, 3, p_drop, o1));
                HIPCHECK(hipGetLastError());
            }
        }
    }
    // round 6: everything of a layer behind the attention as ONE launch (k_layer_tail_train, mst_tail.h) that writes the tape slots
    // itself -- the sampling path's fused tail with dropout at the three sites, instead of three ring GEMMs moving 52-103 MB each
    const bool fused_tail = !small && e->train_fuse_tail && e->fuse_tail;
    if (fused_tail) {
        for (int l = 0; l < nl; l++) {
            LayerW& w = e->L[l];
            if (!w.tail_dirty) continue;
            hipLaunchKernelGGL(k_pack_tail, dim3(640), dim3(256), 0, st, w.w_out, w.w1, w.w2, w.wtail);
            HIPCHECK(hipGetLastError());
            w.tail_dirty = false;
        }
        CHECK(ensure_dyn_lds((const void*)k_layer_tail_train<4>, TailCfg::SMEM));
    }
    for (int l = 0; !small && l < nl; l++) {
        const LayerW& w = e->L[l];
        const TapeL& a = t.L[l];
        {
            DEpiBiasF16<false> epi{w.b_in, a.qkv, 3 * MST_D, M};
            CHECK((launch_wide(M, 3 * MST_D / 256, RowsDirect{t.sh[l], MST_D}, w.w_in, MST_D, MST_D, epi, st)));
        }
        CHECK(launch_attn_train(a.qkv, a.att, S, rows, make_drop(seed, l, 0, p_drop, o0), key_keep, 0, a.lse, st));
        if (fused_tail) {
            auto td = [&](int site, uint32_t off) { const Drop d = make_drop(seed, l, site, p_drop, off); return TailDrop{d.key, d.thr, d.inv}; };
            const TailTrain tt{t.sh[l], t.sl[l], a.z1h, a.z1l, a.x1h, a.x1l, a.pre, a.hid, a.z2h, a.z2l, td(1, o1), td(2, o2), td(3, o1)};
            hipLaunchKernelGGL(k_layer_tail_train<4>, dim3((M + 63) / 64), dim3(512), TailCfg::SMEM, st, a.att, w.wtail, w.b_out, w.g1, w.be1,
                               w.b1, w.b2, w.g2, w.be2, t.sh[l + 1], t.sl[l + 1], e->gelu_tab, M, tt);
            HIPCHECK(hipGetLastError());
            continue;
        }
        {
            DEpiResidLNTrain epi{w.b_out, w.g1, w.be1, t.sh[l], t.sl[l], a.z1h, a.z1l, a.x1h, a.x1l, M, make_drop(seed, l, 1, p_drop, o1)};
            CHECK((launch_gemm_dma<64, 512, 2, 2, LN_NS, 1, LN_BK>(dim3((M + 63) / 64, 1), RowsDirect{a.att, MST_D}, w.w_out, MST_D, MST_D, epi, st)));
        }
        {
            DEpiRowOp<OpFfn1Train> epi{w.b1, M, OpFfn1Train{a.pre, a.hid, MST_FF, make_drop(seed, l, 2, p_drop, o2)}};
            CHECK((launch_wide(M, MST_FF / 256, RowsDirect{a.x1h, MST_D}, w.w1, MST_D, MST_D, epi, st)));
        }
        {
            DEpiResidLNTrain epi{w.b2, w.g2, w.be2, a.x1h, a.x1l, a.z2h, a.z2l, t.sh[l + 1], t.sl[l + 1], M, make_drop(seed, l, 3, p_drop, o1)};
            CHECK((launch_gemm_dma<64, 512, 2, 2, LN_NS, 1, LN_BK>(dim3((M + 63) / 64, 1), RowsDirect{a.hid, MST_FF}, w.w2, MST_FF, MST_FF, epi, st)));
        }
    }
    return 0;
}

extern "C" int mst_train_forward(mst_engine* e, const float* h_in, int32_t rows, int32_t S, float p_drop, uint64_t seed,
                                 const uint8_t* key_keep, void* tape, float* h_out, void* stream) {
    CHECK(train_check(e, rows, S, p_drop));
    CHECK(train_refuse_styles(e, "mst_train_forward"));
    if (!h_in || !tape || !h_out) return fail("mst_train_forward: null argument");
    hipStream_t st = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    const int M = rows * S, nl = e->cfg.num_layers;
    Tape t;
    tape_layout((char*)tape, nl, tape_rows(M), &t);
    const size_t n = (size_t)M * MST_D;
    hipLaunchKernelGGL(k_split_stream, dim3(1024), dim3(256), 0, st, h_in, n, t.sh[0], t.sl[0]);
    HIPCHECK(hipGetLastError());
    CHECK(train_stack_forward(e, t, rows, S, p_drop, seed, key_keep, st));
    hipLaunchKernelGGL(k_join_stream, dim3(1024), dim3(256), 0, st, t.sh[nl], t.sl[nl], h_out, n);
    HIPCHECK(hipGetLastError());
    return 0;
}

static int train_ws(mst_engine* e) {
    TrainWS& t = e->tw;
    if (t.ready) return 0;
    const size_t Mp = (size_t)e->M_pad;
    t.split_cap = 64;
    CHECK(dmalloc(&t.g0, Mp * MST_D));
    CHECK(dmalloc(&t.g1, Mp * MST_D));
    for (int i = 0; i < 2; i++) {
        CHECK(dmalloc(&t.dbr2[i], Mp * MST_D));
        CHECK(dmalloc(&t.dbr1[i], Mp * MST_D));
        CHECK(dmalloc(&t.dpre[i], Mp * MST_FF));
        CHECK(dmalloc(&t.hidr[i], Mp * MST_FF));
        CHECK(dmalloc(&t.dqkv[i], Mp * 3 * MST_D));
        HIPCHECK(hipEventCreateWithFlags(&t.ev_side[i], hipEventDisableTiming));
    }
    HIPCHECK(hipEventCreateWithFlags(&t.ev_ready, hipEventDisableTiming));
    for (int i = 0; i < 16; i++) HIPCHECK(hipEventCreateWithFlags(&t.ev_layer[i], hipEventDisableTiming));
    CHECK(dmalloc(&t.datt, Mp * MST_D));
    t.part_cap = t.split_cap * (size_t)3 * MST_D * MST_D;
    CHECK(dmalloc(&t.part, t.part_cap));
    CHECK(dmalloc(&t.ln_part, (size_t)512 * 3 * MST_D));
    CHECK(dmalloc(&t.ln_part2, (size_t)512 * 3 * MST_D));
    CHECK(dmalloc(&t.cs_part, (Mp / 128 + 2) * (size_t)3 * MST_D));
    CHECK(dmalloc(&t.zeros, 3 * MST_D + MST_D));          // zero bias [1536] + a 512-float dump for unwanted reductions
    CHECK(dmalloc(&t.gscale, 2));
    CHECK(dmalloc(&t.amax, 1));
    t.ready = true;
    return 0;
}

static int wgrad_flush(mst_engine* e, hipStream_t st) {
    TrainWS& t = e->tw;
    if (t.n_red) {
        hipLaunchKernelGGL(k_splitk_reduce_multi, dim3(768, t.n_red), dim3(256), 0, st, t.red_jobs, t.gscale);
        HIPCHECK(hipGetLastError());
    }
    t.n_red = 0;
    t.part_used = 0;
    return 0;
}

// dW[n_out][k_in] += unscale * dY^T X   (dY: [M][n_out] f16, X: [M][k_in] f16), db += unscale * colsum(dY) if db
static int wgrad(mst_engine* e, const f16* dY, int n_out, const f16* X, int k_in, int M, float* dW, float* db, hipStream_t st) {
    TrainWS& t = e->tw;
    // tiles x splits ~ 128 workgroups (MST_WGRAD_WGS): the partials' round trip grows with the splits -- stack backward at 64 clips 3.11 / 2.96 / 2.85 /
    // 2.95 / 3.11 / 3.37 ms at 64 / 96 / 128 / 256 / 384 / 512, and the dgrad chain on the other stream uses the CUs left; every split contracts a
    // whole number of 32-token slabs
    const int tiles = (n_out / 128) * (k_in / 256);
    static const int wg_target = [] { const char* v = getenv("MST_WGRAD_WGS"); return v ? atoi(v) : 128; }();
    // (round 6, measured and removed: twice the workgroups for layer 0's weight gradients -- they run when the dgrad chain beside them has
    // ended -- 10.11 / 10.15 / 10.20 ms per iteration without, 10.15 / 10.18 / 10.22 ms with: the wgrad stream's tail is not short of CUs)
    int nsplit = (wg_target + tiles - 1) / tiles;
    const int slabs = (M + 31) / 32;
    // round 6: splits a multiple of 8 and every split's tiles on ONE XCD (k_wgrad_tr's xcd_tiles): the slabs of dY and X a split walks are
    // requested by 4 + 4 (W1 / W2) tiles, and those used to sit on all eight L2s.  Same-box A/Bs of the fine-tune line, three alternating rounds
    // on two boxes: 9.76 / 9.86 / 10.04 -> 9.67 / 9.66 / 9.75 ms and 9.95 / 9.94 / 9.89 -> 9.82 / 9.89 / 9.84 ms (the launch itself 49.7 -> 47.8 us:
    // most of the gain is the dgrad stream's, which shares the memory system with it).  A deeper slab ring (5 / 6 slabs: 120 / 144 KB of LDS)
    // was measured with it and is slower -- the 72 KB ring leaves the CU's LDS to a dgrad workgroup.  MST_WGRAD_XCD=0: the 3-D grid of round 5.
    static const int xcd_on = [] { const char* v = getenv("MST_WGRAD_XCD"); return v ? atoi(v) : 1; }();
    bool xcd = xcd_on && M > SMALL_M && slabs >= 64;
    if (xcd) nsplit = ((nsplit + 7) / 8) * 8;
    if (nsplit > slabs) nsplit = slabs;
    if ((size_t)nsplit > t.split_cap) nsplit = (int)t.split_cap;
    if (M <= SMALL_M) nsplit = 1;        // few tokens: one workgroup per tile adds its product straight into dW (no partials, no reduce launch)
    const int kchunk = ((slabs + nsplit - 1) / nsplit) * 32;
    nsplit = (M + kchunk - 1) / kchunk;
    if (nsplit % 8) xcd = false;
    auto kern = k_wgrad_tr;
    CHECK(ensure_dyn_lds((const void*)kern, WgTile::SMEM));
    static_assert(DEpiF32::smem_bytes<128, 256>() <= WgTile::SMEM, "epilogue tile must fit the ring");
    const size_t nelem = (size_t)n_out * k_in;
    // profiling on (mst_profile_enable): every k_wgrad_tr launch of a training pass is bracketed by HIP events on ITS stream (bench.py --mode
    // finetune reads the family "wgrad_tr": the training path's dominant kernel, timed in the run that reports it)
    const int prof_keep = e->prof_now;
    e->prof_now = e->prof_on;
    if (nsplit == 1) {
        DEpiF32 epi{dW, dW, k_in, n_out, t.gscale};
        {
            ProfScope ps(e, FAM_WGRAD, st);
            hipLaunchKernelGGL(kern, dim3(n_out / 128, k_in / 256, 1), dim3(512), WgTile::SMEM, st, dY, n_out, X, k_in, M, kchunk, nelem, epi, 0);
        }
        e->prof_now = prof_keep;
        HIPCHECK(hipGetLastError());
    } else {
        const bool defer = t.red_defer && t.n_red < 4 && t.part_used + (size_t)nsplit * nelem <= t.part_cap;
        if (!defer) CHECK(wgrad_flush(e, st));               // (pending regions start at offset 0 as well)
        float* part = t.part + (defer ? t.part_used : 0);
        DEpiF32 epi{nullptr, part, k_in, n_out};
        {
            ProfScope ps(e, FAM_WGRAD, st);
            if (xcd) hipLaunchKernelGGL(kern, dim3(tiles * nsplit), dim3(512), WgTile::SMEM, st, dY, n_out, X, k_in, M, kchunk, nelem, epi, tiles);
            else hipLaunchKernelGGL(kern, dim3(n_out / 128, k_in / 256, nsplit), dim3(512), WgTile::SMEM, st, dY, n_out, X, k_in, M, kchunk, nelem, epi, 0);
        }
        e->prof_now = prof_keep;
        HIPCHECK(hipGetLastError());
        if (defer) {
            t.red_jobs.j[t.n_red++] = RedJob{part, dW, nelem, nsplit, 0};
            t.part_used += (size_t)nsplit * nelem;
        } else {
            hipLaunchKernelGGL(k_splitk_reduce, dim3((unsigned)((nelem / 4 + 255) / 256)), dim3(256), 0, st, t.part, nsplit, nelem, t.gscale, dW);
            HIPCHECK(hipGetLastError());
        }
    }
    if (db) {
        const int rpb = 128, nrb = (M + rpb - 1) / rpb;      // bias gradient: row-block partials, then an ordered sum (no float atomics)
        hipLaunchKernelGGL(k_colsum_f16, dim3(n_out / 256, nrb), dim3(256), 0, st, dY, n_out, M, rpb, t.gscale, db, t.cs_part);
        HIPCHECK(hipGetLastError());
        if (nrb > 1) {
            hipLaunchKernelGGL(k_sum_partials, dim3((n_out + kFinOut - 1) / kFinOut), dim3(256), 0, st, t.cs_part, nrb, n_out, t.gscale, db);
            HIPCHECK(hipGetLastError());
        }
    }
    return 0;
}

// grads: HOST array of num_layers * 12 device pointers in nn.TransformerEncoderLayer parameter order
// (in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, linear1.weight, linear1.bias, linear2.weight,
//  linear2.bias, norm1.weight, norm1.bias, norm2.weight, norm2.bias); every buffer is ACCUMULATED into.
// device-side gradient scaling: gscale <- the power of two that brings max |g| into [16, 32)
static int grad_scale_from(mst_engine* e, const float* g, size_t n, hipStream_t st) {
    TrainWS& w_ = e->tw;
    HIPCHECK(hipMemsetAsync(w_.amax, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_amax, dim3(512), dim3(256), 0, st, g, n, w_.amax);
    hipLaunchKernelGGL(k_grad_scale, dim3(1), dim3(1), 0, st, w_.amax, w_.gscale);
    HIPCHECK(hipGetLastError());
    return 0;
}

// the eight layers backwards: on entry tw.g1 holds the SCALED gradient wrt the stack output, on exit the scaled gradient
// wrt tape slot 0
static int train_stack_backward(mst_engine* e, const Tape& t, int rows, int S, float p_drop, uint64_t seed, const uint8_t* key_keep,
                                float* const* grads, hipStream_t st) {
    TrainWS& w_ = e->tw;
    const int M = rows * S, nl = e->cfg.num_layers;
    float* gA = w_.g0;      // dz buffers
    float* gB = w_.g1;      // gradient wrt the current layer output
    // one block per CU at most; their partial sums are added in block order (k_ln_bwd_finish).  Sixteen waves per block above LN_BWD_WIDE_M rows
    const bool ln_wide = M > LN_BWD_WIDE_M;
    const int ln_wpb = ln_wide ? 16 : 4;
    const int ln_blocks = (M + ln_wpb - 1) / ln_wpb < 256 ? (M + ln_wpb - 1) / ln_wpb : 256;
    auto ln_bwd = ln_wide ? k_ln_bwd<16> : k_ln_bwd<4>;
    const bool small = e->small_m > 0 && M <= e->small_m;
    // at batch size LayerNorm1's backward rides in the epilogue of the dgrad GEMM in front of it (DEpiLnBwd; MST_FUSE_LN_BWD=0: two launches)
    const int ln_tiles = (M + 63) / 64;
    const bool fuse_ln = e->fuse_ln_bwd && !small && ln_tiles <= 512;   // (512: the partial-sum buffer's rows)
    e->prof_now = 0;
    // The dgrad chain (LayerNorm / GELU / attention backward and the four dgrad GEMMs) is serial; the four wgrads of a
    // layer only consume its by-products, so they run on a second stream beside it.  Their f16 operands are
    // double-buffered by layer parity: the chain of layer l waits for the wgrads of layer l + 2, not l + 1.
    hipStream_t sw = e->wgrad_stream_on ? e->aux_stream[0] : st;
    const bool two = sw != st;
    bool side_used[2] = {false, false};
#define TO_SIDE()                                                   \
    if (two && grads) {                                                \
        HIPCHECK(hipEventRecord(w_.ev_ready, st));                  \
        HIPCHECK(hipStreamWaitEvent(sw, w_.ev_ready, 0));           \
    }
    // with parameter gradients the fused launch also writes dpre, hid and dbr1 as 8-byte pieces from the accumulator layout and is no faster
    // than the three launches yet (113 against 128-155 us beside the wgrad stream: LAB_NOTES R6.9); a frozen stack writes none of them
    const bool fused_bwd = (e->train_fuse_bwd_tail >= 2 || (e->train_fuse_bwd_tail == 1 && !grads)) && !small && ln_tiles <= 512;
    if (fused_bwd) {
        for (int l = 0; l < nl; l++) {
            LayerW& w = e->L[l];
            if (!w.wtail_bwd) CHECK(dmalloc(&w.wtail_bwd, TailCfg::LAYER_BYTES / 2));
            if (!w.tailb_dirty) continue;
            hipLaunchKernelGGL(k_pack_tail_bwd, dim3(640), dim3(256), 0, st, w.w_outT, w.w2T, w.w1T, w.wtail_bwd);
            HIPCHECK(hipGetLastError());
            w.tailb_dirty = false;
        }
        CHECK(ensure_dyn_lds((const void*)k_layer_tail_bwd<true>, TailBwdCfg::SMEM));
        CHECK(ensure_dyn_lds((const void*)k_layer_tail_bwd<false>, TailBwdCfg::SMEM));
        CHECK(ensure_dyn_lds((const void*)k_layer_tail_bwd<false, true>, TailBwdCfg::SMEM));
    }
    const bool fused_ln2 = fused_bwd && e->train_fuse_ln2_bwd && !grads;      // (frozen stacks: with gradients dbr2 and LayerNorm2's sums must reach HBM anyway)
    static const int red_batch = [] { const char* v = getenv("MST_WGRAD_REDUCE_BATCH"); return v ? atoi(v) : 1; }();
    w_.red_defer = red_batch != 0 && grads != nullptr;
    w_.n_red = 0;
    w_.part_used = 0;
    for (int l = nl - 1; l >= 0; l--) {
        const LayerW& w = e->L[l];
        const TapeL& a = t.L[l];
        const int par = l & 1;
        f16 *dbr2 = w_.dbr2[par], *dbr1 = w_.dbr1[par], *dpre = w_.dpre[par], *dqkv = w_.dqkv[par];
        // grads == NULL (frozen stack): no wgrads; the LayerNorm kernel's small reductions land in a scratch vector
        float* dump[12];
        for (int i = 0; i < 12; i++) dump[i] = w_.zeros + 3 * MST_D;
        float* const* G = grads ? grads + (size_t)l * 12 : dump;
        const bool wg = grads != nullptr;
        for (int i = 0; i < 12; i++) if (!G[i]) return fail("mst_train_backward: null gradient buffer (layer %d, tensor %d)", l, i);
        if (two && side_used[par]) HIPCHECK(hipStreamWaitEvent(st, w_.ev_side[par], 0));
        // LayerNorm2 backward: gB -> dz2 (gA, fp32) and the branch gradient dbr2 (f16); dgamma2, dbeta2, db2
        // (round 6, MST_LN_FINISH_MERGE: with parameter gradients and the unfused tail, LayerNorm2's partial sums wait in a buffer of their own and
        // ONE launch behind LayerNorm1's backward finishes both -- a launch less per layer on the dgrad chain, same sums in the same order)
        static const int merge_on = [] { const char* v = getenv("MST_LN_FINISH_MERGE"); return v ? atoi(v) : 1; }();
        const bool merge_fin = merge_on && wg && !fused_bwd;
        if (!fused_ln2) {
        hipLaunchKernelGGL(ln_bwd, dim3(ln_blocks), dim3(64 * ln_wpb), 0, st, gB, a.z2h, a.z2l, w.g2, M, make_drop(seed, l, 3, p_drop), w_.gscale,
                           gA, dbr2, merge_fin ? w_.ln_part2 : w_.ln_part);
        if (wg && !merge_fin) hipLaunchKernelGGL(k_ln_bwd_finish, dim3(3 * MST_D / kFinOut), dim3(256), 0, st, w_.ln_part, ln_blocks, w_.gscale, G[10], G[11], G[7]);
        HIPCHECK(hipGetLastError());
        }
        // d pre = (dbr2 W2) * mask * gelu'(pre); the same epilogue regenerates hid = dropout(GELU(pre)), dW2's operand, from the pre it reads
        // anyway (round 6: the fused training forward no longer writes hid to the tape -- 2 KB per token and layer less, and a frozen stack
        // never needs it)
        f16* hidr = wg ? w_.hidr[par] : nullptr;
        if (fused_bwd) {
            // round 6: FFN2 dgrad + GELU' + FFN1 dgrad + LayerNorm1 backward + out-proj dgrad in ONE launch (mst_tail_bwd.h): dz1 -> gA in place,
            // d att; with gradients wanted also dpre, hid, dbr1 and the tiles' [dgamma1 | dbeta1 | db_out] sums
            auto td = [&](int site) { const Drop d = make_drop(seed, l, site, p_drop); return TailDrop{d.key, d.thr, d.inv}; };
            const TailBwdOut o{wg ? dpre : nullptr, hidr, wg ? dbr1 : nullptr, wg ? w_.ln_part : nullptr};
            const TailBwdLn2 n2{gB, a.z2h, a.z2l, w.g2, td(3)};
            if (fused_ln2) hipLaunchKernelGGL((k_layer_tail_bwd<false, true>), dim3(ln_tiles), dim3(512), TailBwdCfg::SMEM, st, dbr2, w.wtail_bwd, a.pre, a.z1h, a.z1l, w.g1, gA, w_.datt, o, td(1), td(2), M, e->gelu_tab, n2);
            else if (wg) hipLaunchKernelGGL(k_layer_tail_bwd<true>, dim3(ln_tiles), dim3(512), TailBwdCfg::SMEM, st, dbr2, w.wtail_bwd, a.pre, a.z1h, a.z1l, w.g1, gA, w_.datt, o, td(1), td(2), M, e->gelu_tab);
            else hipLaunchKernelGGL(k_layer_tail_bwd<false>, dim3(ln_tiles), dim3(512), TailBwdCfg::SMEM, st, dbr2, w.wtail_bwd, a.pre, a.z1h, a.z1l, w.g1, gA, w_.datt, o, td(1), td(2), M, e->gelu_tab);
            if (wg) hipLaunchKernelGGL(k_ln_bwd_finish, dim3(3 * MST_D / kFinOut), dim3(256), 0, st, w_.ln_part, ln_tiles, w_.gscale, G[8], G[9], G[3]);
            HIPCHECK(hipGetLastError());
            TO_SIDE()
            if (wg) CHECK(wgrad(e, dbr2, MST_D, hidr, MST_FF, M, G[6], nullptr, sw));                  // dW2 += dbr2^T hid
            if (wg) CHECK(wgrad(e, dpre, MST_FF, a.x1h, MST_D, M, G[4], G[5], sw));                    // dW1 += dpre^T x1, db1
            if (wg) CHECK(wgrad(e, dbr1, MST_D, a.att, MST_D, M, G[2], nullptr, sw));                  // dW_out += dbr1^T att
        } else {
        {
            DEpiRowOp<OpGeluBwd> epi{nullptr, M, OpGeluBwd{a.pre, dpre, MST_FF, make_drop(seed, l, 2, p_drop), hidr}};
            CHECK(small ? launch_small(M, MST_FF, RowsDirect{dbr2, MST_D}, w.w2T, MST_D, MST_D, epi, st)
                        : launch_wide(M, MST_FF / 256, RowsDirect{dbr2, MST_D}, w.w2T, MST_D, MST_D, epi, st));
        }
        TO_SIDE()
        if (wg) CHECK(wgrad(e, dbr2, MST_D, hidr, MST_FF, M, G[6], nullptr, sw));                  // dW2 += dbr2^T hid
        if (wg) CHECK(wgrad(e, dpre, MST_FF, a.x1h, MST_D, M, G[4], G[5], sw));                    // dW1 += dpre^T x1, db1
        if (fuse_ln) {
            // g(x1) = dpre W1 + dz2 and LayerNorm1's backward behind it in ONE launch (DEpiLnBwd): dz1 -> gA in place, dbr1, the tiles' sums
            DEpiLnBwd epi{gA, a.z1h, a.z1l, w.g1, M, make_drop(seed, l, 1, p_drop), gA, dbr1, w_.ln_part};
            CHECK((launch_gemm_dma<64, 512, 2, 2, LN_NS, 1, LN_BK>(dim3(ln_tiles, 1), RowsDirect{dpre, MST_FF}, w.w1T, MST_FF, MST_FF, epi, st)));
            if (merge_fin) hipLaunchKernelGGL(k_ln_bwd_finish2, dim3(3 * MST_D / kFinOut, 2), dim3(256), 0, st, LnFinJob{w_.ln_part2, ln_blocks, G[10], G[11], G[7]},
                                              LnFinJob{w_.ln_part, ln_tiles, G[8], G[9], G[3]}, w_.gscale);
            else if (wg) hipLaunchKernelGGL(k_ln_bwd_finish, dim3(3 * MST_D / kFinOut), dim3(256), 0, st, w_.ln_part, ln_tiles, w_.gscale, G[8], G[9], G[3]);
            HIPCHECK(hipGetLastError());
        } else {
        // g(x1) = dpre W1 + dz2  -> gB
        {
            DEpiF32 epi{gA, gB, MST_D, M};
            CHECK(small ? launch_small(M, MST_D, RowsDirect{dpre, MST_FF}, w.w1T, MST_FF, MST_FF, epi, st)
                        : launch_wide(M, MST_D / 256, RowsDirect{dpre, MST_FF}, w.w1T, MST_FF, MST_FF, epi, st));
        }
        // LayerNorm1 backward: gB -> dz1 (gA), dbr1 = d(out-proj output); dgamma1, dbeta1, db_out
        hipLaunchKernelGGL(ln_bwd, dim3(ln_blocks), dim3(64 * ln_wpb), 0, st, gB, a.z1h, a.z1l, w.g1, M, make_drop(seed, l, 1, p_drop), w_.gscale,
                           gA, dbr1, w_.ln_part);
        if (merge_fin) hipLaunchKernelGGL(k_ln_bwd_finish2, dim3(3 * MST_D / kFinOut, 2), dim3(256), 0, st, LnFinJob{w_.ln_part2, ln_blocks, G[10], G[11], G[7]},
                                          LnFinJob{w_.ln_part, ln_blocks, G[8], G[9], G[3]}, w_.gscale);
        else if (wg) hipLaunchKernelGGL(k_ln_bwd_finish, dim3(3 * MST_D / kFinOut), dim3(256), 0, st, w_.ln_part, ln_blocks, w_.gscale, G[8], G[9], G[3]);
        HIPCHECK(hipGetLastError());
        }
        TO_SIDE()
        if (wg) CHECK(wgrad(e, dbr1, MST_D, a.att, MST_D, M, G[2], nullptr, sw));                  // dW_out += dbr1^T att
        // d att = dbr1 W_out
        {
            DEpiBiasF16<false> epi{w_.zeros, w_.datt, MST_D, M};
            CHECK(small ? launch_small(M, MST_D, RowsDirect{dbr1, MST_D}, w.w_outT, MST_D, MST_D, epi, st)
                        : launch_wide(M, MST_D / 256, RowsDirect{dbr1, MST_D}, w.w_outT, MST_D, MST_D, epi, st));
        }
        }   // !fused_bwd
        // attention backward -> d qkv
        CHECK(launch_attn_bwd(a.qkv, a.att, w_.datt, dqkv, S, rows, make_drop(seed, l, 0, p_drop), key_keep, a.lse, small ? 1 : 0, st));
        TO_SIDE()
        if (wg) CHECK(wgrad(e, dqkv, 3 * MST_D, t.sh[l], MST_D, M, G[0], G[1], sw));               // dW_in += dqkv^T x_in, db_in
        if (wg) CHECK(wgrad_flush(e, sw));                                                         // the layer's split-K reduces, one launch
        if (two && wg) {
            HIPCHECK(hipEventRecord(w_.ev_side[par], sw));
            side_used[par] = true;
        }
        if (wg) {
            // everything that writes layer l's 12 gradient tensors is enqueued: the wgrads on `sw` (which waited for the
            // dgrad chain up to the attention backward, i.e. for both LayerNorm-backward kernels of this layer too).
            // A data-parallel reducer makes its communication stream wait for THIS event (mst_train_wait_layer_grads) and
            // starts the layer's all-reduce while the layers below are still being differentiated.
            HIPCHECK(hipEventRecord(w_.ev_layer[l], sw));
            w_.layer_done[l] = true;
        }
        // g(x_in) = dqkv W_in + dz1 -> gB
        {
            DEpiF32 epi{gA, gB, MST_D, M};
            CHECK(small ? launch_small(M, MST_D, RowsDirect{dqkv, 3 * MST_D}, w.w_inT, 3 * MST_D, 3 * MST_D, epi, st)
                        : launch_wide(M, MST_D / 256, RowsDirect{dqkv, 3 * MST_D}, w.w_inT, 3 * MST_D, 3 * MST_D, epi, st));
        }
    }
    w_.red_defer = false;
#undef TO_SIDE
    if (two)
        for (int i = 0; i < 2; i++)
            if (side_used[i]) HIPCHECK(hipStreamWaitEvent(st, w_.ev_side[i], 0));
    return 0;
}

extern "C" int mst_train_backward(mst_engine* e, const void* tape, const float* d_out, int32_t rows, int32_t S, float p_drop,
                                  uint64_t seed, const uint8_t* key_keep, float* d_in, float* const* grads, void* stream) {
    CHECK(train_check(e, rows, S, p_drop));
    if (!tape || !d_out) return fail("mst_train_backward: null argument");
    if (!grads && !d_in) return 0;                       // nothing asked for
    hipStream_t st = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    CHECK(train_ws(e));
    TrainWS& w_ = e->tw;
    const int M = rows * S, nl = e->cfg.num_layers;
    Tape t;
    tape_layout((char*)const_cast<void*>(tape), nl, tape_rows(M), &t);
    const size_t n = (size_t)M * MST_D;
    CHECK(grad_scale_from(e, d_out, n, st));
    hipLaunchKernelGGL(k_scale_f32, dim3(1024), dim3(256), 0, st, d_out, n, w_.gscale, 0, w_.g1);
    HIPCHECK(hipGetLastError());
    CHECK(train_stack_backward(e, t, rows, S, p_drop, seed, key_keep, grads, st));
    if (d_in) {
        hipLaunchKernelGGL(k_scale_f32, dim3(1024), dim3(256), 0, st, w_.g1, n, w_.gscale, 1, d_in);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

extern "C" int mst_train_wait_layer_grads(mst_engine* e, int32_t layer, void* stream) {
    if (!e || layer < 0 || layer >= e->cfg.num_layers) return fail("mst_train_wait_layer_grads: bad arguments");
    if (!e->tw.ready || !e->tw.layer_done[layer]) return fail("mst_train_wait_layer_grads: no backward pass has produced gradients of layer %d yet", layer);
    ON_DEVICE(e->cfg.device);
    HIPCHECK(hipStreamWaitEvent((hipStream_t)stream, e->tw.ev_layer[layer], 0));
    return 0;
}

// ---- the whole denoiser inside the native graph: conditioning token, pose embedding, positional-encoding dropout, the
// trainable stack, output projection (StyleDiffusion.forward / MDM.forward, mdm_forstyledataset.py:602-625 / :315-364, in
// train mode).  Text conditioning as for mst_forward: mst_set_text(batch, cfg = 0) first.
static Drop pe_drop(uint64_t seed, float p, uint32_t elem_off = 0) { return make_drop(seed, 32, 0, p, elem_off); }       // site of its own, beyond any layer

extern "C" int mst_train_model_forward(mst_engine* e, const float* x, const int64_t* t_idx, int32_t batch, int32_t frames,
                                       float p_drop, float p_pe, uint64_t seed, void* tape, float* out, int32_t clip0, int32_t tape_clips,
                                       void* stream) {
    CHECK(check_ready(e, batch, frames, 0));
    const int S = frames + 1;
    if (tape_clips <= 0) { tape_clips = batch; clip0 = 0; }
    if (clip0 < 0 || clip0 + batch > tape_clips) return fail("mst_train_model_forward: clips %d..%d outside a tape of %d", clip0, clip0 + batch, tape_clips);
    CHECK(train_check(e, tape_clips, S, p_drop));
    CHECK(train_refuse_styles(e, "mst_train_model_forward"));
    if (!(p_pe >= 0.f && p_pe < 1.f)) return fail("mst_train_model_forward: positional-encoding dropout %g outside [0, 1)", (double)p_pe);
    if (!x || !t_idx || !tape || !out) return fail("mst_train_model_forward: null argument");
    hipStream_t st = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    const int M = batch * S, nl = e->cfg.num_layers;
    Tape t;
    tape_layout((char*)tape, nl, tape_rows(tape_clips * S), &t);
    tape_shift(t, nl, (size_t)clip0 * S);
    e->prof_now = 0;
    CHECK(ensure_packed(e, st, false));
    const bool table = e->temb_table_on != 0;
    if (table) CHECK(ensure_temb_table(e, st));
    else CHECK(timestep_rows(e, (const long long*)t_idx, batch, st));
    WS ws = ws_slice(e, 0, frames);
    ws.hx = t.sh[0];                                      // the token stream is assembled straight into tape slot 0
    ws.hl = t.sl[0];
    // round 6: PositionalEncoding's dropout rides in the embedding kernel's epilogue (MST_TRAIN_FUSE_PE_DROP=0: k_dropout_stream behind it)
    static const int fuse_pe = [] { const char* v = getenv("MST_TRAIN_FUSE_PE_DROP"); return v ? atoi(v) : 1; }();
    const Drop ped = pe_drop(seed, p_pe, (uint32_t)clip0 * S * MST_D);
    CHECK(assemble_stream(e, ws, x, batch, batch, frames, -1, batch, st, batch, LoopRef(), table ? (const long long*)t_idx : nullptr,
                          (fuse_pe && p_pe > 0.f) ? &ped : nullptr));
    if (p_pe > 0.f && !fuse_pe) {
        hipLaunchKernelGGL(k_dropout_stream, dim3(1024), dim3(256), 0, st, t.sh[0], t.sl[0], (size_t)M * MST_D,
                           pe_drop(seed, p_pe, (uint32_t)clip0 * S * MST_D));
        HIPCHECK(hipGetLastError());
    }
    CHECK(train_stack_forward(e, t, batch, S, p_drop, seed, nullptr, st, clip0));
    ws.hx = t.sh[nl];
    ws.hl = t.sl[nl];
    StepArgs sa{};
    return launch_out_nt<0>(e, ws, 0, batch, frames, out, sa, st, nullptr, nullptr, 1, false, true);
}

extern "C" int mst_train_model_backward(mst_engine* e, const void* tape, const float* d_out, int32_t batch, int32_t frames,
                                        float p_drop, float p_pe, uint64_t seed, float* d_x, float* const* grads, void* stream) {
    const int S = frames + 1;
    CHECK(train_check(e, batch, S, p_drop));
    if (!tape || !d_out) return fail("mst_train_model_backward: null argument");
    if (!grads && !d_x) return 0;
    hipStream_t st = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    CHECK(train_ws(e));
    TrainWS& w_ = e->tw;
    const int M = batch * S, nl = e->cfg.num_layers, F = e->cfg.feats, tot = batch * frames;
    Tape t;
    tape_layout((char*)const_cast<void*>(tape), nl, tape_rows(M), &t);
    const size_t n_out = (size_t)batch * F * frames, n = (size_t)M * MST_D;
    e->prof_now = 0;
    CHECK(grad_scale_from(e, d_out, n_out, st));
    // output projection backward: token-stream gradient rows = (scaled d_out as frame rows) x W_out; token 0 gets none
    hipLaunchKernelGGL(k_frames_f16, dim3((frames + 31) / 32, e->kin_pad / 32, batch), dim3(256), 0, st, d_out, F, frames, e->kin_pad, e->xt,
                       (const float*)w_.gscale, (const LoopDev*)nullptr, 0ull);
    hipLaunchKernelGGL(k_zero_token0, dim3((batch * MST_D + 255) / 256), dim3(256), 0, st, w_.g1, S, batch);
    HIPCHECK(hipGetLastError());
    {
        DEpiFramesGrad epi{w_.g1, frames, S, tot};
        CHECK((launch_gemm_dma<64, 512, 2, 2, 4, 1>(dim3((tot + 63) / 64, 1), RowsDirect{e->xt, e->kin_pad}, e->w_pose_outT, e->kin_pad,
                                                   e->kin_pad, epi, st)));
    }
    CHECK(train_stack_backward(e, t, batch, S, p_drop, seed, nullptr, grads, st));
    if (d_x) {
        if (p_pe > 0.f) {
            hipLaunchKernelGGL(k_mask_f32, dim3(1024), dim3(256), 0, st, w_.g1, n, pe_drop(seed, p_pe));
            HIPCHECK(hipGetLastError());
        }
        // pose embedding backward: d x[b][f][t] = sum_k W_in[k][f] g[b, 1 + t, k]  == the output-projection kernel with W_in^T
        hipLaunchKernelGGL(k_f32_to_f16, dim3(1024), dim3(256), 0, st, w_.g1, n, w_.datt);
        HIPCHECK(hipGetLastError());
        WS ws = ws_slice(e, 0, frames);
        ws.hx = w_.datt;
        StepArgs sa{};
        CHECK(launch_out_nt<0>(e, ws, 0, batch, frames, d_x, sa, st, e->w_pose_inT, w_.zeros));
        hipLaunchKernelGGL(k_scale_f32, dim3(1024), dim3(256), 0, st, d_x, n_out, w_.gscale, 1, d_x);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

// ---- MotionEncoder.forward (mdm_forstyledataset.py:90-124) as one native call: [muQuery | sigmaQuery | pose embedding of the
// frames] + positional rows (+ its dropout), the 8 key-padding-masked layers of THIS engine, token 0 of the result.
// key_keep: [batch][frames + 2] (1 = real key; the two query tokens are always 1).  The engine holds the encoder's own layers
// and the prior's input projection / positional table (engine.load_state_dict with prior_prefix "mdm_model.").
static int menc_check(mst_engine* e, int batch, int frames, float p_drop, float p_pe) {
    if (!e) return fail("null engine");
    const int S = frames + 2;
    if (frames < 1 || S > e->S_max) return fail("motion encoder: %d frames + 2 query tokens exceed the engine's %d tokens", frames, e->S_max);
    CHECK(train_check(e, batch, S, p_drop));
    if (!(p_pe >= 0.f && p_pe < 1.f)) return fail("motion encoder: positional-encoding dropout %g outside [0, 1)", (double)p_pe);
    return 0;
}

extern "C" int mst_motion_encoder_forward(mst_engine* e, const float* x, const float* mu_query, const float* sigma_query,
                                          const uint8_t* key_keep, int32_t batch, int32_t frames, float p_drop, float p_pe,
                                          uint64_t seed, void* tape, float* mu_out, void* stream) {
    CHECK(menc_check(e, batch, frames, p_drop, p_pe));
    CHECK(train_refuse_styles(e, "mst_motion_encoder_forward"));
    if (!x || !mu_query || !sigma_query || !tape || !mu_out) return fail("mst_motion_encoder_forward: null argument");
    hipStream_t st = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    const int S = frames + 2, M = batch * S, nl = e->cfg.num_layers, F = e->cfg.feats, tot = batch * frames;
    Tape t;
    tape_layout((char*)tape, nl, tape_rows(M), &t);
    e->prof_now = 0;
    hipLaunchKernelGGL(k_query_tokens, dim3((batch * 2 * MST_D + 255) / 256), dim3(256), 0, st, mu_query, sigma_query, e->pe, S, batch, t.sh[0], t.sl[0]);
    hipLaunchKernelGGL(k_frames_f16, dim3((frames + 31) / 32, e->kin_pad / 32, batch), dim3(256), 0, st, x, F, frames, e->kin_pad, e->xt,
                       (const float*)nullptr, (const LoopDev*)nullptr, 0ull);
    HIPCHECK(hipGetLastError());
    {
        DEpiEmbedIn epi{e->b_pose_in, e->pe, t.sh[0], t.sl[0], frames, S, tot, 0, 2};
        CHECK((launch_gemm_dma<64, 512, 2, 2, 4, 1>(dim3((tot + 63) / 64, 1), RowsDirect{e->xt, e->kin_pad}, e->w_pose_in, e->kin_pad, e->kin_pad, epi, st)));
    }
    if (p_pe > 0.f) {
        hipLaunchKernelGGL(k_dropout_stream, dim3(1024), dim3(256), 0, st, t.sh[0], t.sl[0], (size_t)M * MST_D, pe_drop(seed, p_pe));
        HIPCHECK(hipGetLastError());
    }
    CHECK(train_stack_forward(e, t, batch, S, p_drop, seed, key_keep, st));
    hipLaunchKernelGGL(k_gather_token0, dim3((batch * MST_D + 255) / 256), dim3(256), 0, st, t.sh[nl], t.sl[nl], S, batch, mu_out);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_motion_encoder_backward(mst_engine* e, const void* tape, const float* d_mu, const uint8_t* key_keep, int32_t batch,
                                           int32_t frames, float p_drop, float p_pe, uint64_t seed, float* d_x, void* stream) {
    CHECK(menc_check(e, batch, frames, p_drop, p_pe));
    if (!tape || !d_mu || !d_x) return fail("mst_motion_encoder_backward: null argument");
    hipStream_t st = (hipStream_t)stream;
    ON_DEVICE(e->cfg.device);
    CHECK(train_ws(e));
    TrainWS& w_ = e->tw;
    const int S = frames + 2, M = batch * S, nl = e->cfg.num_layers, F = e->cfg.feats;
    Tape t;
    tape_layout((char*)const_cast<void*>(tape), nl, tape_rows(M), &t);
    const size_t n = (size_t)M * MST_D, n_out = (size_t)batch * F * frames;
    e->prof_now = 0;
    CHECK(grad_scale_from(e, d_mu, (size_t)batch * MST_D, st));
    hipLaunchKernelGGL(k_seed_token0, dim3(2048), dim3(256), 0, st, d_mu, (const float*)w_.gscale, S, batch, w_.g1);   // only token 0 of every clip carries a gradient
    HIPCHECK(hipGetLastError());
    CHECK(train_stack_backward(e, t, batch, S, p_drop, seed, key_keep, nullptr, st));      // frozen stack: input gradient only
    if (p_pe > 0.f) {
        hipLaunchKernelGGL(k_mask_f32, dim3(1024), dim3(256), 0, st, w_.g1, n, pe_drop(seed, p_pe));
        HIPCHECK(hipGetLastError());
    }
    // pose embedding backward on the frame tokens (rows 2..): d x[b][f][t] = sum_k W_in[k][f] g[b, 2 + t, k]
    hipLaunchKernelGGL(k_f32_to_f16, dim3(1024), dim3(256), 0, st, w_.g1, n, w_.datt);
    HIPCHECK(hipGetLastError());
    WS ws = ws_slice(e, 0, frames);
    ws.hx = w_.datt;
    StepArgs sa{};
    CHECK(launch_out_nt<0>(e, ws, 0, batch, frames, d_x, sa, st, e->w_pose_inT, w_.zeros, 2));
    hipLaunchKernelGGL(k_scale_f32, dim3(1024), dim3(256), 0, st, d_x, n_out, w_.gscale, 1, d_x);
    HIPCHECK(hipGetLastError());
    return 0;
}

// keep-multipliers (0 or 1/(1-p)) of the first n elements of dropout site (layer, site) under `seed`:
// site 0 attention probabilities [(clip*4+head)][q][key], 1 out-proj output [tok][512], 2 FFN hidden [tok][1024],
// 3 FFN output [tok][512].  Lets a test rebuild the exact masked forward in PyTorch.
extern "C" int mst_dropout_mask(uint64_t seed, int32_t layer, int32_t site, float p, uint64_t n, float* out, void* stream) {
    if (!out || site < 0 || site > 3 || layer < 0 || !(p >= 0.f && p < 1.f) || n >= 0xFFFFFFFFull) return fail("mst_dropout_mask: bad arguments");
    hipLaunchKernelGGL(k_dropout_mask, dim3(1024), dim3(256), 0, (hipStream_t)stream, make_drop(seed, layer, site, p), (size_t)n, out);
    HIPCHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ optimizer ABI
extern "C" int64_t mst_adamw_workspace_bytes(int32_t n_tensors, const int64_t* numel) {
    if (n_tensors < 1 || !numel) return -1;
    int64_t chunks = 0;
    for (int i = 0; i < n_tensors; i++) chunks += (numel[i] + kAdamChunk - 1) / kAdamChunk;
    return (int64_t)n_tensors * (int64_t)sizeof(AdamTensor) + chunks * (int64_t)sizeof(AdamChunk) + 512 + chunks * 2 * (int64_t)sizeof(float);
}

extern "C" int mst_adamw_step(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                              float* const* exp_avg_sq, const int64_t* numel, float lr, float beta1, float beta2, float eps,
                              float weight_decay, int32_t step, float* norms_dev, void* workspace_dev, int64_t workspace_bytes,
                              int32_t upload_tables, void* stream) {
    if (n_tensors < 1 || !params || !grads || !exp_avg || !exp_avg_sq || !numel || !workspace_dev || step < 1)
        return fail("mst_adamw_step: bad arguments");
    if (workspace_bytes < mst_adamw_workspace_bytes(n_tensors, numel)) return fail("mst_adamw_step: workspace too small");
    size_t nchunks = 0;
    for (int i = 0; i < n_tensors; i++) {
        if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || numel[i] < 1) return fail("mst_adamw_step: null tensor %d", i);
        nchunks += (size_t)((numel[i] + kAdamChunk - 1) / kAdamChunk);
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace_dev;
    const size_t tb = sizeof(AdamTensor) * (size_t)n_tensors;
    const size_t tb_al = (tb + 255) / 256 * 256;
    // The tables change only when a tensor moves (a new gradient buffer) or the workspace is new: the owner of the
    // workspace tracks that (optim.FusedAdamW keeps the pointer tuple the tables were written from) and says so; the
    // library keeps no per-workspace state (a process-global cache keyed by the workspace address would survive the
    // workspace itself and hand a later optimizer stale tables).
    if (upload_tables) {
        std::vector<AdamTensor> tt(n_tensors);
        std::vector<AdamChunk> cc;
        cc.reserve(nchunks);
        for (int i = 0; i < n_tensors; i++) {
            tt[i] = AdamTensor{params[i], grads[i], exp_avg[i], exp_avg_sq[i], (long long)numel[i]};
            for (long long s0 = 0; s0 < numel[i]; s0 += kAdamChunk) cc.push_back(AdamChunk{i, 0, s0});
        }
        HIPCHECK(hipStreamSynchronize(st));                 // a previous step may still be reading the old tables
        HIPCHECK(hipMemcpy(ws, tt.data(), tb, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(ws + tb_al, cc.data(), sizeof(AdamChunk) * cc.size(), hipMemcpyHostToDevice));
    }
    const float bias1 = 1.0f - (float)pow((double)beta1, (double)step);
    const float bias2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    // grad / param norms: per-chunk partials behind the tables, summed in chunk order (no float atomics: the logged norms and
    // anything derived from them are bit-reproducible)
    float* norm_part = norms_dev ? (float*)(ws + tb_al + ((sizeof(AdamChunk) * nchunks + 255) / 256) * 256) : nullptr;
    hipLaunchKernelGGL(k_adamw_multi, dim3((unsigned)nchunks), dim3(256), 0, st, (const AdamTensor*)ws, (const AdamChunk*)(ws + tb_al),
                       lr, beta1, beta2, eps, weight_decay, bias1, bias2_sqrt, norm_part);
    HIPCHECK(hipGetLastError());
    if (norms_dev) {
        hipLaunchKernelGGL(k_adamw_norms, dim3(1), dim3(256), 0, st, norm_part, (int)nchunks, norms_dev);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ post-sampling ABI
// k_recover_from_ric keeps ang / px / pz / cs / sn, five fp32 rows of `frames` entries, in dynamic LDS: what one workgroup may ask for
// on the current device bounds the clip length, 4096 frames at the most.
extern "C" int mst_recover_max_frames(void) {
    int dev = 0, lds = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
        (void)hipGetLastError();
        fail("mst_recover_max_frames: the device's shared memory per block cannot be read");
        return -1;
    }
    const int n = lds / (int)(5 * sizeof(float));
    return n < 4096 ? n : 4096;
}
extern "C" int mst_recover_from_ric(const float* sample, const float* mean, const float* stdv, int32_t batch, int32_t feats,
                                    int32_t frames, int32_t joints, float* out, void* stream) {
    if (!sample || !mean || !stdv || !out || batch < 1 || frames < 1 || joints < 1) return fail("mst_recover_from_ric: bad arguments");
    if (feats < 4 + 3 * (joints - 1)) return fail("mst_recover_from_ric: %d features cannot hold %d joints", feats, joints);
    const int max_frames = mst_recover_max_frames();
    if (max_frames < 0) return 1;
    if (frames > max_frames)
        return fail("mst_recover_from_ric: frames %d > %d (five fp32 rows of `frames` entries in LDS, capped at 4096)", frames, max_frames);
    // (above 64 KB a launch needs the per-device opt-in; asked once, for the longest clip the device takes)
    if (sizeof(float) * 5 * frames > 64 * 1024) CHECK(ensure_dyn_lds((const void*)k_recover_from_ric, (int)sizeof(float) * 5 * max_frames));
    hipLaunchKernelGGL(k_recover_from_ric, dim3(batch), dim3(256), sizeof(float) * 5 * frames, (hipStream_t)stream, sample, mean, stdv,
                       feats, frames, joints, out);
    HIPCHECK(hipGetLastError());
    return 0;
}

// Joint-space guidance (mst_jguide.h): logp and d logp / d x0 in one launch.  k_joint_guide keeps 32 bytes a frame in dynamic LDS (three
// double rows, two fp32 rows) beside the scans' wave totals; the bound stays inside the 64 KB a launch gets without an opt-in.
extern "C" int mst_joint_guide_max_frames(void) {
    int dev = 0, lds = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
        (void)hipGetLastError();
        fail("mst_joint_guide_max_frames: the device's shared memory per block cannot be read");
        return -1;
    }
    const int n = (lds - 128) / kJgFrameBytes;
    return n < kJgMaxFrames ? n : kJgMaxFrames;
}
extern "C" int mst_joint_guide(const float* x0, const float* mean, const float* stdv, const float* target, const float* weight,
                               const float* scale, const int32_t* lengths, int32_t batch, int32_t feats, int32_t frames, int32_t joints,
                               float* logp, float* grad, float* positions, void* stream) {
    if (!x0 || !mean || !stdv || !target || !weight || !scale || !logp || !grad || batch < 1 || frames < 1 || joints < 1)
        return fail("mst_joint_guide: bad arguments");
    if (feats < 4 + 3 * (joints - 1)) return fail("mst_joint_guide: %d features cannot hold %d joints", feats, joints);
    const int max_frames = mst_joint_guide_max_frames();
    if (max_frames < 0) return 1;
    if (frames > max_frames)
        return fail("mst_joint_guide: frames %d > %d (mst_joint_guide_max_frames: 32 bytes a frame in LDS)", frames, max_frames);
    if ((long long)feats * frames > 0x7fffffffLL || (long long)frames * joints * 3 > 0x7fffffffLL)
        return fail("mst_joint_guide: a clip of %d x %d features and %d joints does not fit 32-bit offsets", feats, frames, joints);
    JGuideArgs a{x0, mean, stdv, target, weight, scale, lengths, feats, frames, joints, logp, grad, positions};
    hipLaunchKernelGGL(k_joint_guide, dim3(batch), dim3(kJgThreads), (size_t)kJgFrameBytes * frames, (hipStream_t)stream, a);
    HIPCHECK(hipGetLastError());
    return 0;
}

// Foot-skate cleanup (mst_feet.h).  The clip length is bounded by the two contact maps k_remove_fs keeps in LDS (8 bytes a frame) and
// capped where mst_recover_from_ric is, so that whatever that returns can be cleaned; the filter's forward result lives in the
// caller's workspace, not in LDS, so the bound does not fall with the joint count.
extern "C" int mst_remove_fs_max_frames(int32_t joints) {
    if (joints < 1) {
        fail("mst_remove_fs_max_frames: joints %d < 1", joints);
        return -1;
    }
    return kFeetMaxFrames;
}
// a, b, c, d, e of the reference's second-order recursion (bvh_utils.py:1889-1898), in double, with its literals
static void butterworth_coefficients(double cutoff, double* k) {
    const double rate = 1.0 / (1.0 / 20);
    const double pi = 3.14159265358979;
    const double wc = tan(cutoff * pi / rate);
    const double k1 = 1.414213562 * wc;
    const double k2 = wc * wc;
    const double a = k2 / (1 + k1 + k2);
    const double b = 2 * a;
    const double k3 = b / k2;
    k[0] = a;
    k[1] = b;
    k[2] = a;
    k[3] = -2 * a + k3;
    k[4] = 1 - (2 * a) - k3;
}
extern "C" int mst_remove_fs(const float* glb, const float* ref, int32_t ref_batch, const int32_t* lengths, int32_t batch, int32_t frames,
                             int32_t joints, const int32_t* foot_ids, int32_t use_vel3, float thr, int32_t use_window,
                             int32_t force_on_floor, int32_t interp_length, int32_t filter_before, int32_t filter_after, float* out,
                             int32_t* contacts, float* foot_vels, double* workspace, int64_t workspace_bytes, void* stream) {
    if (!glb || !foot_ids || batch < 1 || joints < 1 || interp_length < 0) return fail("mst_remove_fs: bad arguments");
    if (!out && !contacts && !foot_vels) return fail("mst_remove_fs: no output asked for");
    if (frames < 2) return fail("mst_remove_fs: frames %d < 2 (a one-frame clip has no velocity)", frames);
    const int max_frames = mst_remove_fs_max_frames(joints);
    if (frames > max_frames) return fail("mst_remove_fs: frames %d > %d (mst_remove_fs_max_frames)", frames, max_frames);
    if (ref && ref_batch != 1 && ref_batch != batch) return fail("mst_remove_fs: reference batch %d is neither 1 nor %d", ref_batch, batch);
    for (int i = 0; i < 4; i++) {
        if (foot_ids[i] < 0 || foot_ids[i] >= joints) return fail("mst_remove_fs: foot id %d outside 0..%d", foot_ids[i], joints - 1);
        for (int j = 0; j < i; j++)
            if (foot_ids[i] == foot_ids[j]) return fail("mst_remove_fs: duplicate foot id %d", foot_ids[i]);
    }
    const int64_t ws_need = (int64_t)sizeof(double) * batch * (frames - 1) * joints * 3;
    if (out && (filter_before || filter_after) && (!workspace || workspace_bytes < ws_need))
        return fail("mst_remove_fs: the filter needs a workspace of %lld bytes", (long long)ws_need);
    FeetArgs p{};
    p.in = glb;
    p.out = out;
    p.ref = ref;
    p.ref_stride = ref && ref_batch == batch && batch > 1 ? (long long)frames * joints * 3 : 0;
    p.lengths = lengths;
    p.T = frames;
    p.J = joints;
    for (int i = 0; i < 4; i++) p.fid[i] = foot_ids[i];
    p.vel3 = use_vel3 != 0;
    p.use_window = use_window != 0;
    p.force_on_floor = force_on_floor != 0;
    p.interp_length = interp_length;
    p.filter_before = filter_before != 0;
    p.filter_after = filter_after != 0;
    p.thr = thr;
    butterworth_coefficients(3, p.kb);
    butterworth_coefficients(2.5, p.ka);
    p.ws = out && (filter_before || filter_after) ? workspace : nullptr;
    p.contacts = contacts;
    p.foot_vels = foot_vels;
    hipLaunchKernelGGL(k_remove_fs, dim3(batch), dim3(256), (size_t)8 * frames, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}

// Joint-rotation fit (mst_ik.h).  k_ik_solve keeps a lane's parameters, both Adam moments and its target in LDS, [slot][64 lanes]; the
// joint count is bounded by that, the clip length by the three rows k_ik_init keeps for the running sums (48 KB at the cap, which
// every device gives a workgroup without an opt-in: the bound needs no device to be asked).
extern "C" int mst_fit_joints_max_joints(void) { return kIkMaxJoints; }
extern "C" int mst_fit_joints_max_frames(int32_t joints) {
    if (joints < 2 || joints > kIkMaxJoints) {
        fail("mst_fit_joints_max_frames: joints %d outside 2..%d", joints, kIkMaxJoints);
        return -1;
    }
    return kIkMaxFrames;
}
extern "C" int mst_fit_joints(const float* data, int64_t stride_batch, int64_t stride_frame, int64_t stride_feat, const float* mean,
                              const float* stdv, const float* target, const int32_t* lengths, int32_t batch, int32_t frames,
                              int32_t feats, int32_t joints, const int32_t* parents, const float* offsets, int32_t iters,
                              int32_t true_gradient, float* cont6d, float* r_pos, float* r_rot_quat, float* positions,
                              float* joint_quats, float* frame_loss, float* grad, void* stream) {
    if (joints < 2 || joints > kIkMaxJoints) return fail("mst_fit_joints: joints %d outside 2..%d (mst_fit_joints_max_joints)", joints, kIkMaxJoints);
    if (iters < 1) return fail("mst_fit_joints: iters %d < 1", iters);
    if (feats != 9 * joints + 1) return fail("mst_fit_joints: feats %d != 9 * %d + 1 (the position-rotation vector)", feats, joints);
    if (frames < 1) return fail("mst_fit_joints: frames %d < 1", frames);
    if (batch < 1) return fail("mst_fit_joints: batch %d < 1", batch);
    if (!parents || !offsets) return fail("mst_fit_joints: null skeleton");
    for (int j = 1; j < joints; j++)
        if (parents[j] < 0 || parents[j] >= j)
            return fail("mst_fit_joints: parents[%d] = %d: not a tree rooted at 0 with parents[j] < j", j, parents[j]);
    if (!data || !target || !cont6d || !r_pos || !r_rot_quat || !positions || !joint_quats) return fail("mst_fit_joints: null argument");
    if ((mean == nullptr) != (stdv == nullptr)) return fail("mst_fit_joints: mean and std come together");
    const int max_frames = mst_fit_joints_max_frames(joints);
    if (max_frames < 0) return 1;
    if (frames > max_frames) return fail("mst_fit_joints: frames %d > %d (mst_fit_joints_max_frames)", frames, max_frames);
    int dev = 0, lds = 0;
    HIPCHECK(hipGetDevice(&dev));
    HIPCHECK(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    const size_t solve_lds = sizeof(float) * kIkLanes * (21 * (size_t)joints + 21);
    if (solve_lds > (size_t)lds) return fail("mst_fit_joints: %d joints need %zu bytes of LDS, the device gives a workgroup %d", joints, solve_lds, lds);
    IkArgs p{};
    p.data = data;
    p.sb = stride_batch;
    p.st = stride_frame;
    p.sf = stride_feat;
    p.mean = mean;
    p.stdv = stdv;
    p.target = target;
    p.lengths = lengths;
    p.B = batch;
    p.T = frames;
    p.J = joints;
    p.iters = iters;
    p.true_gradient = true_gradient != 0;
    for (int j = 0; j < joints; j++) p.leaf[j] = 1;
    for (int j = 0; j < joints; j++) {
        p.parents[j] = j ? parents[j] : 0;
        if (j) p.leaf[parents[j]] = 0;
        for (int k = 0; k < 3; k++) p.off[j][k] = offsets[3 * j + k];
    }
    p.cont6d = cont6d;
    p.r_pos = r_pos;
    p.r_rot = r_rot_quat;
    p.positions = positions;
    p.quats = joint_quats;
    p.frame_loss = frame_loss;
    p.grad = grad;
    const size_t init_lds = sizeof(float) * 3 * frames;      // at most 48 KB: below the opt-in threshold
    hipLaunchKernelGGL(k_ik_init, dim3(batch), dim3(256), init_lds, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    if (solve_lds > 64 * 1024)
        CHECK(ensure_dyn_lds((const void*)k_ik_solve, (int)(sizeof(float) * kIkLanes * (21 * kIkMaxJoints + 21))));
    const long long lanes = (long long)batch * frames;
    hipLaunchKernelGGL(k_ik_solve, dim3((unsigned)((lanes + kIkLanes - 1) / kIkLanes)), dim3(kIkLanes), solve_lds, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}

// Motion encoder (mst_encode.h).  k_encode keeps two fp32 rows of the per-frame forward direction and one root quaternion a frame in
// LDS, 24 bytes a frame whatever the joint count or the mode: 48 KB at the cap, which every device gives a workgroup without an opt-in.
extern "C" int mst_encode_max_frames(int32_t joints, int32_t mode) {
    if (joints < 2 || joints > kEncMaxJoints || (mode != kEncPosRot && mode != kEncHml)) {
        fail("mst_encode_max_frames: joints %d outside 2..%d or mode %d neither 0 (POSROT) nor 1 (HML)", joints, kEncMaxJoints, mode);
        return -1;
    }
    return kEncMaxFrames;
}
// The kinematic chains, link by link in the reference's order (common/skeleton.py:88-103), into the tables k_encode and k_retarget walk.
static int enc_fill_links(const char* who, EncArgs& p, int joints, const int32_t* chains, const int32_t* chain_starts, int num_chains) {
    bool placed[kEncMaxJoints] = {true};
    for (int c = 0; c < num_chains; c++) {
        const int lo = chain_starts[c], hi = chain_starts[c + 1];
        if (lo < 0 || hi <= lo) return fail("%s: chain %d is empty", who, c);
        for (int k = lo; k < hi; k++)
            if (chains[k] < 0 || chains[k] >= joints) return fail("%s: joint %d of chain %d outside 0..%d", who, chains[k], c, joints - 1);
        if (!placed[chains[lo]]) return fail("%s: chain %d starts at joint %d, which no earlier chain has placed", who, c, chains[lo]);
        for (int k = lo + 1; k < hi; k++) {
            if (placed[chains[k]]) return fail("%s: joint %d is named twice as a child (chain %d)", who, chains[k], c);
            placed[chains[k]] = true;
            p.link_child[p.n_links] = chains[k];
            p.link_parent[p.n_links] = chains[k - 1];
            p.link_first[p.n_links] = k == lo + 1;
            p.named[chains[k]] = 1;
            p.n_links++;
        }
    }
    return 0;
}
extern "C" int mst_encode_motion(const float* positions, const float* rotations, const int32_t* lengths, const float* mean, const float* stdv,
                                 int32_t batch, int32_t frames, int32_t joints, int32_t mode, const int32_t* face_ids,
                                 const int32_t* foot_ids, const int32_t* chains, const int32_t* chain_starts, int32_t num_chains,
                                 const float* raw_offsets, float feet_thre, int32_t frames_out, float* sample, int32_t* lengths_out,
                                 float* global_positions, float* local_positions, float* l_velocity, void* stream) {
    if (mode != kEncPosRot && mode != kEncHml) return fail("mst_encode_motion: mode %d is neither 0 (POSROT) nor 1 (HML)", mode);
    if (joints < 2 || joints > kEncMaxJoints) return fail("mst_encode_motion: joints %d outside 2..%d", joints, kEncMaxJoints);
    if (batch < 1) return fail("mst_encode_motion: batch %d < 1", batch);
    if (frames < 2) return fail("mst_encode_motion: frames %d < 2 (a one-frame clip has no velocity row)", frames);
    if (frames_out < 1) return fail("mst_encode_motion: frames_out %d < 1", frames_out);
    const int max_frames = mst_encode_max_frames(joints, mode);
    if (frames > max_frames) return fail("mst_encode_motion: frames %d > %d (mst_encode_max_frames)", frames, max_frames);
    if (!positions || !sample || !lengths_out || !face_ids) return fail("mst_encode_motion: null argument");
    if (mode == kEncPosRot && !rotations) return fail("mst_encode_motion: POSROT needs the rotations");
    if ((mean == nullptr) != (stdv == nullptr)) return fail("mst_encode_motion: mean and std come together");
    for (int i = 0; i < 4; i++) {
        if (face_ids[i] < 0 || face_ids[i] >= joints) return fail("mst_encode_motion: face joint %d outside 0..%d", face_ids[i], joints - 1);
        for (int j = 0; j < i; j++)
            if (face_ids[i] == face_ids[j]) return fail("mst_encode_motion: duplicate face joint %d", face_ids[i]);
    }
    if (mode == kEncHml && (!foot_ids || !chains || !chain_starts || num_chains < 1 || !raw_offsets))
        return fail("mst_encode_motion: HML needs foot ids, kinematic chains and raw offsets");
    EncArgs p{};
    if (foot_ids)
        for (int i = 0; i < 4; i++) {
            if (foot_ids[i] < 0 || foot_ids[i] >= joints) return fail("mst_encode_motion: foot joint %d outside 0..%d", foot_ids[i], joints - 1);
            p.fid[i] = foot_ids[i];
        }
    if (chains && chain_starts && num_chains > 0) CHECK(enc_fill_links("mst_encode_motion", p, joints, chains, chain_starts, num_chains));
    if (raw_offsets)
        for (int j = 0; j < joints; j++)
            for (int k = 0; k < 3; k++) p.raw[j][k] = raw_offsets[3 * j + k];
    {   // scipy.ndimage._gaussian_kernel1d(sigma 20, order 0, radius 80), in double
        double sum = 0.0;
        for (int k = -kEncRadius; k <= kEncRadius; k++) sum += exp(-0.5 / (20.0 * 20.0) * (double)(k * k));
        for (int k = 0; k <= kEncRadius; k++) p.taps[k] = exp(-0.5 / (20.0 * 20.0) * (double)(k * k)) / sum;
    }
    p.pos = positions;
    p.rot = rotations;
    p.lengths = lengths;
    p.mean = mean;
    p.stdv = stdv;
    p.B = batch;
    p.T = frames;
    p.J = joints;
    p.mode = mode;
    p.frames_out = frames_out;
    p.feats = mode == kEncPosRot ? 9 * joints + 1 : 12 * joints - 1;
    p.feet_thre = feet_thre;
    for (int i = 0; i < 4; i++) p.face[i] = face_ids[i];
    p.sample = sample;
    p.out_len = lengths_out;
    p.glob = global_positions;
    p.local = local_positions;
    p.lvel = l_velocity;
    hipLaunchKernelGGL(k_encode, dim3(batch), dim3(kEncThreads), sizeof(float) * 6 * frames, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}

// Motion files (mst_bvh.h).  The decode keeps one scan bit a joint and wave in LDS and everything a frame needs in the caller's workspace,
// so neither bound depends on the device: the joint cap is what the kernel arguments and the lane's two 64-bit scan registers hold, the
// frame cap what one workgroup should walk (see the constants).
extern "C" int mst_bvh_max_joints(void) { return kBvhMaxJoints; }
extern "C" int mst_bvh_max_frames(int32_t joints) {
    if (joints < 1 || joints > kBvhMaxJoints) {
        fail("mst_bvh_max_frames: joints %d outside 1..%d (mst_bvh_max_joints)", joints, kBvhMaxJoints);
        return -1;
    }
    return kBvhMaxFrames;
}
extern "C" int mst_bvh_decode(const float* channels, const int32_t* lengths, int32_t batch, int32_t frames, int32_t num_channels,
                              int32_t joints, const int32_t* parents, const int32_t* rot_cols, const int32_t* pos_cols, const float* offsets,
                              const int32_t* order, float scale, int32_t stride, int32_t phase, const int32_t* select, int32_t num_select,
                              float* workspace, float* rotations, float* positions, float* local_positions, float* global_rotations,
                              void* stream) {
    if (joints < 1 || joints > kBvhMaxJoints) return fail("mst_bvh_decode: joints %d outside 1..%d (mst_bvh_max_joints)", joints, kBvhMaxJoints);
    if (batch < 1) return fail("mst_bvh_decode: batch %d < 1", batch);
    if (frames < 1) return fail("mst_bvh_decode: frames %d < 1", frames);
    if (frames > kBvhMaxFrames) return fail("mst_bvh_decode: frames %d > %d (mst_bvh_max_frames)", frames, kBvhMaxFrames);
    if (num_channels < 3 || num_channels > 6 * joints) return fail("mst_bvh_decode: %d channels outside 3..6 * %d", num_channels, joints);
    if (stride < 1) return fail("mst_bvh_decode: stride %d < 1", stride);
    if (phase < 0 || phase >= stride) return fail("mst_bvh_decode: phase %d outside 0..%d", phase, stride - 1);
    if (phase >= frames) return fail("mst_bvh_decode: phase %d leaves no frame of %d", phase, frames);
    if (num_select < 0 || num_select > kBvhMaxSel) return fail("mst_bvh_decode: %d selected joints outside 0..%d", num_select, kBvhMaxSel);
    if (!channels || !parents || !rot_cols || !pos_cols || !offsets || !order || !workspace || !rotations || !positions || (num_select && !select))
        return fail("mst_bvh_decode: null argument");
    if (!(order[0] >= 0 && order[0] <= 2 && order[1] >= 0 && order[1] <= 2 && order[2] >= 0 && order[2] <= 2) || order[0] == order[1] ||
        order[1] == order[2] || order[0] == order[2])
        return fail("mst_bvh_decode: rotation order (%d, %d, %d) is no permutation of the axes 0, 1, 2", order[0], order[1], order[2]);
    BvhArgs p{};
    if (parents[0] != -1) return fail("mst_bvh_decode: parents[0] = %d: joint 0 is the root (-1)", parents[0]);
    for (int j = 0; j < joints; j++) {
        if (j && (parents[j] < 0 || parents[j] >= j))
            return fail("mst_bvh_decode: parents[%d] = %d: not a tree rooted at 0 with parents[j] < j", j, parents[j]);
        if (rot_cols[j] < -1 || rot_cols[j] + 3 > num_channels) return fail("mst_bvh_decode: rotation column %d of joint %d outside the %d channels", rot_cols[j], j, num_channels);
        if (pos_cols[j] < -1 || pos_cols[j] + 3 > num_channels) return fail("mst_bvh_decode: position column %d of joint %d outside the %d channels", pos_cols[j], j, num_channels);
        p.parent[j] = (short)parents[j];
        p.rot_col[j] = (short)rot_cols[j];
        p.pos_col[j] = (short)pos_cols[j];
        for (int k = 0; k < 3; k++) p.off[j][k] = offsets[3 * j + k];
    }
    for (int s = 0; s < num_select; s++) {
        const int j = select[s];
        if (j < 0 || j >= joints) return fail("mst_bvh_decode: selected joint %d outside 0..%d", j, joints - 1);
        for (int q = 0; q < s; q++)
            if (select[q] == j) return fail("mst_bvh_decode: joint %d is selected twice", j);
        int anc = parents[j];
        while (anc >= 0) {                   // the nearest selected ancestor
            bool in = false;
            for (int q = 0; q < num_select; q++) in = in || select[q] == anc;
            if (in) break;
            anc = parents[anc];
        }
        p.sel[s] = (short)j;
        p.sel_anc[s] = (short)anc;
        p.sel_direct[s] = anc == parents[j];            // the file parent itself, or the file's root (both -1)
    }
    p.ch = channels;
    p.lengths = lengths;
    p.B = batch;
    p.T = frames;
    p.C = num_channels;
    p.Jf = joints;
    p.nsel = num_select;
    p.stride = stride;
    p.phase = phase;
    p.Tout = (frames - phase + stride - 1) / stride;
    p.scale = scale;
    for (int k = 0; k < 3; k++) p.axis[k] = order[k];
    p.ws = workspace;
    p.rot = rotations;
    p.pos = positions;
    p.lpos = local_positions;
    p.grot = global_rotations;
    hipLaunchKernelGGL(k_bvh_decode, dim3(batch), dim3(kBvhThreads), 0, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_quats_to_channels(const float* quats, const float* root_pos, const float* positions, const int32_t* perm, int32_t batch,
                                     int32_t frames, int32_t joints, int32_t order, float* out, void* stream) {
    if (joints < 1 || joints > kBvhMaxJoints) return fail("mst_quats_to_channels: joints %d outside 1..%d (mst_bvh_max_joints)", joints, kBvhMaxJoints);
    if (batch < 1 || frames < 1) return fail("mst_quats_to_channels: %d clips of %d frames", batch, frames);
    if (order != kQ2cZyx && order != kQ2cXzy)
        return fail("mst_quats_to_channels: order %d is neither 0 ('zyx') nor 1 ('xzy'), the file orders whose reverse q2eul converts", order);
    if (!quats || !root_pos || !perm || !out) return fail("mst_quats_to_channels: null argument");
    Q2cArgs p{};
    bool seen[kBvhMaxJoints] = {};
    for (int s = 0; s < joints; s++) {
        if (perm[s] < 0 || perm[s] >= joints || seen[perm[s]]) return fail("mst_quats_to_channels: perm[%d] = %d: not a permutation of 0..%d", s, perm[s], joints - 1);
        seen[perm[s]] = true;
        p.perm[s] = (short)perm[s];
    }
    if (perm[0] != 0) return fail("mst_quats_to_channels: perm[0] = %d: the root is written first", perm[0]);
    p.quats = quats;
    p.root_pos = root_pos;
    p.positions = positions;
    p.B = batch;
    p.T = frames;
    p.J = joints;
    p.order = order;
    p.out = out;
    const long long n = (long long)batch * frames * joints;
    hipLaunchKernelGGL(k_quats_to_channels, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_retarget_max_frames(int32_t joints) {
    if (joints < 2 || joints > kEncMaxJoints) {
        fail("mst_retarget_max_frames: joints %d outside 2..%d", joints, kEncMaxJoints);
        return -1;
    }
    return kRetMaxFrames;
}
extern "C" int mst_retarget_joints(const float* positions, const int32_t* lengths, int32_t batch, int32_t frames, int32_t joints,
                                   const int32_t* face_ids, const int32_t* chains, const int32_t* chain_starts, int32_t num_chains,
                                   const float* raw_offsets, const float* target_offsets, const int32_t* leg_ids, float* out, void* stream) {
    if (joints < 2 || joints > kEncMaxJoints) return fail("mst_retarget_joints: joints %d outside 2..%d", joints, kEncMaxJoints);
    if (batch < 1) return fail("mst_retarget_joints: batch %d < 1", batch);
    if (frames < 1) return fail("mst_retarget_joints: frames %d < 1", frames);
    if (frames > kRetMaxFrames) return fail("mst_retarget_joints: frames %d > %d (mst_retarget_max_frames)", frames, kRetMaxFrames);
    if (!positions || !face_ids || !chains || !chain_starts || num_chains < 1 || !raw_offsets || !target_offsets || !leg_ids || !out)
        return fail("mst_retarget_joints: null argument");
    if (out == positions) return fail("mst_retarget_joints: the output may not be the input");
    EncArgs p{};
    RetArgs x{};
    for (int i = 0; i < 4; i++) {
        if (face_ids[i] < 0 || face_ids[i] >= joints) return fail("mst_retarget_joints: face joint %d outside 0..%d", face_ids[i], joints - 1);
        for (int j = 0; j < i; j++)
            if (face_ids[i] == face_ids[j]) return fail("mst_retarget_joints: duplicate face joint %d", face_ids[i]);
        p.face[i] = face_ids[i];
    }
    CHECK(enc_fill_links("mst_retarget_joints", p, joints, chains, chain_starts, num_chains));
    for (int a = 0; a < 2; a++) {
        if (leg_ids[a] < 1 || leg_ids[a] >= joints) return fail("mst_retarget_joints: leg joint %d outside 1..%d", leg_ids[a], joints - 1);
        x.leg[a] = leg_ids[a];
        x.leg_parent[a] = 0;                 // common/skeleton.py:11-15: a joint no chain names hangs off the root
        for (int l = 0; l < p.n_links; l++)
            if (p.link_child[l] == leg_ids[a]) x.leg_parent[a] = p.link_parent[l];
    }
    for (int j = 0; j < joints; j++)
        for (int k = 0; k < 3; k++) {
            p.raw[j][k] = raw_offsets[3 * j + k];
            x.tgt[j][k] = target_offsets[3 * j + k];
        }
    for (int a = 0; a < 2; a++) {
        float m = 0.f;
        for (int k = 0; k < 3; k++) m = fmaxf(m, fabsf(x.tgt[x.leg[a]][k]));
        x.tgt_leg += m;
    }
    p.pos = positions;
    p.lengths = lengths;
    p.B = batch;
    p.T = frames;
    p.J = joints;
    x.out = out;
    hipLaunchKernelGGL(k_retarget, dim3(batch), dim3(kEncThreads), 0, (hipStream_t)stream, p, x);
    HIPCHECK(hipGetLastError());
    return 0;
}

// Rotation-channel decode (mst_rotdec.h).  Nothing a frame needs is kept in LDS (96 bytes of wave totals for the three scans), so the
// frame bound is the same for every joint count; the joint bound is the chain state a lane keeps in scratch memory (16 floats a joint).
extern "C" int mst_rot_decode_max_joints(void) { return kRotMaxJoints; }
extern "C" int mst_rot_decode_max_frames(int32_t joints) {
    if (joints < 2 || joints > kRotMaxJoints) {
        fail("mst_rot_decode_max_frames: joints %d outside 2..%d", joints, kRotMaxJoints);
        return -1;
    }
    return kRotMaxFrames;
}
extern "C" int mst_rot_decode(const float* data, int64_t stride_batch, int64_t stride_frame, int64_t stride_feat, const float* mean,
                              const float* stdv, const int32_t* lengths, int32_t batch, int32_t frames, int32_t feats, int32_t joints,
                              int32_t route, const int32_t* chains, const int32_t* chain_starts, int32_t num_chains, const float* offsets,
                              const int32_t* face_ids, const float* raw_offsets, const int32_t* out_source, const int32_t* out_parents, int32_t out_joints, float* quats, float* root_pos,
                              float* joint_pos, float* local_rows, void* stream) {
    if (route != kRotHml && route != kRotReal && route != kRotPosIk)
        return fail("mst_rot_decode: route %d is none of 0 (HML_ROT), 1 (REAL_ROT), 2 (POS_IK)", route);
    if (joints < 2 || joints > kRotMaxJoints) return fail("mst_rot_decode: joints %d outside 2..%d (mst_rot_decode_max_joints)", joints, kRotMaxJoints);
    const int want = route != kRotReal ? 12 * joints - 1 : 9 * joints + 1;
    if (feats != want)
        return fail("mst_rot_decode: feats %d != %s = %d, the row of route %d", feats, route != kRotReal ? "12 * joints - 1" : "9 * joints + 1", want, route);
    if (frames < 1) return fail("mst_rot_decode: frames %d < 1", frames);
    if (frames > kRotMaxFrames) return fail("mst_rot_decode: frames %d > %d (mst_rot_decode_max_frames)", frames, kRotMaxFrames);
    if (batch < 1 || batch > 65535) return fail("mst_rot_decode: batch %d outside 1..65535", batch);
    if (!data) return fail("mst_rot_decode: null data");
    if ((mean == nullptr) != (stdv == nullptr)) return fail("mst_rot_decode: mean and std come together");
    if (!chains || !chain_starts || num_chains < 1 || !offsets) return fail("mst_rot_decode: null skeleton (chains, chain starts, offsets)");
    if (!quats && !root_pos && !joint_pos && !local_rows) return fail("mst_rot_decode: no output asked for");
    if (local_rows && route != kRotReal) return fail("mst_rot_decode: the local rows (process_pos_from_real_rot) belong to route 1 (REAL_ROT)");
    RotArgs p{};
    {
        bool placed[kRotMaxJoints] = {true};
        for (int c = 0; c < num_chains; c++) {
            const int lo = chain_starts[c], hi = chain_starts[c + 1];
            if (lo < 0 || hi - lo < 2) return fail("mst_rot_decode: chain %d has fewer than two joints", c);
            for (int k = lo; k < hi; k++)
                if (chains[k] < 0 || chains[k] >= joints) return fail("mst_rot_decode: joint %d of chain %d outside 0..%d", chains[k], c, joints - 1);
            if (!placed[chains[lo]]) return fail("mst_rot_decode: chain %d starts at joint %d, which no earlier chain has placed", c, chains[lo]);
            for (int k = lo + 1; k < hi; k++) {
                if (placed[chains[k]]) return fail("mst_rot_decode: joint %d is named twice as a child (chain %d)", chains[k], c);
                placed[chains[k]] = true;
                p.link_child[p.n_links] = (signed char)chains[k];
                p.link_parent[p.n_links] = (signed char)chains[k - 1];
                p.link_first[p.n_links] = k == lo + 1;
                p.n_links++;
            }
        }
        for (int j = 0; j < joints; j++)
            if (!placed[j]) return fail("mst_rot_decode: joint %d is named by no chain", j);
    }
    if (route == kRotPosIk) {
        if (!face_ids || !raw_offsets) return fail("mst_rot_decode: route 2 (POS_IK) needs the face joints and the raw offsets");
        for (int i = 0; i < 4; i++) {
            if (face_ids[i] < 0 || face_ids[i] >= joints) return fail("mst_rot_decode: face joint %d outside 0..%d", face_ids[i], joints - 1);
            p.face[i] = face_ids[i];
        }
        for (int j = 0; j < joints; j++)
            for (int k = 0; k < 3; k++) p.raw[j][k] = raw_offsets[3 * j + k];
        // scipy.ndimage._gaussian_kernel1d(sigma 20, order 0, radius 80), in double
        double sum = 0.0;
        for (int k = -kRotRadius; k <= kRotRadius; k++) sum += exp(-0.5 / (20.0 * 20.0) * (double)(k * k));
        for (int k = 0; k <= kRotRadius; k++) p.taps[k] = exp(-0.5 / (20.0 * 20.0) * (double)(k * k)) / sum;
    }
    if (route != kRotReal) {
        if (quats) {
            if (!out_source || !out_parents) return fail("mst_rot_decode: routes 0 and 2 write quaternions on the expanded skeleton: null gather map or parents");
            if (out_joints < joints || out_joints > kRotMaxOut) return fail("mst_rot_decode: out_joints %d outside %d..%d", out_joints, joints, kRotMaxOut);
            for (int i = 0; i < out_joints; i++) {
                if (out_source[i] < -1 || out_source[i] >= joints)
                    return fail("mst_rot_decode: out_source[%d] = %d names no joint of 0..%d (-1: identity)", i, out_source[i], joints - 1);
                if (i && (out_parents[i] < 0 || out_parents[i] >= out_joints))
                    return fail("mst_rot_decode: out_parents[%d] = %d outside 0..%d", i, out_parents[i], out_joints - 1);
                p.src[i] = (signed char)out_source[i];
                p.xparent[i] = (signed char)(i ? out_parents[i] : -1);
            }
        }
        p.Jx = quats ? out_joints : joints;
    } else {
        if (out_joints != joints) return fail("mst_rot_decode: route 1 writes the J local quaternions: out_joints %d != joints %d", out_joints, joints);
        p.Jx = joints;
    }
    for (int j = 0; j < joints; j++)
        for (int k = 0; k < 3; k++) p.off[j][k] = offsets[3 * j + k];
    p.data = data;
    p.sb = stride_batch;
    p.st = stride_frame;
    p.sf = stride_feat;
    p.mean = mean;
    p.stdv = stdv;
    p.lengths = lengths;
    p.B = batch;
    p.T = frames;
    p.J = joints;
    p.mode = route;
    p.quats = quats;
    p.root_pos = root_pos;
    p.joints = joint_pos;
    p.local = local_rows;
    const size_t lds = route == kRotPosIk ? sizeof(float) * 2 * frames : 0;      // at most 32 KB: below the opt-in threshold
    hipLaunchKernelGGL(k_rot_decode, dim3(batch), dim3(kRotThreads), lds, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ the SMPL body (mst_smpl.h)
static int smpl_counts(const char* who, int32_t live, int32_t vertices) {
    if (vertices <= 0) return fail("%s: %d vertices", who, vertices);
    if (live < 1) return fail("%s: %d live frames", who, live);
    if ((int64_t)live * vertices * 3 >= ((int64_t)1 << 40)) return fail("%s: %d frames x %d vertices is beyond any device", who, live, vertices);
    return 0;
}
extern "C" int64_t mst_smpl_packed_bytes(int32_t vertices) {
    if (vertices <= 0) {
        fail("mst_smpl_packed_bytes: %d vertices", vertices);
        return -1;
    }
    return (int64_t)((vertices + kSmplTileV - 1) / kSmplTileV) * kSmplTileFloats * 4;
}
extern "C" int64_t mst_smpl_workspace_bytes(int32_t live, int32_t vertices, int32_t keep_vertices) {
    if (smpl_counts("mst_smpl_workspace_bytes", live, vertices)) return -1;
    return smpl_carve(nullptr, live, vertices, keep_vertices != 0).bytes;
}
extern "C" int mst_smpl_pack_body(const float* posedirs, const float* shapedirs, int32_t vertices, float* packed, void* stream) {
    if (vertices <= 0) return fail("mst_smpl_pack_body: %d vertices", vertices);
    if (!posedirs || !shapedirs || !packed) return fail("mst_smpl_pack_body: null posedirs, shapedirs or destination");
    const int64_t total = mst_smpl_packed_bytes(vertices) / 4;
    hipLaunchKernelGGL(k_smpl_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, posedirs, shapedirs, packed, vertices, total);
    HIPCHECK(hipGetLastError());
    return 0;
}
extern "C" int mst_smpl_pose(const float* x, int64_t stride_batch, int64_t stride_joint, int64_t stride_feat, int64_t stride_frame,
                             const int32_t* frame_ids, int32_t live, int32_t batch, int32_t frames, int32_t sample_joints, int32_t joints,
                             int32_t vertices, int32_t keep_vertices, int32_t pose_rep, int32_t glob, const float* glob_rot, const float* betas, float beta, const float* j0,
                             const float* jdirs, const int32_t* parents, int32_t trans_joint, void* workspace, float* rotations,
                             float* joints_out, void* stream) {
    if (joints != kSmplJoints) return fail("mst_smpl_pose: a body of %d joints; only SMPL's %d are built", joints, kSmplJoints);
    if (!x || !j0 || !jdirs || !parents || !workspace) return fail("mst_smpl_pose: null sample, joint tables, parents or workspace");
    CHECK(smpl_counts("mst_smpl_pose", live, vertices));
    if (batch < 1 || frames < 1 || (int64_t)batch * frames > INT32_MAX) return fail("mst_smpl_pose: %d clips of %d frames", batch, frames);
    if (!frame_ids && (batch != 1 || live != frames)) return fail("mst_smpl_pose: without frame ids every frame of ONE clip is live (batch %d, live %d, frames %d)", batch, live, frames);
    if (live > (int64_t)batch * frames) return fail("mst_smpl_pose: %d live frames in %d clips of %d", live, batch, frames);
    if (pose_rep < kSmplRot6d || pose_rep > kSmplRotvec) return fail("mst_smpl_pose: pose_rep %d is none of 0 (rot6d), 1 (rotmat), 2 (rotquat), 3 (rotvec)", pose_rep);
    const int need = glob ? kSmplJoints : kSmplJoints - 1;
    if (sample_joints < need) return fail("mst_smpl_pose: the sample has %d rotation rows, %d are read (glob %d)", sample_joints, need, glob != 0);
    if (!glob && !glob_rot) return fail("mst_smpl_pose: glob = 0 needs the global rotation");
    if (trans_joint >= 0 && !joints_out) return fail("mst_smpl_pose: a translation row without a joints output");
    if (parents[0] != -1) return fail("mst_smpl_pose: parents[0] = %d, the root's is -1", parents[0]);
    SmplPoseArgs p{};
    for (int j = 1; j < kSmplJoints; j++) {
        if (parents[j] < 0 || parents[j] >= j) return fail("mst_smpl_pose: parents[%d] = %d is not an earlier joint", j, parents[j]);
        p.parents[j] = (signed char)parents[j];
    }
    p.parents[0] = -1;
    const SmplWorkspace ws = smpl_carve(workspace, live, vertices, keep_vertices != 0);
    p.x = x; p.sb = stride_batch; p.sj = stride_joint; p.sf = stride_feat; p.st = stride_frame;
    p.frame_ids = frame_ids; p.N = live; p.B = batch; p.T = frames; p.rep = pose_rep; p.glob = glob != 0;
    if (glob_rot)
        for (int c = 0; c < 3; c++) p.glob_rot[c] = glob_rot[c];
    p.betas = betas; p.beta = beta; p.J0 = j0; p.Jdirs = jdirs; p.trans_joint = trans_joint;
    p.A = ws.A; p.rows = ws.rows; p.posed = ws.posed; p.rot = rotations; p.out = joints_out;
    hipLaunchKernelGGL(k_smpl_pose, dim3((live + 63) / 64), dim3(64), 0, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}
extern "C" int mst_smpl_skin(const float* packed, const float* v_template, const float* weights, int32_t vertices, int32_t keep_vertices, const int32_t* frame_ids,
                             int32_t live, int32_t batch, int32_t frames, void* workspace, const float* trans, int64_t trans_stride_batch,
                             int64_t trans_stride_axis, int64_t trans_stride_frame, float* out, int64_t out_stride_batch, int64_t out_stride_frame,
                             int64_t out_stride_vertex, int64_t out_stride_axis, void* stream) {
    if (!packed || !v_template || !weights || !workspace) return fail("mst_smpl_skin: null body arrays or workspace");
    CHECK(smpl_counts("mst_smpl_skin", live, vertices));
    if (batch < 1 || frames < 1 || (int64_t)batch * frames > INT32_MAX) return fail("mst_smpl_skin: %d clips of %d frames", batch, frames);
    if (!out && !keep_vertices) return fail("mst_smpl_skin: no output: neither a destination nor the workspace's vertices");
    if (out && !frame_ids && (batch != 1 || live != frames)) return fail("mst_smpl_skin: without frame ids every frame of ONE clip is live");
    if (!out && trans) return fail("mst_smpl_skin: the workspace's vertices carry no translation");
    const SmplWorkspace ws = smpl_carve(workspace, live, vertices, keep_vertices != 0);
    SmplSkinArgs p{};
    p.packed = packed; p.v_template = v_template; p.weights = weights; p.A = ws.A; p.rows = ws.rows;
    p.N = live; p.V = vertices; p.T = frames; p.B = batch;
    if (out) {
        p.frame_ids = frame_ids; p.trans = trans; p.tb = trans_stride_batch; p.tc = trans_stride_axis; p.tt = trans_stride_frame;
        p.out = out; p.ob = out_stride_batch; p.ot = out_stride_frame; p.ov = out_stride_vertex; p.oc = out_stride_axis;
    } else {                                 // [N][V][3] for k_smpl_regress: frame n as frame n of one clip
        p.frame_ids = nullptr; p.B = 1; p.T = live;
        p.out = ws.verts; p.ob = 0; p.ot = (int64_t)vertices * 3; p.ov = 3; p.oc = 1;
    }
    CHECK(ensure_dyn_lds((const void*)k_smpl_skin, kSmplTileFloats * 4));
    // frame tiles are dealt to 8 waves x `split` workgroups a vertex tile: enough workgroups to cover the chip when the body is small.
    // A tile's arithmetic does not depend on which wave runs it.
    const int vt = (vertices + kSmplTileV - 1) / kSmplTileV, ft = (live + 15) / 16, per = kSmplSkinThreads / 64;
    const int split = std::max(1, std::min((ft + per - 1) / per, (512 + vt - 1) / vt));
    hipLaunchKernelGGL(k_smpl_skin, dim3(vt, split), dim3(kSmplSkinThreads), kSmplTileFloats * 4, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}
extern "C" int mst_smpl_regress(void* workspace, const float* extra, const int32_t* vertex_ids, int32_t vertices, const int32_t* frame_ids,
                                int32_t live, int32_t batch, int32_t frames, const int32_t* map, int32_t map_len, int32_t root,
                                const float* trans, int64_t trans_stride_batch, int64_t trans_stride_axis, int64_t trans_stride_frame,
                                float* out, void* stream) {
    if (!workspace || !extra || !vertex_ids || !map || !out) return fail("mst_smpl_regress: null workspace, regressor, vertex ids, joint map or output");
    CHECK(smpl_counts("mst_smpl_regress", live, vertices));
    if (batch < 1 || frames < 1 || (int64_t)batch * frames > INT32_MAX) return fail("mst_smpl_regress: %d clips of %d frames", batch, frames);
    if (!frame_ids && (batch != 1 || live != frames)) return fail("mst_smpl_regress: without frame ids every frame of ONE clip is live");
    if (map_len < 1 || map_len > kSmplAllJoints) return fail("mst_smpl_regress: a list of %d joints outside 1..%d", map_len, kSmplAllJoints);
    if (root < -1 || root >= map_len) return fail("mst_smpl_regress: root %d outside the list of %d (-1: none subtracted)", root, map_len);
    SmplRegressArgs p{};
    for (int i = 0; i < kSmplVertexIds; i++) {
        if (vertex_ids[i] < 0 || vertex_ids[i] >= vertices) return fail("mst_smpl_regress: vertex id %d outside 0..%d", vertex_ids[i], vertices - 1);
        p.vertex_ids[i] = vertex_ids[i];
    }
    for (int i = 0; i < map_len; i++) {
        if (map[i] < 0 || map[i] >= kSmplAllJoints) return fail("mst_smpl_regress: map[%d] = %d outside 0..%d", i, map[i], kSmplAllJoints - 1);
        p.map[i] = map[i];
    }
    const SmplWorkspace ws = smpl_carve(workspace, live, vertices, true);
    p.verts = ws.verts; p.posed = ws.posed; p.extra = extra; p.frame_ids = frame_ids; p.N = live; p.V = vertices; p.T = frames; p.B = batch;
    p.map_len = map_len; p.root = root; p.trans = trans; p.tb = trans_stride_batch; p.tc = trans_stride_axis; p.tt = trans_stride_frame;
    p.out = out;
    hipLaunchKernelGGL(k_smpl_regress, dim3(live), dim3(256), 0, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ the SMPLify-3D objective (mst_smplify.h)
extern "C" int64_t mst_smplify_packed_prior_bytes(void) { return (int64_t)kFitPackedFloats * 4; }
extern "C" int mst_smplify_pack_prior(const float* precisions, const float* means, const float* neg_log_weights, void* packed, void* stream) {
    if (!precisions || !means || !neg_log_weights || !packed) return fail("mst_smplify_pack_prior: null precisions, means, constants or destination");
    hipLaunchKernelGGL(k_smplify_pack, dim3((kFitPackedFloats + 255) / 256), dim3(256), 0, (hipStream_t)stream, precisions, means, neg_log_weights, (float*)packed);
    HIPCHECK(hipGetLastError());
    return 0;
}
extern "C" int64_t mst_smplify_workspace_bytes(int32_t frames) {
    if (frames < 1) {
        fail("mst_smplify_workspace_bytes: %d frames", frames);
        return -1;
    }
    return ((int64_t)frames * kFitJoints * 3 * 4 + 255) / 256 * 256;
}
extern "C" int mst_smplify_objective(int32_t stage, int32_t nj, int32_t frames, const float* body_pose, const float* global_orient, const float* betas,
                                     const float* camera_translation, const float* target, const float* conf, const float* preserve,
                                     const float* camera_estimate, const float* j0, const float* jdirs, const int32_t* parents,
                                     const void* packed_prior, const mst_smplify_weights* weights, void* workspace, float* per_frame,
                                     float* loss, float* grad_body_pose, float* grad_global_orient, float* grad_betas,
                                     float* grad_camera_translation, float* rotations, void* stream) {
    if (stage != kFitCamera && stage != kFitBody) return fail("mst_smplify_objective: stage %d is neither 0 (camera) nor 1 (body)", stage);
    if (nj != 22 && nj != kFitJoints) return fail("mst_smplify_objective: %d target joints; 22 (AMASS) or 24 (orig)", nj);
    if (frames < 1) return fail("mst_smplify_objective: %d frames", frames);
    if (!body_pose || !global_orient || !betas || !camera_translation || !target || !j0 || !jdirs || !parents || !weights || !workspace || !per_frame)
        return fail("mst_smplify_objective: null pose, orientation, betas, camera translation, target, joint tables, parents, weights, workspace or per-frame loss");
    if (stage == kFitBody && (!conf || !preserve || !packed_prior)) return fail("mst_smplify_objective: the body stage needs the confidences, the preserved pose and the packed prior");
    if (stage == kFitCamera && !camera_estimate) return fail("mst_smplify_objective: the camera stage needs the camera estimate");
    if (stage == kFitCamera && (grad_body_pose || grad_betas)) return fail("mst_smplify_objective: the camera stage has no body-pose or betas gradient");
    if (parents[0] != -1) return fail("mst_smplify_objective: parents[0] = %d, the root's is -1", parents[0]);
    FitArgs p{};
    for (int j = 1; j < kFitJoints; j++) {
        if (parents[j] < 0 || parents[j] >= j) return fail("mst_smplify_objective: parents[%d] = %d is not an earlier joint", j, parents[j]);
        p.parents[j] = (signed char)parents[j];
    }
    p.parents[0] = -1;
    p.stage = stage; p.nj = nj; p.N = frames; p.pose = body_pose; p.orient = global_orient; p.betas = betas; p.cam = camera_translation;
    p.target = target; p.conf = conf; p.preserve = preserve; p.cam_est = camera_estimate; p.J0 = j0; p.Jdirs = jdirs;
    p.packed = (const float*)packed_prior;
    p.sel[0] = 2; p.sel[1] = 1; p.sel[2] = 17; p.sel[3] = 16;       // RHip, LHip, RShoulder, LShoulder in both joint categories
    p.sigma = weights->sigma; p.w_joint = weights->joint; p.w_prior = weights->prior; p.w_angle = weights->angle; p.w_shape = weights->shape;
    p.w_keep = weights->keep; p.w_depth = weights->depth;
    p.per_frame = per_frame; p.joints = (float*)workspace; p.g_pose = grad_body_pose; p.g_orient = grad_global_orient; p.g_betas = grad_betas;
    p.g_cam = grad_camera_translation; p.rot = rotations;
    hipLaunchKernelGGL(k_smplify, dim3((frames + kFitFrames - 1) / kFitFrames), dim3(64), 0, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    if (loss) {
        hipLaunchKernelGGL(k_smplify_sum, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)per_frame, frames, loss);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ pose tracks (mst_track.h)
// Neither kernel keeps anything on chip, so the bounds are sanity checks on the arguments and the same on every device.
extern "C" int mst_track_max_frames(int32_t joints) {
    if (joints < 1 || joints > kTrackMaxJoints) {
        fail("mst_track_max_frames: joints %d outside 1..%d", joints, kTrackMaxJoints);
        return -1;
    }
    return kTrackMaxFrames;
}
static int track_rate(const char* what, int32_t batch, int32_t frames, int32_t up, int32_t down) {
    if (batch < 1) return fail("%s: batch %d < 1", what, batch);
    if (frames < 2) return fail("%s: frames %d < 2: a track is resampled interval by interval", what, frames);
    if (frames > kTrackMaxFrames) return fail("%s: frames %d > %d (mst_track_max_frames)", what, frames, kTrackMaxFrames);
    if (up < 1 || up > kTrackMaxRate || down < 1 || down > kTrackMaxRate) return fail("%s: rate %d / %d: each outside 1..%d", what, up, down, kTrackMaxRate);
    return 0;
}
static int track_out_frames(int32_t frames, int32_t up, int32_t down) { return (int)(((long long)(frames - 1) * up + down - 1) / down); }

extern "C" int mst_track_resample(const float* quats, const float* points, const int32_t* lengths, int32_t batch, int32_t frames,
                                  int32_t joints, int32_t num_points, int32_t up, int32_t down, int32_t shortest, float* quats_out,
                                  float* points_out, void* stream) {
    CHECK(track_rate("mst_track_resample", batch, frames, up, down));
    if (joints < 0 || joints > kTrackMaxJoints) return fail("mst_track_resample: joints %d outside 0..%d", joints, kTrackMaxJoints);
    if (num_points < 0 || num_points > kTrackMaxJoints) return fail("mst_track_resample: points %d outside 0..%d", num_points, kTrackMaxJoints);
    if (joints + num_points < 1) return fail("mst_track_resample: neither a rotation track nor a point track");
    if ((joints > 0) != (quats != nullptr) || (joints > 0) != (quats_out != nullptr))
        return fail("mst_track_resample: %d joints but the rotation track or its output is %s", joints, joints ? "null" : "given");
    if ((num_points > 0) != (points != nullptr) || (num_points > 0) != (points_out != nullptr))
        return fail("mst_track_resample: %d points but the point track or its output is %s", num_points, num_points ? "null" : "given");
    if ((quats && quats_out == quats) || (points && points_out == points)) return fail("mst_track_resample: an output may not be its input");
    TrackResampleArgs p{};
    p.quats = quats; p.points = points; p.lengths = lengths; p.B = batch; p.T = frames; p.J = joints; p.P = num_points;
    p.Tout = track_out_frames(frames, up, down); p.up = up; p.down = down; p.shortest = shortest != 0;
    p.quats_out = quats_out; p.points_out = points_out;
    const long long n = (long long)batch * p.Tout * (joints + num_points), blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail("mst_track_resample: %lld outputs are more than one launch takes", n);
    hipLaunchKernelGGL(k_track_resample, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_track_joints(const float* rotations, int32_t is_matrix, int32_t rot_joints, const float* transl, const float* betas,
                                const float* est_joints, int32_t est_joint_count, const int32_t* lengths, int32_t batch, int32_t frames,
                                int32_t up, int32_t down, int32_t shortest, int32_t with_trans, const float* j0, const float* jdirs,
                                const int32_t* parents, float* out, float* est_out, void* stream) {
    CHECK(track_rate("mst_track_joints", batch, frames, up, down));
    if (batch > 65535) return fail("mst_track_joints: batch %d > 65535", batch);
    if (rot_joints < kTrackChain || rot_joints > kTrackMaxJoints)
        return fail("mst_track_joints: %d rotations a frame outside %d..%d (the chain reads the first %d)", rot_joints, kTrackChain, kTrackMaxJoints, kTrackChain);
    if (!rotations || !betas || !j0 || !jdirs || !parents || !out) return fail("mst_track_joints: null rotations, betas, joint tables, parents or output");
    if (with_trans && !transl) return fail("mst_track_joints: with_trans without a translation track");
    if ((est_joints != nullptr) != (est_out != nullptr)) return fail("mst_track_joints: the estimator's joint track and its output come together");
    if (est_joints && (est_joint_count < kTrackChain || est_joint_count > kTrackMaxJoints))
        return fail("mst_track_joints: %d estimator joints a frame outside %d..%d", est_joint_count, kTrackChain, kTrackMaxJoints);
    if (parents[0] != -1) return fail("mst_track_joints: parents[0] = %d, the root's is -1", parents[0]);
    TrackJointsArgs p{};
    p.parents[0] = -1;
    for (int j = 1; j < kTrackChain; j++) {
        if (parents[j] < 0 || parents[j] >= j) return fail("mst_track_joints: parents[%d] = %d is not an earlier joint", j, parents[j]);
        p.parents[j] = (signed char)parents[j];
    }
    p.rot = rotations; p.rot_mat = is_matrix != 0; p.Jr = rot_joints; p.transl = transl; p.betas = betas; p.extra = est_joints;
    p.Je = est_joints ? est_joint_count : 0; p.lengths = lengths; p.B = batch; p.T = frames; p.Tout = track_out_frames(frames, up, down);
    p.up = up; p.down = down; p.shortest = shortest != 0; p.with_trans = with_trans != 0; p.J0 = j0; p.Jdirs = jdirs; p.out = out;
    p.extra_out = est_out;
    hipLaunchKernelGGL(k_track_joints, dim3((p.Tout + kTrackThreads - 1) / kTrackThreads, batch), dim3(kTrackThreads), 0, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ clips to video frames (mst_render.h)
extern "C" int mst_render_max_frames(void) { return kRenderMaxFrames; }
extern "C" int mst_render_max_joints(void) { return kRenderMaxJoints; }
extern "C" int mst_render_chains_drawn(void) { return kRenderChains; }
extern "C" int mst_render_max_traces(void) { return kRenderMaxTraces; }
extern "C" int mst_render_max_side(void) { return kRenderMaxSide; }
extern "C" int mst_render_chunk(void) { return kRenderChunk; }

static int render_scene(const char* what, const mst_render_scene* s, RenderArgs& p) {
    if (!s) return fail("%s: null scene", what);
    if (s->batch < 1 || s->batch > 65535) return fail("%s: batch %d outside 1..65535", what, s->batch);
    if (s->frames < 1 || s->frames > kRenderMaxFrames) return fail("%s: frames %d outside 1..%d (mst_render_max_frames)", what, s->frames, kRenderMaxFrames);
    if (s->joints < 1 || s->joints > kRenderMaxJoints) return fail("%s: joints %d outside 1..%d (mst_render_max_joints)", what, s->joints, kRenderMaxJoints);
    if (!s->joints_dev) return fail("%s: null joints", what);
    if (s->stride_batch < 1 || s->stride_frame < 1 || s->stride_joint < 1 || s->stride_coord < 1)
        return fail("%s: strides %lld, %lld, %lld, %lld: each at least 1 element", what, (long long)s->stride_batch, (long long)s->stride_frame,
                    (long long)s->stride_joint, (long long)s->stride_coord);
    if (!(s->scale == s->scale) || s->scale - s->scale != 0.f) return fail("%s: scale is not finite", what);
    p.joints = s->joints_dev; p.joints2 = s->joints2_dev; p.sB = s->stride_batch; p.sT = s->stride_frame; p.sJ = s->stride_joint;
    p.sC = s->stride_coord; p.lengths = s->lengths_dev; p.B = s->batch; p.T = s->frames; p.J = s->joints; p.scale = s->scale;
    return 0;
}

extern "C" int mst_render_bounds(const mst_render_scene* scene, float* bounds, void* stream) {
    RenderArgs p{};
    CHECK(render_scene("mst_render_bounds", scene, p));
    if (!bounds) return fail("mst_render_bounds: null bounds");
    if ((const void*)bounds == (const void*)p.joints || (const void*)bounds == (const void*)p.joints2 || (const void*)bounds == (const void*)p.lengths)
        return fail("mst_render_bounds: the output may not be an input");
    hipLaunchKernelGGL(k_render_bounds, dim3(p.B), dim3(kRenderThreads), 0, (hipStream_t)stream, p, bounds);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_render_frames(const mst_render_scene* scene, const float* bounds, const mst_render_view* v, uint8_t* out, float* out_float,
                                 void* stream) {
    const char* what = "mst_render_frames";
    RenderArgs p{};
    CHECK(render_scene(what, scene, p));
    if (!v) return fail("%s: null view", what);
    if (!bounds || !out) return fail("%s: null bounds or output", what);
    if (v->width < kRenderMinSide || v->width > kRenderMaxSide || v->height < kRenderMinSide || v->height > kRenderMaxSide)
        return fail("%s: image %d x %d: each side %d..%d (mst_render_max_side)", what, v->width, v->height, kRenderMinSide, kRenderMaxSide);
    if (v->n_chains < 0 || v->n_chains > kRenderMaxChains) return fail("%s: %d chains outside 0..%d", what, v->n_chains, kRenderMaxChains);
    if (v->n_chains > 0 && (!v->chain_offsets_host || !v->chain_joints_host)) return fail("%s: %d chains but null chain tables", what, v->n_chains);
    if (v->n_chains > 0 && v->chain_offsets_host[0] != 0) return fail("%s: chain offsets start at %d, not 0", what, v->chain_offsets_host[0]);
    for (int c = 0; c < v->n_chains; c++) {
        const int o = v->chain_offsets_host[c], e = v->chain_offsets_host[c + 1];
        if (e < o || e - o > kRenderMaxChainPoints) return fail("%s: chain %d holds %d points, outside 0..%d", what, c, e - o, kRenderMaxChainPoints);
        for (int i = o; i < e; i++)
            if (v->chain_joints_host[i] < 0 || v->chain_joints_host[i] >= p.J)
                return fail("%s: chain %d names joint %d, outside 0..%d", what, c, v->chain_joints_host[i], p.J - 1);
    }
    p.n_chains = v->n_chains < kRenderChains ? v->n_chains : kRenderChains;     // every chain is checked, the first five are drawn
    if (p.n_chains > 0 && v->chain_offsets_host[p.n_chains] > kRenderMaxChainPoints)
        return fail("%s: the %d chains drawn hold %d points, more than %d", what, p.n_chains, v->chain_offsets_host[p.n_chains], kRenderMaxChainPoints);
    for (int c = 0; c <= p.n_chains; c++) p.chain_off[c] = (unsigned char)(p.n_chains ? v->chain_offsets_host[c] : 0);
    for (int i = 0; i < p.chain_off[p.n_chains]; i++) p.chain_joint[i] = (unsigned char)v->chain_joints_host[i];
    if (v->n_traces < 0 || v->n_traces > kRenderMaxTraces) return fail("%s: %d traces outside 0..%d (mst_render_max_traces)", what, v->n_traces, kRenderMaxTraces);
    if (v->n_traces > 0 && (!v->trace_kinds_host || !v->trace_joints_host)) return fail("%s: %d traces but null trace tables", what, v->n_traces);
    for (int i = 0; i < v->n_traces; i++) {
        if (v->trace_kinds_host[i] < 0 || v->trace_kinds_host[i] > 2) return fail("%s: trace %d of kind %d, outside 0..2", what, i, v->trace_kinds_host[i]);
        if (v->trace_joints_host[i] < 0 || v->trace_joints_host[i] >= p.J)
            return fail("%s: trace %d names joint %d, outside 0..%d", what, i, v->trace_joints_host[i], p.J - 1);
        p.trace_kind[i] = (unsigned char)v->trace_kinds_host[i];
        p.trace_joint[i] = (unsigned char)v->trace_joints_host[i];
    }
    p.n_traces = v->n_traces;
    if (v->overlay_dev && v->overlay_batch != 1 && v->overlay_batch != p.B)
        return fail("%s: an overlay of %d images for %d clips: 1 or the batch", what, v->overlay_batch, p.B);
    if (!(v->t0 >= 0 && v->t0 < v->t1 && v->t1 <= p.T)) return fail("%s: frame range %d..%d is not 0 <= t0 < t1 <= %d", what, v->t0, v->t1, p.T);
    if (!(v->dpi > 0.f) || v->dpi - v->dpi != 0.f) return fail("%s: dpi is not a positive finite number", what);
    const void* ins[] = {p.joints, p.joints2, p.lengths, bounds, v->palette_dev, v->overlay_dev};
    for (const void* in : ins)
        if (in && (in == (const void*)out || in == (const void*)out_float)) return fail("%s: an output may not be an input", what);
    if ((const void*)out == (const void*)out_float) return fail("%s: the two outputs may not be one buffer", what);
    p.bounds = bounds; p.palette = v->palette_dev;
    for (int r = 0; r < 2; r++)
        for (int c = 0; c < 4; c++) p.M[4 * r + c] = v->proj[4 * r + c];
    for (int c = 0; c < 4; c++) p.M[8 + c] = v->proj[12 + c];                  // the depth row is not read: nothing is depth-tested
    for (int i = 0; i < 6; i++) p.A[i] = v->affine[i];
    p.W = v->width; p.H = v->height;
    // line widths of 4 pt and 2 pt: w = pt * dpi / 72 pixels formed in double and rounded once, the reach w / 2 + 0.5 in float32
    const float w_chain = (float)(4.0 * (double)v->dpi / 72.0), w_trace = (float)(2.0 * (double)v->dpi / 72.0);
    p.reach_chain = w_chain * 0.5f + 0.5f; p.reach_trace = w_trace * 0.5f + 0.5f;
    p.overlay = v->overlay_dev; p.overlay_batch = v->overlay_batch; p.t0 = v->t0; p.frames_out = v->t1 - v->t0; p.out = out; p.outf = out_float;
    const int tiles = ((p.W + kRenderTile - 1) / kRenderTile) * ((p.H + kRenderTile - 1) / kRenderTile);
    hipLaunchKernelGGL(k_render_frames, dim3(tiles, p.frames_out, p.B), dim3(kRenderThreads), 0, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ meshes to video frames (mst_mesh.h)
extern "C" int mst_mesh_max_vertices(void) { return kMeshMaxVertices; }
extern "C" int mst_mesh_max_faces(void) { return kMeshMaxFaces; }
extern "C" int mst_mesh_max_side(void) { return kMeshMaxSide; }
extern "C" int mst_mesh_max_samples(void) { return kMeshMaxSamples; }
extern "C" int mst_mesh_chunk(void) { return kMeshChunk; }

extern "C" uint64_t mst_mesh_workspace_bytes(int32_t batch, int32_t frames_out, int32_t vertices) {
    if (batch < 1 || frames_out < 1 || vertices < 1 || vertices > kMeshMaxVertices) return 0;
    return (uint64_t)batch * (uint64_t)frames_out * (uint64_t)mesh_frame_floats(vertices) * sizeof(float);
}

static bool mesh_finite(const float* a, int n) {
    for (int i = 0; i < n; i++)
        if (!(a[i] - a[i] == 0.f)) return false;
    return true;
}

static int mesh_scene(const char* what, const mst_mesh_scene* s, bool topology, MeshArgs& p) {
    if (!s) return fail("%s: null scene", what);
    if (s->batch < 1 || s->batch > 65535) return fail("%s: batch %d outside 1..65535", what, s->batch);
    if (s->frames < 1 || s->frames > kMeshMaxFrames) return fail("%s: frames %d outside 1..%d", what, s->frames, kMeshMaxFrames);
    if (s->vertices < 1 || s->vertices > kMeshMaxVertices)
        return fail("%s: vertices %d outside 1..%d (mst_mesh_max_vertices)", what, s->vertices, kMeshMaxVertices);
    if (!s->vertices_dev) return fail("%s: null vertices", what);
    if (s->stride_batch < 1 || s->stride_frame < 1 || s->stride_vertex < 1 || s->stride_coord < 1)
        return fail("%s: strides %lld, %lld, %lld, %lld: each at least 1 element", what, (long long)s->stride_batch, (long long)s->stride_frame,
                    (long long)s->stride_vertex, (long long)s->stride_coord);
    p.verts = s->vertices_dev; p.sB = s->stride_batch; p.sT = s->stride_frame; p.sV = s->stride_vertex; p.sC = s->stride_coord;
    p.lengths = s->lengths_dev; p.B = s->batch; p.T = s->frames; p.V = s->vertices;
    if (!topology) return 0;
    const int V = s->vertices, F = s->faces;
    if (F < 1 || F > kMeshMaxFaces) return fail("%s: faces %d outside 1..%d (mst_mesh_max_faces)", what, F, kMeshMaxFaces);
    if (!s->faces_host || !s->faces_dev) return fail("%s: null faces (a host copy and a device copy)", what);
    if (!s->adj_offsets_host || !s->adj_offsets_dev || !s->adj_faces_host || !s->adj_faces_dev)
        return fail("%s: null adjacency (host and device copies of the offsets and of the face lists)", what);
    for (int i = 0; i < 3 * F; i++)
        if (s->faces_host[i] < 0 || s->faces_host[i] >= V)
            return fail("%s: face %d names vertex %d, outside 0..%d", what, i / 3, s->faces_host[i], V - 1);
    if (s->adj_offsets_host[0] != 0 || s->adj_offsets_host[V] != 3 * F)
        return fail("%s: adjacency rows sum to %d from %d, not to 3 x faces = %d from 0", what, s->adj_offsets_host[V], s->adj_offsets_host[0], 3 * F);
    for (int v = 0; v < V; v++)
        if (s->adj_offsets_host[v + 1] < s->adj_offsets_host[v]) return fail("%s: adjacency offsets fall at vertex %d", what, v);
    for (int i = 0; i < 3 * F; i++)
        if (s->adj_faces_host[i] < 0 || s->adj_faces_host[i] >= F)
            return fail("%s: adjacency entry %d names face %d, outside 0..%d", what, i, s->adj_faces_host[i], F - 1);
    p.F = F; p.faces = s->faces_dev; p.adj_off = s->adj_offsets_dev; p.adj_face = s->adj_faces_dev;
    return 0;
}

static int mesh_view(const char* what, const mst_mesh_view* v, void* ws, uint64_t ws_bytes, MeshArgs& p) {
    if (!v) return fail("%s: null view", what);
    if (!v->proj_host || !v->proj_dev) return fail("%s: null matrix (a host copy and a device copy)", what);
    if (v->proj_batch != 1 && v->proj_batch != p.B) return fail("%s: %d matrices for %d clips: 1 or the batch", what, v->proj_batch, p.B);
    if (!mesh_finite(v->proj_host, 16 * v->proj_batch) || !mesh_finite(v->affine, 6)) return fail("%s: a matrix or the affine is not finite", what);
    if (v->width < kMeshMinSide || v->width > kMeshMaxSide || v->height < kMeshMinSide || v->height > kMeshMaxSide)
        return fail("%s: image %d x %d: each side %d..%d (mst_mesh_max_side)", what, v->width, v->height, kMeshMinSide, kMeshMaxSide);
    if (v->samples < 1 || v->samples > kMeshMaxSamples) return fail("%s: samples %d outside 1..%d (mst_mesh_max_samples)", what, v->samples, kMeshMaxSamples);
    if (v->ids_sample < 0 || v->ids_sample >= v->samples * v->samples)
        return fail("%s: ids_sample %d outside 0..%d", what, v->ids_sample, v->samples * v->samples - 1);
    if (!mesh_finite(v->light, 3) || !mesh_finite(&v->ambient, 1) || !mesh_finite(v->background, 4))
        return fail("%s: the light, ambient or background is not finite", what);
    if (!(v->t0 >= 0 && v->t0 < v->t1 && v->t1 <= p.T)) return fail("%s: frame range %d..%d is not 0 <= t0 < t1 <= %d", what, v->t0, v->t1, p.T);
    if (!ws) return fail("%s: null workspace", what);
    const uint64_t need = mst_mesh_workspace_bytes(p.B, v->t1 - v->t0, p.V);
    if (ws_bytes < need)
        return fail("%s: workspace of %llu bytes, mst_mesh_workspace_bytes says %llu", what, (unsigned long long)ws_bytes, (unsigned long long)need);
    if (((uintptr_t)ws & 3) != 0) return fail("%s: the workspace is not 4-byte aligned", what);
    p.proj = v->proj_dev; p.proj_batch = v->proj_batch;
    for (int i = 0; i < 6; i++) p.A[i] = v->affine[i];
    p.W = v->width; p.H = v->height;
    for (int i = 0; i < 3; i++) p.light[i] = v->light[i];
    p.ambient = v->ambient; p.colors = v->colors_dev;
    for (int i = 0; i < 4; i++) p.bg[i] = v->background[i];
    p.t0 = v->t0; p.frames_out = v->t1 - v->t0; p.ids_sample = v->ids_sample; p.ws = (float*)ws;
    return 0;
}

extern "C" int mst_mesh_bounds(const mst_mesh_scene* scene, float* bounds, void* stream) {
    MeshArgs p{};
    CHECK(mesh_scene("mst_mesh_bounds", scene, false, p));
    if (!bounds) return fail("mst_mesh_bounds: null bounds");
    if ((const void*)bounds == (const void*)p.verts || (const void*)bounds == (const void*)p.lengths)
        return fail("mst_mesh_bounds: the output may not be an input");
    hipLaunchKernelGGL(k_mesh_bounds, dim3(p.B), dim3(kMeshThreads), 0, (hipStream_t)stream, p, bounds);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_mesh_vertices(const mst_mesh_scene* scene, const mst_mesh_view* view, void* workspace, uint64_t workspace_bytes, void* stream) {
    const char* what = "mst_mesh_vertices";
    MeshArgs p{};
    CHECK(mesh_scene(what, scene, true, p));
    CHECK(mesh_view(what, view, workspace, workspace_bytes, p));
    const void* ins[] = {p.verts, p.lengths, p.faces, p.adj_off, p.adj_face, p.proj, p.colors};
    for (const void* in : ins)
        if (in && in == (const void*)workspace) return fail("%s: the workspace may not be an input", what);
    hipLaunchKernelGGL(k_mesh_vertices, dim3(mesh_blocks(p.V), p.frames_out, p.B), dim3(kMeshThreads), 0, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_mesh_frames(const mst_mesh_scene* scene, const mst_mesh_view* view, const void* workspace, uint64_t workspace_bytes, uint8_t* out,
                               float* out_float, int32_t* out_ids, void* stream) {
    const char* what = "mst_mesh_frames";
    MeshArgs p{};
    CHECK(mesh_scene(what, scene, true, p));
    CHECK(mesh_view(what, view, const_cast<void*>(workspace), workspace_bytes, p));
    if (!out) return fail("%s: null output", what);
    if (((uintptr_t)out & 3) != 0 || ((uintptr_t)out_float & 15) != 0 || ((uintptr_t)out_ids & 3) != 0)
        return fail("%s: the image is 4-byte aligned, the float image 16-byte, the face-index image 4-byte", what);
    const void* ins[] = {p.verts, p.lengths, p.faces, p.adj_off, p.adj_face, p.proj, p.colors, workspace};
    for (const void* in : ins)
        if (in && (in == (const void*)out || in == (const void*)out_float || in == (const void*)out_ids)) return fail("%s: an output may not be an input", what);
    if ((const void*)out == (const void*)out_float || (const void*)out == (const void*)out_ids || (out_float && (const void*)out_float == (const void*)out_ids))
        return fail("%s: the outputs may not share a buffer", what);
    p.out = out; p.outf = out_float; p.ids = out_ids;
    const dim3 grid(((p.W + kMeshTile - 1) / kMeshTile) * ((p.H + kMeshTile - 1) / kMeshTile), p.frames_out, p.B), block(kMeshThreads);
    switch (view->samples) {
        case 1: hipLaunchKernelGGL(k_mesh_frames<1>, grid, block, 0, (hipStream_t)stream, p); break;
        case 2: hipLaunchKernelGGL(k_mesh_frames<2>, grid, block, 0, (hipStream_t)stream, p); break;
        case 3: hipLaunchKernelGGL(k_mesh_frames<3>, grid, block, 0, (hipStream_t)stream, p); break;
        default: hipLaunchKernelGGL(k_mesh_frames<4>, grid, block, 0, (hipStream_t)stream, p); break;
    }
    HIPCHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ evaluators and statistics (mst_eval.h)
static bool eval_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int mst_eval_gemm(const float* a, const float* w, const float* bias, const float* add, float* c, int32_t m, int32_t n, int32_t k,
                             int64_t lda, int64_t ldc, int64_t ldadd, int32_t mode, int32_t batch, int32_t frames_in, int32_t channels,
                             int64_t ldx, int64_t stride_batch, const float* scale, const float* shift, int32_t leaky, void* stream) {
    if (!a || !w || !c) return fail("mst_eval_gemm: null operand");
    if (m < 1 || n < 1 || k < 1) return fail("mst_eval_gemm: M %d, N %d, K %d: each at least 1", m, n, k);
    if ((m + EVAL_BM - 1) / EVAL_BM > 65535) return fail("mst_eval_gemm: M %d above %d rows", m, 65535 * EVAL_BM);
    if (ldc < n) return fail("mst_eval_gemm: ldc %lld < N %d", (long long)ldc, n);
    if (add && ldadd < n) return fail("mst_eval_gemm: ldadd %lld < N %d", (long long)ldadd, n);
    if ((scale == nullptr) != (shift == nullptr)) return fail("mst_eval_gemm: scale and shift come together");
    EvalGemmArgs p{};
    p.a = a; p.w = w; p.bias = bias; p.add = add; p.scale = scale; p.shift = shift; p.c = c;
    p.M = m; p.N = n; p.K = k; p.mode = mode; p.leaky = leaky != 0;
    p.lda = lda; p.ldc = ldc; p.ldadd = ldadd; p.ldx = ldx; p.sb = stride_batch;
    p.Tin = 1; p.Tout = 1; p.C = 1;
    if (mode == kEvalPlain) {
        if (lda < k) return fail("mst_eval_gemm: lda %lld < K %d", (long long)lda, k);
        if (scale) return fail("mst_eval_gemm: the affine belongs to the conv prologues");
    } else if (mode == kEvalConvRows || mode == kEvalConvSample) {
        if (batch < 1 || frames_in < 2 || channels < 1) return fail("mst_eval_gemm: conv prologue: batch %d, frames %d (>= 2), channels %d", batch, frames_in, channels);
        const int t_out = (frames_in - 2) / 2 + 1;
        if (k != 4 * channels) return fail("mst_eval_gemm: conv prologue: K %d != 4 * channels %d", k, channels);
        if ((int64_t)batch * t_out != m) return fail("mst_eval_gemm: conv prologue: M %d != batch %d * output frames %d", m, batch, t_out);
        if (ldx < channels) return fail("mst_eval_gemm: conv prologue: %lld features a frame < channels %d", (long long)ldx, channels);
        const int64_t need = mode == kEvalConvRows ? (int64_t)frames_in * ldx : ldx * frames_in;
        if (stride_batch < need) return fail("mst_eval_gemm: conv prologue: batch stride %lld < %lld", (long long)stride_batch, (long long)need);
        p.Tin = frames_in; p.Tout = t_out; p.C = channels;
    } else {
        return fail("mst_eval_gemm: mode %d is none of 0 (plain), 1 (conv over rows), 2 (conv over a sample)", mode);
    }
    hipLaunchKernelGGL(k_gemm_f32, dim3((n + EVAL_BN - 1) / EVAL_BN, (m + EVAL_BM - 1) / EVAL_BM), dim3(256), 0, (hipStream_t)stream, p);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_eval_gru(const float* xproj, const float* w_hh, const float* b_hh, const float* hidden, const int32_t* steps_dev,
                            int32_t batch, int32_t positions, int32_t width, int32_t max_steps, float* work, float* out, void* stream) {
    if (!xproj || !w_hh || !b_hh || !hidden || !steps_dev || !work || !out) return fail("mst_eval_gru: null operand");
    if (width < 64 || width % 64) return fail("mst_eval_gru: width %d is no multiple of 64", width);
    if (batch < 1 || positions < 1) return fail("mst_eval_gru: batch %d, positions %d: each at least 1", batch, positions);
    if (max_steps < 1 || max_steps > positions) return fail("mst_eval_gru: %d steps outside 1..%d positions", max_steps, positions);
    if (!eval_aligned16(w_hh) || !eval_aligned16(work) || !eval_aligned16(out)) return fail("mst_eval_gru: w_hh, work and out are read 16 bytes at a time: unaligned pointer");
    const int64_t tiles = (int64_t)(width / EVAL_GRU_UNITS) * ((batch + EVAL_GRU_CLIPS - 1) / EVAL_GRU_CLIPS);
    if (tiles > 0x7fffffff) return fail("mst_eval_gru: batch %d too large", batch);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t hn = (int64_t)batch * 2 * width;
    EvalGruArgs p{xproj, w_hh, b_hh, steps_dev, batch, positions, width};
    hipLaunchKernelGGL(k_gru_init, dim3((unsigned)((hn + 255) / 256)), dim3(256), 0, st, hidden, work, batch, width);
    HIPCHECK(hipGetLastError());
    for (int s = 0; s < max_steps; s++) {
        const float* h_in = work + (s & 1) * hn;
        float* h_out = s == max_steps - 1 ? out : work + ((s + 1) & 1) * hn;
        hipLaunchKernelGGL(k_gru_step, dim3((unsigned)tiles, 2), dim3(256), 0, st, p, h_in, h_out, s);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

extern "C" int mst_eval_layernorm(const float* x, const float* gamma, const float* beta, float* y, int32_t rows, int32_t width, float eps,
                                  int32_t leaky, void* stream) {
    if (!x || !gamma || !beta || !y) return fail("mst_eval_layernorm: null operand");
    if (rows < 1 || width < 1) return fail("mst_eval_layernorm: rows %d, width %d: each at least 1", rows, width);
    hipLaunchKernelGGL(k_ln_leaky, dim3(rows), dim3(64), 0, (hipStream_t)stream, x, gamma, beta, y, width, eps, leaky != 0);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_eval_dist_rank(const float* e1, const float* e2, int32_t n1, int32_t n2, int32_t d, float* dist, int32_t* rank, void* stream) {
    if (!e1 || !e2 || !dist) return fail("mst_eval_dist_rank: null operand");
    if (n1 < 1 || n2 < 1) return fail("mst_eval_dist_rank: %d x %d rows: each at least 1", n1, n2);
    if (d < 1 || d > EVAL_DIST_MAX_D) return fail("mst_eval_dist_rank: %d features outside 1..%d", d, EVAL_DIST_MAX_D);
    if (rank && n1 != n2) return fail("mst_eval_dist_rank: the rank of the diagonal needs a square matrix, got %d x %d", n1, n2);
    hipLaunchKernelGGL(k_dist_rank, dim3(n1), dim3(256), sizeof(float) * d, (hipStream_t)stream, e1, e2, n1, n2, d, dist, rank);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_eval_cov(const float* a, int32_t n, int32_t d, double* mean, double* cov, void* stream) {
    if (!a || !mean) return fail("mst_eval_cov: null operand");
    if (d < 1 || d > 16 * 65535) return fail("mst_eval_cov: %d features outside 1..%d", d, 16 * 65535);
    if (n < 1 || (cov && n < 2)) return fail("mst_eval_cov: %d rows: the covariance needs at least 2", n);
    hipLaunchKernelGGL(k_col_mean_f64, dim3((d + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, n, d, mean);
    HIPCHECK(hipGetLastError());
    if (cov) {
        hipLaunchKernelGGL(k_cov_f64, dim3((d + 15) / 16, (d + 15) / 16), dim3(256), 0, (hipStream_t)stream, a, mean, n, d, cov);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

extern "C" int mst_eval_pair_norms(const float* a, const float* b, const int32_t* ia, const int32_t* ib, int32_t pairs, int32_t na, int32_t nb,
                                   int32_t d, float* out, void* stream) {
    if (!a || !b || !ia || !ib || !out) return fail("mst_eval_pair_norms: null operand");
    if (pairs < 1 || na < 1 || nb < 1 || d < 1) return fail("mst_eval_pair_norms: pairs %d, rows %d / %d, features %d: each at least 1", pairs, na, nb, d);
    hipLaunchKernelGGL(k_pair_norms, dim3((pairs + 3) / 4), dim3(256), 0, (hipStream_t)stream, a, b, ia, ib, pairs, na, nb, d, out);
    HIPCHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ CLIP text tower (mst_clip.h)
// workspace of M packed rows: x f32 [M][512] | h f16 [M][512] | qkv f16 [M][1536] | att f16 [M][512] | u f16 [M][2048]
static int64_t clip_workspace_bytes(int64_t rows) { return rows * (CLIP_D * 4 + CLIP_D * 2 + 3 * CLIP_D * 2 + CLIP_D * 2 + CLIP_FF * 2); }

extern "C" int mst_clip_pack_weight(const void* src, int32_t src_is_f16, int32_t n, int32_t k, void* dst, void* stream) {
    if (!src || !dst) return fail("mst_clip_pack_weight: null operand");
    if (n < 16 || n % 16) return fail("mst_clip_pack_weight: %d output rows are no multiple of 16", n);
    if (k < 32 || k % 32) return fail("mst_clip_pack_weight: %d input columns are no multiple of 32", k);
    if (!eval_aligned16(src) || !eval_aligned16(dst)) return fail("mst_clip_pack_weight: src and dst are accessed 16 bytes at a time: unaligned pointer");
    const int64_t items = (int64_t)n * k / 8;
    const dim3 grid((unsigned)((items + 255) / 256));
    if (src_is_f16)
        hipLaunchKernelGGL(k_clip_pack<f16>, grid, dim3(256), 0, (hipStream_t)stream, (const f16*)src, (f16*)dst, n, k);
    else
        hipLaunchKernelGGL(k_clip_pack<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)src, (f16*)dst, n, k);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_clip_plan(const int32_t* lens_host, int32_t batch, int32_t context, int32_t* offsets_host, int32_t* total_rows,
                             int64_t* workspace_bytes) {
    if (!lens_host || !offsets_host || !total_rows || !workspace_bytes) return fail("mst_clip_plan: null argument");
    if (batch < 1 || batch > 65535) return fail("mst_clip_plan: batch %d outside 1..65535", batch);
    if (context < 1 || context > CLIP_CTX) return fail("mst_clip_plan: context %d outside 1..%d", context, CLIP_CTX);
    int64_t rows = 0;
    for (int b = 0; b < batch; b++) {
        if (lens_host[b] < 1 || lens_host[b] > context)
            return fail("mst_clip_plan: prompt %d has %d live rows, outside 1..%d (context)", b, lens_host[b], context);
        offsets_host[b] = (int32_t)rows;
        rows += lens_host[b];
    }
    *total_rows = (int32_t)rows;
    *workspace_bytes = clip_workspace_bytes(rows);
    return 0;
}

extern "C" int mst_clip_encode(const mst_clip_weights* w, const int32_t* ids, int32_t batch, int32_t ids_stride, const int32_t* lens,
                               const int32_t* offsets, int32_t total_rows, void* workspace, int64_t workspace_bytes, float* out, void* stream) {
    if (!w || !ids || !lens || !offsets || !workspace || !out) return fail("mst_clip_encode: null operand");
    if (w->width != CLIP_D) return fail("mst_clip_encode: width %d: only the %d-wide tower is built", w->width, CLIP_D);
    if (w->heads != CLIP_H) return fail("mst_clip_encode: heads %d: only %d heads of %d are built", w->heads, CLIP_H, CLIP_HD);
    if (w->ffn != CLIP_FF) return fail("mst_clip_encode: ffn %d: only the %d-wide FFN is built", w->ffn, CLIP_FF);
    if (w->layers < 1) return fail("mst_clip_encode: layers %d: at least 1", w->layers);
    if (w->vocab < 1) return fail("mst_clip_encode: vocab %d: at least 1", w->vocab);
    if (w->context < 1 || w->context > CLIP_CTX) return fail("mst_clip_encode: context %d outside 1..%d", w->context, CLIP_CTX);
    if (!w->tok_emb_dev || !w->pos_emb_dev || !w->lnf_g_dev || !w->lnf_b_dev || !w->proj_dev || !w->layer_host)
        return fail("mst_clip_encode: null tensor in the weight table");
    for (int l = 0; l < w->layers; l++) {
        const mst_clip_layer& y = w->layer_host[l];
        if (!y.ln1_g_dev || !y.ln1_b_dev || !y.wqkv_dev || !y.bqkv_dev || !y.wo_dev || !y.bo_dev || !y.ln2_g_dev || !y.ln2_b_dev || !y.w1_dev ||
            !y.b1_dev || !y.w2_dev || !y.b2_dev)
            return fail("mst_clip_encode: null tensor in layer %d of the weight table", l);
    }
    if (batch < 1 || batch > 65535) return fail("mst_clip_encode: batch %d outside 1..65535", batch);
    if (ids_stride < 1 || ids_stride > w->context) return fail("mst_clip_encode: %d ids a prompt outside 1..%d (context)", ids_stride, w->context);
    if (total_rows < batch || (int64_t)total_rows > (int64_t)batch * ids_stride)
        return fail("mst_clip_encode: %d packed rows outside %d..%lld (batch .. batch * ids a prompt)", total_rows, batch, (long long)batch * ids_stride);
    if (workspace_bytes < clip_workspace_bytes(total_rows))
        return fail("mst_clip_encode: workspace of %lld bytes < %lld (mst_clip_plan)", (long long)workspace_bytes, (long long)clip_workspace_bytes(total_rows));
    if (!eval_aligned16(workspace) || !eval_aligned16(w->tok_emb_dev) || !eval_aligned16(w->pos_emb_dev))
        return fail("mst_clip_encode: workspace and embeddings are accessed 16 bytes at a time: unaligned pointer");
    const hipStream_t st = (hipStream_t)stream;
    const int M = total_rows;
    char* ws = (char*)workspace;
    float* x = (float*)ws;
    f16* h = (f16*)(ws + (size_t)M * CLIP_D * 4);
    f16* qkv = h + (size_t)M * CLIP_D;
    f16* att = qkv + (size_t)M * 3 * CLIP_D;
    f16* u = att + (size_t)M * CLIP_D;
    const unsigned mt = (unsigned)((M + CLIP_BM - 1) / CLIP_BM);

    ClipEmbedArgs ea{ids, lens, offsets, (const f16*)w->tok_emb_dev, (const f16*)w->pos_emb_dev, w->layer_host[0].ln1_g_dev,
                     w->layer_host[0].ln1_b_dev, x, h, ids_stride, w->vocab, w->context, M};
    hipLaunchKernelGGL(k_clip_embed, dim3(batch), dim3(256), 0, st, ea);
    HIPCHECK(hipGetLastError());
    for (int l = 0; l < w->layers; l++) {
        const mst_clip_layer& y = w->layer_host[l];
        const bool last = l == w->layers - 1;
        ClipGemmArgs g{};
        g.M = M;
        g.a = h; g.w = (const f16*)y.wqkv_dev; g.bias = y.bqkv_dev; g.out = qkv; g.N = 3 * CLIP_D; g.K = CLIP_D;
        hipLaunchKernelGGL(k_clip_gemm<kClipStore>, dim3(mt, 3 * CLIP_D / CLIP_BN), dim3(512), 0, st, g);
        HIPCHECK(hipGetLastError());
        ClipAttnArgs aa{qkv, lens, offsets, att, M};
        hipLaunchKernelGGL(k_clip_attn, dim3(CLIP_H, batch), dim3(256), 0, st, aa);
        HIPCHECK(hipGetLastError());
        g.a = att; g.w = (const f16*)y.wo_dev; g.bias = y.bo_dev; g.x = x; g.g = y.ln2_g_dev; g.b = y.ln2_b_dev; g.out = h; g.N = CLIP_D; g.K = CLIP_D;
        hipLaunchKernelGGL(k_clip_gemm<kClipResid>, dim3(mt, 1), dim3(512), 0, st, g);
        HIPCHECK(hipGetLastError());
        g.a = h; g.w = (const f16*)y.w1_dev; g.bias = y.b1_dev; g.x = nullptr; g.g = nullptr; g.b = nullptr; g.out = u; g.N = CLIP_FF; g.K = CLIP_D;
        hipLaunchKernelGGL(k_clip_gemm<kClipGelu>, dim3(mt, CLIP_FF / CLIP_BN), dim3(512), 0, st, g);
        HIPCHECK(hipGetLastError());
        g.a = u; g.w = (const f16*)y.w2_dev; g.bias = y.b2_dev; g.x = x; g.out = h; g.N = CLIP_D; g.K = CLIP_FF;
        g.g = last ? nullptr : w->layer_host[l + 1].ln1_g_dev;
        g.b = last ? nullptr : w->layer_host[l + 1].ln1_b_dev;
        hipLaunchKernelGGL(k_clip_gemm<kClipResid>, dim3(mt, 1), dim3(512), 0, st, g);
        HIPCHECK(hipGetLastError());
    }
    ClipFinalArgs fa{x, lens, offsets, w->lnf_g_dev, w->lnf_b_dev, (const f16*)w->proj_dev, out, M};
    hipLaunchKernelGGL(k_clip_final, dim3(batch), dim3(512), 0, st, fa);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int mst_set_precise(mst_engine* e, int32_t on) {
    if (!e) return fail("mst_set_precise: null engine");
    e->precise = on != 0;
    // 2 = switched on, but weights uploaded so far lack their lo halves: the caller uploads them again (DenoiserEngine.set_precise does)
    return (e->precise && !e->lo_missing.empty()) ? 2 : 0;
}

// ------------------------------------------------------------------------------------------ debug ABI
extern "C" int mst_set_trunk_groups(mst_engine* e, int32_t on) {
    if (!e) return fail("mst_set_trunk_groups: null engine");
    e->trunk_groups = on != 0;
    if (e->trunk_err[0]) {                   // after a give-up: the counters hold whatever the abandoned launch left -- start clean
        ON_DEVICE(e->cfg.device);
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemset(e->trunk_cnt, 0, (size_t)e->cfg.max_rows * 32 * sizeof(unsigned)));
        e->trunk_err[0] = 0;
    }
    return 0;
}
extern "C" int mst_debug_stop_after(mst_engine* e, int32_t layer, int32_t stage) {
    if (!e) return fail("mst_debug_stop_after: null engine");
    e->dbg_layer = layer;
    e->dbg_stage = stage;
    return 0;
}

extern "C" int mst_debug_copy(mst_engine* e, const char* which, void* dst_dev, uint64_t nbytes, void* stream) {
    if (!e || !which || !dst_dev) return fail("mst_debug_copy: null argument");
    std::string w(which);
    const void* src = nullptr;
    size_t cap = 0;
    if (w == "hs") {           // the stream as float32: joined from its f16 hi/lo halves on the fly
        const size_t n = nbytes / 4;
        if (nbytes > (size_t)e->M_pad * MST_D * 4) return fail("mst_debug_copy: hs holds %zu bytes", (size_t)e->M_pad * MST_D * 4);
        hipLaunchKernelGGL(k_join_stream, dim3(1024), dim3(256), 0, (hipStream_t)stream, e->hx, e->hl, (float*)dst_dev, n);
        HIPCHECK(hipGetLastError());
        return 0;
    }
    if (w == "hx") { src = e->hx; cap = (size_t)e->M_pad * MST_D * 2; }
    else if (w == "qkv") { src = e->qkv; cap = (size_t)e->M_pad * 3 * MST_D * 2; }
    else if (w == "att") { src = e->att; cap = (size_t)e->M_pad * MST_D * 2; }
    else if (w == "hid") { src = e->hid; cap = (size_t)e->M_pad * MST_FF * 2; }
    else if (w == "temb") { src = e->temb; cap = (size_t)e->temb_cap * MST_D * 4; }
    else if (w == "textproj") { src = e->textproj; cap = (size_t)e->cfg.max_rows * MST_D * 4; }
    else return fail("mst_debug_copy: unknown buffer '%s'", which);
    if (nbytes > cap) return fail("mst_debug_copy: %llu bytes requested, buffer holds %zu", (unsigned long long)nbytes, cap);
    HIPCHECK(hipMemcpyAsync(dst_dev, src, nbytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
