// Several fine-tuned styles in one batch (StyleBank): the encoder stack's weights are chosen per clip.
//
// Two styles differ only in the 96 tensors of the encoder stack (the prior's projections, timestep MLP, text projection and positional
// table are shared), so only the stack's launches need to know a clip's style.  Every (slot, layer) has one StyleLayer record in device
// memory; a workgroup reads its record with scalar loads when it starts (the resident trunk's TrunkLayer is the precedent) and then runs
// the SAME body as the single-style kernel.  The single-style kernels are untouched: these are separate __global__ wrappers.
//
//   k_qkv_attention2_style  one workgroup per (clip, head), as k_qkv_attention2: a clip never spans two styles.  The clip's slot comes
//                           from a per-row table; a clip order table places the clips on XCDs (identity = plain order).
//   k_layer_tail_seg        one workgroup per SEGMENT: a maximal run of one slot's rows inside one tile.  The tile is computed whole with
//                           the segment's weights and only the rows [row_lo, row_hi) are stored.
//   k_rows_gemm_seg         the same segment scheme for the small-launch GEMMs (and their LayerNorm prologue).
//   k_ln_rows_style         one wave per row, the row's slot looked up through its clip.
//
// Why a tile that straddles two styles may run twice, both runs updating the stream IN PLACE (k_layer_tail reads its residual rows from
// hx / hl and writes the result over them): every stage of the tail is row-independent.  The MFMA products are per token row (a row of
// the result depends on that row of the operand only); LayerNorm1 and LayerNorm2 reduce over the 512 features of ONE row, and their
// statistics are exchanged between the lanes / waves that hold pieces of that same row only; GELU is elementwise.  So a run computes its
// own segment's rows from those rows' inputs alone, whatever the other run has meanwhile written over the OTHER rows of the tile, and it
// stores nothing else.  The only global stores of the inference tail are the LayerNorm2 rows (indexed by token row, guarded by the
// segment bounds); nothing is written per tile.  The vmcnt accounting does not change: the guard is wave-uniform, exactly like the
// existing `tok < M` guard of the last tile.  k_rows_gemm_seg writes another buffer than it reads, so there the argument is not even
// needed.
#pragma once
#include "mst_attn.h"
#include "mst_elem.h"
#include "mst_small.h"
#include "mst_tail.h"

namespace mst {

// one (slot, layer): the tensors sampling reads (no transposed training copies, no precise-mode lo halves)
struct StyleLayer {
    const f16* wqkv; const float* b_in;                               // fused QKV + attention
    const f16* wtail; const float *b_out, *g1, *be1, *b1, *b2, *g2, *be2;  // fused layer tail (and the LayerNorm vectors of the small path)
    const f16 *wsm_in, *wsm_out, *wsm_1, *wsm_2;                      // small-launch GEMM fragments
};
// a run of one slot's rows inside one tile: the tile starts at row0, rows [row_lo, row_hi) are this workgroup's to store
struct StyleSeg { int row0, row_lo, row_hi, slot; };

typedef const StyleLayer __attribute__((address_space(4)))* StyleTab;
typedef const StyleSeg __attribute__((address_space(4)))* SegTab;
typedef const int __attribute__((address_space(4)))* IntTab;

template <int NT16>
__global__ __launch_bounds__(512) void k_qkv_attention2_style(const f16* __restrict__ hx, const StyleLayer* __restrict__ lay, int nl,
                                                              const int* __restrict__ row_slot, const int* __restrict__ order,
                                                              f16* __restrict__ out, int S) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nclip = gridDim.x / MST_H, full = (nclip / 8) * 8 * MST_H;
    int pos, head;
    if ((int)blockIdx.x < full) {
        const int grp = blockIdx.x >> 5, within = blockIdx.x & 31;
        pos = grp * 8 + (within & 7);
        head = within >> 3;
    } else {
        const int r = blockIdx.x - full;
        pos = (nclip / 8) * 8 + r / MST_H;
        head = r % MST_H;
    }
    const int clip = ((IntTab)(unsigned long long)order)[pos];
    const StyleTab rec = (StyleTab)(unsigned long long)lay + ((IntTab)(unsigned long long)row_slot)[clip] * nl;
    qa2_body<NT16, false>(smem, hx, rec->wqkv, rec->b_in, out, S, clip, head, GroupSync{nullptr, 0u, nullptr}, false, 0);
}

template <int NTB>
__global__ __launch_bounds__(512) void k_layer_tail_seg(const f16* __restrict__ att, const StyleLayer* __restrict__ lay, int nl,
                                                        const StyleSeg* __restrict__ segs, f16* __restrict__ hx, f16* __restrict__ hl,
                                                        const float* __restrict__ gelu_tab) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SegTab sg = (SegTab)(unsigned long long)segs + blockIdx.x;
    const int row0 = sg->row0, lo = sg->row_lo, hi = sg->row_hi;
    const StyleTab w = (StyleTab)(unsigned long long)lay + sg->slot * nl;
    tail_body<NTB, false, false, true>(smem, att, w->wtail, w->b_out, w->g1, w->be1, w->b1, w->b2, w->g2, w->be2, hx, hl, gelu_tab, hi, row0,
                                       GroupSync{nullptr, 0u, nullptr}, 0, TailTrain{}, lo);
}

// MODE 0: QKV (its LayerNorm prologue is the PREVIOUS layer's LayerNorm2: lay_prev); MODE 1: FFN1 (prologue: this layer's LayerNorm1);
// MODE 2, KS 16: out-projection; MODE 2, KS 32: FFN2.  ln carries the buffers only; its vectors come from the segment's slot.
template <int KS, int MODE, int LNF, int NTB>
__global__ __launch_bounds__(512) void k_rows_gemm_seg(const f16* __restrict__ X, const StyleLayer* __restrict__ lay, const StyleLayer* __restrict__ lay_prev,
                                                       int nl, const StyleSeg* __restrict__ segs, void* __restrict__ out, int ldo, LnRows ln) {
    const SegTab sg = (SegTab)(unsigned long long)segs + blockIdx.x;
    const int row0 = sg->row0, lo = sg->row_lo, hi = sg->row_hi, slot = sg->slot;
    const StyleTab w = (StyleTab)(unsigned long long)lay + slot * nl;
    const f16* wpk = MODE == 0 ? w->wsm_in : MODE == 1 ? w->wsm_1 : KS == 16 ? w->wsm_out : w->wsm_2;
    const float* bias = MODE == 0 ? w->b_in : MODE == 1 ? w->b1 : nullptr;
    if constexpr (LNF) {
        const StyleTab p = MODE == 0 ? (StyleTab)(unsigned long long)lay_prev + slot * nl : w;
        if constexpr (MODE == 0) { ln.bias = p->b2; ln.gamma = p->g2; ln.beta = p->be2; }
        else { ln.bias = p->b_out; ln.gamma = p->g1; ln.beta = p->be1; }
    }
    rows_gemm_body<KS, MODE, LNF, NTB, true>(X, wpk, bias, out, ldo, hi, ln, FfnTrain{}, row0, lo);
}

// which = 0: LayerNorm1 (b_out, g1, be1), 1: LayerNorm2 (b2, g2, be2) of the row's slot; token row -> transformer row = row / S
__global__ __launch_bounds__(256) void k_ln_rows_style(const float* __restrict__ acc, const StyleLayer* __restrict__ lay, int nl, int which,
                                                       const int* __restrict__ row_slot, int S, f16* hi, f16* lo, int M, f16* ohi, f16* olo) {
    if (!ohi) { ohi = hi; olo = lo; }
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= M) return;
    const StyleTab w = (StyleTab)(unsigned long long)lay + ((IntTab)(unsigned long long)row_slot)[row / S] * nl;
    if (which == 0) ln_rows_body(acc, w->b_out, w->g1, w->be1, hi, lo, ohi, olo, row);
    else ln_rows_body(acc, w->b2, w->g2, w->be2, hi, lo, ohi, olo, row);
}

}  // namespace mst
