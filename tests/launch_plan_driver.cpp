// Driver of tests/test_launch_plan_cpu.py: evaluates csrc/mst_plan.h -- the only project header it includes -- on the cases it reads.
//   argv: ntb1_m ntb2_from.   stdin, one case per line: the 13 PlanKnobs words in the struct's order, then rows and T.
//   stdout, one line per case: plan_trunk's eight fields for (slices, instrumented) = (1, 0), (1, 1), (3, 0), (3, 1); rows_ntb of the
//   launch's token rows; then for cfg = 0, 1 with `rows` as the batch: plan_slices' count n and slice_of(batch, n, i) for i < n.
//   argv: "embed".   stdin, one case per line: feats and T.
//   stdout, one line per case: plan_embed_in's three fields for (precise, embed_fast) = (0, 0), (0, 1), (1, 0), (1, 1); then
//   embed_next_ksn and plan_embed_out's seven fields for every (cfg, precise, embed_fast, mode 0..6, hi_lo, custom_w), the last fastest.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mst_plan.h"

static int embed_cases() {
    int feats, T;
    while (scanf("%d %d", &feats, &T) == 2) {
        for (int precise = 0; precise < 2; precise++)
            for (int fast = 0; fast < 2; fast++) {
                const mst::EmbedInPlan p = mst::plan_embed_in(feats, precise, fast);
                printf("%d %d %d ", p.kin_pad, p.ks, p.kernel);
            }
        for (int cfg = 0; cfg < 2; cfg++)
            for (int precise = 0; precise < 2; precise++)
                for (int fast = 0; fast < 2; fast++) {
                    printf("%d ", mst::embed_next_ksn(feats, T, precise, fast));
                    for (int mode = 0; mode < 7; mode++)
                        for (int hi_lo = 0; hi_lo < 2; hi_lo++)
                            for (int custom = 0; custom < 2; custom++) {
                                const mst::EmbedOutPlan p = mst::plan_embed_out(feats, T, cfg, precise, fast, mode, hi_lo, custom);
                                printf("%d %d %d %d %d %d %d ", p.kernel, p.nbw, p.nx, p.staged, p.ksn, p.ring_bf, p.ring_xs);
                            }
                }
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "embed")) return embed_cases();
    if (argc != 3) return 2;
    const int ntb1_m = atoi(argv[1]), ntb2_from = atoi(argv[2]);
    int w[mst::PLAN_KNOB_WORDS], rows, T;
    for (;;) {
        for (int& v : w)
            if (scanf("%d", &v) != 1) return 0;
        if (scanf("%d %d", &rows, &T) != 2) return 3;
        static_assert(mst::PLAN_KNOB_WORDS == 13, "the case format lists 13 knobs");
        const mst::PlanKnobs k{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12]};
        for (int slices = 1; slices <= 3; slices += 2)
            for (int ins = 0; ins < 2; ins++) {
                const mst::TrunkPlan p = mst::plan_trunk(k, rows, T, slices, ins);
                printf("%d %d %d %d %d %d %d %d ", p.path, p.precise, p.lnf, p.qkv_attn, p.fuse_tail, p.ln128, p.tail_ntb, p.nt16);
            }
        printf("%d", mst::rows_ntb(rows * (T + 1), ntb1_m, ntb2_from));
        for (int cfg = 0; cfg < 2; cfg++) {
            const int n = mst::plan_slices(k, rows, cfg, T);
            printf(" %d", n);
            for (int i = 0; i < n; i++) printf(" %d %d", mst::slice_of(rows, n, i).first, mst::slice_of(rows, n, i).clips);
        }
        printf("\n");
    }
}
