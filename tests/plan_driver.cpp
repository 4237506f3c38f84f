// Driver of tests/test_launch_plan.py: the planner (okge_plan.h) on the CPU, no HIP header anywhere.
// stdin, one case per line:  B N d cus k range_n n_groups n_filter TAIL_SPLIT GT_MBYTES B_SPLIT STREAMK DQ_SPLIT   ("-": knob unset)
// stdout, one JSON object per case: every field of every plan and layout.
#include <cstdio>
#include <cstring>

#include "../open_knowledge_graph_embeddings_amd/csrc/okge_plan.h"

using namespace okge;

static Knob knob(const char *tok)
{
    Knob k;
    if (std::strcmp(tok, "-") != 0) { k.set = true; k.v = std::atoi(tok); }
    return k;
}

#define I(x, f) std::printf("\"%s\":%lld,", #f, (long long)(x).f)

static void sweep(const char *name, const SweepPlan &p)
{
    std::printf("\"%s\":{", name);
    I(p, tiles); I(p, main_tiles); I(p, tail_tiles); I(p, tail_split); I(p, tail_b_per_block);
    std::printf("\"sk_wgs\":%d},", p.sk_wgs);
}

int main()
{
    long long B, N, d, cus, k, range_n, n_groups, n_filter;
    char kn[5][32];
    while (std::scanf("%lld %lld %lld %lld %lld %lld %lld %lld %31s %31s %31s %31s %31s", &B, &N, &d, &cus, &k, &range_n, &n_groups,
                      &n_filter, kn[0], kn[1], kn[2], kn[3], kn[4]) == 13) {
        Knobs kb;
        kb.tail_split = knob(kn[0]); kb.gt_mbytes = knob(kn[1]); kb.b_split = knob(kn[2]); kb.streamk = knob(kn[3]); kb.dq_split = knob(kn[4]);
        Shape s;
        if (!make_shape((int)B, (int)N, (int)d, s)) { std::printf("{\"ok\":0}\n"); continue; }
        std::printf("{\"ok\":1,");
        I(s, B); I(s, N); I(s, d); I(s, Bpad); I(s, KB); I(s, D16); I(s, LDK); I(s, ldq); I(s, tiles);
        std::printf("\"score_total\":%zu,", score_layout(s).total);
        const TrainPlan p = plan_train(s, (int)cus, kb);
        I(p, range_tiles); I(p, n_ranges); I(p, range_n); I(p, ldg); I(p, b_split); I(p, b_per_block);
        I(p, sk_wgs); I(p, sk_chunks); I(p, tail_tiles); I(p, tail_split); I(p, tail_b_per_block); I(p, nsplit);
        I(p, n_loss_partials); I(p, dc_slabs); I(p, dc_slab_rows);
        const Ranges rg = plan_ranges(s, (int)cus, kb);
        std::printf("\"lse_ranges\":[%d,%d,%d],", rg.range_tiles, rg.n_ranges, rg.range_n);
        I(lse_layout(s, rg), lse_bytes);
        const TrainLayout l = train_layout(s, p);
        I(l, off_Q); I(l, off_tptr); I(l, off_stats); I(l, off_lse); I(l, off_ysum); I(l, off_run); I(l, score_bytes); I(l, lse_bytes);
        I(l, off_loss); I(l, off_GT); I(l, off_Cm); I(l, off_slab); I(l, off_dcs); I(l, off_Qp); I(l, loss_bytes); I(l, dcs_bytes); I(l, total);
        const RowGradsLayout rl = row_grads_layout(s, l.total);
        std::printf("\"rows\":[%zu,%zu,%zu,%zu],", rl.off_EV, rl.off_RV, rl.off_ids, rl.total);
        sweep("sweep", plan_sweep(s, s.tiles, (int)cus, kb));                                       // a sweep of the whole call
        sweep("sweep_last", plan_sweep(s, s.tiles - (p.n_ranges - 1) * p.range_tiles, (int)cus, kb));   // ... of the last train range
        TopkPlan tp;
        if (plan_topk(s, (int)k, (int)range_n, (int)cus, tp))
            std::printf("\"topk\":[%d,%d,%d,%zu,%zu,%zu,%zu],", tp.range_tiles, tp.n_ranges, tp.range_n, tp.off_Q,
                        tp.off_part, tp.off_X, tp.total);
        else
            std::printf("\"topk\":null,");
        EvalLayout e;
        if (eval_layout(s, n_groups, n_filter, e))
            std::printf("\"eval\":[%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%d]", e.off_Q, e.off_true, e.off_filt, e.off_rps, e.off_gshift, e.off_grow,
                        e.off_counts, e.total, (int)e.slab);
        else
            std::printf("\"eval\":null");
        std::printf("}\n");
    }
    return 0;
}
