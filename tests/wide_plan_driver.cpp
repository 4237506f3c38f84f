// Driver of the wide path's planner (okge_plan.h: make_wide_shape, plan_wide, wide_train_layout, wide_score_layout) for
// tests/test_wide_plan.py.  Plain C++17, no HIP: one line "B N d gt_mbytes" (gt_mbytes < 0: the default) per case on stdin, one
// JSON object per case on stdout.
#include <cstdio>

#include "../open_knowledge_graph_embeddings_amd/csrc/okge_plan.h"

using namespace okge;

int main()
{
    int B, N, d, gt;
    while (std::scanf("%d %d %d %d", &B, &N, &d, &gt) == 4) {
        Knobs k;
        if (gt >= 0) { k.gt_mbytes.set = true; k.gt_mbytes.v = gt; }
        WideShape s;
        if (!make_wide_shape(B, N, d, s)) {
            std::printf("{\"ok\": 0, \"is_wide\": %d}\n", is_wide(d) ? 1 : 0);
            continue;
        }
        const WidePlan p = plan_wide(s, k);
        const WideTrainLayout l = wide_train_layout(s, p);
        const WideScoreLayout sc = wide_score_layout(s);
        std::printf("{\"ok\": 1, \"is_wide\": 1, \"Bpad\": %d, \"ldq\": %d, \"tiles\": %d, \"row_blocks\": %d, \"tile_n\": %d, "
                    "\"range_tiles\": %d, \"n_ranges\": %d, \"range_n\": %d, \"ldg\": %d, \"dq_splits\": %d, \"dq_k_per\": %d, "
                    "\"n_loss_partials\": %d, \"tile_bytes\": %zu, "
                    "\"regions\": [[%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu], "
                    "[%zu, %zu], [%zu, %zu], [%zu, %zu]], "
                    "\"score_bytes\": %zu, \"lse_bytes\": %zu, \"total\": %zu, \"score_total\": %zu, \"score_off_Q\": %zu}\n",
                    s.Bpad, s.ldq, s.tiles, s.row_blocks, WIDE_TN, p.range_tiles, p.n_ranges, p.range_n, p.ldg, p.dq_splits, p.dq_k_per,
                    p.n_loss_partials, p.tile_bytes,
                    l.off_Q, (size_t)s.Bpad * s.ldq * 4, l.off_tptr, (size_t)(s.tiles + 1) * 4, l.off_stats, (size_t)p.range_tiles * s.Bpad * 8,
                    l.off_lse, (size_t)s.Bpad * 4, l.off_ysum, (size_t)s.Bpad * 4, l.off_run, (size_t)s.Bpad * 8,
                    l.off_loss, (size_t)p.n_loss_partials * 8, l.off_G, (size_t)s.Bpad * p.ldg * 4, l.off_Cm, (size_t)p.range_n * s.ldq * 4,
                    l.off_dC, (size_t)p.range_n * s.ldq * 4, l.off_dQ, (size_t)s.Bpad * s.ldq * 4,
                    l.off_slab, (size_t)p.dq_splits * s.Bpad * s.ldq * 4,
                    l.score_bytes, l.lse_bytes, l.total, sc.total, sc.off_Q);
    }
    return 0;
}
