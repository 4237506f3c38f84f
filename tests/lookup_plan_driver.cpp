// Driver of the lookup variants' workspace layout (okge_plan.h: lookup_layout) for tests/test_lookup_variants_plan.py.  Plain
// C++17, no HIP: one line "entity_rows relation_rows d training" per case on stdin, one JSON object per case on stdout; the
// region sizes are written from the shape here, not read back from the layout.
#include <cstdio>

#include "../open_knowledge_graph_embeddings_amd/csrc/okge_plan.h"

using namespace okge;

int main()
{
    long long re, rr;
    int d, training;
    while (std::scanf("%lld %lld %d %d", &re, &rr, &d, &training) == 4) {
        LookupLayout l;
        if (!lookup_layout(re, rr, d, training != 0, l)) {
            std::printf("{\"ok\": 0}\n");
            continue;
        }
        const size_t rows = (size_t)(re + rr), D = (size_t)d;
        std::printf("{\"ok\": 1, \"max_chunks\": %d, \"chunk\": %d, \"max_calls\": %d, \"total\": %zu, \"regions\": [[%zu, %zu], [%zu, %zu], "
                    "[%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu]",
                    l.max_chunks, LOOKUP_BN_CHUNK, LOOKUP_MAX_CALLS, l.total, l.off_X, rows * D * 4, l.off_saved,
                    (size_t)LOOKUP_MAX_CALLS * 4 * D * 4, l.off_stat, (size_t)LOOKUP_MAX_CALLS * 2 * D * 8, l.off_part, (size_t)l.max_chunks * 2 * D * 8, l.off_norm, rows * 8, l.off_Wt,
                    2 * D * D * 4, l.off_P, (size_t)re * D * 4);
        if (training)
            std::printf(", [%zu, %zu], [%zu, %zu], [%zu, %zu], [%zu, %zu]", l.off_G1, rows * D * 4, l.off_G2, (size_t)re * D * 4, l.off_slab,
                        (size_t)2 * LOOKUP_MAX_SPLITS * D * D * 4, l.off_Xbn, (size_t)re * D * 4);
        std::printf("]}\n");
    }
    return 0;
}
