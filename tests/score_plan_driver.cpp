// score_plan_driver - the plan of a scoring launch (juicer_amd/csrc/jd_score_plan.h) under plain g++, for tests/test_score_plan_cpu.py.
// stdin: one launch per line
//   D n_gmm hybrid mlp fast n_rows max_blocks used_row_tiles has_list n_rt_list
// stdout, per line:
//   verdict kernel grid lds_bytes list_tile_rows large_kernel large_lds_bytes tile_rows tile_states row_tiles tiles dp
// (list_tile_rows: score_plan_tile_rows, what check_score_rows asks; large_*: score_plan_large, what gmm_tiles128_occupancy asks)
#include <cstdio>

#include "jd_score_plan.h"

int main()
{
    int D, G, hybrid, mlp, fast, n_rows, max_blocks, used_row_tiles, has_list, n_rt_list;
    while (scanf("%d %d %d %d %d %d %d %d %d %d", &D, &G, &hybrid, &mlp, &fast, &n_rows, &max_blocks, &used_row_tiles, &has_list, &n_rt_list) == 10) {
        const ScorePlan p = score_plan(ScorePlanIn{D, G, hybrid != 0, mlp != 0, fast != 0, n_rows, max_blocks, used_row_tiles, has_list != 0, n_rt_list});
        const ScoreLarge large = score_plan_large(D, hybrid != 0, mlp != 0, fast != 0);
        printf("%d %d %u %zu %d %d %zu %d %d %lld %lld %d\n", (int)p.verdict, p.kernel, p.grid, p.lds_bytes,
               score_plan_tile_rows(D, hybrid != 0, mlp != 0, fast != 0), large.kernel, large.lds_bytes, p.tile_rows, p.tile_states, p.row_tiles, p.tiles,
               p.dp);
    }
    return 0;
}
