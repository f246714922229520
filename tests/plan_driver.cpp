// plan_driver.cpp - runs plan_clusters (juicer_amd/csrc/jd_plan.h) over cases read from stdin, for tests/test_plan_cpu.py.
// Every number is an integer; real-valued inputs come in thousandths ("_m").  Input: the number of cases, then per case
//   n_work has_weight n_bg nwg_all max_cw fg_cw_cap bg_cw_cap bg_weight_m weighted plan_mode plan_min_cw a_m b_m a2_m b2_m load_scale_m
//   gmm_ms_per_wg_m xl_ok xl_slack_m rebalance bg_rebalance rebalance_frac_m rebalance_min_us_m weight_m[n_work] bg_left_m[n_bg]
// Output, one line per case:  weighted xl grid Cw n_slots rebalance_at n_items {idx first cw fg}*   (n_slots as launch_search
// passes it to the kernel: 0 for a weighted plan)
#include <cstdio>
#include <vector>

#include "jd_plan.h"

static bool rd(long long *v) { return scanf("%lld", v) == 1; }

int main()
{
    long long n_cases = 0;
    if (!rd(&n_cases)) return 2;
    for (long long c = 0; c < n_cases; ++c) {
        long long v[23];
        for (long long &x : v) if (!rd(&x)) return 2;
        PlanIn in;
        in.n_work = (int)v[0]; in.n_bg = (int)v[2]; in.nwg_all = (int)v[3]; in.max_cw = (int)v[4];
        in.fg_cw_cap = (int)v[5]; in.bg_cw_cap = (int)v[6]; in.bg_weight = v[7] / 1000.0;
        in.weighted = v[8] != 0; in.plan_mode = (int)v[9]; in.plan_min_cw = (int)v[10];
        in.a_us = v[11] / 1000.0; in.b_us = v[12] / 1000.0; in.a2_us = v[13] / 1000.0; in.b2_us = v[14] / 1000.0;
        in.load_scale = v[15] / 1000.0;
        // (as launch_search prices the scoring beside a launch: per workgroup the running batch may use)
        in.gmm_cu_us = v[16] > 0 ? v[16] / 1000.0 * 1e3 * (in.nwg_all - in.n_bg) : 0.0;
        in.xl_ok = v[17] != 0; in.xl_slack = v[18] / 1000.0;
        in.rebalance = v[19] != 0; in.bg_rebalance = v[20] != 0; in.rebalance_frac = v[21] / 1000.0; in.rebalance_min_us = v[22] / 1000.0;
        if (in.n_work < 1 || in.n_bg < 0) return 2;
        std::vector<double> weight((size_t)in.n_work), bg_left((size_t)in.n_bg);
        long long x = 0;
        for (double &w : weight) { if (!rd(&x)) return 2; w = x / 1000.0; }
        for (double &w : bg_left) { if (!rd(&x)) return 2; w = x / 1000.0; }
        in.weight = v[1] ? weight.data() : nullptr;
        in.bg_left = bg_left.data();
        const PlanOut out = plan_clusters(in);
        printf("%d %d %d %d %d %d %d", out.weighted ? 1 : 0, out.xl ? 1 : 0, out.grid, out.Cw, out.weighted ? 0 : out.n_slots, out.rebalance_at,
               (int)out.items.size());
        for (const PlanItem &p : out.items) printf(" %d %d %d %d", p.idx, p.first, p.cw, p.fg ? 1 : 0);
        printf("\n");
    }
    return 0;
}
