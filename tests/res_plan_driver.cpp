// res_plan_driver.cpp - runs plan_resident (juicer_amd/csrc/jd_plan.h) over cases read from stdin, for tests/test_res_plan_cpu.py.
// Input: the number of cases, then per case
//   n_cus n_streams rows_per_buf max_cw cap_slots cap_items pipeline free_cus slot xl keep_se SW WG_PER_CU SLOT_WG_PER_CU GMM_ROWS2 RES_RING_W
// (free_cus .. keep_se: the development knobs, -1 unset).  Output, one line per case:  verdict rows Cw slot xl park_cus park_fill
#include <cstdio>

#include "jd_plan.h"

static bool rd(long long *v) { return scanf("%lld", v) == 1; }

int main()
{
    long long n_cases = 0;
    if (!rd(&n_cases)) return 2;
    for (long long c = 0; c < n_cases; ++c) {
        long long v[16];
        for (long long &x : v) if (!rd(&x)) return 2;
        ResPlanIn in;
        in.n_cus = (int)v[0]; in.n_streams = (int)v[1]; in.rows_per_buf = (int)v[2]; in.max_cw = (int)v[3];
        in.cap_slots = v[4]; in.cap_items = v[5]; in.pipeline = v[6] != 0;
        in.free_cus = (int)v[7]; in.slot = (int)v[8]; in.xl = (int)v[9]; in.keep_se = (int)v[10];
        in.sw = (int)v[11]; in.wg_per_cu = (int)v[12]; in.slot_wg_per_cu = (int)v[13]; in.gmm_rows2 = (int)v[14]; in.res_ring_w = (int)v[15];
        if (in.n_cus < 1 || in.n_streams < 1 || in.rows_per_buf < 1) return 2;
        const ResPlanOut out = plan_resident(in);
        printf("%d %d %d %d %d %d %d\n", (int)out.verdict, out.rows, out.Cw, out.slot ? 1 : 0, out.xl ? 1 : 0, out.park_cus, out.park_fill);
    }
    return 0;
}
