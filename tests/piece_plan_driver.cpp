// piece_plan_driver.cpp - runs plan_piece_rows and plan_resident_scoring_wgs (juicer_amd/csrc/jd_plan.h) over cases read from stdin, for
// tests/test_piece_plan_cpu.py.  Input: the number of cases, then per case a letter and four integers:
//   p n_state_groups resident_scoring_wgs lo hi   ->  rows of a piece
//   w n_cus n_slots occ_slot occ_gmm              ->  scoring workgroups resident beside the slots
#include <cstdio>

#include "jd_plan.h"

int main()
{
    long long n_cases = 0;
    if (scanf("%lld", &n_cases) != 1) return 2;
    for (long long c = 0; c < n_cases; ++c) {
        char what = 0;
        int v[4];
        if (scanf(" %c %d %d %d %d", &what, &v[0], &v[1], &v[2], &v[3]) != 5) return 2;
        if (what == 'p') printf("%d\n", plan_piece_rows(v[0], v[1], v[2], v[3]));
        else if (what == 'w') printf("%d\n", plan_resident_scoring_wgs(v[0], v[1], v[2], v[3]));
        else return 2;
    }
    return 0;
}
