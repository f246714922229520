// jd_plan.h - which stream of a search launch runs on which workgroups, as a function of plain data (no HIP, no decoder: compiled and
// tested on the CPU, tests/test_plan_cpu.py): given the frames every stream has ahead and the workgroups the chip offers, the size and
// the first workgroup of every stream's cluster - uniform clusters, or the weighted plan (clusters sized so that the streams finish
// together), the batch behind the running one beside it, its XCD-local packing, and when to cut the launch short for a new plan.
// launch_search (jd_host_launch.h) turns the result into the kernel's work list.
// At the end, plan_resident: the geometry of the search kernels that stay on the device (jd_host_resident.h: jd_res_start;
// tests/test_res_plan_cpu.py).
#pragma once

#include <algorithm>
#include <numeric>
#include <queue>
#include <utility>
#include <vector>

struct PlanIn {
    const double *weight;                 // per stream of the running batch: the frames it has in this launch (null: none - uniform clusters)
    int n_work;                           // streams of the running batch (>= 1)
    const double *bg_left; int n_bg;      // streams of the batch behind: the frames each has ahead
    int nwg_all;                          // workgroups of the launch (what the scoring reserve leaves)
    int max_cw;                           // largest cluster the arenas and JD_CW allow
    int fg_cw_cap, bg_cw_cap;             // two batches in flight: largest cluster of the running batch / of the batch behind
    double bg_weight;                     // ... and the part of bg_left the plan counts
    bool weighted;                        // JD_WEIGHTED
    int plan_mode, plan_min_cw;           // JD_PLAN, JD_PLAN_MIN_CW
    double a_us, b_us, a2_us, b2_us;      // the cost model of plan_mode 0 / of plan_mode 1
    double load_scale;                    // ... whose b scales with the decoder's load
    double gmm_cu_us;                     // plan_mode 1: CU-time of the scoring beside the launch (0: none)
    bool xl_ok; double xl_slack;          // XCD-local launches allowed / by how much the packed plan may end later
    bool rebalance, bg_rebalance;         // re-planning under way: on at all / with the batch behind beside it
    double rebalance_frac, rebalance_min_us;
};

struct PlanItem {
    int idx;                              // which stream: < n_work the running batch's, else n_work + that of the batch behind
    int first, cw;                        // its cluster: first workgroup and size
    bool fg;                              // the launch is there for it (the running batch)
};

struct PlanOut {
    std::vector<PlanItem> items;          // in launch order
    int grid = 0;                         // workgroups to launch
    int Cw = 1, n_slots = 1;              // the uniform clusters' size and how many of them the grid holds
    int rebalance_at = 0;                 // SearchArgs::rebalance_at
    bool xl = false;                      // every cluster inside one eighth of the grid: the XCD-local kernel
    bool weighted = false;                // the weighted plan was made (items may hold streams of the batch behind)
};

// A stream's frame costs about  a + b / workgroups  (a: the barriers and list set-up of a frame; b: the part that divides over the
// cluster), so a stream finishes after  frames * (a + b / C).
struct PlanCost {
    double a_us, b_us;
    double finish_us(double frames, int c) const { return std::max(frames, 1.0) * (a_us + b_us / std::max(c, 1)); }
};

struct PlanCaps {                         // the largest cluster of stream k of the plan
    int n_work, mcw, mcw_bg;
    int of(int k) const { return k < n_work ? mcw : mcw_bg; }
};

// plan_mode 1 (JD_PLAN=1; measured, not the default): the MEASURED curve - configs[1]'s longest stream with every
// cluster capped at C = 1 .. 8 workgroups takes 86, 56, 46, 41, 38, 35.5, -, 32 us per frame: a + b / C with a = 24.6,
// b = 61.4 to within 2 % - and whole workgroups dealt GREEDILY: every stream starts with plan_min_cw, the next one
// goes to the stream that would finish last, until the grid is used up; beside a launch the next batch's table is
// scored, so workgroups that would shorten the launch below what the chip needs for BOTH (a cluster's barrier
// share a * C burns CU-time) are not dealt.  The launch itself gets much shorter (configs[1]: 38.5 -> 35.3 ms
// un-cut, 29.6 with every workgroup dealt) but the step does not: scored ahead it is bound by CU-time either
// way (38.2-39.2 against 38.3-39.6 ms), in the serial order it gains 5-7 % with b = 61.4 and nothing with a
// b that is safe for streams heavier than the longest one (one b serves all streams, and a stream that gets
// ONE workgroup on a b that is too small is the straggler), and the configs[4] graph loses 1-2 %.
// cw: the running batch's clusters (out).  Returns the workgroups dealt.
static inline int plan_greedy(const PlanIn &in, const PlanCost &m, int nwg, int mcw, std::vector<int> &cw)
{
    const int n_work = in.n_work;
    const double a_us = m.a_us, b_us = m.b_us;
    std::priority_queue<std::pair<double, int>> pq;
    double cu_us = 0.0;                                                // CU-time of the plan so far
    const int c0 = std::max(1, std::min(std::min(in.plan_min_cw, mcw), nwg / n_work));   // every stream starts with this many
    for (int k = 0; k < n_work; ++k) {
        const double fr = std::max(in.weight[k], 1.0);
        cw[(size_t)k] = c0;
        pq.push({fr * (a_us + b_us / c0), k});
        cu_us += fr * (a_us * c0 + b_us);
    }
    int used = n_work * c0;
    while (used < nwg && !pq.empty()) {
        const std::pair<double, int> top = pq.top();
        const int k = top.second;
        if (cw[(size_t)k] >= mcw) break;                               // the launch cannot end sooner than this stream
        if (in.gmm_cu_us > 0.0 && top.first <= (cu_us + in.gmm_cu_us) / nwg) break;
        pq.pop();
        const double fr = std::max(in.weight[k], 1.0);
        ++cw[(size_t)k]; ++used;
        cu_us += fr * a_us;
        pq.push({fr * (a_us + b_us / cw[(size_t)k]), k});
    }
    return used;
}

// the workgroups the streams want if all are to finish after tau (each within 1 .. its cap); out: per stream, or null
static inline double plan_need(double tau, const std::vector<double> &wt, const PlanCost &m, const PlanCaps &caps, std::vector<double> *out)
{
    double tot = 0.0;
    for (int k = 0; k < (int)wt.size(); ++k) {
        const double fr = std::max(wt[(size_t)k], 1.0);
        const double slack = tau / fr - m.a_us;
        double c = slack > 1e-9 ? m.b_us / slack : 1e9;
        c = std::min(std::max(c, 1.0), (double)caps.of(k));
        if (out) (*out)[(size_t)k] = c;
        tot += c;
    }
    return tot;
}

// plan_mode 0: wt[k] = frames stream k has in this launch.  The launch ends with its last stream: the C_k that make all
// streams finish together solve  C_k = b / (tau / frames_k - a)  for the smallest common tau the device's workgroups allow
// (bisection).  a and b were fitted on configs[1] (DESIGN.md "cluster sizes"); sizing by a stream's measured work per
// frame (a pilot launch, or the previous chunk's counters) was tried and is slower - the work of the frames ahead is not
// the work of the frames behind.  The constants are those fitted in round 2 (a = 10, b = 360 - right at 58 ms per step,
// wrong now, but erring towards larger short clusters, which is what re-planning and scoring ahead forgive), the clusters
// the floor of the continuous solution.
// cw: one cluster per entry of wt (out).
static inline void plan_bisect(const std::vector<double> &wt, const PlanCost &m, const PlanCaps &caps, int nwg_plan, std::vector<int> &cw)
{
    const int n_plan = (int)wt.size();
    double lo_t = 0.0, hi_t = 1.0;
    while (plan_need(hi_t, wt, m, caps, nullptr) > nwg_plan && hi_t < 1e15) hi_t *= 2.0;
    for (int step = 0; step < 60; ++step) {
        const double mid = 0.5 * (lo_t + hi_t);
        if (plan_need(mid, wt, m, caps, nullptr) > nwg_plan) lo_t = mid; else hi_t = mid;
    }
    std::vector<double> want((size_t)n_plan);
    plan_need(hi_t, wt, m, caps, &want);
    int used = 0;
    std::vector<std::pair<double, int>> frac;
    for (int k = 0; k < n_plan; ++k) {
        cw[(size_t)k] = std::max(1, std::min(caps.of(k), (int)want[(size_t)k]));
        used += cw[(size_t)k];
        frac.push_back({want[(size_t)k] - (int)want[(size_t)k], k});
    }
    std::sort(frac.begin(), frac.end(), [](const std::pair<double, int> &x, const std::pair<double, int> &y) { return x.first > y.first; });
    for (int pass = 0; pass < 4 && used < nwg_plan; ++pass)                // left-over workgroups: largest remainders first
        for (size_t i = 0; i < frac.size() && used < nwg_plan; ++i)
            if (cw[(size_t)frac[i].second] < caps.of(frac[i].second)) { ++cw[(size_t)frac[i].second]; ++used; }
    while (used > nwg_plan) {                                              // (rounding can only overshoot by the floor of ones)
        int big = 0;
        for (int k = 1; k < n_plan; ++k) if (cw[(size_t)k] > cw[(size_t)big]) big = k;
        if (cw[(size_t)big] <= 1) break;
        --cw[(size_t)big]; --used;
    }
}

// The clusters of the running batch and, behind them, of the batch behind (n_work + n_bg sizes).
static inline std::vector<int> plan_sizes(const PlanIn &in, const PlanCost &m, const PlanCaps &caps, int nwg)
{
    const int n_work = in.n_work, n_bg = in.n_bg;
    if (in.plan_mode == 1) {
        std::vector<int> cw((size_t)n_work, 1);
        const int used = plan_greedy(in, m, nwg, caps.mcw, cw);
        // The streams of the batch behind join the plan: one workgroup each, plus what the plan of this batch leaves,
        // dealt evenly (up to JD_BG_CW) - they are ordinary clusters from here on, only not what the launch waits for.
        // (the measured-curve plan deals this batch only: the rest, evenly)
        if (n_bg > 0) cw.insert(cw.end(), (size_t)n_bg, std::max(1, std::min(caps.mcw_bg, 1 + std::max(0, nwg - used) / n_bg)));
        return cw;
    }
    // One plan for both batches: a stream of the batch behind counts with a part of the frames it has ahead
    // (bg_weight: its turn as the batch the caller waits for is still to come - it has two launches to get through)
    // and so gets workgroups by its length like everybody else: the long utterances, which are what the NEXT launch
    // will last as long as, are the ones that get ahead.
    std::vector<double> wt(in.weight, in.weight + n_work);
    for (int i = 0; i < n_bg; ++i) wt.push_back(in.bg_weight * in.bg_left[i]);
    std::vector<int> cw(wt.size(), 1);
    plan_bisect(wt, m, caps, nwg + n_bg, cw);
    return cw;
}

// XCD-local launch (jd_search.h): every cluster inside one eighth of the grid - the clusters go, largest
// first, into the eighth with the most room; one that fits nowhere shrinks to the room there is, and what
// an eighth has left over in the end goes to its cluster with the latest predicted finish.  The packed plan
// is taken if the model says it ends no more than 4 % after the unpacked one (what plain stores and L2
// atomics are measured to be worth): a cluster squeezed into a corner is a long tail.
// cw_all: the unpacked clusters; pos, cwx: the packed ones (out).  False: the launch stays unpacked.
static inline bool plan_pack_xcd(const PlanIn &in, const PlanCost &m, const PlanCaps &caps, const std::vector<int> &cw_all,
                                 std::vector<int> &pos, std::vector<int> &cwx)
{
    const int n_work = in.n_work, n_tot = (int)cw_all.size(), bin = in.nwg_all / 8;
    // (a stream of the batch behind is not on the launch's critical path)
    auto t_of = [&](int k, int c) { return (k >= n_work || in.weight[k] <= 0.0) ? 0.0 : m.finish_us(in.weight[k], c); };
    std::vector<int> order((size_t)n_tot), room(8, bin);
    std::vector<std::vector<int>> member(8);
    pos.assign((size_t)n_tot, 0);
    cwx = cw_all;
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cwx[(size_t)x] > cwx[(size_t)y]; });
    for (int k : order) {
        int b = 0;
        for (int q = 1; q < 8; ++q) if (room[(size_t)q] > room[(size_t)b]) b = q;
        if (room[(size_t)b] <= 0) return false;
        cwx[(size_t)k] = std::min(cwx[(size_t)k], room[(size_t)b]);
        member[(size_t)b].push_back(k);
        room[(size_t)b] -= cwx[(size_t)k];
    }
    for (int b = 0; b < 8; ++b) {
        while (room[(size_t)b] > 0 && !member[(size_t)b].empty()) {
            int late = -1;
            for (int k : member[(size_t)b])
                if (cwx[(size_t)k] < caps.of(k) && (late < 0 || t_of(k, cwx[(size_t)k]) > t_of(late, cwx[(size_t)late]))) late = k;
            if (late < 0) break;
            ++cwx[(size_t)late]; --room[(size_t)b];
        }
        int at = b * bin;
        for (int k : member[(size_t)b]) { pos[(size_t)k] = at; at += cwx[(size_t)k]; }
    }
    double tau_plain = 0.0, tau_xl = 0.0;
    for (int k = 0; k < n_work; ++k) {
        tau_plain = std::max(tau_plain, t_of(k, cw_all[(size_t)k]));
        tau_xl = std::max(tau_xl, t_of(k, cwx[(size_t)k]));
    }
    return !(tau_xl > in.xl_slack * tau_plain);
}

// Re-planning under way (SearchArgs::rebalance_at): the plan makes the streams finish together only as
// far as frames predict work; when a fifth of the grid has run out of work the launch is cut short and the
// rest planned anew - worth it while the rest is long against the ~0.2 ms a relaunch costs.
// (not with the batch behind beside it: a cut stops ITS streams too, every leg pays the launch's set-up again and
// the workgroups a finished cluster leaves are few against what the batch behind keeps busy anyway - measured at
// configs[1]: 35.4 ms per step with cuts, 30.2 without; JD_BG_REBALANCE=1 brings them back)
static inline int plan_rebalance_at(const PlanIn &in, const PlanCost &m, const PlanOut &out)
{
    if (!(in.rebalance && in.n_work >= 4 && (in.n_bg == 0 || in.bg_rebalance))) return 0;
    // (stream k's frames with the cluster of the k-th item IN LAUNCH ORDER, as this estimate has always been made: in an
    // XCD-local plan, sorted by first workgroup, that is another stream's cluster)
    double tau = 0.0;
    for (int k = 0; k < in.n_work; ++k) tau = std::max(tau, m.finish_us(in.weight[k], out.items[(size_t)k].cw));
    return tau > in.rebalance_min_us ? std::max(1, (int)(in.rebalance_frac * out.grid)) : 0;
}

static inline PlanOut plan_clusters(const PlanIn &in)
{
    PlanOut out;
    const int n_work = in.n_work, n_bg = in.n_bg;
    const int nwg = in.nwg_all - n_bg;                                 // what the plan of the running batch may use
    out.Cw = std::max(1, std::min(in.max_cw, nwg / n_work));
    out.n_slots = std::min(n_work, std::max(1, nwg / out.Cw));
    out.weighted = in.weight && in.weighted && (n_work > 1 || n_bg > 0) && in.max_cw > 1 && nwg >= 2 * n_work;
    if (!out.weighted) {
        // uniform clusters, the batch behind (if any) not in the launch; more streams than clusters: the clusters take them in turn
        for (int k = 0; k < n_work; ++k) out.items.push_back({k, k * out.Cw, out.Cw, true});
        out.grid = out.n_slots * out.Cw;
        out.xl = in.xl_ok && out.Cw > 1 && (out.grid & 7) == 0 && ((out.grid >> 3) % out.Cw) == 0;   // uniform clusters that tile the eighths
        return out;
    }
    // (with the batch behind beside it: past eight workgroups a cluster gains little - 32 us per frame against 28 at
    // sixteen - and the workgroups do more for the streams of the batch behind, JD_FG_CW)
    const int mcw = n_bg > 0 ? std::min(in.max_cw, in.fg_cw_cap) : in.max_cw;
    const bool greedy = in.plan_mode == 1;
    const PlanCost m{greedy ? in.a2_us : in.a_us, (greedy ? in.b2_us : in.b_us) * in.load_scale};
    const PlanCaps caps{n_work, mcw, std::max(1, std::min(in.bg_cw_cap, in.max_cw))};
    const std::vector<int> cw_all = plan_sizes(in, m, caps, nwg);
    const int n_tot = n_work + n_bg;
    std::vector<int> pos, cwx;
    out.xl = in.xl_ok && (in.nwg_all & 7) == 0 && plan_pack_xcd(in, m, caps, cw_all, pos, cwx);
    if (out.xl) {
        for (int k = 0; k < n_tot; ++k) out.items.push_back({k, pos[(size_t)k], cwx[(size_t)k], k < n_work});
        // (the kernel searches by first workgroup)
        std::sort(out.items.begin(), out.items.end(), [](const PlanItem &x, const PlanItem &y) { return x.first < y.first; });
        out.grid = in.nwg_all;
    } else {
        int first = 0;
        for (int k = 0; k < n_tot; ++k) {
            out.items.push_back({k, first, cw_all[(size_t)k], k < n_work});
            first += cw_all[(size_t)k];
        }
        out.grid = first;
    }
    out.rebalance_at = plan_rebalance_at(in, m, out);
    return out;
}

// ------------------------------------------------------------------------------------------------------------------
// The geometry of the search kernels that STAY on the device (jd_host_resident.h: jd_res_start): the rows of a likelihood buffer, the
// streams' clusters, which kernel serves them and where the slots go.  The build's constants come in as fields (no HIP macro here).
struct ResPlanIn {
    int n_cus, n_streams, rows_per_buf;
    int max_cw;                           // largest cluster JD_CW allows
    long long cap_slots, cap_items;       // ... and the arenas: instance slots and frontier items per stream
    bool pipeline;                        // the batch pipeline drives the kernel: every stream a slot of ONE workgroup
    int free_cus, slot, xl, keep_se;      // development knobs (JD_RES_FREE_CUS, JD_RES_SLOT, JD_RES_XL, JD_SLOT_KEEP_SE), -1: unset
    int sw, wg_per_cu, slot_wg_per_cu, gmm_rows2, res_ring_w;   // the build's SW, WG_PER_CU, SLOT_WG_PER_CU, GMM_ROWS2, RES_RING_W
};

enum ResPlanVerdict {
    RES_PLAN_OK = 0,
    RES_PLAN_LIMITS,                      // more than 1024 streams, or more row tiles than a scoring launch's list holds
    RES_PLAN_CLUSTERS,                    // the clusters of k_resident do not fit the device
    RES_PLAN_SLOTS,                       // the slots of k_slot are not all resident at once
};

struct ResPlanOut {                       // (what follows the point a verdict other than ok was reached stays 0)
    ResPlanVerdict verdict = RES_PLAN_OK;
    int rows = 0;                         // rows per likelihood buffer: whole scoring tiles
    int Cw = 0;                           // workgroups per cluster
    bool slot = false;                    // one workgroup per stream: the slot kernel (jd_slot.h), SLOT_WG_PER_CU of them per CU
    bool xl = false;                      // k_resident's XCD-local flavour of the memory operations - a cluster of one sits on one XCD
    int park_cus = 0, park_fill = 0;      // slots: CUs parked while the grid is dealt, and the slots that find room beside them
};

static inline ResPlanOut plan_resident(const ResPlanIn &in)
{
    ResPlanOut out;
    const int n = in.n_streams;
    const int tiles = (in.rows_per_buf + in.gmm_rows2 - 1) / in.gmm_rows2;
    out.rows = tiles * in.gmm_rows2;
    if (n > 1024 || 2 * n * tiles > in.res_ring_w) { out.verdict = RES_PLAN_LIMITS; return out; }
    // clusters: what the arenas allow, and a sixth of the chip left to the scoring, collection and finish kernels
    const int cw_cap = (int)std::max<long long>(1, std::min<long long>(in.cap_slots / (64 * in.sw), in.cap_items / (512 * in.sw)));
    // (the scoring of what the streams search: about 1.6 CUs per stream at their pace, and a quarter of the chip at least -
    // sixteen C++ callers: 407 k frames/s with 24 CUs left, 433 k with 40, 469 k with 64, 462 k with 96)
    int free_cus = std::min(in.n_cus / 2, std::max(in.n_cus / 4, (n * 8) / 5));
    if (in.free_cus >= 0 && in.free_cus < in.n_cus) free_cus = in.free_cus;
    out.Cw = std::max(1, std::min(std::min(in.max_cw, cw_cap), (in.n_cus * in.wg_per_cu - free_cus) / n));
    if (in.pipeline) out.Cw = 1;                                       // (however few they are)
    // One workgroup per stream: the slot kernel (jd_slot.h) - compiled for four waves per SIMD, SLOT_WG_PER_CU workgroups per CU,
    // every per-frame word in LDS.  (JD_RES_SLOT=0, development: k_resident's one-workgroup clusters, one per CU.)
    out.slot = out.Cw == 1 && in.slot != 0;
    if (!out.slot && out.Cw * n > in.n_cus * in.wg_per_cu) { out.verdict = RES_PLAN_CLUSTERS; return out; }
    // (the slot kernel's workgroups answer a mailbox: one that is never dispatched never answers - all of them resident, or none)
    if (out.slot && n > in.n_cus * in.slot_wg_per_cu) { out.verdict = RES_PLAN_SLOTS; return out; }
    out.xl = out.Cw == 1 && in.xl != 0;
    if (out.slot) {
        // (whole CUs per shader engine: 32 engines of n_cus / 32 CUs each, every one keeps the same number for the slots)
        const int per_se = std::max(1, in.n_cus / 32);
        int keep_se = per_se;
        if (in.keep_se >= 1 && in.keep_se <= per_se && in.keep_se * 32 * in.slot_wg_per_cu >= n) keep_se = in.keep_se;
        out.park_cus = (per_se - keep_se) * 32;
        out.park_fill = std::min(n, keep_se * 32 * in.slot_wg_per_cu);
    }
    return out;
}

// ------------------------------------------------------------------------------------------------------------------
// The batch pipeline's scoring launches (jd_host_resident.h: pump_score).  A piece is a grid of row tiles x state groups; the device
// holds `resident_scoring_wgs` of the scoring kernel's workgroups at once beside the slots, so the piece runs in rounds of that
// many, and the kernel behind it on the side stream cannot start under a last round that is half empty.

// Scoring workgroups resident at once beside the slots, from what the runtime says of each kernel ALONE: occ_slot slot workgroups
// fill a CU, occ_gmm scoring workgroups fill one, and a CU that holds k slots has (occ_slot - k) / occ_slot of itself left.  The
// slots are dealt one per CU first (jd_host_resident.h: park_and_launch_slots).
static inline int plan_resident_scoring_wgs(int n_cus, int n_slots, int occ_slot, int occ_gmm)
{
    if (n_cus < 1 || occ_slot < 1 || occ_gmm < 1) return 1;
    const int base = std::max(0, n_slots) / n_cus, extra = std::max(0, n_slots) % n_cus;   // `extra` CUs hold base + 1 slots
    auto beside = [&](int k) { return k >= occ_slot ? 0 : occ_gmm * (occ_slot - k) / occ_slot; };
    return std::max(1, extra * beside(base + 1) + (n_cus - extra) * beside(base));
}

// Rows per piece: the multiple of 128 (GMM_ROWS2) in [lo, hi] whose tiles - rows / 128 x n_state_groups - leave the smallest share
// of their last round empty; of two that leave the same, the smaller.  (lo, hi: rounded inwards to whole tiles; one tile at least.)
#define PLAN_PIECE_TILE 128
static inline long long plan_piece_waste(long long row_tiles, int n_state_groups, int resident_scoring_wgs)
{
    const long long w = std::max(1, resident_scoring_wgs), tiles = row_tiles * std::max(1, n_state_groups);
    return (w - tiles % w) % w;                                        // workgroup places of the last round nobody takes
}
static inline int plan_piece_rows(int n_state_groups, int resident_scoring_wgs, int lo, int hi)
{
    long long t_lo = std::max(1, (lo + PLAN_PIECE_TILE - 1) / PLAN_PIECE_TILE), t_hi = std::max(1, hi / PLAN_PIECE_TILE);
    if (t_hi < t_lo) t_hi = t_lo;
    long long best = t_lo, best_w = plan_piece_waste(t_lo, n_state_groups, resident_scoring_wgs);
    for (long long t = t_lo + 1; t <= t_hi && best_w > 0; ++t) {
        const long long w = plan_piece_waste(t, n_state_groups, resident_scoring_wgs);
        if (w < best_w) { best = t; best_w = w; }
    }
    return (int)(best * PLAN_PIECE_TILE);
}
