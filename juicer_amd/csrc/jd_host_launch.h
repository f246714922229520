// jd_host_launch.h - launch_search (included by jd_device.hip): how the streams of a work list get their workgroups for ONE persistent
// launch of the search - uniform clusters, the weighted plan (clusters sized so that the streams finish together), its XCD-local
// packing, the batch behind the running one beside it, the slot kernel as a plain launch for more streams than CUs - and the loop
// around the launches (Path collections, re-planning cuts).  Reference: the per-file loop of DecoderBatchTest::run,
// src/DecoderBatchTest.cpp:738-771, as one launch for many utterances.
#pragma once

#include "jd_plan.h"

// The first words of a stream's StreamCtl as the host reads them back (the kernels' struct, jd_search.h, stays as it is).
struct StreamHead { int frame, T, error, needs_init, started, lst_nw, n_rec_hint; float best_emit; int dirty_nw[2]; };
#define HEAD_AT(f) static_assert(offsetof(StreamHead, f) == offsetof(StreamCtl, f), "StreamHead::" #f " is not where StreamCtl has it")
HEAD_AT(frame); HEAD_AT(T); HEAD_AT(error); HEAD_AT(needs_init); HEAD_AT(started); HEAD_AT(lst_nw); HEAD_AT(n_rec_hint); HEAD_AT(best_emit);
HEAD_AT(dirty_nw);
#undef HEAD_AT
static_assert(sizeof(StreamHead) == 40, "StreamHead: ten words");

// The heads of streams [s0, s0 + n) as they stand now - or, given a stream, behind everything queued on it (waited for).
static int read_heads(jd_dec *d, int s0, int n, std::vector<StreamHead> *out, hipStream_t st)
{
    out->resize((size_t)n);
    if (st) {
        HIPCHK(hipMemcpy2DAsync(out->data(), sizeof(StreamHead), d->d_ctl + s0, sizeof(StreamCtl), sizeof(StreamHead), (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    } else
        HIPCHK(hipMemcpy2D(out->data(), sizeof(StreamHead), d->d_ctl + s0, sizeof(StreamCtl), sizeof(StreamHead), (size_t)n, hipMemcpyDeviceToHost));
    return JD_OK;
}

// The load (instances + arcs per stream-frame) of the streams of a work list so far, from their statistics:
// scales the cost model's b (jd_dec::load_scale).  Called when the decoder has not seen a batch yet.
static int learn_load(jd_dec *d, const std::vector<int2> &work_in)
{
    std::vector<long long> st((size_t)d->max_streams * ST_N);
    std::vector<StreamHead> head;
    HIPCHK(hipMemcpy2D(st.data(), ST_N * sizeof(long long), (const char *)d->d_ctl + offsetof(StreamCtl, st), sizeof(StreamCtl),
                       ST_N * sizeof(long long), (size_t)d->max_streams, hipMemcpyDeviceToHost));
    const int hr = read_heads(d, 0, d->max_streams, &head, nullptr);
    if (hr) return hr;
    double work = 0.0, frames = 0.0;
    for (const int2 &w : work_in) {
        work += (double)st[(size_t)w.x * ST_N + ST_INSTS] + (double)st[(size_t)w.x * ST_N + ST_ARCS];
        frames += (double)head[(size_t)w.x].frame;
    }
    if (frames > 0.0) d->load_scale = ahead_load(work, frames);
    return JD_OK;
}

// the flavours of k_search (jd_search.h): HMMs of up to 5 / 8 states, agent-scope / XCD-local memory model, static / lazily
// composed graph, word / model-level output
typedef void (*SearchKernel)(SearchArgs);
static SearchKernel search_kernel(bool ne3, bool xl, bool lazy, bool mdl)
{
    static const SearchKernel tab[16] = {
        k_search<6, false, false, false>, k_search<6, false, true, false>, k_search<6, true, false, false>, k_search<6, true, true, false>,
        k_search<3, false, false, false>, k_search<3, false, true, false>, k_search<3, true, false, false>, k_search<3, true, true, false>,
        k_search<6, false, false, true>, k_search<6, false, true, true>, k_search<6, true, false, true>, k_search<6, true, true, true>,
        k_search<3, false, false, true>, k_search<3, false, true, true>, k_search<3, true, false, true>, k_search<3, true, true, true>,
    };
    return tab[(mdl ? 8 : 0) + (ne3 ? 4 : 0) + (xl ? 2 : 0) + (lazy ? 1 : 0)];
}


// ... and of k_slot_batch (jd_slot.h): HMM size class, word / model-level output
static SearchKernel slot_kernel(bool ne3, bool mdl)
{
    static const SearchKernel tab[4] = { k_slot_batch<3, true>, k_slot_batch<6, true>, k_slot_batch<3, false>, k_slot_batch<6, false> };
    return tab[(mdl ? 0 : 2) + (ne3 ? 0 : 1)];
}

// the decoder's place in the per-device tables (g_search_mu and its counters)
static size_t dev_index(const jd_dec *d) { return (size_t)std::min(std::max(d->device, 0), JD_MAX_DEVICES - 1); }

// The device's search lock, taken: whoever waits for it is counted (a resident kernel makes room: jd_res_should_yield), and
// whoever gets it counts the turn up (jd_res_yield: the one who let go sees the waiter take it).
static std::unique_lock<std::mutex> lock_search(size_t dev_i)
{
    g_search_waiters[dev_i].fetch_add(1);
    std::unique_lock<std::mutex> lock(g_search_mu[dev_i]);
    g_search_waiters[dev_i].fetch_sub(1);
    g_search_turn[dev_i].fetch_add(1);
    return lock;
}

static int pf_launch(jd_dec *d);
static bool pf_wants_scoring(const jd_dec *d);
static bool pf_scoring_in_flight(const jd_dec *d);
static int pf_background(jd_dec *d, int fg_bank, const std::vector<StreamHead> *heads, hipStream_t st, std::vector<int2> *work, std::vector<double> *left);
static int mark_init(jd_dec *d, int s0, int n, hipStream_t st);

// room for n work items in d_work
static int ensure_work_cap(jd_dec *d, int n)
{
    if (n <= d->work_cap) return JD_OK;
    if (d->d_work) (void)hipFree(d->d_work);
    d->d_work = nullptr; d->work_cap = 0;
    const size_t cap = std::max<size_t>((size_t)n, (size_t)d->max_streams);
    HIPCHK(hipMalloc(&d->d_work, cap * sizeof(int4)));
    d->work_cap = (int)cap;
    return JD_OK;
}

// Two batches in flight: the plan makes the clusters of this batch finish together and the utterances of the
// batch behind fill what is left - nothing idles, and the scoring of the table after that, which lives on idle CUs,
// would finish long after the launch (and the batch behind the next one start late).  So the scoring gets CUs of its
// own (jd_ahead.h: ahead_reserve); the search is planned on the rest.
static int scoring_reserve(jd_dec *d, bool planned, bool first_launch, int nwg_all)
{
    if (!(d->fg_bank >= 0 && d->pf_armed && planned && (pf_wants_scoring(d) || pf_scoring_in_flight(d)))) return 0;
    if (first_launch) d->reserve_now = ahead_reserve(d->score_reserve, d->gmm_ms_per_row, d->last_wave_ms, ahead_scoring_rows(d->pf_q), nwg_all);
    return d->reserve_now;                                             // (the legs of a re-planned launch leave the same CUs alone)
}

// two batches in flight: the utterances of the batch behind this one, one workgroup each at least, on a quarter of the grid at most
static int fetch_background(jd_dec *d, hipStream_t st, int n_work, int nwg_all, std::vector<int2> *bg, std::vector<double> *bg_left)
{
    const bool started = !d->pf_q.empty() && d->pf_q.front().bank >= 0;
    std::vector<StreamHead> heads;
    if (started) { const int hr = read_heads(d, 0, d->max_streams, &heads, nullptr); if (hr) return hr; }
    const int br = pf_background(d, d->fg_bank, started ? &heads : nullptr, st, bg, bg_left);
    if (br) return br;
    if (ahead_bg_clipped((int)bg->size(), n_work, nwg_all)) { bg->clear(); bg_left->clear(); }
    return JD_OK;
}

// The plan of one launch (jd_plan.h) from the decoder's knobs.  nwg_all: the workgroups the scoring reserve leaves.
static PlanOut plan_launch(const jd_dec *d, const std::vector<double> *weight, int n_work, const std::vector<double> &bg_left, int nwg_all)
{
    PlanIn in;
    in.weight = weight ? weight->data() : nullptr; in.n_work = n_work;
    in.bg_left = bg_left.data(); in.n_bg = (int)bg_left.size();
    in.nwg_all = nwg_all;
    // a wave segment holds at least one 64-record chunk of instances and 512 frontier items (one wave
    // writes the whole epsilon closure of the items it expands)
    const int cw_cap = (int)std::max<int64_t>(1, std::min<int64_t>(d->cap_slots / (64 * SW), d->cap_items / (512 * SW)));
    in.max_cw = std::min(d->max_cw, cw_cap);
    in.fg_cw_cap = d->fg_cw_cap; in.bg_cw_cap = d->bg_cw_cap; in.bg_weight = d->bg_weight;
    in.weighted = d->weighted != 0; in.plan_mode = d->plan_mode; in.plan_min_cw = d->plan_min_cw;
    in.a_us = d->model_a_us; in.b_us = d->model_b_us; in.a2_us = d->model2_a_us; in.b2_us = d->model2_b_us; in.load_scale = d->load_scale;
    in.gmm_cu_us = (d->plan_mode == 1 && d->pf_armed && pf_wants_scoring(d))
                 ? d->pf_gmm_weight * 1e3 * d->gmm_ms_per_row * ahead_scoring_rows(d->pf_q) * (nwg_all - in.n_bg) : 0.0;
    in.xl_ok = d->xl_ok; in.xl_slack = d->xl_slack;
    in.rebalance = d->rebalance != 0; in.bg_rebalance = d->bg_rebalance != 0;
    in.rebalance_frac = d->rebalance_frac; in.rebalance_min_us = d->rebalance_min_us;
    return plan_clusters(in);
}

// k_search is persistent and its clusters spin at barriers of their own: ALL its workgroups have to be resident
// at once (one per CU) ... and the kernel must fit a CU the way the grid assumes: asked of the runtime once per decoder, for the
// flavours it may launch (a build with other SW / WG_PER_CU / LDS sizes, or a device with smaller CUs,
// fails here with a message instead of after a 30 s barrier time-out)
static int check_occupancy(jd_dec *d, bool ne3)
{
    if (d->occupancy_ok) return JD_OK;
    const bool lz = d->C.lazy != nullptr;
    for (int v = 0; v < 2; ++v) {
        int per_cu = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)search_kernel(ne3, v != 0, lz, d->models), SNT, 0));
        if (per_cu < WG_PER_CU)
            return jd_fail(JD_EHIP, "k_search needs %d workgroup(s) of %d threads resident per CU, the device takes %d: "
                           "its clusters could not all be resident at once", WG_PER_CU, SNT, per_cu);
    }
    d->occupancy_ok = true;
    return JD_OK;
}

// (a launch beside which the next batch's table is scored is not cut short for a re-plan while that scoring runs -
// status[4]: its blocks sit on the CUs that finished clusters left, and a relaunch would wait for them to drain)
// Whether that pays depends on what the scoring is against the search: where it is a fifth of it (configs[1]) the
// whole scoring fits the tail the clusters leave and the step is the one uncut launch (47.3 -> 40.9 ms; re-planned
// at will: 46.3); where it is a few per cent (the 14 M-arc graph: 13 of 340 ms) the tail begins late, the scoring
// would hold the re-planning up for the whole launch (348 against 343 ms serial) and is better slotted in at the
// cuts (340).  Decided by the measured costs of this decoder's last waves.
static bool hold_replan_for_scoring(const jd_dec *d, const std::vector<double> *weight)
{
    if (!(d->pf_armed && pf_wants_scoring(d))) return false;
    double frames_now = 0.0;
    if (weight) for (double w : *weight) frames_now += w;
    return ahead_hold_replan(d->pf_rebalance, d->gmm_ms_per_row, ahead_scoring_rows(d->pf_q), d->search_ms_per_frame, frames_now);
}

// More streams than the chip has CUs, one workgroup each: the slot kernel as a plain launch (jd_slot.h: k_slot_batch) - a
// workgroup per stream, two per CU, the dispatcher deals the next one when one leaves - instead of k_search's
// one-per-CU workgroups that take their streams one after the other.  (JD_SLOT_BATCH=1 / 0, development: always / never.)
static int want_slot_batch(jd_dec *d, const SearchArgs &A, const std::vector<int2> &work_in, int n_bg, int nwg_all, hipStream_t st, bool *slot_batch)
{
    const int n_work = (int)work_in.size();
    *slot_batch = A.n_slots > 0 && A.Cw == 1 && n_bg == 0 && n_work > nwg_all && !d->C.lazy && !A.cells;
    if (const char *e = jd_dev_env("JD_SLOT_BATCH")) *slot_batch = atoi(e) != 0 && A.Cw == 1 && n_bg == 0 && !d->C.lazy && !A.cells && (A.n_slots > 0 || n_work == 1);
    if (!*slot_batch) return JD_OK;
    // The slot kernel reads lists of ITS geometry only (eight wave segments, slot_run: JDE_GEOM), k_search those of any.  A stream
    // in the middle of an utterance whose last frames were written by a cluster of several workgroups - jd_streams_push or the
    // broker's ticks served 100 streams with clusters of two, then more streams joined - stays with k_search for this launch:
    // the shape of the launch alone does not decide.  (The streams' heads as they stand behind everything queued on `st`.)
    std::vector<StreamHead> hd;
    const int hr = read_heads(d, 0, d->max_streams, &hd, st);
    if (hr) return hr;
    for (const int2 &w : work_in) {
        const StreamHead &h = hd[(size_t)w.x];
        if (h.started && !h.needs_init && h.error == 0 && (h.lst_nw != SW || h.dirty_nw[0] != SW || h.dirty_nw[1] != SW)) { *slot_batch = false; break; }
    }
    if (!*slot_batch && getenv("JD_VERBOSE"))
        fprintf(stderr, "k_slot_batch: a stream's lists were written by a cluster of several workgroups - this launch stays with k_search\n");
    return JD_OK;
}

// The streams of work_in that are not through, and what each has ahead in the next launch.  A stream that stopped for a
// collection after n frames will, by and large, stop again after as many (its records per frame change slowly): what it
// has ahead IN THE NEXT LAUNCH is the smaller of that and the frames it has left - sized by that, the streams stop together
// instead of idling.
static int next_round(jd_dec *d, const std::vector<int2> &work_in, int f0, int f_end, std::vector<int> *frame_before,
                      std::vector<int2> *rest, std::vector<double> *weight_now)
{
    std::vector<StreamHead> head;
    const int hr = read_heads(d, 0, d->max_streams, &head, nullptr);
    if (hr) return hr;
    rest->clear(); weight_now->clear();
    if (d->load_scale == 1.0) { const int lr = learn_load(d, work_in); if (lr) return lr; }   // first batch of this decoder
    if (frame_before->empty()) frame_before->assign((size_t)d->max_streams, f0);
    for (const int2 &w : work_in) {
        const StreamHead &h = head[(size_t)w.x];
        const int end = std::min(h.T, f_end), left = end - h.frame;
        const int done = h.frame - (*frame_before)[(size_t)w.x];
        (*frame_before)[(size_t)w.x] = h.frame;
        // (a launch cut short for a re-plan says nothing about when a stream's arena fills up: then the frames left count)
        if (left > 0 && h.error == 0) {
            rest->push_back(w);
            weight_now->push_back((double)((done > 0 && d->h_status[3] == 0) ? std::min(left, done) : left));
        }
    }
    return JD_OK;
}

// Advance the streams of `work` ({stream, likelihood slot}) through frames [.., f_end) with ONE
// persistent launch (k_search): every stream gets a cluster of workgroups, one 512-thread workgroup
// per CU in total, all resident at once (the clusters synchronise with barriers of their own).  A
// launch stops a stream early when its Path arena needs collecting; the collection (k_gc_*) runs
// after such a launch and the launch is repeated until every stream is through.
static int launch_search(jd_dec *d, const std::vector<int2> &work_first, const float *ll, long long ll_stride, int f0, int f_end,
                         hipStream_t st, const std::vector<double> *weight_first = nullptr)
{
    if (work_first.empty()) return JD_OK;
    std::vector<int2> work_in = work_first, rest;
    std::vector<int2> bg;                                              // streams of the batch behind, advanced beside these (pf_background)
    std::vector<double> bg_left;                                       // ... and the frames each has ahead
    std::vector<double> weight_now;
    std::vector<int> frame_before;                                     // per stream: where the previous launch found it
    const std::vector<double> *weight = weight_first;
    const bool ne3 = d->am->max_n <= 5;
    const int max_rounds = (f_end - f0) + 64;                          // every launch makes at least one frame of progress
    for (int it = 0;; ++it) {
        const int n_work = (int)work_in.size();
        int nwg_all = std::max(1, d->n_cus * WG_PER_CU);
        const bool planned = weight && d->weighted;
        int reserve = scoring_reserve(d, planned, it == 0, nwg_all);
        bg.clear(); bg_left.clear();
        if (d->fg_bank >= 0 && planned) { const int br = fetch_background(d, st, n_work, nwg_all, &bg, &bg_left); if (br) return br; }
        const int n_bg = (int)bg.size();
        while (reserve > 0 && nwg_all - reserve - n_bg < 2 * n_work) reserve -= 8;
        nwg_all -= std::max(reserve, 0);
        const int wr = ensure_work_cap(d, n_work + n_bg);
        if (wr) return wr;
        SearchArgs A;
        A.C = d->C; A.ctl = d->d_ctl; A.streams = d->d_streams; A.work = d->d_work; A.n_work = n_work; A.n_prio = 0;
        A.cells = (d->d_cells && ll == d->d_ll_slab) ? d->d_cells + 2 : nullptr;   // (the first two words: the counter of jd_dec_debug_cells)
        const PlanOut P = plan_launch(d, weight, n_work, bg_left, nwg_all);
        A.Cw = P.Cw; A.n_slots = P.n_slots;
        if (P.weighted) {
            if (n_bg > 0) { A.n_prio = n_work; A.n_work = n_work + n_bg; d->bg_ran = true; }
            // (two batches in flight: clusters of one or two workgroups - one chunk of items per wave, i.e. full 64-item passes,
            // does better there than two: 31.2 against 31.9 ms per step; the heavy workloads lose 3-5 % with one)
            if (n_bg > 0 && !d->xch_forced) A.C.x_chunks = 1;
            A.n_slots = 0;
        }
        const int prio_flag = (P.weighted && n_bg > 0) ? 0x40000000 : 0;   // (SearchArgs::n_prio: which work items the launch is there for)
        std::vector<int4> work;
        for (const PlanItem &p : P.items) {
            const int2 &w = p.idx < n_work ? work_in[(size_t)p.idx] : bg[(size_t)(p.idx - n_work)];
            work.push_back(make_int4(w.x, w.y, p.first, p.cw | (p.fg ? prio_flag : 0)));
        }
        const int grid = P.grid;
        const bool xl = P.xl;
        HIPCHK(hipMemcpyAsync(d->d_work, work.data(), work.size() * sizeof(int4), hipMemcpyHostToDevice, st));
        A.ll = ll; A.ll_stride = ll_stride; A.f0 = f0; A.f_end = f_end;
        A.status = d->d_status; A.dbg = d->d_dbg; A.rebalance_at = P.rebalance_at;
        A.xl_selftest = jd_dev_env("JD_XL_SELFTEST") ? 1 : 0;                 // (test knob, see SearchArgs)
        A.resident = d->d_resident; A.launch_seq = ++d->launch_seq;
        struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) (void)hipEventDestroy(e); } } ev0, ev1;
        HIPCHK(hipEventCreate(&ev0.e)); HIPCHK(hipEventCreate(&ev1.e));
        const hipEvent_t e0 = ev0.e, e1 = ev1.e;
        const int orc = check_occupancy(d, ne3);
        if (orc) return orc;
        // Two persistent launches dispatched side by side - two decoders of this process on one device,
        // driven from two host threads - could each hold part of the CUs and wait for the rest until the barriers time
        // out: launches on one device are serialised here, from dispatch to completion.  (Other PROCESSES on the device
        // are outside this lock: the dispatcher starts the workgroups of a kernel in order, and a kernel that cannot
        // become fully resident ends in JDE_BARRIER after 30 s instead of hanging.)
        const std::unique_lock<std::mutex> search_lock = lock_search(dev_index(d));
        GpuLockGuard process_lock(d->device);                              // (other processes on this GPU: see GpuFileLock)
        const bool hold_replan = hold_replan_for_scoring(d, weight);
        bool slot_batch = false;
        const int sr = want_slot_batch(d, A, work_in, n_bg, nwg_all, st, &slot_batch);
        if (sr) return sr;
        hipLaunchKernelGGL(jd_zero_bar_kernel, dim3((A.n_work + 255) / 256), dim3(256), 0, st, d->d_ctl, d->d_work, A.n_work, d->d_status,
                           hold_replan ? 1 : 0);
        HIPCHK(hipEventRecord(e0, st));
        // the kernel flavour: HMM size class x XCD-local x lazily composed graph
        if (slot_batch) hipLaunchKernelGGL(slot_kernel(ne3, d->models), dim3((unsigned)n_work), dim3(SNT), 0, st, A);
        else hipLaunchKernelGGL(search_kernel(ne3, xl, d->C.lazy != nullptr, d->models), dim3(grid), dim3(SNT), 0, st, A);
        HIPCHK(hipEventRecord(e1, st));
        HIPCHK(hipGetLastError());
        if (d->pf_armed && pf_wants_scoring(d)) {
            // the next batch's table is scored beside this launch (jd_dec_prefetch_scores): its kernel is enqueued once
            // the search is resident - the last workgroup of the grid says so in a host-mapped word - so that scoring
            // blocks never sit on a CU a search workgroup is waiting for (2 ms: it goes ahead anyway)
            const auto tr0 = std::chrono::steady_clock::now();
            // (k_slot_batch: nothing has to be resident at once - its workgroups come and go - and nobody writes the word)
            while (!slot_batch && __atomic_load_n(d->h_resident, __ATOMIC_ACQUIRE) != A.launch_seq &&
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count() < 2.0) { }
            const int pr = pf_launch(d);
            if (pr) { (void)hipStreamSynchronize(st); return pr; }       // (k_search is in flight: not left behind with the launch lock released)
        }
        HIPCHK(hipMemcpyAsync(d->h_status, d->d_status, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) d->timing.search_ms += ms;
        if (getenv("JD_VERBOSE")) {                                        // development
            int cmin = 1 << 30, cmax = 0;
            for (const PlanItem &p : P.items) { cmin = std::min(cmin, p.cw); cmax = std::max(cmax, p.cw); }
            fprintf(stderr, "%s: %d streams, grid %d (clusters %d..%d workgroups, %s%s), frames [%d, %d): %.3f ms\n", slot_batch ? "k_slot_batch" : "k_search", n_work,
                    slot_batch ? n_work : grid, cmin, cmax, A.n_slots ? "uniform" : "weighted", xl ? ", XCD-local" : "", f0, f_end, ms);
            if (d->h_status[3]) fprintf(stderr, "          cut short for a re-plan: %d streams go on\n", d->h_status[0]);
        }
        if (d->h_status[1] != 0) {
            // a cluster of an XCD-local launch found itself on several XCDs and left its stream untouched: from
            // now on this decoder launches the agent-scope kernel (the loop below repeats the launch)
            d->xl_ok = false;
            if (getenv("JD_VERBOSE")) fprintf(stderr, "k_search: %d cluster(s) not on one XCD - agent-scope launches from here on\n", d->h_status[1]);
        }
        d->timing.search_launches += 1;
        if (slot_batch) d->timing.slot_launches += 1;
        d->timing.cluster_wgs = A.Cw;
        if (d->h_status[0] == 0 && d->h_status[1] == 0) break;
        d->timing.relaunches += 1;
        if (it >= max_rounds) return jd_fail(JD_ENOMEM, "Path arena too small: no progress after %d garbage collections", it);
        // Some streams stopped for a collection of their Path records (k_gc_*: no-ops for the streams below
        // their mark): the launch is repeated for the streams that are not through, with clusters sized for
        // what each of them still has ahead.
        // (not when every stop was for a re-plan, or a stream ahead of its turn stopping with the launch)
        if (d->h_status[0] > d->h_status[3] + d->h_status[6]) {
            launch_gc(d->C, d->d_ctl, d->d_streams, d->d_work, A.n_work, 0, ne3, d->n_cus, st);
            HIPCHK(hipGetLastError());
            // PARTIAL_DECODING: the trace rides on the collection (:362-368) - the caller has to see the stream as it
            // stands right after one (jd_stream_push; it goes on from there)
            if (d->return_on_collect) { HIPCHK(hipStreamSynchronize(st)); d->collected_now = true; return JD_OK; }
        }
        const int nr = next_round(d, work_in, f0, f_end, &frame_before, &rest, &weight_now);
        if (nr) return nr;
        if (rest.empty()) break;
        work_in.swap(rest);
        weight = weight_first ? &weight_now : nullptr;
    }
    return JD_OK;
}
