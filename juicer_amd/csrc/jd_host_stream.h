// jd_host_stream.h - the IDecoder seam of the C ABI (included by jd_device.hip): jd_stream_init / _push / _finish (IDecoder::init /
// processFrame / finish, src/Decoder.h:18-30, src/WFSTDecoderLite.cpp:139-372), jd_streams_push (several callers' frames in one launch),
// PARTIAL_DECODING (jd_dec_set_partial_interval, jd_stream_partial, jd_streams_trace: src/WFSTDecoderLite.cpp:822-896) for one stream
// and for a list of them, and the collection bookkeeping.
#pragma once

extern "C" int jd_stream_init(jd_dec *d, int32_t s)
{
    if (!d || s < 0 || s >= d->max_streams) return jd_fail(JD_EINVAL, "jd_stream_init: bad stream");
    int rc = check_device(d->device);
    if (rc) return rc;
    rc = ensure_arenas(d);
    if (rc) return rc;
    // (the streaming interface names its streams itself: whatever a stream of batches had been started ahead on them is
    // dropped - the batch concerned starts again when it is decoded)
    pf_discard(d);
    if (d->lazy_in[(size_t)s]) { d->lazy_in[(size_t)s] = 0; jd_lazy_leave(d->net, 1); }   // (an utterance that was never finished)
    bool net_failed = false;
    rc = jd_lazy_enter(d->net, 1, &net_failed);                       // (may start a new arena generation)
    if (rc) return rc;
    if (net_failed) {                                                  // as in jd_decode_batch_device
        jd_lazy_leave(d->net, 1);
        return jd_fail(JD_ENOMEM, "the lazily composed network has run out of room and other utterances are inside it: "
                       "it starts again when they are through (capacity %d states, %lld arcs)", d->net->n_states, (long long)d->net->n_arcs);
    }
    d->lazy_in[(size_t)s] = d->net->lazy_dev != nullptr;
    rc = mark_init(d, s, 1, d->s_search);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(d->s_search));
    d->stream_T[(size_t)s] = 0;
    d->stream_started[(size_t)s] = 1;
    d->stream_open[(size_t)s] = 0;
    d->last_collect[(size_t)s] = -1; d->last_trace[(size_t)s] = -1;    // WFSTDecoderLite.cpp:179-181, 202-206
    d->n_collect_host[(size_t)s] = 0;
    d->partial_label[(size_t)s].clear(); d->partial_time[(size_t)s].clear();
    d->partial_m[(size_t)s] = jd_dec::PartialModels();
    return JD_OK;
}

// tracePartialPath (:824-868) on stream s at the frame it has reached; extends the stream's
// partialPaths when a converged record is found.  Model-level output: the same launch exports the whole chain below that
// record as well (jd_stream_partial_models).
static int trace_partial(jd_dec *d, int s, int *found)
{
    if (!d->d_partial_out) { int rc = dmalloc(d, &d->d_partial_out, 3); if (rc) return rc; }
    if (d->models && !d->d_partial_model) { int rc = dmalloc(d, &d->d_partial_model, (size_t)6 * d->res_cap); if (rc) return rc; }
    std::vector<int32_t> &L = d->partial_label[(size_t)s], &Tm = d->partial_time[(size_t)s];
    const int last_frame = Tm.empty() ? -1 : Tm.back();
    int *pm = d->models ? d->d_partial_model : nullptr;
    hipStream_t st = d->s_search;
    if (d->am->max_n <= 5)
        hipLaunchKernelGGL(k_partial<3>, dim3(1), dim3(1024), 0, st, d->C, d->d_ctl, d->d_streams, s, last_frame, d->d_partial_out, pm);
    else hipLaunchKernelGGL(k_partial<6>, dim3(1), dim3(1024), 0, st, d->C, d->d_ctl, d->d_streams, s, last_frame, d->d_partial_out, pm);
    HIPCHK(hipGetLastError());
    d->timing.trace_launches += 1;
    int ho[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(ho, d->d_partial_out, (pm ? 3 : 2) * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    d->last_trace[(size_t)s] = d->stream_T[(size_t)s] - 1;             // :867
    if (found) *found = ho[0];
    if (!ho[0]) return JD_OK;
    if (ho[1] > d->res_cap) return jd_fail(JD_ENOMEM, "stream %d: partial path has %d records (> %d)", s, ho[1], d->res_cap);
    if (pm && ho[2] > d->res_cap)
        return jd_fail(JD_ENOMEM, "stream %d: the model-level partial path has %d records (> %d, the result capacity)", s, ho[2], d->res_cap);
    // the chain from the root to the found record; the records traced before are its prefix
    L.resize((size_t)ho[1]); Tm.resize((size_t)ho[1]);
    const int *base = d->d_res + (size_t)s * 5 * d->res_cap;           // res_label, res_time: arrays 0 and 1 of the stream
    HIPCHK(hipMemcpy(L.data(), base, (size_t)ho[1] * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(Tm.data(), base + d->res_cap, (size_t)ho[1] * 4, hipMemcpyDeviceToHost));
    if (pm) {
        const size_t nm = (size_t)ho[2];
        std::vector<int32_t> h(6 * nm);
        if (nm)
            HIPCHK(hipMemcpy2D(h.data(), nm * 4, pm, (size_t)d->res_cap * 4, nm * 4, 6, hipMemcpyDeviceToHost));
        jd_dec::PartialModels &P = d->partial_m[(size_t)s];
        const float *f = (const float *)h.data();
        P.model.assign(h.begin(), h.begin() + nm); P.label.assign(h.begin() + nm, h.begin() + 2 * nm);
        P.time.assign(h.begin() + 2 * nm, h.begin() + 3 * nm);
        P.score.assign(f + 3 * nm, f + 4 * nm); P.ac.assign(f + 4 * nm, f + 5 * nm); P.lm.assign(f + 5 * nm, f + 6 * nm);
    }
    return JD_OK;
}

// trace_partial for a list of streams (each once; word level), each at the frame it has reached: ONE k_partial_many launch and ONE
// copy back - the {found, n} heads and, behind them, the records that are new to the host (k_partial_many, jd_gc.h).  found
// (or null): per entry.  A stream whose trace fails (a chain longer than the result capacity) does not keep the others from
// theirs; the first such error is returned.
static int trace_partial_many(jd_dec *d, const std::vector<int> &ss, int32_t *found)
{
    const int n = (int)ss.size();
    if (n == 0) return JD_OK;
    const size_t M = (size_t)d->max_streams, head_at = 4 * M, per = 2 + 2 * (size_t)PARTIAL_SHARE, words = head_at + per * M;
    if (!d->d_pmany) { int rc = dmalloc(d, &d->d_pmany, words); if (rc) return rc; }
    if (!d->h_pmany) HIPCHK(hipHostMalloc((void **)&d->h_pmany, words * sizeof(int)));
    int4 *hw = (int4 *)d->h_pmany;
    for (int i = 0; i < n; ++i) {
        const std::vector<int32_t> &L = d->partial_label[(size_t)ss[(size_t)i]], &Tm = d->partial_time[(size_t)ss[(size_t)i]];
        hw[i] = make_int4(ss[(size_t)i], Tm.empty() ? -1 : Tm.back(), (int)L.size(), 0);
    }
    hipStream_t st = d->s_search;
    int *d_out = d->d_pmany + head_at, *ho = d->h_pmany + head_at;
    HIPCHK(hipMemcpyAsync(d->d_pmany, hw, (size_t)n * sizeof(int4), hipMemcpyHostToDevice, st));
    if (d->am->max_n <= 5)
        hipLaunchKernelGGL(k_partial_many<3>, dim3((unsigned)n), dim3(1024), 0, st, d->C, d->d_ctl, d->d_streams, (const int4 *)d->d_pmany, n, d_out);
    else hipLaunchKernelGGL(k_partial_many<6>, dim3((unsigned)n), dim3(1024), 0, st, d->C, d->d_ctl, d->d_streams, (const int4 *)d->d_pmany, n, d_out);
    HIPCHK(hipGetLastError());
    d->timing.trace_launches += 1;
    HIPCHK(hipMemcpyAsync(ho, d_out, per * (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int rc_all = JD_OK;
    for (int i = 0; i < n; ++i) {
        const int s = ss[(size_t)i], fnd = ho[2 * i], len = ho[2 * i + 1];
        d->last_trace[(size_t)s] = d->stream_T[(size_t)s] - 1;        // :867
        if (found) found[i] = fnd;
        if (!fnd) continue;
        if (len > d->res_cap) {
            const int rc = jd_fail(JD_ENOMEM, "stream %d: partial path has %d records (> %d)", s, len, d->res_cap);
            if (!rc_all) rc_all = rc;
            continue;
        }
        std::vector<int32_t> &L = d->partial_label[(size_t)s], &Tm = d->partial_time[(size_t)s];
        const int have = (int)L.size();
        L.resize((size_t)len); Tm.resize((size_t)len);
        if (len - have <= PARTIAL_SHARE) {                             // (the records traced before are the chain's prefix)
            const int *stage = ho + 2 * (size_t)n + 2 * (size_t)PARTIAL_SHARE * i;
            for (int k = have; k < len; ++k) { L[(size_t)k] = stage[2 * (k - have)]; Tm[(size_t)k] = stage[2 * (k - have) + 1]; }
        } else {                                                       // more than its share of the staging area: from its result arrays
            const int *base = d->d_res + (size_t)s * 5 * d->res_cap;
            HIPCHK(hipMemcpy(L.data(), base, (size_t)len * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(Tm.data(), base + d->res_cap, (size_t)len * 4, hipMemcpyDeviceToHost));
        }
    }
    return rc_all;
}

extern "C" int jd_stream_push(jd_dec *d, int32_t s, const float *frames, int32_t n_frames)
{
    if (!d || s < 0 || s >= d->max_streams || n_frames < 0 || (n_frames > 0 && !frames))
        return jd_fail(JD_EINVAL, "jd_stream_push: bad argument");
    if (!d->stream_started[(size_t)s]) return jd_fail(JD_ESTATE, "jd_stream_push before jd_stream_init");
    int rc = check_device(d->device);
    if (rc) return rc;
    if (n_frames > 0) d->stream_open[(size_t)s] = 1;
    const int D = d->am->D, G = d->am->n_gmm, Fc = d->Fc;
    hipStream_t st = d->s_search;
    pf_discard(d);                                                     // (the streaming path scores into table 0)
    for (int done = 0, n = 0; done < n_frames; done += n) {
        n = std::min(Fc, n_frames - done);
        // PARTIAL_DECODING rides on the path collection (:362-368): a chunk ends at the frame rule's frame
        // (the first frame f with f - lastPathCollectFrame > 100)
        const int f_collect = d->last_collect[(size_t)s] + 101;
        if (d->partial_interval > 0) n = std::min(n, std::max(1, f_collect + 1 - d->stream_T[(size_t)s]));
        if ((size_t)n * D > d->push_cap) {
            if (d->d_push) (void)hipFree(d->d_push);
            HIPCHK(hipMalloc(&d->d_push, (size_t)Fc * D * sizeof(float)));
            d->push_cap = (size_t)Fc * D;
        }
        HIPCHK(hipMemcpyAsync(d->d_push, frames + (size_t)done * D, (size_t)n * D * sizeof(float),
                              hipMemcpyHostToDevice, st));
        std::vector<int> src((size_t)Fc, -1);
        for (int i = 0; i < n; ++i) src[(size_t)i] = i;
        if ((size_t)Fc > d->row_src_cap[0]) {
            if (d->d_row_src[0]) (void)hipFree(d->d_row_src[0]);
            d->d_row_src[0] = nullptr; d->row_src_cap[0] = 0;
            HIPCHK(hipMalloc(&d->d_row_src[0], (size_t)Fc * sizeof(int)));
            d->row_src_cap[0] = (size_t)Fc;
        }
        HIPCHK(hipMemcpyAsync(d->d_row_src[0], src.data(), (size_t)Fc * sizeof(int), hipMemcpyHostToDevice, st));
        const int f0 = d->stream_T[(size_t)s];
        const int Tnew = f0 + n;
        HIPCHK(hipMemcpyAsync(d->d_T + s, &Tnew, sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(jd_set_T_kernel, dim3(1), dim3(64), 0, st, d->d_ctl, s, 1, d->d_T + s);
        rc = launch_gmm(d->am, d->amb, d->d_push, d->d_row_src[0], n, d->d_ll[0], st);
        if (rc) return rc;
        if (d->partial_interval <= 0) {
            rc = launch_search(d, std::vector<int2>(1, make_int2(s, 0)), d->d_ll[0], (long long)Fc * G, f0, Tnew, st);
            if (rc) { d->stream_dirty[(size_t)s] = 1; return rc; }
            d->stream_T[(size_t)s] = Tnew;
            continue;
        }
        // PARTIAL_DECODING: collectPaths runs after a frame when the count rule fires (path_rule_fires, evaluated by
        // the kernel after every frame: the launch then stops, the collection runs and launch_search comes back) or
        // the frame rule does (the chunk ends there), and the trace rides on it (:362-368)
        for (;;) {
            d->return_on_collect = true; d->collected_now = false;
            rc = launch_search(d, std::vector<int2>(1, make_int2(s, 0)), d->d_ll[0], (long long)Fc * G, f0, Tnew, st);
            d->return_on_collect = false;
            if (rc) { d->stream_dirty[(size_t)s] = 1; return rc; }
            StreamCtl hc;
            HIPCHK(hipMemcpy(&hc, d->d_ctl + s, sizeof hc, hipMemcpyDeviceToHost));
            if (hc.error != 0) { d->stream_T[(size_t)s] = Tnew; d->stream_dirty[(size_t)s] = 1; break; }   // (reported by jd_stream_finish)
            const int at = hc.frame - 1;                               // the last frame processed
            // (with the reference's counts a collection that only the arena asked for is none of the reference's: it neither
            // counts nor carries a trace, and the launch goes on behind it)
            const bool ref = d->C.pcount != nullptr;
            bool collected = ref ? hc.n_collect > d->n_collect_host[(size_t)s] : d->collected_now;
            if (!collected && hc.frame >= Tnew && (at - d->last_collect[(size_t)s] > 100 ||
                                                   path_rule_fires(ref ? hc.n_paths_ref : hc.n_paths, ref ? hc.path_new_ref : hc.path_new))) {
                // the rule fires behind the chunk's last frame (the kernel looks before a frame, not after the last one)
                DecConst Cg = d->C;
                Cg.gc_threshold = -1;                                  // (every started stream collects)
                launch_gc(Cg, d->d_ctl, d->d_streams, nullptr, 1, s, d->am->max_n <= 5, d->n_cus, st);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(st));
                collected = true;
            }
            d->stream_T[(size_t)s] = hc.frame;
            if (collected) {
                d->last_collect[(size_t)s] = at;                       // :746
                d->n_collect_host[(size_t)s] += 1;
                if (at - d->last_trace[(size_t)s] > d->partial_interval) {
                    rc = trace_partial(d, s, nullptr);
                    if (rc) return rc;
                }
            }
            if (hc.frame >= Tnew) break;
        }
    }
    return JD_OK;
}

// jd_stream_push for SEVERAL streams at once: the frames of all of them are scored by ONE launch of the scoring
// kernel and searched by ONE persistent launch, every stream a cluster of its own - what a broker that serves
// many IDecoder instances (jd_broker_*, jd_broker.cpp) makes of the pushes that have arrived since its last tick.
// A call takes any number of frames per stream (the tables are sized for the call).  The streams may sit at
// different frames: row r of the common table is frame stream_T[s] + (r - first row of s) of stream s.
// PARTIAL_DECODING (jd_dec_set_partial_interval > 0): the rows are scored once and the streams advance in ROUNDS, in each of which
// every stream is served as jd_stream_push's loop serves its one - streams_push_rounds.

// The search of a jd_streams_push call under PARTIAL_DECODING.  work_all: {stream, likelihood slot} of the streams that brought
// frames, target: the frame each is to reach.  A round is ONE launch_search that comes back after a collection, one copy of the
// control blocks, at most one launch_gc (the streams whose frame or count rule fires behind their last frame of the round) and at
// most one k_partial_many launch (the streams that collected and whose trace is due); a stream's frame limit for the round is
// the frame rule's frame, so a round is to the stream what a chunk is to jd_stream_push.
static int streams_push_rounds(jd_dec *d, const std::vector<int2> &work_all, const std::vector<int> &target, hipStream_t st)
{
    const bool ne3 = d->am->max_n <= 5, ref = d->C.pcount != nullptr;
    const long long G = d->am->n_gmm;
    const size_t nw = work_all.size();
    std::vector<int> hT((size_t)d->max_streams), limit(nw, 0), gc_list, tr_list;
    std::vector<char> out(nw, 0);                                      // failed in this call: left out of the later rounds
    std::vector<size_t> act;
    std::vector<int2> work;
    std::vector<double> weight;
    std::vector<StreamCtl> hc;
    std::vector<int4> gw;
    for (;;) {
        act.clear(); work.clear(); weight.clear();
        int f_end = 0, s_lo = d->max_streams, s_hi = -1;
        for (int s = 0; s < d->max_streams; ++s) hT[(size_t)s] = d->stream_T[(size_t)s];
        for (size_t k = 0; k < nw; ++k) {
            const int s = work_all[k].x, at = d->stream_T[(size_t)s];
            if (out[k] || at >= target[k]) continue;
            // the chunk ends at the frame rule's frame: the first frame f with f - lastPathCollectFrame > 100
            limit[k] = std::min(target[k], std::max(at + 1, d->last_collect[(size_t)s] + 102));
            hT[(size_t)s] = limit[k];
            act.push_back(k); work.push_back(work_all[k]); weight.push_back((double)(limit[k] - at));
            f_end = std::max(f_end, limit[k]); s_lo = std::min(s_lo, s); s_hi = std::max(s_hi, s);
        }
        if (act.empty()) break;
        HIPCHK(hipMemcpyAsync(d->d_T, hT.data(), hT.size() * sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(jd_set_T_kernel, dim3((d->max_streams + 63) / 64), dim3(64), 0, st, d->d_ctl, 0, d->max_streams, d->d_T);
        HIPCHK(hipGetLastError());
        // (no re-planning cuts under way: a stream cut short stops at a frame of the launch's choosing, and a rule that fires behind
        // exactly that frame would go unseen - the kernel looks before every frame of a launch but its first, the host behind a
        // stream's last frame of the round only)
        const int rebalance = d->rebalance;
        d->rebalance = 0; d->return_on_collect = true; d->collected_now = false;
        int rc = launch_search(d, work, d->d_ll[0], G, 0, f_end, st, &weight);
        d->rebalance = rebalance; d->return_on_collect = false;
        if (rc) { (void)hipStreamSynchronize(st); for (const int2 &w : work) d->stream_dirty[(size_t)w.x] = 1; return rc; }
        hc.resize((size_t)(s_hi - s_lo + 1));
        HIPCHK(hipMemcpy(hc.data(), d->d_ctl + s_lo, hc.size() * sizeof(StreamCtl), hipMemcpyDeviceToHost));
        gc_list.clear(); tr_list.clear();
        std::vector<char> collected(act.size(), 0);
        for (size_t a = 0; a < act.size(); ++a) {
            const size_t k = act[a];
            const int s = work_all[k].x;
            const StreamCtl &c = hc[(size_t)(s - s_lo)];
            if (c.error != 0) { d->stream_T[(size_t)s] = target[k]; d->stream_dirty[(size_t)s] = 1; out[k] = 1; continue; }   // (reported by jd_stream_finish)
            const int at = c.frame - 1;                                // the last frame processed
            // whether a collection of the reference's ran on THIS stream: its own count (k_gc_remap counts the reference's
            // collections where the decoder keeps the reference's counts - one that only the arena asked for is none of
            // them and carries no trace - and every collection where it does not)
            collected[a] = c.n_collect > d->n_collect_host[(size_t)s];
            if (!collected[a] && c.frame >= limit[k] && (at - d->last_collect[(size_t)s] > 100 ||
                                                         path_rule_fires(ref ? c.n_paths_ref : c.n_paths, ref ? c.path_new_ref : c.path_new))) {
                gc_list.push_back(s);                                  // the rule fires behind the round's last frame
                collected[a] = 1;
            }
            d->stream_T[(size_t)s] = c.frame;
        }
        if (!gc_list.empty()) {
            rc = ensure_work_cap(d, (int)gc_list.size());
            if (rc) return rc;
            gw.clear();
            for (int s : gc_list) gw.push_back(make_int4(s, 0, 0, 0));
            HIPCHK(hipMemcpyAsync(d->d_work, gw.data(), gw.size() * sizeof(int4), hipMemcpyHostToDevice, st));
            DecConst Cg = d->C;
            Cg.gc_threshold = -1;                                      // (every listed stream collects)
            launch_gc(Cg, d->d_ctl, d->d_streams, d->d_work, (int)gw.size(), 0, ne3, d->n_cus, st);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
        }
        for (size_t a = 0; a < act.size(); ++a) {
            if (!collected[a]) continue;
            const int s = work_all[act[a]].x, at = d->stream_T[(size_t)s] - 1;
            d->last_collect[(size_t)s] = at;                           // :746
            d->n_collect_host[(size_t)s] += 1;
            if (at - d->last_trace[(size_t)s] > d->partial_interval) tr_list.push_back(s);
        }
        rc = trace_partial_many(d, tr_list, nullptr);
        if (rc) return rc;
    }
    return JD_OK;
}

extern "C" int jd_streams_push(jd_dec *d, int32_t n, const int32_t *streams, const float *const *frames, const int32_t *n_frames)
{
    if (!d || n < 0 || (n > 0 && (!streams || !frames || !n_frames))) return jd_fail(JD_EINVAL, "jd_streams_push: bad argument");
    int rc = check_device(d->device);
    if (rc) return rc;
    const int D = d->am->D, G = d->am->n_gmm;
    std::vector<char> seen((size_t)d->max_streams, 0);
    long long rows = 0;
    for (int i = 0; i < n; ++i) {
        const int s = streams[i];
        if (s < 0 || s >= d->max_streams || n_frames[i] < 0 || (n_frames[i] > 0 && !frames[i]) || seen[(size_t)s])
            return jd_fail(JD_EINVAL, "jd_streams_push: bad stream %d (each stream once)", s);
        if (!d->stream_started[(size_t)s]) return jd_fail(JD_ESTATE, "jd_streams_push before jd_stream_init (stream %d)", s);
        seen[(size_t)s] = 1;
        if (n_frames[i] > 0) d->stream_open[(size_t)s] = 1;
        rows += n_frames[i];
    }
    if (rows == 0) return JD_OK;
    if (rows > 0x7fffff00LL) return jd_fail(JD_EINVAL, "jd_streams_push: more than 2^31 frames in one call");
    hipStream_t st = d->s_search;
    pf_discard(d);                                                     // (the streaming path scores into table 0)
    const size_t tile_rows = ((size_t)rows + GMM_ROWS2 - 1) / GMM_ROWS2 * GMM_ROWS2;
    rc = ensure_table(d, 0, tile_rows * (size_t)G, tile_rows);
    if (rc) return rc;
    if ((size_t)rows * D > d->push_cap) {
        if (d->d_push) (void)hipFree(d->d_push);
        d->d_push = nullptr; d->push_cap = 0;
        HIPCHK(hipMalloc(&d->d_push, tile_rows * D * sizeof(float)));
        d->push_cap = tile_rows * D;
    }
    // rows: stream after stream, packed; row_src is the identity (the frames are packed the same way).  Everything the
    // launch needs from the host - frames, row table, frames available per stream - goes through ONE pinned staging
    // buffer: a tick of the broker is sixteen callers' frames, and sixteen copies from pageable memory were a tenth of it.
    const size_t need = (size_t)rows * D * sizeof(float) + tile_rows * sizeof(int) + (size_t)d->max_streams * sizeof(int);
    if (need > d->stage_cap) {
        if (d->h_stage) (void)hipHostFree(d->h_stage);
        d->h_stage = nullptr; d->stage_cap = 0;
        HIPCHK(hipHostMalloc((void **)&d->h_stage, need + need / 2));
        d->stage_cap = need + need / 2;
    }
    float *h_frames = (float *)d->h_stage;
    int *h_src = (int *)(d->h_stage + (size_t)rows * D * sizeof(float));
    int *h_T = h_src + tile_rows;
    std::vector<int> Tnew((size_t)n);
    std::vector<int2> work;
    std::vector<double> weight;
    size_t r0 = 0;
    int f_end = 0;
    for (int s = 0; s < d->max_streams; ++s) h_T[s] = d->stream_T[(size_t)s];     // (the other streams keep theirs)
    for (int i = 0; i < n; ++i) {
        if (n_frames[i] == 0) continue;
        const int s = streams[i];
        memcpy(h_frames + r0 * D, frames[i], (size_t)n_frames[i] * D * sizeof(float));
        Tnew[(size_t)i] = d->stream_T[(size_t)s] + n_frames[i];
        h_T[s] = Tnew[(size_t)i];
        // (k_search reads row  slot + (f - f0)  with f0 = 0: the slot is the stream's first row minus its first frame)
        work.push_back(make_int2(s, (int)((long long)r0 - d->stream_T[(size_t)s])));
        weight.push_back((double)n_frames[i]);
        f_end = std::max(f_end, Tnew[(size_t)i]);
        r0 += (size_t)n_frames[i];
    }
    for (size_t r = 0; r < tile_rows; ++r) h_src[r] = r < (size_t)rows ? (int)r : -1;
    HIPCHK(hipMemcpyAsync(d->d_push, h_frames, (size_t)rows * D * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d->d_row_src[0], h_src, tile_rows * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d->d_T, h_T, (size_t)d->max_streams * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(jd_set_T_kernel, dim3((d->max_streams + 63) / 64), dim3(64), 0, st, d->d_ctl, 0, d->max_streams, d->d_T);
    HIPCHK(hipGetLastError());
    rc = launch_gmm(d->am, d->amb, d->d_push, d->d_row_src[0], (int)rows, d->d_ll[0], st);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }             // (the staging buffer is the next call's too)
    if (d->partial_interval > 0) {
        std::vector<int> target;
        for (int i = 0; i < n; ++i) if (n_frames[i] > 0) target.push_back(Tnew[(size_t)i]);
        return streams_push_rounds(d, work, target, st);
    }
    rc = launch_search(d, work, d->d_ll[0], (long long)G, 0, f_end, st, &weight);
    if (rc) { (void)hipStreamSynchronize(st); for (const int2 &w : work) d->stream_dirty[(size_t)w.x] = 1; return rc; }
    for (int i = 0; i < n; ++i) if (n_frames[i] > 0) d->stream_T[(size_t)streams[i]] = Tnew[(size_t)i];
    return JD_OK;
}

// tracePartialPath now on each of the listed streams (jd_stream_partial with trace_now, for a list): one launch, one fetch
extern "C" int jd_streams_trace(jd_dec *d, int32_t n, const int32_t *streams, int32_t *found)
{
    if (!d || n < 0 || (n > 0 && !streams)) return jd_fail(JD_EINVAL, "jd_streams_trace: bad argument");
    if (d->models) return jd_fail(JD_ESTATE, "jd_streams_trace: word level only (model-level output: jd_stream_partial / jd_stream_partial_models)");
    std::vector<char> seen((size_t)d->max_streams, 0);
    std::vector<int> ss, at;
    for (int i = 0; i < n; ++i) {
        const int s = streams[i];
        if (s < 0 || s >= d->max_streams || seen[(size_t)s]) return jd_fail(JD_EINVAL, "jd_streams_trace: bad stream %d (each stream once)", s);
        if (!d->stream_started[(size_t)s]) return jd_fail(JD_ESTATE, "jd_streams_trace before jd_stream_init (stream %d)", s);
        seen[(size_t)s] = 1;
        if (found) found[i] = 0;
        if (d->stream_T[(size_t)s] > 0) { ss.push_back(s); at.push_back(i); }   // (nothing to trace before the first frame, as jd_stream_partial)
    }
    int rc = check_device(d->device);
    if (rc) return rc;
    std::vector<int32_t> fnd(ss.size(), 0);
    rc = trace_partial_many(d, ss, fnd.data());
    if (found) for (size_t k = 0; k < ss.size(); ++k) found[at[k]] = fnd[k];
    return rc;
}

extern "C" int jd_dec_get_partial_interval(const jd_dec *d, int32_t *interval)
{
    if (!d || !interval) return jd_fail(JD_EINVAL, "jd_dec_get_partial_interval: null argument");
    *interval = d->partial_interval;
    return JD_OK;
}


#include "jd_host_resident.h"

// collectPaths runs (WFSTDecoderLite.cpp:362) of stream s since its init, and the frame after which the last one ran
// (lastPathCollectFrame, :746; -1: none yet).  Counted while PARTIAL_DECODING is on (jd_dec_set_partial_interval > 0).
extern "C" int jd_stream_collect_info(jd_dec *d, int32_t s, int32_t *n_collections, int32_t *last_collect_frame)
{
    if (!d || s < 0 || s >= d->max_streams) return jd_fail(JD_EINVAL, "jd_stream_collect_info: bad argument");
    if (n_collections) *n_collections = d->n_collect_host[(size_t)s];
    if (last_collect_frame) *last_collect_frame = d->last_collect[(size_t)s];
    return JD_OK;
}

// setPartialDecodeOptions (WFSTDecoderLite.cpp:892-896; the reference reads PartialTraceInterval
// from the environment, :116-119)
// (the Path counts behind one arriving token, closure_path_counts: jd_prep.h)

// Diagnostics / tests (host only, no device): the per-state counts of closure_path_counts - what jd_dec_set_partial_interval puts
// on the device for collectPaths' count trigger - into out[n_states]; *acyclic = 0 when the label-less part of the graph has
// a cycle (the counts are then not used)
extern "C" int jd_debug_closure_path_counts(const jd_net *net, const jd_am *am, int32_t *out, int32_t *acyclic)
{
    if (!net || !am || !out || !acyclic) return jd_fail(JD_EINVAL, "jd_debug_closure_path_counts: null argument");
    if (net->lazy_dev) return jd_fail(JD_EINVAL, "jd_debug_closure_path_counts: not for a lazily composed network");
    std::vector<int> P;
    *acyclic = closure_path_counts(net, am, P) ? 1 : 0;
    for (int q = 0; q < net->n_states; ++q) out[q] = P[(size_t)q];
    return JD_OK;
}

extern "C" int jd_dec_set_partial_interval(jd_dec *d, int32_t interval)
{
    if (!d || interval < 0) return jd_fail(JD_EINVAL, "jd_dec_set_partial_interval: traceInterval >= 0");
    if (interval > 0 && d->models)
        return jd_fail(JD_EINVAL, "jd_dec_set_partial_interval: partial traces are not available with model-level output "
                       "(jd_stream_partial with trace_now is)");
    d->partial_interval = interval;
    d->C.path_rule = interval > 0 ? 1 : 0;             // (the kernel then watches collectPaths' count rule as well)
    d->C.pcount = nullptr;
    if (interval > 0 && !d->net->lazy_dev && d->C.end_win <= 0.0f && d->C.word_win <= 0.0f) {
        // ... on the reference's own counts where they are a static property of the graph
        if (!d->d_pcount) {
            int rc = check_device(d->device);
            if (rc) return rc;
            std::vector<int> P;
            if (closure_path_counts(d->net, d->am, P)) {
                if (!d->state_new.empty()) P = permute_by_state(d->state_new, P);   // (the kernels index it by the decoder's own state numbers)
                rc = dupload(d, &d->d_pcount, P.data(), P.size());
                if (rc) return rc;
            }
        }
        d->C.pcount = d->d_pcount;
    }
    return JD_OK;
}

// nPath and nPathNew of stream s as collectPaths' trigger reads them (WFSTDecoderLite.cpp:360): the reference's counts
// where this decoder keeps them (*exact = 1), else the records in this build's arena and what its last collection kept
extern "C" int jd_stream_path_counts(jd_dec *d, int32_t s, int32_t *n_path, int32_t *n_path_new, int32_t *exact)
{
    if (!d || s < 0 || s >= d->max_streams) return jd_fail(JD_EINVAL, "jd_stream_path_counts: bad argument");
    if (!d->stream_started[(size_t)s]) return jd_fail(JD_ESTATE, "jd_stream_path_counts before jd_stream_init");
    int rc = check_device(d->device);
    if (rc) return rc;
    StreamCtl hc;
    HIPCHK(hipMemcpy(&hc, d->d_ctl + s, sizeof hc, hipMemcpyDeviceToHost));
    const bool ref = d->C.pcount != nullptr;
    if (n_path) *n_path = ref ? hc.n_paths_ref : hc.n_paths;
    if (n_path_new) *n_path_new = ref ? hc.path_new_ref : hc.path_new;
    if (exact) *exact = ref ? 1 : 0;
    return JD_OK;
}

extern "C" int jd_stream_partial(jd_dec *d, int32_t s, int32_t trace_now, int32_t cap, int32_t *n, int32_t *labels,
                                 int32_t *times, int32_t *found)
{
    if (!d || s < 0 || s >= d->max_streams || cap < 0 || !n) return jd_fail(JD_EINVAL, "jd_stream_partial: bad argument");
    if (!d->stream_started[(size_t)s]) return jd_fail(JD_ESTATE, "jd_stream_partial before jd_stream_init");
    int rc = check_device(d->device);
    if (rc) return rc;
    int fnd = 0;
    if (trace_now && d->stream_T[(size_t)s] > 0) {
        rc = trace_partial(d, s, &fnd);
        if (rc) return rc;
    }
    const std::vector<int32_t> &L = d->partial_label[(size_t)s], &Tm = d->partial_time[(size_t)s];
    *n = (int32_t)L.size();
    for (int k = 0; k < std::min<int>(cap, *n); ++k) {
        if (labels) labels[k] = L[(size_t)k];
        if (times) times[k] = Tm[(size_t)k];
    }
    if (found) *found = fnd;
    return JD_OK;
}

extern "C" int jd_stream_partial_models(jd_dec *d, int32_t s, int32_t trace_now, int32_t cap, int32_t *n, int32_t *model,
                                        int32_t *label, int32_t *time, float *score, float *ac, float *lm, int32_t *found)
{
    if (!d || s < 0 || s >= d->max_streams || cap < 0 || !n) return jd_fail(JD_EINVAL, "jd_stream_partial_models: bad argument");
    if (!d->models) return jd_fail(JD_ESTATE, "jd_stream_partial_models: the decoder's output level is JD_OUTPUT_WORDS");
    if (!d->stream_started[(size_t)s]) return jd_fail(JD_ESTATE, "jd_stream_partial_models before jd_stream_init");
    int rc = check_device(d->device);
    if (rc) return rc;
    int fnd = 0;
    if (trace_now && d->stream_T[(size_t)s] > 0) {
        rc = trace_partial(d, s, &fnd);
        if (rc) return rc;
    }
    const jd_dec::PartialModels &P = d->partial_m[(size_t)s];
    *n = (int32_t)P.model.size();
    const size_t k = (size_t)std::min<int>(cap, *n);
    if (k) {
        if (model) memcpy(model, P.model.data(), k * 4);
        if (label) memcpy(label, P.label.data(), k * 4);
        if (time) memcpy(time, P.time.data(), k * 4);
        if (score) memcpy(score, P.score.data(), k * 4);
        if (ac) memcpy(ac, P.ac.data(), k * 4);
        if (lm) memcpy(lm, P.lm.data(), k * 4);
    }
    if (found) *found = fnd;
    return JD_OK;
}

extern "C" int jd_stream_finish(jd_dec *d, int32_t s, jd_hyp *out)
{
    if (!d || s < 0 || s >= d->max_streams || !out) return jd_fail(JD_EINVAL, "jd_stream_finish: bad argument");
    if (!d->stream_started[(size_t)s]) return jd_fail(JD_ESTATE, "jd_stream_finish before jd_stream_init");
    int rc = check_device(d->device);
    if (rc) return rc;
    if (d->stream_T[(size_t)s] == 0) {                                 // init() directly followed by finish(): recognitionStart only
        rc = launch_search(d, std::vector<int2>(1, make_int2(s, 0)), d->d_ll[0], 0, 0, 0, d->s_search);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(jd_finish_kernel, dim3(1), dim3(64), 0, d->s_search, d->d_ctl, d->d_streams, s, 1, res_model_of(d));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(d->s_search));
    // results of stream s are stored at result slot s
    std::vector<jd_hyp> tmp((size_t)d->max_streams);
    rc = fetch_results(d, s, 1, tmp.data(), s);
    *out = tmp[(size_t)s];
    d->stream_open[(size_t)s] = 0;
    if (d->lazy_in[(size_t)s]) { d->lazy_in[(size_t)s] = 0; jd_lazy_leave(d->net, 1); }   // the utterance has left the network
    if (d->partial_interval > 0 && out->n >= 0) {                      // :245-251 one more trace, from the best token
        std::vector<int32_t> &L = d->partial_label[(size_t)s], &Tm = d->partial_time[(size_t)s];
        L.resize((size_t)out->n); Tm.resize((size_t)out->n);
        for (int k = 0; k < out->n; ++k) { L[(size_t)k] = out->label[out->n - 1 - k]; Tm[(size_t)k] = out->time[out->n - 1 - k]; }
    }
    return rc;
}
