// jd_host_stream.h - the IDecoder seam of the C ABI (included by jd_device.hip): jd_stream_init / _push / _finish (IDecoder::init /
// processFrame / finish, src/Decoder.h:18-30, src/WFSTDecoderLite.cpp:139-372), jd_streams_push (several callers' frames in one launch),
// PARTIAL_DECODING (jd_dec_set_partial_interval, jd_stream_partial, jd_streams_trace: src/WFSTDecoderLite.cpp:822-896) for one stream
// and for a list of them (at model level: jd_streams_trace_models), the current best hypothesis of live streams (jd_streams_best; its
// decisions: jd_best.h), their end-of-utterance view (jd_streams_final; jd_final.h), and the collection bookkeeping.  What is
// DECIDED here - the stream's record, the argument checks, where a chunk or a round ends and what the control words behind a launch mean, the packing of a call, k_partial_many's layout - is jd_push.h
// (plain functions, tested on the CPU); this file makes the copies, launches and synchronisations between those steps.
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
    d->push[(size_t)s].init();
    return JD_OK;
}

// (JD_VERBOSE) "push:" lines: what jd_push.h's schedule was given -> what it returned (tests/test_gpu_push_inputs.py)
static bool push_verbose() { return getenv("JD_VERBOSE") != nullptr; }
// the control words of a stream that jd_push.h reads; ref: the decoder keeps the reference's counts
static PushCtl push_ctl(const StreamCtl &c, bool ref)
{
    return PushCtl{c.error, c.frame, c.n_collect, ref ? c.n_paths_ref : c.n_paths, ref ? c.path_new_ref : c.path_new};
}
static PushAfter push_after_launch(int s, const PushStream &P, const PushCtl &c, int limit, int fail_T, bool by_flag, bool flag, bool verbose)
{
    const PushAfter a = push_after(P, c, limit, fail_T, by_flag, flag);
    if (verbose)
        fprintf(stderr, "push: after stream %d error %d frame %d n_collect %d n_path %d n_path_new %d limit %d fail_T %d by_flag %d flag %d host_n_collect %d "
                "last_collect %d -> failed %d at %d collected %d host_collects %d T %d\n", s, c.error, c.frame, c.n_collect, c.n_path, c.n_path_new, limit, fail_T,
                (int)by_flag, (int)flag, P.n_collect, P.last_collect, (int)a.failed, a.at, (int)a.collected, (int)a.host_collects, a.T);
    return a;
}
static bool push_book(int s, PushStream &P, int at, int interval, bool verbose)
{
    const int last_trace = P.last_trace;
    const bool due = push_book_collection(P, at, interval);
    if (verbose)
        fprintf(stderr, "push: book stream %d at %d last_trace %d interval %d -> due %d last_collect %d n_collect %d\n", s, at, last_trace, interval, (int)due,
                P.last_collect, P.n_collect);
    return due;
}

// tracePartialPath (:824-868) on stream s at the frame it has reached; extends the stream's
// partialPaths when a converged record is found.  Model-level output: the same launch exports the whole chain below that
// record as well (jd_stream_partial_models).
static int trace_partial(jd_dec *d, int s, int *found)
{
    if (!d->d_partial_out) { int rc = dmalloc(d, &d->d_partial_out, 3); if (rc) return rc; }
    if (d->models && !d->d_partial_model) { int rc = dmalloc(d, &d->d_partial_model, (size_t)6 * d->res_cap); if (rc) return rc; }
    PushStream &S = d->push[(size_t)s];
    std::vector<int32_t> &L = S.partial_label, &Tm = S.partial_time;
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
    S.last_trace = S.T - 1;                                            // :867
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
        PushModels &P = S.partial_m;
        const float *f = (const float *)h.data();
        P.model.assign(h.begin(), h.begin() + nm); P.label.assign(h.begin() + nm, h.begin() + 2 * nm);
        P.time.assign(h.begin() + 2 * nm, h.begin() + 3 * nm);
        P.score.assign(f + 3 * nm, f + 4 * nm); P.ac.assign(f + 4 * nm, f + 5 * nm); P.lm.assign(f + 5 * nm, f + 6 * nm);
    }
    return JD_OK;
}

// trace_partial for a list of streams (each once; word level), each at the frame it has reached: ONE k_partial_many launch and ONE
// copy back - the {found, n} heads and, behind them, the records that are new to the host (k_partial_many, jd_gc.h; the layout and
// what a reply means: jd_push.h).  found (or null): per entry.  A stream whose trace fails (a chain longer than the result capacity)
// does not keep the others from theirs; the first such error is returned.
static_assert(sizeof(PartialRequest) == sizeof(int4), "k_partial_many's work list is int4");
static int trace_partial_many(jd_dec *d, const std::vector<int> &ss, int32_t *found)
{
    const int n = (int)ss.size();
    if (n == 0) return JD_OK;
    const PartialManyLayout Y = partial_many_layout(d->max_streams);
    if (!d->d_pmany) { int rc = dmalloc(d, &d->d_pmany, Y.words); if (rc) return rc; }
    if (!d->h_pmany) HIPCHK(hipHostMalloc((void **)&d->h_pmany, Y.words * sizeof(int)));
    PartialRequest *hw = (PartialRequest *)d->h_pmany;
    for (int i = 0; i < n; ++i) hw[i] = partial_many_request(d->push[(size_t)ss[(size_t)i]], ss[(size_t)i]);
    hipStream_t st = d->s_search;
    int *d_out = d->d_pmany + Y.head_at, *ho = d->h_pmany + Y.head_at;
    HIPCHK(hipMemcpyAsync(d->d_pmany, hw, (size_t)n * sizeof(int4), hipMemcpyHostToDevice, st));
    if (d->am->max_n <= 5)
        hipLaunchKernelGGL(k_partial_many<3>, dim3((unsigned)n), dim3(1024), 0, st, d->C, d->d_ctl, d->d_streams, (const int4 *)d->d_pmany, n, d_out);
    else hipLaunchKernelGGL(k_partial_many<6>, dim3((unsigned)n), dim3(1024), 0, st, d->C, d->d_ctl, d->d_streams, (const int4 *)d->d_pmany, n, d_out);
    HIPCHK(hipGetLastError());
    d->timing.trace_launches += 1;
    HIPCHK(hipMemcpyAsync(ho, d_out, Y.reply_words(n) * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int rc_all = JD_OK;
    for (int i = 0; i < n; ++i) {
        const int s = ss[(size_t)i], fnd = ho[2 * i], len = ho[2 * i + 1];
        PushStream &S = d->push[(size_t)s];
        S.last_trace = S.T - 1;                                        // :867
        if (found) found[i] = fnd;
        const int have = (int)S.partial_label.size();
        const PartialReply reply = partial_many_reply(fnd, len, have, d->res_cap);
        if (reply == PARTIAL_NOT_FOUND) continue;
        if (reply == PARTIAL_TOO_LONG) {
            const int rc = jd_fail(JD_ENOMEM, "stream %d: partial path has %d records (> %d)", s, len, d->res_cap);
            if (!rc_all) rc_all = rc;
            continue;
        }
        S.partial_label.resize((size_t)len); S.partial_time.resize((size_t)len);
        if (reply == PARTIAL_FROM_STAGE) partial_many_take(S, have, len, ho + partial_many_stage_at(n, i));
        else {
            const int *base = d->d_res + (size_t)s * 5 * d->res_cap;
            HIPCHK(hipMemcpy(S.partial_label.data(), base, (size_t)len * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(S.partial_time.data(), base + d->res_cap, (size_t)len * 4, hipMemcpyDeviceToHost));
        }
    }
    return rc_all;
}

// Score and search frames [row0, row0 + n_frames) of the host buffer `frames` on stream s, chunk by chunk: jd_stream_push's frames
// (row0 = 0, span null) or, for a spliced model, the rows that a push plan releases from its staging buffer (jd_splice.h: span is their
// common span there; a chunk sends up the piece of the buffer its windows read, splice_rows_window, and its rows' spans are that piece).
static int push_rows(jd_dec *d, int32_t s, const float *frames, int32_t row0, int32_t n_frames, const JdSpan *span)
{
    int rc = JD_OK;
    PushStream &P = d->push[(size_t)s];
    const int D = d->am->D, G = d->am->n_gmm, Fc = d->Fc;
    const int left = d->am->mlp_left, right = d->am->mlp_right;       // (0, 0 for every unspliced model)
    const bool verbose = push_verbose();
    hipStream_t st = d->s_search;
    pf_discard(d);                                                     // (the streaming path scores into table 0)
    for (int done = 0, n = 0; done < n_frames; done += n) {
        // PARTIAL_DECODING rides on the path collection (:362-368): a chunk ends at the frame rule's frame
        n = push_chunk_frames(Fc, n_frames - done, d->partial_interval, P.last_collect, P.T);
        if (verbose)
            fprintf(stderr, "push: chunk stream %d Fc %d left %d interval %d last_collect %d T %d -> n %d\n", s, Fc, n_frames - done, d->partial_interval,
                    P.last_collect, P.T, n);
        int b0 = row0 + done, b1 = b0 + n;                             // the frames that go up: the chunk's own, or its windows'
        if (span) splice_rows_window(left, right, *span, row0 + done, n, &b0, &b1);
        const int n_up = b1 - b0;
        if ((size_t)n_up * D > d->push_cap) { rc = dregrow(&d->d_push, &d->push_cap, (size_t)(Fc + left + right) * D, false); if (rc) return rc; }
        HIPCHK(hipMemcpyAsync(d->d_push, frames + (size_t)b0 * D, (size_t)n_up * D * sizeof(float),
                              hipMemcpyHostToDevice, st));
        std::vector<int> src((size_t)Fc, -1);
        for (int i = 0; i < n; ++i) src[(size_t)i] = row0 + done + i - b0;
        if ((size_t)Fc > d->row_src_cap[0]) { rc = dregrow(&d->d_row_src[0], &d->row_src_cap[0], (size_t)Fc, false); if (rc) return rc; }
        HIPCHK(hipMemcpyAsync(d->d_row_src[0], src.data(), (size_t)Fc * sizeof(int), hipMemcpyHostToDevice, st));
        if (span) {
            d->h_row_span[0].assign((size_t)Fc, JdSpan{0, n_up - 1});
            if ((size_t)Fc > d->row_span_cap[0]) { rc = dregrow(&d->d_row_span[0], &d->row_span_cap[0], (size_t)Fc, false); if (rc) return rc; }
            HIPCHK(hipMemcpyAsync(d->d_row_span[0], d->h_row_span[0].data(), (size_t)Fc * sizeof(JdSpan), hipMemcpyHostToDevice, st));
        }
        const int f0 = P.T;
        const int Tnew = f0 + n;
        HIPCHK(hipMemcpyAsync(d->d_T + s, &Tnew, sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(jd_set_T_kernel, dim3(1), dim3(64), 0, st, d->d_ctl, s, 1, d->d_T + s);
        rc = launch_gmm(d->am, d->amb, d->d_push, d->d_row_src[0], n, d->d_ll[0], st, 0, 0, -1, nullptr, 0, nullptr, span ? d->d_row_span[0] : nullptr);
        if (rc) return rc;
        if (d->partial_interval <= 0) {
            rc = launch_search(d, std::vector<int2>(1, make_int2(s, 0)), d->d_ll[0], (long long)Fc * G, f0, Tnew, st);
            if (rc) { d->stream_dirty[(size_t)s] = 1; return rc; }
            P.T = Tnew;
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
            // (with the reference's counts a collection that only the arena asked for is none of the reference's: it neither
            // counts nor carries a trace, and the launch goes on behind it - so the launch's own flag serves without them only)
            const bool ref = d->C.pcount != nullptr;
            const PushAfter a = push_after_launch(s, P, push_ctl(hc, ref), Tnew, Tnew, !ref, d->collected_now, verbose);
            if (a.failed) { P.T = a.T; d->stream_dirty[(size_t)s] = 1; break; }   // (reported by jd_stream_finish)
            if (a.host_collects) {
                // the rule fires behind the chunk's last frame (the kernel looks before a frame, not after the last one)
                DecConst Cg = d->C;
                Cg.gc_threshold = -1;                                  // (every started stream collects)
                launch_gc(Cg, d->d_ctl, d->d_streams, nullptr, 1, s, d->am->max_n <= 5, d->n_cus, st);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(st));
            }
            P.T = a.T;
            if (a.collected && push_book(s, P, a.at, d->partial_interval, verbose)) {
                rc = trace_partial(d, s, nullptr);
                if (rc) return rc;
            }
            if (a.T >= Tnew) break;
        }
    }
    return JD_OK;
}

// A push of a spliced model's stream (jd_splice.h: splice_push_plan): the kept frames go in front of the new ones, the rows the plan
// releases - none, perhaps - are scored and searched, and the stream keeps what a later window still reads.  finishing: jd_stream_finish's
// call, no new frames - the frames held back become rows with the right edge clamped.
static int push_spliced(jd_dec *d, int32_t s, const float *frames, int32_t n_frames, bool finishing)
{
    PushStream &P = d->push[(size_t)s];
    const size_t D = (size_t)d->am->D;
    const SplicePush plan = splice_push_plan(d->am->mlp_left, d->am->mlp_right, P.pushed, n_frames, finishing);
    std::vector<float> buf((size_t)plan.n_buf * D);
    memcpy(buf.data(), P.held.data() + (P.held.size() - (size_t)plan.n_front * D), (size_t)plan.n_front * D * sizeof(float));
    if (n_frames > 0) memcpy(buf.data() + (size_t)plan.n_front * D, frames, (size_t)n_frames * D * sizeof(float));
    const int rc = plan.n_rows > 0 ? push_rows(d, s, buf.data(), plan.row_buf, plan.n_rows, &plan.span) : JD_OK;
    // (on a failure the stream is dirty and jd_stream_finish reports it: the record still says what was pushed)
    P.pushed += n_frames;
    P.held.assign(buf.end() - (ptrdiff_t)((size_t)plan.n_keep * D), buf.end());
    return rc;
}

extern "C" int jd_stream_push(jd_dec *d, int32_t s, const float *frames, int32_t n_frames)
{
    const PushCheck chk = push_check_one(d ? &d->push : nullptr, s, frames != nullptr, n_frames);
    if (chk.verdict == PUSH_ARG_NOT_STARTED) return jd_fail(JD_ESTATE, "jd_stream_push before jd_stream_init");
    if (chk.verdict != PUSH_ARG_OK) return jd_fail(JD_EINVAL, "jd_stream_push: bad argument");
    const int rc = check_device(d->device);
    if (rc) return rc;
    if (n_frames > 0) d->push[(size_t)s].open = 1;
    if (d->am->mlp_spliced) return n_frames > 0 ? push_spliced(d, s, frames, n_frames, false) : JD_OK;
    return push_rows(d, s, frames, 0, n_frames, nullptr);
}

extern "C" int jd_stream_held_frames(jd_dec *d, int32_t s, int32_t *held)
{
    if (!d || s < 0 || s >= d->max_streams || !held) return jd_fail(JD_EINVAL, "jd_stream_held_frames: bad argument");
    const PushStream &P = d->push[(size_t)s];
    *held = (d->am->mlp_spliced && P.started) ? P.pushed - P.T : 0;
    return JD_OK;
}

// jd_stream_push for SEVERAL streams at once: the frames of all of them are scored by ONE launch of the scoring
// kernel and searched by ONE persistent launch, every stream a cluster of its own - what a broker that serves
// many IDecoder instances (jd_broker_*, jd_broker.cpp) makes of the pushes that have arrived since its last tick.
// A call takes any number of frames per stream (the tables are sized for the call).  The streams may sit at
// different frames: row r of the common table is frame T + (r - first row of s) of stream s (push_pack).
// PARTIAL_DECODING (jd_dec_set_partial_interval > 0): the rows are scored once and the streams advance in ROUNDS, in each of which
// every stream is served as jd_stream_push's loop serves its one - streams_push_rounds.

// The search of a jd_streams_push call under PARTIAL_DECODING.  work_all: {stream, likelihood slot} of the streams that brought
// frames, target: the frame each is to reach.  A round is ONE launch_search that comes back after a collection, one copy of the
// control blocks, at most one launch_gc (the streams whose frame or count rule fires behind their last frame of the round) and at
// most one k_partial_many launch (the streams that collected and whose trace is due); a stream's frame limit for the round is
// the frame rule's frame, so a round is to the stream what a chunk is to jd_stream_push (push_round_plan, push_after).
static int streams_push_rounds(jd_dec *d, const std::vector<int2> &work_all, const std::vector<int> &target, hipStream_t st)
{
    const bool ne3 = d->am->max_n <= 5, ref = d->C.pcount != nullptr, verbose = push_verbose();
    const long long G = d->am->n_gmm;
    const size_t nw = work_all.size();
    std::vector<int> ws(nw), gc_list, tr_list;
    for (size_t k = 0; k < nw; ++k) ws[k] = work_all[k].x;
    std::vector<char> out(nw, 0);                                      // failed in this call: left out of the later rounds
    PushRound R;
    std::vector<int2> work;
    std::vector<StreamCtl> hc;
    std::vector<PushAfter> after;
    std::vector<int4> gw;
    for (;;) {
        push_round_plan(d->push, ws, target, out, &R);
        if (verbose)
            fprintf(stderr, "push: round T %s last_collect %s work %s target %s out %s -> act %s limit %s hT %s f_end %d s_lo %d s_hi %d\n",
                    pipe_list(d->max_streams, [&](int s) { return d->push[(size_t)s].T; }).c_str(),
                    pipe_list(d->max_streams, [&](int s) { return d->push[(size_t)s].last_collect; }).c_str(), pipe_list((int)nw, [&](int k) { return ws[(size_t)k]; }).c_str(),
                    pipe_list((int)nw, [&](int k) { return target[(size_t)k]; }).c_str(), pipe_list((int)nw, [&](int k) { return out[(size_t)k]; }).c_str(),
                    pipe_list((int)R.act.size(), [&](int a) { return R.act[(size_t)a]; }).c_str(),
                    pipe_list((int)R.act.size(), [&](int a) { return R.limit[R.act[(size_t)a]]; }).c_str(),
                    pipe_list(d->max_streams, [&](int s) { return R.hT[(size_t)s]; }).c_str(), R.f_end, R.s_lo, R.s_hi);
        if (R.act.empty()) break;
        work.clear();
        for (size_t k : R.act) work.push_back(work_all[k]);
        HIPCHK(hipMemcpyAsync(d->d_T, R.hT.data(), R.hT.size() * sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(jd_set_T_kernel, dim3((d->max_streams + 63) / 64), dim3(64), 0, st, d->d_ctl, 0, d->max_streams, d->d_T);
        HIPCHK(hipGetLastError());
        // (no re-planning cuts under way: a stream cut short stops at a frame of the launch's choosing, and a rule that fires behind
        // exactly that frame would go unseen - the kernel looks before every frame of a launch but its first, the host behind a
        // stream's last frame of the round only)
        const int rebalance = d->rebalance;
        d->rebalance = 0; d->return_on_collect = true; d->collected_now = false;
        int rc = launch_search(d, work, d->d_ll[0], G, 0, R.f_end, st, &R.weight);
        d->rebalance = rebalance; d->return_on_collect = false;
        if (rc) { (void)hipStreamSynchronize(st); for (const int2 &w : work) d->stream_dirty[(size_t)w.x] = 1; return rc; }
        hc.resize((size_t)(R.s_hi - R.s_lo + 1));
        HIPCHK(hipMemcpy(hc.data(), d->d_ctl + R.s_lo, hc.size() * sizeof(StreamCtl), hipMemcpyDeviceToHost));
        gc_list.clear(); tr_list.clear(); after.clear();
        for (size_t k : R.act) {
            const int s = ws[k];
            PushStream &P = d->push[(size_t)s];
            // whether a collection of the reference's ran on THIS stream: its own count, never the launch's flag
            const PushAfter a = push_after_launch(s, P, push_ctl(hc[(size_t)(s - R.s_lo)], ref), R.limit[k], target[k], false, false, verbose);
            after.push_back(a);
            P.T = a.T;
            if (a.failed) { d->stream_dirty[(size_t)s] = 1; out[k] = 1; }   // (reported by jd_stream_finish)
            else if (a.host_collects) gc_list.push_back(s);            // the rule fires behind the round's last frame
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
        for (size_t a = 0; a < R.act.size(); ++a) {
            const int s = ws[R.act[a]];
            if (after[a].collected && push_book(s, d->push[(size_t)s], after[a].at, d->partial_interval, verbose)) tr_list.push_back(s);
        }
        rc = trace_partial_many(d, tr_list, nullptr);
        if (rc) return rc;
    }
    return JD_OK;
}

extern "C" int jd_streams_push(jd_dec *d, int32_t n, const int32_t *streams, const float *const *frames, const int32_t *n_frames)
{
    if (push_check_call(d != nullptr, n, streams && frames && n_frames).verdict != PUSH_ARG_OK) return jd_fail(JD_EINVAL, "jd_streams_push: bad argument");
    int rc = check_device(d->device);
    if (rc) return rc;
    const int D = d->am->D, G = d->am->n_gmm;
    long long rows = 0;
    const PushCheck chk = push_check_entries(d->push, n, streams, frames, n_frames, &rows);
    if (chk.verdict == PUSH_ARG_BAD_STREAM) return jd_fail(JD_EINVAL, "jd_streams_push: bad stream %d (each stream once)", chk.stream);
    if (chk.verdict == PUSH_ARG_NOT_STARTED) return jd_fail(JD_ESTATE, "jd_streams_push before jd_stream_init (stream %d)", chk.stream);
    if (rows == 0) return JD_OK;
    if (d->am->mlp_spliced)
        return jd_fail(JD_EINVAL, "jd_streams_push: this decoder's models are spliced (jd_am_mlp_splice), and splicing is served one stream at a time: jd_stream_push");
    if (chk.verdict == PUSH_ARG_TOO_MANY_ROWS) return jd_fail(JD_EINVAL, "jd_streams_push: more than 2^31 frames in one call");
    hipStream_t st = d->s_search;
    pf_discard(d);                                                     // (the streaming path scores into table 0)
    // rows: stream after stream, packed; row_src is the identity (the frames are packed the same way).  Everything the
    // launch needs from the host - frames, row table, frames available per stream - goes through ONE pinned staging
    // buffer: a tick of the broker is sixteen callers' frames, and sixteen copies from pageable memory were a tenth of it.
    PushPack K;
    push_pack(d->push, n, streams, n_frames, rows, D, GMM_ROWS2, &K);
    rc = ensure_table(d, 0, K.tile_rows * (size_t)G, K.tile_rows);
    if (rc) return rc;
    if ((size_t)rows * D > d->push_cap) { rc = dregrow(&d->d_push, &d->push_cap, K.tile_rows * D, false); if (rc) return rc; }
    if (K.need > d->stage_cap) { rc = dregrow(&d->h_stage, &d->stage_cap, push_grown(K.need), true); if (rc) return rc; }
    float *h_frames = (float *)d->h_stage;
    int *h_src = (int *)(d->h_stage + K.src_at), *h_T = (int *)(d->h_stage + K.T_at);
    std::vector<int2> work;
    for (size_t w = 0; w < K.work.size(); ++w) {
        memcpy(h_frames + K.row0[w] * D, frames[K.entry[w]], (size_t)n_frames[K.entry[w]] * D * sizeof(float));
        work.push_back(make_int2(K.work[w].stream, K.work[w].slot));
    }
    push_pack_fill(d->push, K, h_src, h_T);
    HIPCHK(hipMemcpyAsync(d->d_push, h_frames, (size_t)rows * D * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d->d_row_src[0], h_src, K.tile_rows * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d->d_T, h_T, (size_t)d->max_streams * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(jd_set_T_kernel, dim3((d->max_streams + 63) / 64), dim3(64), 0, st, d->d_ctl, 0, d->max_streams, d->d_T);
    HIPCHK(hipGetLastError());
    rc = launch_gmm(d->am, d->amb, d->d_push, d->d_row_src[0], (int)rows, d->d_ll[0], st);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }             // (the staging buffer is the next call's too)
    if (d->partial_interval > 0) return streams_push_rounds(d, work, K.target, st);
    rc = launch_search(d, work, d->d_ll[0], (long long)G, 0, K.f_end, st, &K.weight);
    if (rc) { (void)hipStreamSynchronize(st); for (const int2 &w : work) d->stream_dirty[(size_t)w.x] = 1; return rc; }
    for (size_t w = 0; w < K.work.size(); ++w) d->push[(size_t)K.work[w].stream].T = K.target[w];
    return JD_OK;
}

// tracePartialPath now on each of the listed streams (jd_stream_partial with trace_now, for a list): one launch, one fetch
extern "C" int jd_streams_trace(jd_dec *d, int32_t n, const int32_t *streams, int32_t *found)
{
    if (push_check_call(d != nullptr, n, streams != nullptr).verdict != PUSH_ARG_OK) return jd_fail(JD_EINVAL, "jd_streams_trace: bad argument");
    if (d->models) return jd_fail(JD_ESTATE, "jd_streams_trace: word level only (model-level output: jd_stream_partial / jd_stream_partial_models)");
    std::vector<int> ss, at;
    const PushCheck chk = push_check_trace(d->push, n, streams, found, &ss, &at);
    if (chk.verdict == PUSH_ARG_BAD_STREAM) return jd_fail(JD_EINVAL, "jd_streams_trace: bad stream %d (each stream once)", chk.stream);
    if (chk.verdict == PUSH_ARG_NOT_STARTED) return jd_fail(JD_ESTATE, "jd_streams_trace before jd_stream_init (stream %d)", chk.stream);
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

// The current best hypothesis of each listed stream at the frame it has reached (k_best_many, jd_gc.h; the layout and what a reply
// means: jd_best.h): ONE launch, one workgroup per stream that has a frame, and ONE copy back - the heads and, behind them, the chains
// that fit a staging share; a longer chain is fetched from the stream's result arrays.  The chains stay with the streams' records
// (PushStream::best) for jd_stream_best_words / _models.  A chain longer than the result capacity fails its stream's entry alone; the
// first such error is returned.
static_assert(sizeof(BestRequest) == sizeof(int4), "k_best_many's work list is int4");
static_assert(sizeof(jd_best) == sizeof(BestHead) && offsetof(jd_best, score) == offsetof(BestHead, score), "jd_best is BestHead");
static int best_many(jd_dec *d, const std::vector<int> &ss, const std::vector<int> &at, jd_best *out)
{
    const int n = (int)ss.size();
    if (n == 0) return JD_OK;
    const BestLayout Y = best_layout(d->max_streams);
    if (!d->d_best) { int rc = dmalloc(d, &d->d_best, Y.words); if (rc) return rc; }
    if (!d->h_best) HIPCHK(hipHostMalloc((void **)&d->h_best, Y.words * sizeof(int)));
    BestRequest *hw = (BestRequest *)d->h_best;
    for (int i = 0; i < n; ++i) hw[i] = best_request(ss[(size_t)i]);
    hipStream_t st = d->s_search;
    int *d_out = d->d_best + Y.head_at, *ho = d->h_best + Y.head_at;
    HIPCHK(hipMemcpyAsync(d->d_best, hw, (size_t)n * sizeof(int4), hipMemcpyHostToDevice, st));
    if (d->am->max_n <= 5)
        hipLaunchKernelGGL(k_best_many<3>, dim3((unsigned)n), dim3(1024), 0, st, d->C, d->d_ctl, d->d_streams, (const int4 *)d->d_best, n, d_out, res_model_of(d));
    else
        hipLaunchKernelGGL(k_best_many<6>, dim3((unsigned)n), dim3(1024), 0, st, d->C, d->d_ctl, d->d_streams, (const int4 *)d->d_best, n, d_out, res_model_of(d));
    HIPCHK(hipGetLastError());
    d->best_launches += 1;
    HIPCHK(hipMemcpyAsync(ho, d_out, Y.reply_words(n) * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    d->best_copies += 1;
    int rc_all = JD_OK;
    std::vector<int32_t> rows, mrow;
    for (int i = 0; i < n; ++i) {
        const int s = ss[(size_t)i];
        PushStream &S = d->push[(size_t)s];
        BestHead h;
        memcpy(&h, ho + (size_t)BEST_HEAD * i, sizeof h);
        h.frame = S.T;
        const BestReply reply = best_reply(h.found, h.n_records, d->res_cap);
        if (reply == BEST_NOT_FOUND || reply == BEST_TOO_LONG) {
            best_clear(S.best);
            if (reply == BEST_TOO_LONG) {
                const int rc = jd_fail(JD_ENOMEM, "stream %d: the best hypothesis has %d records (> %d, the result capacity)", s, h.n_records, d->res_cap);
                if (!rc_all) rc_all = rc;
            }
            h = best_none(S.T);
        } else if (reply == BEST_FROM_STAGE) best_take_stage(S.best, h.n_records, ho + BEST_STAGE_AT(n, i));
        else {
            const size_t nr = (size_t)h.n_records;
            rows.resize(5 * nr);
            HIPCHK(hipMemcpy2D(rows.data(), nr * 4, d->d_res + (size_t)s * 5 * d->res_cap, (size_t)d->res_cap * 4, nr * 4, 5, hipMemcpyDeviceToHost));
            d->best_copies += 1;
            if (d->models) {
                mrow.resize(nr);
                HIPCHK(hipMemcpy(mrow.data(), d->d_res_model + (size_t)s * d->res_cap, nr * 4, hipMemcpyDeviceToHost));
                d->best_copies += 1;
            }
            best_take_rows(S.best, h.n_records, rows.data(), d->models ? mrow.data() : nullptr);
        }
        memcpy(&out[at[(size_t)i]], &h, sizeof h);
    }
    return rc_all;
}

extern "C" int jd_streams_best(jd_dec *d, int32_t n, const int32_t *streams, jd_best *out)
{
    if (push_check_call(d != nullptr, n, streams && out).verdict != PUSH_ARG_OK) return jd_fail(JD_EINVAL, "jd_streams_best: bad argument");
    if (d->res && d->res->on && !d->pipe_on) return jd_fail(JD_ESTATE, "jd_streams_best: a broker drives this decoder's resident kernel");
    std::vector<int> ss, at;
    const BestCheck chk = best_check(d->push, n, streams, &ss, &at);
    if (chk.verdict == BEST_ARG_BAD_STREAM) return jd_fail(JD_EINVAL, "jd_streams_best: bad stream %d (each stream once)", chk.stream);
    if (chk.verdict == BEST_ARG_NOT_STARTED) return jd_fail(JD_ESTATE, "jd_streams_best before jd_stream_init (stream %d)", chk.stream);
    if (chk.verdict == BEST_ARG_RESIDENT) return jd_fail(JD_ESTATE, "jd_streams_best: stream %d is a broker's (its utterance runs on the resident kernel)", chk.stream);
    int rc = check_device(d->device);
    if (rc) return rc;
    // (a stream without a frame has nothing to look at: not found, its list empty)
    for (int i = 0; i < n; ++i) {
        PushStream &S = d->push[(size_t)streams[i]];
        if (S.T > 0) continue;
        best_clear(S.best);
        const BestHead h = best_none(S.T);
        memcpy(&out[i], &h, sizeof h);
    }
    return best_many(d, ss, at, out);
}

extern "C" int jd_stream_best_words(jd_dec *d, int32_t s, int32_t cap, int32_t *n, int32_t *label, int32_t *time, float *score, float *ac, float *lm)
{
    if (!d || s < 0 || s >= d->max_streams || cap < 0 || !n) return jd_fail(JD_EINVAL, "jd_stream_best_words: bad argument");
    if (!d->push[(size_t)s].started) return jd_fail(JD_ESTATE, "jd_stream_best_words before jd_stream_init");
    best_words(d->push[(size_t)s].best, cap, n, label, time, score, ac, lm);
    return JD_OK;
}

extern "C" int jd_stream_best_models(jd_dec *d, int32_t s, int32_t cap, int32_t *n, int32_t *model, int32_t *label, int32_t *time, float *score,
                                     float *ac, float *lm)
{
    if (!d || s < 0 || s >= d->max_streams || cap < 0 || !n) return jd_fail(JD_EINVAL, "jd_stream_best_models: bad argument");
    if (!d->models) return jd_fail(JD_ESTATE, "jd_stream_best_models: the decoder's output level is JD_OUTPUT_WORDS");
    if (!d->push[(size_t)s].started) return jd_fail(JD_ESTATE, "jd_stream_best_models before jd_stream_init");
    best_models(d->push[(size_t)s].best, cap, n, model, label, time, score, ac, lm);
    return JD_OK;
}

// the k_best_many launches and the device-to-host copies the jd_streams_best calls of this decoder have made
extern "C" int jd_dec_best_stats(const jd_dec *d, int64_t *launches, int64_t *copies)
{
    if (!d) return jd_fail(JD_EINVAL, "jd_dec_best_stats: null decoder");
    if (launches) *launches = d->best_launches;
    if (copies) *copies = d->best_copies;
    return JD_OK;
}

// The end-of-utterance view of each listed stream at the frame it has reached (k_final_many, jd_gc.h; the layout and what a reply
// means: jd_final.h): what jd_stream_finish would return now, read without finishing.  ONE launch, one workgroup per stream that has a
// frame, and ONE copy back - the heads and, behind them, the chains that fit a staging share; a longer chain is fetched from the
// stream's result arrays.  The chains stay with the streams' records (PushStream::fin) for jd_stream_final_words / _models.  A chain
// longer than the result capacity fails its stream's entry alone; the first such error is returned.
static_assert(sizeof(FinalRequest) == sizeof(int4), "k_final_many's work list is int4");
static_assert(sizeof(jd_final) == sizeof(FinalHead) && offsetof(jd_final, score) == offsetof(FinalHead, score), "jd_final is FinalHead");
static int final_many(jd_dec *d, const std::vector<int> &ss, const std::vector<int> &at, jd_final *out)
{
    const int n = (int)ss.size();
    if (n == 0) return JD_OK;
    const FinalLayout Y = final_layout(d->max_streams);
    if (!d->d_final) { int rc = dmalloc(d, &d->d_final, Y.words); if (rc) return rc; }
    if (!d->h_final) HIPCHK(hipHostMalloc((void **)&d->h_final, Y.words * sizeof(int)));
    FinalRequest *hw = (FinalRequest *)d->h_final;
    for (int i = 0; i < n; ++i) hw[i] = final_request(ss[(size_t)i]);
    hipStream_t st = d->s_search;
    int *d_out = d->d_final + Y.head_at, *ho = d->h_final + Y.head_at;
    HIPCHK(hipMemcpyAsync(d->d_final, hw, (size_t)n * sizeof(int4), hipMemcpyHostToDevice, st));
    if (d->models)
        hipLaunchKernelGGL(k_final_many<true>, dim3((unsigned)n), dim3(FINAL_THREADS), 0, st, d->d_ctl, d->d_streams, (const int4 *)d->d_final, n, d_out, d->d_res_model);
    else
        hipLaunchKernelGGL(k_final_many<false>, dim3((unsigned)n), dim3(FINAL_THREADS), 0, st, d->d_ctl, d->d_streams, (const int4 *)d->d_final, n, d_out, (int *)nullptr);
    HIPCHK(hipGetLastError());
    d->final_launches += 1;
    HIPCHK(hipMemcpyAsync(ho, d_out, Y.reply_words(n) * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    d->final_copies += 1;
    int rc_all = JD_OK;
    std::vector<int32_t> rows, mrow;
    for (int i = 0; i < n; ++i) {
        const int s = ss[(size_t)i];
        PushStream &S = d->push[(size_t)s];
        FinalHead h;
        memcpy(&h, ho + (size_t)FINAL_HEAD * i, sizeof h);
        h.frame = S.T;
        const FinalReply reply = final_reply(h.found, h.n_records, d->res_cap);
        if (reply == FINAL_NOT_FOUND || reply == FINAL_TOO_LONG) {
            best_clear(S.fin);
            if (reply == FINAL_TOO_LONG) {
                const int rc = jd_fail(JD_ENOMEM, "stream %d: the final hypothesis has %d records (> %d, the result capacity)", s, h.n_records, d->res_cap);
                if (!rc_all) rc_all = rc;
            }
            h = final_none(S.T);
        } else if (reply == FINAL_FROM_STAGE) final_take_stage(S.fin, h.n_records, ho + FINAL_STAGE_AT(n, i));
        else {
            const size_t nr = (size_t)h.n_records;
            rows.resize(5 * nr);
            HIPCHK(hipMemcpy2D(rows.data(), nr * 4, d->d_res + (size_t)s * 5 * d->res_cap, (size_t)d->res_cap * 4, nr * 4, 5, hipMemcpyDeviceToHost));
            d->final_copies += 1;
            if (d->models) {
                mrow.resize(nr);
                HIPCHK(hipMemcpy(mrow.data(), d->d_res_model + (size_t)s * d->res_cap, nr * 4, hipMemcpyDeviceToHost));
                d->final_copies += 1;
            }
            final_take_rows(S.fin, h.n_records, rows.data(), d->models ? mrow.data() : nullptr);
        }
        S.fin_tot[0] = h.score; S.fin_tot[1] = h.ac; S.fin_tot[2] = h.lm;
        memcpy(&out[at[(size_t)i]], &h, sizeof h);
    }
    return rc_all;
}

extern "C" int jd_streams_final(jd_dec *d, int32_t n, const int32_t *streams, jd_final *out)
{
    if (push_check_call(d != nullptr, n, streams && out).verdict != PUSH_ARG_OK) return jd_fail(JD_EINVAL, "jd_streams_final: bad argument");
    if (d->res && d->res->on && !d->pipe_on) return jd_fail(JD_ESTATE, "jd_streams_final: a broker drives this decoder's resident kernel");
    std::vector<int> ss, at;
    const BestCheck chk = final_check(d->push, n, streams, &ss, &at);
    if (chk.verdict == BEST_ARG_BAD_STREAM) return jd_fail(JD_EINVAL, "jd_streams_final: bad stream %d (each stream once)", chk.stream);
    if (chk.verdict == BEST_ARG_NOT_STARTED) return jd_fail(JD_ESTATE, "jd_streams_final before jd_stream_init (stream %d)", chk.stream);
    if (chk.verdict == BEST_ARG_RESIDENT) return jd_fail(JD_ESTATE, "jd_streams_final: stream %d is a broker's (its utterance runs on the resident kernel)", chk.stream);
    int rc = check_device(d->device);
    if (rc) return rc;
    // (a stream without a frame has nothing behind it: not found, its list empty)
    for (int i = 0; i < n; ++i) {
        PushStream &S = d->push[(size_t)streams[i]];
        if (S.T > 0) continue;
        best_clear(S.fin);
        S.fin_tot[0] = S.fin_tot[1] = S.fin_tot[2] = 0.0f;
        const FinalHead h = final_none(S.T);
        memcpy(&out[i], &h, sizeof h);
    }
    return final_many(d, ss, at, out);
}

extern "C" int jd_stream_final_words(jd_dec *d, int32_t s, int32_t cap, int32_t *n, int32_t *label, int32_t *time, float *score, float *ac, float *lm)
{
    if (!d || s < 0 || s >= d->max_streams || cap < 0 || !n) return jd_fail(JD_EINVAL, "jd_stream_final_words: bad argument");
    const PushStream &S = d->push[(size_t)s];
    if (!S.started) return jd_fail(JD_ESTATE, "jd_stream_final_words before jd_stream_init");
    final_words(S.fin, S.fin_tot, cap, n, label, time, score, ac, lm);
    return JD_OK;
}

extern "C" int jd_stream_final_models(jd_dec *d, int32_t s, int32_t cap, int32_t *n, int32_t *model, int32_t *label, int32_t *time, float *score,
                                      float *ac, float *lm)
{
    if (!d || s < 0 || s >= d->max_streams || cap < 0 || !n) return jd_fail(JD_EINVAL, "jd_stream_final_models: bad argument");
    if (!d->models) return jd_fail(JD_ESTATE, "jd_stream_final_models: the decoder's output level is JD_OUTPUT_WORDS");
    if (!d->push[(size_t)s].started) return jd_fail(JD_ESTATE, "jd_stream_final_models before jd_stream_init");
    final_models(d->push[(size_t)s].fin, cap, n, model, label, time, score, ac, lm);
    return JD_OK;
}

// the k_final_many launches and the device-to-host copies the jd_streams_final calls of this decoder have made
extern "C" int jd_dec_final_stats(const jd_dec *d, int64_t *launches, int64_t *copies)
{
    if (!d) return jd_fail(JD_EINVAL, "jd_dec_final_stats: null decoder");
    if (launches) *launches = d->final_launches;
    if (copies) *copies = d->final_copies;
    return JD_OK;
}

// trace_partial for a list of streams (each once) of a MODEL-level decoder, each at the frame it has reached: ONE
// k_partial_many_models launch and ONE copy back - the {found, n, nm} heads and, behind them, the words and model records that are
// new to the host (jd_gc.h; the layout and what a reply means: jd_push.h).  Both lists of a stream are updated, as trace_partial
// updates both.  A stream whose trace fails (a list longer than the result capacity) does not keep the others from theirs; the first
// such error is returned.
static_assert(sizeof(PartialModelsRequest) == sizeof(int4), "k_partial_many_models' work list is int4");
static int trace_partial_many_models(jd_dec *d, const std::vector<int> &ss, int32_t *found)
{
    const int n = (int)ss.size();
    if (n == 0) return JD_OK;
    const PartialModelsLayout Y = partial_models_layout(d->max_streams);
    if (!d->d_pmm) { int rc = dmalloc(d, &d->d_pmm, Y.words); if (rc) return rc; }
    if (!d->d_pmm_area) { int rc = dmalloc(d, &d->d_pmm_area, partial_models_area_words(d->max_streams, d->res_cap)); if (rc) return rc; }
    if (!d->h_pmm) HIPCHK(hipHostMalloc((void **)&d->h_pmm, Y.words * sizeof(int)));
    PartialModelsRequest *hw = (PartialModelsRequest *)d->h_pmm;
    for (int i = 0; i < n; ++i) hw[i] = partial_models_request(d->push[(size_t)ss[(size_t)i]], ss[(size_t)i]);
    hipStream_t st = d->s_search;
    int *d_out = d->d_pmm + Y.head_at, *ho = d->h_pmm + Y.head_at;
    HIPCHK(hipMemcpyAsync(d->d_pmm, hw, (size_t)n * sizeof(int4), hipMemcpyHostToDevice, st));
    if (d->am->max_n <= 5)
        hipLaunchKernelGGL(k_partial_many_models<3>, dim3((unsigned)n), dim3(1024), 0, st, d->C, d->d_ctl, d->d_streams, (const int4 *)d->d_pmm, n, d_out, d->d_pmm_area);
    else
        hipLaunchKernelGGL(k_partial_many_models<6>, dim3((unsigned)n), dim3(1024), 0, st, d->C, d->d_ctl, d->d_streams, (const int4 *)d->d_pmm, n, d_out, d->d_pmm_area);
    HIPCHK(hipGetLastError());
    d->timing.trace_launches += 1;
    HIPCHK(hipMemcpyAsync(ho, d_out, Y.reply_words(n) * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int rc_all = JD_OK;
    std::vector<int32_t> words, rows;
    for (int i = 0; i < n; ++i) {
        const int s = ss[(size_t)i];
        const int *h = ho + (size_t)PM_HEAD * i;
        const int fnd = h[0], len = h[1], nm = h[2];
        PushStream &S = d->push[(size_t)s];
        S.last_trace = S.T - 1;                                        // :867
        if (found) found[i] = fnd;
        const int have = (int)S.partial_label.size(), have_m = (int)S.partial_m.model.size();
        const PartialModelsReply reply = partial_models_reply(fnd, len, nm, have, have_m, d->res_cap);
        if (reply == PARTIAL_M_NOT_FOUND) continue;
        if (reply == PARTIAL_M_TOO_LONG) {
            const int rc = len > d->res_cap ? jd_fail(JD_ENOMEM, "stream %d: partial path has %d records (> %d)", s, len, d->res_cap)
                                            : jd_fail(JD_ENOMEM, "stream %d: the model-level partial path has %d records (> %d, the result capacity)", s, nm, d->res_cap);
            if (!rc_all) rc_all = rc;
            continue;
        }
        if (reply == PARTIAL_M_FROM_STAGE) { partial_models_take(S, have, len, have_m, nm, ho + PM_STAGE_AT(n, i)); continue; }
        words.resize(2 * (size_t)len); rows.resize((size_t)PM_FIELDS * (size_t)nm);
        HIPCHK(hipMemcpy2D(words.data(), (size_t)len * 4, d->d_res + (size_t)s * 5 * d->res_cap, (size_t)d->res_cap * 4, (size_t)len * 4, 2, hipMemcpyDeviceToHost));
        if (nm)
            HIPCHK(hipMemcpy2D(rows.data(), (size_t)nm * 4, d->d_pmm_area + (size_t)s * PM_FIELDS * d->res_cap, (size_t)d->res_cap * 4, (size_t)nm * 4, PM_FIELDS,
                               hipMemcpyDeviceToHost));
        partial_models_take_arrays(S, len, words.data(), nm, rows.data());
    }
    return rc_all;
}

// tracePartialPath now on each of the listed streams of a model-level decoder (jd_stream_partial_models with trace_now, for a list):
// one launch, one fetch.  Explicit traces only: the interval stays refused at model level.
extern "C" int jd_streams_trace_models(jd_dec *d, int32_t n, const int32_t *streams, int32_t *found)
{
    if (push_check_call(d != nullptr, n, streams != nullptr).verdict != PUSH_ARG_OK) return jd_fail(JD_EINVAL, "jd_streams_trace_models: bad argument");
    if (!d->models) return jd_fail(JD_ESTATE, "jd_streams_trace_models: the decoder's output level is JD_OUTPUT_WORDS (word level: jd_streams_trace)");
    std::vector<int> ss, at;
    const PushCheck chk = push_check_trace(d->push, n, streams, found, &ss, &at);
    if (chk.verdict == PUSH_ARG_BAD_STREAM) return jd_fail(JD_EINVAL, "jd_streams_trace_models: bad stream %d (each stream once)", chk.stream);
    if (chk.verdict == PUSH_ARG_NOT_STARTED) return jd_fail(JD_ESTATE, "jd_streams_trace_models before jd_stream_init (stream %d)", chk.stream);
    int rc = check_device(d->device);
    if (rc) return rc;
    std::vector<int32_t> fnd(ss.size(), 0);
    rc = trace_partial_many_models(d, ss, fnd.data());
    if (found) for (size_t k = 0; k < ss.size(); ++k) found[at[k]] = fnd[k];
    return rc;
}

// collectPaths runs (WFSTDecoderLite.cpp:362) of stream s since its init, and the frame after which the last one ran
// (lastPathCollectFrame, :746; -1: none yet).  Counted while PARTIAL_DECODING is on (jd_dec_set_partial_interval > 0).
extern "C" int jd_stream_collect_info(jd_dec *d, int32_t s, int32_t *n_collections, int32_t *last_collect_frame)
{
    if (!d || s < 0 || s >= d->max_streams) return jd_fail(JD_EINVAL, "jd_stream_collect_info: bad argument");
    if (n_collections) *n_collections = d->push[(size_t)s].n_collect;
    if (last_collect_frame) *last_collect_frame = d->push[(size_t)s].last_collect;
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
    if (!d->push[(size_t)s].started) return jd_fail(JD_ESTATE, "jd_stream_path_counts before jd_stream_init");
    int rc = check_device(d->device);
    if (rc) return rc;
    StreamCtl hc;
    HIPCHK(hipMemcpy(&hc, d->d_ctl + s, sizeof hc, hipMemcpyDeviceToHost));
    const bool ref = d->C.pcount != nullptr;
    const PushCtl c = push_ctl(hc, ref);
    if (n_path) *n_path = c.n_path;
    if (n_path_new) *n_path_new = c.n_path_new;
    if (exact) *exact = ref ? 1 : 0;
    return JD_OK;
}

extern "C" int jd_stream_partial(jd_dec *d, int32_t s, int32_t trace_now, int32_t cap, int32_t *n, int32_t *labels,
                                 int32_t *times, int32_t *found)
{
    if (!d || s < 0 || s >= d->max_streams || cap < 0 || !n) return jd_fail(JD_EINVAL, "jd_stream_partial: bad argument");
    const PushStream &S = d->push[(size_t)s];
    if (!S.started) return jd_fail(JD_ESTATE, "jd_stream_partial before jd_stream_init");
    int rc = check_device(d->device);
    if (rc) return rc;
    int fnd = 0;
    if (trace_now && S.T > 0) {
        rc = trace_partial(d, s, &fnd);
        if (rc) return rc;
    }
    const std::vector<int32_t> &L = S.partial_label, &Tm = S.partial_time;
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
    if (!d->push[(size_t)s].started) return jd_fail(JD_ESTATE, "jd_stream_partial_models before jd_stream_init");
    int rc = check_device(d->device);
    if (rc) return rc;
    int fnd = 0;
    if (trace_now && d->push[(size_t)s].T > 0) {
        rc = trace_partial(d, s, &fnd);
        if (rc) return rc;
    }
    const PushModels &P = d->push[(size_t)s].partial_m;
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
    if (!d->push[(size_t)s].started) return jd_fail(JD_ESTATE, "jd_stream_finish before jd_stream_init");
    int rc = check_device(d->device);
    if (rc) return rc;
    if (d->am->mlp_spliced && d->push[(size_t)s].pushed > d->push[(size_t)s].T && !d->stream_dirty[(size_t)s]) {
        rc = push_spliced(d, s, nullptr, 0, true);                     // the frames held back: rows now, the right edge clamped
        if (rc) return rc;
    }
    if (d->push[(size_t)s].T == 0) {                                   // init() directly followed by finish(): recognitionStart only
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
    if (d->lazy_in[(size_t)s]) { d->lazy_in[(size_t)s] = 0; jd_lazy_leave(d->net, 1); }   // the utterance has left the network
    d->push[(size_t)s].finish(d->partial_interval > 0, out->n, out->label, out->time);     // :245-251 one more trace, from the best token
    return rc;
}
