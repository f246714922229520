// jd_host_paths.h - jd_debug_paths (included by jd_device.hip): the Path collection (launch_gc), the PARTIAL_DECODING trace (k_partial,
// k_partial_many, k_partial_many_models) and the end-of-utterance view (k_final_many) of jd_gc.h on a state the CALLER describes - Path
// arenas, instance records, frontier items, dirty lists, arrival keys, a tiny graph - instead of one a search left behind.  No decoder, network or model: the description (jd_paths.h, plain words, validated
// before any device call) is laid out exactly as the kernels expect it, uploaded, the listed operations run through the production
// launches, and the state afterwards comes back.  No kernel of its own.  tests/test_gpu_paths.py holds what comes back to
// tests/paths_ref.py, word for word (the two live views: tests/test_gpu_paths_live.py, tests/paths_live_ref.py).
#pragma once

#include <string>

#include "jd_paths.h"

static_assert(PD_MAXW == MAXW && PD_TOT_N == TOT_N && PD_TOT_REC0 == TOT_REC0 && PD_TOT_DIRTY0 == TOT_DIRTY0 && PD_SHARE == PARTIAL_SHARE, "jd_paths.h: the kernels' constants");
static_assert(PD_FINAL_HEAD == FINAL_HEAD && PD_FINAL_SHARE == FINAL_SHARE && FINAL_FIELDS == 6 && PD_PM_HEAD == PM_HEAD && PD_PM_SHARE == PM_SHARE && PM_FIELDS == 6, "jd_paths.h: the live views' constants");
static_assert(PD_GC_WORDS * 4 == sizeof(GcState) && sizeof(PathRec) == 32 && sizeof(JdArc) == 16 && GC_MAXG == 32, "jd_paths.h: the kernels' structs");
static_assert(RecLayout<3>::HF == 2 && RecLayout<6>::HF == 3 && RecLayout<3>::CHUNK_BYTES == 5 * 1024 && RecLayout<6>::CHUNK_BYTES == 9 * 1024, "jd_paths.h: RecLayout");

// what one call holds on the device; freed when the call is over, however it ends
struct PathsDev {
    std::vector<void *> allocs;
    ~PathsDev() { for (void *p : allocs) (void)hipFree(p); }
    template <typename T> int upload(T **p, const void *src, size_t bytes)
    {
        void *q = nullptr;
        HIPCHK(hipMalloc(&q, std::max<size_t>(bytes, 256)));
        allocs.push_back(q);
        if (src && bytes) HIPCHK(hipMemcpy(q, src, bytes, hipMemcpyHostToDevice));
        else HIPCHK(hipMemset(q, 0, std::max<size_t>(bytes, 256)));
        *p = (T *)q;
        return JD_OK;
    }
    // ... n words, each the sentinel
    int filled(int **p, size_t n, int32_t sentinel)
    {
        const std::vector<int32_t> h(std::max<size_t>(n, 1), sentinel);
        return upload(p, h.data(), h.size() * 4);
    }
};

extern "C" int jd_debug_paths(int32_t device, const int32_t *desc, int64_t n_desc, int32_t *out, int64_t out_cap, int64_t *n_out)
{
    if (!desc || n_desc < 0 || !n_out) return jd_fail(JD_EINVAL, "jd_debug_paths: bad argument");
    PdDesc D;
    std::string err;
    if (!pd_parse(desc, n_desc, &D, &err)) return jd_fail(JD_EINVAL, "jd_debug_paths: %s", err.c_str());
    *n_out = D.out_words;
    if (!out || out_cap < D.out_words) return jd_fail(JD_ENOMEM, "jd_debug_paths: %lld words come back, room for %lld", (long long)D.out_words, (long long)out_cap);
    int rc = check_device(device);
    if (rc) return rc;
    PathsDev dev;
    const bool ne3 = D.NE == 3;
    const int B = D.n_streams;

    DecConst C{};
    {
        std::vector<JdArc> arcs((size_t)std::max(D.n_arcs, 1), JdArc{0, 0.0f, 0, 0});
        for (int a = 0; a < D.n_arcs; ++a) arcs[(size_t)a].in = D.arc_in[a];
        int *d_row_ptr = nullptr; JdArc *d_arcs = nullptr; int *d_pcount = nullptr;
        if ((rc = dev.upload(&d_row_ptr, D.row_ptr, ((size_t)D.n_states + 1) * 4)) || (rc = dev.upload(&d_arcs, arcs.data(), arcs.size() * sizeof(JdArc)))) return rc;
        if (D.pcount && (rc = dev.upload(&d_pcount, nullptr, (size_t)D.n_states * 4))) return rc;      // (only its presence is read)
        C.row_ptr = d_row_ptr; C.arcs = d_arcs; C.pcount = d_pcount;
    }
    C.n_states = D.n_states; C.lazy = nullptr;
    C.cap_slots = (unsigned)D.cap_slots; C.cap_items = (unsigned)D.cap_items; C.cap_new = (unsigned)D.cap_new;
    C.srec_stride = 16u; C.srec_arr = 16u * (unsigned)D.n_states; C.srec_estride = 8u; C.srec_par = 8u * (unsigned)D.n_states;   // split8
    int cap_max = 1;

    std::vector<StreamCtl> h_ctl((size_t)B);
    std::vector<StreamDev> h_streams((size_t)B);
    for (int s = 0; s < B; ++s) {
        const PdStream &P = D.streams[(size_t)s];
        StreamCtl &c = h_ctl[(size_t)s];
        StreamDev &S = h_streams[(size_t)s];
        memset((void *)&c, 0, sizeof c);
        memset((void *)&S, 0, sizeof S);
        c.started = P.started; c.needs_init = P.needs_init; c.error = P.error; c.frame = P.frame; c.path_new = P.path_new; c.n_collect = P.n_collect;
        c.n_paths_ref = P.n_paths_ref; c.path_new_ref = P.path_new_ref; c.lst_nw = P.lst_nw; c.n_paths = P.n_paths;
        c.dirty_nw[(P.frame & 1) ^ 1] = P.dirty_nw; c.dirty_nw[P.frame & 1] = 0;
        c.best_final.score = 0.0f; c.best_final.path = P.best_final;
        cap_max = std::max(cap_max, P.cap_paths);
        std::vector<int32_t> img, img2;
        pd_image_rec(D, P, &img);
        if ((rc = dev.upload(&S.rec, img.data(), img.size() * 4))) return rc;
        pd_image_srec(D, P, &img);
        if ((rc = dev.upload(&S.srec, img.data(), img.size() * 4))) return rc;
        pd_image_items(D, P, &img);
        if ((rc = dev.upload(&S.items, img.data(), img.size() * 4))) return rc;
        pd_image_dirty(D, P, &img);
        if ((rc = dev.upload(&S.dirtyl, img.data(), img.size() * 4))) return rc;
        pd_image_counts(D, P, &img, &img2);
        if ((rc = dev.upload(&S.tot, img.data(), img.size() * 4)) || (rc = dev.upload(&S.item_end, img2.data(), img2.size() * 4))) return rc;
        pd_image_paths(P, &img);
        if ((rc = dev.upload(&S.paths, img.data(), img.size() * 4))) return rc;
        if ((rc = dev.upload(&S.paths2, nullptr, (size_t)P.cap_paths * sizeof(PathRec))) || (rc = dev.upload(&S.gc_idx, nullptr, (size_t)P.cap_paths * 4)) ||
            (rc = dev.upload(&S.gc_state, nullptr, sizeof(GcState))))
            return rc;
    }
    C.cap_paths = cap_max;
    StreamCtl *d_ctl = nullptr; StreamDev *d_streams = nullptr;
    if ((rc = dev.upload(&d_ctl, h_ctl.data(), h_ctl.size() * sizeof(StreamCtl))) || (rc = dev.upload(&d_streams, h_streams.data(), h_streams.size() * sizeof(StreamDev))))
        return rc;

    // the operations, one after the other on the null stream; a trace's result arrays are the operation's own, hung into the streams'
    // records (read back first: a collection has swapped the arenas there)
    struct TraceOut { int *d = nullptr; size_t words = 0; };
    std::vector<TraceOut> traces;
    for (const PdOp &O : D.ops) {
        if (O.kind == PD_COLLECT) {
            int4 *d_work = nullptr;
            if (O.n_work) {
                int4 hw[PD_MAX_STREAMS];
                for (int k = 0; k < O.n_work; ++k) hw[k] = make_int4(O.streams[k], 0, 0, 0);
                if ((rc = dev.upload(&d_work, hw, (size_t)O.n_work * sizeof(int4)))) return rc;
            }
            C.gc_threshold = O.gc_threshold; C.path_rule = O.path_rule;
            const int n_work = O.n_work ? O.n_work : 1;
            launch_gc(C, d_ctl, d_streams, d_work, n_work, O.streams[0], ne3, O.G * n_work, nullptr);
            HIPCHK(hipGetLastError());
            HIPCHK(hipDeviceSynchronize());
            continue;
        }
        const size_t cap = (size_t)O.res_cap;
        HIPCHK(hipMemcpy(h_streams.data(), d_streams, h_streams.size() * sizeof(StreamDev), hipMemcpyDeviceToHost));
        if (O.kind == PD_FINAL_MANY || O.kind == PD_TRACE_MANY_MODELS) {
            // [the kernel's reply buffer][per entry: the result arrays it uses][by STREAM: the model rows | the model lists]
            const bool fin = O.kind == PD_FINAL_MANY;
            const int n = O.n_work;
            const size_t reply = fin ? final_layout(n).reply_words(n) : partial_models_layout(n).reply_words(n), per_entry = (fin ? 5 : 2) * cap;
            TraceOut T;
            T.words = (size_t)(fin ? PdOp::final_words(n, B, O.res_cap) : PdOp::pm_words(n, B, O.res_cap));
            int *d_buf = nullptr;
            if ((rc = dev.filled(&d_buf, T.words, D.sentinel))) return rc;
            T.d = d_buf;
            int *by_stream = d_buf + reply + per_entry * (size_t)n;
            int4 hw[PD_MAX_STREAMS];
            for (int k = 0; k < n; ++k) {
                StreamDev &S = h_streams[(size_t)O.streams[k]];
                S.res_label = d_buf + reply + per_entry * (size_t)k; S.res_time = S.res_label + cap; S.res_cap = O.res_cap;
                if (fin) {
                    S.res_score = (float *)(S.res_time + cap); S.res_ac = S.res_score + cap; S.res_lm = S.res_ac + cap;
                    // the three floats of best_final; its path stays what the device holds (a collection may have remapped it)
                    StreamCtl c;
                    HIPCHK(hipMemcpy((void *)&c, d_ctl + O.streams[k], sizeof c, hipMemcpyDeviceToHost));
                    memcpy(&c.best_final.score, &O.final_tok[k][0], 4); memcpy(&c.best_final.ac, &O.final_tok[k][1], 4); memcpy(&c.best_final.lm, &O.final_tok[k][2], 4);
                    HIPCHK(hipMemcpy(d_ctl + O.streams[k], (const void *)&c, sizeof c, hipMemcpyHostToDevice));
                    hw[k] = make_int4(O.streams[k], 0, 0, 0);
                } else hw[k] = make_int4(O.streams[k], O.last_frame[k], O.have[k], O.have_m[k]);
            }
            HIPCHK(hipMemcpy(d_streams, h_streams.data(), h_streams.size() * sizeof(StreamDev), hipMemcpyHostToDevice));
            int4 *d_work = nullptr;
            if ((rc = dev.upload(&d_work, hw, (size_t)n * sizeof(int4)))) return rc;
            if (fin) {
                if (O.model_level) hipLaunchKernelGGL(k_final_many<true>, dim3((unsigned)n), dim3(FINAL_THREADS), 0, 0, d_ctl, d_streams, (const int4 *)d_work, n, d_buf, by_stream);
                else hipLaunchKernelGGL(k_final_many<false>, dim3((unsigned)n), dim3(FINAL_THREADS), 0, 0, d_ctl, d_streams, (const int4 *)d_work, n, d_buf, (int *)nullptr);
            } else if (ne3) hipLaunchKernelGGL(k_partial_many_models<3>, dim3((unsigned)n), dim3(1024), 0, 0, C, d_ctl, d_streams, (const int4 *)d_work, n, d_buf, by_stream);
            else hipLaunchKernelGGL(k_partial_many_models<6>, dim3((unsigned)n), dim3(1024), 0, 0, C, d_ctl, d_streams, (const int4 *)d_work, n, d_buf, by_stream);
            HIPCHK(hipGetLastError());
            HIPCHK(hipDeviceSynchronize());
            traces.push_back(T);
            continue;
        }
        // [out: 3 | PD_TRACE_MANY's buffer][per entry: res_label, res_time][pm: 6 res_cap]
        const size_t head = O.kind == PD_TRACE ? 3 : (size_t)(2 + 2 * PARTIAL_SHARE) * (size_t)O.n_work;
        TraceOut T;
        T.words = O.kind == PD_TRACE ? 3 + 8 * cap : head;
        int *d_buf = nullptr;
        if ((rc = dev.filled(&d_buf, head + 2 * cap * (size_t)O.n_work + 6 * cap, D.sentinel))) return rc;
        T.d = d_buf;
        for (int k = 0; k < O.n_work; ++k) {
            StreamDev &S = h_streams[(size_t)O.streams[k]];
            S.res_label = d_buf + head + 2 * cap * (size_t)k; S.res_time = S.res_label + cap; S.res_cap = O.res_cap;
        }
        HIPCHK(hipMemcpy(d_streams, h_streams.data(), h_streams.size() * sizeof(StreamDev), hipMemcpyHostToDevice));
        if (O.kind == PD_TRACE) {
            int *pm = O.model_level ? d_buf + head + 2 * cap : nullptr;
            if (ne3) hipLaunchKernelGGL(k_partial<3>, dim3(1), dim3(1024), 0, 0, C, d_ctl, d_streams, O.streams[0], O.last_frame[0], d_buf, pm);
            else hipLaunchKernelGGL(k_partial<6>, dim3(1), dim3(1024), 0, 0, C, d_ctl, d_streams, O.streams[0], O.last_frame[0], d_buf, pm);
        } else {
            int4 hw[PD_MAX_STREAMS];
            int4 *d_work = nullptr;
            for (int k = 0; k < O.n_work; ++k) hw[k] = make_int4(O.streams[k], O.last_frame[k], O.have[k], 0);
            if ((rc = dev.upload(&d_work, hw, (size_t)O.n_work * sizeof(int4)))) return rc;
            const int n = O.n_work;
            if (ne3) hipLaunchKernelGGL(k_partial_many<3>, dim3((unsigned)n), dim3(1024), 0, 0, C, d_ctl, d_streams, (const int4 *)d_work, n, d_buf);
            else hipLaunchKernelGGL(k_partial_many<6>, dim3((unsigned)n), dim3(1024), 0, 0, C, d_ctl, d_streams, (const int4 *)d_work, n, d_buf);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        traces.push_back(T);
    }

    // the state afterwards
    HIPCHK(hipMemcpy(h_streams.data(), d_streams, h_streams.size() * sizeof(StreamDev), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy((void *)h_ctl.data(), d_ctl, h_ctl.size() * sizeof(StreamCtl), hipMemcpyDeviceToHost));
    int32_t *o = out;
    for (int s = 0; s < B; ++s) {
        const PdStream &P = D.streams[(size_t)s];
        const StreamCtl &c = h_ctl[(size_t)s];
        const StreamDev &S = h_streams[(size_t)s];
        if (c.n_paths < 0 || c.n_paths > P.n_paths) return jd_fail(JD_ESTATE, "jd_debug_paths: stream %d comes back with %d Path records of %d", s, c.n_paths, P.n_paths);
        GcState gs;
        HIPCHK(hipMemcpy(&gs, S.gc_state, sizeof gs, hipMemcpyDeviceToHost));
        const int32_t head[PD_OUT_STREAM_WORDS] = {c.n_paths, c.path_new, c.n_collect, c.n_paths_ref, c.path_new_ref, c.best_final.path,
                                                   gs.active, gs.kept, gs.kept_ref, gs.by_rule};
        memcpy(o, head, sizeof head);
        o += PD_OUT_STREAM_WORDS;
        std::vector<int32_t> img((size_t)8 * (size_t)std::max(c.n_paths, 1));
        HIPCHK(hipMemcpy(img.data(), S.paths, (size_t)c.n_paths * sizeof(PathRec), hipMemcpyDeviceToHost));
        for (long long q = 0; q < c.n_paths; ++q)
            for (int k = 0; k < 7; ++k) *o++ = img[(size_t)(8 * q + k)];
        img.resize((size_t)(2LL * D.cap_slots * pd_rec_bytes(D.NE) / 4));
        HIPCHK(hipMemcpy(img.data(), S.rec, img.size() * 4, hipMemcpyDeviceToHost));
        pd_read_rec(D, P, img, o);
        o += P.n_inst_all * D.NE;
        img.resize((size_t)(16LL * D.cap_items));
        HIPCHK(hipMemcpy(img.data(), S.items, img.size() * 4, hipMemcpyDeviceToHost));
        pd_read_items(D, P, img, o);
        o += P.n_items_all;
    }
    for (const TraceOut &T : traces) {
        HIPCHK(hipMemcpy(o, T.d, T.words * 4, hipMemcpyDeviceToHost));
        o += T.words;
    }
    *n_out = (int64_t)(o - out);
    return JD_OK;
}
