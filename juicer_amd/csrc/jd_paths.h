// jd_paths.h - jd_debug_paths' description of a stream state as plain data (no HIP: compiled and tested on the CPU,
// tests/paths_driver.cpp, tests/test_paths_ref_cpu.py): the words of a description, their validation - nothing that passes it lets a
// kernel of jd_gc.h follow an index out of an arena - and the byte images of the lists exactly as the kernels read them.
// jd_host_paths.h allocates, uploads these images, runs launch_gc / k_partial / k_partial_many / k_final_many / k_partial_many_models on them and
// reads the state back.
//
// A description is a list of int32 words (floats as their bits):
//   desc   := PD_MAGIC NE n_streams n_ops cap_slots cap_items cap_new pcount sentinel
//             n_states row_ptr[n_states + 1] arc_in[row_ptr[n_states]]                  (arc in-labels with their ARC_FLAGS bits)
//             stream * n_streams   op * n_ops
//   stream := started needs_init error frame path_new n_collect n_paths_ref path_new_ref best_final_path lst_nw dirty_nw cap_paths n_paths
//             {prev frame label model score ac lm} * n_paths
//             arrival[n_states]                  the item (w * seg_item + k, of the last frame's parity) a state's arrival key names; -1: key 0
//             {n_inst {nStates source_state {score path} * (nStates - 2)} * n_inst} * waves            (waves = max(lst_nw, 0))
//             {n_items path * n_items} * waves                                                       (frontier items of the last frame)
//             {n_dirty state * n_dirty} * dirty_waves          (dirty_waves = lst_nw <= 0 ? 0 : dirty_nw > 0 ? dirty_nw : lst_nw)
//   op     := PD_COLLECT n_work stream * max(n_work, 1) G gc_threshold path_rule              (n_work 0: one stream, null work list)
//           | PD_TRACE stream last_frame res_cap model_level
//           | PD_TRACE_MANY n {stream last_frame have} * n res_cap
//           | PD_FINAL_MANY n {stream score ac lm} * n res_cap model_level      (k_final_many; the three floats of the stream's best_final are
//                                                                                 set first, its path is the stream's - as remapped by any
//                                                                                 earlier PD_COLLECT)
//           | PD_TRACE_MANY_MODELS n {stream last_frame have have_m} * n res_cap             (k_partial_many_models)
// and what comes back is
//   per stream: n_paths path_new n_collect n_paths_ref path_new_ref best_final_path active kept kept_ref by_rule
//               {prev frame label model score ac lm} * n_paths   path of every token slot [wave][instance][NE]   path of every item
//   per PD_TRACE: out[3] res_label[res_cap] res_time[res_cap] pm[6 res_cap]; per PD_TRACE_MANY: the 2 n + 2 PARTIAL_SHARE n words of its buffer
//   per PD_FINAL_MANY: the (PD_FINAL_HEAD + 6 PD_FINAL_SHARE) n words of its buffer, per entry res_label res_time res_score res_ac res_lm
//               [res_cap each], then the model rows [n_streams][res_cap] (written at model_level 1 only)
//   per PD_TRACE_MANY_MODELS: the (PD_PM_HEAD + 2 PD_SHARE + 6 PD_PM_SHARE) n words of its buffer, per entry res_label res_time [res_cap each],
//               then the streams' model lists [n_streams][6][res_cap]
// (all of a trace's or a look's words prefilled with the sentinel).
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#define PD_MAGIC 0x4a445031
enum { PD_COLLECT = 1, PD_TRACE = 2, PD_TRACE_MANY = 3, PD_FINAL_MANY = 4, PD_TRACE_MANY_MODELS = 5 };
// what the kernels' headers call these (jd_host_paths.h holds them to the kernels' own with static_asserts)
#define PD_MAXW 512
#define PD_TOT_N 10
#define PD_TOT_REC0 0
#define PD_TOT_DIRTY0 3
#define PD_SHARE 32
#define PD_FINAL_HEAD 8
#define PD_FINAL_SHARE 64
#define PD_PM_HEAD 4
#define PD_PM_SHARE 112
#define PD_GC_WORDS 68
#define PD_MAX_STREAMS 4
#define PD_MAX_PATHS (1 << 18)
#define PD_MAX_OPS 8
#define PD_MAX_CAP (1 << 21)          // records, items, dirty entries per stream
#define PD_MAX_RES_CAP (1 << 16)
#define PD_STREAM_WORDS 13
#define PD_OUT_STREAM_WORDS 10

struct PdStream {
    int started, needs_init, error, frame, path_new, n_collect, n_paths_ref, path_new_ref, best_final, lst_nw, dirty_nw, cap_paths, n_paths;
    const int32_t *paths = nullptr, *arrival = nullptr;
    int waves = 0, dirty_waves = 0;
    long long n_inst_all = 0, n_items_all = 0;
    std::vector<const int32_t *> rec, item, dirty;      // per wave: at its count word
};
struct PdOp {
    int kind = 0;
    int n_work = 0, streams[PD_MAX_STREAMS] = {0, 0, 0, 0}, G = 0, gc_threshold = 0, path_rule = 0;                       // PD_COLLECT
    int last_frame[PD_MAX_STREAMS] = {0, 0, 0, 0}, have[PD_MAX_STREAMS] = {0, 0, 0, 0}, res_cap = 0, model_level = 0;     // the traces
    int have_m[PD_MAX_STREAMS] = {0, 0, 0, 0};                                                                            // PD_TRACE_MANY_MODELS
    int32_t final_tok[PD_MAX_STREAMS][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};                                  // PD_FINAL_MANY: score, ac, lm (bits)
    // the words a look or a model trace of n entries brings back
    static long long final_words(int n, int n_streams, int res_cap) { return (PD_FINAL_HEAD + 6LL * PD_FINAL_SHARE) * n + 5LL * res_cap * n + (long long)n_streams * res_cap; }
    static long long pm_reply_words(int n) { return (PD_PM_HEAD + 2LL * PD_SHARE + 6LL * PD_PM_SHARE) * n; }
    static long long pm_words(int n, int n_streams, int res_cap) { return pm_reply_words(n) + 2LL * res_cap * n + 6LL * n_streams * res_cap; }
};
struct PdDesc {
    int NE = 0, n_streams = 0, n_ops = 0, cap_slots = 0, cap_items = 0, cap_new = 0, pcount = 0, sentinel = 0, n_states = 0, n_arcs = 0;
    const int32_t *row_ptr = nullptr, *arc_in = nullptr;
    std::vector<PdStream> streams;
    std::vector<PdOp> ops;
    long long out_words = 0;          // at most this many come back (a collection only shrinks an arena)
};

// make_geo's segment sizes
struct PdGeo { long long seg_rec, seg_item, seg_new; };
inline PdGeo pd_geo(const PdDesc &D, int nw)
{
    return PdGeo{(long long)(((unsigned)D.cap_slots / (unsigned)nw) & ~63u), (long long)((unsigned)D.cap_items / (unsigned)nw),
                 (long long)((unsigned)D.cap_new / (unsigned)nw)};
}
inline int pd_hf(int NE) { return NE == 3 ? 2 : 3; }                    // RecLayout<NE>::HF
inline long long pd_chunk_bytes(int NE) { return (long long)(pd_hf(NE) + NE) * 1024; }
inline long long pd_rec_bytes(int NE) { return (long long)(pd_hf(NE) + NE) * 16; }

struct PdReader {
    const int32_t *w; long long n, at = 0;
    bool take(int *v) { if (at >= n) return false; *v = w[at++]; return true; }
    const int32_t *span(long long k) { if (k < 0 || at + k > n) return nullptr; const int32_t *p = w + at; at += k; return p; }
};

inline bool pd_err(std::string *err, const char *fmt, long long a = 0, long long b = 0, long long c = 0)
{
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b, c);
    *err = buf;
    return false;
}

// One stream's words.  Everything a kernel will use as an index is held to its range here.
inline bool pd_parse_stream(PdReader &R, const PdDesc &D, int s, PdStream *S, std::string *err)
{
    const int32_t *h = R.span(PD_STREAM_WORDS);
    if (!h) return pd_err(err, "stream %lld: the description ends inside it", s);
    S->started = h[0]; S->needs_init = h[1]; S->error = h[2]; S->frame = h[3]; S->path_new = h[4]; S->n_collect = h[5];
    S->n_paths_ref = h[6]; S->path_new_ref = h[7]; S->best_final = h[8]; S->lst_nw = h[9]; S->dirty_nw = h[10]; S->cap_paths = h[11];
    S->n_paths = h[12];
    if (S->frame < 0) return pd_err(err, "stream %lld: frame %lld < 0", s, S->frame);
    if (S->cap_paths < 1 || S->cap_paths > PD_MAX_PATHS) return pd_err(err, "stream %lld: an arena of %lld records (1 .. %lld)", s, S->cap_paths, PD_MAX_PATHS);
    if (S->n_paths < 0 || S->n_paths > S->cap_paths) return pd_err(err, "stream %lld: n_paths %lld outside [0, %lld]", s, S->n_paths, S->cap_paths);
    if (S->lst_nw > PD_MAXW || S->dirty_nw < 0 || S->dirty_nw > PD_MAXW) return pd_err(err, "stream %lld: lst_nw %lld / dirty_nw %lld above MAXW", s, S->lst_nw, S->dirty_nw);
    if (S->path_new < 0 || S->n_collect < 0 || S->n_paths_ref < 0 || S->path_new_ref < 0) return pd_err(err, "stream %lld: a negative counter", s);
    if (S->best_final < -1 || S->best_final >= S->n_paths) return pd_err(err, "stream %lld: best_final.path %lld outside [-1, %lld)", s, S->best_final, S->n_paths);
    S->paths = R.span(7LL * S->n_paths);
    if (!S->paths) return pd_err(err, "stream %lld: the description ends inside the Path arena", s);
    for (int q = 0; q < S->n_paths; ++q)
        if (S->paths[7LL * q] < -1 || S->paths[7LL * q] >= q) return pd_err(err, "stream %lld: prev[%lld] = %lld outside [-1, q)", s, q, S->paths[7LL * q]);
    S->arrival = R.span(D.n_states);
    if (!S->arrival) return pd_err(err, "stream %lld: the description ends inside the arrival keys", s);
    S->waves = S->lst_nw > 0 ? S->lst_nw : 0;
    S->dirty_waves = S->lst_nw <= 0 ? 0 : S->dirty_nw > 0 ? S->dirty_nw : S->lst_nw;
    if (S->lst_nw <= 0 && S->dirty_nw != 0) return pd_err(err, "stream %lld: dirty_nw without writer waves", s);
    const PdGeo g = S->waves ? pd_geo(D, S->waves) : PdGeo{0, 0, 0}, gd = S->dirty_waves ? pd_geo(D, S->dirty_waves) : PdGeo{0, 0, 0};
    for (int w = 0; w < S->waves; ++w) {
        S->rec.push_back(R.w + R.at);
        int n_inst;
        if (!R.take(&n_inst)) return pd_err(err, "stream %lld: the description ends inside the instance records", s);
        if (n_inst < 0 || n_inst > g.seg_rec) return pd_err(err, "stream %lld wave %lld: %lld instances beyond the segment", s, w, n_inst);
        for (int q = 0; q < n_inst; ++q) {
            int n, src;
            if (!R.take(&n) || !R.take(&src)) return pd_err(err, "stream %lld: the description ends inside the instance records", s);
            if (n < 3 || n > D.NE + 2) return pd_err(err, "stream %lld wave %lld: nStates %lld outside [3, NE + 2]", s, w, n);
            if (src < 0 || src >= D.n_states) return pd_err(err, "stream %lld wave %lld: source state %lld outside the graph", s, w, src);
            const int32_t *t = R.span(2LL * (n - 2));
            if (!t) return pd_err(err, "stream %lld: the description ends inside the instance records", s);
            for (int j = 0; j < n - 2; ++j)
                if (t[2 * j + 1] < -1 || t[2 * j + 1] >= S->n_paths) return pd_err(err, "stream %lld wave %lld: a token's path %lld outside [-1, n_paths)", s, w, t[2 * j + 1]);
        }
        S->n_inst_all += n_inst;
    }
    for (int w = 0; w < S->waves; ++w) {
        S->item.push_back(R.w + R.at);
        int n_it;
        if (!R.take(&n_it)) return pd_err(err, "stream %lld: the description ends inside the items", s);
        if (n_it < 0 || n_it > g.seg_item) return pd_err(err, "stream %lld wave %lld: %lld items beyond the segment", s, w, n_it);
        const int32_t *t = R.span(n_it);
        if (!t) return pd_err(err, "stream %lld: the description ends inside the items", s);
        for (int k = 0; k < n_it; ++k)
            if (t[k] < -1 || t[k] >= S->n_paths) return pd_err(err, "stream %lld wave %lld: an item's path %lld outside [-1, n_paths)", s, w, t[k]);
        S->n_items_all += n_it;
    }
    for (int w = 0; w < S->dirty_waves; ++w) {
        S->dirty.push_back(R.w + R.at);
        int n_d;
        if (!R.take(&n_d)) return pd_err(err, "stream %lld: the description ends inside the dirty list", s);
        if (n_d < 0 || n_d > gd.seg_new) return pd_err(err, "stream %lld dirty wave %lld: %lld states beyond the segment", s, w, n_d);
        const int32_t *t = R.span(n_d);
        if (!t) return pd_err(err, "stream %lld: the description ends inside the dirty list", s);
        for (int k = 0; k < n_d; ++k)
            if (t[k] < 0 || t[k] >= D.n_states) return pd_err(err, "stream %lld dirty wave %lld: state %lld outside the graph", s, w, t[k]);
    }
    for (int st = 0; st < D.n_states; ++st) {
        const int a = S->arrival[st];
        if (a == -1) continue;
        bool ok = a >= 0 && S->waves > 0 && g.seg_item > 0;
        if (ok) { const long long w = a / g.seg_item, k = a % g.seg_item; ok = w < S->waves && k < S->item[(size_t)w][0]; }
        if (!ok) return pd_err(err, "stream %lld: the arrival key of state %lld names item %lld, which is not written", s, st, a);
    }
    return true;
}

inline bool pd_parse(const int32_t *w, long long n, PdDesc *D, std::string *err)
{
    PdReader R{w, n};
    const int32_t *h = R.span(10);
    if (!h || h[0] != PD_MAGIC) return pd_err(err, "not a description");
    D->NE = h[1]; D->n_streams = h[2]; D->n_ops = h[3]; D->cap_slots = h[4]; D->cap_items = h[5]; D->cap_new = h[6]; D->pcount = h[7];
    D->sentinel = h[8]; D->n_states = h[9];
    if (D->NE != 3 && D->NE != 6) return pd_err(err, "NE %lld (3 or 6)", D->NE);
    if (D->n_streams < 1 || D->n_streams > PD_MAX_STREAMS) return pd_err(err, "%lld streams (1 .. %lld)", D->n_streams, PD_MAX_STREAMS);
    if (D->n_ops < 0 || D->n_ops > PD_MAX_OPS) return pd_err(err, "%lld operations (0 .. %lld)", D->n_ops, PD_MAX_OPS);
    if (D->cap_slots < 64 || D->cap_slots % 64 || D->cap_slots > PD_MAX_CAP || D->cap_items < 1 || D->cap_items > PD_MAX_CAP || D->cap_new < 1 ||
        D->cap_new > PD_MAX_CAP)
        return pd_err(err, "capacities %lld / %lld / %lld (records: a multiple of 64; all in [1, 2^21])", D->cap_slots, D->cap_items, D->cap_new);
    if (D->pcount != 0 && D->pcount != 1) return pd_err(err, "pcount %lld (0 or 1)", D->pcount);
    if (D->n_states < 1 || D->n_states > 4096) return pd_err(err, "%lld states (1 .. 4096)", D->n_states);
    D->row_ptr = R.span((long long)D->n_states + 1);
    if (!D->row_ptr || D->row_ptr[0] != 0) return pd_err(err, "row_ptr: missing, or row_ptr[0] != 0");
    for (int q = 0; q < D->n_states; ++q)
        if (D->row_ptr[q + 1] < D->row_ptr[q] || D->row_ptr[q + 1] > 65536) return pd_err(err, "row_ptr[%lld] decreases or exceeds 65536", q + 1);
    D->n_arcs = D->row_ptr[D->n_states];
    D->arc_in = R.span(D->n_arcs);
    if (!D->arc_in) return pd_err(err, "the description ends inside the arcs");
    D->streams.assign((size_t)D->n_streams, PdStream());
    long long out = 0;
    for (int s = 0; s < D->n_streams; ++s) {
        PdStream &S = D->streams[(size_t)s];
        if (!pd_parse_stream(R, *D, s, &S, err)) return false;
        out += PD_OUT_STREAM_WORDS + 7LL * S.n_paths + S.n_inst_all * D->NE + S.n_items_all;
    }
    D->ops.assign((size_t)D->n_ops, PdOp());
    for (int i = 0; i < D->n_ops; ++i) {
        PdOp &O = D->ops[(size_t)i];
        if (!R.take(&O.kind)) return pd_err(err, "the description ends inside operation %lld", i);
        auto stream_ok = [&](int s) { return s >= 0 && s < D->n_streams; };
        if (O.kind == PD_COLLECT) {
            if (!R.take(&O.n_work) || O.n_work < 0 || O.n_work > D->n_streams) return pd_err(err, "operation %lld: a work list of %lld streams", i, O.n_work);
            const int ns = O.n_work ? O.n_work : 1;
            for (int k = 0; k < ns; ++k) {
                if (!R.take(&O.streams[k]) || !stream_ok(O.streams[k])) return pd_err(err, "operation %lld: bad stream", i);
                for (int j = 0; j < k; ++j) if (O.streams[j] == O.streams[k]) return pd_err(err, "operation %lld: stream %lld twice", i, O.streams[k]);
            }
            if (!R.take(&O.G) || !R.take(&O.gc_threshold) || !R.take(&O.path_rule)) return pd_err(err, "the description ends inside operation %lld", i);
            if (O.G < 1 || O.G > 32) return pd_err(err, "operation %lld: G %lld outside 1 .. 32", i, O.G);
            if (O.path_rule != 0 && O.path_rule != 1) return pd_err(err, "operation %lld: path_rule %lld (0 or 1)", i, O.path_rule);
        } else if (O.kind == PD_TRACE) {
            O.n_work = 1;
            if (!R.take(&O.streams[0]) || !R.take(&O.last_frame[0]) || !R.take(&O.res_cap) || !R.take(&O.model_level))
                return pd_err(err, "the description ends inside operation %lld", i);
            if (!stream_ok(O.streams[0])) return pd_err(err, "operation %lld: bad stream", i);
            if (O.model_level != 0 && O.model_level != 1) return pd_err(err, "operation %lld: model_level %lld (0 or 1)", i, O.model_level);
        } else if (O.kind == PD_TRACE_MANY) {
            if (!R.take(&O.n_work) || O.n_work < 1 || O.n_work > D->n_streams) return pd_err(err, "operation %lld: a work list of %lld streams", i, O.n_work);
            for (int k = 0; k < O.n_work; ++k) {
                if (!R.take(&O.streams[k]) || !R.take(&O.last_frame[k]) || !R.take(&O.have[k])) return pd_err(err, "the description ends inside operation %lld", i);
                if (!stream_ok(O.streams[k]) || O.have[k] < 0) return pd_err(err, "operation %lld: bad stream, or have < 0", i);
                for (int j = 0; j < k; ++j) if (O.streams[j] == O.streams[k]) return pd_err(err, "operation %lld: stream %lld twice", i, O.streams[k]);
            }
            if (!R.take(&O.res_cap)) return pd_err(err, "the description ends inside operation %lld", i);
        } else if (O.kind == PD_FINAL_MANY || O.kind == PD_TRACE_MANY_MODELS) {
            if (!R.take(&O.n_work) || O.n_work < 1 || O.n_work > D->n_streams) return pd_err(err, "operation %lld: a work list of %lld streams", i, O.n_work);
            for (int k = 0; k < O.n_work; ++k) {
                int a, b, c;
                if (!R.take(&O.streams[k]) || !R.take(&a) || !R.take(&b) || !R.take(&c)) return pd_err(err, "the description ends inside operation %lld", i);
                if (!stream_ok(O.streams[k])) return pd_err(err, "operation %lld: bad stream", i);
                for (int j = 0; j < k; ++j) if (O.streams[j] == O.streams[k]) return pd_err(err, "operation %lld: stream %lld twice", i, O.streams[k]);
                if (O.kind == PD_FINAL_MANY) { O.final_tok[k][0] = a; O.final_tok[k][1] = b; O.final_tok[k][2] = c; }
                else {
                    O.last_frame[k] = a; O.have[k] = b; O.have_m[k] = c;
                    if (b < 0 || c < 0) return pd_err(err, "operation %lld: have %lld / have_m %lld < 0", i, b, c);
                }
            }
            if (!R.take(&O.res_cap)) return pd_err(err, "the description ends inside operation %lld", i);
            if (O.kind == PD_FINAL_MANY) {
                if (!R.take(&O.model_level)) return pd_err(err, "the description ends inside operation %lld", i);
                if (O.model_level != 0 && O.model_level != 1) return pd_err(err, "operation %lld: model_level %lld (0 or 1)", i, O.model_level);
            }
        } else return pd_err(err, "operation %lld: kind %lld", i, O.kind);
        if (O.kind != PD_COLLECT) {
            if (O.res_cap < 1 || O.res_cap > PD_MAX_RES_CAP) return pd_err(err, "operation %lld: res_cap %lld outside [1, 2^16]", i, O.res_cap);
            out += O.kind == PD_TRACE ? 3 + 8LL * O.res_cap : O.kind == PD_TRACE_MANY ? (2LL + 2LL * PD_SHARE) * O.n_work
                   : O.kind == PD_FINAL_MANY ? PdOp::final_words(O.n_work, D->n_streams, O.res_cap) : PdOp::pm_words(O.n_work, D->n_streams, O.res_cap);
        }
    }
    if (R.at != n) return pd_err(err, "%lld words behind the description's end", n - R.at);
    D->out_words = out;
    return true;
}

// ---- the byte images, as the kernels address them (int32 words; p = frame & 1: the list the next frame reads, p ^ 1: the last frame's)

// instance records, [2][cap_slots]: RecLayout<NE> chunks of 64, wave segment w at chunk w * (seg_rec >> 6)
inline void pd_image_rec(const PdDesc &D, const PdStream &S, std::vector<int32_t> *img)
{
    img->assign((size_t)(2LL * D.cap_slots * pd_rec_bytes(D.NE) / 4), 0);
    if (!S.waves) return;
    const PdGeo g = pd_geo(D, S.waves);
    const int p = S.frame & 1, HF = pd_hf(D.NE);
    for (int w = 0; w < S.waves; ++w) {
        const int32_t *r = S.rec[(size_t)w];
        const int n_inst = *r++;
        const long long seg = (long long)p * D.cap_slots * pd_rec_bytes(D.NE) + (long long)w * (g.seg_rec >> 6) * pd_chunk_bytes(D.NE);
        for (int q = 0; q < n_inst; ++q) {
            const int n = r[0], src = r[1];
            int32_t *rec = img->data() + (seg + (long long)(q >> 6) * pd_chunk_bytes(D.NE) + (long long)(q & 63) * 16) / 4;
            rec[0] = 0; rec[1] = n; rec[2] = src; rec[3] = 0;
            for (int j = 1; j <= D.NE; ++j) {
                int32_t *t = rec + (long long)(HF + j - 1) * 256;
                if (j < n - 1) { t[0] = r[2 * j]; t[1] = 0; t[2] = 0; t[3] = r[2 * j + 1]; }
                else t[0] = t[1] = t[2] = t[3] = D.sentinel;
            }
            r += 2 + 2 * (n - 2);
        }
    }
}
// the path word of every token slot back out of such an image, [wave][instance][NE]
inline void pd_read_rec(const PdDesc &D, const PdStream &S, const std::vector<int32_t> &img, int32_t *out)
{
    if (!S.waves) return;
    const PdGeo g = pd_geo(D, S.waves);
    const int p = S.frame & 1, HF = pd_hf(D.NE);
    for (int w = 0; w < S.waves; ++w) {
        const int n_inst = S.rec[(size_t)w][0];
        const long long seg = (long long)p * D.cap_slots * pd_rec_bytes(D.NE) + (long long)w * (g.seg_rec >> 6) * pd_chunk_bytes(D.NE);
        for (int q = 0; q < n_inst; ++q) {
            const int32_t *rec = img.data() + (seg + (long long)(q >> 6) * pd_chunk_bytes(D.NE) + (long long)(q & 63) * 16) / 4;
            for (int j = 1; j <= D.NE; ++j) *out++ = rec[(long long)(HF + j - 1) * 256 + 3];
        }
    }
}
// frontier items, [2][cap_items] of 32 bytes (token, then {arc, out, to, flag}): the last frame's at parity p ^ 1
inline long long pd_item_word(const PdDesc &D, const PdStream &S, const PdGeo &g, int w, int k)
{
    return 8 * ((long long)((S.frame & 1) ^ 1) * D.cap_items + (long long)w * g.seg_item + k);
}
inline void pd_image_items(const PdDesc &D, const PdStream &S, std::vector<int32_t> *img)
{
    img->assign((size_t)(16LL * D.cap_items), 0);
    if (!S.waves) return;
    const PdGeo g = pd_geo(D, S.waves);
    for (int w = 0; w < S.waves; ++w)
        for (int k = 0; k < S.item[(size_t)w][0]; ++k) (*img)[(size_t)pd_item_word(D, S, g, w, k) + 3] = S.item[(size_t)w][1 + k];
}
inline void pd_read_items(const PdDesc &D, const PdStream &S, const std::vector<int32_t> &img, int32_t *out)
{
    if (!S.waves) return;
    const PdGeo g = pd_geo(D, S.waves);
    for (int w = 0; w < S.waves; ++w)
        for (int k = 0; k < S.item[(size_t)w][0]; ++k) *out++ = img[(size_t)pd_item_word(D, S, g, w, k) + 3];
}
// the dirty lists, [2][cap_new]: the last frame's at parity p ^ 1, in segments of ITS writer waves
inline void pd_image_dirty(const PdDesc &D, const PdStream &S, std::vector<int32_t> *img)
{
    img->assign((size_t)(2LL * D.cap_new), 0);
    if (!S.dirty_waves) return;
    const PdGeo gd = pd_geo(D, S.dirty_waves);
    for (int w = 0; w < S.dirty_waves; ++w)
        for (int k = 0; k < S.dirty[(size_t)w][0]; ++k)
            (*img)[(size_t)((long long)((S.frame & 1) ^ 1) * D.cap_new + (long long)w * gd.seg_new + k)] = S.dirty[(size_t)w][1 + k];
}
// the per-wave counts: tot[TOT_N][MAXW] and item_end[MAXW]
inline void pd_image_counts(const PdDesc &, const PdStream &S, std::vector<int32_t> *tot, std::vector<int32_t> *item_end)
{
    tot->assign((size_t)PD_TOT_N * PD_MAXW, 0);
    item_end->assign((size_t)PD_MAXW, 0);
    const int p = S.frame & 1;
    for (int w = 0; w < S.waves; ++w) {
        (*tot)[(size_t)(PD_TOT_REC0 + p) * PD_MAXW + (size_t)w] = S.rec[(size_t)w][0];
        (*item_end)[(size_t)w] = S.item[(size_t)w][0];
    }
    for (int w = 0; w < S.dirty_waves; ++w) (*tot)[(size_t)(PD_TOT_DIRTY0 + (p ^ 1)) * PD_MAXW + (size_t)w] = S.dirty[(size_t)w][0];
}
// the per-state words in the split8 layout (srec_stride 16, srec_arr 16 n, srec_estride 8, srec_par 8 n): n bids of 16 bytes, then the arrival
// keys of parity 0, then those of parity 1, 8 bytes each.  A key that is there: some score in the high word, the item in the low one.
#define PD_KEY_HIGH 0xc0000000u
inline void pd_image_srec(const PdDesc &D, const PdStream &S, std::vector<int32_t> *img)
{
    img->assign((size_t)(8LL * D.n_states), 0);
    const int q = (S.frame & 1) ^ 1;
    for (int st = 0; st < D.n_states; ++st)
        if (S.arrival[st] >= 0) {
            const size_t at = (size_t)(4LL * D.n_states + 2LL * q * D.n_states + 2LL * st);
            (*img)[at] = S.arrival[st]; (*img)[at + 1] = (int32_t)PD_KEY_HIGH;
        }
}
// the Path arena: 32-byte records, the last word padding
inline void pd_image_paths(const PdStream &S, std::vector<int32_t> *img)
{
    img->assign((size_t)(8LL * S.cap_paths), 0);
    for (long long q = 0; q < S.n_paths; ++q)
        for (int k = 0; k < 7; ++k) (*img)[(size_t)(8 * q + k)] = S.paths[7 * q + k];
}
