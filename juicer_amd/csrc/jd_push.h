// jd_push.h - the streaming interface (jd_stream_init / _push / _finish, jd_streams_push, jd_streams_trace) as DECISIONS: the host's
// record of a stream, what a call's arguments are refused for, PARTIAL_DECODING's schedule (src/WFSTDecoderLite.cpp:358-368: where a
// chunk or a round ends, what the control words read behind a launch mean, who collects, when a trace is due), the packing of a
// jd_streams_push call and the layout of k_partial_many's and k_partial_many_models' buffers.  Plain functions over plain structs, no HIP: jd_host_stream.h makes
// the copies, launches and synchronisations between them; tests/push_driver.cpp runs them on the CPU (tests/test_push_cpu.py).  That
// driver carries a twin of jd_stream_push's loop and of streams_push_rounds with the device replaced by a model: whoever changes how
// these functions are called changes both.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "jd_prep.h"            // path_rule_fires, PARTIAL_SHARE: what the kernels use of the same rules

// collectPaths runs behind frame f when f - lastPathCollectFrame > 100 (WFSTDecoderLite.cpp:360-362, the frame rule), or when the
// count rule fires (path_rule_fires)
enum { PATH_COLLECT_EVERY = 100 };

// ---- one stream of the streaming interface, as the host knows it (lazy_in and stream_dirty are the device run's, jd_dec)
struct PushModels { std::vector<int32_t> model, label, time; std::vector<float> score, ac, lm; };
struct PushStream {
    int T = 0;                                         // frames pushed - and searched - so far
    // a spliced model's stream (jd_splice.h): the frames pushed, of which T are searched, and the last ones of them, which a later
    // window still reads (splice_push_plan: at most left + right while the stream is open); 0 / empty for every other model
    int pushed = 0;
    std::vector<float> held;
    int started = 0;
    int open = 0;                                      // frames pushed since the stream's init, not finished yet (jd_dec_set_output_level)
    int resident = 0;                                  // the utterance was begun on the resident kernel (jd_res_init: a broker's stream)
    // PARTIAL_DECODING (WFSTDecoderLite.h:199-205)
    int last_collect = -1, last_trace = -1;            // lastPathCollectFrame, lastPartialTraceFrame
    int n_collect = 0;                                 // collections of the stream's utterance so far (jd_stream_collect_info)
    std::vector<int32_t> partial_label, partial_time;  // partialPaths, oldest first
    PushModels partial_m;                              // ... the model-level list of the same traces (jd_stream_partial_models)
    PushModels best;                                   // the best token's record chain as of the last jd_streams_best, oldest first (jd_best.h)
    PushModels fin;                                    // bestFinalToken's record chain as of the last jd_streams_final, oldest first (jd_final.h)
    float fin_tot[3] = {0.0f, 0.0f, 0.0f};             // ... and its totals: the token's score, ac, lm with the final-state weight
    void init()                                        // jd_stream_init (WFSTDecoderLite.cpp:179-181, 202-206)
    {
        T = 0; started = 1; open = 0; resident = 0;
        pushed = 0; held.clear();
        last_collect = -1; last_trace = -1; n_collect = 0;
        partial_label.clear(); partial_time.clear();
        partial_m = PushModels();
        best = PushModels();
        fin = PushModels(); fin_tot[0] = fin_tot[1] = fin_tot[2] = 0.0f;
    }
    void begin() { T = 0; started = 1; open = 0; resident = 1; pushed = 0; held.clear(); }     // jd_res_init: the broker's stream begins an utterance (it runs no PARTIAL_DECODING)
    void taken_over() { started = 0; T = 0; open = 0; resident = 0; pushed = 0; held.clear(); }   // a batch takes every stream over (jd_decode_batch_device)
    // jd_stream_finish: under PARTIAL_DECODING one more trace, from the best token (:245-251) - the hypothesis (n < 0: none) comes
    // newest first, partialPaths are oldest first
    void finish(bool partial, int n, const int32_t *label, const int32_t *time)
    {
        open = 0;
        if (!partial || n < 0) return;
        partial_label.resize((size_t)n); partial_time.resize((size_t)n);
        for (int k = 0; k < n; ++k) { partial_label[(size_t)k] = label[n - 1 - k]; partial_time[(size_t)k] = time[n - 1 - k]; }
    }
};

// ---- what a call's arguments are refused for (the texts are the callers'), and the stream concerned
enum PushArg { PUSH_ARG_OK = 0, PUSH_ARG_BAD, PUSH_ARG_BAD_STREAM, PUSH_ARG_NOT_STARTED, PUSH_ARG_TOO_MANY_ROWS };
struct PushCheck { PushArg verdict; int stream; };
// jd_stream_push(d, s, frames, n_frames); S null: no decoder
static inline PushCheck push_check_one(const std::vector<PushStream> *S, int s, bool has_frames, int n_frames)
{
    if (!S || s < 0 || s >= (int)S->size() || n_frames < 0 || (n_frames > 0 && !has_frames)) return PushCheck{PUSH_ARG_BAD, s};
    if (!(*S)[(size_t)s].started) return PushCheck{PUSH_ARG_NOT_STARTED, s};
    return PushCheck{PUSH_ARG_OK, s};
}
// jd_streams_push(d, n, streams, frames, n_frames) and jd_streams_trace(d, n, streams, found): the call as a whole ...
static inline PushCheck push_check_call(bool has_dec, int n, bool has_lists)
{
    return PushCheck{(!has_dec || n < 0 || (n > 0 && !has_lists)) ? PUSH_ARG_BAD : PUSH_ARG_OK, -1};
}
// ... and jd_streams_push's entries, in order: each stream once, in range, started, frames where it says it brings some.  Every entry
// that brings frames opens its stream as it passes (as recorded: the entries in front of a refused one have), *rows: the frames of the
// call - at most 0x7fffff00, what the row numbers of a table can say.
static inline PushCheck push_check_entries(std::vector<PushStream> &S, int n, const int32_t *streams, const float *const *frames, const int32_t *n_frames,
                                           long long *rows)
{
    std::vector<char> seen(S.size(), 0);
    *rows = 0;
    for (int i = 0; i < n; ++i) {
        const int s = streams[i];
        if (s < 0 || s >= (int)S.size() || n_frames[i] < 0 || (n_frames[i] > 0 && !frames[i]) || seen[(size_t)s]) return PushCheck{PUSH_ARG_BAD_STREAM, s};
        if (!S[(size_t)s].started) return PushCheck{PUSH_ARG_NOT_STARTED, s};
        seen[(size_t)s] = 1;
        if (n_frames[i] > 0) S[(size_t)s].open = 1;
        *rows += n_frames[i];
    }
    return PushCheck{*rows > 0x7fffff00LL ? PUSH_ARG_TOO_MANY_ROWS : PUSH_ARG_OK, -1};
}
// ... and jd_streams_trace's: found[] (or null) is cleared as the entries pass; ss / at: the streams that have a frame to trace from
// and their places in the list (nothing to trace before the first frame, as jd_stream_partial)
static inline PushCheck push_check_trace(const std::vector<PushStream> &S, int n, const int32_t *streams, int32_t *found, std::vector<int> *ss, std::vector<int> *at)
{
    std::vector<char> seen(S.size(), 0);
    for (int i = 0; i < n; ++i) {
        const int s = streams[i];
        if (s < 0 || s >= (int)S.size() || seen[(size_t)s]) return PushCheck{PUSH_ARG_BAD_STREAM, s};
        if (!S[(size_t)s].started) return PushCheck{PUSH_ARG_NOT_STARTED, s};
        seen[(size_t)s] = 1;
        if (found) found[i] = 0;
        if (S[(size_t)s].T > 0) { ss->push_back(s); at->push_back(i); }
    }
    return PushCheck{PUSH_ARG_OK, -1};
}

// ---- PARTIAL_DECODING's schedule (:358-368).  The trace rides on the path collection, and the kernel looks for the count rule before
// every frame of a launch but its first - so a launch takes a stream from frame T to the frame rule's frame at the most: the first
// frame f with f - lastPathCollectFrame > 100 is the last one processed, and the host looks behind it.  At least one frame; never
// beyond `target`.  To jd_stream_push that is a chunk, to jd_streams_push a round.
static inline int push_limit(int T, int target, int last_collect)
{
    return std::min(target, std::max(T + 1, last_collect + PATH_COLLECT_EVERY + 2));
}
// the frames of jd_stream_push's next chunk: what fits the table (Fc) of what is left, and under PARTIAL_DECODING up to the limit
static inline int push_chunk_frames(int Fc, int left, int interval, int last_collect, int T)
{
    const int n = std::min(Fc, left);
    return interval > 0 ? push_limit(T, T + n, last_collect) - T : n;
}

// A round of jd_streams_push under PARTIAL_DECODING.  work[k]: the stream of entry k of the call, target[k]: the frame it is to reach,
// out[k]: it failed in this call.  act: the entries that take part (not out, not there yet), with their weights (frames ahead);
// limit[k] for those; hT: every stream's frame count for the device, the limit where it takes part; f_end: the largest limit; s_lo ..
// s_hi: the control blocks to read behind the launch (streams in between ride along).
struct PushRound {
    std::vector<size_t> act;
    std::vector<int> limit, hT;
    std::vector<double> weight;
    int f_end, s_lo, s_hi;
};
static inline void push_round_plan(const std::vector<PushStream> &S, const std::vector<int> &work, const std::vector<int> &target, const std::vector<char> &out,
                                   PushRound *R)
{
    R->act.clear(); R->weight.clear();
    R->limit.resize(work.size(), 0); R->hT.resize(S.size());
    R->f_end = 0; R->s_lo = (int)S.size(); R->s_hi = -1;
    for (size_t s = 0; s < S.size(); ++s) R->hT[s] = S[s].T;
    for (size_t k = 0; k < work.size(); ++k) {
        const int s = work[k], at = S[(size_t)s].T;
        if (out[k] || at >= target[k]) continue;
        R->limit[k] = push_limit(at, target[k], S[(size_t)s].last_collect);
        R->hT[(size_t)s] = R->limit[k];
        R->act.push_back(k); R->weight.push_back((double)(R->limit[k] - at));
        R->f_end = std::max(R->f_end, R->limit[k]); R->s_lo = std::min(R->s_lo, s); R->s_hi = std::max(R->s_hi, s);
    }
}

// Behind a launch: the stream's control words as read there (StreamCtl; the two counts are the reference's where the decoder keeps
// them), and what they mean for a stream that was to reach `limit`.  An error: the stream stands at fail_T and is dirty (reported by
// jd_stream_finish).  Else it stands at `frame`, and a collection of the reference's ran on it or not.  "Collected", by_flag: the
// launch says it came back behind a collection (launch_flag; one stream, without the reference's counts - launch_search says so
// whenever it ran the collection, the arena's own included); else: the device has counted one more than the host (k_gc_remap counts
// the reference's collections where the decoder keeps the reference's counts - one that only the arena asked for is none of them and
// carries no trace - and every collection where it does not).  Where none ran and the stream is through its limit, the frame rule or
// the count rule may fire behind that last frame, which the kernel does not look behind: the host has to collect (host_collects).
struct PushCtl { int error, frame, n_collect, n_path, n_path_new; };
struct PushAfter { bool failed; int at; bool collected, host_collects; int T; };   // at: the last frame processed
static inline PushAfter push_after(const PushStream &P, const PushCtl &c, int limit, int fail_T, bool by_flag, bool launch_flag)
{
    PushAfter a{false, -1, false, false, fail_T};
    if (c.error != 0) { a.failed = true; return a; }
    a.at = c.frame - 1;
    a.collected = by_flag ? launch_flag : c.n_collect > P.n_collect;
    if (!a.collected && c.frame >= limit && (a.at - P.last_collect > PATH_COLLECT_EVERY || path_rule_fires(c.n_path, c.n_path_new)))
        a.host_collects = a.collected = true;
    a.T = c.frame;
    return a;
}
// ... booked, once the collection has run (:746); true: the trace is due (:362-368)
static inline bool push_book_collection(PushStream &P, int at, int interval)
{
    P.last_collect = at;
    P.n_collect += 1;
    return at - P.last_trace > interval;
}

// ---- a jd_streams_push call, packed: the rows of the common table are the entries' frames, stream after stream; row r of it is
// frame T + (r - first row) of its stream.  k_search reads row  slot + (f - f0)  with f0 = 0: the slot is the stream's first row minus
// its first frame (negative where the stream stands behind its first row).  The scoring kernels take whole tiles of `tile` rows.
// Everything the launch needs from the host goes through ONE pinned staging buffer: [frames: rows x D floats][row_src: tile_rows
// ints][T: a frame count per stream].
struct PushWork { int stream, slot; };
struct PushPack {
    long long rows; size_t tile_rows;
    std::vector<PushWork> work;                        // per entry that brings frames, in the call's order
    std::vector<size_t> entry, row0;                   // ... its place in the call, its first row
    std::vector<double> weight;
    std::vector<int> target;                           // ... the frame it is to reach (Tnew)
    int f_end;
    size_t src_at, T_at, need;                         // byte offsets of row_src and T in the staging buffer, and its size
};
static inline size_t push_tile_rows(long long rows, int tile) { return ((size_t)rows + (size_t)tile - 1) / (size_t)tile * (size_t)tile; }
static inline size_t push_grown(size_t need) { return need + need / 2; }   // the staging buffer grows by half more than asked
static inline void push_pack(const std::vector<PushStream> &S, int n, const int32_t *streams, const int32_t *n_frames, long long rows, int D, int tile, PushPack *K)
{
    K->rows = rows; K->tile_rows = push_tile_rows(rows, tile);
    K->work.clear(); K->entry.clear(); K->row0.clear(); K->weight.clear(); K->target.clear();
    K->f_end = 0;
    K->src_at = (size_t)rows * (size_t)D * sizeof(float); K->T_at = K->src_at + K->tile_rows * sizeof(int);
    K->need = K->T_at + S.size() * sizeof(int);
    size_t r0 = 0;
    for (int i = 0; i < n; ++i) {
        if (n_frames[i] == 0) continue;
        const PushStream &P = S[(size_t)streams[i]];
        K->work.push_back(PushWork{streams[i], (int)((long long)r0 - P.T)});
        K->entry.push_back((size_t)i); K->row0.push_back(r0);
        K->weight.push_back((double)n_frames[i]);
        K->target.push_back(P.T + n_frames[i]);
        K->f_end = std::max(K->f_end, K->target.back());
        r0 += (size_t)n_frames[i];
    }
}
// ... the two integer regions: row_src is the identity (the frames are packed the same way), -1 in the rest of the last tile; the
// streams of the call get their targets, the others keep their frame counts
static inline void push_pack_fill(const std::vector<PushStream> &S, const PushPack &K, int *h_src, int *h_T)
{
    for (size_t s = 0; s < S.size(); ++s) h_T[s] = S[s].T;
    for (size_t w = 0; w < K.work.size(); ++w) h_T[K.work[w].stream] = K.target[w];
    for (size_t r = 0; r < K.tile_rows; ++r) h_src[r] = r < (size_t)K.rows ? (int)r : -1;
}

// ---- k_partial_many's buffers (jd_gc.h), for max_streams entries: [int4 work list][{found, n} heads][staging: PARTIAL_SHARE (label,
// frame) pairs per entry].  A launch of n entries writes its n heads and, behind them, its n shares - partial_many_stage_at - and the
// host fetches reply_words(n) in ONE copy.
struct PartialManyLayout {
    size_t head_at, per, words;
    size_t reply_words(int n) const { return per * (size_t)n; }
};
static inline PartialManyLayout partial_many_layout(int max_streams)
{
    const size_t M = (size_t)max_streams, head_at = 4 * M, per = 2 + 2 * (size_t)PARTIAL_SHARE;
    return PartialManyLayout{head_at, per, head_at + per * M};
}
// where entry i's share begins in the words a launch of n entries writes (k_partial_many computes `stage` by the same expression,
// written out there: through a function the kernel's registers came out numbered differently)
static inline size_t partial_many_stage_at(int n, int i) { return 2 * (size_t)n + 2 * (size_t)PARTIAL_SHARE * i; }
// the request of a stream: {stream, the frame of the last record the host has of it (-1: none), the records it has, -}
struct PartialRequest { int stream, last_frame, have, pad; };
static inline PartialRequest partial_many_request(const PushStream &P, int s)
{
    return PartialRequest{s, P.partial_time.empty() ? -1 : P.partial_time.back(), (int)P.partial_label.size(), 0};
}
// the reply {found, len} of a stream of which the host has `have` records (they are the chain's prefix): nothing converged; a chain
// longer than the result capacity (an error, the stream's alone); the new records from its share of the staging area; or, more than a
// share of them, the whole chain from the stream's result arrays
enum PartialReply { PARTIAL_NOT_FOUND = 0, PARTIAL_TOO_LONG, PARTIAL_FROM_STAGE, PARTIAL_FROM_RESULTS };
static inline PartialReply partial_many_reply(int found, int len, int have, int res_cap)
{
    if (!found) return PARTIAL_NOT_FOUND;
    if (len > res_cap) return PARTIAL_TOO_LONG;
    return len - have <= PARTIAL_SHARE ? PARTIAL_FROM_STAGE : PARTIAL_FROM_RESULTS;
}
// ... from the staging share: records [have, len)
static inline void partial_many_take(PushStream &P, int have, int len, const int *stage)
{
    for (int k = have; k < len; ++k) { P.partial_label[(size_t)k] = stage[2 * (k - have)]; P.partial_time[(size_t)k] = stage[2 * (k - have) + 1]; }
}

// ---- k_partial_many_models' buffers (jd_gc.h; jd_streams_trace_models), for max_streams entries: [int4 work list][heads: PM_HEAD words
// per entry: found, n (word records), nm (model records), -][staging per entry: PARTIAL_SHARE (label, frame) pairs, then PM_SHARE model
// records of PM_FIELDS words, field-major].  A launch of n entries writes its n heads and, behind them, its n shares, and the host
// fetches reply_words(n) in ONE copy.  A trace's lists extend the lists of the trace before it (both of them: the model list ends at
// the record the word list ends at), so only the words [have, n) and the model records [have_m, nm) are new to the host.
// PM_SHARE: the word share is PARTIAL_SHARE = 32 new words per trace (its reasoning: at k_partial_many).  A model-level chain carries
// every model the path has left beside the word labels; on the measured utterance of DESIGN.md section 7 that is 59 model entries
// where the word list has 17, so the model records that 32 new words bring are 32 * 59 / 17 = 111.06: 112, which also keeps every
// field of a share a multiple of 16 bytes long (448 bytes).  A stream with more new records of either kind (a first trace late in a
// long utterance) is read from the device arrays instead.
#define PM_SHARE 112
#define PM_FIELDS 6             // model, label, time, score, ac, lm
#define PM_HEAD 4
#define PM_PER ((size_t)PM_HEAD + 2 * (size_t)PARTIAL_SHARE + (size_t)PM_FIELDS * PM_SHARE)
// where entry i's share begins in the words a launch of n entries writes: its word pairs first, its model records behind them, field
// f of new record k (kernel and host)
#define PM_STAGE_AT(n, i) ((size_t)PM_HEAD * (size_t)(n) + (2 * (size_t)PARTIAL_SHARE + (size_t)PM_FIELDS * PM_SHARE) * (size_t)(i))
#define PM_STAGE_MODELS (2 * (size_t)PARTIAL_SHARE)
#define PM_STAGE_WORD(f, k) (PM_STAGE_MODELS + (size_t)(f) * PM_SHARE + (size_t)(k))
struct PartialModelsLayout {
    size_t head_at, per, words;
    size_t reply_words(int n) const { return per * (size_t)n; }
};
static inline PartialModelsLayout partial_models_layout(int max_streams)
{
    const size_t M = (size_t)max_streams, head_at = 4 * M;
    return PartialModelsLayout{head_at, PM_PER, head_at + PM_PER * M};
}
// the per-stream area the kernel exports a trace's model list into: [model, label, time, score, ac, lm][res_cap] for every stream
static inline size_t partial_models_area_words(int max_streams, int res_cap) { return (size_t)max_streams * PM_FIELDS * (size_t)res_cap; }
// the request of a stream: {stream, the frame of the last word record the host has of it (-1: none), the word records it has, the
// model records it has}
struct PartialModelsRequest { int stream, last_frame, have, have_m; };
static inline PartialModelsRequest partial_models_request(const PushStream &P, int s)
{
    return PartialModelsRequest{s, P.partial_time.empty() ? -1 : P.partial_time.back(), (int)P.partial_label.size(), (int)P.partial_m.model.size()};
}
// the reply {found, n, nm} of a stream of which the host has `have` words and `have_m` model records: nothing converged; a list
// longer than the result capacity (an error, the stream's alone); the new entries of both lists from its share of the staging area;
// or - more than a share of either, or a host that is ahead of the device (never after a trace of this library) - both lists whole
// from the device arrays
enum PartialModelsReply { PARTIAL_M_NOT_FOUND = 0, PARTIAL_M_TOO_LONG, PARTIAL_M_FROM_STAGE, PARTIAL_M_FROM_ARRAYS };
static inline PartialModelsReply partial_models_reply(int found, int n, int nm, int have, int have_m, int res_cap)
{
    if (!found) return PARTIAL_M_NOT_FOUND;
    if (n > res_cap || nm > res_cap) return PARTIAL_M_TOO_LONG;
    if (have > n || have_m > nm) return PARTIAL_M_FROM_ARRAYS;
    return (n - have <= PARTIAL_SHARE && nm - have_m <= PM_SHARE) ? PARTIAL_M_FROM_STAGE : PARTIAL_M_FROM_ARRAYS;
}
static inline void partial_models_resize(PushModels &M, size_t n) { M.model.resize(n); M.label.resize(n); M.time.resize(n); M.score.resize(n); M.ac.resize(n); M.lm.resize(n); }
// ... from the staging share (the entry's, at PM_STAGE_AT): words [have, n) and model records [have_m, nm)
static inline void partial_models_take(PushStream &P, int have, int n, int have_m, int nm, const int *stage)
{
    P.partial_label.resize((size_t)n); P.partial_time.resize((size_t)n);
    for (int k = have; k < n; ++k) { P.partial_label[(size_t)k] = stage[2 * (k - have)]; P.partial_time[(size_t)k] = stage[2 * (k - have) + 1]; }
    PushModels &M = P.partial_m;
    partial_models_resize(M, (size_t)nm);
    for (int k = have_m; k < nm; ++k) {
        const int j = k - have_m;
        M.model[(size_t)k] = stage[PM_STAGE_WORD(0, j)]; M.label[(size_t)k] = stage[PM_STAGE_WORD(1, j)]; M.time[(size_t)k] = stage[PM_STAGE_WORD(2, j)];
        memcpy(&M.score[(size_t)k], &stage[PM_STAGE_WORD(3, j)], 4); memcpy(&M.ac[(size_t)k], &stage[PM_STAGE_WORD(4, j)], 4);
        memcpy(&M.lm[(size_t)k], &stage[PM_STAGE_WORD(5, j)], 4);
    }
}
// ... or whole from the device arrays: words = [label, time][n] as fetched, rows = [model, label, time, score, ac, lm][nm]
static inline void partial_models_take_arrays(PushStream &P, int n, const int32_t *words, int nm, const int32_t *rows)
{
    const size_t N = (size_t)n, NM = (size_t)nm;
    P.partial_label.assign(words, words + N); P.partial_time.assign(words + N, words + 2 * N);
    PushModels &M = P.partial_m;
    partial_models_resize(M, NM);
    if (!NM) return;
    memcpy(M.model.data(), rows, NM * 4); memcpy(M.label.data(), rows + NM, NM * 4); memcpy(M.time.data(), rows + 2 * NM, NM * 4);
    memcpy(M.score.data(), rows + 3 * NM, NM * 4); memcpy(M.ac.data(), rows + 4 * NM, NM * 4); memcpy(M.lm.data(), rows + 5 * NM, NM * 4);
}
