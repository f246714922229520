// jd_best.h - the current best hypothesis of live streams (jd_streams_best, jd_stream_best_words / _models) as DECISIONS: the request
// of a stream, the layout of k_best_many's buffers (jd_gc.h), what a reply means and the word projection of a model-level list.  Plain
// functions over plain structs, no HIP: jd_host_stream.h makes the copies and the launch; tests/best_driver.cpp runs them on the CPU
// (tests/test_best_cpu.py).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "jd_push.h"            // PushModels: the host's copy of a list, held with the stream's record (PushStream::best)

// ---- k_best_many's buffers, for max_streams entries: [int4 work list][heads: BEST_HEAD words per entry][staging: BEST_SHARE records
// of BEST_FIELDS words per entry, field-major].  A launch of n entries writes its n heads and, behind them, its n shares, and the host
// fetches reply_words(n) in ONE copy.
// BEST_SHARE: the hypothesis is sent whole at every call (it is revised, not extended).  A live utterance of a few hundred frames has
// a few dozen records at model level, fewer at word level: 64 records (1.5 KiB per stream, 24 KiB a copy for sixteen callers) take
// those; a longer chain is fetched from the stream's result arrays instead.
#define BEST_SHARE 64
#define BEST_FIELDS 6           // model, label, time, score, ac, lm (the fields of jd_model_hyp)
#define BEST_HEAD 12            // found, frame, n_words, n_records, model, state, score, ac, lm, 3 spare: the first nine are jd_best
// where entry i's share begins in the words a launch of n entries writes, and field f of record k inside a share (kernel and host)
#define BEST_STAGE_AT(n, i) ((size_t)BEST_HEAD * (size_t)(n) + (size_t)(BEST_FIELDS * BEST_SHARE) * (size_t)(i))
#define BEST_STAGE_WORD(f, k) ((size_t)(f) * BEST_SHARE + (size_t)(k))

// the head of an entry as the kernel writes it (the host fills `frame`: the frames pushed); jd_best of the C ABI is the same nine words
struct BestHead { int32_t found, frame, n_words, n_records, model, state; float score, ac, lm; };
static_assert(sizeof(BestHead) == 9 * 4 && sizeof(BestHead) <= BEST_HEAD * 4, "k_best_many writes the head word by word");

// the request of a stream: {stream, -, -, -}
struct BestRequest { int32_t stream, pad0, pad1, pad2; };
static inline BestRequest best_request(int s) { return BestRequest{s, 0, 0, 0}; }

// jd_streams_best's entries, in order (the call as a whole: push_check_call): each stream once, in range, started by jd_stream_init -
// a stream whose utterance a broker began on the resident kernel is not the caller's to look at.  ss / at: the streams that have a
// frame to look behind and their places in the list.
enum BestArg { BEST_ARG_OK = 0, BEST_ARG_BAD_STREAM, BEST_ARG_NOT_STARTED, BEST_ARG_RESIDENT };
struct BestCheck { BestArg verdict; int stream; };
static inline BestCheck best_check(const std::vector<PushStream> &S, int n, const int32_t *streams, std::vector<int> *ss, std::vector<int> *at)
{
    const PushCheck c = push_check_trace(S, n, streams, nullptr, ss, at);
    if (c.verdict == PUSH_ARG_BAD_STREAM) return BestCheck{BEST_ARG_BAD_STREAM, c.stream};
    if (c.verdict == PUSH_ARG_NOT_STARTED) return BestCheck{BEST_ARG_NOT_STARTED, c.stream};
    for (int i = 0; i < n; ++i)
        if (S[(size_t)streams[i]].resident) return BestCheck{BEST_ARG_RESIDENT, streams[i]};
    return BestCheck{BEST_ARG_OK, -1};
}

struct BestLayout {
    size_t head_at, per, words;
    size_t reply_words(int n) const { return per * (size_t)n; }
};
static inline BestLayout best_layout(int max_streams)
{
    const size_t M = (size_t)max_streams, head_at = 4 * M, per = (size_t)BEST_HEAD + (size_t)BEST_FIELDS * BEST_SHARE;
    return BestLayout{head_at, per, head_at + per * M};
}

// the reply of a stream: no live emitting token; a chain longer than the result capacity (an error, the stream's alone); the chain from
// its share of the staging area; or, more than a share, from the stream's result arrays
enum BestReply { BEST_NOT_FOUND = 0, BEST_TOO_LONG, BEST_FROM_STAGE, BEST_FROM_RESULTS };
static inline BestReply best_reply(int found, int n_records, int res_cap)
{
    if (!found) return BEST_NOT_FOUND;
    if (n_records > res_cap) return BEST_TOO_LONG;
    return n_records <= BEST_SHARE ? BEST_FROM_STAGE : BEST_FROM_RESULTS;
}
// what the caller gets for a stream that has no hypothesis (not listed to the kernel, not found, or too long: the chain is not delivered)
static inline BestHead best_none(int frame) { return BestHead{0, frame, 0, 0, 0, 0, 0.0f, 0.0f, 0.0f}; }

static inline void best_clear(PushModels &M) { M.model.clear(); M.label.clear(); M.time.clear(); M.score.clear(); M.ac.clear(); M.lm.clear(); }
static inline void best_resize(PushModels &M, size_t n) { M.model.resize(n); M.label.resize(n); M.time.resize(n); M.score.resize(n); M.ac.resize(n); M.lm.resize(n); }
// ... the n records of a share of the staging area
static inline void best_take_stage(PushModels &M, int n, const int32_t *stage)
{
    best_resize(M, (size_t)n);
    if (n <= 0) return;
    const size_t b = (size_t)n * 4;
    memcpy(M.model.data(), stage + BEST_STAGE_WORD(0, 0), b); memcpy(M.label.data(), stage + BEST_STAGE_WORD(1, 0), b);
    memcpy(M.time.data(), stage + BEST_STAGE_WORD(2, 0), b); memcpy(M.score.data(), stage + BEST_STAGE_WORD(3, 0), b);
    memcpy(M.ac.data(), stage + BEST_STAGE_WORD(4, 0), b); memcpy(M.lm.data(), stage + BEST_STAGE_WORD(5, 0), b);
}
// ... or of the stream's result arrays: rows = [label, time, score, ac, lm][n] as fetched, models = the model row (null: word level, 0)
static inline void best_take_rows(PushModels &M, int n, const int32_t *rows, const int32_t *models)
{
    best_resize(M, (size_t)n);
    if (n <= 0) return;
    const size_t N = (size_t)n, b = N * 4;
    if (models) memcpy(M.model.data(), models, b);
    else memset(M.model.data(), 0, b);
    memcpy(M.label.data(), rows, b); memcpy(M.time.data(), rows + N, b);
    memcpy(M.score.data(), rows + 2 * N, b); memcpy(M.ac.data(), rows + 3 * N, b); memcpy(M.lm.data(), rows + 4 * N, b);
}

// The word projection of a list: its entries with a label, in order (on a word-level decoder every entry has one).  *n = how many
// there are; the first `cap` of them are written, each output where it is not null (jd_stream_partial's conventions).
static inline void best_words(const PushModels &M, int cap, int32_t *n, int32_t *label, int32_t *time, float *score, float *ac, float *lm)
{
    int w = 0;
    for (size_t k = 0; k < M.label.size(); ++k) {
        if (M.label[k] == 0) continue;
        if (w < cap) {
            if (label) label[w] = M.label[k];
            if (time) time[w] = M.time[k];
            if (score) score[w] = M.score[k];
            if (ac) ac[w] = M.ac[k];
            if (lm) lm[w] = M.lm[k];
        }
        ++w;
    }
    *n = w;
}
// ... and the list itself
static inline void best_models(const PushModels &M, int cap, int32_t *n, int32_t *model, int32_t *label, int32_t *time, float *score, float *ac, float *lm)
{
    *n = (int32_t)M.model.size();
    const size_t k = (size_t)(cap < *n ? (cap < 0 ? 0 : cap) : *n);
    if (!k) return;
    if (model) memcpy(model, M.model.data(), k * 4);
    if (label) memcpy(label, M.label.data(), k * 4);
    if (time) memcpy(time, M.time.data(), k * 4);
    if (score) memcpy(score, M.score.data(), k * 4);
    if (ac) memcpy(ac, M.ac.data(), k * 4);
    if (lm) memcpy(lm, M.lm.data(), k * 4);
}
