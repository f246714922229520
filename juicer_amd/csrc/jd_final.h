// jd_final.h - the end-of-utterance view of live streams (jd_streams_final, jd_stream_final_words / _models): the hypothesis
// jd_stream_finish would return right now - bestFinalToken's Path chain with the final-state weight - read without ending the
// utterance, as DECISIONS: the request of a stream, the layout of k_final_many's buffers (jd_gc.h), what a reply means, the argument
// check, taking a list from a share or from the result rows, and the word projection.  Plain functions over plain structs, no HIP:
// jd_host_stream.h makes the copies and the launch; tests/final_driver.cpp runs them on the CPU (tests/test_final_cpu.py).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "jd_best.h"            // PushModels' helpers (best_clear, best_resize, best_take_rows, best_words, best_models), best_check

// ---- k_final_many's buffers, for max_streams entries: [int4 work list][heads: FINAL_HEAD words per entry][staging: FINAL_SHARE
// records of FINAL_FIELDS words per entry, field-major].  A launch of n entries writes its n heads and, behind them, its n shares, and
// the host fetches reply_words(n) in ONE copy.
// FINAL_SHARE: BEST_SHARE's reasoning (jd_best.h) holds word for word - the hypothesis is sent whole at every call, because the best
// final token of this frame need not continue the one of the frame before (it is revised, not extended), and it is a chain of the
// same arena seen from a final state instead of an emitting one: a few dozen records at model level for a live utterance of a few
// hundred frames, fewer at word level.  64 records (1.5 KiB per stream, 24 KiB a copy for sixteen callers) take those; a longer chain
// is fetched from the stream's result arrays instead.
#define FINAL_SHARE 64
#define FINAL_FIELDS 6          // model, label, time, score, ac, lm (the fields of jd_model_hyp)
#define FINAL_HEAD 8            // found, frame, n_words, n_records, score, ac, lm, 1 spare: the first seven are jd_final
#define FINAL_THREADS 256       // k_final_many's workgroup (why: at the kernel)
// where entry i's share begins in the words a launch of n entries writes, and field f of record k inside a share (kernel and host)
#define FINAL_STAGE_AT(n, i) ((size_t)FINAL_HEAD * (size_t)(n) + (size_t)(FINAL_FIELDS * FINAL_SHARE) * (size_t)(i))
#define FINAL_STAGE_WORD(f, k) ((size_t)(f) * FINAL_SHARE + (size_t)(k))

// the head of an entry as the kernel writes it (the host fills `frame`: the frames pushed); jd_final of the C ABI is the same seven words
struct FinalHead { int32_t found, frame, n_words, n_records; float score, ac, lm; };
static_assert(sizeof(FinalHead) == 7 * 4 && sizeof(FinalHead) <= FINAL_HEAD * 4, "k_final_many writes the head word by word");

// the request of a stream: {stream, -, -, -}
struct FinalRequest { int32_t stream, pad0, pad1, pad2; };
static inline FinalRequest final_request(int s) { return FinalRequest{s, 0, 0, 0}; }

// jd_streams_final's entries are checked as jd_streams_best's are (best_check): each stream once, in range, started by
// jd_stream_init, not a broker's.  ss / at: the streams that have a frame to look behind and their places in the list.
static inline BestCheck final_check(const std::vector<PushStream> &S, int n, const int32_t *streams, std::vector<int> *ss, std::vector<int> *at)
{
    return best_check(S, n, streams, ss, at);
}

struct FinalLayout {
    size_t head_at, per, words;
    size_t reply_words(int n) const { return per * (size_t)n; }
};
static inline FinalLayout final_layout(int max_streams)
{
    const size_t M = (size_t)max_streams, head_at = 4 * M, per = (size_t)FINAL_HEAD + (size_t)FINAL_FIELDS * FINAL_SHARE;
    return FinalLayout{head_at, per, head_at + per * M};
}

// the reply of a stream: no token in a final state; a chain longer than the result capacity (an error, the stream's alone); the chain
// from its share of the staging area; or, more than a share, from the stream's result arrays
enum FinalReply { FINAL_NOT_FOUND = 0, FINAL_TOO_LONG, FINAL_FROM_STAGE, FINAL_FROM_RESULTS };
static inline FinalReply final_reply(int found, int n_records, int res_cap)
{
    if (!found) return FINAL_NOT_FOUND;
    if (n_records > res_cap) return FINAL_TOO_LONG;
    return n_records <= FINAL_SHARE ? FINAL_FROM_STAGE : FINAL_FROM_RESULTS;
}
// what the caller gets for a stream that has no final hypothesis (not listed to the kernel, not found, or too long)
static inline FinalHead final_none(int frame) { return FinalHead{0, frame, 0, 0, 0.0f, 0.0f, 0.0f}; }

// ... the n records of a share of the staging area
static inline void final_take_stage(PushModels &M, int n, const int32_t *stage)
{
    best_resize(M, (size_t)n);
    if (n <= 0) return;
    const size_t b = (size_t)n * 4;
    memcpy(M.model.data(), stage + FINAL_STAGE_WORD(0, 0), b); memcpy(M.label.data(), stage + FINAL_STAGE_WORD(1, 0), b);
    memcpy(M.time.data(), stage + FINAL_STAGE_WORD(2, 0), b); memcpy(M.score.data(), stage + FINAL_STAGE_WORD(3, 0), b);
    memcpy(M.ac.data(), stage + FINAL_STAGE_WORD(4, 0), b); memcpy(M.lm.data(), stage + FINAL_STAGE_WORD(5, 0), b);
}
// ... or of the stream's result arrays (best_take_rows: rows = [label, time, score, ac, lm][n] as fetched, models = the model row or null)
static inline void final_take_rows(PushModels &M, int n, const int32_t *rows, const int32_t *models) { best_take_rows(M, n, rows, models); }

// The word projection of the list (best_words), as jd_stream_finish makes the word result of a model-level decode: the entries
// with a label, and the NEWEST of them carries the hypothesis' totals (the final-state weight is the word result's too,
// fetch_results; at word level the newest entry is the chain's last record and has them already).  tot: the head's score, ac, lm.
static inline void final_words(const PushModels &M, const float tot[3], int cap, int32_t *n, int32_t *label, int32_t *time, float *score, float *ac, float *lm)
{
    best_words(M, cap, n, label, time, score, ac, lm);
    const int w = *n;
    if (w <= 0 || w > cap) return;
    if (score) score[w - 1] = tot[0];
    if (ac) ac[w - 1] = tot[1];
    if (lm) lm[w - 1] = tot[2];
}
// ... and the list itself
static inline void final_models(const PushModels &M, int cap, int32_t *n, int32_t *model, int32_t *label, int32_t *time, float *score, float *ac, float *lm)
{
    best_models(M, cap, n, model, label, time, score, ac, lm);
}
