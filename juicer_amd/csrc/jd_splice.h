// jd_splice.h - context splicing of neural acoustic models (jd_am_mlp_splice) as plain data: its limits and argument check, the
// definition of the window, the ROW SPAN that a row of a spliced launch carries beside row_src, the spans of a batch, the PUSH PLAN of
// a live stream, and the host twin.  Pure: no HIP, no device, no library state - tests/splice_driver.cpp includes it under plain g++
// (tests/test_splice_cpu.py).
//
// The model.  A spliced model is its parent's network on a window of frames: its feature vectors hold D = in_dim / C values,
// C = left + right + 1, and the network's input for frame t of an utterance of T frames is
//   x[c D + d] = frame[clamp(t + c - left, 0, T - 1)][d]      c = 0 .. C - 1  (the oldest frame first; the edges repeat)
// After the gather the arithmetic is the parent's (jd_mlp_forward_row / jd_mlp_bf16_forward_row on the gathered vector): a spliced
// model on raw frames gives, bit for bit, what its parent gives on the same frames spliced by the caller.
//
// The row span.  Beside row_src[r], the CENTRE frame of row r in the launch's feature buffer, a spliced launch carries
// JdSpan span[r] = {lo, hi}: the first and the last frame of that buffer the row may read - its utterance's bounds there.  Piece c
// of the row is frame jd_splice_frame(row_src[r], c, left, span[r]) = clamp(row_src[r] + c - left, lo, hi): whatever row_src says,
// a read stays inside [lo, hi].  A row with row_src < 0 is unused and its span is not read.
//
// A batch (splice_wave_spans).  Whole utterances lie back to back in the feature buffer, so utterance u's rows - in every chunk of
// the likelihood tables - carry {ustart[u], ustart[u] + T[u] - 1}: a window crosses a chunk's edge freely.
//
// A live stream (splice_push_plan).  A frame becomes a row once `right` more frames have been pushed; at the finish the rest become
// rows with the right edge clamped.  With P0 frames pushed before and n now, rows are the absolute frames [rel0, rel1),
//   rel(P, finishing) = finishing ? P : max(0, P - right),    rel0 = rel(P0, false), rel1 = rel(P0 + n, finishing)
// and the stream keeps the frames a later row can still read: [keep(rel), P), keep(rel) = max(0, rel - left) - at most left + right
// while it is open.  The staging buffer of a push is the kept frames [keep(rel0), P0) in front of the n new ones; absolute frame f is
// its frame f - keep(rel0), and every row's span is the whole buffer {0, n_buf - 1}: frame 0 of the buffer is the utterance's frame 0
// whenever a window reaches that far back, and its last frame is the utterance's last at the finish (before it, no window reaches
// behind it).
#ifndef JD_SPLICE_H
#define JD_SPLICE_H

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "jd_arena.h"           // WavePlan: the rows of a batch
#include "jd_mlp.h"
#include "jd_mlp_bf16.h"

#define JD_SPLICE_MAX_CONTEXT (JD_MLP_MAX_DIM - 1)   // left + right: C <= in_dim <= JD_MLP_MAX_DIM

struct JdSpan { int32_t lo, hi; };                 // frames of the launch's feature buffer, inclusive

// 0, or why (left, right) cannot splice a network of in_dim inputs (msg names the cause); *D: the frames' size
static inline int jd_splice_check(int in_dim, int left, int right, int *D, char *msg, size_t cap)
{
    if (left < 0 || right < 0) { snprintf(msg, cap, "context (%d, %d): left and right are frames, 0 or more", left, right); return 1; }
    const long long C = (long long)left + right + 1;
    if (C > in_dim || in_dim % (int)C != 0) {
        snprintf(msg, cap, "in_dim = %d is not a multiple of left + right + 1 = %lld frames", in_dim, C);
        return 2;
    }
    if (D) *D = in_dim / (int)C;
    return 0;
}

// the frame of piece c of a row whose centre frame is `centre`
static JD_MLP_HD int jd_splice_frame(int centre, int c, int left, const JdSpan s)
{
    const int f = centre + c - left;
    return f < s.lo ? s.lo : (f > s.hi ? s.hi : f);
}

// what a spliced kernel is told beside its unspliced twin's JdMlpDev (m.in_dim stays the network's), and the LDS its tile's spans take
// behind the unspliced kernel's (rows: JD_MLP_ROWS / JD_MLP_BF16_ROWS)
static inline JdMlpDev jd_splice_dev(JdMlpDev m, int left, int right)
{
    m.base_dim = m.in_dim / (left + right + 1); m.left = left; m.right = right;
    return m;
}
static inline size_t jd_splice_lds_bytes(int rows) { return (size_t)rows * sizeof(JdSpan); }

// the network's input of a row: x[C D] from frames [.][D]
static inline void jd_splice_gather(const float *frames, int D, int left, int right, int centre, const JdSpan s, float *x)
{
    const int C = left + right + 1;
    for (int c = 0; c < C; ++c) {
        const float *f = frames + (size_t)jd_splice_frame(centre, c, left, s) * D;
        for (int d = 0; d < D; ++d) x[(size_t)c * D + d] = f[d];
    }
}

// ---- a batch: span[r] for every entry of P.row_src (unused rows: {0, 0}, never read)
static inline void splice_wave_spans(const WavePlan &P, const int64_t *ustart, std::vector<JdSpan> *span)
{
    span->assign(P.n_rows_all, JdSpan{0, 0});
    for (int c = 0; c < P.n_chunks; ++c)
        for (int u = 0; u < P.nb; ++u) {
            const int n = std::max(0, std::min(P.T[(size_t)u], (c + 1) * P.Fc) - c * P.Fc);
            JdSpan *dst = span->data() + P.chunk_row0[(size_t)c] + (size_t)P.row_off[(size_t)c * P.nb + u];
            const JdSpan s{(int32_t)ustart[u], (int32_t)(ustart[u] + P.T[(size_t)u] - 1)};
            for (int dt = 0; dt < n; ++dt) dst[dt] = s;
        }
}

// ---- a live stream
struct SplicePush {
    int n_front = 0;            // kept frames in front of the new ones in the staging buffer
    int n_buf = 0;              // frames of the staging buffer: n_front + the new ones
    int buf_frame0 = 0;         // the absolute frame of the buffer's frame 0
    int row_first = 0, n_rows = 0;      // the absolute frames that become rows now: [row_first, row_first + n_rows)
    int row_buf = 0;            // ... the first one's place in the buffer
    JdSpan span{0, 0};          // every row's span, in buffer frames
    int keep_first = 0, n_keep = 0;     // the absolute frames the stream keeps behind this push: [keep_first, keep_first + n_keep)
    int held = 0;               // frames pushed and not yet rows
};
static inline int splice_released(int left, int right, int pushed, bool finishing) { (void)left; return finishing ? pushed : std::max(0, pushed - right); }
static inline int splice_keep_first(int left, int released) { return std::max(0, released - left); }
static inline SplicePush splice_push_plan(int left, int right, int pushed_before, int n_new, bool finishing)
{
    SplicePush p;
    const int rel0 = splice_released(left, right, pushed_before, false), keep0 = splice_keep_first(left, rel0);
    const int pushed = pushed_before + n_new, rel1 = splice_released(left, right, pushed, finishing);
    p.n_front = pushed_before - keep0;
    p.n_buf = p.n_front + n_new;
    p.buf_frame0 = keep0;
    p.row_first = rel0; p.n_rows = rel1 - rel0;
    p.row_buf = rel0 - keep0;
    p.span = JdSpan{0, std::max(0, p.n_buf - 1)};
    p.keep_first = splice_keep_first(left, rel1); p.n_keep = pushed - p.keep_first;
    p.held = pushed - rel1;
    return p;
}
// The piece of the staging buffer that rows [row, row + n) of it read (a chunk of a push goes up on its own): frames [*b0, *b1)
static inline void splice_rows_window(int left, int right, const JdSpan s, int row, int n, int *b0, int *b1)
{
    *b0 = std::max((int)s.lo, row - left);
    *b1 = std::min((int)s.hi + 1, row + n + right);
}

// ---- the host twin: rows of ONE utterance (frames [n][D], spans {0, n - 1}), or of a row map with spans
// bf16: jd_mlp_bf16_forward_row's numerics, else jd_mlp_forward_row's.  out [n_rows][width[stop_layer]] / [n_rows][n_phones]
template <class M>
static inline void jd_splice_forward_host(const JdMlpDesc &d, int left, int right, bool bf16, const float *w, const float *b, const float *log_prior,
                                          const float *frames, int n_frames, int stop_layer, float *out, const M &math, bool tied)
{
    const int C = left + right + 1, D = d.in_dim / C;
    const int ow = stop_layer >= 0 ? d.width[stop_layer] : d.width[d.n_layers - 1];
    std::vector<float> x((size_t)d.in_dim);
    const JdSpan s{0, n_frames - 1};
    for (int r = 0; r < n_frames; ++r) {
        jd_splice_gather(frames, D, left, right, r, s, x.data());
        if (bf16) jd_mlp_bf16_forward_row(d, w, b, log_prior, x.data(), stop_layer, out + (size_t)r * ow, math, tied);
        else jd_mlp_forward_row(d, w, b, log_prior, x.data(), stop_layer, out + (size_t)r * ow, math, tied);
    }
}
#endif
