// jd_ahead.h - working ahead (jd_dec_prefetch_scores, "two batches in flight"): the queue of announced batches, their likelihood
// tables, the two banks of streams and the wave that consumes them, as DECISIONS - plain functions over plain structs, no HIP.
// jd_device.hip (decode_wave, pf_*, jd_decode_batch_device) and jd_host_launch.h make the HIP calls these decisions ask for;
// tests/ahead_driver.cpp runs them on the CPU (tests/test_ahead_cpu.py).  The queue is the device file's own std::deque of entries
// that derive from AheadEntry: the functions here are templates over it and never copy it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "jd_arena.h"

enum AheadState { AHEAD_NONE = 0, AHEAD_ANNOUNCED = 1, AHEAD_SCORED = 2 };   // SCORED: its scoring has been enqueued (table `buf`)
// jd_dec::fg_buf, the table(s) of the wave being decoded: one of 0..2, or
enum { FG_NONE = -1, FG_BOTH = -2 };               // none / tables 0 and 1, in chunks (nothing is scored ahead meanwhile)
enum { AHEAD_TABLES = 3, AHEAD_QUEUE_MAX = 3, AHEAD_PROBE_FRAMES = 32 };

// A batch announced with jd_dec_prefetch_scores, without its two events (jd_device.hip: Prefetch)
struct AheadEntry {
    AheadState state = AHEAD_NONE;
    const float *feats = nullptr;              // the feature buffer it was announced with (compared, never read here)
    int nb = 0;
    std::vector<int64_t> ustart, ulen;
    WavePlan plan;
    int buf = 0;                               // SCORED: its table
    int bank = -1;                             // >= 0: its utterances have been started, on this bank of streams
};

// ---- the queue's predicates
template <class Q> static inline bool ahead_any_scored(const Q &q)
{
    for (const AheadEntry &F : q) if (F.state == AHEAD_SCORED) return true;
    return false;
}
template <class Q> static inline bool ahead_any_started(const Q &q)
{
    for (const AheadEntry &F : q) if (F.bank >= 0) return true;
    return false;
}
template <class Q> static inline bool ahead_any_worked(const Q &q) { return ahead_any_scored(q) || ahead_any_started(q); }

// a table that neither the running wave (fg_buf) nor a batch scored ahead holds; -1: none.  (FG_BOTH matches no table: the callers
// see to it that nothing is scored beside a wave in chunks)
template <class Q> static inline int ahead_free_table(const Q &q, int fg_buf)
{
    for (int t = 0; t < AHEAD_TABLES; ++t) {
        bool used = t == fg_buf;
        for (const AheadEntry &F : q) if (F.state == AHEAD_SCORED && F.buf == t) used = true;
        if (!used) return t;
    }
    return -1;
}
// the first announced batch can be scored now: a table is free and the slab, which cannot grow while tables are in use, holds it
template <class Q> static inline bool ahead_wants_scoring(const Q &q, int fg_buf, size_t G, size_t ll_cap)
{
    for (const AheadEntry &F : q) if (F.state == AHEAD_ANNOUNCED) return ahead_free_table(q, fg_buf) >= 0 && F.plan.max_rows * G <= ll_cap;
    return false;
}
template <class Q> static inline double ahead_scoring_rows(const Q &q)
{
    double rows = 0.0;
    for (const AheadEntry &F : q) if (F.state == AHEAD_ANNOUNCED) rows += (double)F.plan.chunk_rows[0];
    return rows;
}

// ---- announcing.  A wave joins the queue (at most three; one more is silently not taken) when it fits the streams; one whose table
// would be cut into chunks is not announced.  In two steps, because the wave is laid out (plan_wave) between them.
static inline bool ahead_admits(int nb, int max_streams, size_t queued) { return nb > 0 && nb <= max_streams && queued < (size_t)AHEAD_QUEUE_MAX; }
template <class Q, class E> static inline bool ahead_enqueue(Q &q, E &&F, const float *feats, int nb, bool front)
{
    if (F.plan.n_chunks != 1) return false;
    F.feats = feats; F.nb = nb; F.state = AHEAD_ANNOUNCED;
    if (front) q.push_front(std::move(F)); else q.push_back(std::move(F));
    return true;
}

// ---- decode_wave.  claim: is this wave the one at the head of the queue?  Only a batch whose table has been scored ahead can be.
// If it is not, what has been scored or started ahead is for a batch that is not coming now and is dropped - unless the wave is
// being decoded again (retry), which finds the waves behind it there.  Announcements nothing was done for stay either way.
struct AheadClaim { bool mine, drop; };
template <class Q> static inline AheadClaim ahead_claim(const Q &q, const float *feats, int nb, const int64_t *ustart, const int64_t *ulen, bool retry)
{
    if (q.empty()) return {false, false};
    const AheadEntry &F = q.front();
    const bool mine = F.state == AHEAD_SCORED && F.feats == feats && F.nb == nb && std::equal(ustart, ustart + nb, F.ustart.begin()) &&
                      std::equal(ulen, ulen + nb, F.ulen.begin());
    return {mine, !mine && ahead_any_worked(q) && !retry};
}

// place: the streams the wave runs on.  A single-chunk wave that fills at most half of them runs on one of two banks (pipe), so
// that the batch behind it can be started beside it; a claimed batch that was started goes on where it is (resumed); otherwise
// bank 0, or 1 when a queued batch holds 0 (at most one does).  q: the queue without the claimed entry.
//   discard: a wave in chunks needs tables 0 and 1 - nothing scored or started ahead survives it
//   unbank:  a wave outside the banks takes the streams a batch behind it was started on - that batch starts again (its table stays)
struct AheadPlace { bool pipe, resumed, discard, unbank; int bank, s0; };
template <class Q> static inline AheadPlace ahead_place(const Q &q, int n_chunks, int nb, int max_streams, bool pipeline, bool lazy, bool mine, int my_bank)
{
    const int B = max_streams / 2;
    AheadPlace p{};
    p.pipe = pipeline && B > 0 && nb <= B && n_chunks == 1 && !lazy;
    p.discard = n_chunks > 1 && ahead_any_worked(q);
    p.unbank = !p.discard && !p.pipe && ahead_any_started(q);
    p.resumed = mine && p.pipe && my_bank >= 0;
    if (p.pipe) {
        p.bank = p.resumed ? my_bank : 0;
        if (!p.resumed) for (const AheadEntry &F : q) if (F.bank == p.bank) p.bank ^= 1;
    }
    p.s0 = p.pipe ? p.bank * B : 0;
    return p;
}

// tables of a wave that was not scored ahead, before the slab is grown: the floats per table - this wave's, or what a queued batch
// needs if that is more (the three tables are of one size) - and, when the slab has to grow (which loses what is in it), that the
// scored-ahead tables go first and an eighth of room is added.  A wave in chunks asks for its own size only.
struct AheadNeed { size_t floats; bool drop_scored; };
template <class Q> static inline AheadNeed ahead_table_need(const Q &q, size_t max_rows, size_t G, size_t ll_cap, bool chunked)
{
    size_t need = max_rows * G;
    if (chunked) return {need, false};
    for (const AheadEntry &F : q) need = std::max(need, F.plan.max_rows * G);
    if (need > ll_cap) return {need + need / 8, true};
    return {need, false};
}
// ... and after it: the table taken (chunks alternate between 0 and 1), or none free - everything ahead is dropped and it takes 0
struct AheadTake { int table; bool discard; };
template <class Q> static inline AheadTake ahead_table_take(const Q &q, bool chunked)
{
    const int t = chunked ? 0 : ahead_free_table(q, FG_NONE);
    return {std::max(t, 0), t < 0};
}

// chunk work: the {stream, first row in the chunk's table} of every stream with frames in chunk c, and the frames each has there
// (a launch lasts as long as its slowest stream: the clusters are sized by them).  frame0: where the streams stand (a batch started
// ahead is frames in).  Chunk 0 carries recognitionStart, so a stream at frame 0 is in it whatever its length.  Returns the frames.
template <class I2> static inline long long ahead_chunk_work(const WavePlan &P, int c, int s0, long long row0, const std::vector<int> &frame0,
                                                             std::vector<I2> *work, std::vector<double> *weight)
{
    const int c0 = c * P.Fc, c1 = (c + 1) * P.Fc;
    long long frames = 0;
    work->clear(); weight->clear();
    for (int u = 0; u < P.nb; ++u) {
        const int T = P.T[(size_t)u], from = std::max(c0, frame0[(size_t)u]);
        if ((c == 0 && frame0[(size_t)u] == 0) || T > from) {
            I2 w; w.x = s0 + u; w.y = (int)(row0 + P.row_off[(size_t)c * P.nb + u]);
            work->push_back(w);
            weight->push_back((double)(std::min(T, c1) - from));
            frames += std::min(T, c1) - from;
        }
    }
    return frames;
}
// The decoder's very first batch: nothing is known about the load yet and the cluster sizes depend on it - a launch of 32 frames
// finds out.  When it applies, its weights, and what is left of the chunk's work behind it.
static inline bool ahead_probe_applies(double load_scale, bool weighted, int c, const WavePlan &P, bool resumed)
{
    return load_scale == 1.0 && weighted && c == 0 && P.nb > 1 && std::min(P.maxT, (c + 1) * P.Fc) - c * P.Fc > 128 && !resumed;
}
static inline std::vector<double> ahead_probe_weights(const std::vector<double> &weight)
{
    std::vector<double> wp(weight.size());
    for (size_t i = 0; i < wp.size(); ++i) wp[i] = std::min(weight[i], (double)AHEAD_PROBE_FRAMES);
    return wp;
}
template <class I2> static inline void ahead_probe_rest(const WavePlan &P, int c, int s0, std::vector<I2> *work, std::vector<double> *weight)
{
    const int c_mid = c * P.Fc + AHEAD_PROBE_FRAMES, c1 = (c + 1) * P.Fc;
    std::vector<I2> w2; std::vector<double> wt2;
    for (const I2 &w : *work) {
        const int T = P.T[(size_t)(w.x - s0)];
        if (T > c_mid) { w2.push_back(w); wt2.push_back((double)(std::min(T, c1) - c_mid)); }
    }
    work->swap(w2); weight->swap(wt2);
}

// ---- the batch behind the running one (pf_background).  Searching ahead pays where a frame is a chain of dependent steps and
// workgroups wait - not where it is bytes: a stream-frame of several hundred thousand instances keeps every workgroup it can get busy,
// and a second batch on the same chip only splits them (measured: the 14 M-arc graph 119 k -> 55 k frames/s, configs[3] 5.3 k ->
// 0.8 k).  The decoder knows its load from the batches it has decoded (load_scale: instances + arcs per stream-frame over
// configs[1]'s 23.7 k); beyond bg_max_load times that the batch behind waits for its turn.
enum AheadBg { AHEAD_BG_NONE = 0, AHEAD_BG_START, AHEAD_BG_GO_ON };   // nothing / start the head (once its table is ready) / it has been started
template <class Q> static inline AheadBg ahead_bg_step(const Q &q, bool pipeline, bool lazy, double load_scale, double bg_max_load, int max_streams)
{
    if (q.empty() || !pipeline || lazy || load_scale > bg_max_load) return AHEAD_BG_NONE;
    const AheadEntry &F = q.front();
    if (F.state != AHEAD_SCORED || F.nb > max_streams / 2 || F.plan.n_chunks != 1) return AHEAD_BG_NONE;
    return F.bank < 0 ? AHEAD_BG_START : AHEAD_BG_GO_ON;
}
// Its streams as work items for the launch being planned and the frames each has left.  heads: null right after the start (every
// utterance, all its frames), else the heads of every stream as of now (the unfinished ones; a stream in error is left alone).
template <class I2, class H> static inline void ahead_bg_work(const AheadEntry &F, int s0, long long row0, const std::vector<H> *heads,
                                                             std::vector<I2> *work, std::vector<double> *left)
{
    for (int u = 0; u < F.nb; ++u) {
        const int T = F.plan.T[(size_t)u], at = heads ? (*heads)[(size_t)(s0 + u)].frame : 0;
        if (heads && !((*heads)[(size_t)(s0 + u)].error == 0 && at < T)) continue;
        I2 w; w.x = s0 + u; w.y = (int)(row0 + F.plan.row_off[(size_t)u]);
        work->push_back(w);
        left->push_back((double)(T - at));
    }
}
// launch_search: one workgroup each at least, on a quarter of the grid at most, and the running batch keeps two per stream
static inline bool ahead_bg_clipped(int n_bg, int n_work, int nwg_all) { return n_bg > nwg_all / 4 || nwg_all - n_bg < 2 * n_work; }

// CUs left to a scoring beside a launch with two batches in flight: as set (score_reserve >= 0), else as many as carry its cost
// over a launch as long as the last wave was; a multiple of eight (the XCD-local numbering), a third of the chip at most
static inline int ahead_reserve(int score_reserve, double gmm_ms_per_row, double last_wave_ms, double rows, int nwg_all)
{
    int r = score_reserve;
    if (r < 0) r = (gmm_ms_per_row > 0.0 && last_wave_ms > 0.0) ? (int)std::ceil(gmm_ms_per_row * rows * nwg_all / last_wave_ms) : 0;
    return std::min((r + 7) & ~7, (nwg_all / 3) & ~7);
}
// a launch beside which a table is scored is not cut short for a re-plan while that scoring runs: never (pf_rebalance 1), always
// (0), or (-1) when the scoring is a tenth of the search or more by the costs measured on this decoder's last waves
static inline bool ahead_hold_replan(int pf_rebalance, double gmm_ms_per_row, double rows, double search_ms_per_frame, double frames_now)
{
    const double est_gmm = gmm_ms_per_row * rows, est_search = search_ms_per_frame * frames_now;
    return pf_rebalance == 0 || (pf_rebalance < 0 && est_gmm > 0.0 && est_search > 0.0 && est_gmm >= 0.1 * est_search);
}

// ---- jd_decode_batch_device.  More utterances than streams: successive waves.  A wave lasts as long as its longest utterance, so
// the waves are formed from the utterances sorted by length (stable; results do not depend on which utterances share a wave).
static inline std::vector<int> ahead_wave_order(const int64_t *offs, int n_utts, int max_streams)
{
    std::vector<int> order((size_t)n_utts);
    std::iota(order.begin(), order.end(), 0);
    if (n_utts > max_streams)
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return offs[a + 1] - offs[a] > offs[b + 1] - offs[b]; });
    return order;
}
// the wave that begins at order[u0]: its utterances' first frames and lengths; returns how many (0: there is none)
static inline int ahead_wave_slice(const int64_t *offs, const std::vector<int> &order, int u0, int max_streams, int64_t *ustart, int64_t *ulen)
{
    const int nb = std::max(0, std::min(max_streams, (int)order.size() - u0));
    for (int i = 0; i < nb; ++i) {
        const int u = order[(size_t)(u0 + i)];
        ustart[i] = offs[u]; ulen[i] = offs[u + 1] - offs[u];
    }
    return nb;
}
// The load of a batch - instances + arcs per stream-frame over configs[1]'s 23.7 k - scales the cost model's b (jd_dec::load_scale):
// the first batch sets it, later ones are averaged in
static inline double ahead_load(double work, double frames) { return std::min(1e5, std::max(0.25, work / frames / 23700.0)); }
static inline double ahead_load_update(double load_scale, double load_sum, double load_frames)
{
    if (!(load_frames > 0.0)) return load_scale;
    const double scale = ahead_load(load_sum, load_frames);
    return load_scale == 1.0 ? scale : 0.5 * (load_scale + scale);
}

// ---- JD_VERBOSE: the queue as "state,buf,bank,nb,max_rows,same;..." (same: announced with these features, starts and lengths)
template <class Q> static inline std::string ahead_describe(const Q &q, const float *feats, int nb, const int64_t *ustart, const int64_t *ulen)
{
    std::string s;
    for (const AheadEntry &F : q) {
        const bool same = F.feats == feats && F.nb == nb && std::equal(ustart, ustart + nb, F.ustart.begin()) && std::equal(ulen, ulen + nb, F.ulen.begin());
        char b[96];
        snprintf(b, sizeof b, "%s%d,%d,%d,%d,%zu,%d", s.empty() ? "" : ";", (int)F.state, F.buf, F.bank, F.nb, F.plan.max_rows, same ? 1 : 0);
        s += b;
    }
    return s.empty() ? "-" : s;
}
