// jd_arena.h - how large a stream's arenas are, where each piece of them sits in the stream's share of the slab, and how a wave of
// utterances is laid out in likelihood tables, as functions of plain data (no device runtime, no decoder: compiled and tested on the CPU,
// tests/test_arena_cpu.py).  The decoder's ensure_arenas_try and plan_wave ask the runtime for the free memory, call these, and
// allocate what they say.  What the kernels' structs weigh comes in as numbers (ArenaSizes), filled from sizeof where the structs are.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// ------------------------------------------------------------------------------------------------ a stream's arenas

struct ArenaSizes {
    int64_t rec_bytes_small, rec_bytes_large;   // an instance record of models of up to 5 states / of more (RecLayout<3>, <6>)
    size_t path_rec, tok, item, state_rec;      // PathRec, Tok, a frontier item's second half (int4), StateRec
    int gc_words;                               // GcState, in ints
    int tot_n, maxw, hist_bins, sw;             // TOT_N, MAXW, HIST_MAX_BINS, SW
};

// the pieces of a stream's share, in the order they lie in it
enum { AR_REC, AR_LIVE, AR_SREC, AR_ITEMS, AR_NEWL, AR_DIRTYL, AR_TOT, AR_ITEM_END, AR_PATHS, AR_PATHS2, AR_GC_IDX, AR_GC_STATE, AR_HIST, AR_N };

struct ArenaDims {
    int64_t cap_slots, cap_items, cap_paths, cap_new;
    int64_t n_arcs, n_states;
    int max_n;                                  // most states of a model: which record layout
    ArenaSizes z;
};

static inline int64_t arena_rec_bytes(const ArenaSizes &z, int max_n) { return max_n <= 5 ? z.rec_bytes_small : z.rec_bytes_large; }

// A stream's arenas are 256-byte aligned pieces of one block, each of at least one element: off[piece] is where it starts.
// Returns the bytes of the block.
static inline size_t arena_layout(const ArenaDims &a, size_t off[AR_N])
{
    const int64_t rec_bytes = arena_rec_bytes(a.z, a.max_n);
    const struct { int64_t n; size_t elem; } piece[AR_N] = {
        /* AR_REC      */ {2 * a.cap_slots * (rec_bytes / 4), sizeof(int)},
        /* AR_LIVE     */ {a.n_arcs, 1},
        /* AR_SREC     */ {a.n_states, a.z.state_rec},
        /* AR_ITEMS    */ {4 * a.cap_items, a.z.item},
        /* AR_NEWL     */ {a.cap_new, 2 * sizeof(int)},
        /* AR_DIRTYL   */ {2 * a.cap_new, sizeof(int)},
        /* AR_TOT      */ {(int64_t)a.z.tot_n * a.z.maxw, sizeof(int)},
        /* AR_ITEM_END */ {a.z.maxw, sizeof(int)},
        /* AR_PATHS    */ {a.cap_paths, a.z.path_rec},
        /* AR_PATHS2   */ {a.cap_paths, a.z.path_rec},
        /* AR_GC_IDX   */ {a.cap_paths, sizeof(int)},
        /* AR_GC_STATE */ {a.z.gc_words, sizeof(int)},
        /* AR_HIST     */ {2 * (int64_t)a.z.hist_bins, sizeof(int)},
    };
    size_t at = 0;
    for (int p = 0; p < AR_N; ++p) {
        off[p] = at;
        at += (std::max<size_t>((size_t)piece[p].n, 1) * piece[p].elem + 255) & ~(size_t)255;
    }
    return at;
}

struct ArenaIn {
    size_t free_bytes;                          // free device memory (without the cached slab)
    size_t cached_bytes;                        // the slab a previous decoder left on the device (0: none)
    double mem_fraction;                        // the part of both that all streams together may take
    int B;                                      // streams
    int64_t n_arcs, n_states;
    int Fc, n_gmm, max_n;                       // frames of a streaming chunk, tied states, most states of a model
    int64_t cap_slots, cap_items, cap_paths;    // set by the caller (<= 0: not set)
    int64_t slots_hint;                         // jd_dec_set_max_alloc_models
    ArenaSizes z;
};

enum ArenaStatus { ARENA_OK = 0, ARENA_TOO_LARGE };

struct ArenaCaps {
    ArenaStatus status;
    int64_t cap_slots, cap_items, cap_paths, cap_new;   // (ARENA_TOO_LARGE: the first three as picked, cap_new 0)
    int64_t gc_threshold;
    int64_t lim_rec, lim_item;                  // the addressing limits of records and items
    int passes;                                 // fit passes run
};

static inline void arena_caps(const ArenaIn &in, ArenaCaps *out)
{
    const int B = in.B, SW = in.z.sw;
    const int64_t rec_bytes = arena_rec_bytes(in.z, in.max_n);
    const bool auto_slots = in.cap_slots <= 0, auto_items = in.cap_items <= 0, auto_paths = in.cap_paths <= 0;
    const int64_t lim_rec = (0xe0000000LL / (2 * rec_bytes)) & ~63LL, lim_item = 0xe0000000LL / 64;
    *out = ArenaCaps();
    out->lim_rec = lim_rec; out->lim_item = lim_item;
    // The slab a previous decoder left on this device (slab_take) is there without waiting for the driver to clear
    // memory - 5-6 s for the default share of a 288 GB device - but only if this decoder's arenas FIT it, and two
    // decoders never ask for quite the same: the free memory has moved by a table or a network since.  So when the
    // sizes come out above the cached slab by a few per cent (up to 6: a smaller Path arena means more collections - the
    // 14 M-arc bench graph lost 4 % of its throughput to arenas fitted to a slab a fifth short), they are scaled down
    // to it (further passes).  What a pass made of a capacity the caller set - raised to a cluster's least, rounded - is what the
    // next pass counts with.
    double fit = 1.0;
    int64_t cap_slots = in.cap_slots, cap_items = in.cap_items, cap_paths = in.cap_paths;
    for (int pass = 0; pass < 3; ++pass) {
        out->passes = pass + 1;
        if (pass) { if (auto_slots) cap_slots = 0; if (auto_items) cap_items = 0; if (auto_paths) cap_paths = 0; }
        // Capacities the caller did not set: sized for 288 GB of HBM, not for frugality.  70% of the
        // free memory is split over the streams; of a stream's share (after its per-arc / per-state
        // tables) 50% goes to instance records, 20% to frontier items, 30% to Path records - each
        // between a floor that suits narrow beams and the most the graph can ever need.  Record and
        // item arenas are addressed with 32-bit byte offsets (buffer descriptors): < 4 GiB each.
        const size_t free_b = in.free_bytes + in.cached_bytes;        // (the cached slab is this decoder's to take)
        const double n_arcs = (double)in.n_arcs, n_states = (double)in.n_states;
        const double fixed = n_arcs * 1.0 + n_states * (double)in.z.state_rec + 2.0 * in.Fc * in.n_gmm * sizeof(float);
        const double budget = std::max(0.0, fit * in.mem_fraction * (double)free_b / B - fixed);
        const double rec_b = 2.0 * rec_bytes, item_b = 2.0 * (in.z.tok + in.z.item) + 32.0;
        const double path_b = 2.0 * in.z.path_rec + 4.0;
        auto pick = [](double share, int64_t lo, int64_t hi) {
            return std::max<int64_t>(std::min<int64_t>(hi, (int64_t)share), std::min(lo, hi));
        };
        if (cap_slots <= 0) {
            cap_slots = pick(0.5 * budget / rec_b, 1 << 19, std::min<int64_t>(in.n_arcs + 65536, lim_rec));
            if (in.slots_hint > cap_slots) cap_slots = std::min<int64_t>(in.slots_hint, lim_rec);   // setMaxAllocModels: more room, never less
        }
        if (cap_items <= 0)
            cap_items = pick(0.2 * budget / item_b, 1 << 21, std::min<int64_t>(std::max<int64_t>(2 * in.n_arcs + 65536, 1 << 21), lim_item));
        // (records and items stop at their addressing limits: what they leave of the budget goes to the Path
        // records - every collection of those is a stop of the stream's launch - up to 16 per arc of the
        // graph: small graphs do not write more, and tens of GB take seconds to allocate)
        if (cap_paths <= 0)
            cap_paths = pick(std::max(0.3 * budget, budget - (double)cap_slots * rec_b - (double)cap_items * item_b) / path_b,
                             1 << 21, std::min<int64_t>(0x40000000LL, std::max<int64_t>(1 << 24, 16 * in.n_arcs)));
        out->cap_slots = cap_slots; out->cap_items = cap_items; out->cap_paths = cap_paths;
        if (cap_slots > lim_rec || cap_items > lim_item || cap_paths > 0x7fffff00LL) { out->status = ARENA_TOO_LARGE; return; }
        // every wave of a stream's cluster owns 1/NW of each arena; small arenas limit the cluster
        // size instead (launch_search), down to one workgroup per stream
        out->cap_slots = cap_slots = std::max<int64_t>(cap_slots, 64 * SW) & ~63LL;
        out->cap_items = cap_items = std::max<int64_t>(cap_items, 64 * SW);
        out->cap_new = std::min<int64_t>(4 * cap_items, 0x7fffff00LL);
        size_t off[AR_N];
        const ArenaDims dims = {out->cap_slots, out->cap_items, out->cap_paths, out->cap_new, in.n_arcs, in.n_states, in.max_n, in.z};
        const double need = (double)arena_layout(dims, off) * B, cached = (double)in.cached_bytes;
        if (cached <= 0.0 || need <= cached || need > 1.06 * cached || !(auto_slots || auto_items || auto_paths)) break;
        fit *= 0.998 * cached / need;
    }
    // a stream stops for a collection when its Path records pass this mark (checked between frames): half
    // of a small arena, all but the larger of an eighth / 4 M records of a large one (a frame writes at
    // most one record per frontier item; running out anyway is the JD_ENOMEM that names the arena)
    out->gc_threshold = std::max<int64_t>(out->cap_paths / 2, out->cap_paths - std::max<int64_t>(out->cap_paths / 8, 4 << 20));
}

// ------------------------------------------------------------------------------------------------ a wave's likelihood tables

// How one wave of utterances is laid out in likelihood tables (wave_layout): frames per chunk, the rows of every chunk
// (stream after stream, packed) and the source frame of every row.
struct WavePlan {
    int nb = 0, Fc = 128, n_chunks = 1, maxT = 0;
    std::vector<int> T;                        // frames per stream
    std::vector<size_t> chunk_row0;            // first entry of chunk c in row_src
    // [chunk][stream]: first row of the stream in the chunk's table; rows per chunk (a multiple of the scoring tile)
    std::vector<int> row_off, chunk_rows;
    std::vector<int> row_src;                  // row -> frame of d_feats (-1: unused)
    size_t max_rows = 0, n_rows_all = 0;
};

struct WaveIn {
    int nb;                                    // utterances of the wave (<= max_streams)
    const int64_t *ustart, *ulen;              // first frame and frames of each
    size_t free_bytes;                         // free device memory
    size_t ll_cap;                             // floats per likelihood table as allocated
    int G;                                     // tied states
    int fc_env;                                // JD_FC: frames per chunk (0: decided here)
    int tile;                                  // rows of a scoring tile (GMM_ROWS2)
};

enum WaveCode { WAVE_OK = 0, WAVE_BAD_LENGTH, WAVE_CHUNK_ROWS, WAVE_BATCH_FRAMES };
struct WaveStatus { WaveCode code; int utt; };         // utt: the utterance of WAVE_BAD_LENGTH (else -1)

// Lay a wave of nb <= max_streams utterances out in likelihood tables.
// Frames per chunk.  A search launch lasts as long as its slowest stream and streams do not wait
// for each other inside a launch, so the fewer launches the better: one chunk covers the longest
// utterance when the likelihood table (frames of the batch x tied states floats, 288 GB of HBM to
// draw on) fits a quarter of the free memory; otherwise the batch is decoded in several chunks,
// scored alternately into two tables.  A chunk's table holds the frames the streams really have
// in it, packed stream after stream (only the last 128-row scoring tile of a chunk is partly empty).
static inline WaveStatus wave_layout(const WaveIn &in, WavePlan *plan)
{
    const int nb = in.nb, G = in.G, tile = in.tile;
    WavePlan &P = *plan;
    P = WavePlan();
    P.nb = nb;
    P.T.assign((size_t)nb, 0);
    long long sumT = 0;
    for (int u = 0; u < nb; ++u) {
        const int64_t t = in.ulen[u];
        if (t < 0 || t > 0x3fffffff) return {WAVE_BAD_LENGTH, u};
        P.T[(size_t)u] = (int)t;
        P.maxT = std::max(P.maxT, (int)t);
        sumT += t;
    }
    int Fc = std::max(128, (P.maxT + 127) / 128 * 128);
    {
        // (three tables of one size are kept: ensure_slab)
        const double have = 0.25 * (double)in.free_bytes + 3.0 * (double)in.ll_cap * sizeof(float);
        const double per_frame = (double)nb * G * sizeof(float);       // (a chunk holds at most nb * Fc rows)
        if (3.0 * (double)(sumT + 128) * G * sizeof(float) > have && 3.0 * (double)Fc * per_frame > have)
            Fc = std::max(128, (int)(have / 3.0 / per_frame) / 128 * 128);
        if (in.fc_env > 0) Fc = in.fc_env;
    }
    P.Fc = Fc;
    const int n_chunks = P.n_chunks = std::max(1, (P.maxT + Fc - 1) / Fc);   // chunk 0 also carries recognitionStart
    // rows of a chunk: stream u's frames [c0, min(T_u, c1)) start at row_off[c][u]
    P.chunk_row0.assign((size_t)n_chunks + 1, 0);
    P.row_off.assign((size_t)n_chunks * nb, 0); P.chunk_rows.assign((size_t)n_chunks, 0);
    for (int c = 0; c < n_chunks; ++c) {
        long long r = 0;
        for (int u = 0; u < nb; ++u) {
            P.row_off[(size_t)c * nb + u] = (int)r;
            r += std::max(0, std::min(P.T[(size_t)u], (c + 1) * Fc) - c * Fc);
        }
        if (r > 0x7fffff00LL) return {WAVE_CHUNK_ROWS, -1};
        P.chunk_rows[(size_t)c] = (int)((r + tile - 1) / tile * tile);
        P.chunk_row0[(size_t)c + 1] = P.chunk_row0[(size_t)c] + (size_t)P.chunk_rows[(size_t)c];
        P.max_rows = std::max(P.max_rows, (size_t)P.chunk_rows[(size_t)c]);
    }
    P.max_rows = std::max<size_t>(P.max_rows, (size_t)tile);
    // row -> source frame table for all chunks
    P.n_rows_all = std::max<size_t>(P.chunk_row0[(size_t)n_chunks], 1);
    P.row_src.assign(P.n_rows_all, -1);
    for (int c = 0; c < n_chunks; ++c)
        for (int u = 0; u < nb; ++u) {
            const int n = std::max(0, std::min(P.T[(size_t)u], (c + 1) * Fc) - c * Fc);
            int *dst = P.row_src.data() + P.chunk_row0[(size_t)c] + (size_t)P.row_off[(size_t)c * nb + u];
            for (int dt = 0; dt < n; ++dt) {
                const int64_t src = in.ustart[u] + (int64_t)c * Fc + dt;
                if (src > 0x7fffffff) return {WAVE_BATCH_FRAMES, -1};
                dst[dt] = (int)src;
            }
        }
    return {WAVE_OK, -1};
}
