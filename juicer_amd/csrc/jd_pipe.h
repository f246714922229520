// jd_pipe.h - batches through the resident slot kernel, utterance by utterance (JD_FLOW_RESIDENT), as DECISIONS: the host's record of
// a stream's mailbox, the pipeline's bookkeeping, and what the pump, the announcement and the handing back decide - which slot takes
// which utterance, which command carries a result slot, when a new ready number is needed, which rows the next scoring piece covers,
// when the watchdog gives up, what survives a drain.  Plain functions over plain structs, no HIP: jd_host_resident.h makes the
// launches, event queries, mailbox accesses and statistics they ask for; tests/pipe_driver.cpp runs them on the CPU
// (tests/test_pipe_cpu.py).  That driver carries a twin of jd_host_resident.h's pump_harvest, pump_refill, pump_score, pipe_announce,
// pipe_decode and pipe_drain with the device replaced by a model: whoever changes how these functions are called changes both.
#pragma once

#include <algorithm>
#include <cstdint>
#include <deque>
#include <numeric>
#include <string>
#include <vector>

#include "jd_score_plan.h"      // SCORE_SMALL_BELOW: below how many tiles a scoring launch takes the small ones (pipe_piece_bounds)

enum {
    PIPE_CHUNK = 128,                    // frames per command: what a slot runs before it looks at its mailbox again (jd_dec_quiesce waits that long)
    PIPE_PIECE_ROWS0 = 6144,             // rows per scoring launch where nothing is planned (JD_PIPE_DECOUPLE=0)
    PIPE_EXPORTS = 64,                   // slots per jd_finish_export_kernel launch (jd_gc.h: ExportList)
    PIPE_DEPTH_MAX = 32
};

// ---- the mailbox protocol as the host sees it, for one stream (jd_res_*: the broker's streams and the pipeline's slots alike)
struct ResStream {
    unsigned seq;                                      // last sequence number posted
    unsigned rid;                                      // the last ready number enqueued for it (Resident::d_ready: how far the side stream has come)
    int T_posted, T_done, err_done;
    int slot_posted, vslot_posted;                     // (vslot_posted: ResPost::vslot of the command, -1 none)
    bool exported;                                     // the last report says the slot has exported its utterance (ResDone::exported)
    bool busy;                                         // a command is posted and its report not yet taken
    bool init_pending;                                 // ... and it begins an utterance (ResPost::init): a re-post must say so again
    // The kernel starts: the numbers of both sides begin again.  What the host knows of a stream beyond them - where it stands, a
    // report not yet taken, an init that a re-post has to repeat - survives a restart; a new record (T_now: where the decoder's
    // stream stands) is idle there.
    void reset(const int *T_now)
    {
        seq = rid = 0u;
        if (T_now) { T_posted = T_done = *T_now; err_done = slot_posted = 0; vslot_posted = -1; exported = busy = init_pending = false; }
    }
};
// The command "frames up to T, likelihood rows from `slot`": the record of it, and what goes into the mailbox (ResPost) - `word` last.
// init: the command begins an utterance.  vslot (the pipeline's slots): the command ends one.
struct ResCommand { int T, init, vslot; unsigned ready_id; unsigned long long word; };
static inline ResCommand res_stream_command(ResStream &S, int T, int slot, bool init, int vslot)
{
    S.seq += 1;
    S.busy = true;
    S.T_posted = T; S.slot_posted = slot; S.vslot_posted = vslot; S.exported = false;
    if (init) S.init_pending = true;
    return ResCommand{T, init ? 1 : 0, vslot, S.rid, ((unsigned long long)S.seq << 32) | (unsigned)slot};
}
static inline void res_stream_begin(ResStream &S) { S.T_done = 0; S.err_done = 0; }   // (the pipeline) an utterance begins: the stream stands at frame 0
// The report (ResDone): is it the answer to the command posted (seq, read first), and then what it says.  Returns the frames advanced.
static inline bool res_stream_answered(const ResStream &S, unsigned seq) { return seq == S.seq; }
static inline int res_stream_report(ResStream &S, int frame, int error, int exported)
{
    const int advanced = std::max(0, frame - S.T_done);
    S.T_done = frame; S.err_done = error; S.exported = exported != 0;
    S.init_pending = false;
    S.busy = false;
    return advanced;
}
// through, no error, short of what was posted: the stream stopped for a Path collection (or its command was never seen)
static inline bool res_stream_stopped(const ResStream &S) { return S.err_done == 0 && S.T_done < S.T_posted; }

// ---- the pipeline's bookkeeping
enum PipeUttState { PIPE_UTT_QUEUED = 0, PIPE_UTT_RUNNING = 1, PIPE_UTT_THROUGH = 2 };
struct PipeUtt { PipeUttState state = PIPE_UTT_QUEUED; int slot = -1, T = 0; long long row0 = 0; };
struct PipeBatch {
    const float *feats = nullptr; int n = 0; int table = 0; int next = 0, n_done = 0;   // (feats: compared, never read here)
    size_t rows = 0, rows_scored = 0;                  // rows of its table, and how many of them have a scoring launch enqueued
    int n_kexport = 0;                                 // utterances of it exported by jd_finish_export_kernel (on the side stream)
    bool scored = false;                               // its table is scored to the last row (the event of its table has completed)
    int n_commands = 0, n_pieces = 0;                  // (JD_VERBOSE) commands the pump posted for it, scoring launches
    std::vector<int64_t> offs;
    std::vector<PipeUtt> u;
    std::vector<int> order;                            // its utterances by length, longest first: the order in which slots take them
};
struct PipeState {
    int K = 0, max_batch = 0, n_slots = 0;
    size_t table_rows = 0;
    std::deque<PipeBatch> q;
    std::vector<char> table_used;
    std::vector<int> slot_batch_id, slot_utt;          // per slot: the batch (its serial number) and utterance it runs, -1: free
    std::vector<char> slot_dirty;
    std::vector<char> slot_kexport;                    // per slot: its last utterance went out by jd_finish_export_kernel (side stream)
    long long serial0 = 0;                             // serial number of q.front()
    int chunk = PIPE_CHUNK;
    // Scoring launches, a piece at a time: up to max_out of them enqueued - one running, one behind it - each with its event; the
    // oldest is event piece_turn.
    size_t piece_rows = PIPE_PIECE_ROWS0;              // rows per scoring launch (plan_piece_rows, or JD_PIPE_PIECE)
    int piece_out = 0, piece_turn = 0, max_out = 2;
    // JD_PIPE_DECOUPLE=0 (development) clears it: every export by the kernel on the side stream, a ready number with every
    // utterance, one piece of PIPE_PIECE_ROWS0 rows in flight
    bool decouple = true;
    long long frames_done = 0;
};
static inline int pipe_vslot(const PipeState &P, const PipeBatch &B, int utt) { return B.table * P.max_batch + utt; }

// ---- jd_dec_set_pipeline(JD_FLOW_RESIDENT): depth and slots as given (0: default), checked in this order
enum PipeSetVerdict { PIPE_SET_OK = 0, PIPE_SET_DEPTH, PIPE_SET_SLOTS, PIPE_SET_DEVICE, PIPE_SET_NOT_WITH };
struct PipeSetting { PipeSetVerdict verdict; int depth, slots; };
static inline PipeSetting pipe_setting(int depth, int slots, int max_streams, int n_cus, int slot_wg_per_cu, bool lazy, bool hybrid)
{
    if (slots == 0) slots = max_streams;
    // (batches in the slots + the one being handed back + what is being scored: 256 slots and batches of 64 need ten - a batch
    // is handed back when its longest utterance is through, ~150 ms after it was taken up at 130 us per frame)
    if (depth == 0) depth = std::min((int)PIPE_DEPTH_MAX, std::max(8, slots / 32 + 2));
    PipeSetVerdict v = PIPE_SET_OK;
    if (depth < 2 || depth > PIPE_DEPTH_MAX) v = PIPE_SET_DEPTH;
    else if (slots < 1 || slots > max_streams) v = PIPE_SET_SLOTS;
    // the slots are workgroups of a mailbox kernel: ALL of them have to be on the device at once (slot_wg_per_cu per CU at most) -
    // a workgroup that never gets a CU never answers, and the batch whose utterance was posted to it never comes back
    else if (slots > n_cus * slot_wg_per_cu) v = PIPE_SET_DEVICE;
    else if (lazy || hybrid) v = PIPE_SET_NOT_WITH;
    return PipeSetting{v, depth, slots};
}

// ---- sizing (pipe_fill): for batches like the first one announced (n_utts utterances, `rows` frames), tables and result slots for
// batches up to twice that: a larger one later starts the pipeline again, with larger ones.  The development knobs, -1 unset: a chunk
// below 16 is ignored, JD_PIPE_DECOUPLE clears `decouple` when 0.  Returns the number of virtual result slots.
struct PipeSizeIn { int depth, pipe_slots, max_streams, n_utts; size_t rows; int tile, chunk_knob, decouple_knob; };
static inline size_t pipe_size(PipeState &P, const PipeSizeIn &in)
{
    P.K = in.depth; P.max_batch = 2 * in.n_utts;
    P.n_slots = (in.pipe_slots > 0 && in.pipe_slots <= in.max_streams) ? in.pipe_slots : in.max_streams;
    if (in.chunk_knob >= 16) P.chunk = in.chunk_knob;
    P.decouple = in.decouple_knob != 0;
    P.max_out = P.decouple ? 2 : 1;
    P.table_rows = ((2 * in.rows + 1024) + (size_t)in.tile - 1) / (size_t)in.tile * (size_t)in.tile;
    P.table_used.assign((size_t)P.K, 0);
    P.slot_batch_id.assign((size_t)P.n_slots, -1); P.slot_utt.assign((size_t)P.n_slots, -1); P.slot_dirty.assign((size_t)P.n_slots, 0);
    P.slot_kexport.assign((size_t)P.n_slots, 0);
    return (size_t)P.K * (size_t)P.max_batch;
}
// Rows per scoring launch: the bounds plan_piece_rows (jd_plan.h) chooses between - 4096 to 8192 rows (DESIGN.md 3.4's sweep: shorter
// pieces pay per launch, longer ones hold what waits behind them) - and the state groups of a row tile.  A launch of fewer than
// SCORE_SMALL_BELOW tiles is one of small (group_small-state) tiles (jd_score_plan.h: score_plan); where the longest piece is not,
// no piece is to fall below it.  (group, group_small, tile: the caller passes the same header's GMM_GT, GMM_GT_SMALL, GMM_ROWS2)
struct PipePieceBounds { int lo, hi, groups; };
static inline PipePieceBounds pipe_piece_bounds(int n_gmm, int group, int group_small, int tile)
{
    PipePieceBounds b{4096, 8192, (n_gmm + group - 1) / group};
    if ((long long)(b.hi / tile) * b.groups < SCORE_SMALL_BELOW) b.groups = (n_gmm + group_small - 1) / group_small;
    else b.lo = std::max(b.lo, (SCORE_SMALL_BELOW + b.groups - 1) / b.groups * tile);
    return b;
}
// ... what was planned (0: nothing - the kernels of other tiles, JD_PIPE_DECOUPLE=0), unless JD_PIPE_PIECE says otherwise: a piece
// below 128 is ignored, else rounded down to the tile
static inline size_t pipe_size_piece(size_t planned, int piece_knob, int tile)
{
    if (piece_knob >= 128) return (size_t)piece_knob / (size_t)tile * (size_t)tile;
    return planned ? planned : (size_t)PIPE_PIECE_ROWS0;
}

// ---- announcing (jd_dec_prefetch_scores).  Does a batch go this way at all; has it outgrown the tables (the pipeline starts again,
// larger); is the queue full; and the enqueue: the first free table, each utterance's frames and first row, the order of taking.
static inline bool pipe_takes(bool pipe_mode, bool lazy, bool partial, bool hybrid, int n_utts) { return pipe_mode && !lazy && !partial && !hybrid && n_utts >= 1; }
static inline bool pipe_outgrown(const PipeState &P, int n_utts, size_t rows) { return n_utts > P.max_batch || rows > P.table_rows; }
static inline bool pipe_full(const PipeState &P) { return (int)P.q.size() >= P.K; }
static inline void pipe_started(PipeState &P) { P.serial0 = 0; P.frames_done = 0; }   // the kernel comes onto the device for the first batch
static inline const PipeBatch &pipe_enqueue(PipeState &P, const float *feats, int n_utts, const int64_t *offs)
{
    PipeBatch B;
    B.feats = feats; B.n = n_utts; B.offs.assign(offs, offs + n_utts + 1);
    int t = 0;
    while (t < P.K && P.table_used[(size_t)t]) ++t;
    B.table = t; P.table_used[(size_t)t] = 1;
    B.u.resize((size_t)n_utts);
    const long long base = (long long)t * (long long)P.table_rows;
    for (int u = 0; u < n_utts; ++u) { B.u[(size_t)u].T = (int)(offs[u + 1] - offs[u]); B.u[(size_t)u].row0 = base + (offs[u] - offs[0]); }
    B.order.resize((size_t)n_utts);
    std::iota(B.order.begin(), B.order.end(), 0);
    std::stable_sort(B.order.begin(), B.order.end(), [&](int a, int b) { return B.u[(size_t)a].T > B.u[(size_t)b].T; });
    B.rows = (size_t)(offs[n_utts] - offs[0]); B.rows_scored = 0;      // (scored by the pump, a piece at a time, on the CUs the slots leave)
    P.q.push_back(std::move(B));
    return P.q.back();
}

// ---- the pump, step 1: a slot whose report is in.  One that stopped for a Path collection collects and goes on, one in the middle
// of its utterance gets its next frames (the command that ends the utterance names its result slot), one whose utterance is through
// is free: its result is in its virtual result slot already (the report says "exported": k_slot), or goes there by
// jd_finish_export_kernel - after an error, and wherever the slot did not.
enum PipeHarvestAct { PIPE_COLLECT = 0, PIPE_NEXT = 1, PIPE_THROUGH = 2 };
struct PipeHarvest {
    PipeHarvestAct act;
    int T, row_slot, vslot;                            // NEXT: the command
    bool kexport, dirty;                               // THROUGH: the kernel exports it (to the utterance's result slot); its arenas may be inconsistent
};
static inline bool pipe_slot_occupied(const PipeState &P, int s) { return P.slot_batch_id[(size_t)s] >= 0; }
static inline PipeBatch &pipe_slot_batch(PipeState &P, int s) { return P.q[(size_t)(P.slot_batch_id[(size_t)s] - P.serial0)]; }
static inline PipeHarvest pipe_harvest(const ResStream &S, const PipeUtt &U, int vslot, int chunk, bool decouple)
{
    PipeHarvest h{PIPE_COLLECT, 0, 0, -1, false, false};
    const int er = S.err_done, fr = S.T_done;
    if (res_stream_stopped(S)) return h;
    if (er == 0 && fr < U.T) {
        h.act = PIPE_NEXT;
        h.T = std::min(U.T, fr + chunk); h.row_slot = (int)U.row0; h.vslot = (decouple && h.T == U.T) ? vslot : -1;
        return h;
    }
    h.act = PIPE_THROUGH;
    h.kexport = !(S.exported && er == 0);
    h.dirty = er != 0;                                 // (out of the game until the pipeline stops)
    return h;
}
// ... what follows THROUGH: a slot the kernel exports for waits for it with its next utterance (pipe_refill); the utterance, its
// batch, the slot
static inline void pipe_harvest_kexport(PipeState &P, int s) { P.slot_kexport[(size_t)s] = 1; pipe_slot_batch(P, s).n_kexport += 1; }
static inline void pipe_harvest_through(PipeState &P, int s, const PipeHarvest &h, int frames)
{
    PipeBatch &B = pipe_slot_batch(P, s);
    B.u[(size_t)P.slot_utt[(size_t)s]].state = PIPE_UTT_THROUGH; B.n_done += 1; P.frames_done += frames;
    if (h.dirty) P.slot_dirty[(size_t)s] = 1;
    P.slot_batch_id[(size_t)s] = -1;
}
// the kernel's export list (jd_gc.h: ExportList) takes one more; true: it is full and goes out now
template <class EL> static inline bool pipe_export_add(EL *el, int s, int vslot)
{
    el->slot[el->n] = s; el->vslot[el->n] = vslot; el->n += 1;
    return el->n == PIPE_EXPORTS;
}

// ---- the pump, step 2: free, clean slots take the next queued utterances - from the first batch that has any left, and only once
// its scoring is enqueued to the last row.  Where the host knows that the table is scored (table_done(t): the batch's event, asked
// under `decouple` while `scored` is false, once per assignment) and the slot's last result went out without the side stream, the
// command carries the ready number the slot has: nothing to wait for.  Otherwise (bump) a new ready number, counted up behind the
// kernel export and every scoring launch enqueued so far.
struct PipeAssign { int slot, batch, utt; bool bump; };                // (batch: its index in the queue)
template <class Done> static inline void pipe_refill(PipeState &P, Done &&table_done, std::vector<PipeAssign> *out)
{
    size_t bi = 0;
    for (int s = 0; s < P.n_slots; ++s) {
        if (P.slot_batch_id[(size_t)s] >= 0 || P.slot_dirty[(size_t)s]) continue;
        while (bi < P.q.size() && P.q[bi].next >= P.q[bi].n) ++bi;
        if (bi >= P.q.size() || P.q[bi].rows_scored < P.q[bi].rows) break;
        PipeBatch &B = P.q[bi];
        if (P.decouple && !B.scored && table_done(B.table)) B.scored = true;
        const int ui = B.order[(size_t)B.next++];                      // (longest first: a batch is handed back when its LAST utterance is through)
        B.u[(size_t)ui].state = PIPE_UTT_RUNNING; B.u[(size_t)ui].slot = s;
        P.slot_batch_id[(size_t)s] = (int)(P.serial0 + (long long)bi); P.slot_utt[(size_t)s] = ui;
        out->push_back(PipeAssign{s, (int)bi, ui, !B.scored || P.slot_kexport[(size_t)s] != 0});
        P.slot_kexport[(size_t)s] = 0;
    }
}
// the first command of an assigned utterance (it begins it; it may end it as well)
struct PipeFirst { int T, row_slot, vslot; };
static inline PipeFirst pipe_refill_command(const PipeState &P, const PipeAssign &a)
{
    const PipeBatch &B = P.q[(size_t)a.batch];
    const PipeUtt &U = B.u[(size_t)a.utt];
    const int T = std::min(U.T, P.chunk);
    return PipeFirst{T, (int)U.row0, (P.decouple && T == U.T) ? pipe_vslot(P, B, a.utt) : -1};
}

// ---- the pump, step 3: scoring, a piece at a time.  A batch's table in ONE launch holds the side stream for ~20 ms, and whatever a
// slot waits for on that stream - a kernel export, a ready number - queues up behind it.  Up to max_out pieces are enqueued, one
// running and one behind it, so that the stream has no gap between them.  Batches in queue order; behind a batch's last piece, the
// event that tells pipe_refill its table is scored.
template <class Done> static inline void pipe_pieces_retire(PipeState &P, Done &&piece_done)
{
    while (P.piece_out > 0 && piece_done(P.piece_turn)) { P.piece_out -= 1; P.piece_turn ^= 1; }
}
struct PipePiece {
    int batch;                                         // its index in the queue, -1: nothing to launch now
    size_t feat_row, base_row, rows;                   // from this row of the batch's features, to this row of the tables
    int table, event;                                  // the piece's event (0 / 1)
    bool last;                                         // the batch's event follows
};
static inline PipePiece pipe_piece_next(const PipeState &P)
{
    PipePiece p{-1, 0, 0, 0, 0, 0, false};
    if (P.piece_out >= P.max_out) return p;
    for (size_t bi = 0; bi < P.q.size(); ++bi) {
        const PipeBatch &B = P.q[bi];
        if (B.rows_scored >= B.rows) continue;
        p.batch = (int)bi; p.table = B.table;
        p.rows = std::min(P.piece_rows, B.rows - B.rows_scored);
        p.feat_row = (size_t)B.offs[0] + B.rows_scored;
        p.base_row = (size_t)B.table * P.table_rows + B.rows_scored;
        p.event = P.piece_turn ^ (P.piece_out & 1);
        p.last = B.rows_scored + p.rows >= B.rows;
        break;
    }
    return p;
}
static inline void pipe_piece_launched(PipeState &P, const PipePiece &p)
{
    PipeBatch &B = P.q[(size_t)p.batch];
    B.rows_scored += p.rows; B.n_pieces += 1; P.piece_out += 1;
}

// ---- handing back (jd_decode_batch_device of the oldest announced batch).  Is the batch asked for the announced one: the same
// address, count and offsets (if not: as if nothing had been announced).
static inline bool pipe_is_head(const PipeState &P, const float *feats, int n_utts, const int64_t *offs)
{
    const PipeBatch &F = P.q.front();
    bool same = F.feats == feats && F.n == n_utts;
    for (int u = 0; same && u <= n_utts; ++u) same = F.offs[(size_t)u] == offs[u];
    return same;
}
static inline bool pipe_head_done(const PipeState &P) { return P.q.front().n_done == P.q.front().n; }
// ... and done: the side stream is waited for only where the kernel exported one of its utterances there.  What the slots exported
// themselves is in memory since their reports, and the side stream has pieces of later batches on it.
static inline bool pipe_head_needs_sync(const PipeState &P) { return P.q.front().n_kexport > 0; }
// The watchdog of the wait: no utterance through for 30 s means something is stuck - better an error, and the other paths, than a
// caller that waits for ever; a kernel that has gone by itself (nobody gave it a command for 5 s) comes back, three times.
struct PipeWatch { int restarts = 0; long long seen_frames = -1, t_progress_ns = 0; };
static inline bool pipe_watch_stuck(PipeWatch &W, long long frames_done, long long now_ns)
{
    if (frames_done != W.seen_frames) { W.seen_frames = frames_done; W.t_progress_ns = now_ns; return false; }
    return (double)(now_ns - W.t_progress_ns) / 1e9 > 30.0;
}
static inline bool pipe_watch_gives_up(PipeWatch &W) { return ++W.restarts > 3; }
// the slots the head's utterances ran on, and the head leaves the queue; true: nothing is announced behind it (the kernel leaves)
static inline void pipe_head_slots(const PipeState &P, std::vector<int> *slot_of)
{
    const PipeBatch &F = P.q.front();
    slot_of->resize((size_t)F.n);
    for (int u = 0; u < F.n; ++u) (*slot_of)[(size_t)u] = F.u[(size_t)u].slot;
}
static inline bool pipe_pop(PipeState &P)
{
    P.table_used[(size_t)P.q.front().table] = 0;
    P.q.pop_front();
    P.serial0 += 1;
    return P.q.empty();
}
// Everything in flight is dropped (the kernel has left; the batches concerned are decoded from scratch when their turn comes).  Slots
// left in the middle of an utterance, or failed, make their streams dirty.  (piece_turn, serial0 and frames_done stay as they are.)
template <class Dirty> static inline void pipe_drain_reset(PipeState &P, Dirty *stream_dirty)
{
    P.piece_out = 0;
    P.q.clear();
    std::fill(P.table_used.begin(), P.table_used.end(), 0);
    std::fill(P.slot_batch_id.begin(), P.slot_batch_id.end(), -1);
    for (int s = 0; s < P.n_slots; ++s) {
        if (P.slot_dirty[(size_t)s]) (*stream_dirty)[(size_t)s] = 1;
        P.slot_dirty[(size_t)s] = 0; P.slot_kexport[(size_t)s] = 0;
    }
}

// ---- JD_VERBOSE: "a,b,c" of a batch's utterances (their lengths, first rows, the order of taking)
template <class F> static inline std::string pipe_list(int n, F &&value)
{
    std::string s;
    for (int i = 0; i < n; ++i) { s += (i ? "," : ""); s += std::to_string((long long)value(i)); }
    return s.empty() ? "-" : s;
}
