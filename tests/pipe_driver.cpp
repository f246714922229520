// pipe_driver.cpp - runs the decisions of the slot pipeline (juicer_amd/csrc/jd_pipe.h) over lines read from stdin, for
// tests/test_pipe_cpu.py and tests/test_gpu_pipe_inputs.py: one line in, one line of integers out (tests/pipe_cases.py writes the lines
// and reads the columns).
//
// Single decisions: setting size bounds takes outgrown full enqueue harvest harvest_many.
// Scripts: `reset` makes a model decoder in JD_FLOW_RESIDENT - no pipeline yet - and `announce`, `decode`, `wait`, `quiesce`, `drain`
// are what jd_dec_prefetch_scores, jd_decode_batch_device (its first turn of the waiting loop, and every further one), jd_dec_quiesce
// and a setter do to it.  The host functions here are jd_host_resident.h's, step for step, with every HIP call and every mailbox
// read replaced by what the line says the device did (the model has no thread and no time of its own):
//   <dev> = n_rep {slot frame error exported}  n_left {slot}  n_late {slot}  pieces_done  n_tab {table}  clock_ns
// n_rep: reports that are in (each answers the slot's last command); n_left: workgroups that have left the kernel; n_late: ... that
// leave behind this turn's pump (the waiting loop's own look); pieces_done: scoring pieces that have completed since, oldest
// first; n_tab: tables whose batch event has completed; clock_ns: what the clock reads, from the start of the decode.
// Output: rc status, the number of integers of the log, the log - everything the host did, in order, each entry its kind and
// arguments (LOG_*) - and the state (print_state).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>

#include "jd_pipe.h"

static const float g_feats[16] = {0};                                 // feature buffers are told apart by address: &g_feats[id]

struct In {
    std::istringstream s;
    long long i() { long long v = 0; if (!(s >> v)) { fprintf(stderr, "pipe_driver: short line\n"); exit(2); } return v; }
    std::vector<int64_t> vec(int n) { std::vector<int64_t> v((size_t)std::max(n, 0)); for (int64_t &x : v) x = i(); return v; }
};
static std::vector<long long> g_out;
static void put(long long v) { g_out.push_back(v); }

enum { LOG_COMMAND = 1,       // slot T row_slot init vslot ready_id seq
       LOG_BUMP,              // slot id
       LOG_KEXPORT,           // n {slot vslot}
       LOG_PIECE,             // table feat_row base_row rows event batch_event
       LOG_COLLECT,           // slot
       LOG_QUERY_PIECE,       // event answer
       LOG_QUERY_TABLE,       // table answer
       LOG_STOP,              // lost
       LOG_START,
       LOG_SYNC,              // the side stream, for the kernel's exports of the batch handed back
       LOG_FETCH,             // first vslot, n {slot_of}
       LOG_WIPE };            // stream
enum { RC_OK = 0, RC_LOST = 1, RC_STUCK = 2, RC_KEEPS_ENDING = 3, RC_FULL = 4 };
enum { ST_NOT_THIS_WAY = 0, ST_HANDLED = 1, ST_WAITING = 2 };

struct Done { unsigned seq; int frame, error, left, exported; };
struct ExportList { int n; int slot[64]; int vslot[64]; };
struct Model {
    int depth = 0, pipe_slots = 0, max_streams = 0, tile = 128, chunk_knob = -1, decouple_knob = -1, piece_knob = -1;
    size_t planned = 0;
    bool have_pipe = false, pipe_on = false, res_on = false;
    PipeState P;
    std::vector<ResStream> stream;                                     // Resident::stream ...
    std::vector<Done> done;                                            // ... and h_done
    std::vector<char> stream_dirty;
    std::vector<int> stream_T;
    bool piece_pending[2] = {false, false};                            // ev_piece, ev_batch: recorded and not yet completed
    std::vector<int> piece_fifo;
    std::vector<char> table_pending;
    PipeWatch W;
    long long utts_through = 0, batches_back = 0, frames_searched = 0, rows_scored = 0;
    std::vector<long long> log;
};
static void lg(Model &m, std::initializer_list<long long> v) { m.log.insert(m.log.end(), v); }

// ==== the host side: jd_host_resident.h's functions over jd_pipe.h, the device replaced by the model.  This is a TWIN of res_harvest,
// res_command, jd_res_collect, pump_harvest, pump_refill, pump_score, pipe_pump, pipe_fill, pipe_announce, pipe_decode and pipe_drain
// there - the same calls into jd_pipe.h, in the same order, with the same arguments - and is kept in step with them by hand: the golden
// pins jd_pipe.h and this order of calls; the GPU tests pin that the real functions make them.
static bool res_harvest(Model &m, int s)
{
    ResStream &S = m.stream[(size_t)s];
    if (!S.busy) return true;
    if (!res_stream_answered(S, m.done[(size_t)s].seq)) return false;
    m.frames_searched += res_stream_report(S, m.done[(size_t)s].frame, m.done[(size_t)s].error, m.done[(size_t)s].exported);
    if (S.err_done != 0) m.stream_dirty[(size_t)s] = 1;
    m.stream_T[(size_t)s] = S.T_done;
    return true;
}
static bool res_any_left(const Model &m, int n)
{
    for (int s = 0; s < n; ++s) if (m.done[(size_t)s].left != 0) return true;
    return false;
}
static int jd_res_stop(Model &m)
{
    if (!m.res_on) return RC_OK;
    m.piece_pending[0] = m.piece_pending[1] = false; m.piece_fifo.clear();   // (it synchronises the side stream)
    std::fill(m.table_pending.begin(), m.table_pending.end(), 0);
    bool lost = false;
    for (int s = 0; s < (int)m.stream.size(); ++s)
        if (!res_harvest(m, s)) {
            m.stream[(size_t)s].busy = false;
            if (!m.done[(size_t)s].left) { lost = true; m.stream_dirty[(size_t)s] = 1; }
        }
    m.res_on = false;
    lg(m, {LOG_STOP, lost});
    return lost ? RC_LOST : RC_OK;
}
static int jd_res_start(Model &m)
{
    if (m.res_on) return RC_OK;
    for (Done &D : m.done) D = Done{0u, 0, 0, 0, 0};
    for (ResStream &S : m.stream) S.reset(nullptr);
    m.res_on = true;
    lg(m, {LOG_START});
    return RC_OK;
}
static void res_bump(Model &m, int n, const int *streams)
{
    for (int i = 0; i < n; ++i) lg(m, {LOG_BUMP, streams[i], (long long)++m.stream[(size_t)streams[i]].rid});
}
static void res_command(Model &m, int s, int T, int slot, bool init, int vslot)
{
    const ResCommand C = res_stream_command(m.stream[(size_t)s], T, slot, init, vslot);
    lg(m, {LOG_COMMAND, s, C.T, (long long)(int)(unsigned)(C.word & 0xffffffffu), C.init, C.vslot, (long long)C.ready_id, (long long)(C.word >> 32)});
}
static void jd_res_collect(Model &m, int s)
{
    lg(m, {LOG_COLLECT, s});
    res_bump(m, 1, &s);
    const ResStream &S = m.stream[(size_t)s];
    res_command(m, s, S.T_posted, S.slot_posted, S.init_pending, S.vslot_posted);
}
static void pipe_drain(Model &m)
{
    if (!m.have_pipe || !m.pipe_on) return;
    (void)jd_res_stop(m);
    m.pipe_on = false;
    pipe_drain_reset(m.P, &m.stream_dirty);
}
static void pipe_export(Model &m, ExportList *EL)
{
    if (EL->n == 0) return;
    lg(m, {LOG_KEXPORT, EL->n});
    for (int k = 0; k < EL->n; ++k) lg(m, {EL->slot[k], EL->vslot[k]});
    EL->n = 0;
}
static void pump_harvest(Model &m)
{
    PipeState &P = m.P;
    ExportList EL; EL.n = 0;
    for (int s = 0; s < P.n_slots; ++s) {
        if (!pipe_slot_occupied(P, s) || !res_harvest(m, s)) continue;
        const ResStream &S = m.stream[(size_t)s];
        PipeBatch &B = pipe_slot_batch(P, s);
        const int ui = P.slot_utt[(size_t)s];
        const PipeHarvest h = pipe_harvest(S, B.u[(size_t)ui], pipe_vslot(P, B, ui), P.chunk, P.decouple);
        if (h.act == PIPE_COLLECT) jd_res_collect(m, s);
        else if (h.act == PIPE_NEXT) { res_command(m, s, h.T, h.row_slot, false, h.vslot); B.n_commands += 1; }
        else {
            if (h.kexport) {
                pipe_harvest_kexport(P, s);
                if (pipe_export_add(&EL, s, pipe_vslot(P, B, ui))) pipe_export(m, &EL);
            }
            pipe_harvest_through(P, s, h, S.T_done);
            m.utts_through += 1;
        }
    }
    pipe_export(m, &EL);
}
static void pump_score(Model &m)
{
    PipeState &P = m.P;
    pipe_pieces_retire(P, [&](int e) { lg(m, {LOG_QUERY_PIECE, e, !m.piece_pending[e]}); return !m.piece_pending[e]; });
    for (PipePiece p = pipe_piece_next(P); p.batch >= 0; p = pipe_piece_next(P)) {
        m.piece_pending[p.event] = true; m.piece_fifo.push_back(p.event);
        pipe_piece_launched(P, p); m.rows_scored += (long long)p.rows;
        if (p.last) m.table_pending[(size_t)p.table] = 1;
        lg(m, {LOG_PIECE, p.table, (long long)p.feat_row, (long long)p.base_row, (long long)p.rows, p.event, p.last});
    }
}
static void pump_refill(Model &m)
{
    PipeState &P = m.P;
    std::vector<PipeAssign> who;
    std::vector<int> bump;
    pipe_refill(P, [&](int t) { lg(m, {LOG_QUERY_TABLE, t, !m.table_pending[(size_t)t]}); return !m.table_pending[(size_t)t]; }, &who);
    if (who.empty()) return;
    for (const PipeAssign &a : who) if (a.bump) bump.push_back(a.slot);
    if (!bump.empty()) res_bump(m, (int)bump.size(), bump.data());
    for (const PipeAssign &a : who) {
        const PipeFirst c = pipe_refill_command(P, a);
        res_stream_begin(m.stream[(size_t)a.slot]);
        res_command(m, a.slot, c.T, c.row_slot, true, c.vslot);
        P.q[(size_t)a.batch].n_commands += 1;
    }
}
static int pipe_pump(Model &m)
{
    if (m.res_on && res_any_left(m, m.P.n_slots)) { const int rc = jd_res_stop(m); if (rc) return rc; }
    if (!m.res_on) (void)jd_res_start(m);
    pump_harvest(m);
    pump_refill(m);
    pump_score(m);
    return RC_OK;
}
static size_t pipe_fill(Model &m, int n_utts, size_t rows)
{
    m.P = PipeState();
    const size_t V = pipe_size(m.P, PipeSizeIn{m.depth, m.pipe_slots, m.max_streams, n_utts, rows, m.tile, m.chunk_knob, m.decouple_knob});
    m.P.piece_rows = pipe_size_piece(m.P.decouple ? m.planned : 0, m.piece_knob, m.tile);
    m.table_pending.assign((size_t)m.P.K, 0);
    m.piece_pending[0] = m.piece_pending[1] = false; m.piece_fifo.clear();
    m.have_pipe = true;
    return V;
}
static int pipe_announce(Model &m, int n_utts, const float *feats, const int64_t *offs, int *taken)
{
    *taken = 0;
    if (!pipe_takes(true, false, false, false, n_utts)) return RC_OK;
    const size_t rows = (size_t)(offs[n_utts] - offs[0]);
    if (m.have_pipe && pipe_outgrown(m.P, n_utts, rows)) { pipe_drain(m); m.have_pipe = false; }
    if (!m.have_pipe) (void)pipe_fill(m, n_utts, rows);
    if (pipe_full(m.P)) return RC_FULL;
    if (!m.pipe_on) {
        for (int s = 0; s < m.P.n_slots; ++s)
            if (m.stream_dirty[(size_t)s]) { lg(m, {LOG_WIPE, s}); m.stream_dirty[(size_t)s] = 0; }
        (void)jd_res_start(m);
        m.pipe_on = true;
        pipe_started(m.P);
    }
    (void)pipe_enqueue(m.P, feats, n_utts, offs);
    *taken = 1;
    return pipe_pump(m);
}
// one turn of pipe_decode's waiting loop (`late`: workgroups that leave behind the pump); ST_WAITING: it sleeps and comes again
static int pipe_decode_turn(Model &m, long long clock_ns, const std::vector<int64_t> &late, int *status)
{
    PipeState &P = m.P;
    *status = ST_WAITING;
    const int rc = pipe_pump(m);
    if (rc) { pipe_drain(m); *status = ST_NOT_THIS_WAY; return rc; }
    if (pipe_head_done(P)) {
        const PipeBatch &F = P.q.front();
        if (pipe_head_needs_sync(P)) lg(m, {LOG_SYNC});
        std::vector<int> slot_of;
        pipe_head_slots(P, &slot_of);
        lg(m, {LOG_FETCH, pipe_vslot(P, F, 0), F.n});
        for (int s : slot_of) lg(m, {s});
        m.batches_back += 1;
        if (pipe_pop(P)) pipe_drain(m);
        *status = ST_HANDLED;
        return RC_OK;
    }
    for (int64_t s : late) m.done[(size_t)s].left = 1;                // (as of the moment the clock is read)
    if (pipe_watch_stuck(m.W, P.frames_done, clock_ns)) { pipe_drain(m); *status = ST_NOT_THIS_WAY; return RC_STUCK; }
    if (m.res_on && res_any_left(m, P.n_slots)) {
        const int rs = jd_res_stop(m);
        if (rs || pipe_watch_gives_up(m.W)) { pipe_drain(m); *status = ST_NOT_THIS_WAY; return rs ? rs : RC_KEEPS_ENDING; }
    }
    return RC_OK;
}
static bool pipe_decode_begin(Model &m, int n_utts, const float *feats, const int64_t *offs)
{
    if (!m.have_pipe || !m.pipe_on || m.P.q.empty()) return false;
    if (!pipe_is_head(m.P, feats, n_utts, offs)) { pipe_drain(m); return false; }
    m.W = PipeWatch();
    return true;
}
// ==== (end of the host side)

static void print_state(const Model &m)
{
    const PipeState &P = m.P;
    put(m.have_pipe); put(m.pipe_on); put(m.res_on);
    put(P.K); put(P.max_batch); put(P.n_slots); put(P.chunk); put(P.decouple); put(P.max_out); put((long long)P.piece_rows); put((long long)P.table_rows);
    put(P.serial0); put(P.frames_done); put(P.piece_out); put(P.piece_turn);
    for (int t = 0; t < P.K; ++t) put(P.table_used[(size_t)t]);
    for (int s = 0; s < P.n_slots; ++s) { put(P.slot_batch_id[(size_t)s]); put(P.slot_utt[(size_t)s]); put(P.slot_dirty[(size_t)s]); put(P.slot_kexport[(size_t)s]); }
    put((long long)P.q.size());
    for (const PipeBatch &B : P.q) {
        put((long long)(B.feats - g_feats)); put(B.n); put(B.table); put(B.next); put(B.n_done); put(B.n_kexport); put((long long)B.rows); put((long long)B.rows_scored); put(B.scored);
        for (const PipeUtt &U : B.u) { put((long long)U.state); put(U.slot); put(U.T); put(U.row0); }
        for (int o : B.order) put(o);
    }
    put((long long)m.stream.size());
    for (size_t s = 0; s < m.stream.size(); ++s) {
        const ResStream &S = m.stream[s];
        put(m.stream_dirty[s]); put(S.seq); put(S.rid); put(S.T_posted); put(S.T_done); put(S.err_done); put(S.busy); put(S.init_pending); put(S.exported);
    }
    put(m.utts_through); put(m.batches_back); put(m.frames_searched); put(m.rows_scored);
}
static void finish(Model &m, int rc, int status)
{
    put(rc); put(status); put((long long)m.log.size());
    for (long long v : m.log) put(v);
    m.log.clear();
    print_state(m);
}
static void model_reset(Model &m, int depth, int pipe_slots, int max_streams, int tile, int chunk, int decouple, size_t planned, int piece)
{
    m = Model();
    m.depth = depth; m.pipe_slots = pipe_slots; m.max_streams = max_streams; m.tile = tile; m.chunk_knob = chunk; m.decouple_knob = decouple;
    m.planned = planned; m.piece_knob = piece;
    const int zero = 0;
    m.stream.resize((size_t)max_streams);
    for (ResStream &S : m.stream) S.reset(&zero);
    m.done.assign((size_t)max_streams, Done{0u, 0, 0, 0, 0});
    m.stream_dirty.assign((size_t)max_streams, 0); m.stream_T.assign((size_t)max_streams, 0);
}
// <dev>: what the device did since the last line; returns the clock, *late the workgroups that leave behind the pump
static long long read_device(Model &m, In &in, std::vector<int64_t> *late)
{
    for (int k = (int)in.i(); k > 0; --k) {
        const int s = (int)in.i(), frame = (int)in.i(), error = (int)in.i(), exported = (int)in.i();
        Done &D = m.done[(size_t)s];
        D.seq = m.stream[(size_t)s].seq; D.frame = frame; D.error = error; D.exported = exported;
    }
    for (int64_t s : in.vec((int)in.i())) m.done[(size_t)s].left = 1;
    *late = in.vec((int)in.i());
    for (int k = (int)in.i(); k > 0 && !m.piece_fifo.empty(); --k) {
        const int e = m.piece_fifo.front();
        m.piece_fifo.erase(m.piece_fifo.begin());
        if (std::find(m.piece_fifo.begin(), m.piece_fifo.end(), e) == m.piece_fifo.end()) m.piece_pending[e] = false;
    }
    for (int64_t t : in.vec((int)in.i())) m.table_pending[(size_t)t] = 0;
    return in.i();
}
static std::vector<int64_t> offsets(const std::vector<int64_t> &len)
{
    std::vector<int64_t> offs(len.size() + 1, 0);
    for (size_t u = 0; u < len.size(); ++u) offs[u + 1] = offs[u] + len[u];
    return offs;
}
static void run_script(const std::string &cmd, In &in, Model &m)
{
    std::vector<int64_t> late;
    int rc = RC_OK, status = ST_NOT_THIS_WAY;
    if (cmd == "reset") {
        // reset depth pipe_slots max_streams tile chunk_knob decouple_knob planned piece_knob
        const int depth = (int)in.i(), slots = (int)in.i(), streams = (int)in.i(), tile = (int)in.i(), chunk = (int)in.i(), dec = (int)in.i();
        const size_t planned = (size_t)in.i();
        model_reset(m, depth, slots, streams, tile, chunk, dec, planned, (int)in.i());
    } else if (cmd == "announce" || cmd == "decode") {
        const float *feats = &g_feats[in.i()];
        const std::vector<int64_t> len = in.vec((int)in.i()), offs = offsets(len);
        const long long clock = read_device(m, in, &late);
        if (cmd == "announce") rc = pipe_announce(m, (int)len.size(), feats, offs.data(), &status);
        else if (pipe_decode_begin(m, (int)len.size(), feats, offs.data())) rc = pipe_decode_turn(m, clock, late, &status);
    } else if (cmd == "wait") {
        const long long clock = read_device(m, in, &late);
        if (m.have_pipe && m.pipe_on && !m.P.q.empty()) rc = pipe_decode_turn(m, clock, late, &status);   // (else: no decode is waiting)
    } else if (cmd == "quiesce") {
        (void)read_device(m, in, &late);
        if (m.have_pipe && m.pipe_on && m.res_on) rc = jd_res_stop(m);
    } else pipe_drain(m);
    finish(m, rc, status);
}

// ---- single decisions
static void run_harvest(const std::string &cmd, In &in, Model &m)
{
    // harvest chunk decouple max_batch table T_posted frame error exported UT ui row0: one slot, whose report is in, before the pump's step 1
    // harvest_many n: n slots whose utterances of one frame are through, none of them exported by its slot
    const bool many = cmd == "harvest_many";
    const int n = many ? (int)in.i() : 1;
    model_reset(m, 4, 0, n, 128, -1, -1, 0, -1);
    m.have_pipe = m.pipe_on = m.res_on = true;
    PipeState &P = m.P;
    P.K = 4; P.n_slots = n; P.table_rows = 1024;
    P.chunk = many ? PIPE_CHUNK : (int)in.i(); P.decouple = many ? true : in.i() != 0;
    P.max_batch = many ? n : (int)in.i();
    PipeBatch B;
    B.table = many ? 1 : (int)in.i();
    const int T_posted = many ? 1 : (int)in.i(), frame = many ? 1 : (int)in.i(), error = many ? 0 : (int)in.i(), exported = many ? 0 : (int)in.i();
    const int UT = many ? 1 : (int)in.i(), ui = many ? 0 : (int)in.i();
    const long long row0 = many ? 0 : in.i();
    B.n = many ? n : ui + 1; B.next = B.n; B.rows = B.rows_scored = (size_t)B.n * (size_t)UT; B.feats = &g_feats[0];
    B.u.resize((size_t)B.n); B.order.resize((size_t)B.n); B.offs.assign((size_t)B.n + 1, 0);
    P.table_used.assign(4, 0); P.table_used[(size_t)B.table] = 1;
    P.slot_batch_id.assign((size_t)n, -1); P.slot_utt.assign((size_t)n, -1); P.slot_dirty.assign((size_t)n, 0); P.slot_kexport.assign((size_t)n, 0);
    for (int u = 0; u < B.n; ++u) { B.order[(size_t)u] = u; B.u[(size_t)u].T = UT; B.u[(size_t)u].row0 = row0; B.u[(size_t)u].state = PIPE_UTT_THROUGH; }
    B.n_done = B.n;
    for (int s = 0; s < n; ++s) {
        const int u = many ? s : ui;
        B.u[(size_t)u].state = PIPE_UTT_RUNNING; B.u[(size_t)u].slot = s; B.n_done -= 1;
        P.slot_batch_id[(size_t)s] = 0; P.slot_utt[(size_t)s] = u;
        ResStream &S = m.stream[(size_t)s];
        S.seq = 1u; S.busy = true; S.T_posted = T_posted; S.slot_posted = (int)row0;
        m.done[(size_t)s] = Done{1u, frame, error, 0, exported};
    }
    P.q.push_back(std::move(B));
    m.table_pending.assign(4, 0);
    pump_harvest(m);
    finish(m, RC_OK, ST_NOT_THIS_WAY);
}
static void run_single(const std::string &cmd, In &in)
{
    if (cmd == "setting") {
        // setting depth slots max_streams n_cus slot_wg_per_cu lazy hybrid -> verdict depth slots
        const int depth = (int)in.i(), slots = (int)in.i(), streams = (int)in.i(), n_cus = (int)in.i(), per_cu = (int)in.i(), lazy = (int)in.i(), hybrid = (int)in.i();
        const PipeSetting S = pipe_setting(depth, slots, streams, n_cus, per_cu, lazy != 0, hybrid != 0);
        put(S.verdict); put(S.depth); put(S.slots);
    } else if (cmd == "size") {
        // size depth pipe_slots max_streams n_utts rows tile chunk_knob decouple_knob planned piece_knob
        //   -> K max_batch n_slots chunk decouple max_out piece_rows table_rows vslots   (a decoder's "pipe: size" line, JD_VERBOSE)
        PipeSizeIn si;
        si.depth = (int)in.i(); si.pipe_slots = (int)in.i(); si.max_streams = (int)in.i(); si.n_utts = (int)in.i(); si.rows = (size_t)in.i(); si.tile = (int)in.i();
        si.chunk_knob = (int)in.i(); si.decouple_knob = (int)in.i();
        const size_t planned = (size_t)in.i();
        const int piece_knob = (int)in.i();
        PipeState P;
        const size_t V = pipe_size(P, si);
        P.piece_rows = pipe_size_piece(P.decouple ? planned : 0, piece_knob, si.tile);   // (pipe_fill plans under decouple only)
        put(P.K); put(P.max_batch); put(P.n_slots); put(P.chunk); put(P.decouple); put(P.max_out); put((long long)P.piece_rows); put((long long)P.table_rows); put((long long)V);
    } else if (cmd == "bounds") {
        // bounds n_gmm group group_small tile -> lo hi groups
        const int n_gmm = (int)in.i(), group = (int)in.i(), small = (int)in.i(), tile = (int)in.i();
        const PipePieceBounds b = pipe_piece_bounds(n_gmm, group, small, tile);
        put(b.lo); put(b.hi); put(b.groups);
    } else if (cmd == "takes") {
        // takes pipe_mode lazy partial hybrid n_utts
        const int mode = (int)in.i(), lazy = (int)in.i(), partial = (int)in.i(), hybrid = (int)in.i(), n = (int)in.i();
        put(pipe_takes(mode != 0, lazy != 0, partial != 0, hybrid != 0, n));
    } else if (cmd == "outgrown" || cmd == "full") {
        // outgrown max_batch table_rows n_utts rows | full K queued
        PipeState P;
        if (cmd == "full") { P.K = (int)in.i(); P.q.resize((size_t)in.i()); put(pipe_full(P)); return; }
        P.max_batch = (int)in.i(); P.table_rows = (size_t)in.i();
        const int n = (int)in.i();
        put(pipe_outgrown(P, n, (size_t)in.i()));
    } else {
        // enqueue K table_rows used[K] n T[n] -> table row0[n] order[n]   (a decoder's "pipe: announce" line, JD_VERBOSE)
        PipeState P;
        P.K = (int)in.i(); P.table_rows = (size_t)in.i();
        for (int64_t u : in.vec(P.K)) P.table_used.push_back((char)u);
        const std::vector<int64_t> len = in.vec((int)in.i()), offs = offsets(len);
        const PipeBatch &B = pipe_enqueue(P, &g_feats[0], (int)len.size(), offs.data());
        put(B.table);
        for (const PipeUtt &U : B.u) put(U.row0);
        for (int o : B.order) put(o);
    }
}

int main()
{
    Model model;
    for (std::string line; std::getline(std::cin, line);) {
        if (line.empty()) continue;
        In in{std::istringstream(line)};
        std::string cmd;
        in.s >> cmd;
        g_out.clear();
        if (cmd == "reset" || cmd == "announce" || cmd == "decode" || cmd == "wait" || cmd == "quiesce" || cmd == "drain") run_script(cmd, in, model);
        else if (cmd == "harvest" || cmd == "harvest_many") run_harvest(cmd, in, model);
        else if (cmd == "setting" || cmd == "size" || cmd == "bounds" || cmd == "takes" || cmd == "outgrown" || cmd == "full" || cmd == "enqueue") run_single(cmd, in);
        else { fprintf(stderr, "pipe_driver: unknown command %s\n", cmd.c_str()); return 2; }
        for (size_t k = 0; k < g_out.size(); ++k) printf(k ? " %lld" : "%lld", g_out[k]);
        printf("\n");
        fflush(stdout);
    }
    return 0;
}
