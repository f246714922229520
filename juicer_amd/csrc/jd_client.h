// jd_client.h - the broker's (jd_broker.cpp) per-client DECISIONS: a client's record, the broker's settings, what each API call is
// answered with and what it changes, what its waits wait for, and what the two workers - the tick worker over jd_streams_push and
// the worker over the resident search kernel (jd_res_*) - decide about a client between two decoder calls.  Plain functions over a
// plain record, no HIP, no threads, no locks, no clock: times come in as microseconds.  jd_broker.cpp keeps the threads, the mutex,
// the condition variables, the clock and the decoder calls, and calls these with its lock held; tests/broker_driver.cpp runs them
// on the CPU (tests/test_broker_cpu.py), and tests/broker_harness.cpp runs the whole of jd_broker.cpp against a model decoder.
//
// Which combinations of a record's flags are legal is what brk_record_ok says (the tests hold every script step to it).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "juicer_amd.h"         // JD_OK, jd_hyp, jd_broker_stats

// ---- the workers' times, in microseconds
enum {
    BRK_IDLE_STOP_US = 3000,                           // the resident kernel leaves the chip after this long without work
    BRK_YIELD_AFTER_US = 20000,                        // ... and for somebody who waits for the device once it has had this long
    BRK_IDLE_WAIT_US = 200,                            // the resident worker's wait for a request while its kernel is there
    BRK_POLL_SLEEP_US = 20,                            // ... and its sleep between two rounds in which nothing moved
};

// ---- one client
struct BrkClient {
    bool open = false;
    bool want_init = false, want_finish = false;       // requests the worker has not served yet
    bool inited = false;                               // between init and finish
    std::vector<float> pending;                        // frames pushed and not yet handed to the decoder
    int err = JD_OK;                                   // first error of a tick that concerned this client (reported by its next call)
    std::string errmsg;
    bool failed = false;                               // its init or its stream failed: every call up to the next init() reports err
    jd_hyp result{};                                   // of the last finish (arrays owned by the decoder, valid until the stream's next init)
    // the resident kernel's worker: chunks of this client's frames that are scored (or being scored) and not yet posted - at
    // most two, one per likelihood buffer - and the one its cluster is running
    int staged_buf[2] = {0, 0}, staged_n[2] = {0, 0}, n_staged = 0;
    bool running = false; int run_buf = 0;
    bool fresh = false;                                // initialised and nothing posted yet (recognitionStart is still to run)
    bool finishing = false;                            // its result is being fetched (the finisher thread)
    unsigned init_req = 0;                             // counts the client's init() calls: one that arrives while the worker serves
                                                       // another (outside the lock) is still to be served behind it
    bool in_flight = false;                            // the worker holds something of this client outside the lock (frames being
                                                       // staged, a tick it is part of): close waits for that - the slot is somebody else's after it
    int64_t t_post = 0, t_idle = 0;                    // (statistics) its last command posted / found through
    bool was_idle = false;
    std::vector<float> taken;                          // frames on their way into the decoder (a tick's, a likelihood buffer's)
    std::vector<int32_t> plabel, ptime;                // its partialPaths as of the worker's last tick (jd_broker_partial; PARTIAL_DECODING)
};

// what must hold of a record whenever the broker's lock is free (0: all of it; else the number of the first rule broken)
static inline int brk_record_ok(const BrkClient &c)
{
    if (c.n_staged < 0 || c.n_staged > 2) return 1;
    if (c.n_staged + (c.running ? 1 : 0) > 2) return 2;
    if (c.n_staged == 2 && c.staged_buf[0] == c.staged_buf[1]) return 3;
    for (int k = 0; k < c.n_staged; ++k) {
        if (c.staged_buf[k] != 0 && c.staged_buf[k] != 1) return 4;
        if (c.running && c.staged_buf[k] == c.run_buf) return 5;
    }
    if (c.finishing && (c.running || c.n_staged > 0 || !c.inited)) return 6;
    if (!c.open && (c.want_init || c.want_finish || c.inited || !c.pending.empty() || c.running || c.n_staged > 0 || c.finishing || c.in_flight)) return 7;
    if (c.failed && c.err == JD_OK) return 8;
    return 0;
}

// ---- the broker's settings.  The knobs are the JD_BROKER_* strings of jd_dev_env (null: not set); trial_ok: the trial
// jd_res_start of jd_broker_create succeeded - the caller asks once with true to learn whether there is a trial to make and with
// how many rows, and again with its answer (a decoder the resident kernel refuses - a lazily composed network, partial traces -
// keeps the ticks, with the chunk length it was tried with).
struct BrkSettings {
    int max_tick_frames;                               // frames of one client a tick (a chunk) takes at most
    int max_pending_frames;                            // a push waits while its client holds more than this
    int coalesce_us;                                   // a tick waits this long for the other open clients' frames
    int partial_interval;                              // the decoder's: > 0, the tick worker keeps the clients' lists
    bool resident;                                     // the worker drives the resident search kernel instead of ticks
    int fail_init_of;                                  // test hook (JD_BROKER_FAIL_INIT=<client>): that client's inits fail
};
enum { BRK_MAX_RESIDENT_CLIENTS = 64 };                // the ready list of a scoring launch, and the chip's room for clusters and their scoring
static inline BrkSettings brk_settings(int n_clients, int partial_interval, const char *tick_frames, const char *coalesce_us, const char *resident,
                                       const char *fail_init, bool trial_ok)
{
    BrkSettings S{192, 0, 300, partial_interval, n_clients <= BRK_MAX_RESIDENT_CLIENTS, -1};
    bool tick_set = false;
    if (tick_frames) { const int v = atoi(tick_frames); if (v >= 1 && v <= 65536) S.max_tick_frames = v; tick_set = true; }
    if (coalesce_us) { const int v = atoi(coalesce_us); if (v >= 0 && v <= 1000000) S.coalesce_us = v; }
    if (resident) S.resident = atoi(resident) != 0;
    if (fail_init) S.fail_init_of = atoi(fail_init);
    if (S.resident && !tick_set) S.max_tick_frames = 256;              // (whole scoring tiles; a knob that is set and refused keeps 192)
    S.max_pending_frames = 4 * S.max_tick_frames;
    if (!trial_ok) S.resident = false;
    return S;
}

// ---- errors.  The first error that concerns a client stays with it until one of its calls reports it ...
static inline void brk_note_error(BrkClient &c, int rc, const std::string &msg)
{
    if (rc != JD_OK && c.err == JD_OK) { c.err = rc; c.errmsg = msg; }
}
// ... which clears it - unless its init or its stream failed: then every call up to the next init() reports it.  (The text is
// c.errmsg, which stays.)
static inline int brk_take_error(BrkClient &c)
{
    const int e = c.err;
    if (!c.failed) c.err = JD_OK;
    return e;
}
// An init that failed, or a stream that failed on the device: nothing more can be done for the utterance - what the client has
// pushed is dropped, and whoever waits (a push for room, a finish for its result) finds its wait over.  (Every caller notifies
// cv_done under the same hold of the lock.)
static inline void brk_client_failed(BrkClient &c, int rc, const std::string &msg)
{
    brk_note_error(c, rc, msg);
    c.failed = true;
    c.pending.clear(); c.n_staged = 0;
    c.want_finish = false;
}

// ---- predicates that several decisions share
static inline bool brk_in_utterance(const BrkClient &c) { return c.inited || c.want_init; }     // between init() and finish(), as the client sees it
static inline bool brk_finish_asked(const BrkClient &c) { return c.want_finish && c.pending.empty(); }   // finish(), and every frame before it handed on
// a request the worker has not served: both workers wake for it
static inline bool brk_has_request(const BrkClient &c)
{
    return c.open && (c.want_init || c.want_finish || (c.inited && !c.pending.empty()));
}
static inline int brk_pending_frames(const BrkClient &c, int D) { return (int)(c.pending.size() / (size_t)D); }
// the next frames of a client, at most max_frames, from pending to taken: the number taken
static inline int brk_take_frames(BrkClient &c, int D, int max_frames)
{
    const size_t have = c.pending.size() / (size_t)D;
    const size_t take = std::min(have, (size_t)max_frames);
    c.taken.assign(c.pending.begin(), c.pending.begin() + (ptrdiff_t)(take * D));
    c.pending.erase(c.pending.begin(), c.pending.begin() + (ptrdiff_t)(take * D));
    return (int)take;
}

// ---- the API calls: what a call is answered with before it does anything ...
enum BrkVerdict { BRK_OK = 0, BRK_NOT_OPEN, BRK_NOT_BETWEEN, BRK_CLIENT_ERROR };   // BRK_CLIENT_ERROR: brk_take_error, with c.errmsg
// jd_broker_open: the first client that is not open, as new; -1: all are taken
static inline int brk_open(std::vector<BrkClient> &C)
{
    for (size_t i = 0; i < C.size(); ++i)
        if (!C[i].open) { C[i] = BrkClient(); C[i].open = true; return (int)i; }
    return -1;
}
// jd_broker_close: an utterance that was never finished is dropped - its frames here, and what its cluster still has of them
// runs out before the slot is somebody else's (the wait) ...
static inline BrkVerdict brk_close_begin(BrkClient &c)
{
    if (!c.open) return BRK_NOT_OPEN;
    c.pending.clear(); c.want_finish = false;
    return BRK_OK;
}
static inline bool brk_close_may_go(const BrkClient &c) { return !c.want_init && !c.running && c.n_staged == 0 && !c.in_flight && !c.finishing; }
static inline void brk_close_end(BrkClient &c) { c.pending.clear(); c.want_finish = false; c.inited = false; c.open = false; }
// jd_broker_init: init() in the middle of an utterance drops it, as the reference does; one that is still waiting to be served -
// init() twice - is this one.  Nobody waits for the worker: an error of the init comes back with the next call.
static inline BrkVerdict brk_init(BrkClient &c)
{
    if (!c.open) return BRK_NOT_OPEN;
    c.pending.clear(); c.want_finish = false; c.err = JD_OK; c.failed = false;
    c.want_init = true;
    c.init_req += 1;
    c.plabel.clear(); c.ptime.clear();
    return BRK_OK;
}
// jd_broker_push: a failed init comes back here, not as "not between init and finish" ...
static inline BrkVerdict brk_push_begin(const BrkClient &c)
{
    if (!c.open) return BRK_NOT_OPEN;
    if (c.err != JD_OK) return BRK_CLIENT_ERROR;
    if (!brk_in_utterance(c) || c.want_finish) return BRK_NOT_BETWEEN;
    return BRK_OK;
}
// ... it waits for room (or for its client to fail) ...
static inline bool brk_push_may_go(const BrkClient &c, int D, int max_pending_frames) { return c.failed || brk_pending_frames(c, D) <= max_pending_frames; }
// ... and the error is looked for once more behind the wait
static inline BrkVerdict brk_push_end(BrkClient &c, const float *frames, int n_frames, int D)
{
    if (c.err != JD_OK) return BRK_CLIENT_ERROR;
    c.pending.insert(c.pending.end(), frames, frames + (size_t)n_frames * (size_t)D);
    return BRK_OK;
}
// jd_broker_finish: a client whose init failed has no utterance to finish ...
static inline BrkVerdict brk_finish_begin(BrkClient &c)
{
    if (!c.open) return BRK_NOT_OPEN;
    if (c.failed && !c.inited) return BRK_CLIENT_ERROR;
    if (!brk_in_utterance(c)) return BRK_NOT_BETWEEN;
    c.want_finish = true;
    return BRK_OK;
}
// ... it waits for the worker to take the request back, and reports the client's error or c.result
static inline bool brk_finish_may_go(const BrkClient &c) { return !c.want_finish; }
static inline BrkVerdict brk_finish_end(const BrkClient &c) { return c.err != JD_OK ? BRK_CLIENT_ERROR : BRK_OK; }
// jd_broker_partial reads c.plabel / c.ptime of an open client
static inline BrkVerdict brk_partial(const BrkClient &c) { return c.open ? BRK_OK : BRK_NOT_OPEN; }

// a result fetched - by the tick worker, by the finisher thread: the utterance is over
static inline void brk_finished(BrkClient &c, const jd_hyp &res)
{
    c.want_finish = false; c.inited = false; c.finishing = false; c.result = res;
}

// ---- the tick worker
static inline bool brk_tick_has_work(const std::vector<BrkClient> &C)
{
    for (const BrkClient &c : C)
        if (brk_has_request(c)) return true;
    return false;
}
// the coalescing wait ends early once no open client is still to deliver (one that has asked for its result is not)
static inline bool brk_tick_all_ready(const std::vector<BrkClient> &C)
{
    for (const BrkClient &c : C)
        if (c.open && !c.want_finish && c.pending.empty()) return false;
    return true;
}
// A tick: the clients whose init it serves (init_seen: the init() it serves for each), whose frames it takes (in c.taken; frames
// pushed behind an init that has not been served yet go with it - the init comes first) and whose results it fetches (their last
// frames - and their init - go with this tick too).  All of them are in flight until brk_tick_settle.  init_seen lives as long as
// the worker.
struct BrkTick {
    std::vector<int> inits, pushers, finishers;
    std::vector<unsigned> init_seen;
};
static inline void brk_tick_select(std::vector<BrkClient> &C, int D, int max_tick_frames, BrkTick *T)
{
    T->inits.clear(); T->pushers.clear(); T->finishers.clear();
    T->init_seen.resize(C.size(), 0u);
    for (size_t i = 0; i < C.size(); ++i) {
        BrkClient &c = C[i];
        if (!c.open) continue;
        if (c.want_init) { T->inits.push_back((int)i); T->init_seen[i] = c.init_req; }
        if (brk_in_utterance(c) && !c.pending.empty()) {
            (void)brk_take_frames(c, D, max_tick_frames);
            T->pushers.push_back((int)i);
        }
    }
    // (no `inited` here: a finish behind an init of this very tick is served by it, and one behind nothing - finish() refuses that)
    for (size_t i = 0; i < C.size(); ++i)
        if (C[i].open && brk_finish_asked(C[i])) T->finishers.push_back((int)i);
    for (int i : T->inits) C[(size_t)i].in_flight = true;
    for (int i : T->pushers) C[(size_t)i].in_flight = true;
    for (int i : T->finishers) C[(size_t)i].in_flight = true;
}
// A caller whose last frames went with the tick and who asked for its result while the search ran is served at the tick's end -
// not at the end of the next one, which it would sit out.  Unlike a finisher of brk_tick_select it has not had its init looked at
// by this tick: it must be initialised, with no init waiting, and nothing of the tick may have failed for it (rc: the tick's so far).
static inline bool brk_tick_late_finisher(const BrkClient &c, int rc, bool is_finisher)
{
    return c.open && brk_finish_asked(c) && !c.want_init && c.inited && rc == JD_OK && !is_finisher;
}
static inline bool brk_in(const std::vector<int> &v, int i) { return std::find(v.begin(), v.end(), i) != v.end(); }
static inline void brk_tick_late(const std::vector<BrkClient> &C, const BrkTick &T, const std::vector<int> &rc_of, std::vector<int> *late)
{
    late->clear();
    for (size_t i = 0; i < C.size(); ++i)
        if (brk_tick_late_finisher(C[i], rc_of[i], brk_in(T.finishers, (int)i))) late->push_back((int)i);
}
// PARTIAL_DECODING: the clients whose lists are fetched behind a tick (T.finishers with the late ones) - the pushers it did not
// fail for, then the finishers that are not among them ...
static inline void brk_tick_listed(const BrkTick &T, const std::vector<int> &rc_of, std::vector<int> *listed)
{
    listed->clear();
    for (int i : T.pushers) if (rc_of[(size_t)i] == JD_OK) listed->push_back(i);
    for (int i : T.finishers) if (!brk_in(*listed, i)) listed->push_back(i);
}
// ... and whether client i keeps what was fetched: not when an init() came while the tick ran - the list is of the utterance it dropped
static inline bool brk_tick_keeps_list(const BrkClient &c, const BrkTick &T, int i)
{
    if (c.want_init && c.init_req != T.init_seen[(size_t)i]) return false;
    if (c.want_init && !brk_in(T.inits, i)) return false;
    return true;
}
// The tick is over (T.finishers with the late ones; rc_of / msg_of: what failed for whom, res: the finishers' results): errors to
// their clients; an init is served unless init() was called again meanwhile (the next tick's); a failed init fails the client -
// the frames behind it and a finish that waits for them would wait for ever (pushers need inited, finishers an empty queue);
// results to the finishers; nobody is in flight.
static inline void brk_tick_settle(std::vector<BrkClient> &C, const BrkTick &T, const std::vector<int> &rc_of, const std::vector<std::string> &msg_of,
                                   const std::vector<jd_hyp> &res)
{
    for (size_t i = 0; i < C.size(); ++i) brk_note_error(C[i], rc_of[i], msg_of[i]);
    for (int i : T.inits) {
        BrkClient &c = C[(size_t)i];
        if (c.init_req == T.init_seen[(size_t)i]) c.want_init = false;
        c.inited = rc_of[(size_t)i] == JD_OK;
        if (!c.inited && !c.want_init) brk_client_failed(c, rc_of[(size_t)i], msg_of[(size_t)i]);
    }
    for (int i : T.finishers) brk_finished(C[(size_t)i], res[(size_t)i]);
    for (BrkClient &c : C) c.in_flight = false;
}
// (statistics) a tick that pushed something
static inline void brk_tick_count(jd_broker_stats &st, long long frames, long long streams)
{
    if (streams) { st.ticks += 1; st.frames += frames; st.stream_ticks += streams; }
}

// ---- the worker over the resident kernel.  Its kernel is there (on) while somebody has a request or something under way ...
static inline bool brk_res_active(const std::vector<BrkClient> &C)
{
    for (const BrkClient &c : C)
        if (brk_has_request(c) || (c.open && (c.running || c.finishing || c.n_staged > 0))) return true;
    return false;
}
// ... leaves the chip after a few milliseconds without (other decoders, other processes, a caller's device-wide synchronisation
// all wait for it) ...
static inline bool brk_res_stop_when_idle(bool on, int64_t idle_us) { return on && idle_us > BRK_IDLE_STOP_US; }
// ... and makes room for somebody of this process who waits for the device once it has had its time: no new commands (draining),
// and when nothing runs any more the kernel leaves and comes back behind the one that waited
static inline bool brk_res_drain_due(bool should_yield, int64_t on_us) { return should_yield && on_us > BRK_YIELD_AFTER_US; }
static inline bool brk_res_any_running(const std::vector<BrkClient> &C)
{
    for (const BrkClient &c : C)
        if (c.running || c.finishing) return true;
    return false;
}
// jd_res_start failed, or a poll (the kernel has ended): every open client gets the error, and everything anybody waits for is over
static inline void brk_fail_all(std::vector<BrkClient> &C, int rc, const std::string &msg)
{
    for (BrkClient &c : C)
        if (c.open && c.err == JD_OK) { c.err = rc; c.errmsg = msg; }
    for (BrkClient &c : C) { c.want_init = false; c.want_finish = false; c.pending.clear(); c.n_staged = 0; c.running = false; }
}
// A round looks at every client that is open and not with the finisher, in this order:
static inline bool brk_res_looks_at(const BrkClient &c) { return c.open && !c.finishing; }
// 1. where its cluster stands (c.running: jd_res_poll).  A poll that finds the command through with a device error (an arena
// overflow, Histogram's ceiling, a lost workgroup) fails the stream: no more chunks are scored or posted for it and the client's
// next call says why - but a finish under way stays asked for: it goes through brk_res_may_finish as usual, fetches and reports the same
// (a command that stopped short for a Path collection is not through: jd_res_collect sends the rest of it on, the poll counts as "not idle")
static inline bool brk_res_collection_due(int idle, int stopped) { return idle && stopped; }
static inline bool brk_res_stream_fails(const BrkClient &c, int idle, int dev_err) { return idle && dev_err != 0 && !c.failed; }
static inline void brk_res_stream_failed(BrkClient &c, int rc, const std::string &msg)
{
    const bool wf = c.want_finish;
    brk_client_failed(c, rc, msg);
    c.want_finish = wf;
}
// ... the command is through (statistics: us_search, from its post to here)
static inline void brk_res_idle(BrkClient &c, int64_t now_us, jd_broker_stats &st)
{
    c.running = false;
    c.t_idle = now_us; c.was_idle = true;
    st.us_search += c.t_idle - c.t_post;
}
// 2. IDecoder::init (req: c.init_req as the worker found it; init() again meanwhile is served in the next round).  A failed one
// fails the client - a push that waits for room, a finish - unless the next is asked for already
static inline bool brk_res_may_init(const BrkClient &c) { return !c.running && c.n_staged == 0 && c.want_init; }
static inline void brk_res_inited(BrkClient &c, unsigned req, int rc, const std::string &msg)
{
    if (c.init_req == req) c.want_init = false;
    c.inited = rc == JD_OK; c.fresh = rc == JD_OK; c.was_idle = false;
    if (rc && !c.want_init) brk_client_failed(c, rc, msg);
    else brk_note_error(c, rc, msg);
}
// 4. the next chunk to the cluster (before 3: what is scored already goes first).  A finish without frames still runs
// recognitionStart: a chunk of none, in buffer 0
static inline bool brk_res_may_post(const BrkClient &c, bool draining)
{
    return !draining && !c.running && c.inited && (c.n_staged > 0 || (c.fresh && brk_finish_asked(c)));
}
static inline int brk_res_post_buf(const BrkClient &c) { return c.n_staged > 0 ? c.staged_buf[0] : 0; }
static inline int brk_res_post_frames(const BrkClient &c) { return c.n_staged > 0 ? c.staged_n[0] : 0; }
// ... posted (buf, nf as asked above) or not: the staged queue moves up either way (statistics: a chunk is a tick of one stream;
// us_idle: what a cluster waited between two chunks of ONE utterance)
static inline void brk_res_posted(BrkClient &c, int rc, const std::string &msg, int buf, int nf, int64_t now_us, jd_broker_stats &st)
{
    brk_note_error(c, rc, msg);
    if (c.n_staged > 0) { c.staged_buf[0] = c.staged_buf[1]; c.staged_n[0] = c.staged_n[1]; c.n_staged -= 1; }
    if (rc) return;
    c.running = true; c.run_buf = buf; c.fresh = false;
    st.ticks += 1; st.frames += nf; st.stream_ticks += 1;
    c.t_post = now_us;
    if (c.was_idle) st.us_idle += c.t_post - c.t_idle;
}
// 3. frames for a free likelihood buffer.  Unlike push(), which accepts frames behind an init that is still to be served, staging
// waits for that init: the frames are the next utterance's
static inline bool brk_res_may_stage(const BrkClient &c)
{
    return c.inited && !c.failed && !c.want_init && !c.pending.empty() && c.n_staged + (c.running ? 1 : 0) < 2;
}
// ... the buffer: not the running one, not the staged one; -1: none (the three steps are kept as they were: with a chunk running in
// one buffer and the other staged - both taken, which brk_res_may_stage has ruled out before - the choice comes back to the running
// buffer and is refused)
static inline int brk_res_stage_buf(const BrkClient &c)
{
    int buf = 0;
    if (c.running && c.run_buf == 0) buf = 1;
    if (c.n_staged == 1 && c.staged_buf[0] == buf) buf ^= 1;
    return (c.running && c.run_buf == buf) ? -1 : buf;
}
// ... taken for this round's staging call (in c.taken): the number of frames
static inline int brk_res_stage_take(BrkClient &c, int D, int max_tick_frames)
{
    c.in_flight = true;
    return brk_take_frames(c, D, max_tick_frames);
}
// ... and the call's result: the chunk joins the staged queue, or the call's error is the client's
static inline void brk_res_staged(BrkClient &c, int rc, const std::string &msg, int buf, int nf)
{
    if (rc) brk_note_error(c, rc, msg);
    else { c.staged_buf[c.n_staged] = buf; c.staged_n[c.n_staged] = nf; c.n_staged += 1; }
    c.in_flight = false;
}
// 5. IDecoder::finish: everything posted and through, the first command (recognitionStart) among it; handed to the finisher
// thread, which ends with brk_finished
static inline bool brk_res_may_finish(const BrkClient &c)
{
    return !c.running && c.n_staged == 0 && c.inited && !c.fresh && brk_finish_asked(c);
}
static inline void brk_res_to_finisher(BrkClient &c) { c.finishing = true; }
