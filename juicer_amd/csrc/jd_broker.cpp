// jd_broker.cpp - many IDecoder instances on the streams of ONE decoder.
//
// The reference's harness is serial: DecoderBatchTest::run decodes one list entry after the other through one
// IDecoder (src/DecoderBatchTest.cpp:738-771 -> DecoderSingleTest::decodeUtterance, src/DecoderSingleTest.cpp:259-324),
// and its users scale out by running several such processes over split file lists (doc/userman/juicer_userman.tex:584).
// A GPU decoder serves one utterance at a few hundred times real time but a batch of them at ten thousand: the
// search is a chain of dependent steps per frame, and the chip is filled by running many utterances side by side.
// The broker is what lets N serial harness threads do that without knowing of each other: every thread drives its own
// client with the IDecoder protocol - init, push (processFrame x n), finish - and a worker thread turns whatever has
// been pushed since its last tick into ONE scoring launch and ONE persistent search launch over all the streams
// concerned (jd_streams_push), or - up to 64 clients - keeps every client's stream fed in a search kernel that stays
// (jd_res_*).  Clients never touch the decoder: only the worker thread does (and the finisher thread beside the resident
// worker, for results), so the decoder's single-caller rule holds.  PARTIAL_DECODING (an interval set on the decoder before
// jd_broker_create): the tick worker, whose jd_streams_push keeps every stream's trace schedule, leaves each client's partialPaths
// with the client after every tick (jd_broker_partial).
//
// What is decided about a client - what a call is answered with, what a wait waits for, what a tick takes, what a round of the
// resident worker may do for it and what a decoder call's result does to it - is jd_client.h: plain functions over the client's
// record, tested on the CPU.  This file is the rest: the threads, the lock, the three condition variables and who is woken when,
// the clock, and the decoder calls in their order, inside the lock and outside it.  Host code over the C ABI only - nothing here
// knows about HIP, so tests/broker_harness.cpp links this very file against a model decoder and runs it with its threads.
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "jd_client.h"
#include "jd_internal.h"

struct jd_broker {
    jd_dec *dec = nullptr;
    int D = 0, n_clients = 0;
    BrkSettings S{};
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::thread worker;
    bool stop = false;
    std::vector<BrkClient> clients;
    jd_broker_stats stats{};
    // results are fetched by a thread of their own: recognitionFinish's kernel, a synchronisation of the side stream and
    // three copies back are a third of a millisecond in which the worker would post nothing to anybody
    std::thread finisher;
    std::deque<int> fin_q;
    std::condition_variable cv_fin;
};

static int64_t now_us()
{
    return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static int64_t us_since(int64_t t) { return now_us() - t; }

static int client_error(BrkClient &c)
{
    if (c.err == JD_OK) return JD_OK;
    return jd_fail(brk_take_error(c), "%s", c.errmsg.c_str());
}
static int init_stream(jd_broker *b, int i, bool resident)
{
    if (i == b->S.fail_init_of) return jd_fail(JD_EHIP, "jd_broker: init failure injected for client %d", i);
    return resident ? jd_res_init(b->dec, i) : jd_stream_init(b->dec, i);
}

static void broker_loop(jd_broker *b)
{
    std::unique_lock<std::mutex> lk(b->mu);
    std::vector<BrkClient> &C = b->clients;
    BrkTick T;
    std::vector<int> late, listed;
    double search_ms_seen = 0.0;                   // (jd_timing accumulates over the streaming calls)
    for (;;) {
        int64_t t_mark = now_us();
        b->cv_work.wait(lk, [&]() { return b->stop || brk_tick_has_work(C); });
        if (b->stop) return;
        b->stats.us_idle += us_since(t_mark); t_mark = now_us();
        // a tick is the fuller the more clients have frames waiting: give the open ones that have nothing pending yet
        // a moment to deliver - they are all being fed at about the same rate, and one that has just been handed its
        // result is about to start its next utterance (a caller that is through closes its client)
        if (b->S.coalesce_us > 0) {
            b->cv_work.wait_for(lk, std::chrono::microseconds(b->S.coalesce_us), [&]() { return b->stop || brk_tick_all_ready(C); });
            if (b->stop) return;
            b->stats.us_coalesce += us_since(t_mark);
        }
        brk_tick_select(C, b->D, b->S.max_tick_frames, &T);
        lk.unlock();
        b->cv_done.notify_all();                                       // (pushes that waited for room)
        // ---- the decoder is touched from here only
        long long tick_frames = 0, tick_streams = 0;
        std::vector<int> rc_of((size_t)b->n_clients, JD_OK);
        std::vector<std::string> msg_of((size_t)b->n_clients);
        int64_t us_init = 0, us_push = 0, us_finish = 0, us_search = 0;
        t_mark = now_us();
        for (int i : T.inits) {
            rc_of[(size_t)i] = init_stream(b, i, false);
            if (rc_of[(size_t)i]) msg_of[(size_t)i] = jd_last_error();
        }
        us_init = us_since(t_mark); t_mark = now_us();
        if (!T.pushers.empty()) {
            std::vector<int32_t> ss, nn;
            std::vector<const float *> ff;
            long long fr = 0;
            for (int i : T.pushers) {
                if (rc_of[(size_t)i] != JD_OK) continue;               // (its init failed)
                ss.push_back(i); ff.push_back(C[(size_t)i].taken.data()); nn.push_back((int32_t)(C[(size_t)i].taken.size() / (size_t)b->D));
                fr += nn.back();
            }
            const int rc = ss.empty() ? JD_OK : jd_streams_push(b->dec, (int32_t)ss.size(), ss.data(), ff.data(), nn.data());
            if (rc) {
                const std::string m = jd_last_error();
                for (int i : T.pushers) if (rc_of[(size_t)i] == JD_OK) { rc_of[(size_t)i] = rc; msg_of[(size_t)i] = m; }
            }
            tick_frames = fr; tick_streams = (long long)ss.size();
            jd_timing tm;
            if (!ss.empty() && jd_dec_last_timing(b->dec, &tm) == JD_OK) {
                us_search = (int64_t)((tm.search_ms - search_ms_seen) * 1e3);
                search_ms_seen = tm.search_ms;
            }
        }
        us_push = us_since(t_mark); t_mark = now_us();
        std::vector<jd_hyp> res((size_t)b->n_clients);
        auto serve_finishes = [&](const std::vector<int> &who) {
            for (int i : who) {
                memset(&res[(size_t)i], 0, sizeof(jd_hyp));
                const int rc = jd_stream_finish(b->dec, i, &res[(size_t)i]);
                if (rc && rc_of[(size_t)i] == JD_OK) { rc_of[(size_t)i] = rc; msg_of[(size_t)i] = jd_last_error(); }
            }
        };
        serve_finishes(T.finishers);
        lk.lock();
        brk_tick_late(C, T, rc_of, &late);
        lk.unlock();
        serve_finishes(late);
        T.finishers.insert(T.finishers.end(), late.begin(), late.end());
        // PARTIAL_DECODING: the lists of the clients this tick concerned, copied where jd_broker_partial finds them
        std::vector<std::vector<int32_t>> pl, pt;
        listed.clear();
        if (b->S.partial_interval > 0) {
            brk_tick_listed(T, rc_of, &listed);
            pl.resize(listed.size()); pt.resize(listed.size());
            for (size_t k = 0; k < listed.size(); ++k) {
                int32_t np = 0;
                if (jd_stream_partial(b->dec, listed[k], 0, 0, &np, nullptr, nullptr, nullptr) != JD_OK || np == 0) continue;
                pl[k].resize((size_t)np); pt[k].resize((size_t)np);
                (void)jd_stream_partial(b->dec, listed[k], 0, np, &np, pl[k].data(), pt[k].data(), nullptr);
            }
        }
        us_finish = us_since(t_mark);
        lk.lock();
        for (size_t k = 0; k < listed.size(); ++k) {
            BrkClient &c = C[(size_t)listed[k]];
            if (brk_tick_keeps_list(c, T, listed[k])) { c.plabel.swap(pl[k]); c.ptime.swap(pt[k]); }
        }
        b->stats.us_init += us_init; b->stats.us_push += us_push; b->stats.us_finish += us_finish;
        b->stats.us_search += us_search;
        brk_tick_count(b->stats, tick_frames, tick_streams);
        brk_tick_settle(C, T, rc_of, msg_of, res);
        b->cv_done.notify_all();
    }
}


// The worker over the RESIDENT search kernel (jd_resident.h): no ticks.  Every client's stream has a cluster of its own in a
// kernel that stays; its frames are scored into one of the stream's two likelihood buffers as they come (on the side
// stream, beside the search) and posted to the cluster as soon as it is through with the chunk before - every stream at
// its own pace.  init, finish and the Path collections are small kernels on the side stream between two commands.
static void broker_loop_resident(jd_broker *b)
{
    std::unique_lock<std::mutex> lk(b->mu);
    std::vector<BrkClient> &C = b->clients;
    std::vector<int> st_s, st_b, st_n;                                // this round's staging: streams, buffers, frames
    std::vector<const float *> st_f;
    bool on = false;
    bool draining = false;                                            // somebody waits for the device: no new commands, then the kernel makes room
    int64_t idle_since = now_us(), on_since = now_us();
    bool progress = false;
    auto fail_all = [&](int rc, const std::string &msg) {              // (lk held)
        brk_fail_all(C, rc, msg);
        b->cv_done.notify_all();
    };
    auto try_post = [&](int i) {                                       // (lk held)
        BrkClient &c = C[(size_t)i];
        if (!brk_res_may_post(c, draining)) return;
        const int buf = brk_res_post_buf(c), nf = brk_res_post_frames(c);
        lk.unlock();
        const int rc = jd_res_post(b->dec, i, buf, nf);
        const std::string m = rc ? jd_last_error() : "";
        lk.lock();
        brk_res_posted(c, rc, m, buf, nf, now_us(), b->stats);
        progress = true;
    };
    for (;;) {
        const bool active = brk_res_active(C);
        if (b->stop) { if (on) { lk.unlock(); (void)jd_res_stop(b->dec); lk.lock(); } return; }
        if (!active) {
            // nothing to do: the kernel leaves the chip after a few milliseconds and comes back with the next request
            if (brk_res_stop_when_idle(on, us_since(idle_since))) {
                lk.unlock(); (void)jd_res_stop(b->dec); lk.lock();
                on = false;
                continue;
            }
            if (on) b->cv_work.wait_for(lk, std::chrono::microseconds(BRK_IDLE_WAIT_US));
            else b->cv_work.wait(lk);
            continue;
        }
        if (!on) {
            lk.unlock();
            const int rc = jd_res_start(b->dec, b->n_clients, b->S.max_tick_frames);
            const std::string m = rc ? jd_last_error() : "";
            lk.lock();
            if (rc) { fail_all(rc, m); continue; }
            on = true; draining = false; on_since = now_us();
        }
        // another decoder's launch (or another broker's kernel) of this process waits for the device: the chunks that are
        // running run out, the kernel leaves, and comes back behind the one that waited
        if (!draining && brk_res_drain_due(jd_res_should_yield(b->dec) != 0, us_since(on_since))) draining = true;
        if (draining && !brk_res_any_running(C)) {
            lk.unlock(); (void)jd_res_yield(b->dec); lk.lock();
            on = false; draining = false;
            continue;
        }
        progress = false;
        for (int i = 0; i < b->n_clients; ++i) {
            BrkClient &c = C[(size_t)i];
            if (!brk_res_looks_at(c)) continue;
            // 1. where its cluster stands
            if (c.running) {
                int idle = 0, frame = 0, err = 0, stopped = 0;
                lk.unlock();
                int rc = jd_res_poll(b->dec, i, &idle, &frame, &err, &stopped);
                if (rc == JD_OK && brk_res_collection_due(idle, stopped)) { rc = jd_res_collect(b->dec, i); idle = 0; progress = true; }
                const std::string m = rc ? jd_last_error() : "";
                lk.lock();
                if (rc) { fail_all(rc, m); on = false; lk.unlock(); (void)jd_res_stop(b->dec); lk.lock(); break; }
                if (brk_res_stream_fails(c, idle, err)) {
                    lk.unlock();
                    const int er = jd_res_stream_error(b->dec, i, err, frame);
                    const std::string em = jd_last_error();
                    lk.lock();
                    brk_res_stream_failed(c, er, em);
                }
                if (idle) { progress = true; b->cv_done.notify_all(); brk_res_idle(c, now_us(), b->stats); }   // (the clock is read behind the wake-up, as ever)
            }
            // 2. IDecoder::init
            if (brk_res_may_init(c)) {
                const unsigned req = c.init_req;
                lk.unlock();
                const int rc = init_stream(b, i, true);
                const std::string m = rc ? jd_last_error() : "";
                lk.lock();
                brk_res_inited(c, req, rc, m);
                b->cv_done.notify_all();                               // (a push that waits for room, a finish: woken with the error)
                progress = true;
            }
            try_post(i);                                                // 4. (what is scored already goes first: a word in host memory)
            // 3. frames for a free likelihood buffer: taken here, scored below - one launch for all the streams of this round
            if (brk_res_may_stage(c)) {
                const int buf = brk_res_stage_buf(c);
                if (buf >= 0) {
                    const int take = brk_res_stage_take(c, b->D, b->S.max_tick_frames);
                    st_s.push_back(i); st_b.push_back(buf); st_f.push_back(c.taken.data()); st_n.push_back(take);
                }
            }
        }
        if (!st_s.empty()) {
            lk.unlock();
            b->cv_done.notify_all();                                   // (pushes that waited for room)
            const int64_t t_st = now_us();
            const int rc = jd_res_stage_many(b->dec, (int)st_s.size(), st_s.data(), st_b.data(), st_f.data(), st_n.data());
            const std::string m = rc ? jd_last_error() : "";
            lk.lock();
            b->stats.us_push += us_since(t_st);
            for (size_t k = 0; k < st_s.size(); ++k) brk_res_staged(C[(size_t)st_s[k]], rc, m, st_b[k], st_n[k]);
            b->cv_done.notify_all();
            st_s.clear(); st_b.clear(); st_f.clear(); st_n.clear();
            progress = true;
        }
        for (int i = 0; i < b->n_clients; ++i) {
            BrkClient &c = C[(size_t)i];
            if (!brk_res_looks_at(c)) continue;
            try_post(i);
            // 5. IDecoder::finish (handed to the finisher thread)
            if (brk_res_may_finish(c)) {
                brk_res_to_finisher(c);
                b->fin_q.push_back(i);
                b->cv_fin.notify_one();
                progress = true;
            }
        }
        if (!progress) {
            // (the clusters report through host-mapped words: looking again costs nothing on the device)
            lk.unlock();
            std::this_thread::sleep_for(std::chrono::microseconds(BRK_POLL_SLEEP_US));
            lk.lock();
        }
        idle_since = now_us();
    }
}

static void broker_finisher(jd_broker *b)
{
    std::unique_lock<std::mutex> lk(b->mu);
    for (;;) {
        b->cv_fin.wait(lk, [&]() { return b->stop || !b->fin_q.empty(); });
        if (b->fin_q.empty()) return;                                  // (stop, and nothing left to hand out)
        const int i = b->fin_q.front();
        b->fin_q.pop_front();
        jd_hyp res;
        memset(&res, 0, sizeof res);
        lk.unlock();
        const int64_t t_f = now_us();
        const int rc = jd_res_finish(b->dec, i, &res);
        const std::string m = rc ? jd_last_error() : "";
        lk.lock();
        b->stats.us_finish += us_since(t_f);
        BrkClient &c = b->clients[(size_t)i];
        brk_note_error(c, rc, m);
        brk_finished(c, res);
        b->cv_done.notify_all();
        b->cv_work.notify_all();
    }
}

extern "C" int jd_broker_create(jd_broker **out, jd_dec *dec, int32_t n_clients)
{
    if (!out || !dec || n_clients < 1) return jd_fail(JD_EINVAL, "jd_broker_create: bad argument");
    int32_t ms = 0, D = 0;
    int rc = jd_dec_info(dec, &ms, &D);
    if (rc) return rc;
    if (n_clients > ms) return jd_fail(JD_EINVAL, "jd_broker_create: %d clients on a decoder of %d streams", n_clients, ms);
    if (jd_dec_spliced && jd_dec_spliced(dec))
        return jd_fail(JD_EINVAL, "jd_broker_create: the decoder's models are spliced (jd_am_mlp_splice), and splicing is served one stream at a time "
                       "(jd_stream_push), not by a broker");
    int32_t level = 0;
    rc = jd_dec_get_output_level(dec, &level);
    if (rc) return rc;
    if (level & JD_OUTPUT_MODELS) return jd_fail(JD_EINVAL, "jd_broker_create: a broker serves word output only (the decoder's output level has JD_OUTPUT_MODELS)");
    int32_t interval = 0;
    rc = jd_dec_get_partial_interval(dec, &interval);
    if (rc) return rc;
    // the resident search kernel instead of ticks (JD_BROKER_RESIDENT=0: ticks): not with a lazily composed network or partial
    // traces - jd_res_start says so and the clients' first calls would fail, so those decoders keep the ticks
    const char *k_tick = jd_dev_env("JD_BROKER_TICK_FRAMES"), *k_coalesce = jd_dev_env("JD_BROKER_COALESCE_US");
    const char *k_resident = jd_dev_env("JD_BROKER_RESIDENT"), *k_fail = jd_dev_env("JD_BROKER_FAIL_INIT");
    BrkSettings S = brk_settings(n_clients, interval, k_tick, k_coalesce, k_resident, k_fail, true);
    if (S.resident) {
        const bool ok = jd_res_start(dec, n_clients, S.max_tick_frames) == JD_OK;
        if (ok) (void)jd_res_stop(dec);                                // (it comes back with the first request)
        S = brk_settings(n_clients, interval, k_tick, k_coalesce, k_resident, k_fail, ok);
    }
    jd_broker *b = new jd_broker();
    b->dec = dec; b->D = D; b->n_clients = n_clients; b->S = S;
    b->clients.resize((size_t)n_clients);
    b->worker = S.resident ? std::thread(broker_loop_resident, b) : std::thread(broker_loop, b);
    if (S.resident) b->finisher = std::thread(broker_finisher, b);
    *out = b;
    return JD_OK;
}

extern "C" void jd_broker_destroy(jd_broker *b)
{
    if (!b) return;
    { std::lock_guard<std::mutex> lk(b->mu); b->stop = true; }
    b->cv_work.notify_all(); b->cv_done.notify_all(); b->cv_fin.notify_all();
    if (b->finisher.joinable()) b->finisher.join();
    if (b->worker.joinable()) b->worker.join();
    delete b;
}

extern "C" int jd_broker_open(jd_broker *b, int32_t *client)
{
    if (!b || !client) return jd_fail(JD_EINVAL, "jd_broker_open: bad argument");
    std::lock_guard<std::mutex> lk(b->mu);
    const int i = brk_open(b->clients);
    if (i < 0) return jd_fail(JD_ESTATE, "jd_broker_open: all %d clients are taken", b->n_clients);
    *client = i;
    return JD_OK;
}

extern "C" int jd_broker_close(jd_broker *b, int32_t client)
{
    if (!b || client < 0 || client >= b->n_clients) return jd_fail(JD_EINVAL, "jd_broker_close: bad client");
    std::unique_lock<std::mutex> lk(b->mu);
    BrkClient &c = b->clients[(size_t)client];
    if (brk_close_begin(c) == BRK_NOT_OPEN) return jd_fail(JD_ESTATE, "jd_broker_close: client %d is not open", client);
    b->cv_work.notify_all();
    b->cv_done.wait(lk, [&]() { return b->stop || brk_close_may_go(c); });
    brk_close_end(c);
    return JD_OK;
}

extern "C" int jd_broker_init(jd_broker *b, int32_t client)
{
    if (!b || client < 0 || client >= b->n_clients) return jd_fail(JD_EINVAL, "jd_broker_init: bad client");
    std::unique_lock<std::mutex> lk(b->mu);
    if (brk_init(b->clients[(size_t)client]) == BRK_NOT_OPEN) return jd_fail(JD_ESTATE, "jd_broker_init: client %d is not open", client);
    // nobody waits for the worker here: the stream is initialised at the head of the next tick, in front of whatever
    // frames this client has pushed by then (an error of it comes back with the next call)
    b->cv_work.notify_all();
    return JD_OK;
}

extern "C" int jd_broker_push(jd_broker *b, int32_t client, const float *frames, int32_t n_frames)
{
    if (!b || client < 0 || client >= b->n_clients || n_frames < 0 || (n_frames > 0 && !frames))
        return jd_fail(JD_EINVAL, "jd_broker_push: bad argument");
    std::unique_lock<std::mutex> lk(b->mu);
    BrkClient &c = b->clients[(size_t)client];
    switch (brk_push_begin(c)) {
    case BRK_NOT_OPEN: return jd_fail(JD_ESTATE, "jd_broker_push: client %d is not open", client);
    case BRK_CLIENT_ERROR: return client_error(c);
    case BRK_NOT_BETWEEN: return jd_fail(JD_ESTATE, "jd_broker_push: client %d is not between init and finish", client);
    case BRK_OK: break;
    }
    b->cv_done.wait(lk, [&]() { return b->stop || brk_push_may_go(c, b->D, b->S.max_pending_frames); });
    if (brk_push_end(c, frames, n_frames, b->D) == BRK_CLIENT_ERROR) return client_error(c);   // (it failed while this push waited for room)
    b->cv_work.notify_all();
    return JD_OK;
}

extern "C" int jd_broker_finish(jd_broker *b, int32_t client, jd_hyp *out)
{
    if (!b || client < 0 || client >= b->n_clients || !out) return jd_fail(JD_EINVAL, "jd_broker_finish: bad argument");
    std::unique_lock<std::mutex> lk(b->mu);
    BrkClient &c = b->clients[(size_t)client];
    switch (brk_finish_begin(c)) {
    case BRK_NOT_OPEN: return jd_fail(JD_ESTATE, "jd_broker_finish: client %d is not open", client);
    case BRK_CLIENT_ERROR: return client_error(c);
    case BRK_NOT_BETWEEN: return jd_fail(JD_ESTATE, "jd_broker_finish: client %d is not between init and finish", client);
    case BRK_OK: break;
    }
    b->cv_work.notify_all();
    b->cv_done.wait(lk, [&]() { return b->stop || brk_finish_may_go(c); });
    if (brk_finish_end(c) == BRK_CLIENT_ERROR) return client_error(c);
    *out = c.result;
    return JD_OK;
}

extern "C" int jd_broker_partial(jd_broker *b, int32_t client, int32_t cap, int32_t *n, int32_t *labels, int32_t *times)
{
    if (!b || client < 0 || client >= b->n_clients || cap < 0 || !n) return jd_fail(JD_EINVAL, "jd_broker_partial: bad argument");
    std::lock_guard<std::mutex> lk(b->mu);
    const BrkClient &c = b->clients[(size_t)client];
    if (brk_partial(c) == BRK_NOT_OPEN) return jd_fail(JD_ESTATE, "jd_broker_partial: client %d is not open", client);
    *n = (int32_t)c.plabel.size();
    for (int k = 0; k < std::min<int>(cap, *n); ++k) {
        if (labels) labels[k] = c.plabel[(size_t)k];
        if (times) times[k] = c.ptime[(size_t)k];
    }
    return JD_OK;
}

extern "C" int jd_broker_get_stats(jd_broker *b, jd_broker_stats *out)
{
    if (!b || !out) return jd_fail(JD_EINVAL, "jd_broker_get_stats: bad argument");
    std::lock_guard<std::mutex> lk(b->mu);
    *out = b->stats;
    out->resident = b->S.resident ? jd_res_cluster(b->dec) : 0;
    if (b->S.resident) {                                               // (the clusters' own time on their chunks; Path collections)
        out->us_coalesce = jd_res_run_us(b->dec);
        out->us_init = jd_res_collections(b->dec);
    }
    return JD_OK;
}
