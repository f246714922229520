// broker_harness.cpp - the whole of juicer_amd/csrc/jd_broker.cpp, with its threads, lock and condition variables, against the
// model decoder of tests/broker_fake_dec.cpp: a stand-alone program for the CPU (tests/test_broker_cpu.py builds it with plain g++,
// also under -fsanitize=thread and -fsanitize=address,undefined).  Every scenario runs with the tick worker and with the worker
// over the resident kernel where that makes sense; the client threads hold every result to the count and the sum of what they
// pushed, the fake holds the broker to the decoder's calling rules, and a watchdog turns a deadlock into a failure.
//
//   broker_harness [scenario]      prints "ok <scenario> <worker>" per run; status 0: all passed, 1: a check failed,
//                                  2: a scenario did not end in time, 97: the fake's contract was violated
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "broker_fake_dec.h"

#if defined(__SANITIZE_THREAD__)
#include <pthread.h>
#include <time.h>
// libstdc++ waits against the steady clock with pthread_cond_clockwait.  A ThreadSanitizer runtime that does not know that function
// misses that the wait gives the mutex up, and reports every lock taken meanwhile as a double lock and what is done under it as a
// race.  Under ThreadSanitizer the call is therefore turned into the pthread_cond_timedwait it knows - here, for the whole program.
extern "C" int pthread_cond_clockwait(pthread_cond_t *cv, pthread_mutex_t *mu, clockid_t clock, const struct timespec *abstime)
{
    struct timespec now, real;
    clock_gettime(clock, &now);
    clock_gettime(CLOCK_REALTIME, &real);
    long long ns = (long long)(abstime->tv_sec - now.tv_sec) * 1000000000LL + (abstime->tv_nsec - now.tv_nsec);
    ns = (ns < 0 ? 0 : ns) + (long long)real.tv_sec * 1000000000LL + real.tv_nsec;
    struct timespec until;
    until.tv_sec = (time_t)(ns / 1000000000LL); until.tv_nsec = (long)(ns % 1000000000LL);
    return pthread_cond_timedwait(cv, mu, &until);
}
#endif

namespace {
enum { D = 4, DEADLINE_S = 30 };
std::string g_run;                                                      // "<scenario> <worker>", for the messages

[[noreturn]] void fail(const char *fmt, ...)
{
    char text[600];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    fprintf(stderr, "broker_harness: %s: %s\n", g_run.c_str(), text);
    fflush(stderr);
    _Exit(1);
}
#define expect(cond, ...) do { if (!(cond)) fail(__VA_ARGS__); } while (0)
#define ok(call) do { const int rc_ = (call); if (rc_ != JD_OK) fail("%s -> %d (%s)", #call, rc_, jd_last_error()); } while (0)

// a run that does not end within its deadline prints which one and ends the program
struct Watchdog {
    std::mutex mu; std::condition_variable cv; bool done = false; std::thread t;
    Watchdog()
    {
        t = std::thread([this]() {
            std::unique_lock<std::mutex> lk(mu);
            if (!cv.wait_for(lk, std::chrono::seconds(DEADLINE_S), [this]() { return done; })) {
                fprintf(stderr, "broker_harness: %s: did not end within %d s\n", g_run.c_str(), (int)DEADLINE_S);
                fflush(stderr);
                _Exit(2);
            }
        });
    }
    ~Watchdog()
    {
        { std::lock_guard<std::mutex> lk(mu); done = true; }
        cv.notify_all();
        t.join();
    }
};

// the frames of utterance u of caller c: small multiples of a quarter, so that the running float sum is exact enough to differ
// wherever a frame is lost, doubled or out of order - and it is compared for equality with the same sum made here
float value(int c, int u, int f, int k) { return (float)((c * 131 + u * 17 + f * 7 + k * 3) % 23) * 0.25f - 2.0f; }
std::vector<float> frames_of(int c, int u, int n)
{
    std::vector<float> x((size_t)n * D);
    for (int f = 0; f < n; ++f)
        for (int k = 0; k < D; ++k) x[(size_t)f * D + k] = value(c, u, f, k);
    return x;
}
float sum_of(const std::vector<float> &x, int n)
{
    float s = 0.0f;
    for (size_t i = 0; i < (size_t)n * D; ++i) s += x[i];
    return s;
}
const int CHUNKS[] = {1, 7, 33, 100, 257, 64, 3, 129};

struct Rig {
    jd_dec *dec = nullptr;
    jd_broker *b = nullptr;
    bool resident = false;
    Rig(const FakeCfg &cfg, bool want_resident, const std::vector<std::pair<const char *, const char *>> &env = {}, int n_clients = 0)
    {
        fake_env_clear();
        fake_env_set("JD_BROKER_RESIDENT", want_resident ? "1" : "0");
        for (const auto &e : env) fake_env_set(e.first, e.second);
        dec = fake_dec_create(cfg);
        ok(jd_broker_create(&b, dec, n_clients ? n_clients : cfg.max_streams));
        resident = stats().resident > 0;
    }
    jd_broker_stats stats()
    {
        jd_broker_stats st;
        ok(jd_broker_get_stats(b, &st));
        return st;
    }
    ~Rig() { jd_broker_destroy(b); fake_dec_destroy(dec); }
};

// init, push in chunks (from the cycle above, starting at `phase`), finish: the result against what was pushed.  A call that
// fails returns its code (the text is jd_last_error()'s); pause_us: a sleep between two pushes
int utterance(jd_broker *b, int client, int c, int u, int n, int phase = 0, int pause_us = 0)
{
    const std::vector<float> x = frames_of(c, u, n);
    int rc = jd_broker_init(b, client);
    if (rc) return rc;
    for (int at = 0, k = phase; at < n; ++k) {
        const int m = std::min(CHUNKS[k % 8], n - at);
        rc = jd_broker_push(b, client, x.data() + (size_t)at * D, m);
        if (rc) return rc;
        at += m;
        if (pause_us) std::this_thread::sleep_for(std::chrono::microseconds(pause_us));
    }
    jd_hyp h;
    memset(&h, 0xff, sizeof h);
    rc = jd_broker_finish(b, client, &h);
    if (rc) return rc;
    expect((int)h.tot_ac == n, "caller %d utterance %d: %d frames decoded of %d", c, u, (int)h.tot_ac, n);
    expect(h.tot_score == sum_of(x, n), "caller %d utterance %d: sum %.2f, pushed %.2f", c, u, h.tot_score, sum_of(x, n));
    return JD_OK;
}
void in_threads(int n, const std::function<void(int)> &body)
{
    std::vector<std::thread> t;
    for (int c = 0; c < n; ++c) t.emplace_back(body, c);
    for (auto &th : t) th.join();
}
int open_client(jd_broker *b)
{
    int32_t client = -1;
    ok(jd_broker_open(b, &client));
    return client;
}

// ---- the scenarios
void several_clients(bool resident)
{
    FakeCfg cfg;
    Rig r(cfg, resident);
    expect(r.resident == resident, "stats.resident = %d", (int)r.stats().resident);
    std::atomic<long long> pushed{0};
    in_threads(6, [&](int c) {
        const int client = open_client(r.b);
        for (int u = 0; u < 3; ++u) {
            const int n = 1 + (c * 397 + u * 911) % 1500;
            ok(utterance(r.b, client, c, u, n, c + u));
            pushed += n;
        }
        ok(jd_broker_close(r.b, client));
    });
    const jd_broker_stats st = r.stats();
    expect(st.frames == pushed.load(), "stats.frames = %lld, pushed %lld", (long long)st.frames, pushed.load());
    expect(st.ticks > 0 && st.stream_ticks >= st.ticks, "stats: %lld ticks, %lld stream ticks", (long long)st.ticks, (long long)st.stream_ticks);
}
void without_frames(bool resident)
{
    FakeCfg cfg;
    Rig r(cfg, resident);
    in_threads(3, [&](int c) {
        const int client = open_client(r.b);
        ok(utterance(r.b, client, c, 0, c == 1 ? 40 : 0));
        ok(utterance(r.b, client, c, 1, 0));
        ok(utterance(r.b, client, c, 2, 25));
        ok(jd_broker_close(r.b, client));
    });
}
void init_mid_utterance(bool resident)
{
    FakeCfg cfg;
    cfg.polls_per_command = 20;
    Rig r(cfg, resident);
    in_threads(3, [&](int c) {
        const int client = open_client(r.b);
        const std::vector<float> x = frames_of(c, 9, 700);
        ok(jd_broker_init(r.b, client));
        ok(jd_broker_init(r.b, client));                               // (twice: one init)
        ok(jd_broker_push(r.b, client, x.data(), 300 + 100 * c));
        if (c > 0) std::this_thread::sleep_for(std::chrono::microseconds(300 * c));   // (by now a chunk runs and the rest is staged)
        ok(utterance(r.b, client, c, 1, 123 + c));                     // (init: what is left of the 300 is dropped)
        ok(jd_broker_close(r.b, client));
    });
}
void close_unfinished_and_reopen(bool resident)
{
    FakeCfg cfg;
    cfg.polls_per_command = 50;                                        // (a chunk is still running when close comes)
    Rig r(cfg, resident);
    in_threads(3, [&](int c) {
        for (int u = 0; u < 3; ++u) {
            int client = open_client(r.b);
            const std::vector<float> x = frames_of(c, u, 600);
            ok(jd_broker_init(r.b, client));
            ok(jd_broker_push(r.b, client, x.data(), 600));
            ok(jd_broker_close(r.b, client));
            client = open_client(r.b);
            ok(utterance(r.b, client, c, u, 50 + u));
            ok(jd_broker_close(r.b, client));
        }
    });
}
// JD_BROKER_FAIL_INIT=0: the inits of client 0 fail.  Its caller meets the error in a push (one that waits for room, if the worker is
// slow enough) or in its finish; every call up to the next init() reports it, init() itself is accepted; client 1 is not concerned.
void init_failure(bool resident, bool in_finish)
{
    FakeCfg cfg;
    Rig r(cfg, resident, {{"JD_BROKER_FAIL_INIT", "0"}, {"JD_BROKER_TICK_FRAMES", "16"}});
    const int c0 = open_client(r.b), c1 = open_client(r.b);
    expect(c0 == 0 && c1 == 1, "clients %d %d", c0, c1);
    std::thread other([&]() { for (int u = 0; u < 4; ++u) ok(utterance(r.b, c1, 1, u, 333)); });
    for (int round = 0; round < 3; ++round) {
        const std::vector<float> x = frames_of(0, round, 100);
        ok(jd_broker_init(r.b, c0));
        int rc = JD_OK;
        if (!in_finish)
            for (int k = 0; k < 50 && rc == JD_OK; ++k) rc = jd_broker_push(r.b, c0, x.data(), 100);   // (64 pending at the most: the second waits for room)
        jd_hyp h;
        if (in_finish) rc = jd_broker_finish(r.b, c0, &h);
        expect(rc == JD_EHIP && strstr(jd_last_error(), "injected"), "round %d: %d (%s), not the injected failure", round, rc, jd_last_error());
        rc = jd_broker_push(r.b, c0, x.data(), 1);
        expect(rc == JD_EHIP || (in_finish && rc == JD_ESTATE), "a push behind the failure: %d (%s)", rc, jd_last_error());
        rc = jd_broker_finish(r.b, c0, &h);
        expect(rc == JD_EHIP || (in_finish && rc == JD_ESTATE), "a finish behind the failure: %d (%s)", rc, jd_last_error());
    }
    other.join();
    ok(jd_broker_close(r.b, c0));
    ok(jd_broker_close(r.b, c1));
}
void init_failure_push(bool resident) { init_failure(resident, false); }
void init_failure_finish(bool resident) { init_failure(resident, true); }
// stream 1 fails on the device at frame 150 of every utterance that long: its caller is told (by a push or by the finish), the
// others finish correctly, and its next, shorter utterance is fine
void device_error(bool resident)
{
    FakeCfg cfg;
    cfg.err_stream = 1; cfg.err_frame = 150;
    Rig r(cfg, resident);
    std::vector<int> clients;
    for (int c = 0; c < 4; ++c) clients.push_back(open_client(r.b));
    in_threads(4, [&](int c) {
        for (int u = 0; u < 3; ++u) {
            const int rc = utterance(r.b, clients[(size_t)c], c, u, u == 1 ? 100 : 400, c);
            if (clients[(size_t)c] == 1 && u != 1)
                expect(rc == FAKE_STREAM_ERROR && strstr(jd_last_error(), "stream 1 failed"), "utterance %d of the failing stream: %d (%s)", u, rc, jd_last_error());
            else
                expect(rc == JD_OK, "caller %d utterance %d: %d (%s)", c, u, rc, jd_last_error());
        }
        ok(jd_broker_close(r.b, clients[(size_t)c]));
    });
}
void collections(bool resident)
{
    FakeCfg cfg;
    cfg.stop_every = 50;
    Rig r(cfg, resident);
    in_threads(4, [&](int c) {
        const int client = open_client(r.b);
        for (int u = 0; u < 2; ++u) ok(utterance(r.b, client, c, u, 700 + 37 * c, c));
        ok(jd_broker_close(r.b, client));
    });
    expect(fake_dec_counts(r.dec).collects >= 4 * 2 * 10, "%lld collections", fake_dec_counts(r.dec).collects);
    expect(r.stats().us_init == fake_dec_counts(r.dec).collects, "stats.us_init is not the number of collections");
}
void large_push(bool resident)
{
    FakeCfg cfg;
    Rig r(cfg, resident);
    in_threads(2, [&](int c) {
        const int client = open_client(r.b);
        const int n = 2000;                                            // (max_pending_frames is 768 / 1024)
        const std::vector<float> x = frames_of(c, 0, n);
        ok(jd_broker_init(r.b, client));
        ok(jd_broker_push(r.b, client, x.data(), n - 5));
        ok(jd_broker_push(r.b, client, x.data() + (size_t)(n - 5) * D, 5));   // (waits for room)
        jd_hyp h;
        ok(jd_broker_finish(r.b, client, &h));
        expect((int)h.tot_ac == n && h.tot_score == sum_of(x, n), "caller %d: %d frames, sum %.2f", c, (int)h.tot_ac, h.tot_score);
        ok(jd_broker_close(r.b, client));
    });
}
void start_fails_at_create(bool)
{
    FakeCfg cfg;
    cfg.fail_start = true;
    Rig r(cfg, true);
    expect(r.stats().resident == 0, "stats.resident = %d behind a failed trial start", (int)r.stats().resident);
    in_threads(3, [&](int c) {
        const int client = open_client(r.b);
        ok(utterance(r.b, client, c, 0, 500, c));
        ok(jd_broker_close(r.b, client));
    });
    expect(fake_dec_counts(r.dec).pushes > 0 && fake_dec_counts(r.dec).stage_calls == 0, "the tick worker did not serve them");
}
// a partial interval selects the tick worker; a client's list grows monotonically, is empty from init() on and complete behind finish
void partial_lists(bool)
{
    FakeCfg cfg;
    cfg.partial_interval = 50;
    Rig r(cfg, true);
    expect(r.stats().resident == 0, "stats.resident = %d under a partial interval", (int)r.stats().resident);
    in_threads(3, [&](int c) {
        const int client = open_client(r.b);
        for (int u = 0; u < 3; ++u) {
            const int n = 430 + 50 * c + u;
            const std::vector<float> x = frames_of(c, u, n);
            std::vector<int32_t> lab(64), tim(64);
            int32_t np = -1, before = 0;
            ok(jd_broker_init(r.b, client));
            ok(jd_broker_partial(r.b, client, 64, &np, lab.data(), tim.data()));
            expect(np == 0, "caller %d utterance %d: %d entries behind init()", c, u, np);
            for (int at = 0, k = c; at < n; ++k) {
                const int m = std::min(CHUNKS[k % 8], n - at);
                ok(jd_broker_push(r.b, client, x.data() + (size_t)at * D, m));
                at += m;
                ok(jd_broker_partial(r.b, client, 64, &np, lab.data(), tim.data()));
                expect(np >= before && np <= at / 50, "caller %d utterance %d: %d entries behind %d, %d frames pushed", c, u, np, before, at);
                for (int e = 0; e < np; ++e) expect(lab[(size_t)e] == e + 1 && tim[(size_t)e] == (e + 1) * 50 - 1, "caller %d: entry %d is (%d, %d)", c, e, lab[(size_t)e], tim[(size_t)e]);
                before = np;
            }
            jd_hyp h;
            ok(jd_broker_finish(r.b, client, &h));
            ok(jd_broker_partial(r.b, client, 64, &np, lab.data(), tim.data()));
            expect(np == n / 50 + 1 && lab[(size_t)np - 1] == 1000000 + n && tim[(size_t)np - 1] == n - 1, "caller %d utterance %d: %d entries behind finish", c, u, np);
            for (int e = 0; e + 1 < np; ++e) expect(lab[(size_t)e] == e + 1, "caller %d: entry %d behind finish is %d", c, e, lab[(size_t)e]);
            expect((int)h.tot_ac == n && h.tot_score == sum_of(x, n), "caller %d utterance %d: result", c, u);
        }
        ok(jd_broker_close(r.b, client));
    });
}
void yield_and_come_back(bool resident)
{
    FakeCfg cfg;
    cfg.yield_after_polls = 5;
    cfg.polls_per_command = 30;                                        // (a command outlasts a push or two: chunks are staged while the kernel drains)
    Rig r(cfg, resident);
    in_threads(3, [&](int c) {
        const int client = open_client(r.b);
        for (int u = 0; u < 2; ++u) ok(utterance(r.b, client, c, u, 2000, c + u, 1000));   // (some 50 ms: the kernel has had its 20 ms)
        ok(jd_broker_close(r.b, client));
    });
    const FakeCounts n = fake_dec_counts(r.dec);
    expect(n.yields >= 1 && n.starts >= n.yields + 1, "%lld yields, %lld starts", n.yields, n.starts);
}
// the kernel is reported as ended in the middle: every client open at that moment has the error coming (its next call reports it,
// unless that call is init()), nobody hangs, and everything behind the callers' next init() is correct again
void kernel_ended(bool resident)
{
    FakeCfg cfg;
    cfg.end_after_polls = 60;
    Rig r(cfg, resident);
    std::atomic<int> told{0};
    in_threads(4, [&](int c) {
        const int client = open_client(r.b);
        for (int u = 0; u < 4; ++u) {
            int rc = utterance(r.b, client, c, u, 600, c);
            if (rc != JD_OK) {
                expect(rc == JD_ESTATE && strstr(jd_last_error(), "has ended"), "caller %d utterance %d: %d (%s)", c, u, rc, jd_last_error());
                told += 1;
                rc = utterance(r.b, client, c, u, 600, c);
            }
            expect(rc == JD_OK, "caller %d utterance %d again: %d (%s)", c, u, rc, jd_last_error());
        }
        ok(jd_broker_close(r.b, client));
    });
    expect(told.load() >= 1 && told.load() <= 4, "%d callers were told", told.load());
    expect(fake_dec_counts(r.dec).starts >= 2, "the kernel did not come back");
}
// the third staging call and the fifth post fail: the callers concerned are told by their next call - once, the utterance is
// not failed - and begin it again; the chunk of a failed post is lost to the decoder and to the broker alike
void stage_and_post_failures(bool resident)
{
    FakeCfg cfg;
    cfg.fail_stage_nth = 3; cfg.fail_post_nth = 5;
    cfg.polls_per_command = 10;
    Rig r(cfg, resident);
    std::atomic<int> told{0};
    in_threads(3, [&](int c) {
        const int client = open_client(r.b);
        for (int u = 0; u < 3; ++u) {
            int rc = utterance(r.b, client, c, u, 900, c);
            for (int again = 0; rc != JD_OK && again < 2; ++again) {
                expect(rc == JD_EHIP && strstr(jd_last_error(), "fails"), "caller %d utterance %d: %d (%s)", c, u, rc, jd_last_error());
                told += 1;
                rc = utterance(r.b, client, c, u, 900, c);
            }
            expect(rc == JD_OK, "caller %d utterance %d again: %d (%s)", c, u, rc, jd_last_error());
        }
        ok(jd_broker_close(r.b, client));
    });
    // (both failures may meet the same caller before it has made its next call: it is told the first)
    expect(told.load() >= 1 && told.load() <= 4, "%d callers were told", told.load());
    expect(fake_dec_counts(r.dec).stage_calls >= 3 && fake_dec_counts(r.dec).posts >= 5, "the failures were not reached");
}
void destroy_with_idle_clients(bool resident)
{
    FakeCfg cfg;
    Rig r(cfg, resident);
    const int a = open_client(r.b), b = open_client(r.b), c = open_client(r.b);
    ok(utterance(r.b, a, 0, 0, 77));
    ok(jd_broker_init(r.b, b));
    std::this_thread::sleep_for(std::chrono::milliseconds(5));         // (the resident kernel has left by now: 3 ms without work)
    (void)c;
}

struct Scenario { const char *name; void (*run)(bool); bool ticks, resident; };
const Scenario SCENARIOS[] = {
    {"several_clients", several_clients, true, true},
    {"without_frames", without_frames, true, true},
    {"init_mid_utterance", init_mid_utterance, true, true},
    {"close_unfinished_and_reopen", close_unfinished_and_reopen, true, true},
    {"init_failure_push", init_failure_push, true, true},
    {"init_failure_finish", init_failure_finish, true, true},
    {"device_error", device_error, true, true},
    {"collections", collections, false, true},
    {"large_push", large_push, true, true},
    {"start_fails_at_create", start_fails_at_create, true, false},
    {"partial_lists", partial_lists, true, false},
    {"yield_and_come_back", yield_and_come_back, false, true},
    {"kernel_ended", kernel_ended, false, true},
    {"stage_and_post_failures", stage_and_post_failures, false, true},
    {"destroy_with_idle_clients", destroy_with_idle_clients, true, true},
};
}  // namespace

int main(int argc, char **argv)
{
    int runs = 0;
    for (const Scenario &s : SCENARIOS) {
        if (argc > 1 && strcmp(argv[1], s.name) != 0) continue;
        for (int resident = 0; resident < 2; ++resident) {
            if (!(resident ? s.resident : s.ticks)) continue;
            g_run = std::string(s.name) + (resident ? " resident" : " ticks");
            const auto t0 = std::chrono::steady_clock::now();
            {
                Watchdog dog;
                s.run(resident != 0);
            }
            printf("ok %s %d ms\n", g_run.c_str(), (int)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count());
            fflush(stdout);
            runs += 1;
        }
    }
    if (runs == 0) { fprintf(stderr, "broker_harness: no scenario named %s\n", argc > 1 ? argv[1] : "?"); return 1; }
    printf("all %d runs passed\n", runs);
    return 0;
}
