// broker_fake_dec.cpp - a model of the decoder as jd_broker.cpp sees it: struct jd_dec and the 25 functions that file leaves
// undefined, so that the broker - its threads, lock and condition variables included - links into a stand-alone program
// without HIP (tests/broker_harness.cpp, tests/test_broker_cpu.py).
//
// A stream is a frame count, a running float sum of every value pushed to it in order (chunking cannot change it) and two
// likelihood buffers that are free, staged or running; a posted command is through after a set number of polls.  A result is
// a jd_hyp with the count in tot_ac and the sum in tot_score.  The fake can be told to fail and to interrupt (FakeCfg), and it
// holds its caller to what the comments of jd_host_resident.h and jd_host_stream.h ask of one - see check() below: a
// violation ends the program with a message and status 97.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "broker_fake_dec.h"
#include "jd_internal.h"

namespace {
enum { FREE = 0, STAGED, RUNNING };
struct Buf { int state = FREE; std::vector<float> data; int n = 0; long long seq = 0; };
struct Stream {
    bool started = false;               // between init and finish
    bool first_done = false;            // a command has been posted since init (recognitionStart runs with it)
    long long T_posted = 0, T_done = 0;
    float sum = 0.0f;
    bool cmd = false;                   // a command is under way
    int polls_left = 0, run_buf = -1;
    bool stopped = false;               // it stopped short: a Path collection is due
    int err = 0;                        // failed on the device
    Buf buf[2];
    long long stage_seq = 0;
    std::vector<int32_t> plabel, ptime; // PARTIAL_DECODING (the streaming interface)
};
std::mutex g_env_mu;
std::map<std::string, std::string> g_env;
thread_local char g_err[512] = "";
}  // namespace

struct jd_dec {
    FakeCfg cfg;
    std::mutex mu;
    std::vector<Stream> S;
    bool on = false, ever_on = false;
    bool ended = false;                 // the kernel has been reported as ended, and no jd_res_start has come since
    bool end_used = false;
    int rows = 0;
    long long polls_since_start = 0;
    double search_ms = 0.0;
    int in_tick = 0, in_worker = 0, in_finisher = 0;   // calls under way, by who makes them
    std::vector<int> busy;              // ... and by stream
    FakeCounts n{};
};

[[noreturn]] static void violation(const char *call, const char *fmt, ...)
{
    char text[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    fprintf(stderr, "broker_fake_dec: contract violated in %s: %s\n", call, text);
    fflush(stderr);
    _Exit(97);
}
#define check(cond, call, ...) do { if (!(cond)) violation(call, __VA_ARGS__); } while (0)

// Who may be inside the decoder at the same time.  TICK: the calls of the tick worker (the streaming interface) - none overlaps
// anything.  WORKER: the resident worker's calls - none overlaps another of them.  FINISHER: jd_res_finish, the one call that may
// run beside the worker's.  Calls that concern one stream never overlap, whoever makes them.
enum Who { TICK, WORKER, FINISHER };
struct Call {
    jd_dec *d; Who who; std::vector<int> streams;
    Call(jd_dec *d_, Who w, const char *name, std::vector<int> ss) : d(d_), who(w), streams(std::move(ss))
    {
        std::lock_guard<std::mutex> lk(d->mu);
        if (who == TICK) check(d->in_tick + d->in_worker + d->in_finisher == 0, name, "it overlaps another decoder call");
        if (who == WORKER) check(d->in_tick + d->in_worker == 0, name, "it overlaps another call of the worker");
        if (who == FINISHER) check(d->in_tick + d->in_finisher == 0, name, "it overlaps another result fetch");
        for (int s : streams) {
            check(s >= 0 && s < (int)d->S.size(), name, "stream %d out of range", s);
            check(d->busy[(size_t)s] == 0, name, "a call for stream %d is under way", s);
        }
        for (int s : streams) d->busy[(size_t)s] += 1;
        (who == TICK ? d->in_tick : who == WORKER ? d->in_worker : d->in_finisher) += 1;
    }
    ~Call()
    {
        std::lock_guard<std::mutex> lk(d->mu);
        for (int s : streams) d->busy[(size_t)s] -= 1;
        (who == TICK ? d->in_tick : who == WORKER ? d->in_worker : d->in_finisher) -= 1;
    }
};
static void linger() { std::this_thread::sleep_for(std::chrono::microseconds(20)); }   // (room for an overlap to show)

// ---- the harness's side
jd_dec *fake_dec_create(const FakeCfg &cfg)
{
    jd_dec *d = new jd_dec();
    d->cfg = cfg;
    d->S.resize((size_t)cfg.max_streams);
    d->busy.assign((size_t)cfg.max_streams, 0);
    return d;
}
void fake_dec_destroy(jd_dec *d) { delete d; }
FakeCounts fake_dec_counts(jd_dec *d)
{
    std::lock_guard<std::mutex> lk(d->mu);
    return d->n;
}
void fake_env_set(const char *name, const char *value)
{
    std::lock_guard<std::mutex> lk(g_env_mu);
    if (value) g_env[name] = value;
    else g_env.erase(name);
}
void fake_env_clear()
{
    std::lock_guard<std::mutex> lk(g_env_mu);
    g_env.clear();
}

// ---- what jd_broker.cpp links against
int jd_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char *jd_last_error(void) { return g_err; }
const char *jd_dev_env(const char *name)
{
    std::lock_guard<std::mutex> lk(g_env_mu);
    auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}
extern "C" int jd_dec_info(const jd_dec *d, int32_t *max_streams, int32_t *vec_size)
{
    *max_streams = d->cfg.max_streams; *vec_size = d->cfg.D;
    return JD_OK;
}
extern "C" int jd_dec_get_output_level(const jd_dec *, int32_t *level) { *level = 1; return JD_OK; }
extern "C" int jd_dec_get_partial_interval(const jd_dec *d, int32_t *interval) { *interval = d->cfg.partial_interval; return JD_OK; }
extern "C" int jd_dec_last_timing(const jd_dec *d_, jd_timing *out)
{
    jd_dec *d = const_cast<jd_dec *>(d_);
    Call call(d, TICK, "jd_dec_last_timing", {});
    std::lock_guard<std::mutex> lk(d->mu);
    memset(out, 0, sizeof *out);
    out->search_ms = d->search_ms;
    return JD_OK;
}

static int stream_failed(int s, long long frame) { return jd_fail(FAKE_STREAM_ERROR, "fake decoder: stream %d failed on the device at frame %lld", s, frame); }
static jd_hyp result_of(const Stream &st)
{
    jd_hyp h;
    memset(&h, 0, sizeof h);
    h.tot_ac = (float)st.T_done; h.tot_score = st.sum;
    return h;
}

// ---- the streaming interface (the tick worker)
extern "C" int jd_stream_init(jd_dec *d, int32_t s)
{
    Call call(d, TICK, "jd_stream_init", {s});
    std::lock_guard<std::mutex> lk(d->mu);
    Stream &st = d->S[(size_t)s];
    st = Stream();
    st.started = true;
    d->n.inits += 1;
    return JD_OK;
}
extern "C" int jd_streams_push(jd_dec *d, int32_t n, const int32_t *streams, const float *const *frames, const int32_t *n_frames)
{
    std::vector<int> ss(streams, streams + n);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < i; ++k) check(ss[(size_t)i] != ss[(size_t)k], "jd_streams_push", "stream %d twice in one call", ss[(size_t)i]);
    Call call(d, TICK, "jd_streams_push", ss);
    linger();
    std::lock_guard<std::mutex> lk(d->mu);
    d->n.pushes += 1;
    d->search_ms += 0.01;
    for (int i = 0; i < n; ++i) {
        Stream &st = d->S[(size_t)streams[i]];
        check(st.started, "jd_streams_push", "stream %d is not initialised", streams[i]);
        check(n_frames[i] >= 0 && (n_frames[i] == 0 || frames[i]), "jd_streams_push", "stream %d: bad frames", streams[i]);
        if (st.err) continue;                                          // (a failed stream is left out; its finish reports it)
        for (size_t k = 0; k < (size_t)n_frames[i] * (size_t)d->cfg.D; ++k) st.sum += frames[i][k];
        const long long T0 = st.T_done;
        st.T_done += n_frames[i]; st.T_posted = st.T_done;
        if (streams[i] == d->cfg.err_stream && T0 < d->cfg.err_frame && d->cfg.err_frame <= st.T_done) { st.err = 1; st.T_done = d->cfg.err_frame; }
        const int iv = d->cfg.partial_interval;
        while (iv > 0 && (long long)st.plabel.size() < st.T_done / iv) {
            st.plabel.push_back((int32_t)st.plabel.size() + 1);
            st.ptime.push_back((int32_t)st.plabel.size() * iv - 1);
        }
    }
    return JD_OK;
}
extern "C" int jd_stream_finish(jd_dec *d, int32_t s, jd_hyp *out)
{
    Call call(d, TICK, "jd_stream_finish", {s});
    linger();
    std::lock_guard<std::mutex> lk(d->mu);
    Stream &st = d->S[(size_t)s];
    d->n.finishes += 1;
    // (refused, not a violation: behind a failed init the tick worker still asks for the result of a finish that came with it)
    if (!st.started) return jd_fail(JD_ESTATE, "fake decoder: jd_stream_finish: stream %d is not initialised", s);
    st.started = false;
    if (st.err) return stream_failed(s, st.T_done);
    if (d->cfg.partial_interval > 0) { st.plabel.push_back(1000000 + (int32_t)st.T_done); st.ptime.push_back((int32_t)st.T_done - 1); }
    *out = result_of(st);
    return JD_OK;
}
extern "C" int jd_stream_partial(jd_dec *d, int32_t s, int32_t trace_now, int32_t cap, int32_t *n, int32_t *labels, int32_t *times, int32_t *found)
{
    Call call(d, TICK, "jd_stream_partial", {s});
    std::lock_guard<std::mutex> lk(d->mu);
    const Stream &st = d->S[(size_t)s];
    check(trace_now == 0 && cap >= 0 && n, "jd_stream_partial", "bad argument");
    d->n.partials += 1;
    *n = (int32_t)st.plabel.size();
    for (int k = 0; k < cap && k < *n; ++k) {
        if (labels) labels[k] = st.plabel[(size_t)k];
        if (times) times[k] = st.ptime[(size_t)k];
    }
    if (found) *found = 0;
    return JD_OK;
}

// ---- the resident kernel.  Per-stream calls come between jd_res_start and jd_res_stop / jd_res_yield only; once the kernel has
// been reported as ended they are answered with an error instead, up to the next jd_res_start (the broker's worker may have a call
// or two of its round left, and its finisher a fetch under way).
static int gone() { return jd_fail(JD_ESTATE, "fake decoder: the resident search kernel has ended"); }
#define NEEDS_KERNEL(call) do { if (!d->on) { check(d->ended, call, "the resident kernel is not running"); return gone(); } } while (0)

int jd_res_start(jd_dec *d, int n_streams, int rows_per_buf)
{
    Call call(d, WORKER, "jd_res_start", {});
    std::lock_guard<std::mutex> lk(d->mu);
    check(!d->on, "jd_res_start", "the resident kernel is running already");
    check(n_streams >= 1 && n_streams <= d->cfg.max_streams && rows_per_buf >= 1, "jd_res_start", "bad argument");
    if (d->cfg.fail_start) return jd_fail(JD_EHIP, "fake decoder: jd_res_start fails");
    if (d->cfg.partial_interval > 0) return jd_fail(JD_ESTATE, "fake decoder: no resident kernel with partial traces");
    d->on = true; d->ever_on = true; d->ended = false; d->rows = rows_per_buf; d->polls_since_start = 0;
    d->n.starts += 1;
    return JD_OK;
}
static void res_leave(jd_dec *d)                                        // (d->mu held)
{
    d->on = false;
    if (!d->ended) return;
    for (Stream &st : d->S) {                                          // an ended kernel's commands and buffers are nobody's any more
        st.cmd = false; st.stopped = false; st.run_buf = -1;
        st.buf[0].state = st.buf[1].state = FREE;
    }
}
int jd_res_stop(jd_dec *d)
{
    Call call(d, WORKER, "jd_res_stop", {});
    std::lock_guard<std::mutex> lk(d->mu);
    if (!d->on) return JD_OK;
    res_leave(d);
    d->n.stops += 1;
    return JD_OK;
}
int jd_res_yield(jd_dec *d)
{
    Call call(d, WORKER, "jd_res_yield", {});
    std::lock_guard<std::mutex> lk(d->mu);
    if (!d->on) return JD_OK;
    for (const Stream &st : d->S) check(!st.cmd, "jd_res_yield", "a command is running");
    res_leave(d);
    d->n.yields += 1;
    return JD_OK;
}
int jd_res_should_yield(const jd_dec *d_)
{
    jd_dec *d = const_cast<jd_dec *>(d_);
    Call call(d, WORKER, "jd_res_should_yield", {});
    std::lock_guard<std::mutex> lk(d->mu);
    return d->on && d->cfg.yield_after_polls > 0 && d->polls_since_start >= d->cfg.yield_after_polls;
}
// (statistics, read by jd_broker_get_stats from any thread)
int jd_res_cluster(const jd_dec *d_)
{
    jd_dec *d = const_cast<jd_dec *>(d_);
    std::lock_guard<std::mutex> lk(d->mu);
    return d->ever_on ? 4 : 0;
}
long long jd_res_collections(const jd_dec *d_)
{
    jd_dec *d = const_cast<jd_dec *>(d_);
    std::lock_guard<std::mutex> lk(d->mu);
    return d->n.collects;
}
long long jd_res_run_us(const jd_dec *d_)
{
    jd_dec *d = const_cast<jd_dec *>(d_);
    std::lock_guard<std::mutex> lk(d->mu);
    return d->n.polls;
}

int jd_res_init(jd_dec *d, int s)
{
    Call call(d, WORKER, "jd_res_init", {s});
    std::lock_guard<std::mutex> lk(d->mu);
    NEEDS_KERNEL("jd_res_init");
    Stream &st = d->S[(size_t)s];
    check(!st.cmd && !st.stopped, "jd_res_init", "stream %d is not idle", s);
    check(st.buf[0].state == FREE && st.buf[1].state == FREE, "jd_res_init", "stream %d has a chunk staged", s);
    st = Stream();
    st.started = true;
    d->n.res_inits += 1;
    return JD_OK;
}
int jd_res_stage_many(jd_dec *d, int n, const int *streams, const int *bufs, const float *const *frames, const int *n_frames)
{
    std::vector<int> ss(streams, streams + n);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < i; ++k) check(ss[(size_t)i] != ss[(size_t)k], "jd_res_stage_many", "stream %d twice in one call", ss[(size_t)i]);
    Call call(d, WORKER, "jd_res_stage_many", ss);
    linger();
    std::lock_guard<std::mutex> lk(d->mu);
    NEEDS_KERNEL("jd_res_stage_many");
    d->n.stage_calls += 1;
    for (int i = 0; i < n; ++i) {
        const Stream &st = d->S[(size_t)streams[i]];
        check(st.started && !st.err, "jd_res_stage_many", "stream %d is not in an utterance", streams[i]);
        check(bufs[i] == 0 || bufs[i] == 1, "jd_res_stage_many", "stream %d: buffer %d", streams[i], bufs[i]);
        check(st.buf[bufs[i]].state == FREE, "jd_res_stage_many", "stream %d: buffer %d is not free", streams[i], bufs[i]);
        check(n_frames[i] >= 1 && n_frames[i] <= d->rows && frames[i], "jd_res_stage_many", "stream %d: %d frames for a buffer of %d rows", streams[i], n_frames[i], d->rows);
    }
    if (d->n.stage_calls == d->cfg.fail_stage_nth) return jd_fail(JD_EHIP, "fake decoder: staging call %lld fails", d->n.stage_calls);
    for (int i = 0; i < n; ++i) {
        Stream &st = d->S[(size_t)streams[i]];
        Buf &b = st.buf[bufs[i]];
        b.state = STAGED; b.n = n_frames[i]; b.seq = ++st.stage_seq;
        b.data.assign(frames[i], frames[i] + (size_t)n_frames[i] * (size_t)d->cfg.D);
    }
    return JD_OK;
}
int jd_res_post(jd_dec *d, int s, int buf, int n_frames)
{
    Call call(d, WORKER, "jd_res_post", {s});
    std::lock_guard<std::mutex> lk(d->mu);
    NEEDS_KERNEL("jd_res_post");
    Stream &st = d->S[(size_t)s];
    check(st.started, "jd_res_post", "stream %d is not initialised", s);
    check(!st.cmd && !st.stopped, "jd_res_post", "stream %d is not idle", s);
    check(buf == 0 || buf == 1, "jd_res_post", "stream %d: buffer %d", s, buf);
    d->n.posts += 1;
    const bool fails = d->n.posts == d->cfg.fail_post_nth;
    if (n_frames == 0) {                                               // a chunk of none: recognitionStart for a finish without frames
        check(!st.first_done && st.buf[0].state == FREE && st.buf[1].state == FREE, "jd_res_post", "stream %d: a chunk of none behind frames", s);
        if (fails) return jd_fail(JD_EHIP, "fake decoder: post %lld fails", d->n.posts);
        st.run_buf = -1;
    } else {
        Buf &b = st.buf[buf];
        check(b.state == STAGED, "jd_res_post", "stream %d: buffer %d is %s", s, buf, b.state == FREE ? "not staged" : "running");
        check(b.n == n_frames, "jd_res_post", "stream %d: %d frames posted, %d staged", s, n_frames, b.n);
        check(st.buf[buf ^ 1].state != STAGED || st.buf[buf ^ 1].seq > b.seq, "jd_res_post", "stream %d: buffer %d posted before the one staged first", s, buf);
        if (fails) { b.state = FREE; return jd_fail(JD_EHIP, "fake decoder: post %lld fails", d->n.posts); }   // (the chunk is lost)
        for (float x : b.data) st.sum += x;
        st.T_posted += n_frames;
        b.state = RUNNING; st.run_buf = buf;
    }
    st.first_done = true;
    st.cmd = true; st.polls_left = d->cfg.polls_per_command;
    return JD_OK;
}
int jd_res_poll(jd_dec *d, int s, int *idle, int *frame, int *error, int *stopped)
{
    Call call(d, WORKER, "jd_res_poll", {s});
    std::lock_guard<std::mutex> lk(d->mu);
    NEEDS_KERNEL("jd_res_poll");
    Stream &st = d->S[(size_t)s];
    d->n.polls += 1; d->polls_since_start += 1;
    if (d->cfg.end_after_polls > 0 && !d->end_used && d->n.polls >= d->cfg.end_after_polls) { d->end_used = true; d->ended = true; }
    if (d->ended) return gone();
    if (st.cmd && --st.polls_left <= 0) {
        const long long k = d->cfg.stop_every, next = k > 0 ? (st.T_done / k + 1) * k : 0;
        if (s == d->cfg.err_stream && st.T_done < d->cfg.err_frame && d->cfg.err_frame <= st.T_posted) {
            st.T_done = d->cfg.err_frame; st.err = 7; st.cmd = false;
            st.buf[0].state = st.buf[1].state = FREE; st.run_buf = -1;   // (nothing more is scored or run for a failed stream)
        } else if (k > 0 && next < st.T_posted) {
            st.T_done = next; st.stopped = true; st.cmd = false;
        } else {
            st.T_done = st.T_posted; st.cmd = false;
            if (st.run_buf >= 0) st.buf[st.run_buf].state = FREE;
            st.run_buf = -1;
        }
    }
    *idle = st.cmd ? 0 : 1; *frame = (int)st.T_done; *error = st.err; *stopped = st.stopped ? 1 : 0;
    return JD_OK;
}
int jd_res_stream_error(jd_dec *d, int s, int dev_error, int frame)
{
    Call call(d, WORKER, "jd_res_stream_error", {s});
    check(dev_error != 0, "jd_res_stream_error", "stream %d has no error", s);
    return stream_failed(s, frame);
}
int jd_res_collect(jd_dec *d, int s)
{
    Call call(d, WORKER, "jd_res_collect", {s});
    std::lock_guard<std::mutex> lk(d->mu);
    NEEDS_KERNEL("jd_res_collect");
    Stream &st = d->S[(size_t)s];
    check(!st.cmd && st.stopped, "jd_res_collect", "stream %d is not idle and stopped", s);
    st.stopped = false; st.cmd = true; st.polls_left = d->cfg.polls_per_command;   // (the rest of its command again)
    d->n.collects += 1;
    return JD_OK;
}
int jd_res_finish(jd_dec *d, int s, jd_hyp *out)
{
    Call call(d, FINISHER, "jd_res_finish", {s});
    linger();
    std::lock_guard<std::mutex> lk(d->mu);
    NEEDS_KERNEL("jd_res_finish");
    Stream &st = d->S[(size_t)s];
    check(st.started, "jd_res_finish", "stream %d is not initialised", s);
    check(!st.cmd && !st.stopped, "jd_res_finish", "stream %d is not idle", s);
    check(st.buf[0].state == FREE && st.buf[1].state == FREE, "jd_res_finish", "stream %d has a chunk staged", s);
    check(st.first_done && (st.err || st.T_done == st.T_posted), "jd_res_finish", "stream %d has not processed everything", s);
    d->n.res_finishes += 1;
    st.started = false;
    if (st.err) return stream_failed(s, st.T_done);
    *out = result_of(st);
    return JD_OK;
}
