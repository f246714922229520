// push_driver.cpp - juicer_amd/csrc/jd_push.h on the CPU (tests/test_push_cpu.py, tests/test_gpu_push_inputs.py; plain g++, no HIP).
// One line in, one line of integers out.
//
// Single decisions:
//   chunk Fc left interval last_collect T                                  -> n
//   after error frame n_collect n_path n_path_new limit fail_T by_flag flag host_n_collect last_collect last_trace interval
//                                                                          -> failed at collected host_collects T due last_collect n_collect
//         (the booking follows where it collected; due 0 where it did not)
//   book at last_trace interval n_collect                                  -> due last_collect n_collect
//   round nS {T last_collect}*nS nw {stream target out}*nw                 -> nact {entry}* {limit}* {weight}* f_end s_lo s_hi {hT}*nS
//   check1 has_dec nS {started}*nS s has_frames n_frames                   -> verdict
//   call has_dec n has_lists                                               -> verdict
//   pack nS {T started}*nS D tile n {stream n_frames has_frames}*n         -> verdict stream rows {open}*nS, and where the call goes on:
//         tile_rows nwork {stream slot weight target row0 entry}* f_end src_at T_at need grown {h_T}*nS n_identity n_minus_one
//   tracelist nS {T started}*nS n {stream}*n                               -> verdict stream {found}*n nss {ss}* {at}*   (found: 7 where untouched)
//   layout M                                                               -> head_at per words
//   request s nhave {label time}*nhave                                     -> stream last_frame have pad
//   reply found len have res_cap n i                                       -> decision stage_at reply_words
//   finish partial nhave {label time}*nhave n {label time}*n               -> open nlist {label time}*
//
// Scripts: the driver holds the records (and, for each stream, a model of the device: its error word, its collection count) and runs
// the twins of jd_stream_push's loop and of jd_streams_push / streams_push_rounds below, the launches answered by the line's replies:
//   reset M interval ref Fc | init s | takeover | finish s n {label time}*n
//   push1 s n_frames R {spec}*R
//   pushN n {s n_frames R {spec}*R}*n
// spec = kind f n_path n_path_new: what the device meets on the way, by frame, in ascending order (a line's specs are that line's).  The
// kernel looks before every frame of a launch but its first, never behind its last: a launch from T to `limit` stops at the first f
// with T < f < limit.  kind 1, the count rule fires behind frame f - 1: the kernel collects and stops with `frame` = f; where f is the
// launch's limit, the counts n_path / n_path_new are what the host reads there.  kind 2: an error at f (<= limit).  kind 3: a
// collection that only the arena asked for (the launch says so, the stream's count does not move; nothing at the limit).
// -> rc nlog {log}* then per stream T started open last_collect last_trace n_collect dirty dev_n_collect nlist
// log: 1 launch n {stream limit frame}*n | 2 gc n {stream}*n | 3 trace n {stream at}*n | 4 booked stream at due   (at: the last frame processed)
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "jd_push.h"

typedef std::vector<long long> Out;
struct Spec { int kind, f, n_path, n_path_new; };

static int M = 0, interval = 0, ref = 0, Fc = 64;
static std::vector<PushStream> S;
static std::vector<char> dirty;
static std::vector<int> dev_err, dev_nc;
static Out logv;

static int rd(std::istringstream &in) { long long v = 0; in >> v; return (int)v; }

// the device: stream s, at frame P.T, is to reach `limit`; *flag: the launch came back behind a collection
static PushCtl device(int s, int limit, std::deque<Spec> &q, bool *flag)
{
    const int T = S[(size_t)s].T;
    PushCtl c{dev_err[(size_t)s], limit, dev_nc[(size_t)s], 0, 1};
    if (dev_err[(size_t)s]) { c.frame = T; return c; }
    while (!q.empty() && q.front().f <= T) q.pop_front();
    if (q.empty() || q.front().f > limit) return c;
    const Spec sp = q.front();
    q.pop_front();
    if (sp.kind == 2) { dev_err[(size_t)s] = c.error = -3; c.frame = sp.f; }
    else if (sp.f < limit) {
        c.frame = sp.f; *flag = true;
        if (sp.kind == 1) c.n_collect = ++dev_nc[(size_t)s];
    } else if (sp.kind == 1) { c.n_path = sp.n_path; c.n_path_new = sp.n_path_new; }
    return c;
}

// jd_stream_push
static int push_one(int s, int n_frames, std::deque<Spec> &q)
{
    const PushCheck chk = push_check_one(&S, s, true, n_frames);
    if (chk.verdict != PUSH_ARG_OK) return (int)chk.verdict;
    PushStream &P = S[(size_t)s];
    if (n_frames > 0) P.open = 1;
    for (int done = 0, n = 0; done < n_frames; done += n) {
        n = push_chunk_frames(Fc, n_frames - done, interval, P.last_collect, P.T);
        const int Tnew = P.T + n;
        if (interval <= 0) { logv.insert(logv.end(), {1, 1, s, Tnew, Tnew}); P.T = Tnew; continue; }
        for (;;) {
            bool flag = false;
            const PushCtl c = device(s, Tnew, q, &flag);
            logv.insert(logv.end(), {1, 1, s, Tnew, c.frame});
            const PushAfter a = push_after(P, c, Tnew, Tnew, !ref, flag);
            if (a.failed) { P.T = a.T; dirty[(size_t)s] = 1; break; }
            if (a.host_collects) { logv.insert(logv.end(), {2, 1, s}); dev_nc[(size_t)s] += 1; }
            P.T = a.T;
            if (a.collected) {
                const bool due = push_book_collection(P, a.at, interval);
                logv.insert(logv.end(), {4, s, a.at, due});
                if (due) { logv.insert(logv.end(), {3, 1, s, a.at}); P.last_trace = P.T - 1; }
            }
            if (a.T >= Tnew) break;
        }
    }
    return 0;
}

// jd_streams_push and streams_push_rounds
static int push_many(const std::vector<int32_t> &streams, const std::vector<int32_t> &n_frames, std::vector<std::deque<Spec>> &q)
{
    const int n = (int)streams.size();
    static const float some = 0.0f;
    std::vector<const float *> frames((size_t)n, &some);
    long long rows = 0;
    const PushCheck chk = push_check_entries(S, n, streams.data(), frames.data(), n_frames.data(), &rows);
    if (chk.verdict != PUSH_ARG_OK) return (int)chk.verdict;
    if (rows == 0) return 0;
    PushPack K;
    push_pack(S, n, streams.data(), n_frames.data(), rows, 39, 128, &K);
    if (interval <= 0) {
        Out l{1, (long long)K.work.size()};
        for (size_t w = 0; w < K.work.size(); ++w) { l.insert(l.end(), {K.work[w].stream, K.target[w], K.target[w]}); S[(size_t)K.work[w].stream].T = K.target[w]; }
        logv.insert(logv.end(), l.begin(), l.end());
        return 0;
    }
    std::vector<int> ws;
    for (const PushWork &w : K.work) ws.push_back(w.stream);
    std::vector<char> out(ws.size(), 0);
    PushRound R;
    for (;;) {
        push_round_plan(S, ws, K.target, out, &R);
        if (R.act.empty()) break;
        std::vector<PushAfter> after;
        Out l{1, (long long)R.act.size()}, gc, tr;
        for (size_t k : R.act) {
            const int s = ws[k];
            PushStream &P = S[(size_t)s];
            bool flag = false;
            const PushCtl c = device(s, R.limit[k], q[K.entry[k]], &flag);
            l.insert(l.end(), {s, R.limit[k], c.frame});
            const PushAfter a = push_after(P, c, R.limit[k], K.target[k], false, false);
            after.push_back(a);
            P.T = a.T;
            if (a.failed) { dirty[(size_t)s] = 1; out[k] = 1; }
            else if (a.host_collects) { gc.push_back(s); dev_nc[(size_t)s] += 1; }
        }
        logv.insert(logv.end(), l.begin(), l.end());
        if (!gc.empty()) { logv.insert(logv.end(), {2, (long long)gc.size()}); logv.insert(logv.end(), gc.begin(), gc.end()); }
        for (size_t a = 0; a < R.act.size(); ++a) {
            const int s = ws[R.act[a]];
            if (!after[a].collected) continue;
            const bool due = push_book_collection(S[(size_t)s], after[a].at, interval);
            logv.insert(logv.end(), {4, s, after[a].at, due});
            if (due) { tr.push_back(s); tr.push_back(after[a].at); }
        }
        if (!tr.empty()) { logv.insert(logv.end(), {3, (long long)tr.size() / 2}); logv.insert(logv.end(), tr.begin(), tr.end()); }
        for (size_t t = 0; t < tr.size(); t += 2) S[(size_t)tr[t]].last_trace = S[(size_t)tr[t]].T - 1;
    }
    return 0;
}

static std::deque<Spec> read_specs(std::istringstream &in)
{
    std::deque<Spec> q;
    const int R = rd(in);
    for (int r = 0; r < R; ++r) { Spec sp; sp.kind = rd(in); sp.f = rd(in); sp.n_path = rd(in); sp.n_path_new = rd(in); q.push_back(sp); }
    return q;
}

static void state(int rc, Out &o)
{
    o.push_back(rc); o.push_back((long long)logv.size());
    o.insert(o.end(), logv.begin(), logv.end());
    for (int s = 0; s < M; ++s) {
        const PushStream &P = S[(size_t)s];
        o.insert(o.end(), {P.T, P.started, P.open, P.last_collect, P.last_trace, P.n_collect, dirty[(size_t)s], dev_nc[(size_t)s], (long long)P.partial_label.size()});
    }
}

static void read_list(std::istringstream &in, PushStream &P)
{
    const int nh = rd(in);
    for (int k = 0; k < nh; ++k) { P.partial_label.push_back(rd(in)); P.partial_time.push_back(rd(in)); }
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        Out o;
        logv.clear();
        if (cmd == "chunk") {
            const int fc = rd(in), left = rd(in), iv = rd(in), lc = rd(in), T = rd(in);
            o.push_back(push_chunk_frames(fc, left, iv, lc, T));
        } else if (cmd == "after") {
            PushCtl c; c.error = rd(in); c.frame = rd(in); c.n_collect = rd(in); c.n_path = rd(in); c.n_path_new = rd(in);
            const int limit = rd(in), fail_T = rd(in), by_flag = rd(in), flag = rd(in);
            PushStream P; P.n_collect = rd(in); P.last_collect = rd(in); P.last_trace = rd(in);
            const int iv = rd(in);
            const PushAfter a = push_after(P, c, limit, fail_T, by_flag != 0, flag != 0);
            const bool due = a.collected && push_book_collection(P, a.at, iv);
            o = {a.failed, a.at, a.collected, a.host_collects, a.T, due, P.last_collect, P.n_collect};
        } else if (cmd == "book") {
            PushStream P;
            const int at = rd(in);
            P.last_trace = rd(in);
            const int iv = rd(in);
            P.n_collect = rd(in);
            const bool due = push_book_collection(P, at, iv);
            o = {due, P.last_collect, P.n_collect};
        } else if (cmd == "round") {
            std::vector<PushStream> St((size_t)rd(in));
            for (PushStream &P : St) { P.T = rd(in); P.last_collect = rd(in); }
            const int nw = rd(in);
            std::vector<int> work((size_t)nw), target((size_t)nw);
            std::vector<char> out((size_t)nw);
            for (int k = 0; k < nw; ++k) { work[(size_t)k] = rd(in); target[(size_t)k] = rd(in); out[(size_t)k] = (char)rd(in); }
            PushRound R;
            push_round_plan(St, work, target, out, &R);
            o.push_back((long long)R.act.size());
            for (size_t k : R.act) o.push_back((long long)k);
            for (size_t k : R.act) o.push_back(R.limit[k]);
            for (double w : R.weight) o.push_back((long long)w);
            o.insert(o.end(), {R.f_end, R.s_lo, R.s_hi});
            o.insert(o.end(), R.hT.begin(), R.hT.end());
        } else if (cmd == "check1") {
            const int has_dec = rd(in);
            std::vector<PushStream> St((size_t)rd(in));
            for (PushStream &P : St) P.started = rd(in);
            const int s = rd(in), has_frames = rd(in), nf = rd(in);
            o.push_back(push_check_one(has_dec ? &St : nullptr, s, has_frames != 0, nf).verdict);
        } else if (cmd == "call") {
            const int has_dec = rd(in), n = rd(in), has_lists = rd(in);
            o.push_back(push_check_call(has_dec != 0, n, has_lists != 0).verdict);
        } else if (cmd == "pack") {
            std::vector<PushStream> St((size_t)rd(in));
            for (PushStream &P : St) { P.T = rd(in); P.started = rd(in); }
            const int D = rd(in), tile = rd(in), n = rd(in);
            static const float some = 0.0f;
            std::vector<int32_t> streams((size_t)n), nf((size_t)n);
            std::vector<const float *> frames((size_t)n);
            for (int i = 0; i < n; ++i) { streams[(size_t)i] = rd(in); nf[(size_t)i] = rd(in); frames[(size_t)i] = rd(in) ? &some : nullptr; }
            long long rows = 0;
            const PushCheck chk = push_check_entries(St, n, streams.data(), frames.data(), nf.data(), &rows);
            o = {chk.verdict, chk.stream, rows};
            for (const PushStream &P : St) o.push_back(P.open);
            if (chk.verdict == PUSH_ARG_OK && rows > 0) {
                PushPack K;
                push_pack(St, n, streams.data(), nf.data(), rows, D, tile, &K);
                o.insert(o.end(), {(long long)K.tile_rows, (long long)K.work.size()});
                for (size_t w = 0; w < K.work.size(); ++w)
                    o.insert(o.end(), {K.work[w].stream, K.work[w].slot, (long long)K.weight[w], K.target[w], (long long)K.row0[w], (long long)K.entry[w]});
                o.insert(o.end(), {K.f_end, (long long)K.src_at, (long long)K.T_at, (long long)K.need, (long long)push_grown(K.need)});
                std::vector<int> h_src(K.tile_rows), h_T(St.size());
                push_pack_fill(St, K, h_src.data(), h_T.data());
                o.insert(o.end(), h_T.begin(), h_T.end());
                long long same = 0, minus = 0;
                for (size_t r = 0; r < h_src.size(); ++r) { same += h_src[r] == (int)r; minus += h_src[r] == -1; }
                o.insert(o.end(), {same, minus});
            }
        } else if (cmd == "tracelist") {
            std::vector<PushStream> St((size_t)rd(in));
            for (PushStream &P : St) { P.T = rd(in); P.started = rd(in); }
            const int n = rd(in);
            std::vector<int32_t> streams((size_t)n), found((size_t)n, 7);
            for (int i = 0; i < n; ++i) streams[(size_t)i] = rd(in);
            std::vector<int> ss, at;
            const PushCheck chk = push_check_trace(St, n, streams.data(), found.data(), &ss, &at);
            o = {chk.verdict, chk.stream};
            o.insert(o.end(), found.begin(), found.end());
            o.push_back((long long)ss.size());
            o.insert(o.end(), ss.begin(), ss.end()); o.insert(o.end(), at.begin(), at.end());
        } else if (cmd == "layout") {
            const PartialManyLayout Y = partial_many_layout(rd(in));
            o = {(long long)Y.head_at, (long long)Y.per, (long long)Y.words};
        } else if (cmd == "request") {
            PushStream P;
            const int s = rd(in);
            read_list(in, P);
            const PartialRequest r = partial_many_request(P, s);
            o = {r.stream, r.last_frame, r.have, r.pad};
        } else if (cmd == "reply") {
            const int found = rd(in), len = rd(in), have = rd(in), res_cap = rd(in), n = rd(in), i = rd(in);
            o = {partial_many_reply(found, len, have, res_cap), (long long)partial_many_stage_at(n, i), (long long)partial_many_layout(n).reply_words(n)};
        } else if (cmd == "finish" && M == 0) {
            PushStream P;
            const int partial = rd(in);
            read_list(in, P);
            P.open = 1;
            const int n = rd(in);
            std::vector<int32_t> L, Tm;
            for (int k = 0; k < n; ++k) { L.push_back(rd(in)); Tm.push_back(rd(in)); }
            P.finish(partial != 0, n, L.data(), Tm.data());
            o = {P.open, (long long)P.partial_label.size()};
            for (size_t k = 0; k < P.partial_label.size(); ++k) { o.push_back(P.partial_label[k]); o.push_back(P.partial_time[k]); }
        } else if (cmd == "reset") {
            M = rd(in); interval = rd(in); ref = rd(in); Fc = rd(in);
            S.assign((size_t)M, PushStream()); dirty.assign((size_t)M, 0); dev_err.assign((size_t)M, 0); dev_nc.assign((size_t)M, 0);
            state(0, o);
        } else if (cmd == "init") {
            const int s = rd(in);
            S[(size_t)s].init(); dirty[(size_t)s] = 0; dev_err[(size_t)s] = 0; dev_nc[(size_t)s] = 0;     // (mark_init; a dirty stream is wiped first)
            state(0, o);
        } else if (cmd == "takeover") {
            for (PushStream &P : S) P.taken_over();
            state(0, o);
        } else if (cmd == "finish") {
            const int s = rd(in), n = rd(in);
            std::vector<int32_t> L, Tm;
            for (int k = 0; k < n; ++k) { L.push_back(rd(in)); Tm.push_back(rd(in)); }
            S[(size_t)s].finish(interval > 0, n, L.data(), Tm.data());
            state(0, o);
        } else if (cmd == "push1") {
            const int s = rd(in), nf = rd(in);
            std::deque<Spec> q = read_specs(in);
            state(push_one(s, nf, q), o);
        } else if (cmd == "pushN") {
            const int n = rd(in);
            std::vector<int32_t> streams, nf;
            std::vector<std::deque<Spec>> q;
            for (int i = 0; i < n; ++i) { streams.push_back(rd(in)); nf.push_back(rd(in)); q.push_back(read_specs(in)); }
            state(push_many(streams, nf, q), o);
        } else {
            fprintf(stderr, "push_driver: unknown line: %s\n", line.c_str());
            return 2;
        }
        for (size_t k = 0; k < o.size(); ++k) printf("%s%lld", k ? " " : "", o[k]);
        printf("\n");
    }
    return 0;
}
