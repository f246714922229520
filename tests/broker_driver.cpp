// broker_driver.cpp - the broker's per-client decisions (juicer_amd/csrc/jd_client.h) on the CPU, for tests/test_broker_cpu.py.
//
// One case per input line, one line of integers per case.  A line is a list of commands, separated by " ; ", on a handful of
// client records that live from one "reset" to the next: a single decision is a line that resets, sets a record and asks; a
// script is a reset line and a line per step.  The output of a line is what its commands answer, in order, then the statistics
// (ticks frames stream_ticks us_idle us_search) and every record (dump() below).  Errors' texts are numbers here: message m
// is "m<m>".
//
//   reset n D max_tick max_pending            n fresh records; D floats per frame; the two frame limits
//   set i <21 fields>                         record i, field by field (set_record() below; pending as a frame count)
//   settings n interval tick coalesce resident fail trial_ok      the four knobs as words, "-": not set   -> the six settings
//   consts                                    -> the four times
//   open | close_begin i | close_may_go i | close_end i | init i | push_begin i | push_may_go i | push_end i n |
//   finish_begin i | finish_may_go i | finish_end i | partial i | take_error i | note_error i rc m | client_failed i rc m
//   has_work | all_ready | select | late rc*n | listed rc*n | fetched i k | settle rc*n | count frames streams
//   active | stop_idle on us | drain_due should_yield us | any_running | fail_all rc m | looks_at i |
//   collect_due idle stopped | stream_fails i idle err | stream_failed i rc m | idle i now | may_init i | inited i req rc m | may_post i draining |
//   posted i rc m buf nf now | may_stage i | stage_buf i | stage_take i | staged i rc m buf nf | may_finish i | to_finisher i | finished i rc m res
//
//   ok                                        -> brk_record_ok of every record (not part of the golden: the rules are the header's own)
//
// late adds the late finishers to the tick's, as the worker does; fetched is the worker's "keep the list if ..." for a list of k
// entries; settle gives client i the message 100 + i and the result 1000 + i; finished is the finisher thread's two steps.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#ifdef BROKER_RECORD
#include BROKER_RECORD          // (the recorder of tests/golden/broker_golden.json: the same names over the lines jd_client.h replaced)
#else
#include "jd_client.h"
#endif

static std::vector<BrkClient> C;
static BrkTick T;
static jd_broker_stats ST;
static int D = 1, MAX_TICK = 4, MAX_PENDING = 16;
static float next_value = 1.0f;                                         // frames are numbered as they are pushed, over all clients

static std::string msg(int m) { return m ? "m" + std::to_string(m) : std::string(); }
static int msg_id(const std::string &s) { return s.size() > 1 ? atoi(s.c_str() + 1) : 0; }
static void fill(std::vector<float> &v, int frames)
{
    v.clear();
    for (int k = 0; k < frames * D; ++k) v.push_back(next_value++);
}
static void set_record(BrkClient &c, std::istream &in)
{
    int open, want_init, want_finish, inited, pending, err, failed, n_staged, sb0, sn0, sb1, sn1, running, run_buf, fresh, finishing, init_req, in_flight, was_idle;
    long long t_post, t_idle;
    in >> open >> want_init >> want_finish >> inited >> pending >> err >> failed >> n_staged >> sb0 >> sn0 >> sb1 >> sn1 >> running >> run_buf >> fresh >> finishing >>
        init_req >> in_flight >> t_post >> t_idle >> was_idle;
    c = BrkClient();
    c.open = open; c.want_init = want_init; c.want_finish = want_finish; c.inited = inited; fill(c.pending, pending);
    c.err = err; c.errmsg = msg(err ? 9 : 0); c.failed = failed;
    c.n_staged = n_staged; c.staged_buf[0] = sb0; c.staged_n[0] = sn0; c.staged_buf[1] = sb1; c.staged_n[1] = sn1;
    c.running = running; c.run_buf = run_buf; c.fresh = fresh; c.finishing = finishing; c.init_req = (unsigned)init_req; c.in_flight = in_flight;
    c.t_post = t_post; c.t_idle = t_idle; c.was_idle = was_idle;
}
static void dump(std::ostream &out)
{
    out << ' ' << ST.ticks << ' ' << ST.frames << ' ' << ST.stream_ticks << ' ' << ST.us_idle << ' ' << ST.us_search;
    for (const BrkClient &c : C) {
        out << ' ' << c.open << ' ' << c.want_init << ' ' << c.want_finish << ' ' << c.inited << ' ' << c.pending.size() / (size_t)D << ' '
            << (c.pending.empty() ? -1 : (int)c.pending[0]) << ' ' << c.err << ' ' << msg_id(c.errmsg) << ' ' << c.failed << ' ' << c.n_staged;
        for (int k = 0; k < 2; ++k) out << ' ' << (k < c.n_staged ? c.staged_buf[k] : 0) << ' ' << (k < c.n_staged ? c.staged_n[k] : 0);
        out << ' ' << c.running << ' ' << c.run_buf << ' ' << c.fresh << ' ' << c.finishing << ' ' << c.init_req << ' ' << c.in_flight << ' ' << c.t_post << ' '
            << c.t_idle << ' ' << c.was_idle << ' ' << c.taken.size() / (size_t)D << ' ' << (c.taken.empty() ? -1 : (int)c.taken[0]) << ' ' << c.plabel.size() << ' '
            << (int)c.result.tot_ac;
    }
}
static const char *knob(const std::string &w) { return w == "-" ? nullptr : w.c_str(); }

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::ostringstream out;
        std::string cmd;
        while (in >> cmd) {
            int i = 0, a = 0, b = 0, m = 0, n = 0;
            long long t = 0;
            if (cmd == ";") continue;
            else if (cmd == "reset") {
                in >> n >> D >> MAX_TICK >> MAX_PENDING;
                C.assign((size_t)n, BrkClient()); T = BrkTick(); ST = jd_broker_stats(); next_value = 1.0f;
            } else if (cmd == "set") { in >> i; set_record(C[(size_t)i], in); }
            else if (cmd == "settings") {
                std::string k1, k2, k3, k4;
                in >> n >> a >> k1 >> k2 >> k3 >> k4 >> b;
                const BrkSettings S = brk_settings(n, a, knob(k1), knob(k2), knob(k3), knob(k4), b != 0);
                out << ' ' << S.max_tick_frames << ' ' << S.max_pending_frames << ' ' << S.coalesce_us << ' ' << S.partial_interval << ' ' << S.resident << ' ' << S.fail_init_of;
            } else if (cmd == "consts") out << ' ' << BRK_IDLE_STOP_US << ' ' << BRK_YIELD_AFTER_US << ' ' << BRK_IDLE_WAIT_US << ' ' << BRK_POLL_SLEEP_US;
            else if (cmd == "open") out << ' ' << brk_open(C);
            else if (cmd == "close_begin") { in >> i; out << ' ' << brk_close_begin(C[(size_t)i]); }
            else if (cmd == "close_may_go") { in >> i; out << ' ' << brk_close_may_go(C[(size_t)i]); }
            else if (cmd == "close_end") { in >> i; brk_close_end(C[(size_t)i]); }
            else if (cmd == "init") { in >> i; out << ' ' << brk_init(C[(size_t)i]); }
            else if (cmd == "push_begin") { in >> i; out << ' ' << brk_push_begin(C[(size_t)i]); }
            else if (cmd == "push_may_go") { in >> i; out << ' ' << brk_push_may_go(C[(size_t)i], D, MAX_PENDING); }
            else if (cmd == "push_end") {
                in >> i >> n;
                std::vector<float> x;
                fill(x, n);
                out << ' ' << brk_push_end(C[(size_t)i], x.data(), n, D);
            } else if (cmd == "finish_begin") { in >> i; out << ' ' << brk_finish_begin(C[(size_t)i]); }
            else if (cmd == "finish_may_go") { in >> i; out << ' ' << brk_finish_may_go(C[(size_t)i]); }
            else if (cmd == "finish_end") { in >> i; out << ' ' << brk_finish_end(C[(size_t)i]); }
            else if (cmd == "partial") { in >> i; out << ' ' << brk_partial(C[(size_t)i]) << ' ' << C[(size_t)i].plabel.size(); }
            else if (cmd == "take_error") { in >> i; out << ' ' << brk_take_error(C[(size_t)i]); }
            else if (cmd == "note_error") { in >> i >> a >> m; brk_note_error(C[(size_t)i], a, msg(m)); }
            else if (cmd == "client_failed") { in >> i >> a >> m; brk_client_failed(C[(size_t)i], a, msg(m)); }
            else if (cmd == "has_work") out << ' ' << brk_tick_has_work(C);
            else if (cmd == "all_ready") out << ' ' << brk_tick_all_ready(C);
            else if (cmd == "select") {
                brk_tick_select(C, D, MAX_TICK, &T);
                out << ' ' << T.inits.size();
                for (int k : T.inits) out << ' ' << k << ' ' << T.init_seen[(size_t)k];
                out << ' ' << T.pushers.size();
                for (int k : T.pushers) out << ' ' << k << ' ' << C[(size_t)k].taken.size() / (size_t)D;
                out << ' ' << T.finishers.size();
                for (int k : T.finishers) out << ' ' << k;
            } else if (cmd == "late" || cmd == "listed" || cmd == "settle") {
                std::vector<int> rc_of(C.size()), who;
                for (int &r : rc_of) in >> r;
                if (cmd == "settle") {
                    std::vector<std::string> msg_of;
                    std::vector<jd_hyp> res(C.size());
                    for (size_t k = 0; k < C.size(); ++k) { msg_of.push_back(msg(100 + (int)k)); res[k] = jd_hyp(); res[k].tot_ac = (float)(1000 + k); }
                    brk_tick_settle(C, T, rc_of, msg_of, res);
                    continue;
                }
                if (cmd == "late") { brk_tick_late(C, T, rc_of, &who); T.finishers.insert(T.finishers.end(), who.begin(), who.end()); }
                else brk_tick_listed(T, rc_of, &who);
                out << ' ' << who.size();
                for (int k : who) out << ' ' << k;
            } else if (cmd == "fetched") {
                in >> i >> n;
                const bool keeps = brk_tick_keeps_list(C[(size_t)i], T, i);
                if (keeps) { C[(size_t)i].plabel.assign((size_t)n, 1); C[(size_t)i].ptime.assign((size_t)n, 1); }
                out << ' ' << keeps;
            } else if (cmd == "count") { in >> a >> b; brk_tick_count(ST, a, b); }
            else if (cmd == "active") out << ' ' << brk_res_active(C);
            else if (cmd == "stop_idle") { in >> a >> t; out << ' ' << brk_res_stop_when_idle(a != 0, t); }
            else if (cmd == "drain_due") { in >> a >> t; out << ' ' << brk_res_drain_due(a != 0, t); }
            else if (cmd == "any_running") out << ' ' << brk_res_any_running(C);
            else if (cmd == "fail_all") { in >> a >> m; brk_fail_all(C, a, msg(m)); }
            else if (cmd == "looks_at") { in >> i; out << ' ' << brk_res_looks_at(C[(size_t)i]); }
            else if (cmd == "collect_due") { in >> a >> b; out << ' ' << brk_res_collection_due(a, b); }
            else if (cmd == "stream_fails") { in >> i >> a >> b; out << ' ' << brk_res_stream_fails(C[(size_t)i], a, b); }
            else if (cmd == "stream_failed") { in >> i >> a >> m; brk_res_stream_failed(C[(size_t)i], a, msg(m)); }
            else if (cmd == "idle") { in >> i >> t; brk_res_idle(C[(size_t)i], t, ST); }
            else if (cmd == "may_init") { in >> i; out << ' ' << brk_res_may_init(C[(size_t)i]); }
            else if (cmd == "inited") { in >> i >> n >> a >> m; brk_res_inited(C[(size_t)i], (unsigned)n, a, msg(m)); }
            else if (cmd == "may_post") {
                in >> i >> a;
                const bool may = brk_res_may_post(C[(size_t)i], a != 0);
                out << ' ' << may << ' ' << (may ? brk_res_post_buf(C[(size_t)i]) : -1) << ' ' << (may ? brk_res_post_frames(C[(size_t)i]) : -1);
            } else if (cmd == "posted") { in >> i >> a >> m >> b >> n >> t; brk_res_posted(C[(size_t)i], a, msg(m), b, n, t, ST); }
            else if (cmd == "may_stage") {
                in >> i;
                const bool may = brk_res_may_stage(C[(size_t)i]);
                out << ' ' << may << ' ' << (may ? brk_res_stage_buf(C[(size_t)i]) : -1);
            } else if (cmd == "stage_buf") { in >> i; out << ' ' << brk_res_stage_buf(C[(size_t)i]); }
#ifndef BROKER_RECORD
            else if (cmd == "ok") { for (const BrkClient &c : C) out << ' ' << brk_record_ok(c); }
#endif
            else if (cmd == "stage_take") { in >> i; out << ' ' << brk_res_stage_take(C[(size_t)i], D, MAX_TICK); }
            else if (cmd == "staged") { in >> i >> a >> m >> b >> n; brk_res_staged(C[(size_t)i], a, msg(m), b, n); }
            else if (cmd == "may_finish") { in >> i; out << ' ' << brk_res_may_finish(C[(size_t)i]); }
            else if (cmd == "to_finisher") { in >> i; brk_res_to_finisher(C[(size_t)i]); }
            else if (cmd == "finished") {
                in >> i >> a >> m >> n;
                jd_hyp res = jd_hyp();
                res.tot_ac = (float)n;
                brk_note_error(C[(size_t)i], a, msg(m));
                brk_finished(C[(size_t)i], res);
            } else { std::cerr << "broker_driver: unknown command " << cmd << "\n"; return 1; }
            if (!in && !in.eof()) { std::cerr << "broker_driver: bad line: " << line << "\n"; return 1; }
        }
        dump(out);
        std::cout << out.str().substr(1) << "\n";
    }
    return 0;
}
