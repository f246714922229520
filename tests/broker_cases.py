"""What tests/test_broker_cpu.py needs: tests/broker_driver.cpp built with plain g++, the lines it is given (single decisions and scripts, as the
driver's head describes them), how its output lines are read, and the stand-alone program that runs the whole broker against the fake decoder."""
import hashlib
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "juicer_amd", "csrc")
OK, NOT_OPEN, NOT_BETWEEN, CLIENT_ERROR = range(4)
D, MAX_TICK, MAX_PENDING = 2, 4, 16                                      # of every reset line: floats per frame, the two frame limits
STATS = ["ticks", "frames", "stream_ticks", "us_idle", "us_search"]
FIELDS = ["open", "want_init", "want_finish", "inited", "pending", "pending_first", "err", "msg", "failed", "n_staged", "sb0", "sn0", "sb1", "sn1", "running", "run_buf",
          "fresh", "finishing", "init_req", "in_flight", "t_post", "t_idle", "was_idle", "taken", "taken_first", "nlist", "result"]
SET = ["open", "want_init", "want_finish", "inited", "pending", "err", "failed", "n_staged", "sb0", "sn0", "sb1", "sn1", "running", "run_buf", "fresh", "finishing",
       "init_req", "in_flight", "t_post", "t_idle", "was_idle"]


def build_driver(path, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", path,
                           os.path.join(HERE, "broker_driver.cpp")])
    return path


def build_harness(path, extra=(), broker=None):
    """the repository's jd_broker.cpp (or another one), the fake decoder and the harness: no hipcc, no library"""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-pthread", "-Wall", "-g", "-O1", *extra, "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-I", HERE, "-o", path,
                           broker or os.path.join(CSRC, "jd_broker.cpp"), os.path.join(HERE, "broker_fake_dec.cpp"), os.path.join(HERE, "broker_harness.cpp")])
    return path


def run_driver(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    return [[int(x) for x in l.split()] for l in out]


def read_line(o, n):
    """a line's output -> (answers, {stats}, [{record}] * n)"""
    at = len(o) - n * len(FIELDS)
    recs = [dict(zip(FIELDS, o[at + k * len(FIELDS):at + (k + 1) * len(FIELDS)])) for k in range(n)]
    return o[:at - len(STATS)], dict(zip(STATS, o[at - len(STATS):at])), recs


def rec(**kw):
    """the 21 fields of a `set`: an open client by default"""
    f = dict.fromkeys(SET, 0)
    f["open"] = 1
    assert set(kw) <= set(SET), kw
    f.update(kw)
    return " ".join(str(int(f[k])) for k in SET)


def reset(n):
    return "reset %d %d %d %d" % (n, D, MAX_TICK, MAX_PENDING)


def one(cmd, *recs):
    """a single decision: fresh records, set as given, and the command(s)"""
    return " ; ".join([reset(max(len(recs), 1))] + ["set %d %s" % (i, r) for i, r in enumerate(recs)] + [cmd])


def flips(base, keys):
    """[(name, record)]: the base record, and the base with each of the keys flipped"""
    out = [("base", rec(**base))]
    for k in keys:
        b = dict(base)
        b[k] = 0 if base.get(k, 1 if k == "open" else 0) else 1
        out.append((k, rec(**b)))
    return out


# ---- single decisions: (name, line)
def single_cases():
    c = []
    # settings n interval tick coalesce resident fail trial_ok
    def settings(name, n=8, interval=0, tick="-", coalesce="-", resident="-", fail="-", trial=1):
        c.append(("settings_" + name, one("settings %d %d %s %s %s %s %d" % (n, interval, tick, coalesce, resident, fail, trial))))
    settings("default"); settings("64_clients", n=64); settings("65_clients", n=65); settings("65_clients_resident_1", n=65, resident="1")
    settings("resident_0", resident="0"); settings("resident_2", resident="2"); settings("resident_word", resident="yes")
    settings("trial_failed", trial=0); settings("trial_failed_ticks_anyway", resident="0", trial=0); settings("interval_50", interval=50)
    settings("interval_50_trial_failed", interval=50, trial=0)
    for v in ("0", "1", "65536", "65537", "-5", "word"):
        settings("tick_" + v.replace("-", "minus_"), tick=v)
        settings("tick_%s_ticks" % v.replace("-", "minus_"), tick=v, resident="0")
    for v in ("-1", "0", "1000000", "1000001"):
        settings("coalesce_" + v.replace("-", "minus_"), coalesce=v)
    settings("fail_init_3", fail="3"); settings("fail_init_0", fail="0"); settings("fail_init_minus_1", fail="-1")
    c.append(("consts", one("consts")))
    # the API calls
    c += [("open_first_free", one("open", rec(), rec(open=0, err=-3, failed=1, init_req=5), rec(open=0))), ("open_all_taken", one("open", rec(), rec())),
          ("open_is_a_new_record", one("open", rec(open=0, inited=1, pending=3, err=-3, failed=1, n_staged=1, fresh=1, init_req=7, was_idle=1, t_idle=5)))]
    c += [("close_begin_" + n, one("close_begin 0", r)) for n, r in flips(dict(pending=3, want_finish=1, inited=1), ["open"])]
    c += [("close_may_go_" + n, one("close_may_go 0", r)) for n, r in flips(dict(inited=1), ["want_init", "running", "n_staged", "in_flight", "finishing", "want_finish", "pending"])]
    c += [("close_end", one("close_end 0", rec(inited=1, pending=2, want_finish=1, fresh=1)))]
    c += [("init_" + n, one("init 0", r)) for n, r in flips(dict(inited=1, pending=3, want_finish=1, err=-3, failed=1, init_req=4), ["open", "want_init", "failed", "inited"])]
    c += [("push_begin_" + n, one("push_begin 0", r)) for n, r in flips(dict(inited=1), ["open", "inited", "want_init", "want_finish", "err", "failed"])]
    c += [("push_begin_behind_an_unserved_init", one("push_begin 0", rec(want_init=1))), ("push_begin_failed_init", one("push_begin 0", rec(err=-3, failed=1))),
          ("push_begin_error_before_state", one("push_begin 0", rec(err=-3)))]
    for p in (0, 1, MAX_PENDING - 1, MAX_PENDING, MAX_PENDING + 1):
        c.append(("push_may_go_pending_%d" % p, one("push_may_go 0", rec(inited=1, pending=p))))
    c += [("push_may_go_failed_and_full", one("push_may_go 0", rec(inited=1, pending=MAX_PENDING + 1, failed=1, err=-3))),
          ("push_end_ok", one("push_end 0 3", rec(inited=1, pending=2))), ("push_end_no_frames", one("push_end 0 0", rec(inited=1, pending=2))),
          ("push_end_error", one("push_end 0 3", rec(inited=1, err=-3))), ("push_end_failed", one("push_end 0 3", rec(inited=1, err=-3, failed=1)))]
    c += [("finish_begin_" + n, one("finish_begin 0", r)) for n, r in flips(dict(inited=1), ["open", "inited", "want_init", "failed", "err", "want_finish"])]
    c += [("finish_begin_failed_init", one("finish_begin 0", rec(failed=1, err=-3))), ("finish_begin_failed_stream", one("finish_begin 0", rec(failed=1, err=-3, inited=1))),
          ("finish_begin_failed_init_next_asked", one("finish_begin 0", rec(failed=1, err=-3, want_init=1))),
          ("finish_may_go_waiting", one("finish_may_go 0", rec(inited=1, want_finish=1))), ("finish_may_go_served", one("finish_may_go 0", rec())),
          ("finish_end_ok", one("finish_end 0", rec())), ("finish_end_error", one("finish_end 0", rec(err=-4))),
          ("partial_open", one("partial 0", rec())), ("partial_not_open", one("partial 0", rec(open=0)))]
    c += [("take_error_none", one("take_error 0", rec())), ("take_error_once", one("take_error 0 ; take_error 0", rec(err=-3))),
          ("take_error_failed_stays", one("take_error 0 ; take_error 0", rec(err=-3, failed=1))),
          ("note_error_none", one("note_error 0 0 5", rec())), ("note_error_first", one("note_error 0 -3 5", rec())), ("note_error_second", one("note_error 0 -4 5", rec(err=-3))),
          ("client_failed", one("client_failed 0 -3 5", rec(inited=1, pending=3, n_staged=2, sb0=0, sn0=4, sb1=1, sn1=2, want_finish=1))),
          ("client_failed_keeps_first_error", one("client_failed 0 -3 5", rec(inited=1, err=-4)))]
    # the tick worker
    c += [("has_work_" + n, one("has_work", r)) for n, r in flips(dict(), ["want_init", "want_finish", "inited", "pending"])]
    c += [("has_work_inited_with_frames", one("has_work", rec(inited=1, pending=1))), ("has_work_closed_with_requests", one("has_work", rec(open=0, want_init=1, want_finish=1))),
          ("has_work_second_client", one("has_work", rec(), rec(want_finish=1)))]
    c += [("all_ready_" + n, one("all_ready", r)) for n, r in flips(dict(inited=1), ["open", "want_finish", "pending"])]
    c += [("all_ready_one_of_two_is_not", one("all_ready", rec(inited=1, pending=2), rec(inited=1))), ("all_ready_nobody_open", one("all_ready", rec(open=0), rec(open=0)))]
    for p in (0, 1, MAX_TICK - 1, MAX_TICK, MAX_TICK + 1):
        c.append(("select_pending_%d" % p, one("select", rec(inited=1, pending=p))))
        c.append(("stage_take_pending_%d" % p, one("stage_take 0", rec(inited=1, pending=p))))
    c += [("select_frames_behind_an_unserved_init", one("select", rec(want_init=1, pending=3, init_req=2))), ("select_frames_of_nobody", one("select", rec(pending=3))),
          ("select_init_alone", one("select", rec(want_init=1, init_req=9))), ("select_closed", one("select", rec(open=0, want_init=1, want_finish=1, inited=1, pending=2))),
          ("select_finisher", one("select", rec(inited=1, want_finish=1))), ("select_finisher_not_inited", one("select", rec(want_finish=1))),
          ("select_finisher_with_its_init", one("select", rec(want_init=1, want_finish=1, init_req=1))),
          ("select_finisher_with_frames_left", one("select", rec(inited=1, want_finish=1, pending=MAX_TICK + 1))),
          ("select_finisher_with_its_last_frames", one("select", rec(inited=1, want_finish=1, pending=MAX_TICK))),
          ("select_three", one("select", rec(want_init=1, init_req=1), rec(inited=1, pending=9), rec(inited=1, want_finish=1)))]
    late = dict(inited=1, want_finish=1)
    c += [("late_" + n, one("select ; set 0 %s ; late 0" % r, rec(inited=1, pending=2))) for n, r in flips(late, ["open", "want_finish", "pending", "want_init", "inited"])]
    c += [("late_tick_failed_for_it", one("select ; set 0 %s ; late -3" % rec(**late), rec(inited=1, pending=2))), ("late_is_a_finisher_already", one("select ; late 0", rec(**late))),
          ("late_second_of_two", one("select ; set 1 %s ; late 0 0" % rec(**late), rec(inited=1, want_finish=1), rec(inited=1, pending=2)))]
    c += [("listed_pushers_then_finishers", one("select ; listed 0 0 0", rec(inited=1, want_finish=1), rec(inited=1, pending=2), rec(inited=1, pending=2, want_finish=1))),
          ("listed_failed_pusher", one("select ; listed 0 -3 0", rec(inited=1, want_finish=1), rec(inited=1, pending=2), rec(inited=1, pending=2, want_finish=1))),
          ("listed_failed_pusher_that_finishes", one("select ; listed 0 0 -3", rec(inited=1, want_finish=1), rec(inited=1, pending=2), rec(inited=1, pending=2, want_finish=1))),
          ("listed_with_a_late_finisher", one("select ; set 1 %s ; late 0 0 ; listed 0 0" % rec(**late), rec(inited=1, pending=2), rec(inited=1, pending=2)))]
    c += [("fetched_kept", one("select ; fetched 0 3", rec(inited=1, pending=2))), ("fetched_kept_with_its_init", one("select ; fetched 0 3", rec(want_init=1, pending=2, init_req=4))),
          ("fetched_init_again_meanwhile", one("select ; init 0 ; fetched 0 3", rec(want_init=1, pending=2, init_req=4))),
          ("fetched_init_meanwhile", one("select ; init 0 ; fetched 0 3", rec(inited=1, pending=2, init_req=4)))]
    c += [("settle_init_ok", one("select ; settle 0", rec(want_init=1, init_req=1))), ("settle_init_failed", one("select ; settle -3", rec(want_init=1, init_req=1, pending=9, want_finish=1))),
          ("settle_init_again_meanwhile", one("select ; init 0 ; settle 0", rec(want_init=1, init_req=1))),
          ("settle_init_failed_and_again_meanwhile", one("select ; init 0 ; settle -3", rec(want_init=1, init_req=1))),
          ("settle_push_failed", one("select ; settle -4", rec(inited=1, pending=2))), ("settle_push_failed_keeps_first_error", one("select ; settle -4", rec(inited=1, pending=2, err=-3))),
          ("settle_finisher", one("select ; settle 0", rec(inited=1, want_finish=1))), ("settle_finisher_failed", one("select ; settle -4", rec(inited=1, want_finish=1))),
          ("settle_bystander", one("select ; settle 0 -3", rec(inited=1, pending=2), rec(inited=1))),
          ("count_a_tick", one("count 7 2 ; count 5 1", rec())), ("count_no_streams", one("count 7 0", rec()))]
    # the resident worker
    c += [("active_" + n, one("active", r)) for n, r in flips(dict(), ["want_init", "want_finish", "running", "finishing", "n_staged", "inited", "pending"])]
    c += [("active_inited_with_frames", one("active", rec(inited=1, pending=1))), ("active_closed", one("active", rec(open=0, want_init=1, running=1, n_staged=1, finishing=1))),
          ("active_second_client", one("active", rec(), rec(running=1)))]
    c += [("stop_idle_%d_%d" % (on, us), one("stop_idle %d %d" % (on, us))) for on in (0, 1) for us in (0, 3000, 3001)]
    c += [("drain_due_%d_%d" % (sy, us), one("drain_due %d %d" % (sy, us))) for sy in (0, 1) for us in (0, 20000, 20001)]
    c += [("any_running_none", one("any_running", rec(inited=1, n_staged=1), rec())), ("any_running_running", one("any_running", rec(), rec(running=1))),
          ("any_running_finishing", one("any_running", rec(finishing=1, inited=1))), ("any_running_closed_client", one("any_running", rec(open=0, running=1))),
          ("fail_all", one("fail_all -6 9", rec(want_init=1, pending=3), rec(inited=1, err=-3, running=1, n_staged=1, want_finish=1), rec(open=0), rec(inited=1, finishing=1, want_finish=1)))]
    c += [("looks_at_" + n, one("looks_at 0", r)) for n, r in flips(dict(inited=1), ["open", "finishing"])]
    c += [("collect_due_%d_%d" % (i, s), one("collect_due %d %d" % (i, s))) for i in (0, 1) for s in (0, 1)]
    c += [("stream_fails_idle_%d_err_%d_failed_%d" % (i, e, f), one("stream_fails 0 %d %d" % (i, e), rec(inited=1, running=1, failed=f, err=-3 * f))) for i in (0, 1) for e in (0, 7) for f in (0, 1)]
    c += [("stream_failed", one("stream_failed 0 -4 8", rec(inited=1, running=1, pending=3, n_staged=1, sb0=1, sn0=4))),
          ("stream_failed_finish_under_way", one("stream_failed 0 -4 8", rec(inited=1, running=1, want_finish=1))),
          ("stream_failed_keeps_first_error", one("stream_failed 0 -4 8", rec(inited=1, running=1, err=-3))),
          ("idle", one("idle 0 350", rec(inited=1, running=1, run_buf=1, t_post=100))), ("idle_again", one("idle 0 900", rec(inited=1, running=1, t_post=500, t_idle=350, was_idle=1)))]
    c += [("may_init_" + n, one("may_init 0", r)) for n, r in flips(dict(want_init=1), ["want_init", "running", "n_staged", "inited", "pending"])]
    c += [("inited_ok", one("inited 0 3 0 0", rec(want_init=1, init_req=3, was_idle=1))), ("inited_ok_again_meanwhile", one("inited 0 3 0 0", rec(want_init=1, init_req=4))),
          ("inited_failed", one("inited 0 3 -3 7", rec(want_init=1, init_req=3, pending=9, want_finish=1, inited=1, fresh=1))),
          ("inited_failed_again_meanwhile", one("inited 0 3 -3 7", rec(want_init=1, init_req=4, pending=9))),
          ("inited_failed_keeps_first_error", one("inited 0 3 -3 7", rec(want_init=1, init_req=3, err=-4)))]
    post = dict(inited=1, n_staged=1, sb0=1, sn0=3)
    c += [("may_post_" + n, one("may_post 0 0", r)) for n, r in flips(post, ["running", "inited", "n_staged", "open", "failed", "want_init"])]
    c += [("may_post_draining", one("may_post 0 1", rec(**post))), ("may_post_two_staged", one("may_post 0 0", rec(inited=1, n_staged=2, sb0=1, sn0=3, sb1=0, sn1=4)))]
    none = dict(inited=1, fresh=1, want_finish=1)
    c += [("may_post_chunk_of_none_" + n, one("may_post 0 0", r)) for n, r in flips(none, ["fresh", "want_finish", "pending", "inited", "running"])]
    c += [("may_post_chunk_of_none_draining", one("may_post 0 1", rec(**none)))]
    for rc in (0, -3):
        for ns in (0, 1, 2):
            c.append(("posted_rc_%d_staged_%d" % (-rc, ns), one("posted 0 %d 6 %d %d 700" % (rc, 1 if ns else 0, 3 if ns else 0),
                                                                rec(inited=1, fresh=1, n_staged=ns, sb0=1, sn0=3, sb1=0, sn1=4, t_idle=450, was_idle=1))))
    c += [("posted_first_of_an_utterance", one("posted 0 0 0 1 3 700", rec(inited=1, fresh=1, n_staged=1, sb0=1, sn0=3, t_idle=450))),
          ("posted_failed_keeps_first_error", one("posted 0 -3 6 1 3 700", rec(inited=1, n_staged=1, sb0=1, sn0=3, err=-4)))]
    stage = dict(inited=1, pending=2)
    c += [("may_stage_" + n, one("may_stage 0", r)) for n, r in flips(stage, ["inited", "failed", "want_init", "pending", "running", "n_staged", "want_finish", "open"])]
    c += [("may_stage_running_%d_staged_%d" % (r, ns), one("may_stage 0", rec(inited=1, pending=2, running=r, run_buf=0, n_staged=ns, sb0=1, sb1=0))) for r in (0, 1) for ns in (0, 1, 2)]
    # the buffer choice: (running, run_buf) x (n_staged of 0 or 1, staged_buf[0]) - and of 2, which brk_res_may_stage never lets through
    c += [("stage_buf_running_%d_in_%d_staged_%d_in_%d" % (r, rb, ns, sb), one("stage_buf 0", rec(inited=1, pending=2, running=r, run_buf=rb, n_staged=ns, sb0=sb, sn0=3 * ns)))
          for r in (0, 1) for rb in (0, 1) for ns in (0, 1) for sb in (0, 1)]
    c += [("stage_buf_refused", one("may_stage 0 ; stage_buf 0", rec(inited=1, pending=2, running=1, run_buf=0, n_staged=1, sb0=1, sn0=3))),
          ("stage_buf_two_staged", one("stage_buf 0", rec(inited=1, pending=2, n_staged=2, sb0=0, sn0=3, sb1=1, sn1=3)))]
    c += [("staged_rc_%d_staged_%d" % (-rc, ns), one("staged 0 %d 6 %d 4" % (rc, 0 if ns else 1), rec(inited=1, in_flight=1, n_staged=ns, sb0=1, sn0=3))) for rc in (0, -3) for ns in (0, 1)]
    c += [("staged_failed_keeps_first_error", one("staged 0 -3 6 0 4", rec(inited=1, in_flight=1, err=-4)))]
    fin = dict(inited=1, want_finish=1)
    c += [("may_finish_" + n, one("may_finish 0", r)) for n, r in flips(fin, ["running", "n_staged", "inited", "fresh", "want_finish", "pending", "failed", "want_init"])]
    c += [("to_finisher", one("to_finisher 0", rec(**fin))), ("finished", one("finished 0 0 0 1234", rec(inited=1, want_finish=1, finishing=1))),
          ("finished_failed", one("finished 0 -4 8 0", rec(inited=1, want_finish=1, finishing=1))),
          ("finished_failed_keeps_first_error", one("finished 0 -4 8 0", rec(inited=1, want_finish=1, finishing=1, err=-3, failed=1)))]
    return c


# ---- scripts: (name, [line]) - API calls and worker steps on one client or three, in the order the broker makes them
def script_cases():
    r = reset(3)
    tick_up = ["open", "init 0", "has_work", "select", "late 0 0 0", "settle 0 0 0"]                  # client 0 open and initialised by a tick
    res_up = ["open", "init 0", "active", "may_init 0", "inited 0 1 0 0"]                             # ... by the resident worker
    chunk = ["push_begin 0", "push_may_go 0", "push_end 0 6", "may_post 0 0", "may_stage 0", "stage_buf 0", "stage_take 0", "staged 0 0 0 0 4",
             "may_post 0 0", "posted 0 0 0 0 4 100", "may_stage 0", "stage_buf 0", "stage_take 0", "staged 0 0 0 1 2"]   # one chunk runs (buffer 0), one is staged (buffer 1)
    s = [
        ("tick_init_twice", [r, "open", "init 0", "init 0", "all_ready", "select", "late 0 0 0", "settle 0 0 0", "has_work"]),
        ("tick_init_during_a_tick", [r, "open", "init 0", "push_begin 0 ; push_end 0 3", "select", "init 0", "late 0 0 0", "listed 0 0 0", "fetched 0 2", "settle 0 0 0", "has_work",
                                     "select", "late 0 0 0", "settle 0 0 0", "has_work"]),
        ("tick_init_during_a_tick_frames_behind_it", [r, "open", "init 0", "push_end 0 3", "select", "init 0", "push_begin 0", "push_may_go 0", "push_end 0 5", "late 0 0 0",
                                                      "listed 0 0 0", "fetched 0 2", "settle 0 0 0", "select", "late 0 0 0", "listed 0 0 0", "fetched 0 1", "settle 0 0 0",
                                                      "select", "settle 0 0 0", "has_work"]),
        ("tick_late_finisher", [r] + tick_up + ["push_end 0 2", "select", "finish_begin 0", "finish_may_go 0", "late 0 0 0", "listed 0 0 0", "fetched 0 4", "settle 0 0 0",
                                                "finish_may_go 0", "finish_end 0", "partial 0", "has_work"]),
        ("tick_late_finisher_of_a_failed_push", [r] + tick_up + ["push_end 0 2", "select", "finish_begin 0", "late -4 0 0", "listed -4 0 0", "settle -4 0 0", "finish_may_go 0", "has_work",
                                                                 "select", "late 0 0 0", "settle 0 0 0", "finish_may_go 0", "finish_end 0 ; take_error 0"]),
        ("tick_finish_without_frames", [r, "open", "init 0", "finish_begin 0", "all_ready", "select", "late 0 0 0", "settle 0 0 0", "finish_may_go 0", "finish_end 0",
                                        "push_begin 0", "finish_begin 0"]),
        ("tick_failed_init_push_waiting", [r, "open", "init 0", "push_begin 0 ; push_may_go 0 ; push_end 0 21", "push_begin 0", "push_may_go 0", "select", "push_may_go 0", "late -3 0 0",
                                           "settle -3 0 0", "push_may_go 0", "push_end 0 2 ; take_error 0", "push_begin 0 ; take_error 0", "finish_begin 0 ; take_error 0", "has_work",
                                           "init 0", "push_begin 0"]),
        ("tick_failed_init_finish_waiting", [r, "open", "init 0", "finish_begin 0", "select", "late -3 0 0", "settle -3 0 0", "finish_may_go 0", "finish_end 0 ; take_error 0",
                                             "finish_begin 0 ; take_error 0", "init 0", "finish_begin 0"]),
        ("tick_partial_lists", [r] + tick_up + ["open", "init 1", "push_end 0 3", "select", "late 0 0 0", "listed 0 0 0", "fetched 0 1", "fetched 1 0", "settle 0 0 0", "partial 0",
                                                "push_end 0 3 ; push_end 1 2", "select", "init 1", "late 0 0 0", "listed 0 0 0", "fetched 0 2", "fetched 1 5", "settle 0 0 0",
                                                "partial 0 ; partial 1", "init 0", "partial 0"]),
        ("res_finish_without_frames", [r] + res_up + ["finish_begin 0", "may_post 0 0", "posted 0 0 0 0 0 10", "may_stage 0", "may_finish 0", "idle 0 50", "may_post 0 0", "may_finish 0",
                                                      "to_finisher 0", "looks_at 0 ; active ; any_running", "finished 0 0 0 1234", "finish_may_go 0 ; finish_end 0", "active"]),
        ("res_two_chunks_and_finish", [r] + res_up + chunk + ["push_end 0 3", "may_stage 0", "finish_begin 0", "may_finish 0", "collect_due 0 0 ; stream_fails 0 0 0", "idle 0 300",
                                                              "may_init 0 ; may_post 0 0", "posted 0 0 0 1 2 320", "may_stage 0 ; stage_buf 0", "stage_take 0", "staged 0 0 0 0 3", "may_finish 0",
                                                              "idle 0 500", "may_post 0 0", "posted 0 0 0 0 3 520", "idle 0 700", "may_post 0 0 ; may_finish 0", "to_finisher 0",
                                                              "finished 0 0 0 11", "finish_may_go 0 ; finish_end 0"]),
        ("res_failed_init_push_waiting", [r, "open", "init 0", "push_end 0 21", "push_begin 0 ; push_may_go 0", "may_init 0", "inited 0 1 -3 7", "push_may_go 0", "push_end 0 2 ; take_error 0",
                                          "finish_begin 0 ; take_error 0", "active", "init 0", "may_init 0", "inited 0 2 0 0", "push_begin 0"]),
        ("res_failed_init_finish_waiting", [r, "open", "init 0", "finish_begin 0", "may_init 0", "inited 0 1 -3 7", "finish_may_go 0", "finish_end 0 ; take_error 0", "active"]),
        ("res_failed_init_and_init_again_meanwhile", [r, "open", "init 0", "may_init 0", "init 0", "inited 0 1 -3 7", "push_begin 0", "may_init 0", "inited 0 2 0 0", "push_begin 0 ; take_error 0"]),
        ("res_device_error", [r] + res_up + chunk + ["push_end 0 3", "collect_due 1 0 ; stream_fails 0 1 7", "stream_failed 0 -4 8", "idle 0 300", "may_init 0 ; may_post 0 0 ; may_stage 0",
                                                     "may_finish 0", "push_begin 0 ; take_error 0", "finish_begin 0", "may_post 0 0 ; may_stage 0 ; may_finish 0", "to_finisher 0", "finished 0 -4 8 0",
                                                     "finish_may_go 0", "finish_end 0 ; take_error 0", "init 0", "push_begin 0"]),
        ("res_device_error_finish_under_way", [r] + res_up + chunk + ["finish_begin 0", "stream_fails 0 1 7", "stream_failed 0 -4 8", "idle 0 300", "finish_may_go 0",
                                                                      "may_post 0 0 ; may_stage 0 ; may_finish 0", "to_finisher 0", "finished 0 -4 8 0", "finish_may_go 0", "finish_end 0 ; take_error 0"]),
        ("res_stop_for_a_collection", [r] + res_up + chunk + ["collect_due 1 1", "stream_fails 0 0 0", "may_post 0 0 ; may_stage 0", "collect_due 1 0 ; stream_fails 0 1 0", "idle 0 400", "may_post 0 0"]),
        ("res_staging_failure", [r] + res_up + ["push_end 0 6", "may_stage 0 ; stage_buf 0", "stage_take 0", "close_may_go 0", "staged 0 -3 5 0 4", "may_post 0 0", "push_begin 0 ; take_error 0",
                                               "push_begin 0", "may_stage 0 ; stage_buf 0", "stage_take 0", "staged 0 0 0 0 2", "may_post 0 0"]),
        ("res_post_failure", [r] + res_up + ["push_end 0 6", "stage_take 0", "staged 0 0 0 0 4", "stage_buf 0 ; stage_take 0", "staged 0 0 0 1 2", "may_post 0 0", "posted 0 -3 6 0 4 100",
                                            "may_post 0 0", "posted 0 0 0 1 2 120", "finish_begin 0 ; take_error 0", "idle 0 200", "may_finish 0"]),
        ("res_fail_all", [r] + res_up + chunk + ["open", "init 1", "finish_begin 1", "open", "fail_all -6 9", "active ; any_running", "finish_may_go 1 ; finish_end 1 ; take_error 1",
                                                 "push_begin 0 ; take_error 0", "push_begin 0", "close_begin 2 ; close_may_go 2", "close_end 2", "init 1", "may_init 1"]),
        ("res_close_while_a_chunk_runs", [r] + res_up + chunk + ["push_end 0 3", "close_begin 0", "close_may_go 0", "active", "idle 0 300", "close_may_go 0", "may_post 0 0", "posted 0 0 0 1 2 310",
                                                                 "close_may_go 0", "may_stage 0", "idle 0 400", "close_may_go 0", "close_end 0", "active", "open", "init 0", "may_init 0"]),
        ("res_init_mid_utterance", [r] + res_up + chunk + ["init 0", "may_init 0 ; may_stage 0", "idle 0 300", "may_init 0", "may_post 0 0", "posted 0 0 0 1 2 310", "idle 0 400", "may_init 0",
                                                           "inited 0 2 0 0", "may_post 0 0 ; may_stage 0"]),
        ("res_draining_stages_both_buffers", [r] + res_up + chunk + ["push_end 0 7", "idle 0 300", "may_post 0 1", "may_stage 0 ; stage_buf 0", "stage_take 0", "staged 0 0 0 0 4", "may_stage 0",
                                                                     "any_running", "may_post 0 0", "posted 0 0 0 1 2 900"]),
    ]
    # a script that concerns client 0 alone runs on one record: a record per client is what every step prints
    wide = ("tick_partial_lists", "res_fail_all")
    narrow = lambda l: " ".join(l.split()[:2]) if l.split()[0] in ("late", "listed", "settle") else l
    return [(n, ls if n in wide else [reset(1)] + [narrow(l) for l in ls[1:]]) for n, ls in s]


def lines_digest(single, scripts):
    """what ties a golden to the lines it was recorded for"""
    return hashlib.sha256("\n".join([n + ": " + l for n, l in single] + [n + ": " + l for n, ls in scripts for l in ls]).encode()).hexdigest()


def script_clients(reset_line):
    return int(reset_line.split()[1])
