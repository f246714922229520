"""The broker on the CPU, twice over.

Its per-client decisions (juicer_amd/csrc/jd_client.h: the settings, what each API call is answered with and changes, what its waits wait for, what
a tick selects, keeps and settles, what a round of the resident worker may do for a client and what a decoder call's result does to it):
tests/broker_driver.cpp, compiled with plain g++, is held to tests/golden/broker_golden.json - what the lines of jd_broker.cpp that jd_client.h
replaced made of the same inputs, recorded from the commit named in the file - integer by integer; after every step of a script the records are
checked, without the golden, for what must always hold of them.

And the whole of juicer_amd/csrc/jd_broker.cpp - threads, lock, condition variables - linked against a model decoder (tests/broker_fake_dec.cpp) into
a stand-alone program (tests/broker_harness.cpp) that runs plain, under ThreadSanitizer and under AddressSanitizer / UBSan: the callers' threads hold
every result to what they pushed, the fake holds the broker to the decoder's calling rules, a watchdog fails a scenario that does not end.

Kept as recorded, odd as they look: a tick's finisher need not be initialised while a late one must (select_finisher_not_inited, late_inited); push
accepts frames behind an unserved init while staging waits for it (push_begin_behind_an_unserved_init, may_stage_want_init); the staged queue
moves up behind a failed post (posted_rc_3_staged_2); the buffer choice that comes back to the running buffer is refused (stage_buf_refused)."""
import json
import os
import re
import subprocess

import pytest

from broker_cases import (CLIENT_ERROR, FIELDS, MAX_PENDING, MAX_TICK, NOT_BETWEEN, NOT_OPEN, OK, build_driver, build_harness, lines_digest, read_line, run_driver, script_cases,
                          script_clients, single_cases)

HERE = os.path.dirname(os.path.abspath(__file__))
SCENARIOS = ["several_clients", "without_frames", "init_mid_utterance", "close_unfinished_and_reopen", "init_failure_push", "init_failure_finish", "device_error", "collections",
             "large_push", "start_fails_at_create", "partial_lists", "yield_and_come_back", "kernel_ended", "stage_and_post_failures", "destroy_with_idle_clients"]
TICKS_ONLY, RESIDENT_ONLY = {"start_fails_at_create", "partial_lists"}, {"collections", "yield_and_come_back", "kernel_ended", "stage_and_post_failures"}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "broker_golden.json")) as f:
        doc = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{7,40}", doc["commit"]) and "decoder call" in doc["how"]
    return doc


@pytest.fixture(scope="module")
def lines(golden):
    """the driver's input: every single decision, then every script - the lines of broker_cases.py, which are the lines the golden was recorded for (it
    carries their digest, and an output per line under the case's name)"""
    single, scripts = single_cases(), script_cases()
    assert golden["lines_sha256"] == lines_digest(single, scripts)
    assert list(golden["single"]) == [n for n, _ in single] and [(n, len(o)) for n, o in golden["scripts"].items()] == [(n, len(ls)) for n, ls in scripts]
    return [l for _, l in single] + [l for _, ls in scripts for l in ls]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("broker") / "broker_driver"))


@pytest.fixture(scope="module")
def outputs(golden, lines, driver):
    """({name: (line, recorded, output)} of the single decisions, {name: [(line, recorded, output)]} of the scripts)"""
    out = run_driver(driver, lines)
    single = {n: (l, golden["single"][n], o) for (n, l), o in zip(single_cases(), out)}
    at, scripts = len(single), {}
    for n, ls in script_cases():
        scripts[n] = list(zip(ls, golden["scripts"][n], out[at:at + len(ls)]))
        at += len(ls)
    assert at == len(out)
    return single, scripts


def test_single_decisions_match_recorded(outputs):
    single, _ = outputs
    assert len(single) >= 280 and len({l for l, _, _ in single.values()}) == len(single)     # no case twice
    bad = [(name, line, want, got) for name, (line, want, got) in single.items() if want != got]
    for b in bad:
        print(*b)
    assert not bad


def test_scripts_match_recorded(outputs):
    _, scripts = outputs
    assert len(scripts) >= 23
    bad = [(name, line, want, got) for name, steps in scripts.items() for line, want, got in steps if want != got]
    for b in bad:
        print(*b)
    assert not bad


def answers(single, name, n=1):
    return read_line(single[name][2], n)[0]


def test_cases_cover_what_they_must(outputs):
    single, scripts = outputs
    a = lambda name, n=1: answers(single, name, n)
    r = lambda name, k=0, n=1: read_line(single[name][2], n)[2][k]
    # the settings: max_tick max_pending coalesce interval resident fail_init_of
    assert a("settings_default") == [256, 1024, 300, 0, 1, -1] and a("settings_64_clients")[4] == 1 and a("settings_65_clients") == [192, 768, 300, 0, 0, -1]
    assert a("settings_65_clients_resident_1")[4] == 1 and a("settings_resident_0")[:2] == [192, 768] and a("settings_trial_failed") == [256, 1024, 300, 0, 0, -1]
    assert [a("settings_tick_" + v)[0] for v in ("0", "1", "65536", "65537")] == [192, 1, 65536, 192] and a("settings_tick_1")[1] == 4      # (a knob set and refused: 192)
    assert [a("settings_coalesce_" + v)[2] for v in ("minus_1", "0", "1000000", "1000001")] == [300, 0, 1000000, 300]
    assert a("settings_fail_init_3")[5] == 3 and a("settings_interval_50")[3] == 50 and a("consts") == [3000, 20000, 200, 20]
    # the API calls
    assert a("open_first_free", 3) == [1] and a("open_all_taken", 2) == [-1] and r("open_is_a_new_record")["init_req"] == 0
    assert [a("push_begin_" + n) for n in ("base", "open", "inited", "want_finish", "err", "behind_an_unserved_init", "failed_init")] == [
        [OK], [NOT_OPEN], [NOT_BETWEEN], [NOT_BETWEEN], [CLIENT_ERROR], [OK], [CLIENT_ERROR]]
    assert [a("push_may_go_pending_%d" % p) for p in (0, 1, MAX_PENDING - 1, MAX_PENDING, MAX_PENDING + 1)] == [[1], [1], [1], [1], [0]] and a("push_may_go_failed_and_full") == [1]
    assert [a("finish_begin_" + n) for n in ("base", "open", "inited", "want_init", "failed_init", "failed_stream", "failed_init_next_asked")] == [
        [OK], [NOT_OPEN], [NOT_BETWEEN], [OK], [CLIENT_ERROR], [OK], [CLIENT_ERROR]]
    assert a("take_error_once") == [-3, 0] and a("take_error_failed_stays") == [-3, -3] and a("partial_not_open")[0] == NOT_OPEN
    i = r("init_base")
    assert (i["pending"], i["err"], i["failed"], i["want_finish"], i["want_init"], i["init_req"], i["inited"]) == (0, 0, 0, 0, 1, 5, 1)
    assert [a("close_may_go_" + n) for n in ("base", "want_init", "running", "n_staged", "in_flight", "finishing", "want_finish", "pending")] == [[1], [0], [0], [0], [0], [0], [1], [1]]
    # a tick: n_inits {i seen} n_pushers {i frames} n_finishers {i}
    assert [a("select_pending_%d" % p) for p in (0, 1, MAX_TICK - 1, MAX_TICK, MAX_TICK + 1)] == [[0, 0, 0], [0, 1, 0, 1, 0], [0, 1, 0, 3, 0], [0, 1, 0, 4, 0], [0, 1, 0, 4, 0]]
    assert r("select_pending_%d" % (MAX_TICK + 1))["pending"] == 1 and r("select_pending_%d" % (MAX_TICK + 1))["in_flight"] == 1
    assert a("select_frames_behind_an_unserved_init") == [1, 0, 2, 1, 0, 3, 0] and a("select_frames_of_nobody") == [0, 0, 0]
    assert a("select_finisher_not_inited") == [0, 0, 1, 0] and a("late_inited") == [0, 1, 0, 2, 0, 0]                 # the two finisher tests: no `inited` / `inited`
    assert a("select_finisher_with_frames_left") == [0, 1, 0, 4, 0] and a("select_finisher_with_its_last_frames") == [0, 1, 0, 4, 1, 0]
    assert a("late_base")[-2:] == [1, 0] and [a("late_" + n)[-1] for n in ("open", "want_finish", "pending", "want_init", "tick_failed_for_it", "is_a_finisher_already")] == [0] * 6
    assert a("listed_pushers_then_finishers", 3)[-4:] == [3, 1, 2, 0] and a("listed_failed_pusher", 3)[-3:] == [2, 2, 0] and a("listed_failed_pusher_that_finishes", 3)[-4:] == [3, 1, 0, 2]
    assert [a("fetched_" + n)[-1] for n in ("kept", "kept_with_its_init", "init_again_meanwhile", "init_meanwhile")] == [1, 1, 0, 0]
    f = r("settle_init_failed")
    assert (f["failed"], f["err"], f["msg"], f["pending"], f["want_finish"], f["inited"], f["in_flight"]) == (1, -3, 100, 0, 0, 0, 0)
    g = r("settle_init_failed_and_again_meanwhile")
    assert (g["failed"], g["err"], g["want_init"], g["inited"]) == (0, -3, 1, 0)
    assert r("settle_finisher")["result"] == 1000 and r("settle_finisher")["inited"] == 0
    # the resident worker
    assert [a("stop_idle_%d_%d" % (on, us)) for on in (0, 1) for us in (3000, 3001)] == [[0], [0], [0], [1]]
    assert [a("drain_due_%d_%d" % (sy, us)) for sy in (0, 1) for us in (20000, 20001)] == [[0], [0], [0], [1]]
    assert [a("active_" + n) for n in ("base", "want_init", "want_finish", "running", "finishing", "n_staged", "inited", "pending", "inited_with_frames", "closed")] == [
        [0], [1], [1], [1], [1], [1], [0], [0], [1], [0]]
    assert a("stream_fails_idle_1_err_7_failed_0") == [1] and [a("stream_fails_idle_%d_err_%d_failed_%d" % k) for k in ((0, 7, 0), (1, 0, 0), (1, 7, 1))] == [[0], [0], [0]]
    assert r("stream_failed_finish_under_way")["want_finish"] == 1 and r("stream_failed")["n_staged"] == 0 and r("stream_failed")["failed"] == 1
    assert a("may_post_base") == [1, 1, 3] and a("may_post_draining") == [0, -1, -1] and a("may_post_chunk_of_none_base") == [1, 0, 0]
    assert [a("may_post_chunk_of_none_" + n)[0] for n in ("fresh", "want_finish", "pending", "inited", "running", "draining")] == [0] * 6
    p = r("posted_rc_3_staged_2")                                       # (the queue moves up behind a failed post too)
    assert (p["n_staged"], p["sb0"], p["sn0"], p["running"], p["err"], p["fresh"]) == (1, 0, 4, 0, -3, 1)
    p = read_line(single["posted_rc_0_staged_1"][2], 1)
    assert p[1] == {"ticks": 1, "frames": 3, "stream_ticks": 1, "us_idle": 250, "us_search": 0} and (p[2][0]["running"], p[2][0]["run_buf"], p[2][0]["fresh"]) == (1, 1, 0)
    assert read_line(single["posted_first_of_an_utterance"][2], 1)[1]["us_idle"] == 0 and read_line(single["idle"][2], 1)[1]["us_search"] == 250
    assert [a("may_stage_" + n)[0] for n in ("base", "inited", "failed", "want_init", "pending", "running", "n_staged", "want_finish")] == [1, 0, 0, 0, 0, 1, 1, 1]
    assert [a("may_stage_running_%d_staged_%d" % k)[0] for k in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2))] == [1, 1, 0, 1, 0, 0]
    # the buffer choice, all sixteen: never the running buffer, never the staged one where one of each is possible; the refused case
    for run in (0, 1):
        for rb in (0, 1):
            for ns in (0, 1):
                for sb in (0, 1):
                    buf = a("stage_buf_running_%d_in_%d_staged_%d_in_%d" % (run, rb, ns, sb))[0]
                    if run and ns and rb != sb:
                        assert buf == -1, (run, rb, ns, sb)             # both buffers taken (brk_res_may_stage says no before it comes to this): refused
                    else:
                        assert buf in (0, 1) and not (run and buf == rb) and not (ns and buf == sb), (run, rb, ns, sb, buf)
    assert a("stage_buf_refused") == [0, -1, -1]                           # may_stage (and no buffer), stage_buf
    assert [a("may_finish_" + n) for n in ("base", "running", "n_staged", "inited", "fresh", "want_finish", "pending", "failed")] == [[1], [0], [0], [0], [0], [0], [0], [1]]
    fa = read_line(single["fail_all"][2], 4)[2]
    assert [x["err"] for x in fa] == [-6, -3, 0, -6] and all(not (x["want_init"] or x["want_finish"] or x["pending"] or x["n_staged"] or x["running"]) for x in fa) and fa[3]["finishing"] == 1
    # the scripts reach what the GPU tests reach by luck
    st = lambda name, k: read_line(scripts[name][k][2], script_clients(scripts[name][0][0]))
    assert st("tick_init_during_a_tick", 8)[0] == [0] and st("tick_init_during_a_tick", 9)[2][0]["want_init"] == 1 and st("tick_init_during_a_tick", 13)[2][0]["want_init"] == 0
    late = [i for i, (l, _, _) in enumerate(scripts["tick_late_finisher"]) if l.startswith("late")][-1]
    assert st("tick_late_finisher", late)[0] == [1, 0] and st("tick_late_finisher", late + 3)[2][0]["result"] == 1000
    assert st("tick_failed_init_push_waiting", 5)[0] == [0] and st("tick_failed_init_push_waiting", 10)[0] == [1] and st("tick_failed_init_push_waiting", 11)[0] == [CLIENT_ERROR, -3]
    assert st("res_device_error_finish_under_way", -1)[0] == [CLIENT_ERROR, -4]
    assert st("res_close_while_a_chunk_runs", -6)[0] == [1] and st("res_close_while_a_chunk_runs", -9)[0] == [0]


def holds(c):
    """what must hold of a record between two steps, whatever the script: restated here, not read from the header"""
    assert 0 <= c["n_staged"] <= 2 and c["n_staged"] + c["running"] <= 2
    bufs = [c["sb%d" % k] for k in range(c["n_staged"])] + ([c["run_buf"]] if c["running"] else [])
    assert all(b in (0, 1) for b in bufs) and len(set(bufs)) == len(bufs)                    # the staged buffers and the running one are pairwise different
    assert all(c["sn%d" % k] >= 1 for k in range(c["n_staged"]))
    if c["finishing"]:
        assert not c["running"] and c["n_staged"] == 0 and c["inited"]
    if not c["open"]:
        assert not any(c[k] for k in ("want_init", "want_finish", "inited", "pending", "running", "n_staged", "finishing", "in_flight"))
    if c["failed"]:
        assert c["err"] != 0 and c["pending"] == 0 and c["n_staged"] == 0
    assert c["pending"] == 0 or c["inited"] or c["want_init"]                                # frames only within an utterance
    assert 0 <= c["taken"] <= MAX_TICK
    assert (c["err"] == 0) == (c["msg"] == 0) or c["err"] == 0                               # an error has its text


def test_invariants_after_every_script_step(outputs, driver):
    _, scripts = outputs
    n_steps = 0
    for name, steps in scripts.items():
        n = script_clients(steps[0][0])
        prev = None
        for line, _, o in steps:
            _, stats, recs = read_line(o, n)
            for k, c in enumerate(recs):
                try:
                    holds(c)
                except AssertionError:
                    raise AssertionError((name, line, k, c))
                if prev:
                    assert c["init_req"] >= prev[1][k]["init_req"] or not prev[1][k]["open"] or line.startswith("open"), (name, line, k)
            if prev:
                assert all(stats[s] >= prev[0][s] for s in stats), (name, line)                   # the statistics only grow
            prev = (stats, recs)
            n_steps += 1
    assert n_steps >= 500
    # ... and the header's own statement of the same says so of every step too
    for name, steps in scripts.items():
        ls = [l + " ; ok" if i else l for i, (l, _, _) in enumerate(steps)]
        n = script_clients(ls[0])
        for l, o in list(zip(ls, run_driver(driver, ls)))[1:]:
            answers_, _, _ = read_line(o, n)
            assert answers_[-n:] == [0] * n, (name, l, answers_[-n:])


def test_broker_driver_under_sanitizers(lines, outputs, tmp_path_factory):
    """every line once more through the driver built with -fsanitize=address,undefined: the same output, nothing reported"""
    single, scripts = outputs
    driver = build_driver(str(tmp_path_factory.mktemp("broker_san") / "broker_driver_san"), ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert run_driver(driver, lines) == [o for _, _, o in single.values()] + [o for steps in scripts.values() for _, _, o in steps]


@pytest.mark.parametrize("flavour,flags", [("plain", ()), ("thread", ("-fsanitize=thread",)), ("address", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))])
def test_whole_broker_against_the_fake_decoder(flavour, flags, tmp_path_factory):
    """jd_broker.cpp itself with its threads: every scenario with both workers where it has both, nothing reported by the sanitizer, and an end (the
    harness's watchdog gives a scenario 30 s; the timeout here stands behind it)"""
    exe = build_harness(str(tmp_path_factory.mktemp("broker_" + flavour) / "broker_harness"), flags)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-3000:])
    assert p.returncode == 0 and p.stderr == ""
    ran = [tuple(l.split()[1:3]) for l in p.stdout.splitlines() if l.startswith("ok ")]
    want = [(s, w) for s in SCENARIOS for w in ("ticks", "resident") if not (w == "ticks" and s in RESIDENT_ONLY) and not (w == "resident" and s in TICKS_ONLY)]
    assert ran == want and p.stdout.splitlines()[-1] == "all %d runs passed" % len(want)
