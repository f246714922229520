"""The decisions of the streaming interface (juicer_amd/csrc/jd_push.h: a stream's record, the argument checks, PARTIAL_DECODING's schedule for one
stream and for many, the packing of a jd_streams_push call, k_partial_many's layout) on the CPU: tests/push_driver.cpp, compiled with plain g++,
is held to tests/golden/push_golden.json - what the lines of jd_host_stream.h that jd_push.h replaced made of the same inputs, recorded from the
commit named in the file - integer by integer.  After every step of a script the records are checked for what must always hold of them; the one-
stream path and the many-stream path are held to each other over the same replies, and both to a restatement of WFSTDecoderLite.cpp:358-368,
without the golden.

Kept as recorded, odd as they look: the entries in front of a refused entry of jd_streams_push have opened their streams (pack_stream_twice,
pack_not_started); a stream that failed stands at its chunk's end in the one path and at the call's target in the other - and in the one path
the chunks behind the failed one are still launched and fail in turn, so that it stands at the call's target there too (one_stream_fails_one)."""
import json
import os
import re

import pytest

from push_cases import (ARG_BAD, ARG_BAD_STREAM, ARG_NOT_STARTED, ARG_OK, ARG_TOO_MANY_ROWS, CALLS, EVERY, FROM_RESULTS, FROM_STAGE, NOT_FOUND, ROW_LIMIT, SHARE,
                        TILE, TOO_LONG, build_driver, j, read_step, reference_schedule, run_driver, script_cases, script_streams, single_cases)

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "push_golden.json")) as f:
        doc = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{7,40}", doc["commit"]) and "HIP call" in doc["how"]
    return doc


@pytest.fixture(scope="module")
def lines(golden):
    """the driver's input: every single decision, then every script - the lines of push_cases.py, which are the lines the golden was recorded for"""
    single, scripts = single_cases(), script_cases()
    assert [(c["name"], c["line"]) for c in golden["single"]] == single
    assert [(s["name"], s["lines"]) for s in golden["scripts"]] == scripts
    return [l for _, l in single] + [l for _, ls in scripts for l in ls]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("push") / "push_driver"))


@pytest.fixture(scope="module")
def outputs(golden, lines, driver):
    """({name: (line, recorded, output)} of the single decisions, {name: [(line, recorded, output)]} of the scripts)"""
    out = run_driver(driver, lines)
    single = {c["name"]: (c["line"], c["out"], o) for c, o in zip(golden["single"], out)}
    at, scripts = len(golden["single"]), {}
    for s in golden["scripts"]:
        scripts[s["name"]] = list(zip(s["lines"], s["out"], out[at:at + len(s["lines"])]))
        at += len(s["lines"])
    assert at == len(out)
    return single, scripts


def test_single_decisions_match_recorded(outputs):
    single, _ = outputs
    assert len(single) >= 110 and len({l for l, _, _ in single.values()}) == len(single)     # no case twice
    bad = [(name, line, want, got) for name, (line, want, got) in single.items() if want != got]
    for b in bad:
        print(*b)
    assert not bad


def test_scripts_match_recorded(outputs):
    _, scripts = outputs
    assert len(scripts) >= 19
    bad = [(name, line, want, got) for name, steps in scripts.items() for line, want, got in steps if want != got]
    for b in bad:
        print(*b)
    assert not bad


def test_cases_cover_what_they_must(outputs):
    single, scripts = outputs
    out = {n: o for n, (_, _, o) in single.items()}
    # the chunk rule: the first chunk ends with T = 101; room for <= 0, 1, Fc, Fc + 1 frames up to the rule's frame; interval 0; left < Fc
    assert out["chunk_first_ends_with_T_101"] == [EVERY + 1]
    assert [out["chunk_rule_" + n] for n in ("behind_by_50", "room_0", "room_1", "room_Fc_minus_1", "room_Fc", "room_Fc_plus_1")] == [[1], [1], [1], [63], [64], [64]]
    assert out["chunk_interval_0"] == [64] and out["chunk_left_below_Fc"] == [5] and out["chunk_left_below_Fc_rule_nearer"] == [2]
    # after a launch: failed at collected host_collects T due last_collect n_collect
    a = {n[6:]: dict(zip(("failed", "at", "collected", "host_collects", "T", "due", "last_collect", "n_collect"), o)) for n, o in out.items() if n.startswith("after_")}
    assert (a["error"]["failed"], a["error"]["T"], a["error_call_target"]["T"], a["error"]["collected"]) == (1, 64, 300, 0)
    assert (a["short_no_collection"]["collected"], a["short_collected_by_count"]["collected"], a["short_collected_by_count"]["host_collects"]) == (0, 1, 0)
    assert a["short_frame_rule_would_fire"]["collected"] == 0 and a["short_count_rule_would_fire"]["collected"] == 0     # the host looks behind the limit only
    assert [a[n]["host_collects"] for n in ("limit_gap_100", "limit_gap_101", "limit_gap_100_after_a_collection", "limit_gap_101_after_a_collection")] == [0, 1, 0, 1]
    assert [a[n]["host_collects"] for n in ("limit_n_path_10000", "limit_n_path_10001", "limit_ratio_12_exactly", "limit_ratio_above_12", "limit_path_new_0",
                                            "limit_path_new_0_n_path_10000")] == [0, 1, 0, 1, 1, 0]
    assert (a["limit_collected_and_rule"]["collected"], a["limit_collected_and_rule"]["host_collects"]) == (1, 0)
    assert [a[n]["collected"] for n in ("flag_set", "flag_clear_count_moved", "flag_ignored_by_count", "short_collected_by_count")] == [1, 0, 0, 1]   # the two predicates
    assert (a["flag_clear_at_limit_rule_fires"]["host_collects"], a["flag_set_at_limit"]["host_collects"]) == (1, 0)
    assert [a[n]["due"] for n in ("trace_gap_eq_interval", "trace_gap_interval_plus_1", "trace_first", "trace_first_interval_100", "trace_first_interval_99")] == [0, 1, 0, 1, 1]
    assert a["limit_gap_101"]["last_collect"] == 100 and a["limit_gap_101"]["n_collect"] == 1 and a["limit_gap_100"]["last_collect"] == -1
    # a round: nact {entry} {limit} {weight} f_end s_lo s_hi {hT}
    assert out["round_one_at_target"][:3] == [2, 1, 2] and out["round_one_out"][:3] == [2, 1, 2] and out["round_nobody"][0] == 0
    assert out["round_limit_eq_target"][3:5] == [101, 202] == out["round_limit_below_target"][3:5]
    g = out["round_gaps"]
    assert g[:3] == [2, 0, 1] and g[7:10] == [202, 2, 5] and g[10:] == [5, 9, 60, 9, 9, 202, 9, 9]              # s_lo .. s_hi covers streams 3 and 4 too
    # packing: verdict stream rows {open}, tile_rows nwork {stream slot weight target row0 entry} ...
    assert out["pack_entry_with_0_frames"][:3] == [ARG_OK, -1, 15] and out["pack_entry_with_0_frames"][8] == 2 and out["pack_entry_with_0_frames"][4] == 0
    assert out["pack_negative_slot"][9:11] == [2, -7] and out["pack_negative_slot"][15:17] == [1, -37]
    assert [out["pack_rows_" + n][7] for n in ("1", "tile", "tile_plus_1")] == [TILE, TILE, 2 * TILE] and out["pack_rows_tile"][-2:] == [128, 0]
    assert out["pack_rows_tile_plus_1"][-2:] == [129, 127] and out["pack_rows_0"][:3] == [ARG_OK, -1, 0] and len(out["pack_rows_0"]) == 7
    assert out["pack_stream_twice"][:2] == [ARG_BAD_STREAM, 0] and out["pack_stream_twice"][3:7] == [1, 1, 0, 0]    # (the entries in front have opened theirs)
    assert out["pack_not_started"][:2] == [ARG_NOT_STARTED, 3] and out["pack_negative_stream"][:2] == [ARG_BAD_STREAM, -1]
    assert out["pack_row_limit_plus_1"][:3] == [ARG_TOO_MANY_ROWS, -1, ROW_LIMIT + 1] and out["pack_two_to_the_31"][0] == ARG_TOO_MANY_ROWS
    t = out["pack_three_streams"]                                       # src_at T_at need grown: [35 x 39 floats][128 ints][4 ints], half as much again
    assert t[27] == 60 and t[28:32] == [35 * 39 * 4, 35 * 39 * 4 + 128 * 4, 35 * 39 * 4 + 128 * 4 + 16, (35 * 39 * 4 + 128 * 4 + 16) * 3 // 2] and t[32:36] == [10, 60, 12, 0]
    assert [out["check1_" + n] for n in ("ok", "no_decoder", "stream_eq_n", "no_frames_pointer", "zero_frames_no_pointer", "not_started")] == [[ARG_OK], [ARG_BAD], [ARG_BAD],
                                                                                                                                              [ARG_BAD], [ARG_OK], [ARG_NOT_STARTED]]
    assert out["tracelist_ok"] == [ARG_OK, -1, 0, 0, 0, 2, 2, 1, 0, 2] and out["tracelist_twice"][:2] == [ARG_BAD_STREAM, 2]     # (stream 0 has no frame yet)
    # k_partial_many: decision, where the entry's share begins, words fetched
    assert [out["reply_" + n][0] for n in ("not_found", "share", "share_plus_1", "res_cap", "above_res_cap", "above_res_cap_and_share")] == [
        NOT_FOUND, FROM_STAGE, FROM_RESULTS, FROM_STAGE, TOO_LONG, TOO_LONG]
    assert out["reply_first_entry"][1:] == [2 * 16, 16 * (2 + 2 * SHARE)] and out["reply_last_entry"][1] == 2 * 16 + 2 * SHARE * 15
    assert out["layout_16"] == [4 * 16, 2 + 2 * SHARE, 4 * 16 + 16 * (2 + 2 * SHARE)]
    assert out["finish_partial"] == [0, 3, 7, 10, 8, 25, 9, 31] and out["finish_no_hypothesis"] == [0, 2, 7, 10, 8, 25]
    # the scripts reach: a failure in the middle of a call beside streams that go on, a call behind finish and init, a take-over in between
    steps = [read_step(o, 3) for _, _, o in scripts["one_stream_fails_many"]]
    failed = steps[4]
    assert failed["streams"][1]["dirty"] == 1 and failed["streams"][1]["T"] == 250 and [s["T"] for s in failed["streams"]] == [250, 250, 250]
    assert sum(1 for k, *_ in failed["log"] if k == "launch") == 3 and [len(e[1]) for e in failed["log"] if e[0] == "launch"] == [3, 3, 2]
    assert steps[7]["streams"][1]["n_collect"] == 0 and steps[8]["streams"][1]["T"] == 120 and steps[8]["streams"][1]["n_collect"] == 1
    t = [read_step(o, 2) for _, _, o in scripts["takeover_in_between_many"]]
    assert [s["started"] for s in t[4]["streams"]] == [0, 0] and t[5]["rc"] == ARG_NOT_STARTED and t[8]["rc"] == ARG_OK
    assert read_step(scripts["stream_twice"][3][2], 2)["rc"] == ARG_BAD_STREAM


def booked(steps, M):
    """per stream, within its utterances: [[(frame collected behind, trace due)]] - a new list with every init"""
    per = [[[]] for _ in range(M)]
    for line, o in steps:
        if line.startswith("init"):
            per[int(line.split()[1])].append([])
        for e in read_step(o, M)["log"]:
            if e[0] == "booked":
                per[e[1]][-1].append((e[2], e[3]))
    return per


def pushed(line):
    """a push line -> {stream: frames}"""
    w = [int(x) for x in line.split()[1:]]
    if line.startswith("push1"):
        return {w[0]: w[1]}
    out, at = {}, 1
    for _ in range(w[0]):
        out[w[at]] = w[at + 1]
        at += 3 + 4 * w[at + 2]
    return out


def test_invariants_after_every_script_step(outputs):
    _, scripts = outputs
    n_steps = n_failed = 0
    for name, steps in scripts.items():
        M, interval = script_streams(steps[0][0]), int(steps[0][0].split()[2])
        assert steps[0][0].startswith("reset")
        prev = None
        for line, _, o in steps:
            s = read_step(o, M)
            n_steps += 1
            for k, st in enumerate(s["streams"]):
                where = (name, line, k)
                if st["started"]:                                                                # (a take-over sets T back and leaves the rest)
                    assert st["last_trace"] <= st["last_collect"] < st["T"], where
                if prev and not line.startswith("init"):
                    assert st["n_collect"] >= prev["streams"][k]["n_collect"], where             # never decreases within an utterance
                if interval > 0 and st["started"] and not st["dirty"]:
                    assert st["T"] - 1 - st["last_collect"] <= EVERY, where                      # never more than 100 frames behind a collection
            if line.startswith("push") and interval > 0 and s["rc"] == ARG_OK:                   # a failed stream is at its target
                for k, nf in pushed(line).items():
                    if s["streams"][k]["dirty"]:
                        n_failed += 1
                        assert s["streams"][k]["T"] == prev["streams"][k]["T"] + nf, (name, line, k)
            prev = s
    assert n_steps >= 120 and n_failed >= 6


def test_one_stream_path_and_many_stream_path_agree(outputs):
    """the same call list and the same replies through jd_stream_push and through jd_streams_push: the same collections, the same traces due, the
    same records in the end, a failed stream's included"""
    _, scripts = outputs
    for name, (M, *_r) in CALLS.items():
        one, many = [[(l, o) for l, _, o in scripts[name + suffix]] for suffix in ("_one", "_many")]
        assert booked(one, M) == booked(many, M), name
        assert read_step(one[-1][1], M)["streams"] == read_step(many[-1][1], M)["streams"], name


@pytest.mark.parametrize("interval", [1, 150])
def test_frame_rule_alone_collects_after_100_201_302(driver, interval):
    """replies that never collect on the device: whatever the chunking - pushes of 1, 7, 64, 101 and 500 frames, one stream at a time or three
    streams at different offsets in one call, tables of 64 frames or of 512 - every stream collects after exactly frames 100, 201, 302, ... and
    traces where :362-368 say"""
    total = 707
    want_c, want_t = reference_schedule(total, interval)
    assert want_c == list(range(EVERY, total, EVERY + 1)) and len(want_c) == 7
    offsets = (0, 30, 57)
    for Fc in (64, 512):
        for push in (1, 7, 64, 101, 500):
            for many in (False, True):
                lines = [j("reset", 3, interval, 0, Fc), "init 0", "init 1", "init 2"]
                at = [0, 0, 0]
                for s, off in enumerate(offsets):                        # the streams stand at different frames before the common calls
                    if off:
                        lines.append(j("push1", s, off, 0))
                        at[s] = off
                while min(at) < total:
                    n = [min(push, total - a) for a in at]
                    if many:
                        lines.append(j("pushN", 3, [[s, n[s], 0] for s in range(3)]))
                    else:
                        lines += [j("push1", s, n[s], 0) for s in range(3) if n[s]]
                    at = [a + k for a, k in zip(at, n)]
                out = run_driver(driver, lines)
                per = booked(list(zip(lines, out)), 3)
                for s in range(3):
                    got = per[s][-1]
                    assert [f for f, _ in got] == want_c, (Fc, push, many, s)
                    assert [f for f, due in got if due] == want_t, (Fc, push, many, s)
                assert [st["T"] for st in read_step(out[-1], 3)["streams"]] == [total] * 3


def test_count_rule_collections_fall_where_the_reference_puts_them(outputs):
    """device_collections: the kernel's collections (the count rule in the middle of a launch) and the host's (the count rule behind a stream's last
    frame) beside the frame rule, against the restatement of :358-368 given the frames behind which the count rule is said to fire"""
    _, scripts = outputs
    fires = ({29, 135, 150}, {300}, {39})                               # (stream 1: 12000 / 1000 behind frame 299 does not fire, 12001 / 1000 behind 300 does)
    frames = (300, 301, 140)
    for name, interval in (("device_collections", 1), ("device_collections_reference_counts", 150)):
        for suffix in ("_one", "_many"):
            per = booked([(l, o) for l, _, o in scripts[name + suffix]], 3)
            for s in (0, 2) if "reference" in name else (0, 1, 2):
                want_c, want_t = reference_schedule(frames[s], interval, lambda f: f in fires[s])
                assert [f for f, _ in per[s][-1]] == want_c, (name, suffix, s)
                assert [f for f, due in per[s][-1] if due] == want_t, (name, suffix, s)
    assert reference_schedule(300, 1, lambda f: f in fires[0])[0] == [29, 130, 135, 150, 251]
    # with the reference's counts a collection that only the arena asked for is none: no booking, and the launch goes on behind it
    for suffix in ("_one", "_many"):
        steps = [(l, read_step(o, 3)) for l, _, o in scripts["device_collections_reference_counts" + suffix]]
        per = booked([(l, o) for l, _, o in scripts["device_collections_reference_counts" + suffix]], 3)
        assert [f for f, _ in per[1][-1]] == reference_schedule(300, 150, lambda f: f == 249)[0] == [100, 201, 249]
        stops = [x for _, s in steps for e in s["log"] if e[0] == "launch" for x in e[1] if x[0] == 1 and x[2] < x[1]]   # stream 1 short of its limit
        assert [x[2] for x in stops] == [20, 249, 250], (suffix, stops)


def test_push_driver_under_sanitizers(lines, outputs, tmp_path_factory):
    """every line once more through the driver built with -fsanitize=address,undefined: the same output, nothing reported"""
    single, scripts = outputs
    driver = build_driver(str(tmp_path_factory.mktemp("push_san") / "push_driver_san"), ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert run_driver(driver, lines) == [o for _, _, o in single.values()] + [o for steps in scripts.values() for _, _, o in steps]
