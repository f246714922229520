"""The decisions of working ahead (juicer_amd/csrc/jd_ahead.h: the queue of announced batches, their tables, the banks of streams, decode_wave's
claim / place / tables / chunk work, the batch behind, the waves of a batch) on the CPU: tests/ahead_driver.cpp, compiled with plain g++, is held
to tests/golden/ahead_golden.json - what the lines of jd_device.hip and jd_host_launch.h that jd_ahead.h replaced made of the same inputs,
recorded from the commit named in the file - integer by integer; and after every step of a script the queue is checked for what must always
hold of it.

Kept as recorded, odd as they look: a zero-length utterance is a work item of weight 0 in chunk 0 (chunk_zero_length_utterance); free_table
with FG_BOTH matches no table, so table 0 counts as free beside a wave in chunks (free_table_fg-2_*; the callers score nothing meanwhile);
a fourth announcement is silently not taken (announce_fourth_entry, script four_announcements); a stream that stands past the end of a
chunk would be a work item of negative weight (chunk_resumed_beyond_c1: unreachable, a resumed wave has one chunk)."""
import json
import os
import re

import pytest

from ahead_cases import (ANNOUNCED, BG_GO_ON, BG_NONE, BG_START, FG_BOTH, SCORED, build_driver, read_decode, read_queue, run_driver, script_cases,
                         single_cases)

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "ahead_golden.json")) as f:
        doc = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{7,40}", doc["commit"]) and "HIP call" in doc["how"]
    return doc


@pytest.fixture(scope="module")
def lines(golden):
    """the driver's input: every single decision, then every script - the lines of ahead_cases.py, which are the lines the golden was recorded for"""
    single, scripts = single_cases(), script_cases()
    assert [(c["name"], c["line"]) for c in golden["single"]] == single
    assert [(s["name"], s["lines"]) for s in golden["scripts"]] == scripts
    return [l for _, l in single] + [l for _, ls in scripts for l in ls]


@pytest.fixture(scope="module")
def outputs(golden, lines, tmp_path_factory):
    """({name: (line, recorded, output)} of the single decisions, {name: [(line, recorded, output)]} of the scripts)"""
    out = run_driver(build_driver(str(tmp_path_factory.mktemp("ahead") / "ahead_driver")), lines)
    single = {c["name"]: (c["line"], c["out"], o) for c, o in zip(golden["single"], out)}
    at, scripts = len(golden["single"]), {}
    for s in golden["scripts"]:
        scripts[s["name"]] = list(zip(s["lines"], s["out"], out[at:at + len(s["lines"])]))
        at += len(s["lines"])
    assert at == len(out)
    return single, scripts


def test_single_decisions_match_recorded(outputs):
    single, _ = outputs
    assert len(single) >= 150 and len({l for l, _, _ in single.values()}) == len(single)     # no case twice
    for name, (line, want, got) in single.items():
        if want != got:
            print(name, line, "recorded", want, "now", got)
    assert not [name for name, (_, want, got) in single.items() if want != got]


def test_scripts_match_recorded(outputs):
    _, scripts = outputs
    assert len(scripts) >= 12
    bad = [(name, line, want, got) for name, steps in scripts.items() for line, want, got in steps if want != got]
    for b in bad:
        print(*b)
    assert not bad


def test_queue_invariants_after_every_script_step(outputs):
    _, scripts = outputs
    n_waves = 0
    for name, steps in scripts.items():
        for line, _, o in steps:
            if not line.startswith("decode"):
                q = read_queue(o[1:])
                assert len(q) <= 3 and all(e["bank"] < 0 for e in q if e["state"] != SCORED), (name, line)
                continue
            feats, n_utts = (int(x) for x in line.split()[1:3])
            for w in read_decode(o):
                n_waves += 1
                q = w["queue"]
                assert len(q) <= 3, (name, line)                          # the queue never exceeds three entries
                if not w["ok"]:
                    assert q == [], (name, line)                         # the error way out: nothing ahead survives
                    continue
                held = [e["buf"] for e in q if e["state"] == SCORED]
                assert len(held) == len(set(held)) and all(0 <= t < 3 for t in held), (name, line)   # no table held by two queued batches ...
                launched = sum(c["launched"] for c in w["chunks"])
                if w["n_chunks"] == 1:                                   # ... nor by one and the wave that ran (what was scored beside it included)
                    assert w["table"] not in held, (name, line)
                else:
                    assert held == [] and launched == 0, (name, line)
                banks = [e["bank"] for e in q if e["bank"] >= 0]
                assert len(banks) <= 1, (name, line)                     # at most one queued batch holds a bank ...
                if w["pipe"]:
                    assert w["bank"] not in banks and w["s0"] == w["bank"] * (int(steps[0][0].split()[1]) // 2), (name, line)   # ... never the wave's
                else:
                    assert banks == [] and w["s0"] == 0, (name, line)
                if w["mine"]:                                            # a claimed entry is gone from the queue: every table behind it is another's
                    assert w["need"] == 0 and not w["drop"], (name, line)
                    assert n_utts > int(steps[0][0].split()[1]) or all(not (e["feats"] == feats and e["state"] == SCORED and e["buf"] == w["table"]) for e in q)
                assert not (w["drop"] or w["discard"] or w["none_free"]) or all(e["state"] != SCORED or launched for e in q), (name, line)
    assert n_waves >= 70


def test_cases_cover_what_they_must(outputs):
    single, scripts = outputs
    out = {n: o for n, (_, _, o) in single.items()}
    # claim
    assert out["claim_match"] == [1, 0] and out["claim_match_retry"] == [1, 0] and out["claim_empty_queue"] == [0, 0]
    for n in ("other_feats", "other_nb", "other_nb_longer", "one_ustart", "one_ulen"):
        assert out["claim_" + n] == [0, 1], n                           # (the head was scored: dropped)
    assert out["claim_head_announced_not_scored"] == [0, 0] and out["claim_not_mine_nothing_worked"] == [0, 0]
    assert out["claim_not_mine_scored_behind"] == [0, 1] and out["claim_not_mine_only_started"] == [0, 1]
    assert out["claim_not_mine_scored_retry"] == [0, 0] and out["claim_not_mine_only_started_retry"] == [0, 0]
    # place: pipe resumed discard unbank bank s0
    p = {n[6:]: o for n, o in out.items() if n.startswith("place_")}
    assert p["nb_eq_B"] == [1, 0, 0, 0, 0, 0] and p["nb_eq_B_plus_1"] == [0, 0, 0, 0, 0, 0]
    assert p["odd_streams_nb_eq_B"][0] == 1 and p["odd_streams_nb_eq_B_plus_1"][0] == 0 and p["odd_streams_bank_1"] == [1, 0, 0, 0, 1, 3]
    assert p["one_stream"][0] == 0 and p["pipeline_off"][0] == 0 and p["lazy"][0] == 0
    assert p["chunked_scored"][2:4] == [1, 0] and p["chunked_started"][2:4] == [1, 0] and p["chunked_nothing_scored"][2:4] == [0, 0]
    assert p["outside_banks_batch_started"] == [0, 0, 0, 1, 0, 0] and p["pipeline_off_started"][3] == 1 and p["outside_banks_nothing_started"][3] == 0
    assert p["bank_0_held"][4:] == [1, 4] and p["bank_1_held"][4:] == [0, 0]
    assert p["resumed_bank_0"] == [1, 1, 0, 0, 0, 0] and p["resumed_bank_1"] == [1, 1, 0, 0, 1, 4]
    assert p["mine_not_started"] == [1, 0, 0, 0, 1, 4] and p["mine_started_but_outside_banks"][:2] == [0, 0]
    # tables
    assert out["need_fits"] == [48, 0] and out["need_one_float_short"] == [54, 1]
    assert out["need_above_from_this_wave"] == [135, 1] and out["need_above_from_a_queued_batch"] == [135, 1] and out["need_chunked"] == [120, 0]
    assert out["take_announced_table"] == [1, 0] and out["take_all_three_held"] == [0, 1] and out["take_chunked_whatever_is_held"] == [0, 0]
    # free_table: every foreground value and set of scored tables; FG_BOTH matches no table
    for fg in (FG_BOTH, -1, 0, 1, 2):
        for held in ((), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
            free = [t for t in range(3) if t != fg and t not in held]
            assert out["free_table_fg%d_held%s" % (fg, "".join(map(str, held)) or "_none")] == [free[0] if free else -1]
    assert out["free_table_fg-2_held_none"] == [0]
    # announce: admitted n_chunks enqueued queue_size position
    assert out["announce_nb_0"] == [0, 0, 0, 0, -1] and out["announce_nb_max_plus_1"] == [0, 0, 0, 0, -1] and out["announce_nb_max"] == [1, 1, 1, 1, 0]
    assert out["announce_fourth_entry"] == [0, 0, 0, 3, -1] and out["announce_third_entry_back"] == [1, 1, 1, 3, 2] and out["announce_front"] == [1, 1, 1, 3, 0]
    assert out["announce_chunked_plan"] == [1, 3, 0, 0, -1]
    # chunk work: frames n {stream row weight}
    assert out["chunk_zero_length_utterance"] == [12, 3, 0, 0, 5, 1, 5, 0, 2, 5, 7]     # (the empty utterance: a work item of weight 0)
    assert out["chunk_zero_length_in_chunk_1"][:2] == [4, 1]
    assert out["chunk_ends_on_the_boundary"] == [17, 2, 5, 100, 1, 6, 101, 16]           # (16 frames: not in chunk 1; 17: one frame)
    assert out["chunk_resumed_already_at_T"] == [3, 1, 7, 256 + 9, 3] and out["chunk_resumed_beyond_c0"] == [24, 2, 0, 0, 10, 1, 14, 14]
    # (as recorded: a stream already past the chunk's end is a work item of negative weight - no wave can get there, a resumed wave has one chunk)
    assert out["chunk_resumed_beyond_c1"] == [-1, 2, 0, 0, -1, 1, 16, 0]
    # probe split
    assert out["probe_span_128"] == [0] and out["probe_span_129"][0] == 1 and out["probe_nb_1"] == [0] and out["probe_load_scale_known"] == [0]
    assert out["probe_unweighted"] == [0] and out["probe_resumed"] == [0]
    o = out["probe_T_32_and_33"]                                        # 5 items with weights min(w, 32), then those past frame 32
    assert o[:2] == [1, 5] and o[4:17:3] == [32, 32, 32, 0, 31] and o[17:] == [2, 6, 0, 168, 8, 232, 1]
    # background: step bank n {stream row left}
    b = {n[3:]: o for n, o in out.items() if n.startswith("bg_")}
    assert b["first_start"] == [BG_START, 1, 3, 4, 128, 5, 5, 133, 6, 6, 139, 7] and b["first_start_beside_bank_1"][:3] == [BG_START, 0, 3]
    assert b["first_start_table_not_ready"] == [BG_START, -1, 0] and b["first_start_zero_length"][2:] == [2, 4, 0, 0, 5, 0, 4]
    assert b["later_finished_error_running"] == [BG_GO_ON, 1, 1, 6, 139, 4] and b["later_without_heads"] == [BG_GO_ON, 1, 0]
    assert b["load_just_above"] == [BG_NONE, -1, 0] and b["load_at_the_bound"][0] == BG_START
    for n in ("head_only_announced", "head_fills_more_than_a_bank", "head_in_chunks", "pipeline_off", "lazy", "empty_queue", "one_stream"):
        assert b[n][0] == BG_NONE and b[n][2] == 0, n
    assert b["head_fills_a_bank"][0] == BG_START
    # clip rule, reserve, hold-replan
    assert [out["clip_" + n] for n in ("a_quarter", "above_a_quarter", "two_per_stream_left", "less_than_two_per_stream_left")] == [[0], [1], [0], [1]]
    assert out["reserve_rounds_up_to_8"] == [32] and out["reserve_exact_multiple"] == [16] and out["reserve_a_third_at_most"] == [80]
    assert out["reserve_zero_last_wave"] == [0] and out["reserve_as_set"] == [8] and out["reserve_as_set_above_a_third"] == [80]
    assert [out["hold_" + n] for n in ("never_1", "always_0", "auto_a_tenth_exactly", "auto_just_below_a_tenth", "auto_scoring_unknown")] == [[0], [1], [1], [0], [0]]
    # waves: order, n_waves, per wave nb {ustart ulen} nn
    assert out["waves_n_eq_streams_no_sort"][:4] == [0, 1, 2, 1] and out["waves_n_eq_streams_plus_1"][:5] == [1, 3, 2, 0, 2]
    assert out["waves_equal_lengths_keep_index_order"][:5] == [2, 4, 0, 1, 3] and out["waves_partial_last"][8] == 3
    assert out["waves_partial_last"][-2 - 2 * 2 - 1] == 2 and out["waves_partial_last"][-1] == 0
    # load_scale (the doubles' bits)
    bits = lambda v: int.from_bytes(__import__("struct").pack("<d", v), "little")
    assert out["load_first_update"] == [0, bits(2.0)] and out["load_later_update"] == [0, bits(4.0)] and out["load_clamp_low"] == [0, bits(0.25)]
    assert out["load_clamp_high"] == [0, bits(0.5 * (3.0 + 1e5))] and out["load_zero_frames"] == [0, bits(2.5)]
    # scripts: what the sequences reach
    seen = set()
    for name, steps in scripts.items():
        for line, _, o in steps:
            if line.startswith("decode"):
                for w in read_decode(o):
                    seen |= {k for k in ("ok", "mine", "drop", "pipe", "resumed", "drop_scored") if w[k]} | ({"failed"} if not w["ok"] else set())
                    seen |= {"bank 1"} if w["pipe"] and w["bank"] == 1 else set()
                    for c in w["chunks"]:
                        seen |= {"bg step %d" % c["bg_step"], "launched %d" % c["launched"]} | ({"bg work"} if c["n_bg"] else set())
    assert seen >= {"ok", "mine", "drop", "pipe", "resumed", "drop_scored", "failed", "bank 1", "bg step 0", "bg step 1", "bg work",
                    "launched 0", "launched 1", "launched 2"}, seen
    first = [read_decode(o) for l, _, o in scripts["scores_ahead_of_the_search"] if l.startswith("decode")]
    # (the `ahead` argument of the GPU test's decode(): prefetched or not, decode by decode)
    assert [w[0]["mine"] for w in first] == [0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    waves = [read_decode(o) for l, _, o in scripts["scores_ahead_in_waves"] if l.startswith("decode")]
    assert [sum(w["mine"] for w in d) for d in waves] == [2, 2, 1]       # waves 2 and 3 of 3; the batch that rode on the last wave
    two = [read_decode(o)[0] for l, _, o in scripts["two_batches_in_flight"] if l.startswith("decode")]
    assert [w["mine"] for w in two[:8]] == [0, 1, 1, 1, 1, 1, 0, 0] and sum(w["resumed"] for w in two[1:6]) >= 3


def test_ahead_driver_under_sanitizers(lines, outputs, tmp_path_factory):
    """every line once more through the driver built with -fsanitize=address,undefined: the same output, nothing reported"""
    single, scripts = outputs
    driver = build_driver(str(tmp_path_factory.mktemp("ahead_san") / "ahead_driver_san"), ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert run_driver(driver, lines) == [o for _, _, o in single.values()] + [o for steps in scripts.values() for _, _, o in steps]
