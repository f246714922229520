"""The decisions of the slot pipeline (juicer_amd/csrc/jd_pipe.h: the record of a stream's mailbox, the setting, sizing, announcing, the pump's
harvest / refill / scoring, handing back, the drain) on the CPU: tests/pipe_driver.cpp, compiled with plain g++, is held to
tests/golden/pipe_golden.json - what the lines of jd_host_resident.h that jd_pipe.h replaced made of the same inputs, recorded from the commit
named in the file - integer by integer; and after every step of a script the state is checked for what must always hold of it.

Kept as recorded, odd as they look: a zero-length utterance gets one command with T = 0 that both begins and ends it (harvest_through_zero_length,
script three_batches_two_slots); a drain leaves piece_turn, serial0 and frames_done as they are (the next start sets the last two; the turn only
says which of two idle events is used first); a slot that failed is "through" and exported by the kernel whatever its report says of an export
(harvest_error_and_exported); JD_PIPE_PIECE applies with JD_PIPE_DECOUPLE=0 too (size_decouple_0_piece_256)."""
import json
import os
import re

import pytest

from pipe_cases import (COLLECT, HANDLED, NOT_THIS_WAY, QUEUED, RC_FULL, RC_KEEPS_ENDING, RC_LOST, RC_OK, RC_STUCK, RUNNING, SET_DEPTH, SET_DEVICE,
                        SET_NOT_WITH, SET_OK, SET_SLOTS, THROUGH, WAITING, build_driver, read_step, run_driver, script_cases, single_cases)

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "pipe_golden.json")) as f:
        doc = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{7,40}", doc["commit"]) and "HIP call" in doc["how"]
    return doc


@pytest.fixture(scope="module")
def lines(golden):
    """the driver's input: every single decision, then every script - the lines of pipe_cases.py, which are the lines the golden was recorded for"""
    single, scripts = single_cases(), script_cases()
    assert [(c["name"], c["line"]) for c in golden["single"]] == single
    assert [(s["name"], s["lines"]) for s in golden["scripts"]] == scripts
    return [l for _, l in single] + [l for _, ls in scripts for l in ls]


@pytest.fixture(scope="module")
def outputs(golden, lines, tmp_path_factory):
    """({name: (line, recorded, output)} of the single decisions, {name: [(line, recorded, output)]} of the scripts)"""
    out = run_driver(build_driver(str(tmp_path_factory.mktemp("pipe") / "pipe_driver")), lines)
    single = {c["name"]: (c["line"], c["out"], o) for c, o in zip(golden["single"], out)}
    at, scripts = len(golden["single"]), {}
    for s in golden["scripts"]:
        scripts[s["name"]] = list(zip(s["lines"], s["out"], out[at:at + len(s["lines"])]))
        at += len(s["lines"])
    assert at == len(out)
    return single, scripts


def test_single_decisions_match_recorded(outputs):
    single, _ = outputs
    assert len(single) >= 90 and len({l for l, _, _ in single.values()}) == len(single)      # no case twice
    bad = [(name, line, want, got) for name, (line, want, got) in single.items() if want != got]
    for b in bad:
        print(*b)
    assert not bad


def test_scripts_match_recorded(outputs):
    _, scripts = outputs
    assert len(scripts) >= 15
    bad = [(name, line, want, got) for name, steps in scripts.items() for line, want, got in steps if want != got]
    for b in bad:
        print(*b)
    assert not bad


def check_state(s, where):
    """what must always hold of the pipeline's bookkeeping"""
    q = s["q"]
    assert len(q) <= s["K"], where                                      # the queue never exceeds the depth
    tables = [b["table"] for b in q]
    assert len(tables) == len(set(tables)), where                       # no two batches share a table ...
    assert [int(t in tables) for t in range(s["K"])] == s["table_used"], where   # ... and table_used says exactly which are held
    for b in q:
        states = [u["state"] for u in b["u"]]
        assert b["n_done"] == states.count(THROUGH), where
        assert b["next"] == len(states) - states.count(QUEUED), where
        assert 0 <= b["n_kexport"] <= b["n_done"] <= b["next"] <= b["n"], where
        assert b["rows_scored"] <= b["rows"], where
        assert sorted(b["order"]) == list(range(b["n"])), where
        assert [states[o] != QUEUED for o in b["order"]] == [k < b["next"] for k in range(b["n"])], where   # taken in order
    for k in range(1, len(q)):                                          # no batch has rows scored while one in front of it is short of its last row
        assert not (q[k]["rows_scored"] > 0 and any(f["rows_scored"] < f["rows"] for f in q[:k])), where
    assert 0 <= s["piece_out"] <= s["max_out"], where
    running = set()
    for i, sl in enumerate(s["slots"]):
        if sl["batch_id"] < 0:
            continue
        k = sl["batch_id"] - s["serial0"]
        assert 0 <= k < len(q), where                                   # an occupied slot points into the queue ...
        u = q[k]["u"][sl["utt"]]
        assert u["state"] == RUNNING and u["slot"] == i, where           # ... at an utterance that is running, and that names this slot
        assert (k, sl["utt"]) not in running, where
        running.add((k, sl["utt"]))
    n_running = sum(u["state"] == RUNNING for b in q for u in b["u"])
    assert n_running == len(running), where                             # no utterance runs on two slots, none on none


def test_state_invariants_after_every_script_step(outputs):
    _, scripts = outputs
    n_steps = n_commands = 0
    for name, steps in scripts.items():
        prev, posted = None, {}                                          # posted: (batch serial, its features, utterance) -> T of its last command
        for line, _, o in steps:
            s = read_step(o)
            where = (name, line)
            n_steps += 1
            check_state(s, where)
            for kind, e in s["log"]:
                if kind != "command":
                    continue
                n_commands += 1
                sl = s["slots"][e["slot"]]
                if sl["batch_id"] < 0:                                  # (the step went on to drain everything: nothing left to hold the command to)
                    assert not s["pipe_on"], where
                    continue
                k = sl["batch_id"] - s["serial0"]
                b, ui = s["q"][k], sl["utt"]
                u = b["u"][ui]
                assert e["T"] <= u["T"], where                          # never beyond the utterance
                assert e["row_slot"] == u["row0"], where
                key = (name, sl["batch_id"], b["feats"], ui)
                if e["init"]:
                    was_dirty = prev["slots"][e["slot"]]["dirty"] if prev and prev["have_pipe"] and prev["pipe_on"] and e["slot"] < len(prev["slots"]) else 0
                    assert not was_dirty and not sl["dirty"], where      # no dirty slot is ever given an utterance
                    assert b["rows_scored"] == b["rows"], where          # none is given out from a batch whose scoring is not enqueued to its last row
                    grown = e["T"] if key not in posted else e["T"] - posted[key]   # (a re-posted init, behind a collection, grows by nothing)
                else:
                    grown = e["T"] - posted.get(key, e["T"])
                assert 0 <= grown <= s["chunk"], where                  # at most a chunk at a time
                posted[key] = e["T"]
                ends = e["T"] == u["T"]
                assert (e["vslot"] >= 0) == bool(ends and s["decouple"]), where   # a result slot exactly on the command that ends it, under decouple
                if e["vslot"] >= 0:
                    assert e["vslot"] == b["table"] * s["max_batch"] + ui, where
            prev = s
    assert n_steps >= 250 and n_commands >= 150


def test_cases_cover_what_they_must(outputs):
    single, scripts = outputs
    out = {n: o for n, (_, _, o) in single.items()}
    # setting: verdict depth slots
    for slots, depth in ((1, 8), (32, 8), (63, 8), (64, 8), (191, 8), (192, 8), (256, 10), (959, 31), (960, 32), (1024, 32)):
        assert out["setting_default_depth_%d_slots" % slots] == [SET_OK, depth, slots]
        assert depth == min(32, max(8, slots // 32 + 2))
    assert out["setting_default_slots"] == [SET_OK, 8, 48]
    assert [out["setting_depth_%s" % d][0] for d in ("1", "2", "32", "33", "negative")] == [SET_DEPTH, SET_OK, SET_OK, SET_DEPTH, SET_DEPTH]
    assert out["setting_slots_eq_streams"][0] == SET_OK and out["setting_slots_above_streams"][0] == SET_SLOTS and out["setting_slots_negative"][0] == SET_SLOTS
    assert out["setting_slots_fill_device"][0] == SET_OK and out["setting_slots_above_device"][0] == SET_DEVICE
    assert out["setting_lazy"][0] == SET_NOT_WITH and out["setting_hybrid"][0] == SET_NOT_WITH
    assert out["setting_depth_checked_first"][0] == SET_DEPTH and out["setting_slots_before_device"][0] == SET_SLOTS and out["setting_device_before_lazy"][0] == SET_DEVICE
    # size: K max_batch n_slots chunk decouple max_out piece_rows table_rows vslots
    z = {n[5:]: o for n, o in out.items() if n.startswith("size_")}
    assert z["no_knobs"] == [8, 8, 16, 128, 1, 2, 5120, 3072, 64] and z["nothing_planned"][6] == 6144
    assert z["slots_set"][2] == 5 and z["slots_eq_streams"][2] == 16 and z["slots_above_streams"][2] == 16
    assert [z["chunk_%d" % v][3] for v in (0, 15, 16, 300)] == [128, 128, 16, 300]
    assert z["decouple_0"][4:7] == [0, 1, 6144] and z["decouple_1"][4:7] == [1, 2, 5120] and z["decouple_0_piece_256"][4:7] == [0, 1, 256]
    assert [z["piece_%d" % v][6] for v in (127, 128, 255, 256)] == [5120, 128, 128, 256] and z["piece_1000_nothing_planned"][6] == 896
    assert z["rows_64_whole_tiles"][7] == 1152 and z["rows_65"][7] == 1280 and z["rows_0"][7] == 1024 and z["one_utterance"][:2] + z["one_utterance"][8:] == [2, 2, 4]
    # the piece bounds: lo hi groups, on both sides of the switch to 16-state tiles
    assert out["bounds_960_states_small_tiles"] == [4096, 8192, 60] and out["bounds_961_states"] == [8192, 8192, 16]
    assert out["bounds_toy"] == [4096, 8192, 1] and out["bounds_9000_states"] == [4096, 8192, 141] and out["bounds_2000_states"] == [4096, 8192, 32]
    # announcing
    assert [out[n] for n in ("takes", "takes_not_pipe_mode", "takes_lazy", "takes_partial", "takes_hybrid", "takes_no_utterance")] == [[1], [0], [0], [0], [0], [0]]
    assert [out[n] for n in ("outgrown_fits_exactly", "outgrown_one_utterance_more", "outgrown_one_row_more", "full_one_free", "full")] == [[0], [1], [1], [0], [1]]
    assert out["enqueue_first_table"] == [0, 0, 5, 1, 0] and out["enqueue_hole_in_the_middle"] == [1, 1152, 1157, 1, 0]
    assert out["enqueue_hole_in_front"][0] == 0 and out["enqueue_last_table"][:3] == [2, 2304, 2309]
    assert out["enqueue_ties_keep_index_order"][6:] == [1, 3, 0, 2, 4]                     # stable: longest first, equal lengths by index
    assert out["enqueue_zero_length_and_one_frame"] == [1, 1152, 1155, 1155, 1156, 0, 2, 1, 3]
    # harvest: the three actions
    h = {n[8:]: read_step(o) for n, o in out.items() if n.startswith("harvest_") and not n.startswith("harvest_many")}
    kinds = lambda s: [k for k, _ in s["log"]]
    cmd = lambda s: [e for k, e in s["log"] if k == "command"][0]
    for n in ("collect", "collect_one_short", "collect_short_of_the_end"):
        assert kinds(h[n]) == ["collect", "bump", "command"] and h[n]["slots"][0]["batch_id"] == 0, n
    assert cmd(h["collect"])["T"] == 32 and cmd(h["collect_short_of_the_end"])["vslot"] == -1     # (as recorded: the harvest test made the command without one)
    for n, T, v in (("next_fr_at_T_posted", 32, -1), ("next_ends_exactly", 40, 9), ("next_ends_one_below", 39, -1), ("next_ends_one_above", 40, 9),
                    ("next_fr_at_UT_minus_1", 40, 9), ("next_ends_exactly_coupled", 40, -1), ("next_chunk_128", 256, -1)):
        assert kinds(h[n]) == ["command"] and (cmd(h[n])["T"], cmd(h[n])["vslot"], cmd(h[n])["init"], cmd(h[n])["row_slot"]) == (T, v, 0, 2309), n
    for n, kexport, dirty in (("through_exported", 0, 0), ("through_not_exported", 1, 0), ("through_coupled", 1, 0), ("through_exported_coupled", 0, 0),
                              ("through_zero_length", 0, 0), ("through_one_frame", 0, 0), ("error_in_the_middle", 1, 1), ("error_at_the_end", 1, 1),
                              ("error_and_exported", 1, 1)):
        s = h[n]
        assert kinds(s) == (["kexport"] if kexport else []), n
        assert s["slots"][0] == {"batch_id": -1, "utt": 1, "dirty": dirty, "kexport": kexport} and s["q"][0]["u"][1]["state"] == THROUGH, n
        assert s["q"][0]["n_kexport"] == kexport and s["utts_through"] == 1 and (not kexport or s["log"][0][1]["pairs"] == [(0, 9)]), n
    for n, launches in ((63, [63]), (64, [64]), (65, [64, 1]), (129, [64, 64, 1])):                 # the 65th export: the list went out full
        assert [e["n"] for k, e in read_step(out["harvest_many_%d" % n])["log"] if k == "kexport"] == launches
    # scripts: what the sequences reach
    seen, rcs = set(), set()
    for name, steps in scripts.items():
        prev = None
        for line, _, o in steps:
            s = read_step(o)
            rcs.add(s["rc"])
            ks = kinds(s)
            free_before = sum(1 for sl in prev["slots"] if sl["batch_id"] < 0 and not sl["dirty"]) if prev and prev["pipe_on"] else 0
            inits = [e for k, e in s["log"] if k == "command" and e["init"]]
            bumped = {e["slot"] for k, e in s["log"] if k == "bump"}
            if inits and prev and prev["pipe_on"]:
                queued_before = sum(u["state"] == QUEUED for b in prev["q"] for u in b["u"])
                seen.add("fewer free slots than utterances" if len(inits) < queued_before else "more free slots than utterances")
                for e in inits:
                    k = s["slots"][e["slot"]]["batch_id"] - s["serial0"]
                    if 0 <= k < len(s["q"]) and e["slot"] < len(prev["slots"]):
                        kex = prev["slots"][e["slot"]]["kexport"] or any(e["slot"] == sl for kk, x in s["log"] if kk == "kexport" for sl, _ in x["pairs"])
                        seen.add("scored %d kexport %d bump %d" % (s["q"][k]["scored"], kex, e["slot"] in bumped))
                if len({s["slots"][e["slot"]]["batch_id"] for e in inits}) > 1:
                    seen.add("refill crosses into the next batch")
            if prev and prev["pipe_on"] and any(sl["dirty"] and sl["batch_id"] < 0 for sl in prev["slots"]) and inits:
                seen.add("dirty slot skipped")
            if prev and prev["pipe_on"] and prev["q"] and prev["q"][0]["next"] < prev["q"][0]["n"] and prev["q"][0]["rows_scored"] < prev["q"][0]["rows"] and free_before:
                seen.add("head not yet scored to its last row")
            pieces = [e for k, e in s["log"] if k == "piece"]
            for e in pieces:
                seen.add("piece %s" % ("below" if e["rows"] < s["piece_rows"] else "at") + (" last" if e["batch_event"] else ""))
            if len({e["table"] for e in pieces}) > 1:
                seen.add("two batches scored in one call")
            if len(pieces) > 1 and pieces[0]["event"] != pieces[1]["event"]:
                seen.add("second piece behind the first")
            seen |= {"max_out %d" % s["max_out"]} if pieces else set()
            seen |= {"piece_turn %d" % s["piece_turn"]} if "query_piece" in ks else set()
            if "query_table" in ks:
                seen.add("table event asked, answer %d" % max(e["answer"] for k, e in s["log"] if k == "query_table"))
            if inits and "query_table" not in ks and s["decouple"]:
                seen.add("table event not asked once scored")
            seen |= {k for k in ks if k in ("collect", "wipe", "sync", "kexport")}
            seen |= {"stop lost %d" % e["lost"] for k, e in s["log"] if k == "stop"}
            if s["status"] == HANDLED:
                seen.add("pop with a batch behind" if s["pipe_on"] else "pop of the last batch")
            if line.startswith("decode") and s["status"] == NOT_THIS_WAY and s["rc"] == RC_OK:
                seen.add("not the announced batch")
            if prev and any(sl["dirty"] for sl in prev["slots"]) and not s["pipe_on"] and any(st["dirty"] for st in s["streams"]):
                seen.add("drain carries dirt to the streams")
            if any(e["T"] == 0 and e["init"] for k, e in s["log"] if k == "command"):
                seen.add("zero-length utterance")
            seen |= {"decouple %d" % s["decouple"]} if s["have_pipe"] else set()
            prev = s
    want = {"fewer free slots than utterances", "more free slots than utterances", "refill crosses into the next batch", "dirty slot skipped",
            "head not yet scored to its last row", "scored 0 kexport 0 bump 1", "scored 0 kexport 1 bump 1", "scored 1 kexport 0 bump 0", "scored 1 kexport 1 bump 1",
            "piece below last", "piece at", "piece at last", "two batches scored in one call", "second piece behind the first", "max_out 1", "max_out 2",
            "piece_turn 0", "piece_turn 1", "table event asked, answer 0", "table event asked, answer 1", "table event not asked once scored", "collect", "wipe",
            "sync", "kexport", "stop lost 0", "stop lost 1", "pop with a batch behind", "pop of the last batch", "not the announced batch",
            "drain carries dirt to the streams", "zero-length utterance", "decouple 0", "decouple 1"}
    assert seen >= want, sorted(want - seen)
    assert rcs == {RC_OK, RC_LOST, RC_STUCK, RC_KEEPS_ENDING, RC_FULL}
    last = lambda name: read_step(scripts[name][-1][2])
    assert last("kernel_keeps_ending")["rc"] == RC_KEEPS_ENDING and [read_step(o)["rc"] for _, _, o in scripts["kernel_keeps_ending"][2:-1]] == [RC_OK] * 3
    w = [read_step(o) for _, _, o in scripts["watchdog_30_s"]]                             # 30 s exactly is not yet; a nanosecond more is
    assert [s["rc"] for s in w[2:10]] == [RC_OK] * 7 + [RC_STUCK] and all(s["status"] == WAITING for s in w[2:9]) and w[7]["frames_done"] == 50
    assert [read_step(o)["rc"] for _, _, o in scripts["watchdog_reports_are_no_progress"]][-2:] == [RC_OK, RC_STUCK]
    n = [read_step(o) for l, _, o in scripts["not_the_announced_batch"] if l.startswith("decode")]
    assert [s["status"] for s in n] == [NOT_THIS_WAY] * 6 + [WAITING] and all(not s["pipe_on"] for s in n[:6])     # (the last: the announced one)
    # a stop and restart in the middle with one command unanswered, decoupled and coupled: the slot's rest is posted again like behind a
    # collection - a new ready number, the same T and rows, and what the lost command said of init and of the result slot said again
    for name, decouple in (("quiesce_with_one_command_unanswered", 1), ("quiesce_with_one_command_unanswered_coupled", 0),
                           ("quiesce_before_the_first_report", 1), ("quiesce_before_the_first_report_coupled", 0)):
        steps = [(l, read_step(o)) for l, _, o in scripts[name]]
        at = [k for k, (l, s) in enumerate(steps) if l.startswith("quiesce") and any(st["T_done"] < st["T_posted"] and not st["busy"] for st in s["streams"])][0]
        stopped, back = steps[at][1], steps[at + 1][1]
        assert stopped["rc"] == RC_OK and stopped["decouple"] == decouple and stopped["max_out"] == 1 + decouple and not stopped["res_on"], name
        assert ("stop", {"lost": 0}) in stopped["log"] and kinds(back)[0] == "start" and back["res_on"], name
        slot = [k for k, st in enumerate(stopped["streams"]) if st["T_done"] < st["T_posted"]][0]
        lost = [e for l, s in steps[:at] for k, e in s["log"] if k == "command" and e["slot"] == slot][-1]
        i = kinds(back).index("collect")
        (_, c), (_, b), (_, again) = back["log"][i:i + 3]
        assert c["slot"] == b["slot"] == again["slot"] == slot and kinds(back)[i:i + 3] == ["collect", "bump", "command"], name
        assert [again[k] for k in ("T", "row_slot", "init", "vslot")] == [lost[k] for k in ("T", "row_slot", "init", "vslot")], name
        assert again["ready_id"] == b["id"] and again["seq"] == 1, name      # (both sides' numbers began again)
        assert (again["vslot"] >= 0) == bool(decouple and again["T"] == stopped["q"][0]["u"][stopped["slots"][slot]["utt"]]["T"]), name
        if "first_report" in name:
            assert again["init"] == 1 and stopped["streams"][slot]["init_pending"] == 1, name
    for name in ("quiesce_loses_a_workgroup", "quiesce_loses_a_workgroup_coupled"):
        s = [read_step(o) for l, _, o in scripts[name] if l.startswith("quiesce")][0]
        assert s["rc"] == RC_LOST and ("stop", {"lost": 1}) in s["log"] and s["streams"][1]["dirty"] == 1, name
    runs_coupled = {n for n, steps in scripts.items() if read_step(steps[1][2])["decouple"] == 0}
    assert runs_coupled >= {"three_batches_two_slots_coupled", "quiesce_with_one_command_unanswered_coupled", "error_in_one_slot_coupled"}
    assert COLLECT == 0


def test_pipe_driver_under_sanitizers(lines, outputs, tmp_path_factory):
    """every line once more through the driver built with -fsanitize=address,undefined: the same output, nothing reported"""
    single, scripts = outputs
    driver = build_driver(str(tmp_path_factory.mktemp("pipe_san") / "pipe_driver_san"), ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert run_driver(driver, lines) == [o for _, _, o in single.values()] + [o for steps in scripts.values() for _, _, o in steps]
