"""The sizes and the layout of the stream arenas and of a wave's likelihood tables (juicer_amd/csrc/jd_arena.h) on the CPU:
tests/arena_driver.cpp, compiled with plain g++, is held to tests/golden/arena_golden.json - what the lines of ensure_arenas_try and
plan_wave that jd_arena.h replaced made of the same inputs, recorded from the commit named in the file - integer by integer, and the same
outputs are checked for what legal capacities, a legal layout and a legal wave plan are.

The fit to a cached slab: the recorded lines do NOT always end with arenas that fit the slab.  Their three passes scale the SHARE the
automatic capacities are picked from, so what is not picked from the share - a capacity the caller set, an arena at its ceiling or its
floor, the per-arc and per-state words - stays, and the arenas come out above the slab again.  The cases where they do are named in
SLAB_MISSED below and kept as recorded (the slab is then freed and a new one allocated: slower set-up, same results).  The third pass is
reachable for the same reason: "slab_paths_set_need_1pc_above" needs it and fits with it.

wave_layout's "more than 2^31 frames in one chunk" needs three utterances of 0x3fffffff frames; it is reached before any table of rows
is made, so case "err_chunk_rows" runs it.
"""
import json
import os
import re

import pytest

from arena_cases import CAPS_OUT, PIECES, build_driver, caps_line, run_driver, wave_line

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "juicer_amd", "csrc")
# scaled to the cached slab and still above it at the end, as recorded (see above)
SLAB_MISSED = ["slab_auto_B2_need_1pc_above", "slab_auto_B2_need_5_9pc_above", "slab_paths_set_need_5_9pc_above",
               "slab_paths_items_set_need_1pc_above", "slab_paths_items_set_need_5_9pc_above", "slab_ceilings_B1_need_1pc_above",
               "slab_ceilings_B1_need_5_9pc_above"]


def limits(i, sizes):
    """the addressing limits of records and items"""
    rec_bytes = sizes["rec_bytes_small"] if i["max_n"] <= 5 else sizes["rec_bytes_large"]
    return (0xe0000000 // (2 * rec_bytes)) & ~63, 0xe0000000 // 64


def budget(i, sizes):
    """a stream's share of the memory after its per-arc / per-state tables, as arena_caps' first pass has it (IEEE doubles here as there)"""
    fixed = float(i["n_arcs"]) * 1.0 + float(i["n_states"]) * float(sizes["state_rec"]) + 2.0 * i["Fc"] * i["n_gmm"] * 4
    return max(0.0, 1.0 * float.fromhex(i["mem_fraction"]) * float(i["free_bytes"] + i["cached_bytes"]) / i["B"] - fixed)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "arena_golden.json")) as f:
        doc = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{7,40}", doc["commit"])
    return doc


@pytest.fixture(scope="module")
def lines(golden):
    """the driver's input: every capacity case, then every wave case"""
    return [caps_line(dict(golden["caps_defaults"], **c["in"]), golden["sizes"]) for c in golden["caps_cases"]] + \
        [wave_line(dict(golden["wave_defaults"], **c["in"])) for c in golden["wave_cases"]]


@pytest.fixture(scope="module")
def outputs(golden, lines, tmp_path_factory):
    """([(name, input, recorded, output)] of the capacity cases, the same of the wave cases)"""
    out = run_driver(build_driver(str(tmp_path_factory.mktemp("arena") / "arena_driver")), lines)
    n = len(golden["caps_cases"])
    caps = [(c["name"], dict(golden["caps_defaults"], **c["in"]), c["out"], o) for c, o in zip(golden["caps_cases"], out[:n])]
    waves = [(c["name"], dict(golden["wave_defaults"], **c["in"]), c["out"], o) for c, o in zip(golden["wave_cases"], out[n:])]
    return caps, waves


def test_arena_caps_match_recorded(outputs):
    caps, _ = outputs
    assert len(caps) >= 60
    assert len(caps) == len({json.dumps(i, sort_keys=True) for _, i, _, _ in caps})   # no case twice
    for name, _, want, got in caps:
        if want != got:
            print(name, "recorded", want, "now", got)
    assert not [name for name, _, want, got in caps if want != got]


def test_wave_layout_matches_recorded(outputs):
    _, waves = outputs
    assert len(waves) >= 30
    assert len(waves) == len({json.dumps(i, sort_keys=True) for _, i, _, _ in waves})
    assert not [name for name, _, want, got in waves if want != got]
    utt = {name: got[1] for name, _, _, got in waves}                  # the utterance the message names
    assert utt["err_negative_length"] == 1 and utt["err_length_2_30"] == 2


def test_arena_sizes_are_the_builds(golden):
    """the sizes the golden was recorded with are the literals jd_device.hip holds its structs to, and the constants those of the kernels"""
    z = golden["sizes"]

    def define(header, name):
        with open(os.path.join(CSRC, header)) as f:
            m = re.search(r"^#define %s (\d+)\b" % name, f.read(), re.M)
        assert m, (header, name)
        return int(m.group(1))

    with open(os.path.join(CSRC, "jd_device.hip")) as f:
        src = f.read()
    for text in ("RecLayout<3>::REC_BYTES == %d && RecLayout<6>::REC_BYTES == %d" % (z["rec_bytes_small"], z["rec_bytes_large"]),
                 "sizeof(PathRec) == %d && sizeof(Tok) == %d && sizeof(int4) == %d && sizeof(StateRec) == %d" %
                 (z["path_rec"], z["tok"], z["item"], z["state_rec"]),
                 "sizeof(GcState) == 4 * %d" % z["gc_words"],
                 "TOT_N == %d && MAXW == %d && HIST_MAX_BINS == %d && SW == %d" % (z["tot_n"], z["maxw"], z["hist_bins"], z["sw"])):
        assert text in src, text
    assert z["sw"] == define("jd_search.h", "SW") and z["maxw"] == 64 * z["sw"] and z["hist_bins"] == define("jd_device.hip", "HIST_MAX_BINS")
    assert golden["wave_defaults"]["tile"] == define("jd_score_plan.h", "GMM_ROWS2")
    assert all("tile" not in c["in"] for c in golden["wave_cases"])


def test_arena_caps_and_layout_are_legal(golden, outputs):
    caps, _ = outputs
    z = golden["sizes"]
    n_ok = 0
    for name, i, _, o in caps:
        c = dict(zip(CAPS_OUT, o))
        off = o[len(CAPS_OUT):len(CAPS_OUT) + len(PIECES)]
        lim_rec, lim_item = limits(i, z)
        if c["status"] != 0:
            assert o[len(CAPS_OUT) + len(PIECES):] == [lim_rec, lim_item], name
            assert c["cap_slots"] > lim_rec or c["cap_items"] > lim_item or c["cap_paths"] > 0x7fffff00, name
            continue
        n_ok += 1
        assert len(o) == len(CAPS_OUT) + len(PIECES), name
        assert c["cap_slots"] % 64 == 0 and c["cap_slots"] >= 64 * z["sw"], name
        assert c["cap_items"] >= 64 * z["sw"], name
        assert c["cap_new"] == min(4 * c["cap_items"], 0x7fffff00), name
        assert c["cap_slots"] <= lim_rec and c["cap_items"] <= lim_item and 1 <= c["cap_paths"] <= 0x7fffff00, name
        # (what the limits are for: both halves of the record and item arenas within 32-bit byte offsets)
        rec_bytes = z["rec_bytes_small"] if i["max_n"] <= 5 else z["rec_bytes_large"]
        assert 2 * c["cap_slots"] * rec_bytes <= 0xe0000000 and 4 * c["cap_items"] * z["item"] <= 0xe0000000, name
        for k, v in (("cap_slots", i["cap_slots"]), ("cap_items", i["cap_items"])):   # the caller's are kept but for the rounding
            if v > 0:
                assert c[k] == (max(v, 64 * z["sw"]) & ~63 if k == "cap_slots" else max(v, 64 * z["sw"])), name
        assert i["cap_paths"] <= 0 or c["cap_paths"] == i["cap_paths"], name
        p = c["cap_paths"]
        assert c["gc_threshold"] == max(p // 2, p - max(p // 8, 4 << 20)) and 0 <= c["gc_threshold"] < p, name
        # the layout: the pieces in table order, each of at least one element, rounded up to 256 bytes, nothing between them
        count = {"rec": (2 * c["cap_slots"] * (rec_bytes // 4), 4), "live": (i["n_arcs"], 1), "srec": (i["n_states"], z["state_rec"]),
                 "items": (4 * c["cap_items"], z["item"]), "newl": (c["cap_new"], 8), "dirtyl": (2 * c["cap_new"], 4),
                 "tot": (z["tot_n"] * z["maxw"], 4), "item_end": (z["maxw"], 4), "paths": (p, z["path_rec"]), "paths2": (p, z["path_rec"]),
                 "gc_idx": (p, 4), "gc_state": (z["gc_words"], 4), "hist": (2 * z["hist_bins"], 4)}
        at = 0
        for piece, o_p in zip(PIECES, off):
            assert o_p == at and o_p % 256 == 0, (name, piece)
            n, elem = count[piece]
            at += (max(n, 1) * elem + 255) // 256 * 256
        assert c["bytes"] == at, name
    assert n_ok >= 60


def test_arena_fit_to_the_cached_slab(golden, outputs):
    caps, _ = outputs
    z_sw = golden["sizes"]["sw"]
    outs = {name: (i, dict(zip(CAPS_OUT, o))) for name, i, _, o in caps}
    missed, fitted = [], []
    for name, (i, c) in outs.items():
        assert 1 <= c["passes"] <= 3, name
        all_set = i["cap_slots"] > 0 and i["cap_items"] > 0 and i["cap_paths"] > 0
        if i["cached_bytes"] == 0 or all_set or c["status"] != 0:
            assert c["passes"] == 1, name
        if c["passes"] > 1:
            (fitted if c["bytes"] * i["B"] <= i["cached_bytes"] else missed).append(name)
    assert sorted(missed) == sorted(SLAB_MISSED)
    assert len(fitted) >= 4 and "slab_paths_set_need_1pc_above" in fitted and outs["slab_paths_set_need_1pc_above"][1]["passes"] == 3
    # a slab up to 6 % short is scaled to, one further short or large enough is not
    base = outs["grid_B64_f0_7"][1]
    for name, passes in (("slab_auto_need_1pc_above", 2), ("slab_auto_need_5_9pc_above", 2), ("slab_auto_need_6_1pc_above", 1),
                         ("slab_auto_need_equal", 1), ("slab_auto_need_below", 1), ("slab_auto_need_a_fifth_above", 1), ("slab_tiny_cached", 1)):
        i, c = outs[name]
        assert c["passes"] == passes, name
        assert i["free_bytes"] + i["cached_bytes"] == outs["grid_B64_f0_7"][0]["free_bytes"], name
        if passes == 1:
            assert c == base, name
        else:
            assert all(c[k] < base[k] for k in ("cap_slots", "cap_items", "cap_paths", "bytes")), name
    # a capacity the caller set that a pass raises to 64 SW or rounds down to 64: the next pass counts with the adjusted value (what it
    # leaves of the share goes to the Path records, so counting with the value as set gives other Path arenas)
    for tag in ("items_small_set", "slots_odd_set", "slots_small_set", "slots_odd_items_small_set"):
        for short in ("1pc", "5_9pc"):
            i, c = outs["slab_%s_need_%s_above" % (tag, short)]
            assert c["passes"] == 2 and i["cap_paths"] <= 0, (tag, short)
            adjusted = [(i[k], c[k]) for k in ("cap_slots", "cap_items") if i[k] > 0]
            assert adjusted and all(got != want and got == (max(want, 64 * z_sw) & ~63 if want > 64 * z_sw else 64 * z_sw)
                                    for want, got in adjusted), (tag, short)
    for name in ("slab_all_set_need_1pc_above", "slab_all_set_need_5_9pc_above"):        # nothing to scale
        assert outs[name][1] == outs["set_all"][1] and outs[name][1]["bytes"] * 64 > outs[name][0]["cached_bytes"], name


def test_arena_cases_cover_what_they_must(golden, outputs):
    caps, _ = outputs
    z = golden["sizes"]
    outs = {name: dict(zip(CAPS_OUT, o)) for name, _, _, o in caps}
    ins = {name: i for name, i, _, _ in caps}
    seen = set()
    for name, i, _, o in caps:
        c = dict(zip(CAPS_OUT, o))
        lim_rec, lim_item = limits(i, z)
        rec_bytes = z["rec_bytes_small"] if i["max_n"] <= 5 else z["rec_bytes_large"]
        auto = [i[k] <= 0 for k in ("cap_slots", "cap_items", "cap_paths")]
        seen.add("B %d" % i["B"])
        seen.add("mem_fraction %r" % float.fromhex(i["mem_fraction"]))
        seen.add("%d set" % (3 - sum(auto)))
        if c["status"] != 0:
            seen.add("too large: " + ", ".join(k for k, over in (("slots", c["cap_slots"] > lim_rec), ("items", c["cap_items"] > lim_item),
                                                                  ("paths", c["cap_paths"] > 0x7fffff00)) if over))
            continue
        if i["cached_bytes"] or i["slots_hint"]:
            continue                                                   # (the branches below: of the first pass, without a hint)
        b = budget(i, z)
        seen.add("budget 0" if b == 0.0 else "")
        rec_b, item_b, path_b = 2.0 * rec_bytes, 2.0 * (z["tok"] + z["item"]) + 32.0, 2.0 * z["path_rec"] + 4.0
        if auto[0]:
            hi = min(i["n_arcs"] + 65536, lim_rec)
            share = int(0.5 * b / rec_b)
            seen.add("slots floor 1<<19" if share < 1 << 19 <= hi else "slots ceiling below the floor" if hi < 1 << 19 else
                     "slots share" if share < hi else "slots ceiling n_arcs + 65536" if hi < lim_rec else "slots ceiling lim_rec %d" % rec_bytes)
            slots = max(min(hi, share), min(1 << 19, hi))             # (as picked: rounded down to 64 afterwards)
            assert c["cap_slots"] == slots & ~63, name
        if auto[1]:
            hi = min(max(2 * i["n_arcs"] + 65536, 1 << 21), lim_item)
            share = int(0.2 * b / item_b)
            seen.add("items floor 1<<21" if share < 1 << 21 else "items share" if share < hi else
                     "items ceiling lim_item" if hi == lim_item else "items ceiling 2 n_arcs + 65536")
            assert c["cap_items"] == max(min(hi, share), 1 << 21), name
        if auto[2] and auto[0] and auto[1]:
            hi = min(0x40000000, max(1 << 24, 16 * i["n_arcs"]))
            left = b - float(slots) * rec_b - float(c["cap_items"]) * item_b
            share = int(max(0.3 * b, left) / path_b)
            seen.add("paths floor 1<<21" if share < 1 << 21 else "paths share" if share < hi else "paths ceiling 0x40000000" if hi == 0x40000000 else
                     "paths ceiling 1<<24" if hi == 1 << 24 else "paths ceiling 16 n_arcs")
            seen.add("paths take what is left" if left > 1.5 * 0.3 * b else "paths take 30 %" if 0.3 * b > left else "")
            assert c["cap_paths"] == max(min(hi, share), 1 << 21), name
        if not auto[0] and i["cap_slots"] % 64:
            seen.add("set slots no multiple of 64")
        if not all(auto) and not any(auto) and i["cap_slots"] < 64 * z["sw"] and i["cap_items"] < 64 * z["sw"]:
            seen.add("all set, below 64 SW")
    want = ["B 1", "B 2", "B 64"] + ["mem_fraction %r" % f for f in (0.7, 0.35, 0.175, 0.0875)] + ["%d set" % n for n in range(4)] + [
        "too large: slots", "too large: items", "too large: paths", "budget 0", "slots floor 1<<19", "slots ceiling below the floor", "slots share",
        "slots ceiling n_arcs + 65536", "slots ceiling lim_rec 80", "slots ceiling lim_rec 144", "items floor 1<<21", "items share",
        "items ceiling lim_item", "items ceiling 2 n_arcs + 65536", "paths floor 1<<21", "paths share", "paths ceiling 0x40000000",
        "paths ceiling 1<<24", "paths ceiling 16 n_arcs", "paths take what is left", "paths take 30 %", "set slots no multiple of 64",
        "all set, below 64 SW"]
    assert [w for w in want if w not in seen] == []
    # the 30 % share against what records and items leave, with a set capacity as well: a large record arena leaves less than 30 %
    assert outs["set_slots_big_30_share_wins"]["cap_paths"] < outs["set_slots"]["cap_paths"]
    # slots_hint: below, equal to and above the picked value, and above lim_rec
    picked = outs["hint_base"]["cap_slots"]
    assert picked % 64 == 0 and ins["hint_below"]["slots_hint"] == picked - 1 and ins["hint_equal"]["slots_hint"] == picked
    assert outs["hint_below"] == outs["hint_equal"] == outs["hint_base"]
    assert picked < ins["hint_above"]["slots_hint"] < limits(ins["hint_above"], z)[0]
    assert outs["hint_above"]["cap_slots"] == ins["hint_above"]["slots_hint"] & ~63 > picked
    for name in ("hint_above_lim_rec", "hint_above_lim_rec_144"):
        assert ins[name]["slots_hint"] > limits(ins[name], z)[0] == outs[name]["cap_slots"], name
    # gc_threshold on both sides of the two places where its max terms cross
    for p in (8 << 20, 32 << 20):
        assert {d for d in (-8, -2, 0, 2, 8) if "gc_paths_%d" % (p + d) in outs} >= ({-2, 0, 2} if p == 8 << 20 else {-8, 0, 8})
    # every limit itself is a legal capacity, one more is not
    for name in ("at_limit_slots_80", "at_limit_slots_144", "at_limit_items", "at_limit_paths"):
        assert outs[name]["status"] == 0, name
    for name in ("too_large_slots_80", "too_large_slots_144", "too_large_items", "too_large_paths"):
        assert outs[name]["status"] == 1, name


def test_wave_layout_is_legal(outputs):
    _, waves = outputs
    n_ok = 0
    for name, i, _, o in waves:
        if o[0] != 0:
            continue
        n_ok += 1
        nb, Fc, n_chunks, maxT, max_rows, n_rows_all = o[2:8]
        tile = i["tile"]
        rest = o[8:]
        T, rest = rest[:nb], rest[nb:]
        chunk_row0, rest = rest[:n_chunks + 1], rest[n_chunks + 1:]
        row_off, rest = rest[:n_chunks * nb], rest[n_chunks * nb:]
        chunk_rows, row_src = rest[:n_chunks], rest[n_chunks:]
        assert len(row_src) == n_rows_all == max(chunk_row0[-1], 1), name
        assert nb == len(i["ulen"]) and T == i["ulen"] and maxT == max(T), name
        assert Fc >= 16 and n_chunks == max(1, -(-maxT // Fc)), name
        assert Fc == i["fc_env"] or (i["fc_env"] == 0 and Fc % 128 == 0), name
        assert all(r % tile == 0 for r in chunk_rows) and chunk_row0[0] == 0, name
        assert all(chunk_row0[c + 1] - chunk_row0[c] == chunk_rows[c] for c in range(n_chunks)), name
        assert max_rows == max(chunk_rows + [tile]) >= tile, name
        # every (utterance, frame) exactly once, at chunk_row0[c] + row_off[c][u] + dt; every other entry -1
        want = [-1] * n_rows_all
        for u in range(nb):
            for t in range(T[u]):
                c, dt = divmod(t, Fc)
                at = chunk_row0[c] + row_off[c * nb + u] + dt
                assert row_off[c * nb + u] + dt < chunk_rows[c] and want[at] == -1, (name, u, t)
                want[at] = i["ustart"][u] + t
        assert row_src == want, name
    assert n_ok >= 30


def test_wave_cases_cover_what_they_must(outputs):
    _, waves = outputs
    outs = {name: o for name, _, _, o in waves}
    ins = {name: i for name, i, _, _ in waves}
    for T in (0, 1, 127, 128, 129):
        assert ins["one_T%d" % T]["ulen"] == [T] and outs["one_T%d" % T][0] == 0
    assert 0 in ins["ragged_with_empty"]["ulen"] and len(set(ins["ragged_with_empty"]["ulen"])) > 2
    for fc in (16, 48, 128):
        for name in ("fc_env_%d_ragged" % fc, "fc_env_%d_long" % fc):
            assert ins[name]["fc_env"] == fc == outs[name][3], name
        assert outs["fc_env_%d_long" % fc][4] > 2                      # several chunks
    # frames per chunk bound by the memory: down to 128, to 256 (by the free memory, by the tables there are), and not when only one of the
    # two conditions holds
    def conditions(i):
        have = 0.25 * i["free_bytes"] + 3.0 * i["ll_cap"] * 4
        Fc = max(128, (max(i["ulen"]) + 127) // 128 * 128)
        return 3.0 * (sum(i["ulen"]) + 128) * i["G"] * 4 > have, 3.0 * Fc * len(i["ulen"]) * i["G"] * 4 > have, Fc
    for name, Fc in (("mem_bound_Fc128", 128), ("mem_bound_Fc256", 256), ("mem_bound_Fc256_by_ll_cap", 256)):
        assert conditions(ins[name])[:2] == (True, True) and outs[name][3] == Fc < conditions(ins[name])[2], name
    assert ins["mem_bound_Fc256_by_ll_cap"]["free_bytes"] == 0
    for name, cond in (("mem_only_sum_condition", (True, False)), ("mem_only_chunk_condition", (False, True)), ("mem_neither_condition", (False, False))):
        assert conditions(ins[name])[:2] == cond and outs[name][3] == conditions(ins[name])[2], name
    assert [outs[n][0] for n in ("err_negative_length", "err_length_2_30", "err_chunk_rows", "err_source_frame_past_2_31")] == [1, 1, 2, 3]
    assert min(ins["err_negative_length"]["ulen"]) < 0 and 0x40000000 in ins["err_length_2_30"]["ulen"]
    assert outs["ok_source_frame_at_2_31_minus_1"][0] == 0 and max(outs["ok_source_frame_at_2_31_minus_1"]) == 0x7fffffff


def test_arena_driver_under_sanitizers(golden, lines, outputs, tmp_path_factory):
    """every case once more through the driver built with -fsanitize=address,undefined: the same output, nothing reported"""
    caps, waves = outputs
    driver = build_driver(str(tmp_path_factory.mktemp("arena_san") / "arena_driver_san"),
                          ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert run_driver(driver, lines) == [o for _, _, _, o in caps] + [o for _, _, _, o in waves]
