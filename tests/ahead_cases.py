"""What tests/test_ahead_cpu.py and tests/test_gpu_ahead_inputs.py share: tests/ahead_driver.cpp built with plain g++, the lines it is given
(single decisions and scripts, as the driver's head describes them), and how a script's output lines are read."""
import itertools
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "juicer_amd", "csrc")
NONE, ANNOUNCED, SCORED = 0, 1, 2
FG_NONE, FG_BOTH = -1, -2
BG_NONE, BG_START, BG_GO_ON = 0, 1, 2
WAVE_OUT = ["mine", "drop", "pipe", "resumed", "discard", "unbank", "bank", "s0", "need", "drop_scored", "table", "none_free"]
CHUNK_OUT = ["n_work", "frames", "probe", "wants", "bg_step", "n_bg", "clipped", "launched"]
QUEUE_OUT = ["state", "buf", "bank", "nb", "feats"]


def build_driver(path, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I", CSRC, "-o", path,
                           os.path.join(HERE, "ahead_driver.cpp")])
    return path


def run_driver(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    return [[int(x) for x in l.split()] for l in out]


def j(*xs):
    """a line of the driver: words and (nested) lists of integers, flattened"""
    def flat(x):
        if isinstance(x, (list, tuple)):
            for y in x:
                yield from flat(y)
        else:
            yield int(x) if isinstance(x, bool) else x
    return " ".join(str(x) for x in flat(xs))


def hx(v):
    return float(v).hex()


def read_queue(o):
    """[nq, {state buf bank nb feats} * nq] -> list of dicts"""
    assert len(o) == 1 + len(QUEUE_OUT) * o[0], o
    return [dict(zip(QUEUE_OUT, o[1 + k * len(QUEUE_OUT):])) for k in range(o[0])]


def read_decode(o):
    """a `decode` line's output -> [wave]: each a dict of ok, the decisions (WAVE_OUT), n_chunks, chunks, gmm_synced and the queue behind it"""
    n_waves, o = o[0], o[1:]
    waves = []
    while o:
        w = dict(zip(["ok"] + WAVE_OUT + ["n_chunks"], o))
        o = o[len(WAVE_OUT) + 2:]
        w["chunks"] = []
        if w["ok"]:
            for _ in range(w["n_chunks"]):
                w["chunks"].append(dict(zip(CHUNK_OUT, o)))
                o = o[len(CHUNK_OUT):]
            w["gmm_synced"], o = o[0], o[1:]
        n = 1 + len(QUEUE_OUT) * o[0]
        w["queue"], o = read_queue(o[:n]), o[n:]
        waves.append(w)
    assert len(waves) == n_waves or (waves and not waves[-1]["ok"])
    return waves


# ---- single decisions: (name, line)
def single_cases():
    c = []
    # free_table: every foreground value against every set of scored tables, and an announced entry that names a table (holds none)
    for fg in (FG_BOTH, FG_NONE, 0, 1, 2):
        for held in itertools.chain.from_iterable(itertools.combinations(range(3), k) for k in range(4)):
            c.append(("free_table_fg%d_held%s" % (fg, "".join(map(str, held)) or "_none"), j("free_table", fg, len(held), [(SCORED, t) for t in held])))
    c.append(("free_table_announced_names_0", j("free_table", FG_NONE, 2, (ANNOUNCED, 0), (SCORED, 1))))
    # wants-scoring: first announced entry decides; a free table and room in the slab
    c += [("wants_empty", j("wants", 0, 3, 384, 0)),
          ("wants_fits_exactly", j("wants", 0, 3, 384, 1, (ANNOUNCED, 0, 128))),
          ("wants_one_row_too_many", j("wants", 0, 3, 384, 1, (ANNOUNCED, 0, 129))),
          ("wants_no_table", j("wants", 0, 3, 384, 3, (SCORED, 1, 8), (SCORED, 2, 8), (ANNOUNCED, 0, 8))),
          ("wants_fg_both_leaves_a_table", j("wants", FG_BOTH, 3, 384, 1, (ANNOUNCED, 0, 8))),
          ("wants_first_announced_too_large_second_not", j("wants", 0, 3, 384, 2, (ANNOUNCED, 0, 200), (ANNOUNCED, 0, 8))),
          ("wants_only_scored", j("wants", 0, 3, 384, 1, (SCORED, 1, 8))),
          ("rows_none", j("rows", 0)), ("rows_announced_only", j("rows", 3, (ANNOUNCED, 8), (SCORED, 16), (ANNOUNCED, 24)))]
    for name, q in (("empty", []), ("announced", [(ANNOUNCED, -1)]), ("scored", [(ANNOUNCED, -1), (SCORED, -1)]), ("started", [(ANNOUNCED, 1)]),
                    ("scored_and_started", [(SCORED, 0), (ANNOUNCED, -1)])):
        c.append(("any_" + name, j("any", len(q), q)))
    # announce: max_streams front queued fc_env nb ulen
    c += [("announce_nb_0", j("announce_one", 4, 0, 0, 0, 0)),
          ("announce_nb_max_plus_1", j("announce_one", 4, 0, 0, 0, 5, [3] * 5)),
          ("announce_nb_max", j("announce_one", 4, 0, 0, 0, 4, [3, 0, 5, 1])),
          ("announce_fourth_entry", j("announce_one", 4, 0, 3, 0, 2, [3, 4])),
          ("announce_third_entry_back", j("announce_one", 4, 0, 2, 0, 2, [3, 4])),
          ("announce_front", j("announce_one", 4, 1, 2, 0, 2, [3, 4])),
          ("announce_chunked_plan", j("announce_one", 4, 0, 0, 16, 2, [40, 4])),
          ("announce_one_chunk_with_fc_env", j("announce_one", 4, 0, 0, 16, 2, [16, 4]))]
    # claim: retry feats nb ustart ulen n {state bank feats nb ustart ulen}
    me = (0, 2, [0, 3], [3, 5])
    head = lambda state=SCORED, bank=-1, feats=0, nb=2, ustart=(0, 3), ulen=(3, 5): (state, bank, feats, nb, list(ustart), list(ulen))
    behind = (ANNOUNCED, -1, 1, 1, [0], [4])
    for name, retry, q in (("match", 0, [head()]), ("match_started", 0, [head(bank=1), behind]), ("empty_queue", 0, []),
                           ("other_feats", 0, [head(feats=1)]), ("other_nb", 0, [head(nb=1, ustart=(0,), ulen=(3,))]),
                           ("other_nb_longer", 0, [head(nb=3, ustart=(0, 3, 8), ulen=(3, 5, 1))]),
                           ("one_ustart", 0, [head(ustart=(0, 4))]), ("one_ulen", 0, [head(ulen=(3, 6))]),
                           ("head_announced_not_scored", 0, [head(state=ANNOUNCED)]),
                           ("not_mine_nothing_worked", 0, [behind, head(state=ANNOUNCED)]),
                           ("not_mine_scored_behind", 0, [behind, head()]),
                           ("not_mine_only_started", 0, [(ANNOUNCED, 0, 1, 1, [0], [4])]),
                           ("not_mine_scored_retry", 1, [behind, head()]),
                           ("not_mine_only_started_retry", 1, [(ANNOUNCED, 0, 1, 1, [0], [4])]),
                           ("match_retry", 1, [head()])):
        c.append(("claim_" + name, j("claim", retry, me, len(q), q)))
    # place: n_chunks nb max_streams pipeline lazy mine my_bank n {state bank}
    for name, a, q in (("nb_eq_B", (1, 4, 8, 1, 0, 0, -1), []), ("nb_eq_B_plus_1", (1, 5, 8, 1, 0, 0, -1), []),
                       ("odd_streams_nb_eq_B", (1, 3, 7, 1, 0, 0, -1), []), ("odd_streams_nb_eq_B_plus_1", (1, 4, 7, 1, 0, 0, -1), []),
                       ("odd_streams_bank_1", (1, 3, 7, 1, 0, 0, -1), [(SCORED, 0)]),
                       ("one_stream", (1, 1, 1, 1, 0, 0, -1), []), ("pipeline_off", (1, 2, 8, 0, 0, 0, -1), [(SCORED, -1)]),
                       ("pipeline_off_started", (1, 2, 8, 0, 0, 0, -1), [(SCORED, 1)]), ("lazy", (1, 2, 8, 1, 1, 0, -1), []),
                       ("chunked_scored", (2, 2, 8, 1, 0, 0, -1), [(SCORED, -1)]), ("chunked_started", (2, 2, 8, 1, 0, 0, -1), [(ANNOUNCED, 0)]),
                       ("chunked_nothing_scored", (2, 2, 8, 1, 0, 0, -1), [(ANNOUNCED, -1), (ANNOUNCED, -1)]),
                       ("outside_banks_batch_started", (1, 5, 8, 1, 0, 0, -1), [(SCORED, 1), (ANNOUNCED, -1)]),
                       ("outside_banks_nothing_started", (1, 5, 8, 1, 0, 0, -1), [(SCORED, -1)]),
                       ("bank_0_held", (1, 4, 8, 1, 0, 0, -1), [(SCORED, 0), (SCORED, -1)]), ("bank_1_held", (1, 4, 8, 1, 0, 0, -1), [(SCORED, 1)]),
                       ("resumed_bank_0", (1, 4, 8, 1, 0, 1, 0), [(SCORED, -1)]), ("resumed_bank_1", (1, 4, 8, 1, 0, 1, 1), [(SCORED, -1)]),
                       ("mine_not_started", (1, 4, 8, 1, 0, 1, -1), [(SCORED, 0)]), ("mine_started_but_outside_banks", (1, 5, 8, 1, 0, 1, 1), []),
                       ("not_mine_bank_ignored", (1, 4, 8, 1, 0, 0, 1), [])):
        c.append(("place_" + name, j("place", a, len(q), q)))
    # tables: need max_rows G ll_cap chunked n {max_rows} | take chunked n {state buf}
    c += [("need_fits", j("need", 16, 3, 48, 0, 0)), ("need_one_float_short", j("need", 16, 3, 47, 0, 0)),
          ("need_above_from_this_wave", j("need", 40, 3, 48, 0, 1, 8)), ("need_above_from_a_queued_batch", j("need", 8, 3, 48, 0, 2, 8, 40)),
          ("need_queued_fits", j("need", 8, 3, 48, 0, 2, 8, 16)), ("need_empty_slab", j("need", 8, 3, 0, 0, 0)),
          ("need_chunked", j("need", 40, 3, 48, 1, 1, 80)), ("need_eighth_rounds_down", j("need", 5, 3, 0, 0, 0)),
          ("take_all_free", j("take", 0, 0)), ("take_announced_table", j("take", 0, 1, (SCORED, 0))),
          ("take_0_and_1_held", j("take", 0, 2, (SCORED, 1), (SCORED, 0))), ("take_all_three_held", j("take", 0, 3, (SCORED, 2), (SCORED, 0), (SCORED, 1))),
          ("take_chunked", j("take", 1, 0)), ("take_chunked_whatever_is_held", j("take", 1, 1, (SCORED, 0))),
          ("take_announced_names_0", j("take", 0, 1, (ANNOUNCED, 0)))]
    # chunk work: c s0 row0 fc_env nb T frame0
    c += [("chunk_zero_length_utterance", j("chunk", 0, 0, 0, 16, 3, [5, 0, 7], [0, 0, 0])),
          ("chunk_zero_length_in_chunk_1", j("chunk", 1, 0, 100, 16, 3, [20, 0, 7], [0, 0, 0])),
          ("chunk_ends_on_the_boundary", j("chunk", 1, 4, 100, 16, 3, [16, 17, 32], [0, 0, 0])),
          ("chunk_ends_on_the_boundary_chunk_0", j("chunk", 0, 4, 0, 16, 3, [16, 17, 32], [0, 0, 0])),
          ("chunk_resumed_already_at_T", j("chunk", 0, 6, 256, 0, 3, [9, 5, 7], [9, 2, 7])),
          ("chunk_resumed_beyond_c0", j("chunk", 1, 0, 0, 16, 2, [30, 30], [20, 3])),
          ("chunk_resumed_beyond_c1", j("chunk", 1, 0, 0, 16, 2, [40, 40], [33, 32])),
          ("chunk_resumed_at_frame_0_of_zero_length", j("chunk", 0, 2, 8, 0, 2, [0, 4], [0, 1]))]
    # probe split: load_scale weighted resumed s0 fc_env nb T
    c += [("probe_span_128", j("probe", hx(1.0), 1, 0, 0, 0, 2, [128, 100])), ("probe_span_129", j("probe", hx(1.0), 1, 0, 0, 0, 2, [129, 100])),
          ("probe_nb_1", j("probe", hx(1.0), 1, 0, 0, 0, 1, [300])), ("probe_load_scale_known", j("probe", hx(1.5), 1, 0, 0, 0, 2, [300, 100])),
          ("probe_unweighted", j("probe", hx(1.0), 0, 0, 0, 0, 2, [300, 100])), ("probe_resumed", j("probe", hx(1.0), 1, 1, 0, 0, 2, [300, 100])),
          ("probe_T_32_and_33", j("probe", hx(1.0), 1, 0, 6, 0, 5, [200, 32, 33, 0, 31])),
          ("probe_chunked_span", j("probe", hx(1.0), 1, 0, 0, 144, 2, [300, 140]))]
    # background: pipeline lazy load_scale bg_max_load max_streams table_ready fg_bank rows_per_table have_heads n_heads {frame error}
    #             n {state bank buf nb n_chunks T}
    heads = [(0, 0)] * 4 + [(5, 0), (2, 7), (3, 0), (0, 0)]
    def bg(name, q, pipeline=1, lazy=0, load=1.0, ready=1, fg_bank=0, have=1, hd=heads, streams=8):
        c.append(("bg_" + name, j("bg", pipeline, lazy, hx(load), hx(4.0), streams, ready, fg_bank, 64, have, len(hd), hd, len(q), q)))
    fresh, going = (SCORED, -1, 2, 3, 1, [5, 6, 7]), (SCORED, 1, 2, 3, 1, [5, 6, 7])
    bg("first_start", [fresh], have=0); bg("first_start_beside_bank_1", [fresh], fg_bank=1); bg("first_start_table_not_ready", [fresh], ready=0)
    bg("first_start_ignores_heads", [fresh], have=1); bg("first_start_zero_length", [(SCORED, -1, 0, 2, 1, [0, 4])])
    bg("later_finished_error_running", [going]); bg("later_without_heads", [going], have=0)
    bg("load_just_above", [fresh], load=4.0 + 2 ** -50); bg("load_at_the_bound", [fresh], load=4.0)
    bg("head_only_announced", [(ANNOUNCED, -1, 0, 3, 1, [5, 6, 7])]); bg("head_fills_more_than_a_bank", [(SCORED, -1, 2, 5, 1, [5, 6, 7, 1, 1])])
    bg("head_fills_a_bank", [(SCORED, -1, 2, 4, 1, [5, 6, 7, 1])]); bg("head_in_chunks", [(SCORED, -1, 2, 3, 2, [5, 6, 7])])
    bg("pipeline_off", [fresh], pipeline=0); bg("lazy", [fresh], lazy=1); bg("empty_queue", [])
    bg("one_stream", [(SCORED, -1, 2, 1, 1, [5])], streams=1, hd=[(0, 0)])
    # clip rule (n_bg n_work nwg_all), both conditions at their boundaries
    c += [("clip_a_quarter", j("clip", 4, 1, 16)), ("clip_above_a_quarter", j("clip", 5, 1, 16)),
          ("clip_two_per_stream_left", j("clip", 2, 7, 16)), ("clip_less_than_two_per_stream_left", j("clip", 2, 8, 16)), ("clip_nothing", j("clip", 0, 8, 16))]
    # reserve: score_reserve gmm_ms_per_row last_wave_ms rows nwg_all
    c += [("reserve_rounds_up_to_8", j("reserve", -1, hx(0.001), hx(10.0), hx(1000.0), 256)), ("reserve_exact_multiple", j("reserve", -1, hx(0.001), hx(16.0), hx(1000.0), 256)),
          ("reserve_a_third_at_most", j("reserve", -1, hx(0.01), hx(1.0), hx(1000.0), 256)), ("reserve_zero_last_wave", j("reserve", -1, hx(0.001), hx(0.0), hx(1000.0), 256)),
          ("reserve_cost_unknown", j("reserve", -1, hx(0.0), hx(10.0), hx(1000.0), 256)), ("reserve_as_set", j("reserve", 5, hx(0.001), hx(10.0), hx(1000.0), 256)),
          ("reserve_as_set_above_a_third", j("reserve", 200, hx(0.0), hx(0.0), hx(0.0), 256)), ("reserve_set_to_zero", j("reserve", 0, hx(0.001), hx(10.0), hx(1000.0), 256)),
          ("reserve_small_grid", j("reserve", -1, hx(0.001), hx(1.0), hx(1000.0), 20))]
    # hold-replan: pf_rebalance gmm_ms_per_row rows search_ms_per_frame frames_now
    c += [("hold_never_1", j("hold", 1, hx(1.0), hx(10.0), hx(1.0), hx(10.0))), ("hold_always_0", j("hold", 0, hx(0.0), hx(0.0), hx(1.0), hx(10.0))),
          ("hold_auto_a_tenth_exactly", j("hold", -1, hx(1.0), hx(1.0), hx(1.0), hx(10.0))),
          ("hold_auto_just_below_a_tenth", j("hold", -1, hx(1.0), hx(1.0), hx(1.0), hx(10.0 + 2 ** -40))),
          ("hold_auto_scoring_unknown", j("hold", -1, hx(0.0), hx(100.0), hx(1.0), hx(10.0))),
          ("hold_auto_search_unknown", j("hold", -1, hx(1.0), hx(100.0), hx(0.0), hx(10.0))), ("hold_auto_no_frames", j("hold", -1, hx(1.0), hx(100.0), hx(1.0), hx(0.0)))]
    # waves: max_streams n_utts len
    c += [("waves_n_eq_streams_no_sort", j("waves", 3, 3, [2, 9, 4])), ("waves_n_eq_streams_plus_1", j("waves", 3, 4, [2, 9, 4, 7])),
          ("waves_equal_lengths_keep_index_order", j("waves", 2, 5, [4, 4, 6, 4, 6])), ("waves_partial_last", j("waves", 3, 8, [5, 1, 8, 2, 0, 9, 3, 3])),
          ("waves_one_stream", j("waves", 1, 3, [2, 5, 3])), ("waves_none", j("waves", 3, 0)), ("waves_12_streams", j("waves", 12, 13, list(range(13))))]
    # load_scale: load_scale load_sum load_frames
    c += [("load_first_update", j("load", hx(1.0), hx(47400.0 * 10), hx(10.0))), ("load_later_update", j("load", hx(2.0), hx(47400.0 * 30), hx(10.0))),
          ("load_clamp_low", j("load", hx(1.0), hx(10.0), hx(10.0))), ("load_clamp_high", j("load", hx(3.0), hx(1e12), hx(1.0))),
          ("load_zero_frames", j("load", hx(2.5), hx(100.0), hx(0.0))), ("load_measured_exactly_1", j("load", hx(1.0), hx(23700.0 * 8), hx(8.0)))]
    return c


# ---- scripts: (name, [line]); every script begins with reset max_streams pipeline lazy G tile nwg_all load_scale bg_max_load ll_cap
def heads(n, frame=0, error=0):
    return [n, [(frame, error)] * n]


def script_cases():
    s = []
    A8, B8 = [3, 5, 4, 3, 6, 2, 7, 4], [4, 2, 6, 3, 5, 5, 3, 8]
    def ann(feats, lens): return j("announce", feats, len(lens), lens)
    def dec(feats, lens, streams, can_launch=3, ready=1, grow=1, frame=0, error=0): return j("decode", feats, len(lens), lens, can_launch, ready, grow, heads(streams, frame, error))
    reset = lambda streams, pipeline=1, lazy=0, ll_cap=0, load=1.0: j("reset", streams, pipeline, lazy, 3, 8, 64, hx(load), hx(4.0), ll_cap)
    A, B = (0, A8), (1, B8)
    # tests/test_gpu_parity.py::test_scores_ahead_of_the_search, its first decoder (8 streams, batches of 8: outside the banks) ...
    s.append(("scores_ahead_of_the_search", [
        reset(8), ann(*B), dec(*A, 8), ann(*A), dec(*B, 8), ann(*A), dec(*A, 8), dec(*A, 8), dec(*B, 8), ann(*B), dec(*A, 8), dec(*A, 8), ann(*B), dec(*A, 8),
        "announce-none", dec(*B, 8), ann(*A), dec(*B, 8), dec(3, A8, 8)]))
    # ... and its second (3 streams: the batch of 8 goes in three waves formed by length; a batch of three rides on the last wave)
    small3 = (1, B8[:3])
    s.append(("scores_ahead_in_waves", [reset(3), ann(*A), dec(*A, 3), ann(*small3), dec(*A, 3), dec(*small3, 3)]))
    # tests/test_gpu_parity.py::test_two_batches_in_flight, its first block (12 streams, batches of 6: two banks)
    mk = lambda k: [3 + (k * i + k) % 5 for i in range(6)]
    b = {"A": (0, mk(1)), "B": (1, mk(2)), "C": (2, mk(3))}
    two = [reset(12), ann(*b["B"]), ann(*b["C"]), dec(*b["A"], 12)]
    for k, (n, nxt) in enumerate((("B", "A"), ("C", "B"), ("A", "C"), ("B", "A"), ("C", "B"))):
        two += [ann(*b[nxt]), dec(*b[n], 12, frame=2, ready=0 if k == 0 else 1)]
    two += [dec(*b["C"], 12, frame=2), dec(*b["A"], 12), ann(*b["B"]), ann(*b["C"]), dec(3, b["A"][1] + b["B"][1][:4], 12), dec(*b["B"], 12), dec(*b["C"], 12, frame=3)]
    s.append(("two_batches_in_flight", two))
    # the same stream of batches where it cannot run two at once: pipeline off, a lazy network, a heavy load, streams in error
    for name, kw, dkw in (("two_batches_pipeline_off", dict(pipeline=0), {}), ("two_batches_lazy", dict(lazy=1), {}), ("two_batches_heavy_load", dict(load=4.5), {}),
                          ("two_batches_streams_in_error", {}, dict(frame=1, error=7)), ("two_batches_one_scoring_per_launch", {}, dict(can_launch=1)),
                          ("two_batches_no_scoring_possible", {}, dict(can_launch=0))):
        s.append((name, [reset(12, **kw), ann(*b["B"]), ann(*b["C"]), dec(*b["A"], 12, **dkw), ann(*b["A"]), dec(*b["B"], 12, **dkw), ann(*b["B"]),
                         dec(*b["C"], 12, **dkw), dec(*b["A"], 12, **dkw)]))
    # the slab: a queued batch larger than it (the scored tables go, room is added), and a slab that cannot grow (nothing ahead survives)
    big = (2, [30, 40])
    s.append(("slab_grows_for_a_queued_batch", [reset(4), ann(0, [3, 4]), dec(1, [2, 2], 4), ann(*big), dec(0, [3, 4], 4), dec(*big, 4), dec(*big, 4)]))
    s.append(("slab_cannot_grow", [reset(4), ann(0, [3, 4]), dec(1, [2, 2], 4), ann(*big), dec(3, [5, 5], 4, grow=0), dec(0, [3, 4], 4)]))
    s.append(("slab_cannot_grow_at_first", [reset(4), ann(0, [3, 4]), dec(1, [2, 2], 4, grow=0), dec(1, [2, 2], 4)]))
    # four announcements (the fourth is not taken), too many utterances (not taken), an empty batch
    s.append(("four_announcements", [reset(4), ann(0, [3, 4]), ann(1, [2]), ann(2, [1, 1]), ann(3, [5]), ann(4, [1] * 5), dec(0, [3, 4], 4), dec(0, [3, 4], 4),
                                     dec(1, [2], 4), dec(2, [1, 1], 4, frame=1), dec(5, [], 4), dec(3, [5], 4)]))
    # odd streams, one stream
    s.append(("seven_streams", [reset(7), ann(1, [2, 3, 4]), ann(2, [4, 4, 4, 4]), dec(0, [3, 3, 3], 7), dec(1, [2, 3, 4], 7, frame=1), dec(2, [4, 4, 4, 4], 7)]))
    s.append(("one_stream", [reset(1), ann(1, [3]), dec(0, [2], 1), ann(0, [2]), dec(1, [3], 1), dec(0, [2, 4, 1], 1)]))
    return s
