"""What tests/test_push_cpu.py and tests/test_gpu_push_inputs.py share: tests/push_driver.cpp built with plain g++, the lines it is given (single
decisions and scripts, as the driver's head describes them), and how its output lines are read."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "juicer_amd", "csrc")
ARG_OK, ARG_BAD, ARG_BAD_STREAM, ARG_NOT_STARTED, ARG_TOO_MANY_ROWS = range(5)
NOT_FOUND, TOO_LONG, FROM_STAGE, FROM_RESULTS = range(4)
COLLECTS, FAILS, ARENA_ONLY = 1, 2, 3                                   # the kinds of a spec: what the device meets at a frame
EVERY, SHARE, TILE, ROW_LIMIT = 100, 32, 128, 0x7fffff00
AFTER_IN = ["error", "frame", "n_collect", "n_path", "n_path_new", "limit", "fail_T", "by_flag", "flag", "host_n_collect", "last_collect"]
AFTER_OUT = ["failed", "at", "collected", "host_collects", "T"]
STREAM = ["T", "started", "open", "last_collect", "last_trace", "n_collect", "dirty", "dev_n_collect", "nlist"]


def build_driver(path, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", path,
                           os.path.join(HERE, "push_driver.cpp")])
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


def read_step(o, M):
    """a script line's output -> {rc, log: [(kind, ...)], streams: [{...}]}"""
    it = iter(o)
    take = lambda n=None: next(it) if n is None else [next(it) for _ in range(n)]
    s = {"rc": take(), "log": []}
    l = take(take())
    while l:
        kind = l[0]
        if kind == 4:
            s["log"].append(("booked", l[1], l[2], l[3]))
            l = l[4:]
            continue
        n, width, name = l[1], {1: 3, 2: 1, 3: 2}[kind], {1: "launch", 2: "gc", 3: "trace"}[kind]
        s["log"].append((name, [tuple(l[2 + width * k:2 + width * (k + 1)]) for k in range(n)]))
        l = l[2 + width * n:]
    s["streams"] = [dict(zip(STREAM, take(len(STREAM)))) for _ in range(M)]
    assert not list(it), o
    return s


# ---- single decisions: (name, line)
def single_cases():
    c = []
    # chunk: Fc left interval last_collect T.  f_collect = last_collect + 101; f_collect + 1 - T on both sides of 1 and of Fc
    c += [("chunk_first_ends_with_T_101", j("chunk", 512, 500, 1, -1, 0)), ("chunk_rule_behind_by_50", j("chunk", 64, 500, 1, -1, 151)),
          ("chunk_rule_room_0", j("chunk", 64, 500, 1, -1, 101)), ("chunk_rule_room_1", j("chunk", 64, 500, 1, -1, 100)),
          ("chunk_rule_room_Fc", j("chunk", 64, 500, 1, -1, 37)), ("chunk_rule_room_Fc_plus_1", j("chunk", 64, 500, 1, -1, 36)),
          ("chunk_rule_room_Fc_minus_1", j("chunk", 64, 500, 1, -1, 38)), ("chunk_interval_0", j("chunk", 64, 500, 0, -1, 100)),
          ("chunk_interval_0_left_below_Fc", j("chunk", 64, 5, 0, -1, 100)), ("chunk_left_below_Fc", j("chunk", 64, 5, 150, -1, 0)),
          ("chunk_left_below_Fc_rule_nearer", j("chunk", 64, 5, 150, 200, 300)), ("chunk_left_1", j("chunk", 64, 1, 1, 100, 150)),
          ("chunk_after_a_collection_at_100", j("chunk", 512, 500, 1, 100, 101)), ("chunk_after_an_early_collection", j("chunk", 512, 500, 1, 40, 41))]
    # after: error frame n_collect n_path n_path_new limit fail_T by_flag flag host_n_collect last_collect last_trace interval
    def after(name, frame, limit, error=0, n_collect=0, n_path=0, n_path_new=1, fail_T=None, by_flag=0, flag=0, host=0, lc=-1, lt=-1, interval=1):
        c.append(("after_" + name, j("after", error, frame, n_collect, n_path, n_path_new, limit, limit if fail_T is None else fail_T, by_flag, flag, host, lc, lt, interval)))
    after("error", 17, 64, error=-3); after("error_call_target", 17, 64, error=-3, fail_T=300); after("error_by_flag", 17, 64, error=-3, by_flag=1, flag=1)
    after("short_no_collection", 30, 64); after("short_collected_by_count", 30, 64, n_collect=1); after("short_collected_by_count_3_2", 30, 64, n_collect=3, host=2)
    after("short_count_equal", 30, 64, n_collect=2, host=2); after("short_frame_rule_would_fire", 150, 200)   # (behind the limit only)
    after("short_count_rule_would_fire", 30, 64, n_path=20000, n_path_new=0)
    after("limit_gap_100", 100, 100); after("limit_gap_101", 101, 101); after("limit_gap_101_after_a_collection", 152, 152, lc=50, host=1, n_collect=1)
    after("limit_gap_100_after_a_collection", 151, 151, lc=50, host=1, n_collect=1); after("beyond_limit_gap_101", 102, 101)
    after("limit_n_path_10000", 50, 50, n_path=10000, n_path_new=1); after("limit_n_path_10001", 50, 50, n_path=10001, n_path_new=1)
    after("limit_ratio_12_exactly", 50, 50, n_path=12000, n_path_new=1000); after("limit_ratio_above_12", 50, 50, n_path=12001, n_path_new=1000)
    after("limit_path_new_0", 50, 50, n_path=10001, n_path_new=0); after("limit_path_new_0_n_path_10000", 50, 50, n_path=10000, n_path_new=0)
    after("limit_collected_and_rule", 101, 101, n_collect=1)            # (the device's collection serves: no second one)
    after("flag_set", 30, 64, by_flag=1, flag=1); after("flag_clear_count_moved", 30, 64, by_flag=1, flag=0, n_collect=1)
    after("flag_ignored_by_count", 30, 64, by_flag=0, flag=1); after("flag_clear_at_limit_rule_fires", 101, 101, by_flag=1, flag=0)
    after("flag_set_at_limit", 101, 101, by_flag=1, flag=1)
    after("trace_gap_eq_interval", 30, 64, n_collect=1, lt=19, interval=10); after("trace_gap_interval_plus_1", 30, 64, n_collect=1, lt=18, interval=10)
    after("trace_first", 101, 101, interval=150); after("trace_first_interval_100", 101, 101, interval=100); after("trace_first_interval_99", 101, 101, interval=99)
    # book: at last_trace interval n_collect
    c += [("book_due", j("book", 201, 100, 100, 1)), ("book_not_due", j("book", 201, 100, 101, 1)), ("book_first", j("book", 100, -1, 150, 0))]
    # round: nS {T last_collect}*nS nw {stream target out}*nw
    c += [("round_all_run", j("round", 3, [0, -1, 0, -1, 0, -1], 3, [0, 50, 0, 1, 300, 0, 2, 101, 0])),
          ("round_one_at_target", j("round", 3, [50, -1, 101, 100, 7, -1], 3, [0, 50, 0, 1, 300, 0, 2, 101, 0])),
          ("round_one_out", j("round", 3, [10, -1, 101, 100, 7, -1], 3, [0, 50, 1, 1, 300, 0, 2, 101, 0])),
          ("round_limit_eq_target", j("round", 2, [0, -1, 101, 100], 2, [0, 101, 0, 1, 202, 0])),
          ("round_limit_below_target", j("round", 2, [0, -1, 101, 100], 2, [0, 102, 0, 1, 203, 0])),
          ("round_behind_the_rule", j("round", 2, [130, -1, 250, 100], 2, [0, 140, 0, 1, 400, 0])),
          ("round_gaps", j("round", 8, [5, -1, 9, -1, 30, -1, 9, -1, 9, -1, 150, 100, 9, -1, 9, -1], 2, [5, 400, 0, 2, 60, 0])),
          ("round_order_of_the_call", j("round", 4, [0, -1, 0, -1, 0, -1, 0, -1], 3, [3, 10, 0, 0, 20, 0, 2, 30, 0])),
          ("round_nobody", j("round", 2, [50, -1, 60, -1], 2, [0, 50, 0, 1, 60, 1]))]
    # check1: has_dec nS {started}*nS s has_frames n_frames;  call: has_dec n has_lists
    c += [("check1_ok", j("check1", 1, 2, [1, 1], 1, 1, 5)), ("check1_no_decoder", j("check1", 0, 2, [1, 1], 1, 1, 5)), ("check1_negative_stream", j("check1", 1, 2, [1, 1], -1, 1, 5)),
          ("check1_stream_eq_n", j("check1", 1, 2, [1, 1], 2, 1, 5)), ("check1_negative_frames", j("check1", 1, 2, [1, 1], 1, 1, -1)),
          ("check1_no_frames_pointer", j("check1", 1, 2, [1, 1], 1, 0, 5)), ("check1_zero_frames_no_pointer", j("check1", 1, 2, [1, 1], 1, 0, 0)),
          ("check1_not_started", j("check1", 1, 2, [1, 0], 1, 1, 5)), ("check1_bad_before_not_started", j("check1", 1, 2, [1, 0], 1, 0, 5)),
          ("call_ok", j("call", 1, 3, 1)), ("call_no_decoder", j("call", 0, 3, 1)), ("call_negative", j("call", 1, -1, 1)), ("call_no_lists", j("call", 1, 3, 0)),
          ("call_empty_no_lists", j("call", 1, 0, 0))]
    # pack: nS {T started}*nS D tile n {stream n_frames has_frames}*n
    def pack(name, streams, entries, D=39, tile=TILE):
        c.append(("pack_" + name, j("pack", len(streams), streams, D, tile, len(entries), entries)))
    four = [(0, 1), (40, 1), (7, 1), (0, 0)]
    pack("three_streams", four, [(0, 10, 1), (1, 20, 1), (2, 5, 1)]); pack("entry_with_0_frames", four, [(0, 10, 1), (1, 0, 1), (2, 5, 1)])
    pack("entry_with_0_frames_no_pointer", four, [(0, 10, 1), (1, 0, 0), (2, 5, 1)]); pack("negative_slot", four, [(2, 3, 1), (1, 20, 1)])
    pack("slot_0_at_frame_eq_row", [(10, 1), (0, 1)], [(1, 10, 1), (0, 4, 1)]); pack("rows_1", four, [(1, 1, 1)]); pack("rows_tile", four, [(0, 100, 1), (2, 28, 1)])
    pack("rows_tile_plus_1", four, [(0, 100, 1), (2, 29, 1)]); pack("rows_0", four, [(0, 0, 1), (2, 0, 0)]); pack("empty_call", four, [])
    pack("stream_twice", four, [(0, 10, 1), (1, 20, 1), (0, 5, 1)]); pack("stream_twice_0_frames", four, [(0, 10, 1), (0, 0, 1)])
    pack("not_started", four, [(0, 10, 1), (3, 20, 1)]); pack("not_started_first", four, [(3, 20, 1), (0, 10, 1)]); pack("negative_stream", four, [(0, 10, 1), (-1, 20, 1)])
    pack("stream_eq_n", four, [(4, 20, 1)]); pack("negative_frames", four, [(0, -1, 1)]); pack("frames_no_pointer", four, [(1, 3, 1), (0, 10, 0)])
    pack("row_limit_plus_1", four, [(0, 0x40000000, 1), (1, 0x3fffff01, 1)]); pack("two_to_the_31", four, [(0, 0x40000000, 1), (1, 0x40000000, 1)])
    pack("D_13_tile_64", four, [(0, 65, 1)], D=13, tile=64)
    # tracelist: nS {T started}*nS n {stream}*n
    c += [("tracelist_ok", j("tracelist", 4, four, 3, [2, 0, 1])), ("tracelist_twice", j("tracelist", 4, four, 3, [2, 1, 2])),
          ("tracelist_not_started", j("tracelist", 4, four, 3, [1, 3, 2])), ("tracelist_out_of_range", j("tracelist", 4, four, 2, [1, 4])),
          ("tracelist_empty", j("tracelist", 4, four, 0, []))]
    # k_partial_many: layout M; request s nhave {label time}*; reply found len have res_cap n i
    c += [("layout_1", j("layout", 1)), ("layout_16", j("layout", 16)), ("layout_300", j("layout", 300)),
          ("request_none_yet", j("request", 5, 0)), ("request_three", j("request", 2, 3, [7, 10, 8, 25, 9, 31])),
          ("reply_not_found", j("reply", 0, 0, 3, 100, 4, 1)), ("reply_not_found_stale_len", j("reply", 0, 500, 3, 100, 4, 1)),
          ("reply_share", j("reply", 1, 3 + SHARE, 3, 100, 4, 1)), ("reply_share_plus_1", j("reply", 1, 4 + SHARE, 3, 100, 4, 1)),
          ("reply_nothing_new", j("reply", 1, 3, 3, 100, 4, 1)), ("reply_res_cap", j("reply", 1, 100, 90, 100, 4, 1)), ("reply_above_res_cap", j("reply", 1, 101, 90, 100, 4, 1)),
          ("reply_above_res_cap_and_share", j("reply", 1, 101, 3, 100, 4, 1)), ("reply_first_entry", j("reply", 1, 5, 3, 100, 16, 0)), ("reply_last_entry", j("reply", 1, 5, 3, 100, 16, 15)),
          ("reply_only_entry", j("reply", 1, 5, 0, 100, 1, 0))]
    # finish: partial nhave {label time}* n {label time}*n - the hypothesis comes newest first
    c += [("finish_partial", j("finish", 1, 1, [7, 10], 3, [9, 31, 8, 25, 7, 10])), ("finish_no_partial", j("finish", 0, 1, [7, 10], 3, [9, 31, 8, 25, 7, 10])),
          ("finish_no_hypothesis", j("finish", 1, 2, [7, 10, 8, 25], -1)), ("finish_empty_hypothesis", j("finish", 1, 2, [7, 10, 8, 25], 0))]
    return c


# ---- scripts: (name, [line]).  A call list - ("init", s) | ("push", {stream: (frames, [spec])}) | ("finish", s, [(label, time)]) |
# ("takeover",) - becomes the lines of a script twice: every push stream by stream (push1: jd_stream_push) and in one call (pushN:
# jd_streams_push).  The replies are the same: a stream's specs are consumed launch by launch, and with Fc above every push a chunk of
# the one path is a round of the other.  (A spec names a frame, not a launch: the one path cuts its launches at the chunk's end, the other
# at a limit it works out anew for every round.)
def spec(kind, f, n_path=20000, n_path_new=0):
    return [kind, f, n_path, n_path_new]


def script_lines(M, interval, ref, Fc, calls, many):
    lines = [j("reset", M, interval, ref, Fc)]
    for c in calls:
        if c[0] == "init":
            lines.append(j("init", c[1]))
        elif c[0] == "takeover":
            lines.append("takeover")
        elif c[0] == "finish":
            lines.append(j("finish", c[1], len(c[2]), c[2]))
        elif many:
            lines.append(j("pushN", len(c[1]), [[s, nf, len(sp), sp] for s, (nf, sp) in c[1].items()]))
        else:
            lines += [j("push1", s, nf, len(sp), sp) for s, (nf, sp) in c[1].items()]
    return lines


S0 = [spec(COLLECTS, 30), spec(COLLECTS, 136)]
CALLS = {
    # three streams at different offsets, the frame rule alone
    "frame_rule_three_streams": (3, 1, 0, 512, [("init", 0), ("init", 1), ("init", 2), ("push", {1: (30, [])}), ("push", {2: (57, [])}),
                                                ("push", {0: (250, []), 1: (250, []), 2: (250, [])}), ("push", {0: (64, []), 2: (1, [])}),
                                                ("push", {0: (0, []), 1: (101, []), 2: (7, [])}), ("finish", 1, [(5, 300), (4, 120)])]),
    # the kernel's own collections (the count rule in the middle of a launch), and the count rule behind a stream's last frame: 10001 records and
    # none new (fires), a ratio of exactly 12 (does not), above 12 (does)
    "device_collections": (3, 1, 0, 512, [("init", 0), ("init", 1), ("init", 2), ("push", {0: (150, S0), 1: (150, []), 2: (40, [spec(COLLECTS, 40, 10001, 0)])}),
                                          ("push", {0: (150, [spec(COLLECTS, 151)]), 1: (150, [spec(COLLECTS, 300, 12000, 1000)]), 2: (100, [])}),
                                          ("push", {1: (1, [spec(COLLECTS, 301, 12001, 1000)])})]),
    "device_collections_reference_counts": (3, 150, 1, 512, [("init", 0), ("init", 1), ("init", 2),
                                                             ("push", {0: (150, S0), 1: (150, [spec(ARENA_ONLY, 20)]), 2: (40, [spec(COLLECTS, 40, 10001, 0)])}),
                                                             ("push", {0: (150, [spec(COLLECTS, 151)]), 1: (150, [spec(ARENA_ONLY, 249), spec(COLLECTS, 250)]), 2: (100, [])})]),
    # a stream fails in the middle of a call while the others go on; it is finished, begun again and pushed once more
    "one_stream_fails": (3, 1, 0, 512, [("init", 0), ("init", 1), ("init", 2), ("push", {0: (250, []), 1: (250, [spec(FAILS, 120)]), 2: (250, [])}),
                                        ("push", {0: (10, []), 1: (10, []), 2: (10, [])}), ("finish", 1, []), ("init", 1),
                                        ("push", {0: (120, []), 1: (120, []), 2: (120, [])}), ("finish", 0, [(3, 200), (2, 90), (1, 15)]), ("init", 0),
                                        ("push", {0: (102, [])})]),
    "first_launch_fails": (2, 150, 0, 512, [("init", 0), ("init", 1), ("push", {0: (300, [spec(FAILS, 1)]), 1: (300, [])})]),
    # a batch takes the streams over in between: the calls behind it are refused until the streams are begun again
    "takeover_in_between": (2, 1, 0, 512, [("init", 0), ("init", 1), ("push", {0: (120, []), 1: (90, [])}), ("takeover",), ("push", {0: (5, []), 1: (5, [])}),
                                           ("init", 0), ("init", 1), ("push", {0: (101, []), 1: (102, [])})]),
    "interval_0": (2, 0, 0, 512, [("init", 0), ("init", 1), ("push", {0: (300, []), 1: (7, [])}), ("push", {1: (200, [])})]),
    "interval_150": (2, 150, 0, 512, [("init", 0), ("init", 1), ("push", {0: (500, []), 1: (450, [])}), ("push", {0: (500, []), 1: (57, [])})]),
}
# ... and what only one path has: chunks of the table's length (jd_stream_push), a stream listed twice (jd_streams_push)
ONE_ONLY = {"chunks_of_64": (1, 1, 0, 64, [("init", 0), ("push", {0: (300, [])}), ("push", {0: (37, [spec(COLLECTS, 303)])}), ("push", {0: (64, [])})]),
            "chunks_of_64_interval_0": (1, 0, 0, 64, [("init", 0), ("push", {0: (300, [])})])}
MANY_ONLY = [("stream_twice", [j("reset", 2, 1, 0, 512), "init 0", "init 1", j("pushN", 3, [[0, 5, 0], [1, 5, 0], [0, 5, 0]]), j("pushN", 2, [[1, 5, 0], [0, 0, 0]])])]


def script_cases():
    s = [(name + "_one", script_lines(*a, many=False)) for name, a in CALLS.items()] + [(name + "_many", script_lines(*a, many=True)) for name, a in CALLS.items()]
    return s + [(name, script_lines(*a, many=False)) for name, a in ONE_ONLY.items()] + MANY_ONLY


def script_streams(reset_line):
    return int(reset_line.split()[1])


# ---- :358-368 restated: the frames behind which collectPaths runs and tracePartialPath rides on it, for T frames; count_fires(f): the
# count rule's answer behind frame f
def reference_schedule(T, interval, count_fires=lambda f: False):
    last_collect = last_trace = -1
    collects, traces = [], []
    for f in range(T):
        if count_fires(f) or f - last_collect > EVERY:
            collects.append(f)
            last_collect = f
            if interval > 0 and f - last_trace > interval:
                traces.append(f)
                last_trace = f
    return collects, traces
