"""What tests/test_pipe_cpu.py and tests/test_gpu_pipe_inputs.py share: tests/pipe_driver.cpp built with plain g++, the lines it is given (single
decisions and scripts, as the driver's head describes them), and how its output lines are read."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "juicer_amd", "csrc")
QUEUED, RUNNING, THROUGH = 0, 1, 2
COLLECT, NEXT, THROUGH_ACT = 0, 1, 2
SET_OK, SET_DEPTH, SET_SLOTS, SET_DEVICE, SET_NOT_WITH = range(5)
RC_OK, RC_LOST, RC_STUCK, RC_KEEPS_ENDING, RC_FULL = range(5)
NOT_THIS_WAY, HANDLED, WAITING = range(3)
# the log: kind -> (name, the names of its arguments); KEXPORT and FETCH end in a list
LOG = {1: ("command", ["slot", "T", "row_slot", "init", "vslot", "ready_id", "seq"]), 2: ("bump", ["slot", "id"]), 3: ("kexport", ["n"]),
       4: ("piece", ["table", "feat_row", "base_row", "rows", "event", "batch_event"]), 5: ("collect", ["slot"]), 6: ("query_piece", ["event", "answer"]),
       7: ("query_table", ["table", "answer"]), 8: ("stop", ["lost"]), 9: ("start", []), 10: ("sync", []), 11: ("fetch", ["vslot0", "n"]), 12: ("wipe", ["stream"])}
SIZE_IN = ["depth", "slots", "streams", "utts", "rows", "tile", "chunk", "decouple", "planned", "piece"]
SIZE_OUT = ["K", "max_batch", "n_slots", "chunk", "decouple", "max_out", "piece_rows", "table_rows", "vslots"]


def build_driver(path, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, "-o", path, os.path.join(HERE, "pipe_driver.cpp")])
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


def dev(rep=(), left=(), late=(), pieces=0, tabs=(), clock=0):
    """<dev> of a script line: reports {slot frame error exported}, workgroups that left, ... that leave behind the pump, pieces and tables done, clock"""
    return [len(rep), list(rep), len(left), list(left), len(late), list(late), pieces, len(tabs), list(tabs), clock]


def read_log(o):
    """the log of a step -> [(name, {argument: value})]; kexport carries "pairs" [(slot, vslot)], fetch "slot_of" """
    log = []
    while o:
        name, args = LOG[o[0]]
        e, o = dict(zip(args, o[1:])), o[1 + len(args):]
        if name == "kexport":
            e["pairs"], o = [(o[2 * k], o[2 * k + 1]) for k in range(e["n"])], o[2 * e["n"]:]
        if name == "fetch":
            e["slot_of"], o = o[:e["n"]], o[e["n"]:]
        log.append((name, e))
    return log


def read_step(o):
    """a script (or harvest) line's output -> {rc, status, log, and the state behind it}"""
    it = iter(o)
    take = lambda n=None: next(it) if n is None else [next(it) for _ in range(n)]
    s = {"rc": take(), "status": take()}
    s["log"] = read_log(take(take()))
    for k in ("have_pipe", "pipe_on", "res_on", "K", "max_batch", "n_slots", "chunk", "decouple", "max_out", "piece_rows", "table_rows", "serial0",
              "frames_done", "piece_out", "piece_turn"):
        s[k] = take()
    s["table_used"] = take(s["K"])
    s["slots"] = [dict(zip(("batch_id", "utt", "dirty", "kexport"), take(4))) for _ in range(s["n_slots"])]
    s["q"] = []
    for _ in range(take()):
        b = dict(zip(("feats", "n", "table", "next", "n_done", "n_kexport", "rows", "rows_scored", "scored"), take(9)))
        b["u"] = [dict(zip(("state", "slot", "T", "row0"), take(4))) for _ in range(b["n"])]
        b["order"] = take(b["n"])
        s["q"].append(b)
    s["streams"] = [dict(zip(("dirty", "seq", "rid", "T_posted", "T_done", "err_done", "busy", "init_pending", "exported"), take(9))) for _ in range(take())]
    s["utts_through"], s["batches_back"], s["frames_searched"], s["rows_scored"] = take(4)
    assert not list(it), o
    return s


# ---- single decisions: (name, line)
def single_cases():
    c = []
    # setting: depth slots max_streams n_cus slot_wg_per_cu lazy hybrid.  The default depth, each bound on both sides, each rejection
    for slots in (1, 32, 63, 64, 191, 192, 256, 959, 960, 1024):
        c.append(("setting_default_depth_%d_slots" % slots, j("setting", 0, slots, 1024, 512, 2, 0, 0)))
    c += [("setting_default_slots", j("setting", 0, 0, 48, 256, 2, 0, 0)), ("setting_depth_1", j("setting", 1, 4, 8, 256, 2, 0, 0)),
          ("setting_depth_2", j("setting", 2, 4, 8, 256, 2, 0, 0)), ("setting_depth_32", j("setting", 32, 4, 8, 256, 2, 0, 0)),
          ("setting_depth_33", j("setting", 33, 4, 8, 256, 2, 0, 0)), ("setting_depth_negative", j("setting", -1, 4, 8, 256, 2, 0, 0)),
          ("setting_slots_eq_streams", j("setting", 4, 8, 8, 256, 2, 0, 0)), ("setting_slots_above_streams", j("setting", 4, 9, 8, 256, 2, 0, 0)),
          ("setting_slots_negative", j("setting", 4, -1, 8, 256, 2, 0, 0)), ("setting_slots_fill_device", j("setting", 4, 512, 1024, 256, 2, 0, 0)),
          ("setting_slots_above_device", j("setting", 4, 513, 1024, 256, 2, 0, 0)), ("setting_lazy", j("setting", 4, 4, 8, 256, 2, 1, 0)),
          ("setting_hybrid", j("setting", 4, 4, 8, 256, 2, 0, 1)), ("setting_depth_checked_first", j("setting", 40, 9, 8, 4, 2, 1, 1)),
          ("setting_slots_before_device", j("setting", 4, 9, 8, 4, 2, 1, 0)), ("setting_device_before_lazy", j("setting", 4, 9, 16, 4, 2, 1, 0))]
    # size: depth pipe_slots max_streams n_utts rows tile chunk_knob decouple_knob planned piece_knob (-1: knob unset)
    def size(name, depth=8, slots=0, streams=16, utts=4, rows=1000, tile=128, chunk=-1, decouple=-1, planned=5120, piece=-1):
        c.append(("size_" + name, j("size", depth, slots, streams, utts, rows, tile, chunk, decouple, planned, piece)))
    size("no_knobs"); size("nothing_planned", planned=0); size("slots_set", slots=5); size("slots_eq_streams", slots=16); size("slots_above_streams", slots=17)
    size("chunk_15", chunk=15); size("chunk_16", chunk=16); size("chunk_300", chunk=300); size("chunk_0", chunk=0)
    size("decouple_0", decouple=0); size("decouple_1", decouple=1); size("decouple_0_piece_256", decouple=0, piece=256)
    size("piece_127", piece=127); size("piece_128", piece=128); size("piece_255", piece=255); size("piece_256", piece=256); size("piece_1000_nothing_planned", piece=1000, planned=0)
    size("rows_64_whole_tiles", rows=64); size("rows_65", rows=65); size("rows_0", rows=0, utts=1); size("one_utterance", utts=1, rows=7, depth=2)
    # bounds: n_gmm group group_small tile, on both sides of the 1024-tile switch (64 row tiles x 16 state groups)
    c += [("bounds_960_states_small_tiles", j("bounds", 960, 64, 16, 128)), ("bounds_961_states", j("bounds", 961, 64, 16, 128)),
          ("bounds_toy", j("bounds", 7, 64, 16, 128)), ("bounds_9000_states", j("bounds", 9000, 64, 16, 128)), ("bounds_2000_states", j("bounds", 2000, 64, 16, 128))]
    # announce: does it go this way (pipe_mode lazy partial hybrid n_utts), has it outgrown the tables, is the queue full, the enqueue
    c += [("takes", j("takes", 1, 0, 0, 0, 1)), ("takes_not_pipe_mode", j("takes", 0, 0, 0, 0, 1)), ("takes_lazy", j("takes", 1, 1, 0, 0, 1)),
          ("takes_partial", j("takes", 1, 0, 1, 0, 1)), ("takes_hybrid", j("takes", 1, 0, 0, 1, 1)), ("takes_no_utterance", j("takes", 1, 0, 0, 0, 0)),
          ("outgrown_fits_exactly", j("outgrown", 4, 1152, 4, 1152)), ("outgrown_one_utterance_more", j("outgrown", 4, 1152, 5, 10)),
          ("outgrown_one_row_more", j("outgrown", 4, 1152, 2, 1153)), ("full_one_free", j("full", 3, 2)), ("full", j("full", 3, 3))]
    for name, used, T in (("first_table", [0, 0, 0], [5, 40]), ("hole_in_the_middle", [1, 0, 1], [5, 40]), ("hole_in_front", [0, 1, 1], [5, 40]),
                          ("last_table", [1, 1, 0], [5, 40]), ("ties_keep_index_order", [0, 0, 0], [4, 6, 4, 6, 4]), ("zero_length_and_one_frame", [1, 0, 0], [3, 0, 1, 0]),
                          ("one_utterance", [0, 0, 0], [17]), ("already_sorted", [0, 0, 0], [9, 8, 7])):
        c.append(("enqueue_" + name, j("enqueue", len(used), 1152, used, len(T), T)))
    # harvest: chunk decouple max_batch table T_posted frame error exported UT ui row0
    def harvest(name, T_posted, frame, UT, chunk=16, decouple=1, error=0, exported=0):
        c.append(("harvest_" + name, j("harvest", chunk, decouple, 4, 2, T_posted, frame, error, exported, UT, 1, 2309)))
    harvest("collect", 32, 20, 40); harvest("collect_one_short", 32, 31, 40); harvest("collect_short_of_the_end", 40, 39, 40)
    harvest("next_fr_at_T_posted", 16, 16, 40); harvest("next_ends_exactly", 24, 24, 40); harvest("next_ends_one_below", 23, 23, 40)
    harvest("next_ends_one_above", 25, 25, 40); harvest("next_fr_at_UT_minus_1", 39, 39, 40); harvest("next_ends_exactly_coupled", 24, 24, 40, decouple=0)
    harvest("next_chunk_128", 128, 128, 300, chunk=128)
    harvest("through_exported", 40, 40, 40, exported=1); harvest("through_not_exported", 40, 40, 40, exported=0)
    harvest("through_coupled", 40, 40, 40, decouple=0); harvest("through_exported_coupled", 40, 40, 40, decouple=0, exported=1)
    harvest("through_zero_length", 0, 0, 0, exported=1); harvest("through_one_frame", 1, 1, 1, exported=1)
    harvest("error_in_the_middle", 32, 20, 40, error=-3); harvest("error_at_the_end", 40, 40, 40, error=-3); harvest("error_and_exported", 40, 40, 40, error=-3, exported=1)
    for n in (63, 64, 65, 129):
        c.append(("harvest_many_%d" % n, j("harvest_many", n)))
    return c


def script_cases():
    return [(name, list(lines)) for name, lines in SCRIPTS]


# ---- scripts: (name, [line]).  Every script begins with reset depth pipe_slots max_streams tile chunk_knob decouple_knob planned piece_knob;
# the lines that follow carry what the device is said to have done (dev()).  They were written once, by hand-written device policies
# ("every command answered in full", "this slot fails at frame 7", "no piece completes") played against the recorded behaviour, and are data
# since: the golden is recorded for exactly these lines.
SCRIPTS = [('three_batches_two_slots',
  ['reset 3 2 4 128 16 -1 0 -1', 'announce 0 3 17 1 40 0 0 0 0 0 0', 'announce 1 2 16 33 0 0 0 1 1 0 0', 'decode 0 3 17 1 40 2 0 16 0 0 1 16 0 0 0 0 1 1 1 0',
   'wait 2 0 32 0 0 1 17 0 1 0 0 0 0 0', 'wait 2 0 40 0 1 1 1 0 1 0 0 0 0 0', 'announce 2 3 9 0 16 2 0 16 0 0 1 16 0 1 0 0 0 0 0',
   'decode 1 2 16 33 1 0 32 0 0 0 0 1 1 0 0', 'wait 2 0 33 0 1 1 16 0 1 0 0 0 0 0', 'decode 2 3 9 0 16 2 0 9 0 1 1 0 0 1 0 0 0 0 0']),
 ('three_batches_two_slots_coupled',
  ['reset 3 2 4 128 16 0 0 -1', 'announce 0 3 17 1 40 0 0 0 0 0 0', 'announce 1 2 16 33 0 0 0 1 1 0 0', 'decode 0 3 17 1 40 2 0 16 0 0 1 16 0 0 0 0 1 1 1 0',
   'wait 2 0 32 0 0 1 17 0 0 0 0 0 0 0', 'wait 2 0 40 0 0 1 1 0 0 0 0 0 0 0', 'announce 2 3 9 0 16 2 0 16 0 0 1 16 0 0 0 0 0 0 0',
   'decode 1 2 16 33 1 0 32 0 0 0 0 1 1 0 0', 'wait 2 0 33 0 0 1 16 0 0 0 0 0 0 0', 'decode 2 3 9 0 16 2 0 9 0 0 1 0 0 0 0 0 0 0 0']),
 ('more_slots_than_utterances',
  ['reset 2 0 6 128 -1 -1 0 -1', 'announce 0 3 130 128 127 0 0 0 0 0 0', 'decode 0 3 130 128 127 0 0 0 1 1 0 0', 'wait 3 0 128 0 0 1 128 0 1 2 127 0 1 0 0 0 0 0',
   'wait 1 0 130 0 1 0 0 0 0 0', 'announce 1 1 5 0 0 0 0 0 0', 'announce 2 2 300 2 0 0 0 1 1 0 0', 'decode 1 1 5 1 0 5 0 1 0 0 1 1 1 0',
   'decode 2 2 300 2 2 0 128 0 0 1 2 0 1 0 0 0 0 0', 'wait 1 0 256 0 0 0 0 0 0 0', 'wait 1 0 300 0 1 0 0 0 0 0']),
 ('pieces_and_events_lag',
  ['reset 4 2 2 128 16 -1 0 128', 'announce 0 2 200 100 0 0 0 0 0 0', 'announce 1 1 128 0 0 0 0 0 0', 'announce 2 2 20 10 0 0 0 0 0 0', 'decode 0 2 200 100 0 0 0 1 0 0',
   'wait 0 0 0 0 0 0', 'wait 0 0 0 2 0 0', 'wait 1 1 16 0 0 0 0 0 1 0 0', 'wait 2 0 16 0 0 1 32 0 0 0 0 0 0 0', 'wait 2 0 32 0 0 1 48 0 0 0 0 0 0 0',
   'wait 2 0 48 0 0 1 64 0 0 0 0 0 0 0', 'wait 2 0 64 0 0 1 80 0 0 0 0 0 0 0', 'wait 2 0 80 0 0 1 96 0 0 0 0 0 0 0', 'wait 2 0 96 0 0 1 100 0 1 0 0 0 0 0',
   'wait 1 0 112 0 0 0 0 2 2 1 2 0', 'wait 2 0 128 0 0 1 16 0 0 0 0 0 0 0', 'wait 2 0 144 0 0 1 32 0 0 0 0 0 0 0', 'wait 2 0 160 0 0 1 48 0 0 0 0 0 0 0',
   'wait 2 0 176 0 0 1 64 0 0 0 0 0 0 0', 'wait 2 0 192 0 0 1 80 0 0 0 0 0 0 0', 'wait 2 0 200 0 1 1 96 0 0 0 0 0 0 0', 'decode 1 1 128 2 0 16 0 0 1 112 0 0 0 0 0 0 0',
   'wait 2 0 20 0 1 1 128 0 1 0 0 0 0 0', 'decode 2 2 20 10 1 0 10 0 1 0 0 0 0 0']),
 ('kexport_then_scored',
  ['reset 4 2 2 128 16 -1 0 -1', 'announce 0 1 3 0 0 0 0 0 0', 'announce 1 2 4 5 0 0 0 1 1 0 0', 'decode 0 1 3 0 0 0 1 1 1 0', 'wait 1 0 3 0 0 0 0 0 0 0',
   'decode 1 2 4 5 2 0 4 0 1 1 5 0 1 0 0 0 0 0']),
 ('error_in_one_slot',
  ['reset 3 2 4 128 16 -1 0 -1', 'announce 0 4 40 30 20 10 0 0 0 0 0 0', 'announce 1 2 8 8 0 0 0 1 1 0 0', 'decode 0 4 40 30 20 10 0 0 0 1 1 1 0',
   'wait 2 0 7 -3 0 1 16 0 0 0 0 0 0 0', 'wait 1 1 30 0 1 0 0 0 0 0', 'wait 1 1 16 0 0 0 0 0 0 0', 'wait 1 1 20 0 1 0 0 0 0 0', 'wait 1 1 10 0 1 0 0 0 0 0',
   'decode 1 2 8 8 1 1 8 0 1 0 0 0 0 0', 'wait 1 1 8 0 1 0 0 0 0 0', 'announce 2 1 5 0 0 0 0 0 0', 'decode 2 1 5 0 0 0 1 1 0 0', 'wait 1 0 5 0 1 0 0 0 0 0']),
 ('error_in_one_slot_coupled',
  ['reset 3 2 4 128 16 0 0 -1', 'announce 0 3 40 30 20 0 0 0 0 0 0', 'decode 0 3 40 30 20 0 0 0 1 1 0 0', 'wait 1 1 16 -7 1 0 0 0 0 0', 'wait 1 0 16 0 0 0 0 0 0 0',
   'wait 1 0 32 0 0 0 0 0 0 0', 'wait 1 0 40 0 0 0 0 0 0 0', 'wait 1 0 16 0 0 0 0 0 0 0', 'wait 1 0 20 0 0 0 0 0 0 0']),
 ('collections',
  ['reset 3 2 2 128 16 -1 0 -1', 'announce 0 2 40 16 0 0 0 0 0 0', 'decode 0 2 40 16 0 0 0 1 1 0 0', 'wait 2 0 3 0 0 1 15 0 0 0 0 0 0 0',
   'wait 2 0 16 0 0 1 16 0 1 0 0 0 0 0', 'wait 1 0 20 0 0 0 0 0 0 0', 'wait 1 0 32 0 0 0 0 0 0 0', 'wait 1 0 40 0 1 0 0 0 0 0']),
 ('quiesce_with_one_command_unanswered',
  ['reset 3 3 4 128 16 -1 0 -1', 'announce 0 4 50 45 40 8 0 0 0 0 0 0', 'announce 1 1 20 0 0 0 1 1 0 0', 'decode 0 4 50 45 40 8 0 0 0 1 1 1 0',
   'wait 3 0 16 0 0 1 16 0 0 2 16 0 0 0 0 0 0 0', 'quiesce 2 0 32 0 0 1 32 0 0 1 2 0 0 0 0', 'wait 0 0 0 0 0 0', 'wait 3 0 48 0 0 1 45 0 1 2 32 0 0 0 0 0 0 0',
   'wait 3 0 50 0 1 1 8 0 1 2 40 0 1 0 0 0 0 0', 'quiesce 1 0 16 0 0 0 0 0 0 0', 'decode 1 1 20 0 0 0 0 0 0', 'wait 1 0 20 0 1 0 0 0 0 0']),
 ('quiesce_loses_a_workgroup',
  ['reset 3 2 2 128 16 -1 0 -1', 'announce 0 2 50 45 0 0 0 0 0 0', 'decode 0 2 50 45 0 0 0 1 1 0 0', 'quiesce 1 0 16 0 0 0 0 0 0 0', 'wait 0 0 0 0 0 0']),
 ('kernel_left_by_itself',
  ['reset 3 2 2 128 16 -1 0 -1', 'announce 0 2 50 45 0 0 0 0 0 0', 'decode 0 2 50 45 0 0 0 1 1 0 0', 'wait 2 0 16 0 0 1 16 0 0 2 0 1 0 0 0 0',
   'wait 2 0 32 0 0 1 32 0 0 0 0 0 0 0', 'wait 2 0 48 0 0 1 45 0 1 0 0 0 0 0', 'wait 1 0 50 0 1 0 0 0 0 0']),
 ('kernel_keeps_ending',
  ['reset 3 1 1 128 16 -1 0 -1', 'announce 0 1 50 0 0 0 0 0 0', 'decode 0 1 50 0 0 1 0 1 1 0 0', 'wait 0 0 1 0 0 0 0', 'wait 0 0 1 0 0 0 0', 'wait 0 0 1 0 0 0 0']),
 ('watchdog_30_s',
  ['reset 3 1 1 128 16 -1 0 -1', 'announce 0 2 50 3 0 0 0 0 0 0', 'decode 0 2 50 3 0 0 0 1 1 0 5', 'wait 0 0 0 0 0 30000000005', 'wait 1 0 16 0 0 0 0 0 0 30000000005',
   'wait 1 0 32 0 0 0 0 0 0 30000000005', 'wait 1 0 48 0 0 0 0 0 0 30000000005', 'wait 1 0 50 0 1 0 0 0 0 30000000005', 'wait 0 0 0 0 0 60000000005',
   'wait 0 0 0 0 0 60000000006', 'announce 1 1 4 1 0 3 0 1 0 0 0 0 0', 'decode 1 1 4 0 0 0 1 1 0 0', 'wait 1 0 4 0 1 0 0 0 0 0']),
 ('watchdog_reports_are_no_progress',
  ['reset 3 1 1 128 -1 -1 0 -1', 'announce 0 1 5000 0 0 0 0 0 0', 'decode 0 1 5000 0 0 0 1 1 0 0', 'wait 1 0 128 0 0 0 0 0 0 29000000000',
   'wait 1 0 256 0 0 0 0 0 0 30000000001']),
 ('not_the_announced_batch',
  ['reset 3 2 2 128 16 -1 0 -1', 'announce 0 2 6 7 0 0 0 0 0 0', 'decode 1 2 6 7 0 0 0 1 1 0 0', 'decode 0 2 6 7 0 0 0 0 0 0', 'announce 0 2 6 7 0 0 0 0 0 0',
   'decode 0 3 6 7 1 0 0 0 1 1 0 0', 'announce 0 2 6 7 0 0 0 0 0 0', 'decode 0 1 6 0 0 0 1 1 0 0', 'announce 0 2 6 7 0 0 0 0 0 0', 'decode 0 2 7 6 0 0 0 1 1 0 0',
   'announce 0 2 6 7 0 0 0 0 0 0', 'announce 1 2 6 7 0 0 0 1 1 0 0', 'decode 1 2 6 7 2 0 7 0 1 1 6 0 1 0 0 1 1 1 0', 'announce 0 2 6 7 0 0 0 0 0 0',
   'decode 0 2 6 7 0 0 0 1 1 0 0', 'wait 2 0 7 0 1 1 6 0 1 0 0 0 0 0']),
 ('queue_full_and_tables_with_holes',
  ['reset 3 2 2 128 16 -1 0 -1', 'announce 0 1 5 0 0 0 0 0 0', 'announce 1 1 6 0 0 0 1 1 0 0', 'announce 2 1 7 1 0 5 0 1 0 0 1 1 1 0',
   'announce 3 1 8 1 0 6 0 1 0 0 1 1 2 0', 'decode 0 1 5 0 0 0 0 0 0', 'announce 3 1 8 1 0 7 0 1 0 0 0 0 0', 'decode 1 1 6 0 0 0 1 1 0 0',
   'decode 2 1 7 1 0 8 0 1 0 0 0 0 0', 'announce 4 1 9 0 0 0 0 0 0', 'announce 5 2 9 9 0 0 0 1 1 1 0', 'decode 3 1 8 1 0 9 0 1 0 0 1 1 2 0',
   'decode 4 1 9 2 0 9 0 1 1 9 0 1 0 0 0 0 0', 'decode 5 2 9 9 0 0 0 0 0 0']),
 ('outgrowing_the_tables',
  ['reset 3 2 4 128 16 -1 0 -1', 'announce 0 2 5 6 0 0 0 0 0 0', 'announce 1 4 5 6 7 8 0 0 0 1 1 0 0', 'announce 2 5 1 1 1 1 1 2 0 6 0 1 1 5 0 1 0 0 1 1 1 0',
   'decode 2 5 1 1 1 1 1 0 0 0 1 1 0 0', 'wait 2 0 1 0 1 1 1 0 1 0 0 0 0 0', 'wait 2 0 1 0 1 1 1 0 1 0 0 0 0 0', 'wait 1 0 1 0 1 0 0 0 0 0',
   'announce 3 2 1500 550 0 0 0 0 0 0', 'decode 3 2 1500 550 0 0 0 1 1 0 0', 'wait 2 0 16 0 0 1 16 0 0 0 0 0 0 0', 'wait 2 0 32 0 0 1 32 0 0 0 0 0 0 0',
   'wait 2 0 48 0 0 1 48 0 0 0 0 0 0 0', 'wait 2 0 64 0 0 1 64 0 0 0 0 0 0 0', 'wait 2 0 80 0 0 1 80 0 0 0 0 0 0 0', 'wait 2 0 96 0 0 1 96 0 0 0 0 0 0 0',
   'wait 2 0 112 0 0 1 112 0 0 0 0 0 0 0', 'wait 2 0 128 0 0 1 128 0 0 0 0 0 0 0', 'wait 2 0 144 0 0 1 144 0 0 0 0 0 0 0', 'wait 2 0 160 0 0 1 160 0 0 0 0 0 0 0',
   'wait 2 0 176 0 0 1 176 0 0 0 0 0 0 0', 'wait 2 0 192 0 0 1 192 0 0 0 0 0 0 0', 'wait 2 0 208 0 0 1 208 0 0 0 0 0 0 0', 'wait 2 0 224 0 0 1 224 0 0 0 0 0 0 0',
   'wait 2 0 240 0 0 1 240 0 0 0 0 0 0 0', 'wait 2 0 256 0 0 1 256 0 0 0 0 0 0 0', 'wait 2 0 272 0 0 1 272 0 0 0 0 0 0 0', 'wait 2 0 288 0 0 1 288 0 0 0 0 0 0 0',
   'wait 2 0 304 0 0 1 304 0 0 0 0 0 0 0', 'wait 2 0 320 0 0 1 320 0 0 0 0 0 0 0', 'wait 2 0 336 0 0 1 336 0 0 0 0 0 0 0', 'wait 2 0 352 0 0 1 352 0 0 0 0 0 0 0',
   'wait 2 0 368 0 0 1 368 0 0 0 0 0 0 0', 'wait 2 0 384 0 0 1 384 0 0 0 0 0 0 0', 'wait 2 0 400 0 0 1 400 0 0 0 0 0 0 0', 'wait 2 0 416 0 0 1 416 0 0 0 0 0 0 0',
   'wait 2 0 432 0 0 1 432 0 0 0 0 0 0 0', 'wait 2 0 448 0 0 1 448 0 0 0 0 0 0 0', 'wait 2 0 464 0 0 1 464 0 0 0 0 0 0 0', 'wait 2 0 480 0 0 1 480 0 0 0 0 0 0 0',
   'wait 2 0 496 0 0 1 496 0 0 0 0 0 0 0', 'wait 2 0 512 0 0 1 512 0 0 0 0 0 0 0', 'wait 2 0 528 0 0 1 528 0 0 0 0 0 0 0', 'wait 2 0 544 0 0 1 544 0 0 0 0 0 0 0',
   'wait 2 0 560 0 0 1 550 0 1 0 0 0 0 0', 'wait 1 0 576 0 0 0 0 0 0 0', 'wait 1 0 592 0 0 0 0 0 0 0', 'wait 1 0 608 0 0 0 0 0 0 0', 'wait 1 0 624 0 0 0 0 0 0 0',
   'wait 1 0 640 0 0 0 0 0 0 0', 'wait 1 0 656 0 0 0 0 0 0 0', 'wait 1 0 672 0 0 0 0 0 0 0', 'wait 1 0 688 0 0 0 0 0 0 0', 'wait 1 0 704 0 0 0 0 0 0 0',
   'wait 1 0 720 0 0 0 0 0 0 0', 'wait 1 0 736 0 0 0 0 0 0 0', 'wait 1 0 752 0 0 0 0 0 0 0', 'wait 1 0 768 0 0 0 0 0 0 0', 'wait 1 0 784 0 0 0 0 0 0 0',
   'wait 1 0 800 0 0 0 0 0 0 0', 'wait 1 0 816 0 0 0 0 0 0 0', 'wait 1 0 832 0 0 0 0 0 0 0', 'wait 1 0 848 0 0 0 0 0 0 0', 'wait 1 0 864 0 0 0 0 0 0 0',
   'wait 1 0 880 0 0 0 0 0 0 0', 'wait 1 0 896 0 0 0 0 0 0 0', 'wait 1 0 912 0 0 0 0 0 0 0', 'wait 1 0 928 0 0 0 0 0 0 0', 'wait 1 0 944 0 0 0 0 0 0 0',
   'wait 1 0 960 0 0 0 0 0 0 0', 'wait 1 0 976 0 0 0 0 0 0 0', 'wait 1 0 992 0 0 0 0 0 0 0', 'wait 1 0 1008 0 0 0 0 0 0 0', 'wait 1 0 1024 0 0 0 0 0 0 0',
   'wait 1 0 1040 0 0 0 0 0 0 0', 'wait 1 0 1056 0 0 0 0 0 0 0', 'wait 1 0 1072 0 0 0 0 0 0 0', 'wait 1 0 1088 0 0 0 0 0 0 0', 'wait 1 0 1104 0 0 0 0 0 0 0',
   'wait 1 0 1120 0 0 0 0 0 0 0', 'wait 1 0 1136 0 0 0 0 0 0 0', 'wait 1 0 1152 0 0 0 0 0 0 0', 'wait 1 0 1168 0 0 0 0 0 0 0', 'wait 1 0 1184 0 0 0 0 0 0 0',
   'wait 1 0 1200 0 0 0 0 0 0 0', 'wait 1 0 1216 0 0 0 0 0 0 0', 'wait 1 0 1232 0 0 0 0 0 0 0', 'wait 1 0 1248 0 0 0 0 0 0 0', 'wait 1 0 1264 0 0 0 0 0 0 0',
   'wait 1 0 1280 0 0 0 0 0 0 0', 'wait 1 0 1296 0 0 0 0 0 0 0', 'wait 1 0 1312 0 0 0 0 0 0 0', 'wait 1 0 1328 0 0 0 0 0 0 0', 'wait 1 0 1344 0 0 0 0 0 0 0',
   'wait 1 0 1360 0 0 0 0 0 0 0', 'wait 1 0 1376 0 0 0 0 0 0 0', 'wait 1 0 1392 0 0 0 0 0 0 0', 'wait 1 0 1408 0 0 0 0 0 0 0', 'wait 1 0 1424 0 0 0 0 0 0 0',
   'wait 1 0 1440 0 0 0 0 0 0 0', 'wait 1 0 1456 0 0 0 0 0 0 0', 'wait 1 0 1472 0 0 0 0 0 0 0', 'wait 1 0 1488 0 0 0 0 0 0 0', 'wait 1 0 1500 0 1 0 0 0 0 0',
   'announce 4 1 3 0 0 0 0 0 0', 'drain', 'announce 4 1 3 0 0 0 0 0 0', 'decode 4 1 3 0 0 0 1 1 0 0', 'wait 1 0 3 0 1 0 0 0 0 0']),
 ('crossing_batches_in_one_refill',
  ['reset 4 3 3 128 16 -1 0 -1', 'announce 0 2 30 2 0 0 0 0 0 0', 'announce 1 2 12 11 0 0 0 1 1 0 0', 'announce 2 4 5 5 5 5 2 0 16 0 0 1 2 0 1 0 0 1 1 1 0',
   'decode 0 2 30 2 0 0 0 1 1 2 0', 'wait 3 0 30 0 1 1 12 0 1 2 11 0 1 0 0 0 0 0', 'decode 1 2 12 11 3 0 5 0 1 1 5 0 1 2 5 0 1 0 0 0 0 0',
   'decode 2 4 5 5 5 5 1 0 5 0 1 0 0 0 0 0']),
 ('refill_crosses_batches',
  ['reset 4 3 3 128 16 -1 0 -1', 'announce 0 4 10 10 10 10 0 0 0 0 0 0', 'announce 1 2 5 5 0 0 0 1 1 0 0',
   'decode 0 4 10 10 10 10 3 0 10 0 1 1 10 0 1 2 10 0 1 0 0 1 1 1 0', 'wait 3 0 10 0 1 1 5 0 1 2 5 0 1 0 0 0 0 0', 'decode 1 2 5 5 0 0 0 0 0 0']),
 ('quiesce_with_one_command_unanswered_coupled',
  ['reset 3 3 4 128 16 0 0 -1', 'announce 0 4 50 45 40 8 0 0 0 0 0 0', 'announce 1 1 20 0 0 0 1 1 0 0', 'decode 0 4 50 45 40 8 0 0 0 1 1 1 0',
   'wait 3 0 16 0 0 1 16 0 0 2 16 0 0 0 0 0 0 0', 'quiesce 2 0 32 0 0 1 32 0 0 1 2 0 0 0 0', 'wait 0 0 0 0 0 0', 'wait 3 0 48 0 0 1 45 0 0 2 32 0 0 0 0 0 0 0',
   'wait 3 0 50 0 0 1 8 0 0 2 40 0 0 0 0 0 0 0', 'quiesce 1 0 16 0 0 0 0 0 0 0', 'decode 1 1 20 0 0 0 0 0 0', 'wait 1 0 20 0 0 0 0 0 0 0']),
 ('quiesce_before_the_first_report_coupled',
  ['reset 3 2 2 128 16 0 0 -1', 'announce 0 2 12 40 0 0 0 0 0 0', 'decode 0 2 12 40 0 0 0 1 1 0 0', 'quiesce 1 0 16 0 0 1 1 0 0 0 0', 'wait 0 0 0 0 0 0',
   'wait 2 0 32 0 0 1 12 0 0 0 0 0 0 0', 'wait 1 0 40 0 0 0 0 0 0 0']),
 ('quiesce_before_the_first_report',
  ['reset 3 2 2 128 16 -1 0 -1', 'announce 0 2 12 40 0 0 0 0 0 0', 'decode 0 2 12 40 0 0 0 1 1 0 0', 'quiesce 1 0 16 0 0 1 1 0 0 0 0', 'wait 0 0 0 0 0 0',
   'wait 2 0 32 0 0 1 12 0 1 0 0 0 0 0', 'wait 1 0 40 0 1 0 0 0 0 0']),
 ('quiesce_loses_a_workgroup_coupled',
  ['reset 3 2 2 128 16 0 0 -1', 'announce 0 2 50 45 0 0 0 0 0 0', 'decode 0 2 50 45 0 0 0 1 1 0 0', 'quiesce 1 0 16 0 0 0 0 0 0 0', 'wait 0 0 0 0 0 0'])]
