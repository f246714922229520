"""The states and operations jd_debug_paths is run on (tests/test_gpu_paths.py) and tests/paths_ref.py is held to a brute force on
(tests/test_paths_ref_cpu.py, which also asserts that every case has the shape its name says).  Everything is built from fixed seeds.

CASES maps a name to (family, builder); case(name) builds it once.  encode() turns a Desc into the int32 words of
juicer_amd/csrc/jd_paths.h."""
import functools
import os
import shutil
import subprocess

import numpy as np

from paths_ref import COLLECT, LZ, PARTIAL_SHARE, TRACE, TRACE_MANY, Desc, Stream, f2i

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "juicer_amd", "csrc")
PD_MAGIC = 0x4a445031
LIVE, LIVE2, DEAD, NINF = f2i(-1.5), f2i(-3.0e38), f2i(LZ), f2i(-np.inf)     # (LIVE2: just above LOG_ZERO)
TEE_FLAG, SOLE_FLAG = 0x40000000, 0x20000000


# ------------------------------------------------------------------ the words of a description

def encode(D):
    w = [PD_MAGIC, D.NE, len(D.streams), len(D.ops), D.cap_slots, D.cap_items, D.cap_new, D.pcount, D.sentinel, D.n_states]
    w += list(D.row_ptr) + list(D.arc_in)
    parts = [np.asarray(w, np.int64)]
    for s in D.streams:
        parts.append(np.asarray([s.started, s.needs_init, s.error, s.frame, s.path_new, s.n_collect, s.n_paths_ref, s.path_new_ref, s.best_final,
                                 s.lst_nw, s.dirty_nw, s.cap_paths, s.n_paths], np.int64))
        parts.append(s.paths.reshape(-1).astype(np.int64))
        parts.append(np.asarray(s.arrival, np.int64))
        w = []
        for wave in s.rec:
            w.append(len(wave))
            for n, src, toks in wave:
                w += [n, src]
                for sc, p in toks:
                    w += [sc, p]
        for wave in s.items:
            w.append(len(wave))
            w += list(wave)
        for wave in s.dirty:
            w.append(len(wave))
            w += list(wave)
        parts.append(np.asarray(w, np.int64))
    w = []
    for op in D.ops:
        if op[0] == COLLECT:
            _, work, G, thr, rule = op
            w += [COLLECT] + ([0, work] if isinstance(work, int) else [len(work)] + list(work)) + [G, thr, rule]
        elif op[0] == TRACE:
            w += list(op)
        else:
            _, entries, res_cap = op
            w += [TRACE_MANY, len(entries)] + [x for e in entries for x in e] + [res_cap]
    parts.append(np.asarray(w, np.int64))
    return np.concatenate(parts).astype(np.int32)


def build_driver(path, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, "-o", path, os.path.join(HERE, "paths_driver.cpp")])
    return path


def run_driver(driver, descs):
    """a line of words per description -> per description (rc, [integers], message)"""
    text = "\n".join(" ".join(str(int(x)) for x in d) for d in descs) + "\n"
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(descs)
    res = []
    for l in out:
        head, _, msg = l.partition("|")
        v = [int(x) for x in head.split()]
        res.append((v[0], v[1:], msg.strip()))
    return res


def checksum(words):
    """what the driver prints of an image: sum of (i + 1) * word i, the words as unsigned, modulo 2^64"""
    w = np.asarray(words, np.int32).view(np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int((w * (np.arange(w.shape[0], dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))


# ------------------------------------------------------------------ building blocks

def gc_range(n_paths, G, blk):
    """gc_range of jd_gc.h, restated: a workgroup's records, in multiples of 1024"""
    per = (((n_paths + G - 1) // G) + 1023) & ~1023
    return min(n_paths, per * blk), min(n_paths, per * (blk + 1))


def mk_paths(prev, frames=None, labels=None):
    """an arena around the predecessors: frames that never decrease with the index, word labels, and fields whose every bit is the index's"""
    prev = np.asarray(prev, np.int64)
    n = prev.shape[0]
    q = np.arange(n, dtype=np.int64)
    P = np.empty((n, 7), np.int32)
    P[:, 0] = prev
    P[:, 1] = q // 3 if frames is None else frames
    P[:, 2] = 1 + (q * 7) % 997 if labels is None else labels
    P[:, 3] = 5 + (q * 13) % 211
    P[:, 4] = (-0.25 * q).astype(np.float32).view(np.int32)
    P[:, 5] = (0.5 * q).astype(np.float32).view(np.int32)
    P[:, 6] = ((q * 2654435761) & 0xffffffff).astype(np.uint32).view(np.int32)       # (any bits at all, NaNs among them)
    return P


def deal(NE, toks, waves=1, inst_counts=None, n_states=1, first_n=3):
    """the token list dealt to instances of 3, 4, .. NE + 2, 3, .. states in order (left-over slots: live, no path), the instances to
    the waves: inst_counts each, or evenly.  -> rec[wave] = [(nStates, source state, [(score, path)])]"""
    toks = list(toks)
    insts, at, n = [], 0, first_n
    total = None if inst_counts is None else sum(inst_counts)
    while (at < len(toks)) if total is None else (len(insts) < total):
        t = toks[at:at + n - 2]
        at += n - 2
        insts.append((n, len(insts) % n_states, t + [(LIVE, -1)] * (n - 2 - len(t))))
        n = n + 1 if n < NE + 2 else 3
    assert at >= len(toks), "more tokens than the instances hold"
    if inst_counts is None:
        per = -(-len(insts) // waves) if insts else 0
        inst_counts = [max(0, min(per, len(insts) - w * per)) for w in range(waves)]
    rec, at = [], 0
    for c in inst_counts:
        rec.append(insts[at:at + c])
        at += c
    return rec


def deal_items(items, waves=1, item_counts=None):
    items = [int(x) for x in items]
    if item_counts is None:
        per = -(-len(items) // waves) if items else 0
        item_counts = [max(0, min(per, len(items) - w * per)) for w in range(waves)]
    items = items + [-1] * (sum(item_counts) - len(items))
    out, at = [], 0
    for c in item_counts:
        out.append(items[at:at + c])
        at += c
    return out


def live(paths):
    return [(LIVE, int(p)) for p in paths]


def stream(prev, toks=(), items=(), *, NE=3, waves=1, inst_counts=None, item_counts=None, paths=None, **kw):
    return Stream(mk_paths(prev) if paths is None else paths, deal(NE, toks, waves, inst_counts, kw.get("n_states", 1)),
                  deal_items(items, waves, item_counts), **kw)


def collect1(s, G, thr=0, rule=0, NE=3, **kw):
    """one stream, one collection through the null work list"""
    return Desc([s], [(COLLECT, 0, G, thr, rule)], NE=NE, **kw)


def forest(rng, n, back=40):
    """random predecessors, at most `back` records behind (or none)"""
    q = np.arange(n)
    return np.maximum(q - rng.integers(1, back + 1, n), -1)


def forest_roots(rng, prev, share):
    """random roots, added until that share of the records is reachable"""
    n = len(prev)
    seen = np.zeros(n, bool)
    out, kept = [], 0
    for q in rng.permutation(n):
        if kept >= share * n:
            break
        if seen[q]:
            continue
        out.append(int(q))
        while q >= 0 and not seen[q]:
            seen[q] = True
            kept += 1
            q = prev[q]
    return out


# ------------------------------------------------------------------ collection cases

SIZES = (0, 1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769, 131071, 131072, 131073, 140003)
# (4098 and 9218: the only size of the list with two records behind the 16-byte part is 2 itself)
EXTRA_SIZES = (4098, 9218)
SIZE_PAIRS = ((0, 1), (0, 32), (1, 1), (1, 32), (2, 2), (3, 3), (4, 1), (5, 32), (7, 5), (1023, 1), (1023, 2), (1024, 1), (1024, 31), (1025, 3),
              (1025, 32), (4095, 1), (4096, 1), (4096, 5), (4097, 1), (4097, 31), (4098, 1), (8191, 1), (8191, 2), (8192, 2), (8192, 1), (8193, 1),
              (8193, 3), (9218, 2), (32767, 5), (32768, 32), (32769, 31), (32769, 3), (131071, 2), (131072, 32), (131073, 1), (131073, 31),
              (140003, 5), (140003, 1), (140003, 32))
CASES = {}


def add(family, name, builder):
    assert name not in CASES
    CASES[name] = (family, builder)


def size_case(n, G, mark):
    rng = np.random.default_rng(1000 * n + G)
    none = np.full(n, -1)
    if mark == "second":                                   # every second record, as one chain from the newest
        s = stream(np.maximum(np.arange(n) - 2, -1), live([n - 1]), [n - 1, -1])
    elif mark == "forest50":
        prev = forest(rng, n)
        r = forest_roots(rng, prev, 0.5)
        s = stream(prev, live(r[0::2]), r[1::2], best_final=r[0] if r else -1, waves=3)
    elif mark == "stride":                                 # every predecessor in another workgroup's range
        s = stream(np.maximum(np.arange(n) - 1025, -1), live(range(max(0, n - 1025), n, 3)), range(max(0, n - 1024), n, 3), waves=2)
    elif mark == "chain":                                  # everything, as one chain from the newest
        s = stream(np.arange(n) - 1, (), [n - 1])
    elif mark == "none":
        s = stream(forest(rng, n), [(LIVE, -1), (DEAD, n - 1)], [-1, -1])
    elif mark == "first":
        s = stream(none, live([0]))
    elif mark == "last":
        s = stream(none, (), (), best_final=n - 1, inst_counts=[1])
    return collect1(s, G)


for n_, G_ in SIZE_PAIRS:
    marks = ["second", "forest50" if n_ <= 32769 else "stride"]
    if n_ in (0, 1, 5, 1025, 4097, 8193) or (n_, G_) in ((140003, 5), (131073, 31)):
        marks += ["none", "first", "last"]
    if (n_, G_) in ((131073, 1), (131072, 32), (8193, 3), (4096, 1), (3, 3)):
        marks += ["chain"]
    if n_ > 1025 and gc_range(n_, G_, 0)[1] == 1024 and "stride" not in marks:      # ranges of 1024: every predecessor in another one
        marks += ["stride"]
    for m_ in marks:
        if n_ > 0 or m_ in ("second", "none"):
            add("sizes", "size_%d_G%d_%s" % (n_, G_, m_), functools.partial(size_case, n_, G_, m_))


def marks_case(n, G, which):
    """no predecessors: exactly the listed records are kept (as items, over four waves)"""
    return collect1(stream(np.full(n, -1), live(which[:2]), which[2:], waves=4), G)


def range_chain_case(n, G, blk):
    lo, hi = gc_range(n, G, blk)
    prev = np.full(n, -1)
    prev[lo + 1:hi] = np.arange(lo, hi - 1)
    return collect1(stream(prev, live([hi - 1])), G)


def forest_case(n, G, share, seed):
    rng = np.random.default_rng(seed)
    prev = forest(rng, n, 40 if share > 0.05 else 2000)          # (short chains where few records are to be kept)
    r = forest_roots(rng, prev, share)
    return collect1(stream(prev, live(r[:len(r) // 3]), r[len(r) // 3:], waves=5), G)


add("marks", "marks_before_second_trip_0", functools.partial(marks_case, 8193, 1, list(range(4096, 8193, 5))))
add("marks", "marks_before_second_trip_1", functools.partial(marks_case, 8193, 1, [77] + list(range(4096, 8193, 5))))
add("marks", "marks_before_second_trip_4096", functools.partial(marks_case, 8193, 1, list(range(0, 4096)) + list(range(4097, 8193, 2))))
add("marks", "marks_lower_workgroups_0", functools.partial(marks_case, 9218, 3, list(range(8192, 9218))))
add("marks", "marks_lower_workgroups_full", functools.partial(marks_case, 9218, 3, list(range(0, 4096)) + [9000, 9217]))
add("marks", "marks_one_middle_range", functools.partial(range_chain_case, 32769, 5, 2))
for share_ in (1, 50, 99):
    add("marks", "forest_%d_percent" % share_, functools.partial(forest_case, 32769, 3, share_ / 100.0, share_))
add("marks", "forest_1_percent_140003", functools.partial(forest_case, 140003, 5, 0.01, 7))
add("marks", "forest_99_percent_140003", functools.partial(forest_case, 140003, 32, 0.99, 8))


def roots_case(kind):
    n = 6000
    rng = np.random.default_rng(42)
    chain = np.arange(n) - 1
    if kind == "shared_long_chains":                       # an item root and a token root on one long chain each way round, and on the same record
        prev = np.full(n, -1)
        prev[1:3000] = np.arange(0, 2999)
        prev[3001:6000] = np.arange(3000, 5999)
        s = stream(prev, live([2999, 4000, 5999]), [1500, 5999, 5999], waves=2)
    elif kind == "same_root_many_times":
        s = stream(chain, live([4321] * 700), [4321] * 900 + [17] * 50, best_final=4321, waves=3)
    elif kind == "roots_of_minus_one":
        s = stream(forest(rng, n), live([-1, 100, -1, -1]), [-1, 200, -1], best_final=-1, waves=2)
    elif kind == "dead_token_with_path":
        s = stream(forest(rng, n), [(DEAD, 5999), (LIVE, 100), (NINF, 5000), (LIVE2, 300), (DEAD, 100), (DEAD, -1)], [200])
    elif kind == "tokens_only":
        s = stream(forest(rng, n), live([5999, 3000, 10]), ())
    elif kind == "items_only":
        s = stream(forest(rng, n), (), [5999, 3000, 10], inst_counts=[2])
    elif kind == "best_final_only":
        s = stream(forest(rng, n), (), (), best_final=5998, inst_counts=[1], item_counts=[1])
    elif kind == "best_final_minus_one":
        s = stream(forest(rng, n), live([40]), [50], best_final=-1)
    return collect1(s, 2)


for k_ in ("shared_long_chains", "same_root_many_times", "roots_of_minus_one", "dead_token_with_path", "tokens_only", "items_only",
           "best_final_only", "best_final_minus_one"):
    add("roots", "roots_" + k_, functools.partial(roots_case, k_))

# a graph of six states: 0 has an arc with a model, 1 a tee model among label-less arcs, 2 only label-less arcs (flag bits set on them),
# 3 no arcs, 4 a model arc (its key will be zero), 5 a model arc behind a label-less one
GRAPH = dict(row_ptr=(0, 1, 3, 5, 5, 6, 8), arc_in=(7, 0, 9 | TEE_FLAG, 0, SOLE_FLAG, 11 | SOLE_FLAG, 0, 3))


def dirty_case(kind, pcount=1):
    n = 3000
    rng = np.random.default_rng(5)
    prev = forest(rng, n)
    items = [2999, 2500, 2000, 1500, 1000, 500, -1, 2998]
    arrival = [0, 1, 2, 3, -1, 5]                          # (one wave of items: the item's index is its place)
    lst_nw, dirty_nw, dirty = 2, 2, [[0, 1, 2], [3, 4, 5, 0]]
    item_counts = [8, 0]
    if kind == "other_wave_count":
        dirty_nw, dirty = 5, [[0], [], [1, 2, 3], [4], [5, 5]]
    elif kind == "dirty_nw_0":
        dirty_nw = 0
    elif kind == "empty":
        dirty = [[], []]
    s = Stream(mk_paths(prev), deal(3, live([10, 20]), lst_nw, n_states=6), deal_items(items, lst_nw, item_counts), dirty, arrival, n_states=6,
               dirty_nw=dirty_nw, n_paths_ref=n, path_new_ref=n)
    return Desc([s], [(COLLECT, 0, 2, 0, 1)], pcount=pcount, cap_items=16, **GRAPH)


for k_ in ("base", "other_wave_count", "dirty_nw_0", "empty"):
    add("dirty", "dirty_" + k_, functools.partial(dirty_case, k_))
add("dirty", "dirty_without_pcount", functools.partial(dirty_case, "base", 0))


def geometry_case(NE, lst_nw, G, inst_counts, item_counts):
    n = 5000
    rng = np.random.default_rng(lst_nw * 100 + G + NE)
    prev = forest(rng, n)
    n_tok = sum(inst_counts) * 2
    toks = [((LIVE, DEAD, LIVE2)[i % 3], int(p)) for i, p in enumerate(rng.integers(-1, n, n_tok))]
    s = Stream(mk_paths(prev), deal(NE, toks[:sum(inst_counts)], lst_nw, inst_counts), deal_items(rng.integers(-1, n, sum(item_counts)), lst_nw, item_counts))
    return collect1(s, G, NE=NE)


def wave_counts(lst_nw, values):
    """the values in turn over the waves, the last wave's first"""
    return [values[(lst_nw - 1 - w) % len(values)] for w in range(lst_nw)]


for nw_ in (1, 16, 17, 33, 512):
    for G_ in (1, 2):
        NE_ = 3 if (nw_ + G_) % 2 else 6
        add("geometry", "geometry_nw%d_G%d_NE%d" % (nw_, G_, NE_),
            functools.partial(geometry_case, NE_, nw_, G_, wave_counts(nw_, (130, 0, 1, 63, 64, 65)), wave_counts(nw_, (65, 0, 1, 64))))
add("geometry", "geometry_nw33_G2_NE6", functools.partial(geometry_case, 6, 33, 2, wave_counts(33, (65, 64, 0, 130)), wave_counts(33, (1, 65))))
add("geometry", "geometry_nw17_G1_NE3", functools.partial(geometry_case, 3, 17, 1, wave_counts(17, (65, 64, 0, 130)), wave_counts(17, (1, 65))))

INACTIVE = ("not_started", "needs_init", "error", "no_waves", "below_threshold")


def work_stream(seed, n, waves, **kw):
    rng = np.random.default_rng(seed)
    prev = forest(rng, n)
    r = forest_roots(rng, prev, 0.3)
    return stream(prev, live(r[0::2]), r[1::2], waves=waves, best_final=r[-1], **kw)


def work_case(why, n_streams):
    thr = 2500
    ss = [work_stream(1, 9000, 3), work_stream(2, 4097, 1), work_stream(3, 2501, 5), work_stream(4, 12000, 2)][:n_streams]
    kw = {"not_started": dict(started=0), "needs_init": dict(needs_init=1), "error": dict(error=-43)}.get(why, {})
    if why == "no_waves":
        ss[1] = Stream(mk_paths(forest(np.random.default_rng(9), 4097)), [], [], lst_nw=0)
    elif why == "below_threshold":
        ss[1] = work_stream(2, thr, 1)
    else:
        ss[1] = work_stream(2, 4097, 1, **kw)
    order = [2, 0, 1, 3][:n_streams] if n_streams == 4 else [1, 2, 0]
    return Desc(ss, [(COLLECT, order, 3, thr, 0)])


for i_, why_ in enumerate(INACTIVE):
    add("work", "work_%s_%d_streams" % (why_, 3 + i_ % 2), functools.partial(work_case, why_, 3 + i_ % 2))
add("work", "work_part_of_the_streams", lambda: Desc([work_stream(1, 9000, 3), work_stream(2, 4097, 1), work_stream(3, 2501, 5)], [(COLLECT, [2, 0], 4, 0, 0)]))
# (k_gc_begin writes the stream's GcState before it decides: by_rule is 1 for a stream it then leaves alone)
add("work", "work_not_started_while_the_host_asks", lambda: Desc([work_stream(1, 9000, 3), work_stream(2, 4097, 1, started=0)], [(COLLECT, [0, 1], 2, -1, 1)]))
add("work", "work_null_list_second_stream", lambda: Desc([work_stream(1, 9000, 3), work_stream(2, 4097, 1)], [(COLLECT, 1, 4, 0, 0)]))


def counter_case(pcount, thr_at, rule, n_paths_ref=0, path_new_ref=0, path_new=0):
    n = 10500
    s = work_stream(11, n, 2, n_collect=3, n_paths_ref=n_paths_ref, path_new_ref=path_new_ref, path_new=path_new)
    return Desc([s], [(COLLECT, 0, 2, -1 if thr_at is None else n + thr_at, rule)], pcount=pcount)


add("counters", "counters_own_records", functools.partial(counter_case, 0, -1, 0))
add("counters", "counters_threshold_at_n_paths", functools.partial(counter_case, 0, 0, 0))                 # inactive: n_paths > threshold fails
add("counters", "counters_threshold_at_n_paths_rule_off", functools.partial(counter_case, 0, 0, 1, path_new=875))     # 10500 / 875 = 12: does not fire
add("counters", "counters_threshold_at_n_paths_rule_fires", functools.partial(counter_case, 0, 0, 1, path_new=874))
add("counters", "counters_threshold_minus_one", functools.partial(counter_case, 0, None, 1))
add("counters", "counters_threshold_minus_one_rule_off", functools.partial(counter_case, 0, None, 0))
add("counters", "counters_ref_rule_fires", functools.partial(counter_case, 1, -1, 1, 12001, 1000))
add("counters", "counters_ref_rule_at_12", functools.partial(counter_case, 1, -1, 1, 12000, 1000))          # the ratio is 12: not above it
add("counters", "counters_ref_rule_10000", functools.partial(counter_case, 1, -1, 1, 10000, 1))             # nPath is 10000: not above it
add("counters", "counters_ref_rule_10001_first", functools.partial(counter_case, 1, -1, 1, 10001, 0))       # no collection yet: the ratio is +inf
add("counters", "counters_ref_host_asks", functools.partial(counter_case, 1, None, 1, 50, 40))
add("counters", "counters_ref_rule_only_inactive", functools.partial(counter_case, 1, 0, 1, 12000, 1000))
add("counters", "counters_ref_rule_only_active", functools.partial(counter_case, 1, 0, 1, 12001, 1000))


def twice_case():
    D = forest_case(32769, 3, 0.5, 21)
    D.ops = D.ops * 2
    return D


add("counters", "two_collections_in_a_row", twice_case)


# ------------------------------------------------------------------ trace cases

def tstream(prev, tips, *, NE=3, waves=1, frames=None, labels=None, inst_counts=None, **kw):
    """a stream whose instances have one tip each, in their first emitting token"""
    n = 3
    rec_toks = []
    for t in tips:
        rec_toks += [(LIVE, int(t))] + [(LIVE, -1)] * (n - 3)
        n = n + 1 if n < NE + 2 else 3
    return Stream(mk_paths(prev, frames, labels), deal(NE, rec_toks, waves, inst_counts), deal_items((), waves), **kw)


def trace1(s, last_frame=-1, res_cap=16, model=0, NE=3, **kw):
    return Desc([s], [(TRACE, 0, last_frame, res_cap, model)], NE=NE, **kw)


# a tree: a trunk 0..9, then branches
#   10 -> 11 -> 12 (from 9), 13 -> 14 (from 9), 15 (from 11), 16 -> 17 (from 5), 18 (from -1: another root), 19 (from 17)
TREE = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 9, 13, 11, 5, 16, -1, 17]


def chain_case(n_words, res_cap, model=0, extra=0):
    """a chain of n_words word records (model level: `extra` records without a label between and below them), two tips on it"""
    n = n_words * (1 + extra) + extra
    labels = np.zeros(n, np.int64)
    labels[extra::1 + extra] = 1 + np.arange(n_words) % 900
    labels = labels[:n]
    s = tstream(np.arange(n) - 1, [n - 1, n - 1], labels=labels)
    return trace1(s, -1, res_cap, model)


def many_tips_case(NE, waves, per_wave):
    n = 4000
    prev = np.arange(n) - 1
    prev[2000:] = 1999                                      # a trunk of 2000 records, then 2000 leaves on its end
    rng = np.random.default_rng(waves)
    tips_ = 2000 + rng.integers(0, 2000, waves * per_wave)
    return trace1(tstream(prev, tips_, NE=NE, waves=waves, frames=np.arange(n) // 50), 10, 4096, NE=NE)


add("trace", "trace_one_tip", lambda: trace1(tstream(TREE, [12])))
add("trace", "trace_all_tips_equal", lambda: trace1(tstream(TREE, [14] * 5)))
add("trace", "trace_nothing_shared", lambda: trace1(tstream(TREE, [12, 18])))
add("trace", "trace_root_only_shared", lambda: trace1(tstream([-1, 0, 0, 1, 2, 3, 4], [5, 6])))
add("trace", "trace_deep_record_shared", lambda: trace1(tstream(TREE, [12, 14, 15])))
add("trace", "trace_highest_leaves_last", lambda: trace1(tstream(TREE, [15, 12, 14])))          # 15's chain leaves the common part at 11 > 9
add("trace", "trace_highest_leaves_first", lambda: trace1(tstream(TREE, [19, 12, 15])))         # 19's chain leaves it at 5, below the others
add("trace", "trace_tip_is_the_common_record", lambda: trace1(tstream(TREE, [9, 12, 14])))
add("trace", "trace_instance_without_path", lambda: trace1(tstream(TREE, [12, -1, 12])))
add("trace", "trace_no_instance", lambda: trace1(Stream(mk_paths(TREE), [[]], [[]])))
add("trace", "trace_later_token_has_the_path", lambda: trace1(Stream(mk_paths(TREE), [[(5, 0, [(LIVE, -1), (DEAD, 12), (LIVE, 14)]), (3, 0, [(LIVE, 15)])]], [[]])))
add("trace", "trace_frame_equals_last_frame", lambda: trace1(tstream(TREE, [12, 14], frames=np.arange(20) * 2), 18))       # record 9: frame 18
add("trace", "trace_frame_last_frame_plus_one", lambda: trace1(tstream(TREE, [12, 14], frames=np.arange(20) * 2), 17))
add("trace", "trace_records_of_one_frame", lambda: trace1(tstream(TREE, [12, 15], frames=np.int64([0, 0, 1, 1, 1, 2, 2, 2, 2, 3] + [3, 3] + [4] * 8)), 2))
for n_ in (1, 2, 15, 16, 17, 5000):
    add("trace", "trace_chain_%d_res_cap_16" % n_, functools.partial(chain_case, n_, 16))
add("trace", "trace_more_than_1024_tips", functools.partial(many_tips_case, 3, 16, 70))
add("trace", "trace_17_waves", functools.partial(many_tips_case, 6, 17, 5))
add("trace", "trace_33_waves", functools.partial(many_tips_case, 3, 33, 3))
add("trace", "trace_130_instances_in_a_wave_NE6", functools.partial(many_tips_case, 6, 2, 130))
add("trace", "trace_model_unlabelled_between_and_below", functools.partial(chain_case, 5, 64, 1, 2))
add("trace", "trace_model_export_res_cap", functools.partial(chain_case, 4, 12, 1, 2))            # 4 * 3 records from the last word record down
add("trace", "trace_model_export_res_cap_plus_1", functools.partial(chain_case, 4, 11, 1, 2))
add("trace", "trace_word_level_skips_unlabelled", functools.partial(chain_case, 5, 64, 0, 1))


def model_tips_case():
    """tips without a label: each stands for its nearest labelled ancestor"""
    labels = np.int64([3, 0, 4, 0, 0, 5, 0, 0, 0, 0])
    prev = [-1, 0, 1, 2, 3, 2, 5, 6, 4, 8]                  # 2 is common; tips 7 (-> 5) and 9 (-> 2)
    return trace1(tstream(prev, [7, 9], labels=labels), -1, 16, 1)


add("trace", "trace_model_unlabelled_tips", model_tips_case)
add("trace", "trace_model_only_unlabelled", lambda: trace1(tstream([-1, 0, 1], [2, 2], labels=np.int64([0, 0, 0])), -1, 16, 1))


def arrival_case(kind):
    """instances whose source state has an arrival key: the item it names comes before the tokens; dirty states are tips of their own"""
    items = [12, 14, 15, -1, 18]
    if kind == "key_overrides_tokens":                      # tokens say 18 (nothing shared), the entry tokens 12 and 14
        rec, arrival, dirty = [[(3, 0, [(LIVE, 18)]), (4, 4, [(LIVE, 18), (LIVE, -1)])]], [0, -1, -1, -1, 1, -1], [[]]
    elif kind == "key_without_path":                        # the item a key names has no path: the tokens are next
        rec, arrival, dirty = [[(3, 0, [(LIVE, 12)]), (3, 4, [(LIVE, 15)])]], [3, -1, -1, -1, 3, -1], [[]]
    elif kind == "dirty_tips":                              # states 0 and 5 have a model arc; 2 and 3 have not and do not count
        rec, arrival, dirty = [[(3, 1, [(LIVE, 12)])]], [1, -1, 4, 4, -1, 2], [[0, 2, 3, 5]]
    elif kind == "dirty_tip_without_key":                   # state 4 has a model arc and no key: an instance without a path
        rec, arrival, dirty = [[(3, 1, [(LIVE, 12)])]], [1, -1, -1, -1, -1, -1], [[0, 4]]
    s = Stream(mk_paths(TREE), rec, [items], dirty, arrival, n_states=6, dirty_nw=1)
    return Desc([s], [(TRACE, 0, -1, 16, 0)], cap_items=8, **GRAPH)


for k_ in ("key_overrides_tokens", "key_without_path", "dirty_tips", "dirty_tip_without_key"):
    add("trace", "trace_" + k_, functools.partial(arrival_case, k_))
for why_, kw_ in (("not_started", dict(started=0)), ("needs_init", dict(needs_init=1)), ("error", dict(error=-41))):
    add("trace", "trace_inactive_" + why_, functools.partial(lambda kw: trace1(tstream(TREE, [12, 14], **kw)), kw_))
add("trace", "trace_inactive_no_waves", lambda: trace1(Stream(mk_paths(TREE), [], [], lst_nw=0)))


def many_case():
    """three streams under k_partial_many; res_cap 40.  Chains of n word records with have such that n - have is 0, 1, a share, a share + 1,
    n < have, and n > res_cap"""
    def chain(n):
        return tstream(np.arange(n + 3) - 1, [n - 1, n + 1, n + 2], frames=np.arange(n + 3))     # the common record: n - 1
    out = []
    for name, ns, haves in (("0_1_share", (10, 10, 36), (10, 9, 36 - PARTIAL_SHARE)), ("share_plus_1_below_have_above_res_cap", (37, 5, 41), (4, 6, 20)),
                            ("above_res_cap_by_a_share", (40, 41, 39), (8, 41 - PARTIAL_SHARE, 39 - PARTIAL_SHARE - 1))):
        out.append((name, Desc([chain(n) for n in ns], [(TRACE_MANY, [(2, -1, haves[2]), (0, 3, haves[0]), (1, -1, haves[1])], 40)])))
    return out


for name_, D_ in many_case():
    add("trace", "trace_many_" + name_, functools.partial(lambda D: D, D_))
add("trace", "trace_many_one_inactive", lambda: Desc([tstream(TREE, [12, 14]), tstream(TREE, [12, 14], started=0), tstream(TREE, [12, 18])],
                                                     [(TRACE_MANY, [(0, -1, 0), (1, -1, 0), (2, -1, 0)], 16)]))


def trace_collect_trace():
    """a forest of which the collection drops most: the trace before and the trace after give the same answer"""
    rng = np.random.default_rng(77)
    n = 20000
    prev = forest(rng, n, 6)
    prev[10000:] = np.maximum(prev[10000:], 9999)            # everything from 10000 on descends from record 9999
    tips_ = 10000 + rng.integers(0, 10000, 12)
    s = tstream(prev, tips_, waves=4, frames=np.arange(n) // 4)
    return Desc([s], [(TRACE, 0, 100, 8192, 0), (COLLECT, 0, 3, 0, 0), (TRACE, 0, 100, 8192, 0)])


add("trace", "trace_collect_trace", trace_collect_trace)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name][1]()


def names(family):
    return [n for n, (f, _) in CASES.items() if f == family]


FAMILIES = ("sizes", "marks", "roots", "dirty", "geometry", "work", "counters", "trace")
