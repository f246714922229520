"""The Path collection and the partial trace off the GPU: (a) tests/paths_ref.py - what tests/test_gpu_paths.py holds the kernels of
juicer_amd/csrc/jd_gc.h to - against second formulations: per-root walks and the reference's own counting walk
(tracePartialPath, ++jointCount == nActiveInsts in instance order) on small random states, a single descending sweep over the arena
on the named cases; (b) every named case of tests/paths_cases.py has the shape it exists for, read off its arrays (ranges through a
restatement of gc_range); (c) jd_debug_paths' validation (juicer_amd/csrc/jd_paths.h) refuses what could lead a kernel out of an
arena, and its byte images are where a restatement of the kernels' addressing puts them - through tests/paths_driver.cpp, run
plain and under -fsanitize=address,undefined."""
import copy

import numpy as np
import pytest

import paths_cases as pc
import paths_ref as pr
from paths_cases import DEAD, GRAPH, LIVE, LIVE2, NINF, case, gc_range
from paths_ref import COLLECT, PARTIAL_SHARE, TRACE, TRACE_MANY, Desc, Stream

# ------------------------------------------------------------------ (a) second formulations


def brute_kept(D, s, sweep):
    """(kept, kept_ref) as sets.  sweep False: every root's walk to its end; True: the roots marked, then ONE pass from the newest record
    to the oldest that marks the predecessor of every marked record (a predecessor has the smaller index)"""
    ref_roots, other_roots = pr.roots(D, s)
    prev = s.paths[:, 0].tolist()
    out = []
    for start in (ref_roots, ref_roots + other_roots):
        if sweep:
            m = [False] * s.n_paths
            for q in start:
                if q >= 0:
                    m[q] = True
            for q in range(s.n_paths - 1, -1, -1):
                if m[q] and prev[q] >= 0:
                    m[prev[q]] = True
            out.append({q for q in range(s.n_paths) if m[q]})
        else:
            k = set()
            for q in start:
                while q >= 0:
                    k.add(q)
                    q = prev[q]
            out.append(k)
    return out[1], out[0]


def brute_collect(D, s, thr, path_rule, sweep=False):
    """collect_stream's second formulation, on a copy"""
    s = copy.deepcopy(s)
    n_ref, new_ref = (s.n_paths_ref, s.path_new_ref) if D.pcount else (s.n_paths, s.path_new)
    with np.errstate(divide="ignore", invalid="ignore"):
        fires = n_ref > 10000 and np.float32(n_ref) / np.float32(new_ref) > 12
    rule = bool(path_rule) and (thr < 0 or bool(fires))
    if not s.started or s.needs_init or s.error or s.lst_nw <= 0 or not (s.n_paths > thr or rule):
        s.gc = [0, 0, 0, int(rule)]
        return s
    kept, kept_ref = brute_kept(D, s, sweep)
    new = {q: i for i, q in enumerate(sorted(kept))}
    new[-1] = -1
    s.paths = np.int32([[new[int(r[0])]] + [int(x) for x in r[1:]] for q, r in enumerate(s.paths) if q in kept]).reshape(-1, 7)
    s.rec = [[(n, src, [(sc, p if p < 0 else new[p] if pr.is_live(sc) else -1) for sc, p in toks]) for n, src, toks in wave] for wave in s.rec]
    s.items = [[new[p] for p in wave] for wave in s.items]
    s.best_final = new[s.best_final]
    s.gc = [1, len(kept), len(kept_ref), int(rule)]
    s.path_new = len(kept)
    if not D.pcount or rule:
        s.n_collect += 1
    if D.pcount and rule:
        s.n_paths_ref = s.path_new_ref = len(kept_ref)
    return s


def same_stream(D, a, b):
    wa, wb = pr.stream_words(D, a)[0], pr.stream_words(D, b)[0]
    return wa.shape == wb.shape and bool((wa == wb).all())


def brute_trace(D, s, last_frame):
    """tracePartialPath (WFSTDecoderLite.cpp:824-868): every instance's walk counts its visits to the records newer than the last
    traced frame; the first record that all of them have visited is the answer.  -> its index, or None"""
    if not s.started or s.needs_init or s.error or s.lst_nw <= 0:
        return None
    tp = pr.tips(D, s)
    paths = s.paths
    if not tp or any(pr.word_rec(paths, t) < 0 for t in tp):
        return None
    count = {}
    for t in tp:
        q = pr.word_rec(paths, t)
        while q >= 0:
            if paths[q, 1] > last_frame:
                count[q] = count.get(q, 0) + 1
                if count[q] == len(tp):
                    return q
            q = pr.word_rec(paths, paths[q, 0])
    return None


def random_state(seed):
    rng = np.random.default_rng(seed)
    NE = int(rng.choice([3, 6]))
    n = int(rng.integers(0, 60))
    back = int(rng.choice([1, 2, 5, 60]))
    prev = pc.forest(rng, n, back)
    labels = np.where(rng.random(n) < 0.7, 1 + rng.integers(0, 50, n), 0) if seed % 3 == 0 else None
    frames = np.sort(rng.integers(0, max(n // 2, 1), n))
    waves = int(rng.integers(1, 4))
    path = lambda lo=0.3: int(rng.integers(0, n)) if n and rng.random() > lo else -1
    rec = []
    for w in range(waves):
        wave = []
        for _ in range(int(rng.integers(0, 4))):
            ns = int(rng.integers(3, NE + 3))
            wave.append((ns, int(rng.integers(0, 6)), [(int(rng.choice([LIVE, LIVE2, DEAD, NINF])), path()) for _ in range(ns - 2)]))
        rec.append(wave)
    items = [[path() for _ in range(int(rng.integers(0, 4)))] for _ in range(waves)]
    cap_items = 4 * waves
    written = [w * 4 + k for w in range(waves) for k in range(len(items[w]))]
    arrival = [int(rng.choice(written)) if written and rng.random() < 0.4 else -1 for _ in range(6)]
    dirty_nw = int(rng.integers(0, 3))
    dirty = [[int(x) for x in rng.integers(0, 6, int(rng.integers(0, 3)))] for _ in range(dirty_nw if dirty_nw else waves)]
    s = Stream(pc.mk_paths(prev, frames, labels), rec, items, dirty, arrival, n_states=6, dirty_nw=dirty_nw, best_final=path(0.5),
               n_paths_ref=int(rng.integers(0, 100)), path_new_ref=int(rng.integers(0, 5)), n_collect=int(rng.integers(0, 3)))
    return Desc([s], [], NE=NE, pcount=int(rng.integers(0, 2)), cap_items=cap_items, cap_new=8, **GRAPH), rng


def test_reference_against_brute_force_on_random_states():
    n_found = n_active = 0
    for seed in range(400):
        D, rng = random_state(seed)
        s = D.streams[0]
        assert pc.encode(D).dtype == np.int32
        for last_frame in (-1, int(rng.integers(0, 20))):
            want = brute_trace(D, s, last_frame)
            assert pr.trace_answer(D, s, last_frame) == want, seed
            n_found += want is not None
        thr, rule = int(rng.choice([-1, 0, 10, 100])), int(rng.integers(0, 2))
        want = brute_collect(D, s, thr, rule)
        got = copy.deepcopy(s)
        pr.collect_stream(D, got, thr, rule)
        assert same_stream(D, got, want), seed
        assert same_stream(D, got, brute_collect(D, s, thr, rule, sweep=True)), seed
        n_active += got.gc[0]
        # the collection keeps the order of the records: the trace is the same afterwards (where no dead token has a path - the trace
        # takes an instance's first token with a path whatever its score, and the collection clears a dead token's)
        if got.gc[0] and not any(p >= 0 and not pr.is_live(sc) for w in s.rec for _, _, t in w for sc, p in t):
            a, b = pr.trace_stream(D, s, -1, 8, 1)[0], pr.trace_stream(D, got, -1, 8, 1)[0]
            assert (a == b).all(), seed
    assert n_found > 60 and n_active > 200


SWEEP_FAMILIES = ("marks", "roots", "dirty", "geometry", "work", "counters")


@pytest.mark.parametrize("family", SWEEP_FAMILIES + ("sizes",))
def test_reference_against_the_sweep_on_named_cases(family):
    """every collection of the named cases (of the size family: the arenas up to 2^15 + 1 records and three of the large ones)"""
    n = 0
    for name in pc.names(family):
        D = copy.deepcopy(case(name))
        if family == "sizes" and D.streams[0].n_paths > 32769 and name not in ("size_140003_G5_second", "size_131073_G1_chain", "size_131072_G32_stride"):
            continue
        for op in D.ops:
            assert op[0] == COLLECT
            for si in ([op[1]] if isinstance(op[1], int) else op[1]):
                want = brute_collect(D, D.streams[si], op[3], op[4], sweep=True)
                pr.collect_stream(D, D.streams[si], op[3], op[4])
                assert same_stream(D, D.streams[si], want), name
                n += 1
    assert n >= len(pc.names(family)) // 2


def test_trace_cases_against_the_counting_walk():
    for name in pc.names("trace"):
        D = copy.deepcopy(case(name))
        for op in D.ops:
            if op[0] == COLLECT:
                pr.collect_stream(D, D.streams[op[1]], op[3], op[4])
                continue
            for si, last_frame in ([(op[1], op[2])] if op[0] == TRACE else [(e[0], e[1]) for e in op[1]]):
                assert pr.trace_answer(D, D.streams[si], last_frame) == brute_trace(D, D.streams[si], last_frame), name


# ------------------------------------------------------------------ (b) the cases have the shapes they exist for

def scan_trips(n, G):
    """per workgroup: (records, trips of k_gc_scan's loop)"""
    return [(hi - lo, -(-(hi - lo) // 4096)) for lo, hi in (gc_range(n, G, b) for b in range(G))]


def kept_mask(D, si=0):
    s = D.streams[si]
    kept, _ = brute_kept(D, s, True)
    m = np.zeros(s.n_paths, bool)
    m[list(kept)] = True
    return m


def test_gc_range_restatement():
    for n, G in pc.SIZE_PAIRS:
        r = [gc_range(n, G, b) for b in range(G)]
        assert r[0][0] == 0 and r[-1][1] == n and all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert all(lo % 1024 == 0 or lo == n for lo, _ in r) and all((hi - lo) % 1024 == 0 for lo, hi in r if hi < n)


def test_size_cases_cover_what_they_must():
    got = set()
    sizes = set()
    for name in pc.names("sizes"):
        D = case(name)
        (op,) = D.ops
        n, G = D.streams[0].n_paths, op[2]
        sizes.add(n)
        assert (n, G) in pc.SIZE_PAIRS and op[1] == 0
        trips = scan_trips(n, G)
        kept = kept_mask(D)
        per = [r for r, _ in trips]
        for b, (r, t) in enumerate(trips):
            lo, hi = gc_range(n, G, b)
            carry = int(kept[lo:lo + 4096 * (t - 1)].sum()) if t > 1 else 0
            if t == 2 and carry:
                got.add("two trips with a carry")
            if t == 3 and carry and kept[lo:lo + 4096].any() and kept[lo + 4096:lo + 8192].any():
                got.add("three trips with a carry")
            if r > 8192:
                got.add("a range above 8192")
            if r == 4096:
                got.add("a range of 4096")
            if r == 1024:
                got.add("a range of 1024")
            if r & 3 and kept[hi - (r & 3):hi].any():
                last = all(x == 0 for x in per[b + 1:])
                assert last
                got.add("tail %d %s" % (r & 3, "in the last workgroup" if b == G - 1 else "in a middle workgroup") + (" behind a trip" if t > 1 else ""))
        if G > 1 and per[-1] == 0 and per[0] > 0:
            got.add("empty ranges, G %d" % G)
        if G > 1 and 0 < per[-1] < per[0]:
            got.add("a shorter last range")
        if G == 1 and n > 4096:
            got.add("G 1 holds everything")
        if kept.all() and n > 100000 and (D.streams[0].paths[1:, 0] == np.arange(n - 1)).all():
            got.add("one chain through everything")
        if name.endswith("_stride") and gc_range(n, G, 0)[1] == 1024:
            prev = D.streams[0].paths[:, 0]
            q = np.flatnonzero(kept & (prev >= 0))
            assert q.size > 1000 and (prev[q] == q - 1025).all() and (q // 1024 != prev[q] // 1024).all()
            got.add("every predecessor in another range")
    want = ["two trips with a carry", "three trips with a carry", "a range above 8192", "a range of 4096", "a range of 1024",
            "tail 1 in the last workgroup", "tail 3 in the last workgroup", "tail 2 in a middle workgroup", "tail 1 in a middle workgroup",
            "tail 3 in the last workgroup behind a trip", "tail 1 in the last workgroup behind a trip", "tail 2 in the last workgroup behind a trip",
            "empty ranges, G 32", "empty ranges, G 31", "a shorter last range", "G 1 holds everything", "one chain through everything",
            "every predecessor in another range"]
    assert [w for w in want if w not in got] == []
    assert sizes == set(pc.SIZES + pc.EXTRA_SIZES)
    assert {G for _, G in pc.SIZE_PAIRS} == {1, 2, 3, 5, 31, 32}


def test_mark_cases_cover_what_they_must():
    for name, want in (("marks_before_second_trip_0", 0), ("marks_before_second_trip_1", 1), ("marks_before_second_trip_4096", 4096)):
        D = case(name)
        n, G = D.streams[0].n_paths, D.ops[0][2]
        kept = kept_mask(D)
        assert scan_trips(n, G)[0][1] == 3 and int(kept[:4096].sum()) == want and kept[4096:].any(), name
    for name, want in (("marks_lower_workgroups_0", 0), ("marks_lower_workgroups_full", 4096)):
        D = case(name)
        n, G = D.streams[0].n_paths, D.ops[0][2]
        lo, hi = gc_range(n, G, G - 1)
        kept = kept_mask(D)
        assert hi - lo > 0 and gc_range(n, G, 0) == (0, 4096) and int(kept[:lo].sum()) in (want, 2 * want) and int(kept[:4096].sum()) == want, name
        assert kept[lo:hi].any(), name
    D = case("marks_one_middle_range")
    lo, hi = gc_range(32769, 5, 2)
    kept = kept_mask(D)
    assert 0 < lo < hi < 32769 and kept[lo:hi].all() and kept.sum() == hi - lo
    for share in (1, 50, 99):
        kept = kept_mask(case("forest_%d_percent" % share))
        assert abs(kept.mean() - share / 100.0) < 0.02, share
    assert kept_mask(case("forest_1_percent_140003")).mean() < 0.03 and kept_mask(case("forest_99_percent_140003")).mean() >= 0.99
    every = {m: [case(n) for n in pc.names("sizes") if n.endswith("_" + m)] for m in ("none", "first", "last", "second", "chain")}
    assert all(len(v) >= 3 for v in every.values())
    for D in every["none"]:
        assert not kept_mask(D).any()
    for D in every["first"]:
        assert np.flatnonzero(kept_mask(D)).tolist() == [0]
    for D in every["last"]:
        assert np.flatnonzero(kept_mask(D)).tolist() == [D.streams[0].n_paths - 1]
    for D in every["second"]:
        n = D.streams[0].n_paths
        assert np.flatnonzero(kept_mask(D)).tolist() == list(range((n - 1) % 2, n, 2))
    for D in every["chain"]:
        assert kept_mask(D).all()


def test_root_and_dirty_cases_cover_what_they_must():
    D = case("roots_shared_long_chains")
    s = D.streams[0]
    ref_roots, others = pr.roots(D, s)
    # an item below a token on one chain, a token below an item on the other, and one record that is both
    assert 1500 in others and 2999 in ref_roots and 4000 in ref_roots and 5999 in others and 5999 in ref_roots
    _, kept_ref = brute_kept(D, s, False)
    assert len(kept_ref) == 6000
    s = case("roots_same_root_many_times").streams[0]
    assert sum(p == 4321 for w in s.rec for _, _, t in w for _, p in t) == 700 and sum(p == 4321 for w in s.items for p in w) == 900
    s = case("roots_dead_token_with_path").streams[0]
    toks = [t for w in s.rec for _, _, ts in w for t in ts]
    assert (DEAD, 5999) in toks and (NINF, 5000) in toks and (LIVE2, 300) in toks and (DEAD, 100) in toks and (LIVE, 100) in toks
    kept, _ = brute_kept(case("roots_dead_token_with_path"), s, False)
    assert 5999 not in kept and 5000 not in kept and 300 in kept and 100 in kept
    got = copy.deepcopy(s)
    pr.collect_stream(case("roots_dead_token_with_path"), got, 0, 0)
    assert [p for w in got.rec for _, _, ts in w for sc, p in ts if not pr.is_live(sc)] == [-1, -1, -1, -1]
    s = case("roots_best_final_only").streams[0]
    assert s.best_final == 5998 and all(p < 0 for p in pr.roots(case("roots_best_final_only"), s)[0]) and all(p < 0 for w in s.items for p in w)
    assert case("roots_best_final_minus_one").streams[0].best_final == -1
    assert any(len(t) < D.NE for D in (case("geometry_nw1_G1_NE6"),) for w in D.streams[0].rec for _, _, t in w)      # sentinel slots
    # the dirty-list roots
    D = case("dirty_base")
    s = D.streams[0]
    assert D.pcount and [D.has_model(st) for st in range(6)] == [True, True, False, False, True, True]
    assert D.row_ptr[3] == D.row_ptr[4] and s.arrival[4] == -1 and all(D.arc_in[a] & pr.ARC_FLAGS for a in (2, 4, 5))
    assert sorted(st for w in s.dirty for st in w) == [0, 0, 1, 2, 3, 4, 5]
    kept, kept_ref = brute_kept(D, s, False)
    assert {2999, 2500, 500} <= kept_ref and 2000 not in kept_ref and 1500 not in kept_ref and {2000, 1500} <= kept
    _, kept_ref0 = brute_kept(case("dirty_without_pcount"), case("dirty_without_pcount").streams[0], False)
    assert 2999 not in kept_ref0
    assert case("dirty_other_wave_count").streams[0].dirty_nw == 5 != case("dirty_other_wave_count").streams[0].lst_nw
    assert case("dirty_dirty_nw_0").streams[0].dirty_nw == 0 and len(case("dirty_dirty_nw_0").streams[0].dirty) == 2


def test_geometry_work_and_counter_cases_cover_what_they_must():
    seen = set()
    for name in pc.names("geometry"):
        D = case(name)
        s, G = D.streams[0], D.ops[0][2]
        seen.add((s.lst_nw, G))
        seen.add("NE %d" % D.NE)
        seen |= {"inst %d" % len(w) for w in s.rec} | {"items %d" % len(w) for w in s.items}
        seen |= {"nStates %d NE %d" % (n, D.NE) for w in s.rec for n, _, _ in w}
        if s.lst_nw > 16 * G and any(s.rec[w] or s.items[w] for w in range(16 * G, s.lst_nw)):
            seen.add("waves beyond 16 G, G %d" % G)
        assert D.cap_slots // s.lst_nw // 64 * 64 >= max(len(w) for w in s.rec) and D.cap_items // s.lst_nw >= max(len(w) for w in s.items)
    want = [(nw, G) for nw in (1, 16, 17, 33, 512) for G in (1, 2)] + ["NE 3", "NE 6", "waves beyond 16 G, G 1", "waves beyond 16 G, G 2"] + \
        ["inst %d" % k for k in (0, 1, 63, 64, 65, 130)] + ["items %d" % k for k in (0, 1, 64, 65)] + \
        ["nStates %d NE 3" % k for k in (3, 4, 5)] + ["nStates %d NE 6" % k for k in (3, 4, 5, 6, 7, 8)]
    assert [w for w in want if w not in seen] == []
    # work lists: three and four streams of different sizes, one inactive for each reason
    reasons = set()
    for name in pc.names("work"):
        D = case(name)
        (op,) = D.ops
        if isinstance(op[1], int):
            assert op[1] == 1 and len(D.streams) == 2
            continue
        if name == "work_not_started_while_the_host_asks":
            words, what = pr.run(D)
            at = [i for i in range(len(words)) if what(i).startswith("stream 1 head")]
            assert list(words[at[6:10]]) == [0, 0, 0, 1] and not D.streams[1].started and op[3] < 0 and op[4] == 1
            continue
        assert len({s.n_paths for s in D.streams}) == len(D.streams)
        for si in op[1]:
            s = D.streams[si]
            if not pr.is_active(D, s, op[3], False):
                reasons.add((len(op[1]), "not_started" if not s.started else "needs_init" if s.needs_init else "error" if s.error else
                             "no_waves" if s.lst_nw <= 0 else "below_threshold"))
    assert {r for _, r in reasons} == set(pc.INACTIVE) and {k for k, _ in reasons} == {3, 4}
    assert len(case("work_part_of_the_streams").ops[0][1]) == 2 and len(case("work_part_of_the_streams").streams) == 3
    # counters: the three outcomes, the threshold either side, the rule either side
    outcome = {}
    for name in pc.names("counters"):
        D = copy.deepcopy(case(name))
        s = D.streams[0]
        before = (s.n_collect, s.n_paths_ref, s.path_new_ref)
        pr.collect_stream(D, s, D.ops[0][3], D.ops[0][4])
        outcome[name] = (s.gc[0], s.gc[3], s.n_collect - before[0], (s.n_paths_ref, s.path_new_ref) != before[1:])
    assert outcome["counters_own_records"] == (1, 0, 1, False)
    assert outcome["counters_threshold_at_n_paths"] == (0, 0, 0, False)
    assert outcome["counters_threshold_at_n_paths_rule_off"] == (0, 0, 0, False) and outcome["counters_threshold_at_n_paths_rule_fires"] == (1, 1, 1, False)
    assert outcome["counters_threshold_minus_one"] == (1, 1, 1, False) and outcome["counters_threshold_minus_one_rule_off"] == (1, 0, 1, False)
    assert outcome["counters_ref_rule_fires"] == (1, 1, 1, True) and outcome["counters_ref_rule_10001_first"] == (1, 1, 1, True)
    assert outcome["counters_ref_rule_at_12"] == (1, 0, 0, False) and outcome["counters_ref_rule_10000"] == (1, 0, 0, False)
    assert outcome["counters_ref_host_asks"] == (1, 1, 1, True)
    assert outcome["counters_ref_rule_only_inactive"] == (0, 0, 0, False) and outcome["counters_ref_rule_only_active"] == (1, 1, 1, True)
    assert pr.path_rule_fires(10001, 0) and pr.path_rule_fires(12001, 1000) and not pr.path_rule_fires(12000, 1000) and not pr.path_rule_fires(10000, 1)
    D = copy.deepcopy(case("two_collections_in_a_row"))
    s = D.streams[0]
    pr.collect_stream(D, s, 0, 0)
    first = copy.deepcopy(s)
    pr.collect_stream(D, s, 0, 0)
    assert 0 < first.n_paths < 32769 and (s.paths == first.paths).all() and s.rec == first.rec and s.n_collect == first.n_collect + 1


def test_trace_cases_cover_what_they_must():
    def one(name):
        D = case(name)
        op = D.ops[0]
        s = D.streams[op[1]]
        return D, s, op, pr.trace_stream(D, s, op[2], op[3], op[4])[0]
    found = lambda name: int(one(name)[3][0])
    assert found("trace_one_tip") and found("trace_all_tips_equal") and not found("trace_nothing_shared")
    D, s, op, o = one("trace_root_only_shared")
    assert o[0] == 1 and o[1] == 1 and pr.trace_answer(D, s, -1) == 0
    assert pr.trace_answer(*one("trace_deep_record_shared")[:2], -1) == 9
    for name, tips in (("trace_highest_leaves_last", [15, 12, 14]), ("trace_highest_leaves_first", [19, 12, 15])):
        D, s, _, _ = one(name)
        assert pr.tips(D, s) == tips and max(tips) == tips[0]
    high, others = pr.word_chain(s.paths, 19), [pr.word_chain(s.paths, t) for t in (12, 15)]
    assert pr.trace_answer(D, s, -1) == 5 == max(set(high) & set(others[0])) and max(set(others[0]) & set(others[1])) == 11
    D, s, _, _ = one("trace_highest_leaves_last")
    assert pr.trace_answer(D, s, -1) == 9 and max(set(pr.word_chain(s.paths, 15)) & set(pr.word_chain(s.paths, 12))) == 11
    D, s, _, _ = one("trace_tip_is_the_common_record")
    assert pr.trace_answer(D, s, -1) == 9 in pr.tips(D, s)
    assert -1 in pr.tips(*one("trace_instance_without_path")[:2]) and not found("trace_instance_without_path")
    assert pr.tips(*one("trace_no_instance")[:2]) == [] and not found("trace_no_instance")
    D, s, _, _ = one("trace_later_token_has_the_path")
    assert s.rec[0][0][2][0][1] == -1 and not pr.is_live(s.rec[0][0][2][1][0]) and pr.tips(D, s) == [12, 15] and found("trace_later_token_has_the_path")
    # the found record's frame against last_frame
    for name, want in (("trace_frame_equals_last_frame", 0), ("trace_frame_last_frame_plus_one", 1)):
        D, s, op, o = one(name)
        ans = pr.trace_answer(D, s, -1)
        assert s.paths[ans, 1] - op[2] == want and o[0] == want, name
    D, s, op, o = one("trace_records_of_one_frame")
    assert o[0] == 1 and len(set(s.paths[pr.word_chain(s.paths, 11), 1])) < len(pr.word_chain(s.paths, 11))
    # chains around res_cap
    for n in (1, 2, 15, 16, 17, 5000):
        D, s, op, o = one("trace_chain_%d_res_cap_16" % n)
        assert op[3] == 16 and o[0] == 1 and o[1] == n and int((o[3:19] != D.sentinel).sum()) == min(n, 16)
    for name, waves, tips in (("trace_more_than_1024_tips", 16, 1025), ("trace_17_waves", 17, 17), ("trace_33_waves", 33, 33), ("trace_130_instances_in_a_wave_NE6", 2, 260)):
        D, s, op, o = one(name)
        assert s.lst_nw == waves and len(pr.tips(D, s)) >= tips and o[0] == 1 and o[1] == 2000 and all(s.rec), name
    assert max(len(w) for w in one("trace_130_instances_in_a_wave_NE6")[1].rec) == 130 and one("trace_130_instances_in_a_wave_NE6")[0].NE == 6
    assert {case(n).NE for n in pc.names("trace")} == {3, 6}
    # model level
    D, s, op, o = one("trace_model_unlabelled_between_and_below")
    assert op[4] == 1 and s.paths[0, 2] == 0 and s.paths[-1, 2] == 0 and o[1] == 5 and o[2] == 15 and (s.paths[:, 2] == 0).sum() == 12
    for name, fits in (("trace_model_export_res_cap", True), ("trace_model_export_res_cap_plus_1", False)):
        D, s, op, o = one(name)
        assert o[2] == op[3] + (0 if fits else 1) and o[0] == 1 and bool((o[3 + 2 * op[3]:] != D.sentinel).all()) == fits, name
        assert fits or (o[3 + 2 * op[3]:] == D.sentinel).all()
    D, s, op, o = one("trace_model_unlabelled_tips")
    assert all(s.paths[t, 2] == 0 for t in pr.tips(D, s)) and o[0] == 1 and o[1] == 2 and o[2] == 3
    assert not found("trace_model_only_unlabelled")
    # arrival keys and dirty-list tips
    D, s, _, _ = one("trace_key_overrides_tokens")
    assert pr.tips(D, s) == [12, 14] and all(t[0][1] == 18 for _, _, t in s.rec[0]) and found("trace_key_overrides_tokens")
    assert pr.tips(*one("trace_key_without_path")[:2]) == [12, 15]
    assert pr.tips(*one("trace_dirty_tips")[:2]) == [12, 14, 15] and found("trace_dirty_tips")
    assert pr.tips(*one("trace_dirty_tip_without_key")[:2]) == [12, 14, -1]
    for name in pc.names("trace"):
        if name.startswith("trace_inactive_"):
            D, s, op, o = one(name)
            assert o[0] == 0 and o[1] == 0 and (o[2:] == D.sentinel).all(), name
    assert len([n for n in pc.names("trace") if n.startswith("trace_inactive_")]) == 4
    # k_partial_many: n - have at 0, 1, a share and a share + 1, n below have, n above res_cap
    seen = set()
    for name in pc.names("trace"):
        if not name.startswith("trace_many_"):
            continue
        D = case(name)
        (_, entries, res_cap), = D.ops
        assert len(entries) == 3 == len(D.streams)
        buf = pr.trace_many(D, entries, res_cap)
        for i, (si, last_frame, have) in enumerate(entries):
            n = pr.trace_stream(D, D.streams[si], last_frame, res_cap, 0)[1]
            stage = buf[6 + 2 * PARTIAL_SHARE * i:6 + 2 * PARTIAL_SHARE * (i + 1)]
            staged = int((stage != D.sentinel).sum()) // 2
            seen.add(("n - have %d" % (n - have) if n >= have else "n < have") + (", n > res_cap" if n > res_cap else "") + (": staged" if staged else ""))
            assert staged in (0, n - have)
    want = ["n - have 0", "n - have 1: staged", "n - have %d: staged" % PARTIAL_SHARE, "n - have %d" % (PARTIAL_SHARE + 1), "n < have",
            "n - have %d, n > res_cap" % PARTIAL_SHARE]
    assert [w for w in want if w not in seen] == [], seen
    # the collection between two traces drops most records and changes nothing of the answer
    D = copy.deepcopy(case("trace_collect_trace"))
    assert [op[0] for op in D.ops] == [TRACE, COLLECT, TRACE] and D.ops[0] == D.ops[2]
    words, _ = pr.run(D)
    k = 3 + 8 * D.ops[0][3]
    assert (words[-2 * k:-k] == words[-k:]).all() and words[-k] == 1 and words[-k + 1] > 1000
    assert words[0] < D.streams[0].n_paths // 2


# ------------------------------------------------------------------ (c) the validation and the byte images, through the driver

def small():
    """a state with a little of everything: two waves, items, arrival keys, a dirty list, two operations"""
    s = Stream(pc.mk_paths(pc.TREE), [[(3, 0, [(LIVE, 12)]), (5, 4, [(DEAD, 3), (LIVE, -1), (LIVE, 14)])], [(4, 5, [(LIVE, 15), (LIVE, 2)])]],
               [[12, -1, 14], [18]], [[0, 5], [3]], [0, -1, 2, -1, 4, -1], n_states=6, dirty_nw=2, best_final=17, frame=7, cap_paths=32)
    return Desc([s, copy.deepcopy(s)], [(COLLECT, [1, 0], 2, 0, 1), (TRACE, 0, -1, 8, 1), (TRACE_MANY, [(1, -1, 0)], 8)], cap_items=8, cap_new=6,
                pcount=1, **GRAPH)


def edit(f):
    D = small()
    f(D)
    return pc.encode(D)


def set_word(D, attr, v):
    setattr(D.streams[0], attr, v)


def refusals():
    def prev(D): D.streams[0].paths[5, 0] = 5
    def prev2(D): D.streams[1].paths[0, 0] = -2
    def tok(D): D.streams[0].rec[0][0] = (3, 0, [(LIVE, 20)])
    def tok2(D): D.streams[0].rec[1][0] = (4, 5, [(LIVE, 15), (DEAD, -2)])
    def item(D): D.streams[0].items[1][0] = 20
    def arrival(D): D.streams[0].arrival[1] = 3          # wave 0 holds three items: 0, 1, 2
    def arrival2(D): D.streams[0].arrival[1] = 5         # wave 1 (from 4) holds one
    def arrival3(D): D.streams[0].arrival[1] = 8
    def dirty(D): D.streams[0].dirty[1][0] = 6
    def src(D): D.streams[0].rec[0][0] = (3, 6, [(LIVE, 12)])
    def nstates(D): D.streams[0].rec[0][0] = (6, 0, [(LIVE, 12)] * 4)
    def nstates2(D): D.streams[0].rec[0][0] = (2, 0, [])
    def insts(D): D.cap_slots, D.streams[0].rec[0] = 128, [(3, 0, [(LIVE, 1)])] * 65
    def items(D): D.cap_items = 5                          # segments of two items
    def dirties(D): D.cap_new = 3
    def ops(kind):
        def f(D): D.ops = [kind]
        return f
    def five(D): D.streams += [copy.deepcopy(D.streams[0]) for _ in range(3)]
    def big(D): D.streams[0].cap_paths = (1 << 18) + 1
    return [("prev", prev), ("prev", prev2), ("token's path", tok), ("token's path", tok2), ("item's path", item), ("not written", arrival),
            ("not written", arrival2), ("not written", arrival3), ("outside the graph", dirty), ("source state", src), ("nStates", nstates),
            ("nStates", nstates2), ("instances beyond", insts), ("items beyond", items), ("states beyond", dirties),
            ("best_final", lambda D: set_word(D, "best_final", 20)), ("best_final", lambda D: set_word(D, "best_final", -2)),
            ("n_paths", lambda D: set_word(D, "cap_paths", 19)), ("an arena of", big), ("G 0", ops((COLLECT, 0, 0, 0, 0))),
            ("G 33", ops((COLLECT, 0, 33, 0, 0))), ("NE", lambda D: setattr(D, "NE", 4)), ("res_cap", ops((TRACE, 0, -1, 0, 0))),
            ("res_cap", ops((TRACE_MANY, [(0, -1, 0)], 0))), ("streams", five), ("bad stream", ops((TRACE, 2, -1, 8, 0))),
            ("twice", ops((COLLECT, [0, 0], 1, 0, 0))), ("frame", lambda D: set_word(D, "frame", -1)),
            ("MAXW", lambda D: set_word(D, "lst_nw", 513))]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return pc.build_driver(str(tmp_path_factory.mktemp("paths") / "paths_driver"))


def lines():
    """the refusals, the accepted description they are edits of, cut and lengthened descriptions, and the small named cases"""
    ok = pc.encode(small())
    cut = [ok[:k] for k in (0, 5, 12, 30, 40, len(ok) // 2, len(ok) - 1)] + [np.concatenate([ok, np.int32([0])])]
    named = [pc.encode(case(n)) for n in pc.CASES if case(n).streams[0].n_paths <= 6000 and case(n).streams[0].lst_nw <= 33]
    return [edit(f) for _, f in refusals()] + cut + [ok] + named


def test_validation_refuses_what_would_leave_an_arena(driver):
    res = pc.run_driver(driver, lines())
    n = len(refusals())
    for (what, _), (rc, _, msg) in zip(refusals(), res):
        assert rc == -1 and what in msg, (what, msg)
    assert all(rc == -1 for rc, _, _ in res[n:n + 8])
    assert all(rc == 0 for rc, _, _ in res[n + 8:]) and len(res) > n + 60
    # room is asked for what comes back when no collection shrinks an arena
    D = small()
    D.ops = D.ops[1:]
    assert res[n + 8][1][0] == pr.run(D)[0].shape[0] > pr.run(small())[0].shape[0]


def images(D, s):
    """a stream's images by a restatement of the kernels' addressing (jd_gc.h: k_gc_mark, jd_for_each_tip): bytes, viewed as words"""
    p = s.frame & 1
    HF = 2 if D.NE == 3 else 3
    rec_bytes, chunk = (HF + D.NE) * 16, (HF + D.NE) * 1024
    rec = np.zeros(2 * D.cap_slots * rec_bytes // 4, np.int32)
    items = np.zeros(2 * D.cap_items * 8, np.int32)
    dirtyl = np.zeros(2 * D.cap_new, np.int32)
    tot, item_end = np.zeros(10 * 512, np.int32), np.zeros(512, np.int32)
    srec = np.zeros(D.n_states * 8, np.int32)
    nw = s.lst_nw
    seg_rec, seg_item = (D.cap_slots // nw) & ~63, D.cap_items // nw
    for w in range(nw):
        seg = p * D.cap_slots * rec_bytes + w * (seg_rec >> 6) * chunk
        for q, (n, src, toks) in enumerate(s.rec[w]):
            r = seg + (q >> 6) * chunk + (q & 63) * 16
            rec[r // 4:r // 4 + 4] = [0, n, src, 0]
            for j in range(1, D.NE + 1):
                t = (r + (HF + j - 1) * 1024) // 4
                rec[t:t + 4] = [toks[j - 1][0], 0, 0, toks[j - 1][1]] if j < n - 1 else [D.sentinel] * 4
        tot[(0 + p) * 512 + w] = len(s.rec[w])
        for k, path in enumerate(s.items[w]):
            items[(2 * ((p ^ 1) * D.cap_items + w * seg_item + k)) * 4 + 3] = path
        item_end[w] = len(s.items[w])
    dn = len(s.dirty)
    for w in range(dn):
        for k, st in enumerate(s.dirty[w]):
            dirtyl[(p ^ 1) * D.cap_new + w * (D.cap_new // dn) + k] = st
        tot[(3 + (p ^ 1)) * 512 + w] = len(s.dirty[w])
    for st in range(D.n_states):                           # SREC_E_OFF, split8: srec_arr 16 n, srec_par 8 n, srec_estride 8
        if s.arrival[st] >= 0:
            at = (16 * D.n_states + (p ^ 1) * 8 * D.n_states + st * 8) // 4
            srec[at:at + 2] = [s.arrival[st], np.int32(-0x40000000)]
    paths = np.zeros((s.cap_paths, 8), np.int32)
    paths[:s.n_paths, :7] = s.paths
    words, _, _ = pr.stream_words(D, s)
    n_tok = sum(len(w) for w in s.rec) * D.NE
    n_it = sum(len(w) for w in s.items)
    at = 10 + 7 * s.n_paths
    return [rec, srec, items, dirtyl, tot, item_end, paths.reshape(-1), words[at:at + n_tok], words[at + n_tok:at + n_tok + n_it]]


def test_images_are_where_the_kernels_read_them(driver):
    names = ["small"] + [n for n in pc.CASES if case(n).streams[0].n_paths <= 6000 and 0 < case(n).streams[0].lst_nw <= 33]
    descs = [small()] + [case(n) for n in names[1:]]
    res = pc.run_driver(driver, [pc.encode(D) for D in descs])
    assert len(descs) > 60
    odd = [D for D in descs if D.streams[0].frame & 1]
    assert odd and len(odd) < len(descs)                   # both frame parities
    for name, D, (rc, v, _) in zip(names, descs, res):
        assert rc == 0, name
        want = [pc.checksum(img) for s in D.streams for img in images(D, s)]
        assert v[1:] == want, (name, [i for i, (a, b) in enumerate(zip(v[1:], want)) if a != b])


def test_paths_driver_under_sanitizers(driver, tmp_path_factory):
    san = pc.build_driver(str(tmp_path_factory.mktemp("paths_san") / "paths_driver_san"),
                          ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    L = lines()
    assert pc.run_driver(san, L) == pc.run_driver(driver, L)
