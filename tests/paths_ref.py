"""The Path collection and the PARTIAL_DECODING trace, written from their definitions (collectPaths and tracePartialPath of the
reference decoder, and what juicer_amd/csrc/jd_gc.h says it keeps beyond them) with numpy and plain loops - what
jd_debug_paths' device results are held to, word for word (tests/test_gpu_paths.py), and what tests/test_paths_ref_cpu.py holds to a
second, brute-force formulation.

A state is a Desc: a tiny graph, the arena capacities and one to four Stream objects; run(desc) applies the description's
operations to a copy and returns the words jd_debug_paths returns, in its order, with a name for every word."""
import copy
import functools

import numpy as np

LZ = np.float32(-3.402823466e+38)            # LOG_ZERO
ARC_FLAGS = 0x60000000                       # TEE_FLAG | SOLE_FLAG of a device arc's in-label
PARTIAL_SHARE = 32
MAXW = 512
COLLECT, TRACE, TRACE_MANY = 1, 2, 3
PATH_FIELDS = ("prev", "frame", "label", "model", "score", "ac", "lm")


def f2i(x):
    """the bits of a float32, as the int32 word of a description"""
    return int(np.float32(x).view(np.int32))


@functools.lru_cache(maxsize=None)
def is_live(score_bits):
    """score > LZ, on the bits of a float32"""
    return bool(np.int32(score_bits).view(np.float32) > LZ)


class Stream:
    """One stream: the flags and counters of its control block, its Path arena (n x 7 int32: PATH_FIELDS, floats as bits), per
    state the item its arrival key names (-1: no key), and by writer wave its instances [(nStates, source state, [(score bits,
    path)] * (nStates - 2))], the paths of its last frame's items and, by the dirty list's own waves, its dirty states."""

    def __init__(self, paths, rec, items, dirty=None, arrival=None, *, n_states=1, started=1, needs_init=0, error=0, frame=8, path_new=0,
                 n_collect=0, n_paths_ref=0, path_new_ref=0, best_final=-1, lst_nw=None, dirty_nw=0, cap_paths=None):
        self.paths = np.ascontiguousarray(paths, np.int32).reshape(-1, 7)
        self.rec, self.items = rec, items
        self.lst_nw = len(rec) if lst_nw is None else lst_nw
        self.dirty_nw = dirty_nw
        waves = max(self.lst_nw, 0)
        dirty_waves = 0 if self.lst_nw <= 0 else (dirty_nw if dirty_nw > 0 else self.lst_nw)
        self.dirty = [[] for _ in range(dirty_waves)] if dirty is None else dirty
        assert len(rec) == len(items) == waves and len(self.dirty) == dirty_waves
        self.arrival = np.full(n_states, -1, np.int32) if arrival is None else np.ascontiguousarray(arrival, np.int32)
        self.started, self.needs_init, self.error, self.frame = started, needs_init, error, frame
        self.path_new, self.n_collect, self.n_paths_ref, self.path_new_ref, self.best_final = path_new, n_collect, n_paths_ref, path_new_ref, best_final
        self.cap_paths = max(len(self.paths), 1) if cap_paths is None else cap_paths
        self.gc = [0, 0, 0, 0]                   # GcState: active, kept, kept_ref, by_rule

    @property
    def n_paths(self):
        return len(self.paths)


class Desc:
    def __init__(self, streams, ops, *, NE=3, row_ptr=(0, 0), arc_in=(), pcount=0, sentinel=-777, cap_slots=None, cap_items=None, cap_new=None):
        self.streams, self.ops, self.NE, self.pcount, self.sentinel = streams, ops, NE, pcount, sentinel
        self.row_ptr, self.arc_in = list(row_ptr), list(arc_in)
        self.n_states = len(self.row_ptr) - 1
        nw = max([s.lst_nw for s in streams] + [s.dirty_nw for s in streams] + [1])
        most = lambda per: max([len(x) for s in streams for x in per(s)] + [1])
        # the smallest capacities whose segments hold every wave's list, for every stream's number of waves (cases may set larger ones)
        self.cap_slots = nw * ((most(lambda s: s.rec) + 63) // 64 * 64) if cap_slots is None else cap_slots
        self.cap_items = nw * most(lambda s: s.items) if cap_items is None else cap_items
        self.cap_new = nw * most(lambda s: s.dirty) if cap_new is None else cap_new

    def seg_item(self, s):
        return self.cap_items // s.lst_nw

    def item_path(self, s, a):
        """the path of item a = w * seg_item + k of the last frame"""
        return s.items[a // self.seg_item(s)][a % self.seg_item(s)]

    def has_model(self, st):
        return any(self.arc_in[a] & ~ARC_FLAGS for a in range(self.row_ptr[st], self.row_ptr[st + 1]))


def path_rule_fires(n_path, n_path_new):
    """collectPaths' count trigger (WFSTDecoderLite.cpp:360-362): nPath / nPathNew > 12 in IEEE single precision, and nPath > 10000"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool(n_path > 10000 and np.float32(n_path) / np.float32(n_path_new) > np.float32(12.0))


def is_active(D, s, gc_threshold, rule):
    return bool(s.started and not s.needs_init and s.error == 0 and s.lst_nw > 0 and (s.n_paths > gc_threshold or rule))


def roots(D, s):
    """(the reference's roots, the others): paths, -1 among them.  The reference's: the live emitting tokens of the instances and, where
    the reference's counts are kept (pcount), the arrival item of every dirty state that has a key and an arc with a model."""
    ref = [p for wave in s.rec for n, _, toks in wave for sc, p in toks if is_live(sc)]
    if D.pcount:
        ref += [D.item_path(s, s.arrival[st]) for wave in s.dirty for st in wave if s.arrival[st] >= 0 and D.has_model(st)]
    return ref, [p for wave in s.items for p in wave] + [s.best_final]


def reach(prev, start, seen):
    """mark the records reachable from the roots (a walk ends where another one has been)"""
    for q in start:
        while q >= 0 and not seen[q]:
            seen[q] = True
            q = prev[q]
    return seen


def collect_stream(D, s, gc_threshold, path_rule):
    rule = bool(path_rule and (gc_threshold < 0 or (path_rule_fires(s.n_paths_ref, s.path_new_ref) if D.pcount else path_rule_fires(s.n_paths, s.path_new))))
    active = is_active(D, s, gc_threshold, rule)
    s.gc = [int(active), 0, 0, int(rule)]
    if not active:
        return
    n = s.n_paths
    prev = s.paths[:, 0]
    ref_roots, other_roots = roots(D, s)
    kept_ref = reach(prev, ref_roots, np.zeros(n, bool))
    kept = reach(prev, other_roots, kept_ref.copy())
    rank = np.where(kept, np.cumsum(kept) - 1, -1).astype(np.int32)            # the new index: the rank among the kept records
    remap = lambda p: int(rank[p]) if p >= 0 else p
    new = s.paths[kept].copy()
    new[:, 0] = np.where(new[:, 0] >= 0, rank[np.maximum(new[:, 0], 0)], -1)       # (a kept record's predecessor is kept)
    s.paths = new
    s.rec = [[(ns, src, [(sc, (remap(p) if is_live(sc) else -1) if p >= 0 else p) for sc, p in toks]) for ns, src, toks in wave] for wave in s.rec]
    s.items = [[remap(p) for p in wave] for wave in s.items]
    s.best_final = remap(s.best_final)
    k, kr = int(kept.sum()), int(kept_ref.sum())
    s.gc[1:3] = [k, kr]
    s.path_new = k
    if not D.pcount:
        s.n_collect += 1
    elif rule:
        s.n_paths_ref, s.path_new_ref, s.n_collect = kr, kr, s.n_collect + 1


def tips(D, s):
    """one tip per instance - its first token with a Path: the pending entry token of its source state (the item the state's arrival
    key names), then its emitting states in order - and one per dirty state that has an arc with a model: the entry token pending there"""
    out = []
    for wave in s.rec:
        for n, src, toks in wave:
            tip = D.item_path(s, s.arrival[src]) if s.arrival[src] >= 0 else -1
            for _, p in toks:
                if tip < 0:
                    tip = p
            out.append(tip)
    for wave in s.dirty:
        for st in wave:
            if D.has_model(st):
                out.append(D.item_path(s, s.arrival[st]) if s.arrival[st] >= 0 else -1)
    return out


def word_rec(paths, q):
    """the record itself, or its nearest labelled ancestor (model-level output writes records without a word label too)"""
    while q >= 0 and paths[q, 2] == 0:
        q = paths[q, 0]
    return int(q)


def word_chain(paths, q):
    """the word records from q's down to the root, newest first"""
    out = []
    q = word_rec(paths, q)
    while q >= 0:
        out.append(q)
        q = word_rec(paths, paths[q, 0])
    return out


def trace_answer(D, s, last_frame):
    """the newest record common to the word chains of all tips, or None"""
    if not s.started or s.needs_init or s.error != 0 or s.lst_nw <= 0:
        return None
    tp = tips(D, s)
    if not tp or min(tp) < 0:
        return None
    common = None
    for t in sorted(set(tp)):
        anc = set(word_chain(s.paths, t))
        common = anc if common is None else common & anc
        if not common:
            return None
    ans = max(common)
    return ans if s.paths[ans, 1] > last_frame else None


def trace_stream(D, s, last_frame, res_cap, model_level):
    """k_partial's words: out[3], res_label[res_cap], res_time[res_cap], pm[6][res_cap]"""
    out = np.full(3 + 8 * res_cap, D.sentinel, np.int32)
    out[0:2] = 0
    ans = trace_answer(D, s, last_frame)
    if ans is None:
        return out, 0
    chain = word_chain(s.paths, ans)[::-1]                      # oldest first
    n = len(chain)
    m = min(n, res_cap)
    out[3:3 + m] = s.paths[chain[:m], 2]
    out[3 + res_cap:3 + res_cap + m] = s.paths[chain[:m], 1]
    if model_level:
        every = []
        q = ans
        while q >= 0:
            every.append(q)
            q = int(s.paths[q, 0])
        every = every[::-1]
        out[2] = len(every)
        if len(every) <= res_cap:
            pm = out[3 + 2 * res_cap:].reshape(6, res_cap)
            for row, field in enumerate((3, 2, 1, 4, 5, 6)):          # model, label, time, score, ac, lm
                pm[row, :len(every)] = s.paths[every, field]
    out[0:2] = [1, n]
    return out, n


def trace_many(D, entries, res_cap):
    """k_partial_many's buffer: the {found, n} heads, then PARTIAL_SHARE (label, frame) pairs per entry - the records [have, n), staged
    only when there are some, no more than a share and the chain fits the result arrays"""
    k = len(entries)
    buf = np.full(2 * k + 2 * PARTIAL_SHARE * k, D.sentinel, np.int32)
    for i, (si, last_frame, have) in enumerate(entries):
        o, n = trace_stream(D, D.streams[si], last_frame, res_cap, 0)
        buf[2 * i:2 * i + 2] = o[0:2]
        if have < n and n - have <= PARTIAL_SHARE and n <= res_cap:
            stage = buf[2 * k + 2 * PARTIAL_SHARE * i:][:2 * (n - have)]
            stage[0::2] = o[3 + have:3 + n]
            stage[1::2] = o[3 + res_cap + have:3 + res_cap + n]
    return buf


def stream_words(D, s):
    """a stream's part of what jd_debug_paths returns, and a name for every word"""
    head = [s.n_paths, s.path_new, s.n_collect, s.n_paths_ref, s.path_new_ref, s.best_final] + s.gc
    names = [("n_paths",), ("path_new",), ("n_collect",), ("n_paths_ref",), ("path_new_ref",), ("best_final.path",), ("gc.active",), ("gc.kept",),
             ("gc.kept_ref",), ("gc.by_rule",)]
    toks = []
    for w, wave in enumerate(s.rec):
        for q, (n, _, t) in enumerate(wave):
            toks += [p for _, p in t] + [D.sentinel] * (D.NE - len(t))
    its = [p for wave in s.items for p in wave]
    words = np.concatenate([np.int32(head), s.paths.reshape(-1), np.int32(toks), np.int32(its)]).astype(np.int32)
    sizes = (("head", len(head)), ("paths", 7 * s.n_paths), ("token path", len(toks)), ("item path", len(its)))
    return words, names, sizes


def run(D):
    """the description's operations on a copy of its state -> (the words jd_debug_paths returns, name(i): what word i is)"""
    D = copy.deepcopy(D)
    trace_parts = []
    for op in D.ops:
        if op[0] == COLLECT:
            _, work, G, gc_threshold, path_rule = op
            for si in ([work] if isinstance(work, int) else work):
                collect_stream(D, D.streams[si], gc_threshold, path_rule)
        elif op[0] == TRACE:
            _, si, last_frame, res_cap, model_level = op
            trace_parts.append(("trace of stream %d" % si, trace_stream(D, D.streams[si], last_frame, res_cap, model_level)[0]))
        else:
            _, entries, res_cap = op
            trace_parts.append(("trace_many", trace_many(D, entries, res_cap)))
    parts, index = [], []
    for si, s in enumerate(D.streams):
        words, names, sizes = stream_words(D, s)
        parts.append(words)
        at = 0
        for what, n in sizes:
            index.append((sum(len(p) for p in parts[:-1]) + at, n, "stream %d %s" % (si, what)))
            at += n
    for what, words in trace_parts:
        index.append((sum(len(p) for p in parts), len(words), what))
        parts.append(words)
    words = np.concatenate(parts).astype(np.int32)

    def name(i):
        for start, n, what in index:
            if start <= i < start + n:
                k = i - start
                if what.endswith("paths"):
                    return "%s[%d].%s" % (what, k // 7, PATH_FIELDS[k % 7])
                if what.endswith("head"):
                    return "%s word %d (n_paths path_new n_collect n_paths_ref path_new_ref best_final active kept kept_ref by_rule)" % (what, k)
                return "%s[%d]" % (what, k)
        return "word %d" % i
    return words, name


def first_mismatch(got, want, name, case):
    """None, or what the first differing word is"""
    got, want = np.asarray(got), np.asarray(want)
    m = min(got.shape[0], want.shape[0])
    bad = np.flatnonzero(got[:m] != want[:m])
    if bad.size == 0:
        return None if got.shape == want.shape else "%s: %d words come back, %d expected" % (case, got.shape[0], want.shape[0])
    i = int(bad[0])
    return "%s: %s = %d, expected %d (%d words differ)" % (case, name(i), got[i], want[i], bad.size)
