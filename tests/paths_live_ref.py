"""The two live views of jd_debug_paths - PD_FINAL_MANY (k_final_many: the end-of-utterance view) and PD_TRACE_MANY_MODELS
(k_partial_many_models: tracePartialPath with its model-level export, for a work list) - written from their definitions on top of
tests/paths_ref.py: what tests/test_gpu_paths_live.py holds every word the device returns to.

An operation is (FINAL_MANY, [(stream, score bits, ac bits, lm bits)], res_cap, model_level) or (TRACE_MANY_MODELS, [(stream,
last_frame, have, have_m)], res_cap); the older ones are paths_ref's.  run(D) and encode(D) take descriptions with any of the five."""
import copy

import numpy as np

import paths_cases as pc
import paths_ref as pr
from paths_ref import COLLECT, PARTIAL_SHARE, TRACE, TRACE_MANY

FINAL_MANY, TRACE_MANY_MODELS = 4, 5
FINAL_HEAD, FINAL_SHARE, FIELDS = 8, 64, 6
PM_HEAD, PM_SHARE = 4, 112
FINAL_PER = FINAL_HEAD + FIELDS * FINAL_SHARE
PM_PER = PM_HEAD + 2 * PARTIAL_SHARE + FIELDS * PM_SHARE
# a Path record's columns (paths_ref.PATH_FIELDS) in the order of a model-level list: model, label, time, score, ac, lm
LIST_COLS = (3, 2, 1, 4, 5, 6)


def chain_of(paths, q):
    """the records from q down to the root, OLDEST first"""
    out = []
    while q >= 0:
        out.append(q)
        q = int(paths[q, 0])
    return out[::-1]


def final_many(D, entries, res_cap, model_level):
    """k_final_many's words: its buffer (heads, then a share per entry), per entry the five result arrays, then a model row per
    STREAM.  found: the stream is in order, has processed a frame and the token's score is above LOG_ZERO; the chain is
    best_final.path's, oldest first, its newest entry with the token's three scores; written to the arrays where it fits res_cap
    and to the share where it fits that too."""
    k, B = len(entries), len(D.streams)
    buf = np.full(FINAL_PER * k, D.sentinel, np.int32)
    rows = np.full((k, 5, res_cap), D.sentinel, np.int32)
    mrows = np.full((B, res_cap), D.sentinel, np.int32)
    for i, (si, sc, ac, lm) in enumerate(entries):
        s = D.streams[si]
        head = buf[FINAL_HEAD * i:FINAL_HEAD * (i + 1)]
        head[:] = 0
        if not (s.started and not s.needs_init and s.error == 0 and s.frame != 0 and pr.is_live(sc)):
            continue
        chain = chain_of(s.paths, s.best_final)
        n = len(chain)
        recs = s.paths[chain].copy() if n else np.zeros((0, 7), np.int32)
        head[:7] = [1, 0, int((recs[:, 2] != 0).sum()), n, sc, ac, lm]
        if n > res_cap:
            continue
        if n:
            recs[-1, 4:7] = [sc, ac, lm]
        for r, col in enumerate(LIST_COLS[1:]):
            rows[i, r, :n] = recs[:, col]
        if model_level:
            mrows[si, :n] = recs[:, 3]
        if n <= FINAL_SHARE:
            stage = buf[FINAL_HEAD * k + FIELDS * FINAL_SHARE * i:][:FIELDS * FINAL_SHARE].reshape(FIELDS, FINAL_SHARE)
            for r, col in enumerate(LIST_COLS):
                stage[r, :n] = recs[:, col]
    return np.concatenate([buf, rows.reshape(-1), mrows.reshape(-1)])


def trace_many_models(D, entries, res_cap):
    """k_partial_many_models' words: its buffer ({found, n, nm, 0} heads, then per entry PARTIAL_SHARE (label, frame) pairs and
    PM_SHARE records field-major), per entry res_label and res_time, then the model list [6][res_cap] per STREAM.  The trace is
    paths_ref.trace_stream at model level; the words [have, n) and the records [have_m, nm) are staged where both lists fit the
    result capacity, there are some, and no more than a share."""
    k, B = len(entries), len(D.streams)
    buf = np.full(PM_PER * k, D.sentinel, np.int32)
    words = np.full((k, 2, res_cap), D.sentinel, np.int32)
    pm = np.full((B, FIELDS, res_cap), D.sentinel, np.int32)
    for i, (si, last_frame, have, have_m) in enumerate(entries):
        o, n = pr.trace_stream(D, D.streams[si], last_frame, res_cap, 1)
        head = buf[PM_HEAD * i:PM_HEAD * (i + 1)]
        head[:] = [o[0], o[1], o[2] if o[0] else 0, 0]
        words[i] = o[3:3 + 2 * res_cap].reshape(2, res_cap)
        pm[si] = o[3 + 2 * res_cap:].reshape(FIELDS, res_cap)
        nm = int(head[2])
        if not o[0] or n > res_cap or nm > res_cap:
            continue
        stage = buf[PM_HEAD * k + (PM_PER - PM_HEAD) * i:][:PM_PER - PM_HEAD]
        if have < n and n - have <= PARTIAL_SHARE:
            stage[0:2 * (n - have):2] = words[i, 0, have:n]
            stage[1:2 * (n - have):2] = words[i, 1, have:n]
        if have_m < nm and nm - have_m <= PM_SHARE:
            ms = stage[2 * PARTIAL_SHARE:].reshape(FIELDS, PM_SHARE)
            ms[:, :nm - have_m] = pm[si, :, have_m:nm]
    return np.concatenate([buf, words.reshape(-1), pm.reshape(-1)])


def run(D):
    """paths_ref.run for descriptions with any of the five operations -> (the words jd_debug_paths returns, name(i))"""
    D = copy.deepcopy(D)
    parts_after = []
    for op in D.ops:
        if op[0] == COLLECT:
            _, work, G, gc_threshold, path_rule = op
            for si in ([work] if isinstance(work, int) else work):
                pr.collect_stream(D, D.streams[si], gc_threshold, path_rule)
        elif op[0] == TRACE:
            _, si, last_frame, res_cap, model_level = op
            parts_after.append(("trace of stream %d" % si, pr.trace_stream(D, D.streams[si], last_frame, res_cap, model_level)[0]))
        elif op[0] == TRACE_MANY:
            parts_after.append(("trace_many", pr.trace_many(D, op[1], op[2])))
        elif op[0] == FINAL_MANY:
            parts_after.append(("final_many", final_many(D, op[1], op[2], op[3])))
        else:
            assert op[0] == TRACE_MANY_MODELS
            parts_after.append(("trace_many_models", trace_many_models(D, op[1], op[2])))
    parts, index = [], []
    at = 0
    for si, s in enumerate(D.streams):
        words, _, sizes = pr.stream_words(D, s)
        parts.append(words)
        for what, n in sizes:
            index.append((at, n, "stream %d %s" % (si, what)))
            at += n
    for what, words in parts_after:
        index.append((at, len(words), what))
        parts.append(words)
        at += len(words)
    words = np.concatenate(parts).astype(np.int32)

    def name(i):
        for start, n, what in index:
            if start <= i < start + n:
                return "%s[%d]" % (what, i - start)
        return "word %d" % i
    return words, name


def encode(D):
    """paths_cases.encode for descriptions with any of the five operations"""
    bare = copy.copy(D)
    bare.ops = []
    w = pc.encode(bare).tolist()
    w[3] = len(D.ops)
    for op in D.ops:
        if op[0] == COLLECT:
            _, work, G, thr, rule = op
            w += [COLLECT] + ([0, work] if isinstance(work, int) else [len(work)] + list(work)) + [G, thr, rule]
        elif op[0] == TRACE:
            w += list(op)
        elif op[0] == TRACE_MANY:
            w += [TRACE_MANY, len(op[1])] + [x for e in op[1] for x in e] + [op[2]]
        elif op[0] == FINAL_MANY:
            w += [FINAL_MANY, len(op[1])] + [x for e in op[1] for x in e] + [op[2], op[3]]
        elif op[0] == TRACE_MANY_MODELS:
            w += [TRACE_MANY_MODELS, len(op[1])] + [x for e in op[1] for x in e] + [op[2]]
        else:
            w += list(op)                                  # (no operation of the description: its words as they are)
    return np.asarray(w, np.int64).astype(np.int32)


def out_words(D):
    """how many words come back (what the validation announces): the older operations' as paths_ref.run counts them"""
    return int(run(D)[0].shape[0])
