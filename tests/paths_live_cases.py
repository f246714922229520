"""The described states the two live views of jd_debug_paths are run on (tests/test_gpu_paths_live.py) and the validation is held to
(tests/test_paths_live_cpu.py): PD_FINAL_MANY and PD_TRACE_MANY_MODELS, with the building blocks of tests/paths_cases.py.  CASES maps
a name to a builder; everything is built from fixed values."""
import functools

import numpy as np

import paths_cases as pc
from paths_cases import DEAD, LIVE, LIVE2, NINF, TREE, mk_paths, tstream
from paths_live_ref import FINAL_MANY, FINAL_SHARE, PM_SHARE, TRACE_MANY_MODELS
from paths_ref import COLLECT, PARTIAL_SHARE, Desc, Stream, f2i

AC, LM = f2i(-7.25), f2i(-0.5)
CASES = {}


def add(name, builder):
    assert name not in CASES, name
    CASES[name] = builder


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def labels_of(n, every):
    """word labels on every `every`-th record of n, the others without (model-level chains)"""
    lab = np.zeros(n, np.int64)
    lab[every - 1::every] = 1 + np.arange(len(lab[every - 1::every])) % 900
    return lab


def chain(n, every=1, NE=3, **kw):
    """a chain of n records that best_final ends (n = 0: no record, path -1), one instance on it"""
    return tstream(np.arange(n) - 1, [n - 1] if n else [], NE=NE, labels=labels_of(n, every), best_final=n - 1, **kw)


def final1(s, res_cap, model, score=LIVE, NE=3):
    return Desc([s], [(FINAL_MANY, [(0, score, AC, LM)], res_cap, model)], NE=NE)


# ------------------------------------------------------------------ the end-of-utterance view
for model_ in (0, 1):
    for n_ in (0, 1, 2, FINAL_SHARE, FINAL_SHARE + 1, 80, 81):
        # (res_cap 80: 64 and 65 are a share and one more, 81 is the capacity plus one)
        add("final_chain_%d_res_cap_80_model_%d" % (n_, model_), functools.partial(lambda n, m: final1(chain(n, 3 if m else 1), 80, m), n_, model_))
add("final_chain_above_a_share_res_cap_below", lambda: final1(chain(40, 2), 39, 1))                      # 40 records fit a share and not the arrays
add("final_path_minus_1_live_score", lambda: final1(Stream(mk_paths(TREE), [[]], [[]], best_final=-1), 16, 1))
add("final_dead_score_with_a_path", lambda: final1(chain(5), 16, 0, score=DEAD))
add("final_minus_infinity_with_a_path", lambda: final1(chain(5), 16, 1, score=NINF))
add("final_score_just_above_log_zero", lambda: final1(chain(5), 16, 1, score=LIVE2))
add("final_no_frame_yet", lambda: final1(chain(5, frame=0), 16, 0))
add("final_not_started", lambda: final1(chain(5, started=0), 16, 0))
add("final_no_waves", lambda: final1(Stream(mk_paths(TREE), [], [], lst_nw=0, best_final=12), 16, 1))   # (the view needs no list: found)
add("final_tree_branch", lambda: final1(Stream(mk_paths(TREE), [[]], [[]], best_final=19), 16, 1))       # 19 -> 17 -> 16 -> 5 .. 0
add("final_NE6_chain_70", lambda: final1(chain(70, 3, NE=6), 128, 1, NE=6))
add("final_NE6_chain_3", lambda: final1(chain(3, 1, NE=6), 8, 0, NE=6))
add("final_res_cap_1_chain_1", lambda: final1(chain(1), 1, 1))
add("final_res_cap_1_chain_2", lambda: final1(chain(2), 1, 1))


def interleaved(n, NE=3, waves=1):
    """three chains interleaved in one arena (prev = q - 3): the instances hold the first, best_final ends the second, the third is
    garbage - a collection drops it and every kept record moves"""
    prev = np.arange(n) - 3
    prev[:3] = -1
    tip0, fin = (n - 1) // 3 * 3, (n - 2) // 3 * 3 + 1
    return tstream(prev, [tip0, tip0], NE=NE, waves=waves, labels=labels_of(n, 2), best_final=fin)


def final_behind_collect(n, res_cap, NE=3):
    s = interleaved(n, NE)
    ops = [(FINAL_MANY, [(0, LIVE, AC, LM)], res_cap, 1), (COLLECT, 0, 2, 0, 0), (FINAL_MANY, [(0, LIVE2, LM, AC)], res_cap, 1)]
    return Desc([s], ops, NE=NE)


add("final_behind_a_collection_within_a_share", functools.partial(final_behind_collect, 90, 64))
add("final_behind_a_collection_beyond_a_share", functools.partial(final_behind_collect, 900, 512))
add("final_behind_a_collection_NE6", functools.partial(final_behind_collect, 300, 128, 6))


def four_streams(NE=3):
    return [chain(5, 2, NE=NE), chain(6, 2, NE=NE, error=-41), chain(7, 2, NE=NE, needs_init=1), chain(70, 2, NE=NE)]


add("final_four_streams_one_failed_one_before_init", lambda: Desc(four_streams(), [(FINAL_MANY, [(3, LIVE, AC, LM), (1, LIVE, AC, LM), (0, LIVE2, LM, AC), (2, LIVE, AC, LM)], 128, 1)]))
add("final_four_streams_NE6_word_level", lambda: Desc(four_streams(6), [(FINAL_MANY, [(0, LIVE, AC, LM), (1, LIVE, AC, LM), (2, LIVE, AC, LM), (3, DEAD, AC, LM)], 128, 0)], NE=6))
add("final_two_of_three_streams", lambda: Desc([chain(3), chain(65), chain(9)], [(FINAL_MANY, [(2, LIVE, AC, LM), (1, LIVE, AC, LM)], 70, 1)]))


# ------------------------------------------------------------------ the model-level traces for many
def words_chain(n_words, extra, NE=3, **kw):
    """paths_cases.chain_case's stream: n_words word records with `extra` records without a label below each and above the last; two
    tips on its end.  The trace finds the last word record: n_words words, n_words * (1 + extra) model records."""
    n = n_words * (1 + extra) + extra
    lab = np.zeros(n, np.int64)
    lab[extra::1 + extra] = 1 + np.arange(n_words) % 900
    return tstream(np.arange(n) - 1, [n - 1, n - 1], NE=NE, labels=lab, frames=np.arange(n), **kw)


def tm1(s, have, have_m, res_cap, last_frame=-1, NE=3):
    return Desc([s], [(TRACE_MANY_MODELS, [(0, last_frame, have, have_m)], res_cap)], NE=NE)


add("tm_nothing_found_no_instance", lambda: tm1(Stream(mk_paths(TREE), [[]], [[]]), 0, 0, 16))
add("tm_nothing_shared", lambda: tm1(tstream(TREE, [12, 18]), 0, 0, 16))
add("tm_nothing_newer_than_last_frame", lambda: tm1(words_chain(4, 1), 4, 8, 16, last_frame=7))          # the last word record: index 7, frame 7
add("tm_1_word_1_record", lambda: tm1(words_chain(1, 0), 0, 0, 16))
add("tm_1_word_3_records", lambda: tm1(words_chain(1, 2), 0, 0, 16))
# the model share: 28 words x 4 = 112 records, 29 x 4 = 116
add("tm_records_a_share", lambda: tm1(words_chain(28, 3), 0, 0, 512))
add("tm_records_a_share_plus_1", lambda: tm1(words_chain(113, 0), 113 - PARTIAL_SHARE, 0, 512))          # (its 32 new words are staged, its 113 records not)
add("tm_records_a_share_behind", lambda: tm1(words_chain(29, 3), 20, 116 - PM_SHARE, 512))
add("tm_records_a_share_plus_1_behind", lambda: tm1(words_chain(29, 3), 20, 116 - PM_SHARE - 1, 512))
# the word share
add("tm_words_a_share", lambda: tm1(words_chain(PARTIAL_SHARE, 1), 0, 0, 512))
add("tm_words_a_share_plus_1", lambda: tm1(words_chain(PARTIAL_SHARE + 1, 1), 0, 0, 512))
add("tm_words_a_share_behind", lambda: tm1(words_chain(50, 1), 50 - PARTIAL_SHARE, 90, 512))
# have / have_m ahead of, equal to and behind the new length
add("tm_have_equal", lambda: tm1(words_chain(10, 2), 10, 30, 64))
add("tm_have_m_ahead", lambda: tm1(words_chain(10, 2), 9, 31, 64))
add("tm_have_ahead", lambda: tm1(words_chain(10, 2), 11, 29, 64))
add("tm_have_behind_by_one", lambda: tm1(words_chain(10, 2), 9, 29, 64))
# the result capacity
add("tm_records_res_cap", lambda: tm1(words_chain(14, 2), 0, 0, 42))
add("tm_records_res_cap_plus_1", lambda: tm1(words_chain(14, 2), 0, 0, 41))
add("tm_words_res_cap_plus_1", lambda: tm1(words_chain(17, 0), 0, 0, 16))
add("tm_res_cap_1", lambda: tm1(words_chain(1, 0), 0, 0, 1))
add("tm_NE6", lambda: tm1(words_chain(30, 3, NE=6), 3, 12, 256, NE=6))
add("tm_unlabelled_tips_tree", lambda: Desc([tstream([-1, 0, 1, 2, 3, 2, 5, 6, 4, 8], [7, 9], labels=np.int64([3, 0, 4, 0, 0, 5, 0, 0, 0, 0]))],
                                            [(TRACE_MANY_MODELS, [(0, -1, 0, 0)], 16)]))


def tm_four(NE=3):
    ss = [words_chain(5, 2, NE=NE), words_chain(6, 2, NE=NE, error=-41), words_chain(7, 2, NE=NE, needs_init=1), words_chain(40, 3, NE=NE)]
    return Desc(ss, [(TRACE_MANY_MODELS, [(3, -1, 0, 0), (1, -1, 0, 0), (0, 3, 2, 6), (2, -1, 0, 0)], 256)], NE=NE)


add("tm_four_streams_one_failed_one_before_init", tm_four)
add("tm_four_streams_NE6", functools.partial(tm_four, 6))
add("tm_two_of_three_streams", lambda: Desc([words_chain(3, 1), words_chain(40, 3), words_chain(9, 1)], [(TRACE_MANY_MODELS, [(2, -1, 1, 2), (1, -1, 8, 48)], 200)]))


def tm_behind_collect():
    """the trace before and the trace after a collection that moves every kept record give the same lists; then the final view"""
    n = 600
    prev = np.arange(n) - 2
    prev[:2] = -1
    tip = (n - 1) // 2 * 2
    s = tstream(prev, [tip, tip], labels=labels_of(n, 3), frames=np.arange(n), best_final=tip)
    ops = [(TRACE_MANY_MODELS, [(0, -1, 0, 0)], 512), (COLLECT, 0, 2, 0, 0), (TRACE_MANY_MODELS, [(0, -1, 90, 280)], 512), (FINAL_MANY, [(0, LIVE, AC, LM)], 512, 1)]
    return Desc([s], ops)


add("tm_behind_a_collection", tm_behind_collect)


def names(prefix=""):
    return [n for n in CASES if n.startswith(prefix)]
