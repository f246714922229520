"""The two live views on described states, without a device: jd_paths.h's validation of PD_FINAL_MANY and PD_TRACE_MANY_MODELS
through tests/paths_driver.cpp (which passes whatever pd_parse knows) - plain and under -fsanitize=address,undefined as a stand-alone
program -, the room it announces against tests/paths_live_ref.py, that the cases of tests/paths_live_cases.py have the shapes their
names say, and paths_live_ref against a second formulation on those cases."""
import copy

import numpy as np
import pytest

import paths_cases as pc
import paths_live_cases as lc
import paths_live_ref as lr
import paths_ref as pr
from paths_cases import LIVE
from paths_live_ref import FINAL_HEAD, FINAL_MANY, FINAL_PER, FINAL_SHARE, PM_HEAD, PM_PER, PM_SHARE, TRACE_MANY_MODELS
from paths_ref import COLLECT, PARTIAL_SHARE, TRACE

AC, LM = lc.AC, lc.LM


def base():
    return lc.Desc(lc.four_streams()[:3], [(FINAL_MANY, [(0, LIVE, AC, LM), (2, LIVE, AC, LM)], 16, 1), (TRACE_MANY_MODELS, [(1, -1, 0, 0), (0, -1, 2, 4)], 16)])


def refusals():
    def ops(*o):
        def f(D): D.ops = list(o)
        return f
    F = lambda entries, res_cap=16, model=1: (FINAL_MANY, entries, res_cap, model)
    T = lambda entries, res_cap=16: (TRACE_MANY_MODELS, entries, res_cap)
    e = (0, LIVE, AC, LM)
    return [("bad stream", ops(F([(3, LIVE, AC, LM)]))), ("bad stream", ops(F([(-1, LIVE, AC, LM)]))), ("twice", ops(F([e, (1, LIVE, AC, LM), e]))),
            ("res_cap", ops(F([e], 0))), ("res_cap", ops(F([e], -5))), ("res_cap", ops(F([e], (1 << 16) + 1))), ("model_level", ops(F([e], 16, 2))),
            ("model_level", ops(F([e], 16, -1))), ("work list", ops((FINAL_MANY, [], 16, 1))), ("work list", ops(F([e] * 4))),
            ("bad stream", ops(T([(3, -1, 0, 0)]))), ("bad stream", ops(T([(-1, -1, 0, 0)]))), ("twice", ops(T([(1, -1, 0, 0), (1, 5, 1, 1)]))),
            ("res_cap", ops(T([(0, -1, 0, 0)], 0))), ("res_cap", ops(T([(0, -1, 0, 0)], (1 << 16) + 1))), ("< 0", ops(T([(0, -1, -1, 0)]))),
            ("< 0", ops(T([(0, -1, 0, -1)]))), ("< 0", ops(T([(0, -1, 3, -(1 << 31))]))), ("work list", ops((TRACE_MANY_MODELS, [], 16))),
            ("kind", ops((6, 0, 0, 0, 0))), ("best_final", lambda D: setattr(D.streams[0], "best_final", 5))]


def edit(f):
    D = base()
    f(D)
    return lr.encode(D)


def lines():
    ok = lr.encode(base())
    cut = [ok[:len(ok) - k] for k in (1, 2, 3, 6, 7, 8, 10)] + [np.concatenate([ok, np.int32([0])])]
    return [edit(f) for _, f in refusals()] + cut + [ok] + [lr.encode(lc.case(n)) for n in lc.CASES]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return pc.build_driver(str(tmp_path_factory.mktemp("paths_live") / "paths_driver"))


def test_validation_of_the_new_operations(driver):
    """refused: a stream out of range or listed twice, res_cap < 1 or above 2^16, have / have_m negative, a model level that is none, an
    empty or overlong work list, a description that ends inside the operation; accepted: every case, with room for exactly what the
    restatement returns"""
    res = pc.run_driver(driver, lines())
    n = len(refusals())
    for (what, _), (rc, _, msg) in zip(refusals(), res):
        assert rc == -1 and what in msg, (what, msg)
    assert all(rc == -1 for rc, _, _ in res[n:n + 8]), [r[2] for r in res[n:n + 8]]
    assert res[n + 8][0] == 0 and res[n + 8][1][0] == lr.run(base())[0].shape[0]
    assert len(lc.CASES) >= 55
    for name, (rc, v, msg) in zip(lc.CASES, res[n + 9:]):
        assert rc == 0, (name, msg)
        D = lc.case(name)
        if not any(op[0] == COLLECT for op in D.ops):                  # (room is asked for what comes back when no collection shrinks an arena)
            assert v[0] == lr.run(D)[0].shape[0], name


def test_older_descriptions_encode_and_run_as_before():
    for name in ("trace_deep_record_shared", "trace_many_0_1_share", "trace_collect_trace", "two_collections_in_a_row"):
        D = pc.case(name)
        assert np.array_equal(lr.encode(D), pc.encode(D)), name
        assert np.array_equal(lr.run(D)[0], pr.run(D)[0]), name


def test_driver_under_sanitizers(driver, tmp_path_factory):
    san = pc.build_driver(str(tmp_path_factory.mktemp("paths_live_san") / "paths_driver_san"),
                          ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    L = lines()
    assert pc.run_driver(san, L) == pc.run_driver(driver, L)


def final_parts(D, op, words):
    """a PD_FINAL_MANY's words by entry: (head, share as [6][FINAL_SHARE], arrays as [5][res_cap]), and the model rows [stream][res_cap]"""
    _, entries, cap, _ = op
    k = len(entries)
    out = []
    for i in range(k):
        out.append((words[FINAL_HEAD * i:FINAL_HEAD * (i + 1)], words[FINAL_HEAD * k + 384 * i:][:384].reshape(6, FINAL_SHARE),
                    words[FINAL_PER * k + 5 * cap * i:][:5 * cap].reshape(5, cap)))
    return out, words[FINAL_PER * k + 5 * cap * k:].reshape(len(D.streams), cap)


def last_op_words(D):
    """the words of the description's LAST operation, as the restatement gives them"""
    words, _ = lr.run(D)
    op = D.ops[-1]
    n = FINAL_PER * len(op[1]) + 5 * op[2] * len(op[1]) + len(D.streams) * op[2] if op[0] == FINAL_MANY else \
        PM_PER * len(op[1]) + 2 * op[2] * len(op[1]) + 6 * len(D.streams) * op[2]
    return words[-n:]


def test_final_cases_have_the_shapes_their_names_say():
    """... and the restatement, read back, is jd_finish_kernel's walk: newest first from best_final.path, entry 0 with the token's
    scores - written here once more, the other way round"""
    S = D_SENT = -777
    seen = set()
    for name in lc.names("final_"):
        D = lc.case(name)
        op = D.ops[-1]
        if op[0] != FINAL_MANY:
            continue
        after = copy.deepcopy(D)
        for o in D.ops[:-1]:
            if o[0] == COLLECT:
                pr.collect_stream(after, after.streams[o[1]], o[3], o[4])
        parts, mrows = final_parts(D, op, last_op_words(D))
        cap, model = op[2], op[3]
        listed = set()
        for (si, sc, ac, lm), (head, share, arrays) in zip(op[1], parts):
            s = after.streams[si]
            listed.add(si)
            ok = bool(s.started and not s.needs_init and s.error == 0 and s.frame != 0 and pr.is_live(sc))
            assert head[0] == int(ok), name
            if not ok:
                assert not head.any() and (share == S).all() and (arrays == S).all() and (mrows[si] == S).all(), name
                seen.add("not found")
                continue
            # jd_finish_kernel, newest first
            fin, q = [], s.best_final
            while q >= 0:
                rec = s.paths[q].copy()
                if not fin:
                    rec[4:7] = [sc, ac, lm]
                fin.append(rec)
                q = int(rec[0])
            n = len(fin)
            assert list(head) == [1, 0, sum(int(r[2] != 0) for r in fin), n, sc, ac, lm, 0], name
            seen.add("empty" if n == 0 else "share" if n == FINAL_SHARE else "share + 1" if n == FINAL_SHARE + 1 else "one" if n == 1 else "some")
            if n > cap:
                assert (share == S).all() and (arrays == S).all() and (mrows[si] == S).all(), name
                seen.add("above res_cap")
                continue
            old = np.asarray(fin[::-1], np.int32).reshape(n, 7)
            for r, col in enumerate((2, 1, 4, 5, 6)):
                assert np.array_equal(arrays[r, :n], old[:, col]) and (arrays[r, n:] == S).all(), (name, r)
            assert (np.array_equal(mrows[si, :n], old[:, 3]) if model else (mrows[si, :n] == S).all()) and (mrows[si, n:] == S).all(), name
            if n <= FINAL_SHARE:
                for r, col in enumerate((3, 2, 1, 4, 5, 6)):
                    assert np.array_equal(share[r, :n], old[:, col]) and (share[r, n:] == S).all(), (name, r)
            else:
                assert (share == S).all(), name
                seen.add("from the arrays")
        for si in range(len(D.streams)):
            assert si in listed or (mrows[si] == S).all(), name
        if any(o[0] == COLLECT for o in D.ops) and after.streams[op[1][0][0]].best_final != D.streams[op[1][0][0]].best_final:
            seen.add("moved by a collection")
    assert D_SENT == lc.case("final_NE6_chain_3").sentinel
    assert seen >= {"not found", "empty", "one", "share", "share + 1", "above res_cap", "from the arrays", "some", "moved by a collection"}, seen
    assert {lc.case(n).NE for n in lc.names("final_")} == {3, 6}
    four = lc.case("final_four_streams_one_failed_one_before_init")
    assert len(four.streams) == 4 and sum(s.error != 0 for s in four.streams) == 1 and sum(s.needs_init for s in four.streams) == 1


def test_trace_models_cases_have_the_shapes_their_names_say():
    """found / n / nm and what is staged, case by case, from the chains' construction"""
    def heads(name):
        D = lc.case(name)
        op = D.ops[-1]
        w = last_op_words(D)
        k = len(op[1])
        return [(tuple(w[PM_HEAD * i:PM_HEAD * (i + 1)]), w[PM_HEAD * k + (PM_PER - PM_HEAD) * i:][:PM_PER - PM_HEAD]) for i in range(k)]
    S = -777
    staged = lambda st: (int((st[:2 * PARTIAL_SHARE] != S).sum()) // 2, int((st[2 * PARTIAL_SHARE:] != S).sum()) // 6)
    want = {"tm_nothing_found_no_instance": ((0, 0, 0, 0), (0, 0)), "tm_nothing_shared": ((0, 0, 0, 0), (0, 0)),
            "tm_nothing_newer_than_last_frame": ((0, 0, 0, 0), (0, 0)), "tm_1_word_1_record": ((1, 1, 1, 0), (1, 1)),
            "tm_1_word_3_records": ((1, 1, 3, 0), (1, 3)), "tm_records_a_share": ((1, 28, 112, 0), (28, 112)),
            "tm_records_a_share_plus_1": ((1, 113, 113, 0), (32, 0)), "tm_records_a_share_behind": ((1, 29, 116, 0), (9, 112)),
            "tm_records_a_share_plus_1_behind": ((1, 29, 116, 0), (9, 0)), "tm_words_a_share": ((1, 32, 64, 0), (32, 64)),
            "tm_words_a_share_plus_1": ((1, 33, 66, 0), (0, 66)), "tm_words_a_share_behind": ((1, 50, 100, 0), (32, 10)),
            "tm_have_equal": ((1, 10, 30, 0), (0, 0)), "tm_have_m_ahead": ((1, 10, 30, 0), (1, 0)), "tm_have_ahead": ((1, 10, 30, 0), (0, 1)),
            "tm_have_behind_by_one": ((1, 10, 30, 0), (1, 1)), "tm_records_res_cap": ((1, 14, 42, 0), (14, 42)),
            "tm_records_res_cap_plus_1": ((1, 14, 42, 0), (0, 0)), "tm_words_res_cap_plus_1": ((1, 17, 17, 0), (0, 0)),
            "tm_res_cap_1": ((1, 1, 1, 0), (1, 1)), "tm_NE6": ((1, 30, 120, 0), (27, 108))}
    for name, (head, st) in want.items():
        (h, stage), = heads(name)
        assert (h, staged(stage)) == (head, st), name
    four = heads("tm_four_streams_one_failed_one_before_init")
    assert [h for h, _ in four] == [(1, 40, 160, 0), (0, 0, 0, 0), (1, 5, 15, 0), (0, 0, 0, 0)]
    assert [staged(s) for _, s in four] == [(0, 0), (0, 0), (3, 9), (0, 0)]
    assert lc.case("tm_four_streams_NE6").NE == 6
    D = lc.case("tm_behind_a_collection")
    assert [o[0] for o in D.ops] == [TRACE_MANY_MODELS, COLLECT, TRACE_MANY_MODELS, FINAL_MANY]
    # ... whose second trace, behind the collection, has the first one's lists: the model list of the first as the prefix of the second
    words, _ = lr.run(D)
    tail = words[sum(pr.stream_words(D, s)[0].shape[0] for s in D.streams) - 7 * (D.streams[0].n_paths - 300):]      # (the collection keeps 300 records)
    one = PM_PER + 2 * 512 + 6 * 512
    a, b = tail[:one], tail[one:2 * one]
    assert tuple(a[:4]) == tuple(b[:4]) == (1, 100, 299, 0)
    assert np.array_equal(a[PM_PER:], b[PM_PER:])
    assert staged(a[PM_HEAD:PM_PER]) == (0, 0) and staged(b[PM_HEAD:PM_PER]) == (10, 19)
    assert TRACE not in [o[0] for n in lc.CASES for o in lc.case(n).ops] and PM_SHARE == 112
