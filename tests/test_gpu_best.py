"""The current best hypothesis of live streams: jd_streams_best (k_best_many), jd_stream_best_words / _models.

The yardstick where every beam is off is tests/indep_viterbi_best.py - the float64 full trellis, looked at behind the same frames;
under beams it is what must hold between the calls: the converged prefix (jd_stream_partial) is a prefix of the best hypothesis,
the word list is the model list's labelled entries, a joint call equals single calls, and a decode with the calls in between is,
bit for bit, the decode without them."""
import numpy as np
import pytest

import indep_viterbi_best as ib

pytestmark = pytest.mark.gpu

# float32 search against the float64 trellis: the relative tolerance tests/test_gpu_indep.py holds total scores to
# (indep_cases.check_against_viterbi)
TOL = 1e-5
PUSH = 25
FIELDS = ("found", "frame", "n_words", "n_records", "model", "state", "score", "ac", "lm")


def _cfg(name, n_utts=1):
    from juicer_amd import synth
    # (the seeds: chosen on the CPU so that the trellis alone meets the cap on near-ties below - small: none in 21 checked frames,
    # mixed: none in 6)
    return synth.config_small(seed=8, n_utts=n_utts) if name == "small" else synth.config_mixed(seed=12, n_utts=n_utts)


@pytest.fixture(scope="module")
def trellis(built):
    """per model set: (am, net, the utterance, the trellis's best cell behind every 25th frame) - computed once, never changed"""
    out = {}
    for name in ("small", "mixed"):
        am, net, feats, _ = _cfg(name)
        x = feats[0]
        frames = list(range(PUSH, x.shape[0] + 1, PUSH))
        out[name] = (am, net, x, ib.viterbi_best(net, am, ib.gmm_loglik(am, x), frames))
    return out


def _decoder(net, am, models, **kw):
    from juicer_amd import capi
    dec = capi.Decoder(capi.Network.from_synth(net) if not isinstance(net, capi.Network) else net,
                       capi.Models.from_htk(am) if not isinstance(am, capi.Models) else am, **kw)
    if models:
        dec.set_output_level(capi.OUTPUT_WORDS | capi.OUTPUT_MODELS)
    return dec


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).tolist() if a.dtype == np.float32 else a.tolist()


def _lists(dec, s, models):
    """(the word list as five lists, the model list as six or None), floats as their bits"""
    w = tuple(_bits(a) for a in dec.stream_best_words(s))
    if not models:
        return w, None
    m = dec.stream_best_models(s)
    return w, tuple(_bits(getattr(m, k)) for k in ("model", "label", "time", "score", "ac", "lm"))


def _close(got, want):
    return abs(float(got) - want) <= TOL * abs(want)


@pytest.mark.parametrize("models", [False, True], ids=["words", "models"])
@pytest.mark.parametrize("name", ["small", "mixed"])
def test_against_the_trellis(trellis, name, models):
    """Every beam off: behind every 25th frame the best token's arc, state, scores and chain are the trellis's (small: 3-state
    HMMs and the tee model between words; mixed: HMMs of 1-6 emitting states, the NE = 6 layout).  A frame whose best cell has a
    rival with another chain within the tolerance is skipped - float32 may resolve it either way - and at most one in ten may be.
    jd_best.score is the token's own score, normalised frame by frame like every score of jd_hyp: it is held to the trellis as
    ac + lm, and bit for bit between the calls in the tests below."""
    am, net, x, ref = trellis[name]
    assert (am.max_n > 5) == (name == "mixed")
    dec = _decoder(net, am, models)
    dec.stream_init(0)
    checked = skipped = 0
    for f in sorted(ref):
        dec.stream_push(0, x[f - PUSH:f])
        e = dec.streams_best([0])[0]
        r = ref[f]
        assert r is not None and e["found"] == 1 and e["frame"] == f
        checked += 1
        if r["margin"] < TOL * abs(r["score"]):
            skipped += 1
            continue
        # (the seed: no other CELL within the tolerance either, so arc and state are decided as well as the chain)
        assert r["cell_margin"] >= TOL * abs(r["score"]), (name, f, r["cell_margin"])
        chain = [(m, lab, t) for (m, lab, t, _s, _l) in r["chain"]]
        words = [(lab, t) for (_m, lab, t) in chain if lab != 0]
        print("%s frame %d: ac + lm %.4f / %.4f  lm %.5f / %.5f  margin %.3f  records %d" % (name, f, e["ac"] + e["lm"], r["score"], e["lm"], r["lm"], r["margin"], len(chain)))
        assert (e["model"], e["state"]) == (r["model"], r["state"]), (name, f)
        assert e["n_words"] == len(words) and e["n_records"] == (len(chain) if models else len(words)), (name, f)
        # (the search normalises a token's score by the frame's best, as the reference does - WFSTDecoderLite.cpp:321, :408 - so
        # what stands for the trellis's score is ac + lm, as for the totals of tests/indep_cases.check_against_viterbi)
        assert _close(e["ac"] + e["lm"], r["score"]) and _close(e["lm"], r["lm"]) and _close(e["ac"], r["score"] - r["lm"]), (name, f, e, r["score"], r["lm"])
        lab, tim = dec.stream_best_words(0)[:2]
        assert list(zip(lab.tolist(), tim.tolist())) == words, (name, f)
        if models:
            m = dec.stream_best_models(0)
            assert list(zip(m.model.tolist(), m.label.tolist(), m.time.tolist())) == chain, (name, f)
    assert checked >= 6 and skipped * 10 <= checked, (checked, skipped)
    dec.stream_finish(0)
    dec.close()


def _check_invariants(dec, s, f, models, trace_now=True):
    """what holds between the calls at frame f (frames pushed) of stream s; returns (partial words, best words)"""
    e = dec.streams_best([s])[0]
    assert e["frame"] == f
    _, part = dec.stream_partial(s, trace_now=trace_now)
    lab, tim, sc, ac, lm = dec.stream_best_words(s)
    best = list(zip(lab.tolist(), tim.tolist()))
    assert best[:len(part)] == part, (s, f, part, best)
    assert all(a <= b for a, b in zip(tim[:-1], tim[1:])) and (len(tim) == 0 or tim[-1] <= f - 1), (s, f, tim)
    assert e["n_words"] == len(best) and (models or e["n_records"] == len(best))
    if e["found"]:
        assert e["model"] >= 1 and e["state"] >= 1
    if models:
        _, pm = dec.stream_partial_models(s)
        bm = dec.stream_best_models(s)
        assert e["n_records"] == bm.n >= pm.n
        for k in ("model", "label", "time", "score", "ac", "lm"):
            assert _bits(getattr(bm, k)[:pm.n]) == _bits(getattr(pm, k)), (s, f, k)
        keep = bm.label != 0
        for got, want in zip((lab, tim, sc, ac, lm), (bm.label, bm.time, bm.score, bm.ac, bm.lm)):
            assert _bits(got) == _bits(want[keep]), (s, f)
        assert all(a <= b for a, b in zip(bm.time[:-1], bm.time[1:])) and (bm.n == 0 or bm.time[-1] <= f - 1)
    return part, best


BEAMS = [dict(main_beam=150.0), dict(main_beam=150.0, end_beam=100.0, word_beam=100.0)]


@pytest.mark.parametrize("models", [False, True], ids=["words", "models"])
@pytest.mark.parametrize("beams", BEAMS, ids=["main", "end_word"])
def test_prefix_invariant(built, beams, models):
    """Under beams: what the partial trace has converged on is a prefix of the best hypothesis - labels and times, at model level
    all six fields bit for bit -, times do not decrease and end before the frame reached, and the word list is the model list's
    labelled entries."""
    am, net, feats, _ = _cfg("small")
    x = feats[0]
    dec = _decoder(net, am, models, **beams)
    dec.stream_init(0)
    assert dec.streams_best([0])[0] == dict(zip(FIELDS, (0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0)))
    grown = ahead = 0
    for f in range(PUSH, x.shape[0] + 1, PUSH):
        dec.stream_push(0, x[f - PUSH:f])
        part, best = _check_invariants(dec, 0, f, models)
        grown += len(part) > 0
        ahead += len(best) > len(part)
    assert grown >= 4 and ahead >= 4, "vacuous: %d non-empty prefixes, %d hypotheses beyond them" % (grown, ahead)
    dec.stream_finish(0)
    dec.stream_init(0)
    assert dec.stream_best_words(0)[0].shape[0] == 0                   # (empty from jd_stream_init on)
    dec.close()


def test_many_streams(built):
    """Four streams on four utterances - one a push behind, one not yet pushed, one finished and begun again: a joint call is four
    single calls entry for entry, with one launch and one copy."""
    am, net, feats, _ = _cfg("small", n_utts=4)
    dec = _decoder(net, am, False, max_streams=4, main_beam=150.0)
    for s in range(4):
        dec.stream_init(s)
    dec.stream_push(3, feats[3][:60])
    assert dec.streams_best([3])[0]["found"] == 1
    dec.stream_finish(3)
    dec.stream_init(3)
    dec.stream_push(0, feats[0][:50])
    dec.streams_push([0, 1, 3], [feats[0][50:120], feats[1][:70], feats[3][:70]])
    l0, c0 = dec.best_stats()
    joint = dec.streams_best([3, 0, 2, 1])
    l1, c1 = dec.best_stats()
    assert (l1 - l0, c1 - c0) == (1, 1)
    joint_lists = [_lists(dec, s, False) for s in (3, 0, 2, 1)]
    assert [e["frame"] for e in joint] == [70, 120, 0, 70]
    assert [e["found"] for e in joint] == [1, 1, 0, 1] and joint_lists[2][0][0] == []
    assert sum(e["n_words"] for e in joint) >= 3, "vacuous: no words yet"
    assert len(set(map(str, joint_lists))) == 4, "the streams' lists are meant to differ"
    for i, s in enumerate((3, 0, 2, 1)):
        single = dec.streams_best([s])[0]
        assert single == joint[i] and tuple(single) == FIELDS, (s, single, joint[i])
        assert _lists(dec, s, False) == joint_lists[i], s
    assert dec.streams_best([]) == []
    dec.close()


def test_chain_beyond_the_staging_share(built):
    """A late first call on a long input: more records than a share of k_best_many's staging area (64), so the list comes from the
    stream's result arrays - complete, the trellis's record for record - while the stream beside it goes through the staging area."""
    am, net, feats, _ = _cfg("small", n_utts=2)
    x = np.concatenate(feats)
    late = x.shape[0] - 40
    r = ib.viterbi_best(net, am, ib.gmm_loglik(am, x), [late])[late]
    chain = [(m, lab, t) for (m, lab, t, _s, _l) in r["chain"]]
    assert len(chain) > 64 and r["margin"] >= TOL * abs(r["score"]), (len(chain), r["margin"])
    dec = _decoder(net, am, True, max_streams=2)
    dec.stream_init(0); dec.stream_init(1)
    dec.streams_push([0, 1], [x[:late], x[:50]])
    l0, c0 = dec.best_stats()
    e = dec.streams_best([0, 1])
    l1, c1 = dec.best_stats()
    assert l1 - l0 == 1 and c1 - c0 == 3                              # (the heads and shares; stream 0's five arrays; its model row)
    assert e[0]["n_records"] == len(chain) and 0 < e[1]["n_records"] <= 64
    m = dec.stream_best_models(0)
    assert list(zip(m.model.tolist(), m.label.tolist(), m.time.tolist())) == chain
    assert _close(float(m.ac[-1]) + float(m.lm[-1]), r["chain"][-1][3]) and _close(m.lm[-1], r["chain"][-1][4])
    lab, tim = dec.stream_best_words(0)[:2]
    assert list(zip(lab.tolist(), tim.tolist())) == [(lab_, t) for (_m, lab_, t) in chain if lab_ != 0]
    assert dec.stream_best_models(1).n == e[1]["n_records"]
    dec.close()


# Phase X's work counters: how many closure items are written, expanded and walked (and how many Path records that takes) depends on
# the order in which the waves' tokens reach a state - a later, better arrival supersedes an item already written.  They differ between
# two identical decodes (tests/helpers.py holds tot_arcs_visited / tot_paths to the oracle by <= for the same reason); every other
# statistic - the reference's own (helpers.STAT_KEYS) and phase A's counters - is the search's and is compared.
RUN_DEPENDENT = ("tot_arcs_visited", "tot_paths", "tot_items_expanded", "tot_arcs_walked", "tot_closure_items")


def test_does_not_disturb_the_decode(built):
    """The same utterances through jd_streams_push in chunks under a trace interval of 50 and a Path arena small enough to
    collect between the chunks, once plain and once with jd_streams_best behind every chunk: hypotheses, statistics, partial
    lists and collection frames are the same bits, and behind every collection (remapped paths) the lists still hold together."""
    from helpers import STAT_KEYS
    assert not set(STAT_KEYS) & set(RUN_DEPENDENT)
    am, net, feats, _ = _cfg("small", n_utts=4)
    T = max(x.shape[0] for x in feats)
    trail, n_coll = [], 0
    for with_best in (False, True):
        dec = _decoder(net, am, False, max_streams=4, main_beam=150.0, max_paths=1 << 12)
        dec.set_partial_interval(50)
        for s in range(4):
            dec.stream_init(s)
        log = []
        for lo in range(0, T, 37):
            ss = [s for s in range(4) if lo < feats[s].shape[0]]
            dec.streams_push(ss, [feats[s][lo:lo + 37] for s in ss])
            if with_best:
                dec.streams_best(range(4))
                for s in ss:
                    _check_invariants(dec, s, min(lo + 37, feats[s].shape[0]), False, trace_now=False)
            log.append([(dec.stream_partial(s)[1], dec.stream_collect_info(s), dec.stream_path_counts(s)) for s in range(4)])
        n_coll = sum(dec.stream_collect_info(s)[0] for s in range(4))
        relaunches = dec.last_timing()["relaunches"]
        for s in range(4):
            g = dec.stream_finish(s)
            log.append((g.n, g.label.tobytes(), g.time.tobytes(), g.score.tobytes(), g.ac.tobytes(), g.lm.tobytes(), g.tot_score, g.tot_ac, g.tot_lm,
                        sorted((k, v) for k, v in g.stats.items() if k not in RUN_DEPENDENT), dec.stream_partial(s)[1]))
        assert n_coll > 0 or relaunches > 0
        trail.append(log)
        dec.close()
    assert n_coll >= 4, "Path collections were meant to run between the chunks (%d)" % n_coll
    assert len(trail[0]) == len(trail[1])
    for i, (a, b) in enumerate(zip(trail[0], trail[1])):
        assert a == b, "step %d" % i


def test_lazily_composed_network(built):
    """jd_net_create_lazy: the arc's in-label comes from the arena the search composes into - the entries and lists are, frame by
    frame, those on the jd_net_compose'd network, and hold together as above."""
    from juicer_amd import capi, synth
    am = synth.make_models(5, n_gmm=100, n_hmm=45, n_mix=2, n_tm=8, sep=0.6, with_tee=True)
    cl, g = synth.make_cl_g(5, am, n_words=40, n_succ=4, n_tri=30, with_sp=True)
    ncl, ng = capi.Network.from_synth(cl, 1.0, 0.0), capi.Network.from_synth(g, 1.0, 0.0)
    models = capi.Models.from_htk(am)
    static = capi.Network.compose(ncl, ng)
    lazy = capi.Network.lazy(ncl, ng, models, max_states=1 << 16, max_arcs=1 << 18)
    x = synth.sample_utterance(1005, g, am, 10)[0]
    for level in (False, True):
        a, b = _decoder(static, models, level, main_beam=300.0), _decoder(lazy, models, level, main_beam=300.0)
        a.stream_init(0); b.stream_init(0)
        n_words = 0
        for f in range(PUSH, x.shape[0] + 1, PUSH):
            a.stream_push(0, x[f - PUSH:f]); b.stream_push(0, x[f - PUSH:f])
            ea, eb = a.streams_best([0])[0], b.streams_best([0])[0]
            assert eb["found"] == 1 and eb["model"] >= 1
            assert ea == eb, (f, ea, eb)
            assert _lists(a, 0, level) == _lists(b, 0, level), f
            _check_invariants(b, 0, f, level)
            n_words = max(n_words, eb["n_words"])
        assert n_words >= 3
        a.close(); b.close()


def test_refusals(built, monkeypatch):
    from juicer_amd import capi
    am, net, feats, _ = _cfg("small", n_utts=2)
    gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
    dec = capi.Decoder(gnet, gam, max_streams=2, main_beam=150.0)
    dec.stream_init(0)
    for bad, code in (([0, 0], capi.JD_EINVAL), ([2], capi.JD_EINVAL), ([-1], capi.JD_EINVAL), ([0, 1], capi.JD_ESTATE)):
        with pytest.raises(capi.JuicerAmdError) as e:
            dec.streams_best(bad)
        assert e.value.code == code, bad
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.stream_best_words(1)                                       # (before its jd_stream_init)
    assert e.value.code == capi.JD_ESTATE
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.stream_best_models(0)                                      # (a word-level decoder)
    assert e.value.code == capi.JD_ESTATE
    dec.close()
    # a chain longer than the result capacity: that stream's entry fails, the other listed stream gets its own
    monkeypatch.setenv("JD_DEV", "1")
    monkeypatch.setenv("JD_RES_CAP", "16")
    dec = capi.Decoder(gnet, gam, max_streams=2, main_beam=150.0)
    dec.set_output_level(capi.OUTPUT_WORDS | capi.OUTPUT_MODELS)
    dec.stream_init(0); dec.stream_init(1)
    dec.streams_push([0, 1], [feats[0][:300], feats[1][:40]])
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.streams_best([0, 1])
    assert e.value.code == capi.JD_ENOMEM and "stream 0" in str(e.value) and "(> 16" in str(e.value), str(e.value)
    ent = e.value.entries
    assert ent[0]["found"] == 0 and ent[0]["frame"] == 300 and dec.stream_best_models(0).n == 0
    assert ent[1]["found"] == 1 and 0 < ent[1]["n_records"] <= 16 and dec.stream_best_models(1).n == ent[1]["n_records"]
    dec.close()
    monkeypatch.delenv("JD_RES_CAP")
    # a decoder a broker owns: its streams run on the resident kernel
    dec = capi.Decoder(gnet, gam, max_streams=1, main_beam=150.0)
    broker = capi.Broker(dec)
    assert broker.stats()["resident"]                                  # (the resident worker, the default)
    c = broker.open()
    broker.init(c)
    broker.push(c, feats[0][:100])
    assert broker.finish(c).n >= 0
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.streams_best([0])
    assert e.value.code == capi.JD_ESTATE and "broker" in str(e.value)
    broker.close()
    dec.close()
