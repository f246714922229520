"""The end-of-utterance view of live streams: jd_streams_final (k_final_many), jd_stream_final_words / _models.

The definition is "what jd_stream_finish would return now": every entry is held, bit for bit and field for field, to the finish of a
twin decoder that was pushed the same prefix; the word view is held to the CPU oracle's decode of the prefix the way a finished
hypothesis is (helpers.assert_hyp_matches); and a decoder that is looked at after every push is the decoder that never is."""
import types

import numpy as np
import pytest

from helpers import STAT_KEYS, assert_hyp_matches
from live_cases import CASES, MFIELDS, RUN_DEPENDENT, _bits, _case, _decoder, _fbits, _handles

pytestmark = pytest.mark.gpu

FIELDS = ("found", "frame", "n_words", "n_records", "score", "ac", "lm")
def _view(dec, s, models):
    """stream s's lists as of the last streams_final: (five word lists, six model lists or None), floats as their bits"""
    w = tuple(_bits(a) for a in dec.stream_final_words(s))
    if not models:
        return w, None
    m = dec.stream_final_models(s)
    return w, tuple(_bits(getattr(m, k)) for k in MFIELDS)


def _assert_is_finish(e, view, h, models, what):
    """entry e and lists `view` of jd_streams_final are the Hyp h of a jd_stream_finish behind the same frames: reversed, entry for
    entry and bit for bit, the totals included (jd_stream_finish gives an empty result LOG_ZERO totals: the head says the token's)"""
    words, mlist = view
    assert e["found"] == (1 if h.n >= 0 else 0), (what, e, h.n)
    if not e["found"]:
        assert [e[f] for f in FIELDS[2:]] == [0, 0, 0.0, 0.0, 0.0] and all(len(l) == 0 for l in words), (what, e)
        assert mlist is None or all(len(l) == 0 for l in mlist), what
        return
    assert e["n_words"] == h.n, (what, e, h.n)
    for got, f in zip(words, ("label", "time", "score", "ac", "lm")):
        assert got[::-1] == _bits(getattr(h, f)[:h.n]), (what, f)
    tot = None
    if models:
        m = h.models
        assert e["n_records"] == m.n >= h.n, (what, e, m.n)
        for got, f in zip(mlist, MFIELDS):
            assert got[::-1] == _bits(getattr(m, f)[:m.n]), (what, f)
        if m.n > 0:
            tot = (m.tot_score, m.tot_ac, m.tot_lm)
    else:
        assert e["n_records"] == h.n, (what, e)
        if h.n > 0:
            tot = (h.tot_score, h.tot_ac, h.tot_lm)
    if tot is not None:
        assert [_fbits(e[f]) for f in ("score", "ac", "lm")] == [_fbits(t) for t in tot], (what, e, tot)
    assert e["score"] > -1e30, (what, e)


def _twin_finish(twin, x, f):
    twin.stream_init(0)
    if f > 0:
        twin.stream_push(0, x[:f])
    return twin.stream_finish(0)


@pytest.mark.parametrize("max_paths", [0, 1 << 12], ids=["plain", "collecting"])
@pytest.mark.parametrize("models", [False, True], ids=["words", "models"])
@pytest.mark.parametrize("name", CASES)
def test_definition(built, name, models, max_paths):
    """Three streams on three utterances, advanced by jd_streams_push in unequal steps - stream 2 a call behind, every third call
    lists stream 1 without frames - and after every call the final view of all three is the finish of a twin decoder pushed the
    same prefix.  `collecting`: a Path arena of 4096 records, so that collections renumber the records between the looks."""
    _, _, feats, _, steps = _handles(name)
    dec, twin = _decoder(name, models, max_streams=3, max_paths=max_paths), _decoder(name, models, max_streams=1, max_paths=max_paths)
    for s in range(3):
        dec.stream_init(s)
    assert dec.streams_final([0, 1, 2]) == [dict(zip(FIELDS, (0, 0, 0, 0, 0.0, 0.0, 0.0)))] * 3
    T = [0, 0, 0]
    seen = set()
    for call in range(6):
        ss, fr = [], []
        for s in range(3):
            if s == 2 and call == 0:
                continue                                               # (a call behind)
            n = 0 if (s == 1 and call % 3 == 2) else min(steps[s], feats[s].shape[0] - T[s])
            ss.append(s); fr.append(feats[s][T[s]:T[s] + n])
            T[s] += n
        dec.streams_push(ss, fr)
        l0, c0 = dec.final_stats()
        ent = dec.streams_final([2, 0, 1])
        l1, c1 = dec.final_stats()
        assert l1 - l0 == (1 if max(T) > 0 else 0) and c1 - c0 >= l1 - l0
        for e, s in zip(ent, (2, 0, 1)):
            assert e["frame"] == T[s]
            h = _twin_finish(twin, feats[s], T[s])
            _assert_is_finish(e, _view(dec, s, models), h, models, (name, call, s, T[s]))
            seen.add((e["found"], min(e["n_records"], 1)))
    assert (1, 1) in seen and (0, 0) in seen, seen
    dec.close(); twin.close()


@pytest.mark.parametrize("name", ["small", "mixed", "random_3", "random_5"])
def test_against_the_oracle(built, name):
    """The word view behind frames 1, 14, every 50th and the last one against OracleDecoder.decode(x[:f]), compared the way a
    finished hypothesis is (helpers.assert_hyp_matches: labels and times exact, scores to 1e-4), at both output levels.
    found == (oracle n >= 0); on these fixtures the oracle has no final hypothesis at a 1-frame prefix and has one from frame 14
    on, and the third random_3 utterance ends with a hypothesis of 0 records - each is asserted to have been seen."""
    from oracle.oracle import OracleAM, OracleDecoder, OracleNet
    seen = {"none": 0, "some": 0, "empty": 0}
    am, net, feats, kw, _ = _case(name)
    od = OracleDecoder(OracleNet(net), OracleAM(am), **kw)
    ora = {}
    for models in (False, True):
        dec = _decoder(name, models, max_streams=1)
        for u, x in enumerate(feats if name.startswith("random") else feats[:1]):
            T = x.shape[0]
            dec.stream_init(0)
            at = 0
            for f in sorted({1, min(14, T), T} | set(range(50, T, 50))):
                dec.stream_push(0, x[at:f])
                at = f
                e = dec.streams_final([0])[0]
                if (u, f) not in ora:
                    ora[(u, f)] = od.decode(x[:f])
                o = ora[(u, f)]
                what = "%s %s utt %d frame %d" % (name, "models" if models else "words", u, f)
                assert e["found"] == (1 if o.n >= 0 else 0) and e["frame"] == f, (what, e, o.n)
                lab, tim, sc, ac, lm = (a[::-1] for a in dec.stream_final_words(0))
                got = types.SimpleNamespace(n=e["n_words"] if e["found"] else -1, label=lab, time=tim, score=sc, ac=ac, lm=lm,
                                            tot_score=e["score"], tot_ac=e["ac"], tot_lm=e["lm"])
                assert_hyp_matches(got, o, what, check_stats=False)
                seen["none" if not e["found"] else "some" if e["n_words"] else "empty"] += 1
                if not models:
                    assert e["n_records"] == e["n_words"], what
                if f == 1:
                    assert e["found"] == 0, what
                elif f >= 14:
                    assert e["found"] == 1, what
            g = dec.stream_finish(0)
            assert g.n == (e["n_words"] if e["found"] else -1)
        dec.close()
    assert seen["none"] and seen["some"] and (seen["empty"] or name != "random_3"), seen


def _finish_log(dec, s):
    g = dec.stream_finish(s)
    out = [g.n, g.label.tobytes(), g.time.tobytes(), g.score.tobytes(), g.ac.tobytes(), g.lm.tobytes(), _fbits(g.tot_score), _fbits(g.tot_ac), _fbits(g.tot_lm),
           sorted((k, v) for k, v in g.stats.items() if k not in RUN_DEPENDENT), dec.stream_partial(s)[1]]
    if getattr(g, "models", None) is not None:
        out.append([g.models.n] + [getattr(g.models, f).tobytes() for f in MFIELDS])
    return g, out


@pytest.mark.parametrize("models", [False, True], ids=["words_interval_150", "models"])
def test_nothing_is_disturbed(built, models):
    """A decoder looked at after every push - final, best and (word level, interval 150) the scheduled traces, interleaved - is the
    decoder that never is: jd_stream_finish results and statistics, jd_stream_partial lists, jd_stream_collect_info,
    jd_stream_path_counts (where they are the reference's counts: under the interval) and jd_streams_best are the same bits.  And the last final view, taken at the frame the stream is
    finished at, is that finish."""
    assert not set(STAT_KEYS) & set(RUN_DEPENDENT)
    _, _, feats, _, _ = _handles("small")
    T = max(x.shape[0] for x in feats)
    trail, n_coll = [], 0
    for looked_at in (False, True):
        dec = _decoder("small", models, max_streams=3, max_paths=1 << 12)
        if not models:
            dec.set_partial_interval(150)
        for s in range(3):
            dec.stream_init(s)
        log, last = [], {}
        for lo in range(0, T, 37):
            ss = [s for s in range(3) if lo < feats[s].shape[0]]
            dec.streams_push(ss, [feats[s][lo:lo + 37] for s in ss])
            if looked_at:
                dec.streams_best([1, 0])
                ent = dec.streams_final(range(3))
                for s in range(3):
                    last[s] = (ent[s], _view(dec, s, models))
                dec.streams_best([2])
                dec.streams_final([1])
            best = dec.streams_best(range(3))
            counts = [dec.stream_path_counts(s) for s in range(3)]
            # (without the reference's counts - no interval - the figures are the arena's own records, which phase X writes in a
            # run-dependent number, RUN_DEPENDENT's tot_paths: only that they are the arena's is compared then)
            log.append([(best[s], dec.stream_partial(s)[1], dec.stream_collect_info(s), counts[s] if counts[s][2] else counts[s][2]) for s in range(3)])
        n_coll = sum(dec.stream_collect_info(s)[0] for s in range(3))
        for s in range(3):
            g, entry = _finish_log(dec, s)
            log.append(entry)
            if looked_at:
                _assert_is_finish(last[s][0], last[s][1], g, models, ("the last view", s))
                assert last[s][0]["frame"] == feats[s].shape[0]
        trail.append(log)
        dec.close()
    if not models:
        assert n_coll >= 3, "Path collections were meant to run between the chunks (%d)" % n_coll
    assert len(trail[0]) == len(trail[1])
    for i, (a, b) in enumerate(zip(trail[0], trail[1])):
        assert a == b, "step %d" % i


def test_shares_and_counters(built):
    """A late look on concatenated utterances at model level: more records than a share of k_final_many's staging area (64), so the
    list comes from the stream's result arrays - the twin's finish record for record - while the stream beside it goes through the
    staging area.  One launch per call; one copy per call when every chain fits its share."""
    _, _, feats, _, _ = _handles("small")
    x = np.concatenate(feats)
    dec, twin = _decoder("small", True, max_streams=2), _decoder("small", True, max_streams=1)
    dec.stream_init(0); dec.stream_init(1)
    dec.streams_push([0, 1], [x, x[:50]])
    l0, c0 = dec.final_stats()
    e = dec.streams_final([0, 1])
    l1, c1 = dec.final_stats()
    assert e[0]["n_records"] > 64 >= e[1]["n_records"] > 0, e
    assert l1 - l0 == 1 and c1 - c0 == 3                              # (the heads and shares; stream 0's five arrays; its model row)
    _assert_is_finish(e[0], _view(dec, 0, True), _twin_finish(twin, x, x.shape[0]), True, "beyond the share")
    _assert_is_finish(e[1], _view(dec, 1, True), _twin_finish(twin, x, 50), True, "within the share")
    e1 = dec.streams_final([1])
    l2, c2 = dec.final_stats()
    assert (l2 - l1, c2 - c1) == (1, 1) and e1[0] == e[1]
    assert dec.streams_final([]) == [] and dec.final_stats() == (l2, c2)
    dec.close(); twin.close()


def test_lazily_composed_network(built):
    """jd_net_create_lazy: the view is, frame by frame, the one on the jd_net_compose'd network, and the lazily composed network is
    not left (the finish that follows is the composed one's)."""
    from juicer_amd import capi, synth
    am = synth.make_models(5, n_gmm=100, n_hmm=45, n_mix=2, n_tm=8, sep=0.6, with_tee=True)
    cl, g = synth.make_cl_g(5, am, n_words=40, n_succ=4, n_tri=30, with_sp=True)
    ncl, ng = capi.Network.from_synth(cl, 1.0, 0.0), capi.Network.from_synth(g, 1.0, 0.0)
    gam = capi.Models.from_htk(am)
    static = capi.Network.compose(ncl, ng)
    lazy = capi.Network.lazy(ncl, ng, gam, max_states=1 << 16, max_arcs=1 << 18)
    x = synth.sample_utterance(1005, g, am, 10)[0]
    a, b = capi.Decoder(static, gam, main_beam=300.0), capi.Decoder(lazy, gam, main_beam=300.0)
    a.stream_init(0); b.stream_init(0)
    n_found = 0
    for f in range(25, x.shape[0] + 1, 25):
        a.stream_push(0, x[f - 25:f]); b.stream_push(0, x[f - 25:f])
        ea, eb = a.streams_final([0])[0], b.streams_final([0])[0]
        assert ea == eb and _view(a, 0, False) == _view(b, 0, False), (f, ea, eb)
        n_found += eb["found"]
    assert n_found >= 3
    ga, gb = a.stream_finish(0), b.stream_finish(0)
    assert ga.n == gb.n and _bits(ga.label) == _bits(gb.label) and _bits(ga.score) == _bits(gb.score)
    a.close(); b.close()


def test_refusals(built, monkeypatch):
    from juicer_amd import capi
    gnet, gam, feats, _, _ = _handles("small")
    dec = capi.Decoder(gnet, gam, max_streams=2, main_beam=150.0)
    dec.stream_init(0)
    for bad, code in (([0, 0], capi.JD_EINVAL), ([2], capi.JD_EINVAL), ([-1], capi.JD_EINVAL), ([0, 1], capi.JD_ESTATE)):
        with pytest.raises(capi.JuicerAmdError) as e:
            dec.streams_final(bad)
        assert e.value.code == code, bad
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.stream_final_words(1)                                      # (before its jd_stream_init)
    assert e.value.code == capi.JD_ESTATE
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.stream_final_models(0)                                     # (a word-level decoder)
    assert e.value.code == capi.JD_ESTATE
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.streams_trace_models([0])                                  # (a word-level decoder: jd_streams_trace is its call)
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
        dec.streams_final([0, 1])
    assert e.value.code == capi.JD_ENOMEM and "stream 0" in str(e.value) and "(> 16" in str(e.value), str(e.value)
    ent = e.value.entries
    assert ent[0]["found"] == 0 and ent[0]["frame"] == 300 and dec.stream_final_models(0).n == 0
    assert ent[1]["found"] == 1 and 0 < ent[1]["n_records"] <= 16 and dec.stream_final_models(1).n == ent[1]["n_records"]
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
        dec.streams_final([0])
    assert e.value.code == capi.JD_ESTATE and "broker" in str(e.value)
    broker.close()
    dec.close()
