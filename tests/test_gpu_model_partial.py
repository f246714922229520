"""Model-level partial traces (jd_stream_partial_models): the same tracePartialPath as jd_stream_partial, exported at model level -
every record from the root up to the word record the word list ends at, oldest first.

Per trace: its labelled entries are the word list of the same trace, it ends with a word, it is a prefix of the next trace's
list and of the final Hyp.models (reversed), field for field.  The word partials of a model-level decoder are a word-level
decoder's, trace for trace."""
import numpy as np
import pytest

import random_topology as rt

pytestmark = pytest.mark.gpu

WM = 1          # JD_OUTPUT_WORDS
MM = 1 | 2      # JD_OUTPUT_WORDS | JD_OUTPUT_MODELS


def _case(name):
    from juicer_amd import synth
    if name == "small":
        am, net, feats, _ = synth.config_small(n_utts=3)
    elif name == "mixed":
        am, net, feats, _ = synth.config_mixed(n_utts=3)
    else:
        seed = int(name.split("_")[1])
        am = synth.make_models(seed, n_gmm=40, n_hmm=12, n_mix=3, D=13, n_tm=4, with_tee=True)
        net = rt.random_net(seed, am, n_states=60, p_eps=0.2, p_label=0.35)
        feats = [rt.random_walk_features(seed * 10 + k, net, am) for k in range(3)]
    return am, net, feats


FIELDS = ("model", "label", "time", "score", "ac", "lm")


def _prefix(a, b, k, what):
    """the first k entries of ModelHyp-likes a and b (oldest first) are equal, field for field, bit for bit"""
    for f in FIELDS:
        x, y = np.asarray(getattr(a, f))[:k], np.asarray(getattr(b, f))[:k]
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), "%s: %s differs in the first %d entries" % (what, f, k)


def _run(dec, feats, chunk, level):
    """chunks pushed, a trace after each (alternately through either call: both read the same trace)"""
    out = []
    for x in feats:
        dec.stream_init(0)
        traces = []
        for j, i in enumerate(range(0, x.shape[0], chunk)):
            dec.stream_push(0, x[i:i + chunk])
            if level == WM:
                traces.append((dec.stream_partial(0, trace_now=True), None))
            elif j % 2 == 0:
                fm, m = dec.stream_partial_models(0, trace_now=True)
                fw, w = dec.stream_partial(0, trace_now=False)
                traces.append(((fm, w), m))
            else:
                fw, w = dec.stream_partial(0, trace_now=True)
                fm, m = dec.stream_partial_models(0, trace_now=False)
                traces.append(((fw, w), m))
        out.append((traces, dec.stream_finish(0)))
    return out


def _check(case, wres, mres):
    n_found = 0
    for u, ((wt, wh), (mt, mh)) in enumerate(zip(wres, mres)):
        assert len(wt) == len(mt)
        fin = mh.models
        assert fin is not None and fin.n >= 0, (case, u)
        old = type(fin)(n=fin.n, model=fin.model[::-1], label=fin.label[::-1], time=fin.time[::-1], score=fin.score[::-1],
                        ac=fin.ac[::-1], lm=fin.lm[::-1], tot_score=0.0, tot_ac=0.0, tot_lm=0.0)
        prev = None
        for j, ((wtrace, _), ((found, words), m)) in enumerate(zip(wt, mt)):
            what = "%s utt %d trace %d" % (case, u, j)
            assert wtrace == (found, words), what                      # word partials: a word-level decoder's
            lab = m.label != 0
            assert [(int(a), int(b)) for a, b in zip(m.label[lab], m.time[lab])] == words, what
            if m.n:
                assert m.label[-1] != 0, what                          # it ends at the record the word list ends at
                assert (m.model >= 0).all() and ((m.model != 0) | (m.label != 0)).all(), what
            if found:
                n_found += 1
            if prev is not None:
                assert prev.n <= m.n, what
                _prefix(prev, m, prev.n, what)
            # a prefix of the final chain; the final entry 0 carries the final state's weight (jd_model_hyp), a trace not
            assert m.n <= fin.n, what
            k = m.n if m.n < fin.n else m.n - 1
            _prefix(m, old, k, what)
            if m.n == fin.n and m.n:
                for f in ("model", "label", "time"):
                    assert getattr(m, f)[-1] == getattr(old, f)[-1], what
            prev = m
    return n_found


def _traced(case):
    from juicer_amd import capi
    am, net, feats = _case(case)
    gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
    chunk = 29 if case in ("small", "mixed") else max(3, min(x.shape[0] for x in feats) // 5)
    res = []
    for level in (WM, MM):
        d = capi.Decoder(gnet, gam, main_beam=150.0, max_streams=1)
        d.set_output_level(level)
        res.append(_run(d, feats, chunk, level))
        d.close()
    return _check(case, *res)


@pytest.mark.parametrize("case", ["small", "mixed"])
def test_model_partials_are_word_partials_at_model_level(built, case):
    assert _traced(case) > 0, case


def test_model_partials_on_random_topologies(built):
    """(on some random graphs no record is common to every token before the end: those traces find nothing, and their lists
    stay empty - checked all the same)"""
    assert sum(_traced(case) for case in ("random_3", "random_8")) > 0


def test_model_partials_across_collections(built, monkeypatch):
    """several chunks per push (JD_FC=16) and a small Path arena: collections renumber the records between traces"""
    from juicer_amd import capi, synth
    monkeypatch.setenv("JD_DEV", "1")
    monkeypatch.setenv("JD_FC", "16")
    am, net, feats, _ = synth.config_small(n_utts=3)
    gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
    res = []
    for level in (WM, MM):
        d = capi.Decoder(gnet, gam, main_beam=150.0, max_streams=1, max_paths=1 << 12)
        d.set_output_level(level)
        res.append(_run(d, feats, 40, level))
        d.close()
    # (4096 records hold a fraction of what a model-level utterance writes: the decode collects on the way, or fails)
    assert _check("collections", *res) > 0


def test_word_level_decoder_refuses_and_capacity(built, monkeypatch):
    from juicer_amd import capi, synth
    am, net, feats, _ = synth.config_small(n_utts=1)
    gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
    d = capi.Decoder(gnet, gam, main_beam=150.0, max_streams=1)
    d.stream_init(0)
    d.stream_push(0, feats[0][:40])
    with pytest.raises(capi.JuicerAmdError) as e:
        d.stream_partial_models(0, trace_now=True)
    assert e.value.code == capi.JD_ESTATE
    d.stream_finish(0)
    d.close()
    # a chain longer than the result capacity: JD_ENOMEM, as the word partial's
    monkeypatch.setenv("JD_DEV", "1")
    monkeypatch.setenv("JD_RES_CAP", "16")
    d = capi.Decoder(gnet, gam, main_beam=150.0, max_streams=1)
    d.set_output_level(MM)
    d.stream_init(0)
    x = feats[0]
    hit = False
    for i in range(0, x.shape[0], 20):
        d.stream_push(0, x[i:i + 20])
        try:
            f, m = d.stream_partial_models(0, trace_now=True)
            assert m.n <= 16
        except capi.JuicerAmdError as err:
            assert err.code == capi.JD_ENOMEM and "model-level partial" in str(err)
            hit = True
            break
    assert hit
    d.close()
