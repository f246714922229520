"""Model-level output (jd_dec_set_output_level(JD_OUTPUT_WORDS | JD_OUTPUT_MODELS)): which model the best path passed and in which
frames, beside the words.

Two anchors.  Invariance: the search is the same in either mode, so the words of a model-level decode are those of word mode bit
for bit - labels, times, scores, totals - through every flow and kernel.  Structure: the model chain, oldest first, is a path of the
graph from the initial state to a final state (arcs without a model and a word leave no entry), its word labels are the words, its
times never decrease, and only a tee model (or a label-only entry) takes zero frames."""
import numpy as np
import pytest

import indep_cases
import indep_viterbi_np as iv
import random_topology as rt
from helpers import bit_exact

pytestmark = pytest.mark.gpu

WM = 1          # JD_OUTPUT_WORDS
MM = 1 | 2      # JD_OUTPUT_WORDS | JD_OUTPUT_MODELS


def _tee_models(am):
    """in-labels (HMM index + 1) of the models that have a tee transition (the rule of tests/indep_viterbi_np.py)"""
    out = set()
    for h in range(am.n_hmm):
        n = int(am.hmm_nstates[h]); a = am.transp[am.hmm_tm[h]]
        sucs = [j for j in range(n) if a[0, j] > 0]
        if (n - 1) in sucs[1:]:
            out.add(h + 1)
    return out


def _words_of(m):
    keep = m.label != 0
    return m.label[keep], m.time[keep]


def check_model_chain(net, am, hyp, what=""):
    """hyp.models against the graph (see the module's docstring) and against hyp's own words"""
    m = hyp.models
    assert m is not None, what
    if hyp.n < 0:
        assert m.n == -1, what
        return
    assert m.n >= hyp.n, what
    lab, tim = _words_of(m)
    assert np.array_equal(lab, hyp.label) and np.array_equal(tim, hyp.time), what
    if hyp.n > 0:                                                     # (no word: jd_hyp's totals are DecHyp()'s defaults, as in word mode)
        assert (m.tot_score, m.tot_ac, m.tot_lm) == (hyp.tot_score, hyp.tot_ac, hyp.tot_lm), what
    if m.n > 0:
        assert (m.score[0], m.ac[0], m.lm[0]) == (m.tot_score, m.tot_ac, m.tot_lm), what
    # oldest first
    mod, lab, tim = m.model[::-1].tolist(), m.label[::-1].tolist(), m.time[::-1].tolist()
    tees = _tee_models(am)
    prev = 0
    for k in range(m.n):
        assert tim[k] >= prev, "%s: times decrease at entry %d" % (what, k)
        # (frame 0 holds both what passed before the first frame and what left a model in it: not told apart there)
        if tim[k] == prev and prev > 0 and mod[k] != 0:
            assert mod[k] in tees, "%s: model %d of zero frames at entry %d is no tee model" % (what, mod[k], k)
        prev = tim[k]
    # a path of the graph: NFA walk over the arcs that leave an entry, closed over the ones that leave none (epsilon:epsilon)
    src, dst, il, ol = (np.asarray(a, np.int64) for a in (net.src, net.dst, net.ilab, net.olab))
    silent = (il == 0) & (ol == 0)

    def close(states):
        states = set(states)
        todo = list(states)
        while todo:
            s = todo.pop()
            for a in np.flatnonzero((src == s) & silent).tolist():
                d = int(dst[a])
                if d not in states:
                    states.add(d); todo.append(d)
        return states
    cur = close({int(src[0])})
    for k in range(m.n):
        nxt = set()
        for s in cur:
            sel = (src == s) & (il == mod[k]) & (ol == lab[k])
            nxt.update(dst[sel].tolist())
        assert nxt, "%s: entry %d (model %d, label %d) leaves none of the states reached" % (what, k, mod[k], lab[k])
        cur = close(nxt)
    assert cur & set(np.asarray(net.fstate).tolist()), "%s: the chain ends in no final state" % what


def _both(make_dec, run):
    """run(dec) under word output and under model-level output (a fresh decoder each)"""
    out = []
    for level in (WM, MM):
        d = make_dec()
        d.set_output_level(level)
        assert d.output_level() == level
        out.append(run(d))
        d.close()
    return out


def _same_words(a, b, what):
    assert len(a) == len(b)
    for u, (x, y) in enumerate(zip(a, b)):
        assert x.models is None and y.models is not None
        assert bit_exact(y, x), "%s utt %d" % (what, u)
        assert (x.tot_score, x.tot_ac, x.tot_lm) == (y.tot_score, y.tot_ac, y.tot_lm), "%s utt %d" % (what, u)


@pytest.mark.parametrize("case", sorted(indep_cases.CASES))
def test_every_beam_off_words_and_models(built, case):
    """Every beam off: the words are the independent Viterbi's (tests/indep_viterbi_np.py), and the model chain is a path of the graph
    that carries them (tee models, HMMs of 1-6 emitting states, epsilon:word arcs)."""
    from juicer_amd import capi
    am, net, feats, _ = indep_cases.CASES[case]()
    gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
    a, b = _both(lambda: capi.Decoder(gnet, gam, max_streams=len(feats)), lambda d: d.decode_batch(feats))
    _same_words(a, b, case)
    for u, x in enumerate(feats):
        indep_cases.check_against_viterbi(b[u], iv.viterbi(net, am, iv.gmm_loglik(am, x)), "%s utt %d" % (case, u))
        check_model_chain(net, am, b[u], "%s utt %d" % (case, u))
    tees = _tee_models(am)
    if tees:
        assert any(np.isin(h.models.model, list(tees)).any() for h in b), case


def test_model_level_default_is_words_only(built):
    from juicer_amd import capi, synth
    am, net, feats, _ = synth.config_toy()
    dec = capi.Decoder(capi.Network.from_synth(net), capi.Models.from_htk(am), main_beam=150.0)
    assert dec.output_level() == WM
    assert dec.decode_batch(feats[:1])[0].models is None
    with pytest.raises(capi.JuicerAmdError):
        dec.model_result(0)
    with pytest.raises(capi.JuicerAmdError):
        dec.set_output_level(2)                                        # (words are always there)
    dec.close()


@pytest.mark.parametrize("flow", ["serial", "two", "resident"])
def test_flows_give_word_mode_words(built, flow):
    from juicer_amd import capi, synth
    am, net, feats, _ = synth.config_small(n_utts=6)
    gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
    mode = {"serial": capi.FLOW_SERIAL, "two": capi.FLOW_TWO_IN_FLIGHT, "resident": capi.FLOW_RESIDENT}[flow]

    def make():
        d = capi.Decoder(gnet, gam, main_beam=150.0, max_streams=4)
        d.set_pipeline(mode)
        return d

    def run(d):
        return d.decode_batch(feats[:3]) + d.decode_batch(feats[3:])  # (two batches: the second one behind the first)
    a, b = _both(make, run)
    _same_words(a, b, flow)
    for u, h in enumerate(b):
        check_model_chain(net, am, h, "%s utt %d" % (flow, u))


def test_streaming_and_partial_give_word_mode_words(built):
    from juicer_amd import capi, synth
    am, net, feats, _ = synth.config_small(n_utts=2)
    gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)

    def run(d):
        res, parts = [], []
        for x in feats:
            d.stream_init(0)
            for i in range(0, x.shape[0], 29):
                d.stream_push(0, x[i:i + 29])
                parts.append(d.stream_partial(0, trace_now=True))
            res.append(d.stream_finish(0))
        return res, parts
    (a, pa), (b, pb) = _both(lambda: capi.Decoder(gnet, gam, main_beam=150.0, max_streams=1), run)
    _same_words(a, b, "streamed")
    assert pa == pb
    for u, h in enumerate(b):
        check_model_chain(net, am, h, "streamed utt %d" % u)


@pytest.mark.parametrize("slot", [False, True])
def test_slot_kernel_and_one_workgroup_streams(built, monkeypatch, slot):
    from juicer_amd import capi, synth
    monkeypatch.setenv("JD_DEV", "1")
    monkeypatch.setenv("JD_SLOT_BATCH", "1" if slot else "0")
    monkeypatch.setenv("JD_CW", "1")
    am, net, feats, _ = synth.config_mixed(n_utts=4)
    gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
    a, b = _both(lambda: capi.Decoder(gnet, gam, main_beam=180.0, max_streams=len(feats)), lambda d: (d.decode_batch(feats), d.last_timing()))
    assert (a[1]["slot_launches"] > 0) == slot and (b[1]["slot_launches"] > 0) == slot
    _same_words(a[0], b[0], "slot" if slot else "k_search")
    for u, h in enumerate(b[0]):
        check_model_chain(net, am, h, "utt %d" % u)


def test_chunks_and_collections(built, monkeypatch):
    """several chunks per decode (JD_FC) and a small Path arena: collections in between"""
    from juicer_amd import capi, synth
    monkeypatch.setenv("JD_DEV", "1")
    monkeypatch.setenv("JD_FC", "16")
    am, net, feats, _ = synth.config_small(n_utts=4)
    gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
    a, b = _both(lambda: capi.Decoder(gnet, gam, main_beam=150.0, max_streams=4, max_paths=1 << 14), lambda d: d.decode_batch(feats))
    _same_words(a, b, "chunks")
    for u, h in enumerate(b):
        check_model_chain(net, am, h, "utt %d" % u)


@pytest.mark.parametrize("seed", [3, 8, 21])
def test_random_topologies(built, seed):
    from juicer_amd import capi, synth
    am = synth.make_models(seed, n_gmm=40, n_hmm=12, n_mix=3, D=13, n_tm=4, with_tee=True)
    net = rt.random_net(seed, am, n_states=60, p_eps=0.2, p_label=0.35)
    feats = [rt.random_walk_features(seed * 10 + k, net, am) for k in range(3)]
    gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
    for kw in (dict(), dict(main_beam=60.0, end_beam=40.0, word_beam=30.0)):
        a, b = _both(lambda: capi.Decoder(gnet, gam, max_streams=3, **kw), lambda d: d.decode_batch(feats))
        _same_words(a, b, "seed %d %s" % (seed, kw))
        for u, h in enumerate(b):
            check_model_chain(net, am, h, "seed %d utt %d %s" % (seed, u, kw))


def test_lazily_composed_network(built):
    """a network composed while it is searched (jd_net_create_lazy): the k_search flavour that reads its arcs from the arena"""
    from juicer_amd import capi, synth
    am = synth.make_models(31, n_gmm=60, n_hmm=30, n_mix=4, D=13, with_tee=True)
    cl, g = synth.make_cl_g(31, am, n_words=60, n_succ=4, n_tri=0, with_sp=True)
    models = capi.Models.from_htk(am)
    ncl, ng = capi.Network.from_synth(cl, 1.0, 0.0), capi.Network.from_synth(g, 1.0, 0.0)
    lazy = capi.Network.lazy(ncl, ng, models, max_states=1 << 16, max_arcs=1 << 18)
    feats = [synth.sample_utterance(1031 + u, g, am, 5 + u)[0] for u in range(3)]
    a, b = _both(lambda: capi.Decoder(lazy, models, main_beam=300.0, max_streams=3), lambda d: d.decode_batch(feats))
    _same_words(a, b, "lazy")
    for h in b:
        assert h.n > 0 and h.models.n > h.n
        assert (h.models.model > 0).sum() >= h.n


def test_small_arena_and_broker(built):
    from juicer_amd import capi, synth
    am, net, feats, _ = synth.config_small(n_utts=1)
    gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
    dec = capi.Decoder(gnet, gam, main_beam=150.0, max_paths=64)
    dec.set_output_level(MM)
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.decode_batch(feats)
    assert "Path records" in str(e.value)
    dec.close()
    dec = capi.Decoder(gnet, gam, main_beam=150.0, max_streams=2)
    dec.set_output_level(MM)
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.Broker(dec, 2)
    assert "JD_OUTPUT_MODELS" in str(e.value)
    with pytest.raises(capi.JuicerAmdError):
        dec.set_partial_interval(50)
    dec.set_output_level(WM)
    dec.set_partial_interval(50)
    with pytest.raises(capi.JuicerAmdError):
        dec.set_output_level(MM)
    dec.close()


def _rel(a, b, scale):
    return abs(float(a) - float(b)) <= 1e-5 * abs(scale) + 1e-3


@pytest.mark.parametrize("case", sorted(indep_cases.CASES))
def test_every_beam_off_model_chain_is_the_independent_trellis(built, case):
    """Every beam off: the model chain - models, word labels, boundary frames, the score and ac of every entry and so every
    segment's ac - is that of tests/indep_viterbi_models.py (ac and lm: the decoder's score is normalised per frame), a float64 trellis that keeps model boundaries in its back-pointers."""
    import indep_viterbi_models as ivm
    from juicer_amd import capi
    am, net, feats, _ = indep_cases.CASES[case]()
    dec = capi.Decoder(capi.Network.from_synth(net), capi.Models.from_htk(am), max_streams=len(feats))
    dec.set_output_level(MM)
    hyps = dec.decode_batch(feats)
    dec.close()
    n_tee = 0
    for u, x in enumerate(feats):
        what = "%s utt %d" % (case, u)
        ref = ivm.viterbi_models(net, am, iv.gmm_loglik(am, x))
        m = hyps[u].models
        assert ref is not None and m.n == len(ref[2]), (what, m.n, len(ref[2]))
        chain = ref[2][::-1]                                           # newest first, like the decoder's
        assert m.model.tolist() == [r[0] for r in chain], what
        assert m.label.tolist() == [r[1] for r in chain], what
        assert m.time.tolist() == [r[2] for r in chain], what
        tot, tot_lm = ref[0], ref[1]
        # (the decoder's score is normalised frame by frame - WFSTDecoderLite's bestEmitScore - ac and lm are not)
        assert _rel(m.tot_ac, tot - tot_lm, tot) and _rel(m.tot_lm, tot_lm, tot), what
        for k in range(1, m.n):                                        # (entry 0 carries the final weight: the totals)
            s, lm = chain[k][3], chain[k][4]
            assert _rel(m.ac[k], s - lm, tot) and _rel(m.lm[k], lm, tot), (what, k, float(m.ac[k]), s - lm, float(m.lm[k]), lm)
        n_tee += sum(1 for k in range(1, m.n) if m.time[k - 1] == m.time[k] and m.model[k - 1] != 0)
    assert n_tee > 0 or not _tee_models(am), case                      # (zero-frame models were met)


def _hmm_segment(am, h, ll):
    """float64 Viterbi of HMM h (in-label - 1) from its entry state to its exit state over the frames of ll ([n, G])"""
    n = int(am.hmm_nstates[h])
    with np.errstate(divide="ignore"):
        A = np.log(am.transp[am.hmm_tm[h]][:n, :n].astype(np.float64))
    g = am.hmm_gmm[h]
    d = np.full(n, -np.inf); d[0] = 0.0
    for t in range(ll.shape[0]):
        e = np.full(n, -np.inf)
        for j in range(1, n - 1):
            e[j] = np.max(d[:n - 1] + A[:n - 1, j]) + ll[t, g[j]]
        d = e
        d[0] = -np.inf
    return float(np.max(d[1:n - 1] + A[1:n - 1, n - 1]))


def test_bench_beam_segments_are_model_viterbis(built):
    """configs[1]-shaped data at the bench's beam: every segment of a model that took frames carries at most - and almost always
    exactly - the acoustic score of that HMM's own float64 Viterbi over its frames on jd_am_score_frames likelihoods (a pruned
    internal alignment can only score lower)"""
    from juicer_amd import capi, synth
    am, net, feats, _ = synth.config_c2(seed=0, n_utts=4)
    gam = capi.Models.from_htk(am)
    dec = capi.Decoder(capi.Network.from_synth(net), gam, main_beam=150.0, max_streams=len(feats))
    dec.set_output_level(MM)
    hyps = dec.decode_batch(feats)
    dec.close()
    n_seg = n_eq = 0
    for u, (h, x) in enumerate(zip(hyps, feats)):
        assert h.n > 0
        check_model_chain(net, am, h, "utt %d" % u)
        ll = gam.score_frames(x).astype(np.float64)
        mod, tim, ac = h.models.model[::-1], h.models.time[::-1], h.models.ac[::-1].astype(np.float64)
        for k in range(1, h.models.n - 1):                            # (the newest entry's ac has the final weight's share; k = 0: frame 0 is ambiguous)
            a, b = int(tim[k - 1]) + 1, int(tim[k])
            if mod[k] == 0 or b < a:
                continue
            want = _hmm_segment(am, int(mod[k]) - 1, ll[a:b + 1])
            got = ac[k] - ac[k - 1]
            tol = 1e-5 * abs(ac[-1]) + 1e-3
            assert got <= want + tol, ("utt %d entry %d" % (u, k), got, want)
            n_seg += 1
            n_eq += abs(got - want) <= tol
    assert n_seg > 100 and n_eq >= 0.95 * n_seg, (n_seg, n_eq)


def test_level_switch_refused_mid_utterance(built):
    from juicer_amd import capi, synth
    am, net, feats, _ = synth.config_small(n_utts=1)
    dec = capi.Decoder(capi.Network.from_synth(net), capi.Models.from_htk(am), main_beam=150.0)
    dec.set_output_level(MM)
    dec.stream_init(0)
    dec.stream_push(0, feats[0][:50])
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.set_output_level(WM)
    assert "under way" in str(e.value)
    dec.stream_push(0, feats[0][50:])
    h = dec.stream_finish(0)
    assert h.models is not None and h.models.n >= h.n > 0
    dec.set_output_level(WM)                                           # (between utterances: fine)
    dec.stream_init(0)
    dec.stream_push(0, feats[0][:50])
    with pytest.raises(capi.JuicerAmdError):
        dec.set_output_level(MM)
    dec.stream_push(0, feats[0][50:])
    assert bit_exact(dec.stream_finish(0), h)
    dec.close()


def test_result_capacity_and_collections(built, monkeypatch):
    """a model chain longer than the result capacity fails with JD_ENOMEM (words of the same decode fit); a small arena collects
    (k_search relaunches, the resident pipeline's collections) and the words stay word mode's"""
    from juicer_amd import capi, synth
    monkeypatch.setenv("JD_DEV", "1")
    monkeypatch.setenv("JD_RES_CAP", "20")
    am, net, feats, _ = synth.config_small(n_utts=4)
    gnet, gam = capi.Network.from_synth(net), capi.Models.from_htk(am)
    dec = capi.Decoder(gnet, gam, main_beam=150.0)
    w = dec.decode_batch(feats[:1])[0]
    assert 0 < w.n <= 20
    dec.set_output_level(MM)
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.decode_batch(feats[:1])
    assert "model-level result" in str(e.value)
    dec.close()
    monkeypatch.delenv("JD_RES_CAP")
    for flow in (capi.FLOW_SERIAL, capi.FLOW_RESIDENT):
        def make():
            d = capi.Decoder(gnet, gam, main_beam=150.0, max_streams=4, max_paths=1 << 12)
            d.set_pipeline(flow)
            return d

        def run(d):
            h = d.decode_batch(feats)
            return h, d.last_timing()["relaunches"], d.pipeline_stats()["collections"]
        (a, ra, ca), (b, rb, cb) = _both(make, run)
        _same_words(a, b, "flow %d" % flow)
        assert rb + cb > 0, (flow, rb, cb)                                # (launches repeated behind a collection, or the pipeline's own)


def test_tiny_arena_in_the_slot_pipeline(built):
    from juicer_amd import capi, synth
    am, net, feats, _ = synth.config_small(n_utts=2)
    dec = capi.Decoder(capi.Network.from_synth(net), capi.Models.from_htk(am), main_beam=150.0, max_streams=2, max_paths=64)
    dec.set_pipeline(capi.FLOW_RESIDENT)
    dec.set_output_level(MM)
    with pytest.raises(capi.JuicerAmdError) as e:
        dec.decode_batch(feats)
    assert "Path records" in str(e.value)
    dec.close()
