"""The slot kernel's loads (csrc/jd_slot.h: a pass of phase A and an item of phase X ask for their data in groups of dependent loads - a
new-arc pass: list entry -> {arc, arrival key} -> template -> item; an item: item -> XState -> {bids, row, label} -> instance flags ->
arcs) on the smallest graphs at which those loops can go wrong:
  * stars: the start state fans out into N model arcs, N = 1, 63, 64, 65, 130 - a frame's list of new arcs and its exit items end
    exactly at, one short of and one past a 64-lane chunk, with and without a second chunk; all arcs into ONE state (their exit
    tokens bid for it) or each into its own (REC_SOLE: no bid), labelled and unlabelled arcs side by side;
  * a state with a row of 33 arcs (the second batch of instance flags) and one of 60 (a row walked whole);
  * every instantiation of slot_phase_a: plain left-to-right models, the general path with its tables in LDS (JD_NO_LR), with more
    transition matrices than LDS holds, with more tied states than the likelihood row in LDS holds, and the 144-byte records.
Every case is held against the certified CPU oracle (hypotheses bit for bit, the reference's statistics) and against the cluster
kernel, through the plain launch k_slot_batch (JD_CW=1, JD_SLOT_BATCH=1) first and then through the resident pipeline in commands of
16 frames (a mailbox kernel that waits wrongly hangs: the plain launches tell first).  At most two utterances of 40 frames each."""
import numpy as np
import pytest

from helpers import STAT_KEYS, assert_hyp_matches, bit_exact

pytestmark = pytest.mark.gpu

T_MAX = 40
KW = dict(main_beam=250.0)
STAR_N = (1, 63, 64, 65, 130)


def _lr_models(seed, n_gmm=40, n_hmm=20, n_tm=4, n_mix=2):
    from juicer_amd import synth
    return synth.make_models(seed, n_gmm=n_gmm, n_hmm=n_hmm, n_mix=n_mix, n_tm=n_tm, sep=0.7, with_tee=False, with_skip=False)


def _net(n_states, arcs, finals, n_words):
    """arcs: (src, dst, model 1.., word or 0, weight) in any order; FSM convention (tests/random_topology.py): the arcs of a state
    stand together and the first arc's source is the initial state 0."""
    from juicer_amd import synth
    a = np.asarray([(s, d, m, o) for s, d, m, o, _ in arcs], np.int32)
    w = np.asarray([x[4] for x in arcs], np.float32)
    idx = np.lexsort((np.arange(a.shape[0]), a[:, 0]))
    fin = np.asarray(sorted(finals), np.int32)
    return synth.SynthNet(n_states=n_states, src=a[idx, 0], dst=a[idx, 1], ilab=a[idx, 2], olab=a[idx, 3], w_file=w[idx],
                          fstate=fin, fweight_file=(0.5 + 0.01 * np.arange(fin.size)).astype(np.float32), n_words=n_words)


def _star(n, sole):
    """State 0 fans out into n model arcs - into state 1 (bids) or into states 1 .. n (sole) - every second one labelled; from there
    one arc back to the start (so that the fan is entered again and again) and a loop that keeps a hypothesis alive."""
    am = _lr_models(100 + n)
    rng = np.random.default_rng(1000 + n + (7 if sole else 0))
    arcs = []
    for i in range(n):
        d = 1 + i if sole else 1
        arcs.append((0, d, 1 + i % am.n_hmm, (1 + i) if i % 2 else 0, float(0.05 * i + rng.uniform(0.0, 0.04))))
    for d in range(1, (n if sole else 1) + 1):
        arcs.append((d, 0, 1 + (d + 3) % am.n_hmm, 0, float(rng.uniform(0.1, 1.0))))
        if d <= 2: arcs.append((d, d, 1 + (d + 5) % am.n_hmm, n + d, float(rng.uniform(0.1, 1.0))))
    ns = (n if sole else 1) + 1
    return am, _net(ns, arcs, range(1, ns), n + 3)


def _rows():
    """State 1 has a row of 33 model arcs, state 2 one of 60; both rows lead into states 3 and 4, which lead back."""
    am = _lr_models(300)
    rng = np.random.default_rng(301)
    arcs = [(0, 1, 1, 0, 0.1), (0, 2, 2, 1, 0.2)]
    for s, k in ((1, 33), (2, 60)):
        for i in range(k):
            arcs.append((s, 3 + i % 2, 1 + (i + s) % am.n_hmm, (2 + i) if i % 3 == 0 else 0, float(0.03 * i + rng.uniform(0.0, 0.02))))
    arcs += [(3, 0, 5, 0, 0.3), (4, 1, 6, 70, 0.4), (4, 2, 7, 0, 0.5)]
    return am, _net(5, arcs, (3, 4), 80)


def _walks(net, am, seed):
    import random_topology as rt
    return [rt.random_walk_features(seed + u, net, am, n_arcs=6)[:T_MAX] for u in range(2)]


def _lexicon(am, seed):
    """A small word loop over `am` and two utterances of a few words, cut at T_MAX frames."""
    from juicer_amd import synth
    net = synth.make_wfst(seed + 100, am, n_words=20, n_succ=4, with_sp=am.sp_hmm >= 0)
    return net, [synth.sample_utterance(seed + 200 + u, net, am, 2)[0][:T_MAX] for u in range(2)]


def _build(name):
    """-> am, net, feats, env: the knobs that bring the case to its instantiation of slot_phase_a"""
    from juicer_amd import synth
    kind, _, arg = name.partition("-")
    if kind in ("bids", "sole"):
        am, net = _star(int(arg), kind == "sole")
        return am, net, _walks(net, am, 40 + int(arg)), {}
    if kind == "rows":
        am, net = _rows()
        return am, net, _walks(net, am, 60), {}
    if kind == "small":                                                # (tee model, skips: the general path as the decoder picks it)
        am, net, feats, _ = synth.config_small(n_utts=2)
        return am, net, [x[:T_MAX] for x in feats], {}
    if kind == "mixed":                                                # 144-byte records
        am, net, feats, _ = synth.config_mixed(n_utts=2)
        return am, net, [x[:T_MAX] for x in feats], {}
    # plain left-to-right models: lr | nolr (tables in LDS) | manytm (90 matrices x 25 floats > 2048: tables in HBM), each with the
    # likelihood row in LDS or (bigG: 3100 tied states > 3072) gathered from HBM
    big = arg == "bigG"
    am = _lr_models(500 + len(name), n_gmm=3100 if big else 60, n_hmm=30, n_tm=90 if kind == "manytm" else 6, n_mix=1 if big else 2)
    net, feats = _lexicon(am, 500 + len(name))
    return am, net, feats, ({} if kind == "lr" else {"JD_NO_LR": "1"})


CASES = (["%s-%d" % (k, n) for n in STAR_N for k in ("bids", "sole")] + ["rows"] +
         ["lr", "nolr", "manytm", "lr-bigG", "nolr-bigG", "manytm-bigG", "small", "mixed"])
_cache = {}


def _case(name):
    """The case, its oracle results and the cluster kernel's: made once, shared by both tests, never changed."""
    if name not in _cache:
        from oracle.oracle import OracleAM, OracleDecoder, OracleNet
        am, net, feats, env = _build(name)
        assert len(feats) <= 2 and all(0 < x.shape[0] <= T_MAX for x in feats)
        od = OracleDecoder(OracleNet(net), OracleAM(am), **KW)
        _cache[name] = dict(am=am, net=net, feats=feats, env=env, want=[od.decode_certified(x) for x in feats], cluster=None)
    return _cache[name]


def _key(gs):
    return [(g.n, g.label.tobytes(), g.time.tobytes(), g.score.tobytes(), g.ac.tobytes(), g.lm.tobytes()) + tuple(g.stats[k] for k in STAT_KEYS)
            for g in gs]


def _check(name, how, gs, c):
    for u, g in enumerate(gs):
        what = "%s %s utt %d" % (name, how, u)
        assert_hyp_matches(g, c["want"][u], what)
        assert bit_exact(g, c["want"][u]), what
    assert _key(gs) == c["cluster"], "%s %s: not the cluster kernel's result" % (name, how)


def _env(monkeypatch, c, **more):
    for k in ("JD_CW", "JD_SLOT_BATCH", "JD_NO_LR", "JD_PIPE_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("JD_DEV", "1")
    for k, v in dict(c["env"], **more).items():
        monkeypatch.setenv(k, v)


def _cluster(monkeypatch, name, c):
    from juicer_amd import capi
    if c["cluster"] is None:
        _env(monkeypatch, c)
        gd = capi.Decoder(capi.Network.from_synth(c["net"]), capi.Models.from_htk(c["am"]), max_streams=len(c["feats"]), **KW)
        gs = gd.decode_batch(c["feats"])
        assert gd.last_timing()["slot_launches"] == 0
        gd.close()
        c["cluster"] = _key(gs)
        for u, g in enumerate(gs):
            assert_hyp_matches(g, c["want"][u], "%s cluster utt %d" % (name, u))


@pytest.mark.parametrize("name", CASES)
def test_plain_launch(built, name, monkeypatch):
    from juicer_amd import capi
    c = _case(name)
    _cluster(monkeypatch, name, c)
    _env(monkeypatch, c, JD_CW="1", JD_SLOT_BATCH="1")
    gd = capi.Decoder(capi.Network.from_synth(c["net"]), capi.Models.from_htk(c["am"]), max_streams=len(c["feats"]), **KW)
    gs = gd.decode_batch(c["feats"])
    tm = gd.last_timing()
    assert tm["slot_launches"] == tm["search_launches"] > 0, tm        # (every launch was k_slot_batch)
    gd.close()
    _check(name, "k_slot_batch", gs, c)
    if name.startswith(("bids", "sole", "rows")):                      # (the walks are made to come through: something to compare)
        assert any(o.n > 0 for o in c["want"]), name


@pytest.mark.parametrize("name", CASES)
def test_resident_pipeline(built, name, monkeypatch):
    import torch
    from juicer_amd import capi
    c = _case(name)
    _cluster(monkeypatch, name, c)
    _env(monkeypatch, c, JD_PIPE_CHUNK="16")
    feats = c["feats"]
    offs = np.zeros(len(feats) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([x.shape[0] for x in feats])
    d_feats = torch.from_numpy(np.concatenate(feats)).to(torch.device("cuda", 0))
    gd = capi.Decoder(capi.Network.from_synth(c["net"]), capi.Models.from_htk(c["am"]), max_streams=len(feats), **KW)
    try:
        gd.set_pipeline(capi.FLOW_RESIDENT, 3)
        for step in range(2):                                          # (the second batch finds the slots where the first left them)
            gd.prefetch_scores(d_feats.data_ptr(), offs, 0)
            gs = gd.decode_batch_device(d_feats.data_ptr(), offs, 0)
            assert gd.last_timing()["search_launches"] == 0
            _check(name, "k_slot, batch %d" % step, gs, c)
        torch.cuda.synchronize()
        ps = gd.pipeline_stats()
        assert ps["batches_back"] == 2 and ps["frames_searched"] == 2 * int(offs[-1]), ps
    finally:
        gd.close()
