"""jd_dec_set_scoring(JD_SCORE_FAST) for GMM models of ANY vector size (csrc/jd_gmm.h: jd_gmm_fast - jd_gmm_fast39's arithmetic with D at run
time: parameters padded to chunks of 8 dimensions, the feature tile in slabs of 64 dimensions).  Held to what the D = 39 option is held to
(tests/test_gpu_fastscore.py): the table within 1e-4 relative of the exact kernel's, which equals the CPU oracle's bit for bit; 1-best words
and times identical to the oracle's and scores within 1e-4 - through the launch path, the resident slot pipeline and the streaming calls.

The dimensions: both sides of a padding step (16 | 17, 64 | 65), a multiple of the chunk (40), the smallest (1, 2), both sides of the step
from one slab to two (64 | 65), three slabs (129); the tables of TABLE_BIG are large enough for the tiles of 64 tied states (launch_gmm takes
the tiles of 16 below 1024 tiles)."""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import bit_exact, oracle_certified_many
from test_gpu_fastscore import BEAMS, RTOL, _same_words_close_scores

pytestmark = pytest.mark.gpu

DIMS = [1, 2, 13, 16, 17, 40, 64, 65, 100, 129]
# The largest deviation of the fast table from the exact one, relative to max(1, |exact|), MEASURED on an MI355X: per D the worst of the
# three max_mix of test_fast_table_any_dimension (every one of the 30 cases lay in 2.2e-7 .. 4.5e-7), and the two tables of
# test_fast_table_tiles_of_64_states.  The regression bound a test asserts is FOUR TIMES the measured value (1.0e-6 .. 1.8e-6; the headroom
# is for other seeds), never above RTOL: a kernel that lands "just inside 1e-4" is a bug.
TABLE_MEASURED = {1: 4.427e-07, 2: 3.219e-07, 13: 2.844e-07, 16: 2.425e-07, 17: 2.576e-07, 40: 2.481e-07, 64: 2.513e-07, 65: 2.901e-07,
                  100: 2.375e-07, 129: 2.741e-07}
TABLE_BOUND = {D: min(RTOL, 4.0 * m) for D, m in TABLE_MEASURED.items()}
TABLE_BIG = [17, 65]                                      # (both through the tiles of 64 states: one slab, two slabs)
TABLE_BIG_MEASURED = {17: 3.764e-07, 65: 3.306e-07}
TABLE_BIG_BOUND = {D: min(RTOL, 4.0 * m) for D, m in TABLE_BIG_MEASURED.items()}


def _ragged_models(seed, D, n_gmm, max_mix):
    from juicer_amd import synth
    am = synth.make_models(seed, n_gmm=n_gmm, n_hmm=max(4, n_gmm // 3), n_mix=max_mix, D=D, n_tm=4)
    rng = np.random.default_rng(seed + 77)
    am.n_mix = rng.integers(1, max_mix + 1, size=n_gmm).astype(np.int32)
    am.n_mix[0] = max_mix                                 # (both ends of the range are there)
    am.n_mix[1] = 1
    # the weights of a state's first n_mix mixtures sum to 1 (a single mixture's is exactly 1: the model loader insists)
    w = am.weight.astype(np.float64) * (np.arange(max_mix)[None, :] < am.n_mix[:, None])
    am.weight = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    am.weight[am.n_mix == 1, 0] = 1.0
    return am


def _frames(seed, am, n):
    """frames near the models (a component's mean plus noise of its own variance), so that the likelihoods are those of a decode"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, am.n_gmm, size=n)
    return (am.mean[g, 0] + rng.normal(0.0, 1.0, size=(n, am.D)) * np.sqrt(am.var[g, 0])).astype(np.float32)


def _rel(fast, exact):
    return float((np.abs(fast.astype(np.float64) - exact) / np.maximum(1.0, np.abs(exact))).max())


def _check_table(am, x, bound, what):
    from juicer_amd import capi
    from oracle.oracle import OracleAM
    gam = capi.Models.from_htk(am)
    exact = gam.score_frames(x)
    assert np.array_equal(exact.view(np.uint32), OracleAM(am).score_frames(x).view(np.uint32)), what     # the yardstick
    fast = gam.score_frames(x, mode=capi.SCORE_FAST)
    rel = _rel(fast, exact)
    print("fast table %s: max relative deviation %.3e (bound %.1e)" % (what, rel, bound))
    assert np.all(np.isfinite(fast)), what
    assert rel <= RTOL, (what, rel)
    assert rel <= bound <= RTOL, (what, rel)
    assert not np.array_equal(fast.view(np.uint32), exact.view(np.uint32)), what                         # (it IS the other kernel)


@pytest.mark.parametrize("max_mix", [1, 3, 16])
@pytest.mark.parametrize("D", DIMS)
def test_fast_table_any_dimension(built, D, max_mix):
    """300 rows (two row tiles of 128 and 44 rows of a third), 50 tied states (three state tiles of 16 and 2 of a fourth), 1..max_mix
    mixtures"""
    am = _ragged_models(100 + D, D, 50, max_mix)
    _check_table(am, _frames(5 + D, am, 300), TABLE_BOUND[D], "D %d max_mix %d" % (D, max_mix))


@pytest.mark.parametrize("D", TABLE_BIG)
def test_fast_table_tiles_of_64_states(built, D):
    """129 row tiles (the last of 6 rows) x 8 state tiles of 64 (the last of 22): 1032 tiles, the size from which launch_gmm takes them"""
    am = _ragged_models(300 + D, D, 470, 3)
    _check_table(am, _frames(9 + D, am, 128 * 128 + 6), TABLE_BIG_BOUND[D], "D %d, tiles of 64" % D)


@pytest.mark.parametrize("D,D2", [(13, 16), (17, 24), (60, 70), (64, 65)])
def test_padding_is_inert(built, D, D2):
    """the table of a model equals, bit for bit, the table of the same model embedded in D2 dimensions: extra feature columns of any value,
    mean 0 and inverse variance 0 there (the prepared s = sqrt(ivar) = 0, t = -mean s = 0: what the kernel's own padding holds) - within a
    chunk (13 in 16), into the next chunk (17 in 24) and across the step from one slab to two (60 in 70, 64 in 65)"""
    from juicer_amd import capi
    am = _ragged_models(500 + D, D, 37, 5)
    x = _frames(3, am, 200)
    gam = capi.Models.from_htk(am)
    det, mean, ivar = gam.flat()
    mean2 = np.zeros(mean.shape[:2] + (D2,), np.float32)
    ivar2 = np.zeros_like(mean2)
    mean2[..., :D], ivar2[..., :D] = mean, ivar
    rng = np.random.default_rng(8)
    x2 = np.concatenate([x, rng.normal(0.0, 30.0, size=(x.shape[0], D2 - D)).astype(np.float32)], axis=1)
    gam2 = capi.Models.from_flat(det, mean2, ivar2, am.n_mix)
    a, b = gam.score_frames(x, mode=capi.SCORE_FAST), gam2.score_frames(x2, mode=capi.SCORE_FAST)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # (and the model as the flat arrays give it is the model: the embedding is what is compared, not the two constructors)
    c = capi.Models.from_flat(det, mean, ivar, am.n_mix).score_frames(x, mode=capi.SCORE_FAST)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- decodes

def _cfg(D, n_utts=4):
    """config_small's shape (the tee model between words) at a few thousand arcs, D-dimensional.  The seeds are chosen so that the oracle
    alone certifies every utterance under every beam set of BEAMS (decode_certified raises otherwise): tests/test_fastscore_anyd_fixtures.py
    checks that without a GPU."""
    from juicer_amd import synth
    seed = {13: 21, 80: 22}[D]
    am = synth.make_models(seed, n_gmm=60, n_hmm=25, n_mix=3, D=D, n_tm=8, sep=0.6, with_tee=True)
    net = synth.make_wfst(seed + 100, am, n_words=80, n_succ=8, with_sp=True, eps_word_frac=0.02)
    rng = np.random.default_rng(seed + 300)
    feats = [synth.sample_utterance(seed + 1000 + u, net, am, int(rng.integers(5, 11)))[0] for u in range(n_utts)]
    return am, net, feats


_WANT = {}


def _want(D, bi):
    """the oracle's results, once per (D, beam set)"""
    if (D, bi) not in _WANT:
        am, net, feats = _cfg(D)
        want = oracle_certified_many(net, am, feats, **BEAMS[bi])
        assert len(want) == len(feats) and all(o is not None for o in want)       # none was dropped
        _WANT[(D, bi)] = want
    return _WANT[(D, bi)]


@pytest.mark.parametrize("D", [13, 80])
@pytest.mark.parametrize("bi", range(len(BEAMS)))
def test_fast_scoring_keeps_words_and_times_any_dimension(built, D, bi):
    from juicer_amd import capi
    am, net, feats = _cfg(D)
    assert 2000 <= net.n_arcs <= 20000, net.n_arcs
    kw = BEAMS[bi]
    want = _want(D, bi)
    big = (1 << 25) if kw.get("main_beam", 0.0) in (0.0, 200.0) and not kw.get("max_hyps") else 0
    gd = capi.Decoder(capi.Network.from_synth(net), capi.Models.from_htk(am), max_streams=len(feats), max_paths=big, **kw)
    gd.set_scoring(capi.SCORE_FAST)
    gs = gd.decode_batch(feats)
    for u, o in enumerate(want):
        _same_words_close_scores(gs[u], o, "D %d utt %d %s" % (D, u, kw))
    gd.set_scoring(capi.SCORE_EXACT)                      # ... and back: the default is the bit-identical one
    gs = gd.decode_batch(feats)
    for u, o in enumerate(want):
        assert bit_exact(gs[u], o), (D, u, kw)
    gd.close()


def test_fast_scoring_any_dimension_through_the_resident_pipeline(built):
    """announced batches through the slots of the resident kernel, their tables scored by jd_gmm_fast beside the search (two slabs)"""
    import torch
    from juicer_amd import capi
    am, net, feats = _cfg(80)
    bi = 2
    kw = BEAMS[bi]
    want = _want(80, bi)
    dev = torch.device("cuda", 0)
    gd = capi.Decoder(capi.Network.from_synth(net), capi.Models.from_htk(am), max_streams=8, **kw)
    gd.set_scoring(capi.SCORE_FAST)
    gd.set_pipeline(capi.FLOW_RESIDENT, 4, 8)
    offs = np.zeros(len(feats) + 1, np.int64)
    offs[1:] = np.cumsum([f.shape[0] for f in feats])
    d_feats = torch.from_numpy(np.concatenate(feats)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        gd.prefetch_scores(d_feats.data_ptr(), offs, stream)
    for step in range(5):
        if step < 2:
            gd.prefetch_scores(d_feats.data_ptr(), offs, stream)
        gs = gd.decode_batch_device(d_feats.data_ptr(), offs, stream)
        for u, o in enumerate(want):
            _same_words_close_scores(gs[u], o, "pipeline step %d utt %d" % (step, u))
    assert gd.pipeline_stats()["utts_through"] >= 5 * len(feats)
    gd.close()


@pytest.mark.parametrize("D", [13, 80])
def test_fast_scoring_any_dimension_streaming(built, D):
    """jd_stream_push in uneven chunks and jd_streams_push over two streams at different frames: the batch decode's kernel and cells, so
    its words, times AND scores bit for bit"""
    from juicer_amd import capi
    am, net, feats = _cfg(D)
    kw = BEAMS[2]
    gd = capi.Decoder(capi.Network.from_synth(net), capi.Models.from_htk(am), max_streams=len(feats), **kw)
    gd.set_scoring(capi.SCORE_FAST)
    want = gd.decode_batch(feats)
    assert all(o.n > 0 for o in want)
    x = feats[0]
    assert x.shape[0] > 1 + 7 + 64
    gd.stream_init(0)
    pos = 0
    for n in (1, 7, 64, x.shape[0]):
        gd.stream_push(0, x[pos:pos + n])
        pos += n
    assert bit_exact(gd.stream_finish(0), want[0])
    gd.stream_init(1)
    gd.stream_init(2)
    gd.stream_push(1, feats[1][:33])                       # stream 1 is 33 frames ahead
    p1, p2 = 33, 0
    while p1 < feats[1].shape[0] or p2 < feats[2].shape[0]:
        ss, fr = [], []
        if p1 < feats[1].shape[0]:
            ss.append(1); fr.append(feats[1][p1:p1 + 50]); p1 += 50
        if p2 < feats[2].shape[0]:
            ss.append(2); fr.append(feats[2][p2:p2 + 130]); p2 += 130
        gd.streams_push(ss, fr)
    assert bit_exact(gd.stream_finish(1), want[1]) and bit_exact(gd.stream_finish(2), want[2])
    gd.close()


def test_fast39_table_is_the_parent_commits(built):
    """D = 39 still goes to jd_gmm_fast39: the fast table of config_small's models, bit for bit the one recorded from the commit before
    jd_gmm_fast came (tests/golden/fast39_table.json: shape and SHA-256 of the float32 table)"""
    from juicer_amd import capi, synth
    am, _, feats, _ = synth.config_small()
    x = np.concatenate(feats)[:300]
    fast = capi.Models.from_htk(am).score_frames(x, mode=capi.SCORE_FAST)
    with open(os.path.join(os.path.dirname(__file__), "golden", "fast39_table.json")) as f:
        gold = json.load(f)
    assert list(fast.shape) == gold["shape"]
    assert hashlib.sha256(np.ascontiguousarray(fast).tobytes()).hexdigest() == gold["sha256"]
