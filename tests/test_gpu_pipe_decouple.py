"""The resident slot pipeline with the side stream off its critical path (jd_host_resident.h: pump_harvest / pump_refill / pump_score,
jd_slot.h: k_slot's own export): a slot exports the utterance it has finished, an utterance of a table the host knows to be scored
is posted without a new ready number, and up to two scoring pieces are enqueued.  Few slots and several announced batches, so that
every slot hands over many times; every hypothesis - labels, times, scores bit for bit, totals, the reference's statistics - is what
the SAME decoder returns under FLOW_SERIAL, and a batch that fails there fails here with the same code.  The whole file runs a second
time under JD_PIPE_DECOUPLE=0 (kernel exports, a ready number with every utterance, one piece in flight): the fallback paths.
"""
import numpy as np
import pytest

from helpers import STAT_KEYS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small(built):
    from juicer_amd import capi, synth
    am, net, feats, _ = synth.config_small()
    return capi.Network.from_synth(net), capi.Models.from_htk(am), feats


@pytest.fixture(scope="module")
def toy(built):
    from juicer_amd import capi, synth
    am, net, feats, _ = synth.config_toy()
    return capi.Network.from_synth(net), capi.Models.from_htk(am), feats


@pytest.fixture(params=["1", "0"], ids=["decoupled", "JD_PIPE_DECOUPLE=0"])
def knobs(request, monkeypatch):
    monkeypatch.setenv("JD_DEV", "1")
    monkeypatch.setenv("JD_PIPE_DECOUPLE", request.param)
    return monkeypatch


def make_batches(feats, sizes=(7, 5, 9, 6), seed=3):
    """utterances of 1 .. 110 frames cut from the fixture's: a 1-frame one and a 3-frame one (no token reaches a final state: n = -1) in
    the first batches, the others long enough to have words"""
    rng = np.random.RandomState(seed)
    out = []
    for b, n in enumerate(sizes):
        utts = []
        for u in range(n):
            x = feats[(b + u) % len(feats)]
            ln = int(rng.randint(30, 111))
            o = int(rng.randint(0, x.shape[0] - ln))
            utts.append(np.ascontiguousarray(x[o:o + ln]))
        if b == 0:
            utts[2] = np.ascontiguousarray(feats[0][:1])
        if b == 1:
            utts[0] = np.ascontiguousarray(feats[1][:3])
        out.append(utts)
    return out


def on_device(batch):
    import torch
    offs = np.zeros(len(batch) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([x.shape[0] for x in batch])
    return torch.from_numpy(np.concatenate(batch)).to(torch.device("cuda", 0)), offs


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def assert_same(g, w, what):
    assert g.n == w.n, "%s: n %d, serial %d" % (what, g.n, w.n)
    if w.n > 0:
        assert np.array_equal(g.label, w.label) and np.array_equal(g.time, w.time), what
        for f in ("score", "ac", "lm"):
            assert np.array_equal(bits(getattr(g, f)), bits(getattr(w, f))), "%s: %s" % (what, f)
        for f in ("tot_score", "tot_ac", "tot_lm"):
            assert bits(getattr(g, f)) == bits(getattr(w, f)), "%s: %s" % (what, f)
    for k in STAT_KEYS:                                                # (the frame count, the reference's five, instances taken in)
        assert g.stats[k] == w.stats[k], "%s: stat %s %d, serial %d" % (what, k, g.stats[k], w.stats[k])
    gm, wm = getattr(g, "models", None), getattr(w, "models", None)
    assert (gm is None) == (wm is None), what
    if wm is not None:
        assert gm.n == wm.n, what
        if wm.n > 0:
            for f in ("model", "label", "time"):
                assert np.array_equal(getattr(gm, f), getattr(wm, f)), "%s: models.%s" % (what, f)
            for f in ("score", "ac", "lm"):
                assert np.array_equal(bits(getattr(gm, f)), bits(getattr(wm, f))), "%s: models.%s" % (what, f)


def decode_or_code(gd, buf):
    """the batch's hypotheses, or the code of the error its decode raises"""
    from juicer_amd import capi
    try:
        return gd.decode_batch_device(buf[0].data_ptr(), buf[1], 0)
    except capi.JuicerAmdError as e:
        return e.code


def serial_then_resident(gd, batches, order, slots, depth=4, quiesce_at=(), want=None):
    """every batch of `order` under FLOW_SERIAL (or `want`: what is expected of each batch), then the same list announced depth - 1
    ahead through `slots` resident slots; returns (the serial results by batch, the pipeline's statistics)"""
    import torch
    from juicer_amd import capi
    bufs = [on_device(b) for b in batches]
    gd.set_pipeline(capi.FLOW_SERIAL)
    if want is None:
        want = [decode_or_code(gd, bufs[k]) for k in range(len(batches))]
    gd.set_pipeline(capi.FLOW_RESIDENT, depth, slots)
    ahead = depth - 1
    for k in order[:ahead]:
        gd.prefetch_scores(bufs[k][0].data_ptr(), bufs[k][1], 0)
    for i, k in enumerate(order):
        if i + ahead < len(order):
            nk = order[i + ahead]
            gd.prefetch_scores(bufs[nk][0].data_ptr(), bufs[nk][1], 0)
        if i in quiesce_at:                                            # (right behind an announcement: its pieces are on the side stream)
            gd.quiesce()
            torch.cuda.synchronize()
        got = decode_or_code(gd, bufs[k])
        if isinstance(want[k], int):
            assert got == want[k], "step %d batch %d: %r, serial raised %d" % (i, k, got, want[k])
            continue
        assert not isinstance(got, int), "step %d batch %d raised %d" % (i, k, got)
        assert gd.last_timing()["search_launches"] == 0                # (handed back by the pipeline)
        for u, (g, w) in enumerate(zip(got, want[k])):
            assert_same(g, w, "step %d batch %d utt %d" % (i, k, u))
    torch.cuda.synchronize()
    ps = gd.pipeline_stats()
    gd.set_pipeline(capi.FLOW_SERIAL)
    return want, ps


ORDER = [0, 1, 2, 3, 1, 0]


@pytest.mark.parametrize("slots", [2, 4])
def test_hand_overs(small, knobs, slots):
    """the plain case: a 1-frame utterance, utterances without a surviving token, every slot taking many utterances"""
    from juicer_amd import capi
    gnet, gam, feats = small
    batches = make_batches(feats)
    gd = capi.Decoder(gnet, gam, max_streams=9, main_beam=150.0)
    want, ps = serial_then_resident(gd, batches, ORDER, slots)
    assert want[0][2].n == -1 and want[1][0].n == -1                   # (the 1-frame and the 3-frame utterance)
    assert sum(1 for k in range(4) for h in want[k] if h.n > 0) >= 20
    assert ps["utts_through"] == sum(len(batches[k]) for k in ORDER) and ps["slots"] == slots
    gd.close()


def test_hand_overs_toy(toy, knobs):
    gnet, gam, feats = toy
    from juicer_amd import capi
    x = feats[0]
    batches = [[np.ascontiguousarray(x[o:o + n]) for o, n in ((0, 40), (5, 1), (10, 60), (0, x.shape[0]), (20, 33))],
               [np.ascontiguousarray(x[o:o + n]) for o, n in ((3, 50), (0, 2), (7, 45), (30, 64), (1, 70), (2, 31))],
               [np.ascontiguousarray(x[o:o + n]) for o, n in ((0, 25), (9, 80), (4, 4), (0, 55), (6, 47))]]
    gd = capi.Decoder(gnet, gam, max_streams=6)
    serial_then_resident(gd, batches, [0, 1, 2, 0, 2, 1], 3, depth=3)
    gd.close()


def test_model_level_output(small, knobs):
    from juicer_amd import capi
    gnet, gam, feats = small
    gd = capi.Decoder(gnet, gam, max_streams=9, main_beam=150.0)
    gd.set_output_level(capi.OUTPUT_WORDS | capi.OUTPUT_MODELS)
    want, _ = serial_then_resident(gd, make_batches(feats, seed=5), ORDER, 3)
    assert any(h.models.n > h.n > 0 for h in want[2])
    gd.close()


def test_chain_longer_than_the_result_capacity(small, knobs):
    """JD_RES_CAP=16 and model-level output: the chain of a whole utterance of the fixture is longer than a result slot - the export
    stops writing at the capacity and reports the length, the decode raises as FLOW_SERIAL's does; a batch of utterances too
    short for that comes back whole"""
    from juicer_amd import capi
    gnet, gam, feats = small
    knobs.setenv("JD_RES_CAP", "16")
    gd = capi.Decoder(gnet, gam, max_streams=9, main_beam=150.0)
    gd.set_output_level(capi.OUTPUT_WORDS | capi.OUTPUT_MODELS)
    batches = make_batches(feats, seed=7)
    batches[0][1], batches[2][4] = feats[0], feats[1]                  # (whole utterances: a dozen words, several models each)
    batches[3] = [np.ascontiguousarray(feats[u % 4][:n]) for u, n in enumerate((1, 3, 2, 6, 4, 1))]
    want, _ = serial_then_resident(gd, batches, ORDER, 3)
    assert want[0] == capi.JD_ENOMEM and want[2] == capi.JD_ENOMEM and not isinstance(want[3], int)
    gd.close()


def test_short_commands_and_collections(small, knobs):
    """JD_PIPE_CHUNK=16 and a Path arena so small that the slots stop for collections all the time - on an utterance's last command
    too: the command posted behind the collection still ends the utterance, and still names its result slot"""
    from juicer_amd import capi
    gnet, gam, feats = small
    knobs.setenv("JD_PIPE_CHUNK", "16")
    gd = capi.Decoder(gnet, gam, max_streams=9, main_beam=150.0, max_paths=1 << 12)
    _, ps = serial_then_resident(gd, make_batches(feats, seed=11), ORDER, 3)
    assert ps["collections"] >= 20, ps
    gd.close()


def test_arena_error_on_one_stream(small, knobs):
    """An instance arena of 1024 records - eight wave segments of 128 in a slot - and a beam of 90: a frame of the fixture's speech
    keeps 540 instances at the most (the CPU oracle's count, frame by frame), an utterance of sixty identical frames at the features'
    mean 1050 on average and 1470 at its widest, more than the arena holds however they fall on the waves.  Its slot reports the
    error and is out of the game, its result goes out by the kernel, its batch's decode raises JD_ENOMEM - and every other utterance
    is right.  (The arena does not change a result, only whether there is one: what is right comes from FLOW_SERIAL on a decoder of the
    same beam with the default arenas - the launch-per-call kernel splits an arena over the waves of a cluster, and overflows elsewhere.)"""
    from juicer_amd import capi
    gnet, gam, feats = small
    flat = np.tile(np.concatenate(feats).mean(0), (60, 1)).astype(np.float32)
    batches = make_batches(feats, seed=13)
    batches[1][3] = flat
    roomy = capi.Decoder(gnet, gam, max_streams=9, main_beam=90.0)
    roomy.set_pipeline(capi.FLOW_SERIAL)
    want = [decode_or_code(roomy, on_device(b)) for b in batches]
    roomy.close()
    assert not any(isinstance(w, int) for w in want)
    want[1] = capi.JD_ENOMEM
    gd = capi.Decoder(gnet, gam, max_streams=9, main_beam=90.0, max_slots=1024)
    serial_then_resident(gd, batches, [0, 1, 2, 3, 0], 4, want=want)
    gd.close()


def test_many_pieces_and_quiesce(small, knobs):
    """JD_PIPE_PIECE=128: a batch is several pieces, two of them enqueued at a time, and a slot is often free before the table of the
    next batch is scored (no event yet: a ready number behind the pieces); jd_dec_quiesce right behind an announcement, with its
    pieces on the side stream - the kernel comes back and nothing is lost"""
    from juicer_amd import capi
    gnet, gam, feats = small
    knobs.setenv("JD_PIPE_PIECE", "128")
    gd = capi.Decoder(gnet, gam, max_streams=9, main_beam=150.0)
    _, ps = serial_then_resident(gd, make_batches(feats, seed=17), ORDER, 3, quiesce_at=(0, 2, 3))
    assert ps["batches_back"] == len(ORDER) and ps["resident"] == 0
    gd.close()
