"""Context splicing on the device: the spliced flavours of jd_mlp_kernel, jd_mlp_tied_kernel and their bf16 kernels against the
PARENT model on caller-spliced input, on the device, with array_equal - the launch through jd_debug_score_rows_span over utterances
that lie back to back, layer 0 through jd_debug_mlp_activations, decoding (a batch, a score-ahead announcement, two chunks, one stream
pushed in small pieces, partial traces) against the parent decoder on spliced vectors, the refusals, and jd_batch_test -mlpSplice."""
import subprocess

import numpy as np
import pytest

import mlp_cases as mc
import mlp_tied_cases as tc
import splice_cases as sc
from helpers import assert_hyp_matches, bit_exact

pytestmark = pytest.mark.gpu

PREFILL = np.float32(777.25)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pair(shape, tied, bf16, seed=13):
    """(parent, spliced) models of a shape"""
    from juicer_amd import capi
    D, left, right, widths = shape
    layers = sc.parent_layers(shape, seed, tied=tied)
    parent = tc.tied_models(layers, seed)[0] if tied else capi.Models.from_mlp(mc.priors(seed, widths[-1]), 3, layers)
    if bf16:
        parent = parent.to_bf16()
    return parent, parent.splice(left, right)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("tied", [False, True], ids=["plain", "tied300"])
@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_rows_equal_parent_on_spliced_input(built, shape, tied, bf16):
    """utterances of 1, 2, 3, 40, 1 and 17 frames back to back through jd_debug_score_rows_span: the identity map and a permuted map
    with -1 holes whose length is no multiple of the tile, on the full grid and with max_blocks = 1 (one workgroup strides over every
    tile), guard rows in front and behind.  Expected: jd_debug_score_rows of the parent on the utterances spliced by numpy, with the same
    maps.  And layer 0 - the gathered input times the first weights - with the frames as one utterance."""
    from juicer_amd import capi
    D, left, right, widths = shape
    parent, spl = pair(shape, tied, bf16)
    n = sum(sc.UTTERANCES)
    f = sc.raw_frames(1, n, D)
    x = sc.splice_utterances(f, sc.UTTERANCES, left, right)
    lo, hi, _ = sc.utterance_spans(sc.UTTERANCES)
    want_kernel = capi.KERNEL_MLP_SPLICED + int(tied) + 2 * int(bf16)
    tile = 32 if bf16 else 16
    guard = 2
    for name, src in sc.row_maps(n, 3):
        n_rows = src.shape[0]
        prefill = np.full((n_rows + 2 * guard, parent.n_gmms), PREFILL, np.float32)
        want, pk, pg = capi.debug_score_rows(parent, x, src, prefill, guard_rows=guard)
        assert pk == want_kernel - 4
        s = np.maximum(src, 0)
        for mb in (0, 1):
            got, k, g = capi.debug_score_rows(spl, f, src, prefill, guard_rows=guard, max_blocks=mb, row_lo=lo[s], row_hi=hi[s])
            assert k == want_kernel and g == (1 if mb else -(-n_rows // tile)), (name, mb, k, g)
            assert np.array_equal(bits(got), bits(want)), (name, mb, np.argwhere(bits(got) != bits(want))[:4].tolist())
        assert np.all(bits(want[:guard]) == bits(PREFILL)) and np.all(bits(want[-guard:]) == bits(PREFILL))
        assert np.all(want[guard:guard + n_rows][src < 0] == 0.0) and np.isfinite(want[guard:guard + n_rows]).all()
    one = sc.splice(f, left, right)                                             # the frames as ONE utterance
    assert np.array_equal(bits(spl.mlp_activations(f, 0, on_device=True)), bits(parent.mlp_activations(one, 0, on_device=True)))
    assert np.array_equal(bits(spl.mlp_forward(f)), bits(parent.mlp_forward(one)))
    assert np.array_equal(bits(spl.score_frames(f)), bits(parent.score_frames(one)))


def test_device_equals_host_twin_f32(built):
    """... and in f32 the device equals the spliced model's own host twin, as its parent's does"""
    parent, spl = pair(sc.SHAPES[3], False, False)
    f = sc.raw_frames(2, 37, sc.SHAPES[3][0])
    assert np.array_equal(bits(spl.mlp_forward(f)), bits(spl.mlp_forward_host(f)))
    assert np.array_equal(bits(spl.mlp_forward(f[:0])), bits(spl.mlp_forward_host(f[:0])))
    assert spl.mlp_time(f, warmup=1, iters=2).shape == (2,)


# ---- decoding: test_gpu_mlp.py::test_decoding's graph; the parent takes windows of (2, 3) frames of the log-posterior vectors, its
# first layer mlp_cases.decode_net's on the centre frame plus seeded noise on every frame of the window
LEFT, RIGHT = 2, 3


def decode_parent_layers(n_phones, seed, noise=0.02):
    w1, b1, a1 = mc.decode_net(n_phones, seed)[0]
    rng = np.random.default_rng(seed + 100)
    C = LEFT + RIGHT + 1
    w = (noise * rng.standard_normal((w1.shape[0], C * n_phones))).astype(np.float32)
    w[:, LEFT * n_phones:(LEFT + 1) * n_phones] += w1
    return [(w, b1, a1), mc.decode_net(n_phones, seed)[1]]


@pytest.fixture(scope="module")
def decode_case(built):
    """the graph, the parent and the spliced models, raw utterances - one of 2 frames, one of more than 128 - and their spliced vectors"""
    from juicer_amd import capi, synth
    spm = 3
    am, net, feats, _ = synth.config_hybrid(seed=3 + spm, states_per_model=spm)
    parent = capi.Models.from_mlp(am.priors, spm, decode_parent_layers(am.priors.shape[0], spm))
    spl = parent.splice(LEFT, RIGHT)
    long = np.ascontiguousarray(np.concatenate(list(feats) + list(feats))[:170])   # the utterances one after the other, twice over
    assert long.shape[0] > 128
    raw = [np.ascontiguousarray(f) for f in feats[:2]] + [np.ascontiguousarray(feats[0][:2]), long]
    return capi.Network.from_synth(net), parent, spl, raw, [sc.splice(f, LEFT, RIGHT) for f in raw]


KW = dict(main_beam=150.0, max_hyps=100)


@pytest.fixture(scope="module")
def decode_want(decode_case):
    from juicer_amd import capi
    gnet, parent, spl, raw, spliced = decode_case
    want = capi.Decoder(gnet, parent, max_streams=len(raw), **KW).decode_batch(spliced)
    assert want[0].n > 0 and want[1].n > 0
    return want


def same(got, want, what):
    for u, g in enumerate(got):
        assert_hyp_matches(g, want[u], "%s utt %d" % (what, u), check_stats=False)
        assert bit_exact(g, want[u]), "%s utt %d" % (what, u)


def test_decode_batch(decode_case, decode_want):
    """a batch; more utterances than streams (waves); FLOW_SERIAL; jd_dec_info reports the frames' size"""
    from juicer_amd import capi
    gnet, parent, spl, raw, spliced = decode_case
    gd = capi.Decoder(gnet, spl, max_streams=len(raw), **KW)
    same(gd.decode_batch(raw), decode_want, "batch")
    assert spl.vec_size == raw[0].shape[1] and parent.vec_size == 6 * raw[0].shape[1]
    g2 = capi.Decoder(gnet, spl, max_streams=2, **KW)
    same(g2.decode_batch(raw), decode_want, "waves")
    g2.set_pipeline(capi.FLOW_SERIAL)
    same(g2.decode_batch(raw), decode_want, "serial")


def test_decode_batch_scored_ahead(decode_case, decode_want):
    """a stream of equal batches, each announced before it is decoded: a table scored ahead (jd_dec_prefetch_scores) carries spans too"""
    import torch
    from juicer_amd import capi
    gnet, parent, spl, raw, spliced = decode_case
    gd = capi.Decoder(gnet, spl, max_streams=len(raw), **KW)
    offs = np.zeros(len(raw) + 1, np.int64)
    offs[1:] = np.cumsum([f.shape[0] for f in raw])
    d_feats = torch.from_numpy(np.concatenate(raw)).to("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    ahead = 0
    for step in range(3):
        gd.prefetch_scores(d_feats.data_ptr(), offs, stream)
        same(gd.decode_batch_device(d_feats.data_ptr(), offs, stream), decode_want, "announced, step %d" % step)
        ahead += gd.last_timing()["prefetched"]
    assert ahead >= 1


def test_decode_batch_two_chunks(decode_case, decode_want, monkeypatch):
    """the chunk knob of docs/DEV_KNOBS.md forces two chunks: a window crosses the chunks' edge"""
    from juicer_amd import capi
    gnet, parent, spl, raw, spliced = decode_case
    monkeypatch.setenv("JD_DEV", "1")
    monkeypatch.setenv("JD_FC", "128")
    gd = capi.Decoder(gnet, spl, max_streams=len(raw), **KW)
    same(gd.decode_batch(raw), decode_want, "two chunks")
    assert gd.last_timing()["gmm_launches"] == 2


PIECES = (1, 3, 7)


def push_in_pieces(gd, x):
    """pieces of 1, 3 and 7 frames in turn - some smaller than RIGHT - then the finish; held frames after every push"""
    gd.stream_init(0)
    assert gd.stream_held_frames(0) == 0
    pos = i = 0
    while pos < x.shape[0]:
        n = PIECES[i % 3]
        gd.stream_push(0, x[pos:pos + n])
        pos = min(pos + n, x.shape[0])
        i += 1
        assert gd.stream_held_frames(0) == min(RIGHT, pos), (pos, gd.stream_held_frames(0))
    h = gd.stream_finish(0)
    assert gd.stream_held_frames(0) == 0
    return h


@pytest.mark.parametrize("interval", [0, 10])
def test_stream_in_pieces(decode_case, decode_want, interval):
    """one stream pushed in pieces of 1, 3 and 7 frames, then finished - also under a partial-trace interval of 10 (the final result)"""
    from juicer_amd import capi
    gnet, parent, spl, raw, spliced = decode_case
    gd = capi.Decoder(gnet, spl, max_streams=1, **KW)
    if interval:
        gd.set_partial_interval(interval)
    for u in (0, 2, 3):
        same([push_in_pieces(gd, raw[u])], [decode_want[u]], "stream interval %d utt %d" % (interval, u))
    # the parent's stream holds nothing back
    gp = capi.Decoder(gnet, parent, max_streams=1, **KW)
    gp.stream_init(0)
    gp.stream_push(0, spliced[0][:5])
    assert gp.stream_held_frames(0) == 0
    gp.stream_finish(0)


def test_refusals_on_a_decoder(decode_case):
    from juicer_amd import capi
    gnet, parent, spl, raw, spliced = decode_case
    gd = capi.Decoder(gnet, spl, max_streams=2, **KW)
    gd.stream_init(0)
    with pytest.raises(capi.JuicerAmdError) as e:
        gd.streams_push([0], [raw[0][:4]])
    assert e.value.code == capi.JD_EINVAL and "spliced" in str(e.value) and "jd_stream_push" in str(e.value)
    gd.stream_finish(0)
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.Broker(gd, 2)
    assert e.value.code == capi.JD_EINVAL and "jd_broker_create" in str(e.value) and "spliced" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        gd.set_pipeline(capi.FLOW_RESIDENT, 4, 2)
    assert e.value.code == capi.JD_ESTATE and "hybrid" in str(e.value)


def test_batch_test_mlp_splice(decode_case, tmp_path):
    """jd_batch_test -mlpSplice 2,3 on raw HTK files = the same run without it on spliced files, byte for byte - in f32, in bf16,
    and through the IDecoder adapter, which takes a frame a call and pushes them through jd_stream_push"""
    from juicer_amd import build as jbuild, io as jio, synth
    gnet, parent, spl, raw, spliced = decode_case
    _, net, _, _ = synth.config_hybrid(seed=6, states_per_model=3)
    d = tmp_path
    parent.save_mlp(str(d / "m.jmlp"))
    jio.write_fsm(d / "g.fsm", net)
    (d / "out.syms").write_text("<eps> 0\n" + "".join("W%d %d\n" % (i, i) for i in range(1, net.n_words + 1)))
    for kind, xs in (("raw", raw), ("spl", spliced)):
        with open(d / ("%s.txt" % kind), "w") as f:
            for u, x in enumerate(xs):
                jio.write_htk(d / ("%s%d.htk" % (kind, u)), x)
                f.write("%s\n" % (d / ("%s%d.htk" % (kind, u))))

    def run(kind, extra):
        args = [jbuild.BATCH_TEST, "-fsmFName", str(d / "g.fsm"), "-mlpFName", str(d / "m.jmlp"), "-inputFName", str(d / ("%s.txt" % kind)), "-mainBeam", "150",
                "-maxHyps", "100", "-outSymsFName", str(d / "out.syms"), "-outputFormat", "ref", "-batch", str(len(raw))] + extra
        out = subprocess.run(args, capture_output=True, timeout=240)
        assert out.returncode == 0, out.stderr
        return out.stdout

    for extra in ([], ["-mlpBf16"], ["-perFrameAdapter"]):
        a, b = run("raw", ["-mlpSplice", "2,3"] + extra), run("spl", extra)
        assert a == b and len(a.splitlines()) == len(raw) and any(l.split() for l in a.splitlines()), extra
    out = subprocess.run([jbuild.BATCH_TEST, "-mlpSplice", "2,3"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "-mlpSplice needs a network file" in out.stderr and "RAW vectors of in_dim / (L + R + 1) values" in out.stderr
