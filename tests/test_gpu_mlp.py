"""Neural acoustic models on the device: jd_mlp_kernel (csrc/jd_mlp_kernel.h) against the host twin bit for bit - log posteriors and
every layer, over the CPU shapes, shapes that straddle the kernel's tiles, the stated limits and the crafted rows -, the launch
through jd_debug_score_rows, jd_am_score_frames against hybrid models fed the host twin's log posteriors, decoding (batch, streaming
pushes, jd_streams_push) against such a hybrid decoder and the CPU oracle's, the refusals, and jd_batch_test -mlpFName."""
import subprocess

import numpy as np
import pytest

import mlp_cases as mc
from helpers import assert_hyp_matches, bit_exact

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def models_of(layers, seed=0, spm=3):
    from juicer_amd import capi
    return capi.Models.from_mlp(mc.priors(seed, layers[-1][0].shape[0]), spm, layers)


def check_device_equals_host(layers, x, what):
    """the log posteriors and every layer's activations as uint32; a mismatch names the first layer that differs"""
    m = models_of(layers)
    for l in range(len(layers)):
        dev, host = m.mlp_activations(x, l, on_device=True), m.mlp_activations(x, l, on_device=False)
        assert mc.same_floats(dev, host), "%s: layer %d differs first at %s" % (what, l, np.argwhere(bits(dev) != bits(host))[:4].tolist())
    dev, host = m.mlp_forward(x), m.mlp_forward_host(x)
    assert mc.same_floats(dev, host), "%s: log posteriors differ at %s" % (what, np.argwhere(bits(dev) != bits(host))[:4].tolist())


def test_small_shapes_equal_host_twin(built):
    for i, (in_dim, widths, acts) in enumerate(mc.small_shapes()):
        layers = mc.random_net(100 + i, in_dim, widths, acts)
        check_device_equals_host(layers, mc.random_rows(100 + i, 3 + i % 30, in_dim), "small %d" % i)


@pytest.mark.parametrize("shape", mc.tile_shapes(), ids=lambda s: "%d-%s" % (s[0], "-".join(str(w) for w in s[1])))
def test_tile_shapes_equal_host_twin(built, shape):
    in_dim, widths, acts = shape
    layers = mc.random_net(7, in_dim, widths, acts)
    x = mc.random_rows(7, max(mc.TILE_ROWS), in_dim)
    for rows in mc.TILE_ROWS:
        check_device_equals_host(layers, x[:rows], "rows %d" % rows)


@pytest.mark.parametrize("shape", mc.limit_shapes(), ids=lambda s: "%d-%s" % (s[0], "-".join(str(w) for w in s[1][:3])))
def test_limits_equal_host_twin(built, shape):
    in_dim, widths, acts = shape
    layers = mc.random_net(11, in_dim, widths, acts)
    check_device_equals_host(layers, mc.random_rows(11, mc.ROWS + 1, in_dim), "limit")


@pytest.mark.parametrize("case", mc.crafted(), ids=lambda c: c[0])
def test_crafted_rows(built, case):
    """chain order, fusion, an overflowing sigmoid, the logAdd cut, a NaN row: the literals of mlp_cases.crafted from the device"""
    name, layers, x, want, what = case
    m = models_of(layers)
    got = m.mlp_forward(x) if what < 0 else m.mlp_activations(x, what, on_device=True)
    assert mc.same_floats(got, want), (got, want)
    check_device_equals_host(layers, x, name)


def test_operand_maps_with_an_asymmetric_integer_matrix(built):
    """one linear layer, W[j][k] = 100 j + k + 1, unit-vector inputs: the raw logits of input e_k are column k of W exactly - a
    transposed operand map, a permuted k or a misplaced output tile cannot pass"""
    K, N = 37, 41
    w = (100.0 * np.arange(N)[:, None] + np.arange(K)[None, :] + 1.0).astype(np.float32)
    assert not np.array_equal(w[:K, :K], w[:K, :K].T)
    m = models_of([(w, np.zeros(N, np.float32), mc.LINEAR)])
    got = m.mlp_activations(np.eye(K, dtype=np.float32), 0, on_device=True)
    assert np.array_equal(bits(got), bits(w.T))
    b = np.arange(N, dtype=np.float32) * 0.5
    got = models_of([(w, b, mc.LINEAR)]).mlp_activations(np.eye(K, dtype=np.float32), 0, on_device=True)
    assert np.array_equal(bits(got), bits(w.T + b[None, :]))


@pytest.fixture(scope="module")
def table_case(built):
    """a network, frames, the host twin's log posteriors and log priors (computed once)"""
    from juicer_amd import capi
    layers = mc.random_net(21, 19, [40, 23], [mc.SIGMOID])
    pr = mc.priors(21, 23)
    m = capi.Models.from_mlp(pr, 3, layers)
    x = mc.random_rows(21, 50, 19)
    return m, pr, x, m.mlp_forward_host(x), mc.log_priors(pr)


def test_score_rows(table_case):
    """launch_gmm with the decoder's own arguments: rows with row_src = -1 are 0.0f, whole unused tiles included; the guard rows in
    front of and behind the table keep their prefill; max_blocks = 1 changes no bit; the kernel is JD_KERNEL_MLP; a tile list is refused"""
    from juicer_amd import capi
    m, pr, x, logpost, lp = table_case
    rng = np.random.default_rng(3)
    n_rows, guard = 5 * mc.ROWS + 3, 2
    src = rng.integers(0, x.shape[0], n_rows).astype(np.int32)
    src[[0, 7, mc.ROWS - 1, n_rows - 1]] = -1
    src[2 * mc.ROWS:3 * mc.ROWS] = -1                                        # a tile with no used row
    want = np.full((n_rows + 2 * guard, 23), 777.25, np.float32)
    want[guard:guard + n_rows] = np.where(src[:, None] >= 0, logpost[np.maximum(src, 0)] - lp[None, :], np.float32(0.0))
    prefill = np.full_like(want, 777.25)
    got, kernel, grid = capi.debug_score_rows(m, x, src, prefill, guard_rows=guard)
    assert kernel == capi.KERNEL_MLP and grid == 6
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:4].tolist()
    got1, kernel1, grid1 = capi.debug_score_rows(m, x, src, prefill, guard_rows=guard, max_blocks=1)
    assert (kernel1, grid1) == (capi.KERNEL_MLP, 1) and np.array_equal(bits(got1), bits(want))
    got2, _, grid2 = capi.debug_score_rows(m, x, src, prefill, guard_rows=guard, max_blocks=4, skip_unused=1, used_row_tiles=2)
    assert grid2 == 4 and np.array_equal(bits(got2), bits(want))           # (skip_unused / used_row_tiles: ignored, as for hybrid models)
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.debug_score_rows(m, x, src, prefill, guard_rows=guard, rt_base=[0])
    assert e.value.code == capi.JD_EINVAL and "tile lists are not for hybrid models" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.debug_score_rows(m, x, src, prefill, guard_rows=guard, mode=capi.SCORE_FAST)
    assert e.value.code == capi.JD_EINVAL


def test_score_frames_equals_hybrid_on_host_posteriors(table_case):
    from juicer_amd import capi
    m, pr, x, logpost, lp = table_case
    hyb = capi.Models.from_hybrid(pr, 3)
    a, b = m.score_frames(x), hyb.score_frames(logpost)
    assert a.shape == b.shape == (50, 23) and np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(a), bits(logpost - lp[None, :]))


def _stream(gd, x, step=37):
    gd.stream_init(0)
    for pos in range(0, x.shape[0], step):
        gd.stream_push(0, x[pos:pos + step])
    return gd.stream_finish(0)


def _two_streams(gd, xs, step=37):
    for s in (0, 1):
        gd.stream_init(s)
    for pos in range(0, max(x.shape[0] for x in xs), step):
        live = [s for s in (0, 1) if pos < xs[s].shape[0]]
        gd.streams_push(live, [xs[s][pos:pos + step] for s in live])
    return [gd.stream_finish(s) for s in (0, 1)]


@pytest.mark.parametrize("spm", [5, 3])
def test_decoding(built, spm):
    """synth.config_hybrid's log-posterior vectors as input features of mlp_cases.decode_net (noise scale 0.05): the MLP decoder's
    hypotheses equal, labels, times and bit-exact scores, a hybrid decoder's fed the host twin's log posteriors and the CPU oracle's
    hybrid decoder fed the same - decode_batch, streaming pushes of 37 frames, jd_streams_push on two streams at once.
    (tests/test_mlp_cpu.py checks that the oracle certifies these utterances.)"""
    from juicer_amd import capi, synth
    from oracle.oracle import OracleAM, OracleDecoder, OracleNet
    am, net, feats, _ = synth.config_hybrid(seed=3 + spm, states_per_model=spm)
    layers = mc.decode_net(am.priors.shape[0], seed=spm)
    mlp = capi.Models.from_mlp(am.priors, spm, layers)
    hyb = capi.Models.from_hybrid(am.priors, spm)
    oam = OracleAM.from_hybrid(am.priors, spm)
    post = [mlp.mlp_forward_host(x) for x in feats]
    gnet = capi.Network.from_synth(net)
    for kw in mc.DECODE_BEAMS:
        od = OracleDecoder(OracleNet(net), oam, **kw)
        ora = [od.decode_certified(p) for p in post]
        gh = capi.Decoder(gnet, hyb, max_streams=len(feats), **kw)
        want = gh.decode_batch(post)
        gm = capi.Decoder(gnet, mlp, max_streams=len(feats), **kw)
        runs = [("batch", gm.decode_batch(feats)), ("stream", [_stream(gm, feats[0])]), ("streams_push", _two_streams(gm, feats[:2]))]
        for name, got in runs:
            for u, g in enumerate(got):
                what = "spm %d %r %s utt %d" % (spm, kw, name, u)
                assert ora[u].n > 0
                assert_hyp_matches(g, ora[u], what, check_stats=name == "batch")
                assert bit_exact(g, ora[u]), what
                assert_hyp_matches(g, want[u], what, check_stats=False)
                assert bit_exact(g, want[u]), what


def test_refusals_on_mlp_models(table_case, tmp_path):
    from juicer_amd import capi, synth
    m = table_case[0]
    am, net, _, _ = synth.config_hybrid(seed=8, states_per_model=3)
    mlp = capi.Models.from_mlp(am.priors, 3, mc.decode_net(am.priors.shape[0], seed=3))
    gd = capi.Decoder(capi.Network.from_synth(net), mlp, max_streams=2, main_beam=150.0)
    with pytest.raises(capi.JuicerAmdError) as e:
        gd.set_pipeline(capi.FLOW_RESIDENT, 4, 2)
    assert e.value.code == capi.JD_ESTATE and "hybrid" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        gd.set_scoring(capi.SCORE_FAST)
    assert e.value.code == capi.JD_EINVAL and "hybrid" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        m.save_jmbi(str(tmp_path / "m.bin"))
    assert e.value.code == capi.JD_ESTATE and "hybrid" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        m.score_frames(table_case[2], mode=capi.SCORE_FAST)
    assert e.value.code == capi.JD_EINVAL


@pytest.fixture(scope="module")
def cli_case(built, tmp_path_factory):
    """a saved network, the graph, HTK parameter files of width in_dim and the Python decode (made once)"""
    from juicer_amd import build as jbuild, capi, io as jio, synth
    d = tmp_path_factory.mktemp("mlp_cli")
    spm = 3
    am, net, feats, _ = synth.config_hybrid(seed=3 + spm, states_per_model=spm)
    mlp = capi.Models.from_mlp(am.priors, spm, mc.decode_net(am.priors.shape[0], seed=spm))
    mlp.save_mlp(str(d / "m.jmlp"))
    jio.write_fsm(d / "g.fsm", net)
    (d / "out.syms").write_text("<eps> 0\n" + "".join("W%d %d\n" % (i, i) for i in range(1, net.n_words + 1)))
    (d / "mono.txt").write_text("".join("ph%d\n" % h for h in range(am.priors.shape[0])))
    with open(d / "list.txt", "w") as f:
        for u, x in enumerate(feats):
            jio.write_htk(d / ("u%d.htk" % u), x)
            f.write("%s\n" % (d / ("u%d.htk" % u)))
    want = capi.Decoder(capi.Network.from_synth(net), mlp, max_streams=len(feats), main_beam=150.0, max_hyps=100).decode_batch(feats)
    # (-batch: a decoder of as many streams as there are utterances, not of the default 64 - its arenas are the run's time)
    args = [jbuild.BATCH_TEST, "-fsmFName", str(d / "g.fsm"), "-mlpFName", str(d / "m.jmlp"), "-inputFName", str(d / "list.txt"), "-mainBeam", "150",
            "-maxHyps", "100", "-outSymsFName", str(d / "out.syms"), "-outputFormat", "ref", "-batch", str(len(feats))]
    return args, want, d


def test_batch_test_mlp_fname(cli_case):
    """jd_batch_test -mlpFName on a saved network and HTK parameter files: the `ref` lines of the Python decode"""
    args, want, d = cli_case
    out = subprocess.run(args, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(want)
    for u in range(len(want)):
        assert want[u].n > 0 and lines[u].split() == ["W%d" % l for l in want[u].label[::-1]]


def test_batch_test_mlp_phone_names(cli_case):
    """... and with -modelLevelOutput the phones by the names of -monoListFName (a JMLP file holds none); a list of another length
    is refused before anything is decoded"""
    args, want, d = cli_case
    out = subprocess.run(args + ["-modelLevelOutput", "-monoListFName", str(d / "mono.txt")], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(want) and all(l.split() and all(w.startswith("ph") for w in l.split()) for l in lines)
    (d / "short.txt").write_text("a\nb\n")
    out = subprocess.run(args + ["-modelLevelOutput", "-monoListFName", str(d / "short.txt")], capture_output=True, text=True, timeout=240)
    assert out.returncode == 1 and "names 2 phones, the network has 30" in out.stderr
    out = subprocess.run(args + ["-modelLevelOutput"], capture_output=True, text=True, timeout=240)
    assert out.returncode == 1 and "-monoListFName beside -mlpFName" in out.stderr
