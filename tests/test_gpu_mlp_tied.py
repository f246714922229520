"""Tied neural acoustic models on the device: jd_mlp_tied_kernel (csrc/jd_mlp_kernel.h) against the tied host twin bit for bit - every
layer, the raw logits and the log posteriors, over last widths either side of the n-tile pairs, the 8-tile turn, the 128 chains
and the old LDS limit -, the operand map of the wide layer, crafted rows, the launch through jd_debug_score_rows,
jd_am_score_frames against tied hybrid models fed the host twin's posteriors, decoding against such a hybrid decoder and the CPU
oracle's (tying anchored exactly), decoding under HMMs of any topology against the independent Viterbi, the refusals, and
jd_batch_test -mlpTiedFName."""
import subprocess

import numpy as np
import pytest

import indep_cases
import mlp_cases as mc
import mlp_tied_cases as tc
from helpers import assert_hyp_matches, bit_exact

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_device_equals_host(m, n_layers, x, what):
    """every layer's activations (the raw logits for the last) and the log posteriors as uint32; a mismatch names the first layer"""
    for l in range(n_layers):
        dev, host = m.mlp_activations(x, l, on_device=True), m.mlp_activations(x, l, on_device=False)
        assert mc.same_floats(dev, host), "%s: layer %d differs first at %s" % (what, l, np.argwhere(bits(dev) != bits(host))[:4].tolist())
    dev, host = m.mlp_forward(x), m.mlp_forward_host(x)
    assert mc.same_floats(dev, host), "%s: log posteriors differ at %s" % (what, np.argwhere(bits(dev) != bits(host))[:4].tolist())


@pytest.mark.parametrize("P", tc.DEVICE_WIDTHS)
def test_widths_equal_host_twin(built, P):
    x = mc.random_rows(7, max(tc.DEVICE_ROWS), 9)
    for hid in tc.DEVICE_HIDDEN:
        layers = tc.net_for(P, hidden=(hid,), seed=500 + hid, scale=4.0)
        m, _ = tc.tied_models(layers)
        for rows in tc.DEVICE_ROWS:
            check_device_equals_host(m, len(layers), x[:rows], "P %d hidden %d rows %d" % (P, hid, rows))


LIMITS = [(16, [tc.MAX_OUT], []), (mc.MAX_DIM, [mc.MAX_DIM, 1030], [mc.RELU]),
          (6, [9, 8, 7, 9, 8, 7, 9, 8, 7, 9, 8, 7, 9, 8, 7, 150], [mc.SIGMOID, mc.RELU, mc.LINEAR] * 5)]


@pytest.mark.parametrize("shape", LIMITS, ids=lambda s: "%d-%s" % (s[0], "-".join(str(w) for w in s[1][:2])))
def test_limits_equal_host_twin(built, shape):
    """16 -> 16384, 1024 -> 1024 -> 1030 and one network of 16 layers, 17 rows each"""
    in_dim, widths, acts = shape
    layers = mc.random_net(11, in_dim, widths, acts)
    m, _ = tc.tied_models(layers)
    check_device_equals_host(m, len(layers), mc.random_rows(11, 17, in_dim), "limit")


def test_operand_map_of_the_wide_layer(built):
    """one linear layer K = 37, N = 1041, W[j][k] = 100 j + k + 1, unit-vector inputs: the raw logits of input e_k are column k of W
    exactly (every value below 2^24), with and without a bias"""
    K, N = 37, 1041
    w = (100.0 * np.arange(N)[:, None] + np.arange(K)[None, :] + 1.0).astype(np.float32)
    assert float(w.max()) < 2 ** 24 and not np.array_equal(w[:K, :K], w[:K, :K].T)
    m, _ = tc.tied_models([(w, np.zeros(N, np.float32), mc.LINEAR)])
    got = m.mlp_activations(np.eye(K, dtype=np.float32), 0, on_device=True)
    assert np.array_equal(bits(got), bits(w.T))
    b = np.arange(N, dtype=np.float32) * 0.5
    got = tc.tied_models([(w, b, mc.LINEAR)])[0].mlp_activations(np.eye(K, dtype=np.float32), 0, on_device=True)
    assert np.array_equal(bits(got), bits(w.T + b[None, :]))


@pytest.mark.parametrize("case", tc.crafted(), ids=lambda c: c[0])
def test_crafted_rows(built, case):
    """a NaN row, a logit that dominates past the -18.42 cut, all-equal logits: the expectations of mlp_tied_cases.crafted"""
    name, layers, x, want = case
    m, _ = tc.tied_models(layers)
    got = m.mlp_forward(x)
    assert mc.same_floats(got, want), (name, got, want)
    check_device_equals_host(m, len(layers), x, name)


@pytest.fixture(scope="module")
def table_case(built):
    """a network of 1041 outputs, frames, the host twin's log posteriors and the log priors (computed once)"""
    layers = tc.net_for(1041, hidden=(40,), in_dim=19, seed=21)
    m, pr = tc.tied_models(layers, seed=21)
    x = mc.random_rows(21, 50, 19)
    return m, pr, x, m.mlp_forward_host(x), mc.log_priors(pr)


def test_score_rows(table_case):
    """launch_gmm with the decoder's own arguments on a tied model of 1041 outputs: rows with row_src = -1 are 0.0f, a whole unused
    tile included; the guard rows in front of and behind the table keep their prefill bit for bit; max_blocks = 1 changes no bit;
    the kernel is JD_KERNEL_MLP_TIED; tile lists and JD_SCORE_FAST are refused"""
    from juicer_amd import capi
    m, pr, x, logpost, lp = table_case
    rng = np.random.default_rng(3)
    n_rows, guard, G = 5 * mc.ROWS + 3, 2, 1041
    src = rng.integers(0, x.shape[0], n_rows).astype(np.int32)
    src[[0, 7, mc.ROWS - 1, n_rows - 1]] = -1
    src[2 * mc.ROWS:3 * mc.ROWS] = -1                                        # a tile with no used row
    want = np.full((n_rows + 2 * guard, G), 777.25, np.float32)
    want[guard:guard + n_rows] = np.where(src[:, None] >= 0, logpost[np.maximum(src, 0)] - lp[None, :], np.float32(0.0))
    prefill = np.full_like(want, 777.25)
    got, kernel, grid = capi.debug_score_rows(m, x, src, prefill, guard_rows=guard)
    assert kernel == capi.KERNEL_MLP_TIED == 10 and grid == 6
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:4].tolist()
    got1, kernel1, grid1 = capi.debug_score_rows(m, x, src, prefill, guard_rows=guard, max_blocks=1)
    assert (kernel1, grid1) == (capi.KERNEL_MLP_TIED, 1) and np.array_equal(bits(got1), bits(want))
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.debug_score_rows(m, x, src, prefill, guard_rows=guard, rt_base=[0])
    assert e.value.code == capi.JD_EINVAL and "tile lists are not for hybrid models" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.debug_score_rows(m, x, src, prefill, guard_rows=guard, mode=capi.SCORE_FAST)
    assert e.value.code == capi.JD_EINVAL


def test_score_frames_equals_tied_hybrid_on_host_posteriors(table_case):
    from juicer_amd import capi
    m, pr, x, logpost, lp = table_case
    hyb = capi.Models.from_hybrid_tied(capi.Models.from_htk(tc.flat_topology(1041)), pr)
    assert (hyb.vec_size, hyb.n_gmms) == (1041, 1041)
    a, b = m.score_frames(x), hyb.score_frames(logpost)
    assert a.shape == b.shape == (50, 1041) and np.array_equal(bits(a), bits(b))
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
    """mlp_tied_cases.anchor_case: 30 HMMs tied to 22 states.  The tied neural decoder's hypotheses equal - labels, times,
    bit-exact scores, and the batch's statistics against the oracle - a tied hybrid decoder's fed the host twin's log posteriors
    and the CPU oracle's hybrid decoder fed the gathered posteriors x'[:, h] = logpost[:, t(h)] with priors'[h] = priors[t(h)]:
    decode_batch, streaming pushes of 37 frames, jd_streams_push on two streams.  (tests/test_mlp_tied_cpu.py checks that the oracle
    certifies these utterances.)"""
    from juicer_amd import capi
    from oracle.oracle import OracleAM, OracleDecoder, OracleNet
    am, net, feats, pr, layers, tying = tc.anchor_case(spm)
    top = capi.Models.from_htk(am)
    mlp = capi.Models.from_mlp_tied(top, pr, layers)
    hyb = capi.Models.from_hybrid_tied(top, pr)
    post = [mlp.mlp_forward_host(x) for x in feats]
    gnet = capi.Network.from_synth(net)
    for kw in mc.DECODE_BEAMS:
        ora = []
        for p in post:
            xo, po = tc.anchor_oracle_inputs(p, pr, tying)
            ora.append(OracleDecoder(OracleNet(net), OracleAM.from_hybrid(po, spm), **kw).decode_certified(xo))
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


def test_decoding_under_any_topology(built):
    """synth.make_models_mixed's HMMs - 1 to 6 emitting states, a tee model, real state tying - as the topology, every beam off: the
    tied neural decoder equals the tied hybrid decoder bit for bit, and both equal the independent float64 Viterbi over the float32
    score table, under indep_cases.check_against_viterbi's own tolerance; one utterance also through the streaming interface"""
    import indep_viterbi_np as iv
    from juicer_amd import capi
    am, net, xs, pr, layers = tc.mixed_case()
    assert am.max_n == 8 and am.sp_hmm >= 0 and len(set(am.hmm_nstates.tolist())) >= 4
    top = capi.Models.from_htk(am)
    mlp = capi.Models.from_mlp_tied(top, pr, layers)
    hyb = capi.Models.from_hybrid_tied(top, pr)
    post = [mlp.mlp_forward_host(x) for x in xs]
    gnet = capi.Network.from_synth(net)
    gm = capi.Decoder(gnet, mlp, max_streams=len(xs))                         # every beam disabled
    gh = capi.Decoder(gnet, hyb, max_streams=len(xs))
    got, want = gm.decode_batch(xs), gh.decode_batch(post)
    refs = []
    for u, x in enumerate(xs):
        table = mlp.score_frames(x)
        assert np.array_equal(bits(table), bits(post[u] - mc.log_priors(pr)[None, :]))
        ref = iv.viterbi(net, am, table.astype(np.float64))
        assert ref is not None
        refs.append(ref)
        assert_hyp_matches(got[u], want[u], "utt %d" % u, check_stats=False)
        assert bit_exact(got[u], want[u])
        indep_cases.check_against_viterbi(got[u], ref, "tied mlp utt %d" % u)
        indep_cases.check_against_viterbi(want[u], ref, "tied hybrid utt %d" % u)
    s = _stream(gm, xs[0])
    indep_cases.check_against_viterbi(s, refs[0], "streamed")
    assert bit_exact(s, got[0])


def test_refusals_on_tied_models(built, tmp_path):
    from juicer_amd import capi
    am, net, feats, pr, layers, _ = tc.anchor_case(3)
    top = capi.Models.from_htk(am)
    for m in (capi.Models.from_mlp_tied(top, pr, layers), capi.Models.from_hybrid_tied(top, pr)):
        gd = capi.Decoder(capi.Network.from_synth(net), m, max_streams=2, main_beam=150.0)
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
            m.score_frames(np.zeros((1, m.vec_size), np.float32), mode=capi.SCORE_FAST)
        assert e.value.code == capi.JD_EINVAL


@pytest.fixture(scope="module")
def cli_case(built, tmp_path_factory):
    """a saved tied network, an MMF with the topology and the HMMs' names, the graph, HTK parameter files and the Python decode"""
    from juicer_amd import build as jbuild, capi, io as jio
    d = tmp_path_factory.mktemp("mlp_tied_cli")
    spm = 3
    am, net, feats, pr, layers, _ = tc.anchor_case(spm)
    jio.write_mmf(d / "m.mmf", am)
    top = capi.Models.from_mmf_file(str(d / "m.mmf"))
    assert (top.n_hmms, top.n_gmms) == (am.n_hmm, am.n_gmm)
    mlp = capi.Models.from_mlp_tied(top, pr, layers)
    mlp.save_mlp(str(d / "m.jmlp"))
    jio.write_fsm(d / "g.fsm", net)
    (d / "out.syms").write_text("<eps> 0\n" + "".join("W%d %d\n" % (i, i) for i in range(1, net.n_words + 1)))
    with open(d / "list.txt", "w") as f:
        for u, x in enumerate(feats):
            jio.write_htk(d / ("u%d.htk" % u), x)
            f.write("%s\n" % (d / ("u%d.htk" % u)))
    want = capi.Decoder(capi.Network.from_synth(net), mlp, max_streams=len(feats), main_beam=150.0, max_hyps=100).decode_batch(feats)
    args = [jbuild.BATCH_TEST, "-fsmFName", str(d / "g.fsm"), "-htkModelsFName", str(d / "m.mmf"), "-mlpTiedFName", str(d / "m.jmlp"),
            "-inputFName", str(d / "list.txt"), "-mainBeam", "150", "-maxHyps", "100", "-outSymsFName", str(d / "out.syms"), "-outputFormat", "ref",
            "-batch", str(len(feats))]
    return args, want, top.hmm_names(), d


def test_batch_test_mlp_tied_fname(cli_case):
    """jd_batch_test -mlpTiedFName beside an MMF: the `ref` lines of the Python decode; with -modelLevelOutput the phones by the
    MMF's names, no -monoListFName needed; without a models file it is a usage error"""
    args, want, names, d = cli_case
    out = subprocess.run(args, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(want)
    for u in range(len(want)):
        assert want[u].n > 0 and lines[u].split() == ["W%d" % l for l in want[u].label[::-1]]
    out = subprocess.run(args + ["-modelLevelOutput"], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert names and len(lines) == len(want) and all(l.split() and all(w in names for w in l.split()) for l in lines)
    i = args.index("-htkModelsFName")
    out = subprocess.run(args[:i] + args[i + 2:], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "usage: jd_batch_test" in out.stderr
