"""bf16 neural acoustic models on the device: jd_mlp_bf16_kernel / jd_mlp_tied_bf16_kernel (csrc/jd_mlp_bf16_kernel.h) against the
contract of csrc/jd_mlp_bf16.h - exact integer networks (whatever the summation order, the logits are the integer product), the
derived bound of the linear part on realistic data, the log posteriors bit for bit from the device's own logits, row independence
bit for bit, the launch through jd_debug_score_rows, crafted rows, decoding (batch, streaming pushes, jd_streams_push) against a
hybrid decoder and the CPU oracle fed the device's own log posteriors, jd_batch_test -mlpBf16, the refusals."""
import subprocess

import numpy as np
import pytest

import mlp_bf16_cases as bc
import mlp_cases as mc
import mlp_tied_cases as tc
from helpers import assert_hyp_matches, bit_exact

pytestmark = pytest.mark.gpu
R, KG, NT = bc.ROWS, bc.KG, bc.NT


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_TOP = {}


def models_of(layers, tied, seed=0):
    """the bf16 model of a network (phone models of 3 states, or tied ones over mlp_tied_cases.flat_topology), and the priors"""
    from juicer_amd import capi
    P = layers[-1][0].shape[0]
    pr = mc.priors(seed, P)
    if tied:
        if P not in _TOP:
            _TOP[P] = capi.Models.from_htk(tc.flat_topology(P))
        m = capi.Models.from_mlp_tied(_TOP[P], pr, layers)
    else:
        m = capi.Models.from_mlp(pr, 3, layers)
    q = m.to_bf16()
    assert q.mlp_precision == capi.MLP_BF16
    return q, pr


def check_exact(layers, x, want, tied, what):
    """the raw logits of the rows {1, R - 1, R, R + 1, 4 R + 1} of x equal want bit for bit"""
    q, _ = models_of(layers, tied)
    last = len(layers) - 1
    for n in bc.TILE_ROWS:
        got = q.mlp_activations(x[:n], last, on_device=True)
        assert np.array_equal(bits(got), bits(want[:n])), "%s rows %d: first at %s" % (what, n, np.argwhere(bits(got) != bits(want[:n]))[:4].tolist())


@pytest.mark.parametrize("tied", [False, True], ids=["phone", "tied"])
def test_exact_integer_layers(built, tied):
    """single linear layers, weights and inputs integers in [-8, 8], integer biases: every partial sum is below 2^24, so a dropped,
    doubled or permuted k, a transposed operand map or a misplaced tile cannot pass"""
    shapes = [(K, N) for K in bc.INT_KS for N in bc.INT_NS] + [(1024, 1024)] + ([(1024, 16384), (33, 1041)] if tied else [])
    for i, (K, N) in enumerate(shapes):
        w, b = bc.int_layer(i, N, K)
        x = bc.int_rows(i, max(bc.TILE_ROWS), K)
        check_exact([(w, b, mc.LINEAR)], x, bc.int_logits(w, b, x), tied, "K %d N %d" % (K, N))


@pytest.mark.parametrize("tied", [False, True], ids=["phone", "tied"])
def test_operand_maps_with_an_asymmetric_integer_matrix(built, tied):
    """W[j][k] = ((7 j + 3 k) mod 251) - 125, unit-vector inputs: the logits of input e_k are column k of W exactly"""
    for K, N in ((2 * KG + 1, 8 * NT + 1), (4 * R + 1, NT + 1)):
        w, b = bc.asym_layer(N, K)
        assert not np.array_equal(w[:NT, :NT], w[:NT, :NT].T)
        x = np.zeros((max(bc.TILE_ROWS), K), np.float32)
        x[np.arange(x.shape[0]), np.arange(x.shape[0]) % K] = 1.0
        check_exact([(w, b, mc.LINEAR)], x, np.ascontiguousarray(w.T[np.arange(x.shape[0]) % K]), tied, "asym K %d N %d" % (K, N))


@pytest.mark.parametrize("tied", [False, True], ids=["phone", "tied"])
def test_exact_two_layer_relu(built, tied):
    """first-layer weights in {-1, 0, 1}: the hidden values are integers within +-256, bf16-exact, so the second layer is exact too"""
    for i, (K, H, N) in enumerate([(KG + 1, NT + 1, 8 * NT + 1), (2 * KG + 1, 16 * NT + 1, NT - 1), (KG - 1, KG, NT)]):
        layers = bc.relu2_net(50 + i, K, H, N)
        x = bc.int_rows(50 + i, max(bc.TILE_ROWS), K)
        check_exact(layers, x, bc.relu2_logits(layers, x), tied, "relu K %d H %d N %d" % (K, H, N))


def walk_bound(layers, x, tied, what):
    """layer by layer from the DEVICE's previous activations (bf16 values): the float64 sum and S on the host, the bound of
    jd_mlp_bf16.h on the device's output of the layer.  Returns the worst error / bound of the linear part (last layer: raw logits)
    and of the hidden layers (propagated through the activation, plus the bf16 rounding)."""
    q, _ = models_of(layers, tied)
    prev = bc.bf16_round(x)
    worst_lin = worst_hid = 0.0
    n = len(layers)
    for l, (w, b, act) in enumerate(layers):
        assert bc.is_bf16(prev), (what, l)
        s, S = bc.linear_f64(w, b, prev)
        B = bc.bound(w.shape[1], S)
        dev = q.mlp_activations(x, l, on_device=True).astype(np.float64)
        if l == n - 1:
            ratio = np.abs(dev - s) / np.maximum(B, 1e-300)
            worst_lin = max(worst_lin, float(ratio.max()))
            assert np.all(np.abs(dev - s) <= B), "%s: layer %d logits beyond the bound, worst ratio %.3f" % (what, l, ratio.max())
        else:
            if act == mc.RELU:
                a64, lip = np.maximum(s, 0.0), 1.0
            elif act == mc.SIGMOID:
                with np.errstate(over="ignore"):
                    a64, lip = 1.0 / (1.0 + np.exp(-s)), 0.25
            else:
                a64, lip = s, 1.0
            # dev = bf16(a), a = the f32 activation of the device's pre-activation y: |y - s| <= B, so |a - act(s)| <= lip B + the f32
            # evaluation of the activation itself (expf within 1 ulp, the negation exact, the addition and the division half an ulp
            # each, the rounding of y to f32 half an ulp: below 4 ulps = 2^-22 relative), and |bf16(a) - a| <= 2^-8 |a|
            a_err = lip * B + 2.0 ** -22 * np.abs(a64)
            tol = a_err + 2.0 ** -8 * (np.abs(a64) + a_err)
            ratio = np.abs(dev - a64) / np.maximum(tol, 1e-300)
            worst_hid = max(worst_hid, float(ratio.max()))
            assert np.all(np.abs(dev - a64) <= tol), "%s: layer %d activations beyond the bound, worst ratio %.3f" % (what, l, ratio.max())
        prev = dev.astype(np.float32)
    return worst_lin, worst_hid


def test_bound_on_realistic_data(built, capsys):
    """mlp_cases.random_net / random_rows on the tile shapes, the limit shapes and one tied net of 1041 outputs: the derived bound
    2 (K + 1) 2^-23 S holds for every output of every layer; the worst observed error / bound is printed (DESIGN.md records it)"""
    worst = [0.0, 0.0]
    cases = [(s, False) for s in mc.tile_shapes() + mc.limit_shapes()] + [(s, True) for s in mc.tile_shapes()[6:]] + [((47, [129, 1041], [mc.SIGMOID]), True)]
    for i, ((in_dim, widths, acts), tied) in enumerate(cases):
        layers = mc.random_net(300 + i, in_dim, widths, acts)
        a, b = walk_bound(layers, mc.random_rows(300 + i, R + 1, in_dim), tied, "case %d" % i)
        worst = [max(worst[0], a), max(worst[1], b)]
    with capsys.disabled():
        print("\nworst |device - float64| / bound: logits %.4f, hidden activations %.4f" % tuple(worst))


@pytest.mark.parametrize("tied", [False, True], ids=["phone", "tied"])
def test_log_posteriors_from_the_devices_own_logits(built, tied):
    """bit for bit: the restated logZ chain (serial; 128 interleaved for tied) over the raw logits the device returns"""
    for i, (in_dim, widths, acts) in enumerate([(33, [65, 45], [mc.SIGMOID]), (17, [40, 130 if tied else 129], [mc.RELU])] + ([(9, [16, 1041], [mc.SIGMOID])] if tied else [])):
        layers = mc.random_net(400 + i, in_dim, widths, acts, scale=3.0)
        q, pr = models_of(layers, tied)
        x = mc.random_rows(400 + i, R + 2, in_dim)
        z = q.mlp_activations(x, len(layers) - 1, on_device=True)
        got = q.mlp_forward(x)
        rows = [0, R - 1, R, R + 1]
        assert np.array_equal(bits(got[rows]), bits(bc.logpost_rows(z[rows], tied))), i
        ll = q.score_frames(x)
        with np.errstate(all="ignore"):
            assert np.array_equal(bits(ll), bits(got - mc.log_priors(pr)[None, :])), i


@pytest.fixture(scope="module", params=[False, True], ids=["phone", "tied"])
def table_case(built, request):
    """a bf16 model, its priors, frames, the DEVICE's log posteriors of them (one launch of all rows), log priors, tied"""
    tied = request.param
    layers = mc.random_net(21, 19, [40, 1041 if tied else 23], [mc.SIGMOID])
    q, pr = models_of(layers, tied, seed=21)
    x = mc.random_rows(21, 4 * R + 1, 19)
    return q, pr, x, q.mlp_forward(x), mc.log_priors(pr), tied


def test_row_independence(table_case):
    """the same rows as a batch of 1, R - 1, R + 1 and 4 R + 1, at shuffled positions, and under max_blocks = 1: equal bits"""
    from juicer_amd import capi
    q, pr, x, full, lp, tied = table_case
    for n in (1, R - 1, R, R + 1):
        assert np.array_equal(bits(q.mlp_forward(x[:n])), bits(full[:n])), n
    perm = np.random.default_rng(5).permutation(x.shape[0])
    assert np.array_equal(bits(q.mlp_forward(x[perm])), bits(full[perm]))
    src = np.arange(x.shape[0], dtype=np.int32)
    pre = np.zeros((x.shape[0], full.shape[1]), np.float32)
    a, k, g = capi.debug_score_rows(q, x, src, pre)
    b, k1, g1 = capi.debug_score_rows(q, x, src, pre, max_blocks=1)
    assert (g, g1) == (5, 1) and k == k1 and np.array_equal(bits(a), bits(b))
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(a), bits(full - lp[None, :]))


def test_score_rows(table_case):
    """launch_gmm with the decoder's own arguments: rows with row_src = -1 are 0.0f, a whole unused tile included; the guard rows
    keep their prefill; the kernel is the bf16 one and the grid as planned; a tile list and SCORE_FAST are refused"""
    from juicer_amd import capi
    q, pr, x, logpost, lp, tied = table_case
    P = logpost.shape[1]
    rng = np.random.default_rng(3)
    n_rows, guard = 5 * R + 3, 2
    src = rng.integers(0, x.shape[0], n_rows).astype(np.int32)
    src[[0, 7, R - 1, n_rows - 1]] = -1
    src[2 * R:3 * R] = -1                                                    # a tile with no used row
    want = np.full((n_rows + 2 * guard, P), 777.25, np.float32)
    want[guard:guard + n_rows] = np.where(src[:, None] >= 0, logpost[np.maximum(src, 0)] - lp[None, :], np.float32(0.0))
    prefill = np.full_like(want, 777.25)
    kern = capi.KERNEL_MLP_TIED_BF16 if tied else capi.KERNEL_MLP_BF16
    got, kernel, grid = capi.debug_score_rows(q, x, src, prefill, guard_rows=guard)
    assert kernel == kern and grid == 6
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:4].tolist()
    got1, kernel1, grid1 = capi.debug_score_rows(q, x, src, prefill, guard_rows=guard, max_blocks=1)
    assert (kernel1, grid1) == (kern, 1) and np.array_equal(bits(got1), bits(want))
    got2, _, grid2 = capi.debug_score_rows(q, x, src, prefill, guard_rows=guard, max_blocks=4, skip_unused=1, used_row_tiles=2)
    assert grid2 == 4 and np.array_equal(bits(got2), bits(want))
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.debug_score_rows(q, x, src, prefill, guard_rows=guard, rt_base=[0])
    assert e.value.code == capi.JD_EINVAL and "tile lists are not for hybrid models" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.debug_score_rows(q, x, src, prefill, guard_rows=guard, mode=capi.SCORE_FAST)
    assert e.value.code == capi.JD_EINVAL


@pytest.mark.parametrize("tied", [False, True], ids=["phone", "tied"])
def test_nan_and_inf_rows(built, tied):
    """a NaN input row is NaN in that row only - also when one workgroup takes every tile in turn through the same LDS
    (max_blocks = 1) -, and an infinite input makes that row's logits infinite and no other's"""
    from juicer_amd import capi
    layers = mc.random_net(31, 33, [40, 37], [mc.SIGMOID])
    q, pr = models_of(layers, tied)
    x = mc.random_rows(31, 3 * R, 33)
    src = np.arange(3 * R, dtype=np.int32)
    pre = np.zeros((3 * R, 37), np.float32)
    clean, _, _ = capi.debug_score_rows(q, x, src, pre, max_blocks=1)
    assert np.all(np.isfinite(clean))
    y = x.copy()
    y[5, 3] = np.nan
    y[R + 1, :] = np.nan
    got, _, grid = capi.debug_score_rows(q, y, src, pre, max_blocks=1)
    assert grid == 1
    hit = np.zeros(3 * R, bool)
    hit[[5, R + 1]] = True
    assert np.all(np.isnan(got[hit])) and np.array_equal(bits(got[~hit]), bits(clean[~hit]))
    # one linear layer of positive weights: an infinite input makes that row's raw logits +inf and no other's
    w = np.full((NT + 1, KG + 1), 0.5, np.float32)
    q, _ = models_of([(w, np.zeros(NT + 1, np.float32), mc.LINEAR)], tied)
    y = np.ones((R + 1, KG + 1), np.float32)
    y[R, 2] = np.inf
    z = q.mlp_activations(y, 0, on_device=True)
    assert np.all(z[R] == np.inf) and np.all(z[:R] == np.float32(0.5 * (KG + 1)))


def test_conversions_equal_bf16_round(built):
    """the device's two conversions against jd_bf16_round's restatement: an accumulator that leaves a hidden layer (a LINEAR layer
    of zero input hands on its f32 biases) and the caller's features (an identity layer's logits are the rounded inputs) - seeded
    normal values and ties; an activation above the bf16 range becomes inf"""
    rng = np.random.default_rng(9)
    f = np.float32
    ties = np.array([1.00390625, 1.01171875, -1.00390625, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23, 0.0], f)
    for i in range(3):
        b = np.concatenate([ties, (rng.standard_normal(1024 - ties.shape[0]) * 10.0 ** (i - 1)).astype(f)])
        layers = [(np.ones((1024, 1), f), b, mc.LINEAR), (np.zeros((1, 1024), f), np.zeros(1, f), mc.LINEAR)]
        q, _ = models_of(layers, False)
        got = q.mlp_activations(np.zeros((2, 1), f), 0, on_device=True)
        assert np.array_equal(bits(got[0]), bits(bc.bf16_round(b))) and np.array_equal(bits(got[1]), bits(got[0]))
        assert mc.same_floats(got, q.mlp_activations(np.zeros((2, 1), f), 0, on_device=False))
    K = 2 * KG + 1
    q, _ = models_of([(np.eye(K, dtype=f), np.zeros(K, f), mc.LINEAR)], False)
    x = (rng.standard_normal((R + 1, K)) * 3.0).astype(f)
    x[0, :ties.shape[0]] = ties
    assert np.array_equal(bits(q.mlp_activations(x, 0, on_device=True)), bits(bc.bf16_round(x)))
    # 0x7f7f0000 + 2^119 = 0x7f7f8000 exactly: finite in f32, the midpoint past the largest bf16 -> inf (ties to even)
    big = np.array([0x7f7f0000], np.uint32).view(f)[0]
    layers = [(np.array([[big, f(2.0 ** 119)], [1.0, 1.0]], f), np.zeros(2, f), mc.LINEAR), (np.eye(2, dtype=f), np.zeros(2, f), mc.LINEAR)]
    q, _ = models_of(layers, False)
    got = q.mlp_activations(np.ones((1, 2), f), 0, on_device=True)
    assert got[0, 0] == np.inf and got[0, 1] == 2.0
    assert mc.same_floats(got, q.mlp_activations(np.ones((1, 2), f), 0, on_device=False))


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


@pytest.mark.parametrize("tied", [False, True], ids=["phone", "tied"])
def test_decoding(built, tied, capsys):
    """the bf16 model decodes - batch, streaming pushes of 37 frames, jd_streams_push on two streams - to the hypotheses, labels,
    times and bit-exact scores, of a plain hybrid decoder and of the CPU oracle, both fed the log posteriors jd_am_mlp_forward of
    the bf16 model returned.  Whether the words equal the f32 model's is printed, not asserted."""
    from juicer_amd import capi, synth
    from oracle.oracle import OracleAM, OracleDecoder, OracleNet
    spm = 3
    if tied:
        am, net, feats, pr, layers, tying = tc.anchor_case(spm)
        top = capi.Models.from_htk(am)
        f32 = capi.Models.from_mlp_tied(top, pr, layers)
        hyb = capi.Models.from_hybrid_tied(top, pr)
    else:
        am, net, feats, _ = synth.config_hybrid(seed=3 + spm, states_per_model=spm)
        pr = am.priors
        f32 = capi.Models.from_mlp(pr, spm, mc.decode_net(pr.shape[0], seed=spm))
        hyb = capi.Models.from_hybrid(pr, spm)
    q = f32.to_bf16()
    post = [q.mlp_forward(x) for x in feats]
    gnet = capi.Network.from_synth(net)
    for kw in mc.DECODE_BEAMS:
        ora = []
        for p in post:
            xo, po = tc.anchor_oracle_inputs(p, pr, tying) if tied else (p, pr)
            ora.append(OracleDecoder(OracleNet(net), OracleAM.from_hybrid(po, spm), **kw).decode_certified(xo))
        want = capi.Decoder(gnet, hyb, max_streams=len(feats), **kw).decode_batch(post)
        gm = capi.Decoder(gnet, q, max_streams=len(feats), **kw)
        runs = [("batch", gm.decode_batch(feats)), ("stream", [_stream(gm, feats[0])]), ("streams_push", _two_streams(gm, feats[:2]))]
        for name, got in runs:
            for u, g in enumerate(got):
                what = "tied %d %r %s utt %d" % (tied, kw, name, u)
                assert ora[u].n > 0
                assert_hyp_matches(g, ora[u], what, check_stats=name == "batch")
                assert bit_exact(g, ora[u]), what
                assert_hyp_matches(g, want[u], what, check_stats=False)
                assert bit_exact(g, want[u]), what
        ref = capi.Decoder(gnet, f32, max_streams=len(feats), **kw).decode_batch(feats)
        same = sum(list(a.label) == list(b.label) for a, b in zip(runs[0][1], ref))
        with capsys.disabled():
            print("\n%s %r: the bf16 model's words equal the f32 model's on %d of %d utterances" % ("tied" if tied else "phone", kw, same, len(ref)))


def test_refusals_and_batch_test(built, tmp_path):
    """what hybrid models refuse the bf16 model refuses; jd_batch_test -mlpFName ... -mlpBf16 gives the library call's hypotheses,
    and -mlpBf16 without a network file is a usage error"""
    from juicer_amd import build as jbuild, capi, io as jio, synth
    spm, d = 3, tmp_path
    am, net, feats, _ = synth.config_hybrid(seed=3 + spm, states_per_model=spm)
    f32 = capi.Models.from_mlp(am.priors, spm, mc.decode_net(am.priors.shape[0], seed=spm))
    q = f32.to_bf16()
    gd = capi.Decoder(capi.Network.from_synth(net), q, max_streams=len(feats), main_beam=150.0, max_hyps=100)
    with pytest.raises(capi.JuicerAmdError) as e:
        gd.set_pipeline(capi.FLOW_RESIDENT, 4, 2)
    assert e.value.code == capi.JD_ESTATE and "hybrid" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        gd.set_scoring(capi.SCORE_FAST)
    assert e.value.code == capi.JD_EINVAL and "hybrid" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        q.save_jmbi(str(d / "m.bin"))
    assert e.value.code == capi.JD_ESTATE and "hybrid" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        q.score_frames(feats[0], mode=capi.SCORE_FAST)
    assert e.value.code == capi.JD_EINVAL
    want = gd.decode_batch(feats)
    f32.save_mlp(str(d / "m.jmlp"))
    jio.write_fsm(d / "g.fsm", net)
    (d / "out.syms").write_text("<eps> 0\n" + "".join("W%d %d\n" % (i, i) for i in range(1, net.n_words + 1)))
    with open(d / "list.txt", "w") as f:
        for u, x in enumerate(feats):
            jio.write_htk(d / ("u%d.htk" % u), x)
            f.write("%s\n" % (d / ("u%d.htk" % u)))
    args = [jbuild.BATCH_TEST, "-fsmFName", str(d / "g.fsm"), "-mlpFName", str(d / "m.jmlp"), "-mlpBf16", "-inputFName", str(d / "list.txt"), "-mainBeam",
            "150", "-maxHyps", "100", "-outSymsFName", str(d / "out.syms"), "-outputFormat", "ref", "-batch", str(len(feats))]
    out = subprocess.run(args, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(want)
    for u in range(len(want)):
        assert want[u].n > 0 and lines[u].split() == ["W%d" % l for l in want[u].label[::-1]]
    out = subprocess.run([jbuild.BATCH_TEST, "-fsmFName", str(d / "g.fsm"), "-modelsFName", "none.jdam", "-mlpBf16", "-inputFName", str(d / "list.txt")],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "-mlpBf16 needs a network file" in out.stderr
