"""Tied neural acoustic models as far as they can be held without a device: the tied side of csrc/jd_mlp.h through
tests/mlp_tied_driver.cpp (plain g++, libm) and through the C ABI (jd_am_create_hybrid_tied, jd_am_create_mlp_tied,
jd_am_load_mlp_tied, jd_am_mlp_forward_host), against tests/mlp_tied_cases.py: logZ restated from the header's text on the CPU
oracle's logAdd, the limits and refusals, JMLP version 2, and the CPU oracle's certificate for the decoding case of
tests/test_gpu_mlp_tied.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mlp_cases as mc
import mlp_tied_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "juicer_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")


def build_driver(exe, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I", CSRC, "-I", INCLUDE, "-o", exe,
                           os.path.join(HERE, "mlp_tied_driver.cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("mlp_tied") / "mlp_tied_driver"))


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    """the same stand-alone program under AddressSanitizer and UBSan"""
    return build_driver(str(tmp_path_factory.mktemp("mlp_tied_san") / "mlp_tied_driver_san"),
                        ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def drv_forward(drv, tmp, layers, pr, x, stop):
    net, xf, of = str(tmp / "net.jmlp"), str(tmp / "x.f32"), str(tmp / "out.f32")
    with open(net, "wb") as f:
        f.write(mc.jmlp_bytes(pr, 0, layers, version=2))
    x = np.ascontiguousarray(x, np.float32)
    x.tofile(xf)
    subprocess.run([drv, "forward", net, xf, str(x.shape[0]), str(stop), of], check=True)
    return np.fromfile(of, np.float32).reshape(x.shape[0], -1)


@pytest.fixture(scope="module")
def seeded(built):
    """[(P, layers, priors, models, rows, the library twin's raw logits, its log posteriors)] over LOGZ_WIDTHS, computed once.
    scale 4: logits spread over a few units, so that the order of the additions shows in the last bits"""
    out = []
    for i, P in enumerate(tc.LOGZ_WIDTHS):
        layers = tc.net_for(P, hidden=((16, 33, 1)[i % 3],), seed=300 + i, scale=4.0)
        m, pr = tc.tied_models(layers, seed=i)
        x = mc.random_rows(300 + i, 4, 9)
        out.append((P, layers, pr, m, x, m.mlp_activations(x, len(layers) - 1, on_device=False), m.mlp_forward_host(x)))
    return out


def test_host_twin_against_libm(driver, driver_san, seeded, tmp_path):
    """the header under plain g++ with libm's expf / log equals the library's twin (the kernels' replicas) on tied models, bit
    for bit: log posteriors, hybrid scores, raw logits and the hidden layer; the sanitizer build gives the same and reports nothing"""
    for P, layers, pr, m, x, z, lp in seeded:
        assert (m.vec_size, m.n_gmms, m.n_hmms) == (9, P, P) and m.mlp_info()[1][-1] == P
        assert mc.same_floats(drv_forward(driver, tmp_path, layers, pr, x, -1), lp), P
        assert mc.same_floats(drv_forward(driver_san, tmp_path, layers, pr, x, -1), lp), P
        assert mc.same_floats(drv_forward(driver, tmp_path, layers, pr, x, -2), lp - mc.log_priors(pr)[None, :]), P
        for l in range(len(layers)):
            assert mc.same_floats(drv_forward(driver, tmp_path, layers, pr, x, l), m.mlp_activations(x, l, on_device=False)), (P, l)


def test_logz_is_the_interleaved_definition(seeded):
    """an independent restatement - numpy float32 on oracle.log_add_array: 128 interleaved chains, then the chain of the partials -
    gives the twin's log posteriors bit for bit at every width; and on at least one case the serial chain gives OTHER bits, so
    that this test can tell the two definitions apart"""
    differs = []
    for P, layers, pr, m, x, z, lp in seeded:
        want = tc.logpost_of(z, tc.logz_tied(z))
        assert mc.same_floats(lp, want), (P, np.argwhere(lp.view(np.uint32) != want.view(np.uint32))[:4].tolist())
        serial = tc.logpost_of(z, tc.logz_serial(z))
        if not mc.same_floats(serial, want):
            differs.append(P)
        if P <= 1:
            assert mc.same_floats(serial, want)
    assert differs, "the interleaved and the serial chain agree on every seeded case: choose other seeds"
    print("\nwidths at which the serial chain's bits differ from the definition's: %s" % differs)


def test_untied_models_keep_the_serial_chain(built, seeded):
    """jd_am_create_mlp's models on the same networks: logZ is the one serial chain, as ever"""
    from juicer_amd import capi
    for P, layers, pr, m, x, z, lp in seeded:
        if P > mc.MAX_DIM:
            continue
        u = capi.Models.from_mlp(pr, 3, layers)
        assert mc.same_floats(u.mlp_activations(x, len(layers) - 1, on_device=False), z)
        assert mc.same_floats(u.mlp_forward_host(x), tc.logpost_of(z, tc.logz_serial(z))), P


def test_host_twin_against_float64(seeded, capsys):
    """what f32, the -18.42 cut and 128 chains cost against a float64 forward with a true log-sum-exp: measured and printed on
    every run, no pass mark (the sanity bound is the phone models': log posteriors of magnitude <= ~20 in f32)"""
    worst = 0.0
    for P, layers, pr, m, x, z, lp in seeded:
        worst = max(worst, float(np.abs(lp.astype(np.float64) - tc.forward_f64(layers, x)).max()))
    with capsys.disabled():
        print("\nworst |tied host twin - float64| over the seeded cases: %.3e" % worst)
    assert worst < 1e-3


@pytest.mark.parametrize("case", tc.crafted(), ids=lambda c: c[0])
def test_crafted_rows_through_the_abi(built, driver, case, tmp_path):
    name, layers, x, want = case
    m, pr = tc.tied_models(layers)
    assert mc.same_floats(m.mlp_forward_host(x), want), name
    assert mc.same_floats(drv_forward(driver, tmp_path, layers, pr, x, -1), want), name


# ---- limits and refusals
def _check(driver, tied, in_dim, n_out, width, act):
    out = subprocess.run([driver, "check", str(tied), str(in_dim), str(n_out), str(len(width))] + [str(w) for w in width] + [str(a) for a in act],
                         check=True, capture_output=True, text=True).stdout
    return int(out.split()[0]), out


def test_check_limits(driver):
    assert _check(driver, 1, 4, tc.MAX_OUT, [8, tc.MAX_OUT], [1, 0])[0] == 0
    rc, msg = _check(driver, 1, 4, tc.MAX_OUT + 1, [8, tc.MAX_OUT + 1], [1, 0])
    assert rc != 0 and "width[1] = 16385 outside 1 .. 16384 (JD_MLP_MAX_OUT" in msg
    rc, msg = _check(driver, 1, 4, 4, [1025, 4], [1, 0])
    assert rc != 0 and "width[0] = 1025 outside 1 .. 1024 (JD_MLP_MAX_DIM" in msg
    rc, msg = _check(driver, 1, 1025, 4, [4], [0])
    assert rc != 0 and "in_dim = 1025 outside 1 .. 1024 (JD_MLP_MAX_DIM" in msg
    rc, msg = _check(driver, 1, 4, 5, [8, 4], [1, 0])
    assert rc != 0 and "the last width, 4, is not the topology's number of tied states, n_gmm = 5" in msg
    # the phone models' check is as it was
    rc, msg = _check(driver, 0, 4, 1025, [1025], [0])
    assert rc != 0 and "width[0] = 1025 outside 1 .. 1024 (JD_MLP_MAX_DIM: the activations of a 16-row tile stay in LDS)" in msg
    assert _check(driver, 0, 4, 1024, [1024], [0])[0] == 0


def test_lds_budget_and_plan(driver, tmp_path):
    """the tied kernel's LDS holds in_dim and the hidden widths only, plus 16 x 128 partials, and fits a CU at the limit; the plan
    of a tied model is JD_KERNEL_MLP_TIED = 10 on 16-row tiles under max_blocks, and an untied plan is unchanged"""
    layers = tc.net_for(2063, hidden=(33,), in_dim=9)
    net = str(tmp_path / "n.jmlp")
    open(net, "wb").write(mc.jmlp_bytes(mc.priors(0, 2063), 0, layers, version=2))
    out = [int(v) for v in subprocess.run([driver, "dev", net], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == 48 + 4 and out[1] == (2 * 16 * 52 + 32 + 16 * 128) * 4 and out[2] == mc.pad16(2063) + 4
    assert (2 * 16 * (mc.MAX_DIM + 4) + 32 + 16 * tc.LZ_CHAINS) * 4 <= 160 * 1024
    plan = lambda *a: [int(v) for v in subprocess.run([driver, "plan"] + [str(v) for v in a], check=True, capture_output=True, text=True).stdout.split()]
    assert plan(1, 3000, 33, 0) == [10, 3, 16, 0, 0] and plan(1, 3000, 8192, 7) == [10, 7, 16, 0, 0]
    assert plan(0, 1000, 33, 0) == [9, 3, 16, 0, 0]
    hdr = open(os.path.join(INCLUDE, "juicer_amd.h")).read()
    from juicer_amd import capi
    assert "JD_KERNEL_MLP_TIED = 10" in hdr and capi.KERNEL_MLP_TIED == 10
    for s in ("jd_am_create_hybrid_tied", "jd_am_create_mlp_tied", "jd_am_load_mlp_tied"):
        assert s in capi.EXPORTS


def _zero_layers(in_dim, widths):
    out, k = [], in_dim
    for n in widths:
        out.append((np.zeros((n, k), np.float32), np.zeros(n, np.float32), mc.SIGMOID))
        k = n
    return out


def test_refusals_through_the_abi(built):
    from juicer_amd import capi
    top = capi.Models.from_htk(tc.flat_topology(6))
    pr = mc.priors(0, 6)
    ok = capi.Models.from_mlp_tied(top, pr, _zero_layers(4, [8, 6]))
    assert (ok.vec_size, ok.n_gmms, ok.n_hmms, ok.max_states) == (4, 6, 6, 3)

    def refused(call, *texts):
        with pytest.raises(capi.JuicerAmdError) as e:
            call()
        assert e.value.code == capi.JD_EINVAL, str(e.value)
        for t in texts:
            assert t in str(e.value), str(e.value)

    refused(lambda: capi.Models.from_mlp_tied(top, pr, _zero_layers(4, [8, 5])), "jd_am_create_mlp_tied", "the last width, 5, is not the topology's number of tied states, n_gmm = 6")
    refused(lambda: capi.Models.from_mlp_tied(top, pr, _zero_layers(4, [1025, 6])), "width[0] = 1025 outside 1 .. 1024 (JD_MLP_MAX_DIM")
    refused(lambda: capi.Models.from_mlp_tied(top, pr, _zero_layers(1025, [6])), "in_dim = 1025 outside 1 .. 1024")
    bad = pr.copy()
    bad[2] = 0.0
    refused(lambda: capi.Models.from_mlp_tied(top, bad, _zero_layers(4, [6])), "jd_am_create_mlp_tied: prior 2 is not positive")
    refused(lambda: capi.Models.from_hybrid_tied(top, -bad), "jd_am_create_hybrid_tied: prior 0 is not positive")
    # a hybrid or neural topology
    hyb = capi.Models.from_hybrid(pr, 3)
    refused(lambda: capi.Models.from_hybrid_tied(hyb, pr), "jd_am_create_hybrid_tied: topology holds hybrid or neural models")
    refused(lambda: capi.Models.from_mlp_tied(ok, pr, _zero_layers(4, [6])), "jd_am_create_mlp_tied: topology holds hybrid or neural models")
    refused(lambda: capi.Models.from_hybrid_tied(capi.Models.from_hybrid_tied(top, pr), pr), "topology holds hybrid")
    # null arguments, named
    L = capi.lib()
    h = C.c_void_p()
    prp = pr.ctypes.data_as(C.POINTER(C.c_float))
    assert L.jd_am_create_hybrid_tied(C.byref(h), None, prp) == capi.JD_EINVAL and "topology is null" in L.jd_last_error().decode()
    assert L.jd_am_create_hybrid_tied(C.byref(h), top.h, None) == capi.JD_EINVAL and "priors is null" in L.jd_last_error().decode()
    assert L.jd_am_create_hybrid_tied(None, top.h, prp) == capi.JD_EINVAL and "out is null" in L.jd_last_error().decode()
    assert L.jd_am_create_mlp_tied(C.byref(h), None, prp, 4, 1, None, None, None, None) == capi.JD_EINVAL and "topology is null" in L.jd_last_error().decode()
    assert not h.value
    # hybrid models' refusals hold
    for m in (ok, capi.Models.from_hybrid_tied(top, pr)):
        with pytest.raises(capi.JuicerAmdError) as e:
            m.save_jmbi("/nonexistent/x")
        assert e.value.code == capi.JD_ESTATE and "hybrid" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.Models.from_hybrid_tied(top, pr).mlp_info()
    assert e.value.code == capi.JD_ESTATE and "no network" in str(e.value)


def test_limits_through_the_abi(built):
    """last width 16384 accepted, 16385 refused; jd_am_create_mlp with width 1025 is refused with the text it always had"""
    from juicer_amd import capi
    top = capi.Models.from_htk(tc.flat_topology(tc.MAX_OUT))
    m = capi.Models.from_mlp_tied(top, np.full(tc.MAX_OUT, 1.0 / tc.MAX_OUT, np.float32), _zero_layers(2, [tc.MAX_OUT]))
    assert m.n_gmms == tc.MAX_OUT and m.mlp_info() == (2, [tc.MAX_OUT], [0])
    lp = m.mlp_forward_host(np.zeros((1, 2), np.float32))
    assert lp.shape == (1, tc.MAX_OUT) and abs(float(lp[0, 0]) + np.log(tc.MAX_OUT)) < 1e-4
    top1 = capi.Models.from_htk(tc.flat_topology(tc.MAX_OUT + 1))
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.Models.from_mlp_tied(top1, np.full(tc.MAX_OUT + 1, 0.5, np.float32), _zero_layers(2, [tc.MAX_OUT + 1]))
    assert e.value.code == capi.JD_EINVAL and "width[0] = 16385 outside 1 .. 16384 (JD_MLP_MAX_OUT" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.Models.from_mlp(np.full(1025, 0.5, np.float32), 3, _zero_layers(2, [1025]))
    assert e.value.code == capi.JD_EINVAL
    assert "jd_am_create_mlp: width[0] = 1025 outside 1 .. 1024 (JD_MLP_MAX_DIM: the activations of a 16-row tile stay in LDS)" in str(e.value)


# ---- the file
def test_jmlp_version_2(built, driver, driver_san, tmp_path):
    from juicer_amd import capi
    layers = tc.net_for(37, hidden=(31,), in_dim=33, seed=4)
    am = tc.flat_topology(37)
    top = capi.Models.from_htk(am)
    pr = mc.priors(4, 37)
    m = capi.Models.from_mlp_tied(top, pr, layers)
    a, b, c, v1 = [str(tmp_path / n) for n in ("a.jmlp", "b.jmlp", "c.jmlp", "v1.jmlp")]
    m.save_mlp(a)
    raw = open(a, "rb").read()
    assert raw == mc.jmlp_bytes(pr, 0, layers, version=2)                     # the header's layout: states_per_model = 0, n_phones = outputs
    m2 = capi.Models.load_mlp_tied(top, a)
    m2.save_mlp(b)
    assert open(b, "rb").read() == raw
    assert (m2.vec_size, m2.n_gmms, m2.n_hmms, m2.max_states) == (33, 37, 37, 3) and m2.mlp_info() == m.mlp_info()
    x = mc.random_rows(4, 5, 33)
    assert mc.same_floats(m2.mlp_forward_host(x), m.mlp_forward_host(x))
    out = subprocess.run([driver, "read", "1", a, c], check=True, capture_output=True, text=True).stdout
    assert out.split()[0] == "0" and open(c, "rb").read() == raw
    # version mix-ups, both directions: JD_EFORMAT naming the other loader
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.Models.load_mlp(a)
    assert e.value.code == capi.JD_EFORMAT and "jd_am_load_mlp_tied" in str(e.value)
    capi.Models.from_mlp(pr, 3, layers).save_mlp(v1)
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.Models.load_mlp_tied(top, v1)
    assert e.value.code == capi.JD_EFORMAT and "jd_am_load_mlp reads it" in str(e.value)
    # truncated, over-long, states_per_model != 0, a prior that is not positive
    bad_pr = pr.copy()
    bad_pr[3] = -1.0
    for name, data in (("truncated", raw[:-1]), ("half", raw[:len(raw) // 2]), ("longer", raw + b"\0"), ("header", raw[:20]),
                       ("spm", mc.jmlp_bytes(pr, 3, layers, version=2)), ("prior", mc.jmlp_bytes(bad_pr, 0, layers, version=2)),
                       ("version", mc.jmlp_bytes(pr, 0, layers, version=3))):
        p = str(tmp_path / (name + ".jmlp"))
        open(p, "wb").write(data)
        with pytest.raises(capi.JuicerAmdError) as e:
            capi.Models.load_mlp_tied(top, p)
        assert e.value.code == capi.JD_EFORMAT, name
        if name != "prior":                                                   # (that one is the model constructor's refusal)
            out = subprocess.run([driver_san, "read", "1", p], check=True, capture_output=True, text=True).stdout
            assert out.split()[0] != "0", name
    # a sound file beside another HMM set is the caller's mistake
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.Models.load_mlp_tied(capi.Models.from_htk(tc.flat_topology(36)), a)
    assert e.value.code == capi.JD_EINVAL and "37 outputs, the topology 36 tied states" in str(e.value)


def test_version_1_bytes_are_the_parents(built, tmp_path):
    """tests/golden/mlp_v1_parent.jmlp was written by jd_am_save_mlp of the commit before tied models (random_net(4, 33, [31, 7],
    [SIGMOID]), priors(4, 7), 5 states per model): this build writes the same bytes, and reads them"""
    from juicer_amd import capi
    want = open(os.path.join(HERE, "golden", "mlp_v1_parent.jmlp"), "rb").read()
    m = capi.Models.from_mlp(mc.priors(4, 7), 5, mc.random_net(4, 33, [31, 7], [mc.SIGMOID]))
    p = str(tmp_path / "v1.jmlp")
    m.save_mlp(p)
    assert open(p, "rb").read() == want
    q = str(tmp_path / "again.jmlp")
    capi.Models.load_mlp(os.path.join(HERE, "golden", "mlp_v1_parent.jmlp")).save_mlp(q)
    assert open(q, "rb").read() == want


# ---- the oracle's certificate for tests/test_gpu_mlp_tied.py::test_decoding
@pytest.mark.parametrize("spm", [5, 3])
def test_oracle_certifies_the_tied_decoding_utterances(built, spm):
    """the tying shares: fewer tied states than HMMs, at least a third of the HMMs share theirs; at noise 0.05 the CPU oracle's
    hybrid decoder, fed the gathered posteriors, certifies every utterance under both beam sets and finds a hypothesis"""
    from juicer_amd import capi
    from oracle.oracle import OracleAM, OracleDecoder, OracleNet
    assert mc.DECODE_NOISE == 0.05
    am, net, feats, pr, layers, tying = tc.anchor_case(spm)
    assert am.n_gmm < am.n_hmm and 3 * sum(1 for h in range(am.n_hmm) if (tying == tying[h]).sum() > 1) >= am.n_hmm
    mlp = capi.Models.from_mlp_tied(capi.Models.from_htk(am), pr, layers)
    assert (mlp.n_hmms, mlp.n_gmms, mlp.vec_size, mlp.max_states) == (30, 22, 30, spm)
    hn, hg, ht, _ = mlp.topology()
    assert np.array_equal(hg, am.hmm_gmm) and np.array_equal(hn, am.hmm_nstates)
    for kw in mc.DECODE_BEAMS:
        for x in feats:
            xo, po = tc.anchor_oracle_inputs(mlp.mlp_forward_host(x), pr, tying)
            od = OracleDecoder(OracleNet(net), OracleAM.from_hybrid(po, spm), **kw)
            assert od.decode_certified(xo).n > 0
