"""Neural acoustic models as far as they can be held without a device: csrc/jd_mlp.h through tests/mlp_driver.cpp - compiled with
plain g++, and once more with -fsanitize=address,undefined, as a stand-alone program - and through the C ABI (jd_am_create_mlp,
jd_am_mlp_forward_host, jd_am_save_mlp / jd_am_load_mlp), against tests/mlp_cases.py: the forward pass restated on libm's own
fmaf, expf and log, the packed layout and the JMLP file restated from the header's text."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mlp_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "juicer_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")


def build_driver(path, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I", CSRC, "-I", INCLUDE, "-o", path,
                           os.path.join(HERE, "mlp_driver.cpp")])
    return path


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("mlp") / "mlp_driver"))


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("mlp_san") / "mlp_driver_san"),
                        ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def write_net(path, layers, seed=0, spm=3):
    pr = mc.priors(seed, layers[-1][0].shape[0])
    with open(path, "wb") as f:
        f.write(mc.jmlp_bytes(pr, spm, layers))
    return pr


def drv_forward(drv, tmp, layers, x, stop, seed=0):
    net, xf, of = str(tmp / "net.jmlp"), str(tmp / "x.f32"), str(tmp / "out.f32")
    write_net(net, layers, seed)
    x = np.ascontiguousarray(x, np.float32)
    x.tofile(xf)
    subprocess.run([drv, "forward", net, xf, str(x.shape[0]), str(stop), of], check=True)
    return np.fromfile(of, np.float32).reshape(x.shape[0], -1)


@pytest.fixture(scope="module")
def seeded():
    """[(layers, rows, the restatement's log posteriors)] over mlp_cases.small_shapes(), computed once"""
    out = []
    for i, (in_dim, widths, acts) in enumerate(mc.small_shapes()):
        layers = mc.random_net(100 + i, in_dim, widths, acts)
        x = mc.random_rows(100 + i, 3, in_dim)
        out.append((layers, x, mc.forward(layers, x)))
    return out


def test_shapes_cover_the_issue():
    sh = mc.small_shapes()
    assert {s[0] for s in sh} == {1, 2, 33} and {s[1][-1] for s in sh} == {1, 31, 32, 33}
    assert {len(s[1]) for s in sh} == {1, 2, 3} and {a for s in sh for a in s[2]} == {mc.LINEAR, mc.RELU, mc.SIGMOID}
    assert {w for s in sh for w in s[1][:-1]} == {1, 31, 32, 33}


def test_host_twin_equals_restatement_on_seeded_networks(driver, driver_san, seeded, tmp_path):
    """bit for bit: log posteriors, hybrid scores and every layer's activations; the sanitizer build gives the same and reports nothing"""
    for i, (layers, x, want) in enumerate(seeded):
        got = drv_forward(driver, tmp_path, layers, x, -1, seed=i)
        assert mc.same_floats(got, want), (i, got, want)
        if i % 4 == 0:
            assert mc.same_floats(drv_forward(driver_san, tmp_path, layers, x, -1, seed=i), want), i
            lp = mc.log_priors(mc.priors(i, want.shape[1]))
            assert mc.same_floats(drv_forward(driver, tmp_path, layers, x, -2, seed=i), mc.forward(layers, x, -1, lp)), i
            for l in range(len(layers)):
                assert mc.same_floats(drv_forward(driver, tmp_path, layers, x, l, seed=i), mc.forward(layers, x, l)), (i, l)


@pytest.mark.parametrize("case", mc.crafted(), ids=lambda c: c[0])
def test_crafted_rows(driver, driver_san, case, tmp_path):
    """chain order, fusion, an overflowing sigmoid, the logAdd cut, a NaN row: the expected values are the literals of mlp_cases.crafted"""
    name, layers, x, want, what = case
    assert mc.same_floats(mc.forward(layers, x, what), want), "the restatement itself"
    assert mc.same_floats(drv_forward(driver, tmp_path, layers, x, what), want)
    assert mc.same_floats(drv_forward(driver_san, tmp_path, layers, x, what), want)


@pytest.mark.parametrize("case", mc.crafted(), ids=lambda c: c[0])
def test_crafted_rows_through_the_abi(built, case):
    """... and the library's host twin, which runs the kernels' replicas of expf and log instead of libm"""
    from juicer_amd import capi
    name, layers, x, want, what = case
    m = capi.Models.from_mlp(mc.priors(0, layers[-1][0].shape[0]), 3, layers)
    got = m.mlp_forward_host(x) if what < 0 else m.mlp_activations(x, what, on_device=False)
    assert mc.same_floats(got, want)


def test_abi_host_twin_equals_restatement(built, seeded):
    from juicer_amd import capi
    for i, (layers, x, want) in enumerate(seeded):
        m = capi.Models.from_mlp(mc.priors(i, want.shape[1]), 3, layers)
        assert (m.vec_size, m.n_gmms, m.n_hmms) == (layers[0][0].shape[1], want.shape[1], want.shape[1])
        assert m.mlp_info() == (layers[0][0].shape[1], [l[0].shape[0] for l in layers], [int(l[2]) for l in layers[:-1]] + [0])
        assert mc.same_floats(m.mlp_forward_host(x), want), i
        for l in range(len(layers)):
            assert mc.same_floats(m.mlp_activations(x, l, on_device=False), mc.forward(layers, x, l)), (i, l)


def test_host_twin_against_float64(driver, seeded, tmp_path, capsys):
    """What f32 and the -18.42 cut cost against a float64 forward with a true log-sum-exp.  No bound is fixed in advance: the
    restatement's own worst absolute error on the seeded cases is measured, and the host twin - which equals the restatement - is
    allowed exactly that.  (DESIGN.md 3.5 records the figure.)"""
    worst_ref = worst_twin = 0.0
    for i, (layers, x, want) in enumerate(seeded):
        ref = mc.forward_f64(layers, x)
        worst_ref = max(worst_ref, float(np.abs(want.astype(np.float64) - ref).max()))
        worst_twin = max(worst_twin, float(np.abs(drv_forward(driver, tmp_path, layers, x, -1, seed=i).astype(np.float64) - ref).max()))
    with capsys.disabled():
        print("\nworst |f32 contract - float64| over the seeded cases: restatement %.3e, host twin %.3e" % (worst_ref, worst_twin))
    assert worst_twin <= worst_ref
    assert worst_ref < 1e-4                       # (sanity only: log posteriors of magnitude <= ~10 in f32)


def test_pack_round_trip_and_zero_padding(driver, driver_san, tmp_path):
    for drv in (driver, driver_san):
        for i, (in_dim, widths, acts) in enumerate([(33, [31, 17, 5], [1, 2]), (1, [1], []), (16, [16, 32], [0]), (50, [48, 3], [2])]):
            layers = mc.random_net(i, in_dim, widths, acts)
            net = str(tmp_path / "n.jmlp")
            write_net(net, layers)
            files = [str(tmp_path / n) for n in ("wp", "bp", "w2", "b2")]
            subprocess.run([drv, "pack", net] + files, check=True)
            wp, bp, w2, b2 = [np.fromfile(f, np.float32) for f in files]
            want_wp, want_bp = mc.packed(layers)
            assert np.array_equal(wp.view(np.uint32), want_wp.view(np.uint32)) and np.array_equal(bp.view(np.uint32), want_bp.view(np.uint32))
            assert wp.shape[0] == sum(mc.pad16(l[0].shape[0]) * mc.pad16(l[0].shape[1]) for l in layers)
            # padding: every packed element that is no weight is +0.0 (bit pattern 0)
            assert int((wp.view(np.uint32) != 0).sum()) <= sum(l[0].size for l in layers)
            assert np.array_equal(w2.view(np.uint32), np.concatenate([l[0].ravel() for l in layers]).view(np.uint32))
            assert np.array_equal(b2.view(np.uint32), np.concatenate([l[1] for l in layers]).view(np.uint32))
            out = subprocess.run([drv, "dev", net], check=True, capture_output=True, text=True).stdout.split()
            widest = max([mc.pad16(in_dim)] + [mc.pad16(w) for w in widths])
            assert int(out[0]) == widest + 4 and int(out[1]) == (2 * 16 * (widest + 4) + 32) * 4


def test_lds_budget_at_the_limit():
    """two buffers of 16 rows at the widest layer the check admits fit a CU's 160 KB"""
    assert (2 * mc.ROWS * (mc.MAX_DIM + 4) + 2 * mc.ROWS) * 4 <= 160 * 1024


REFUSALS = [
    ((0, 4, 1, [4], []), "in_dim = 0 outside 1 .. 1024"),
    ((1025, 4, 1, [4], []), "in_dim = 1025 outside 1 .. 1024 (JD_MLP_MAX_DIM"),
    ((4, 4, 2, [1025, 4], [0]), "width[0] = 1025 outside 1 .. 1024 (JD_MLP_MAX_DIM"),
    ((4, 4, 2, [0, 4], [0]), "width[0] = 0 outside 1 .. 1024"),
    ((4, 4, 2, [8, 4], [3]), "act[0] = 3 is none of JD_ACT_LINEAR (0), JD_ACT_RELU (1), JD_ACT_SIGMOID (2)"),
    ((4, 4, 2, [8, 5], [1]), "the last width, 5, is not n_phones = 4"),
    ((4, 4, 17, [4] * 17, [0] * 16), "n_layers = 17 outside 1 .. 16 (JD_MLP_MAX_LAYERS)"),
    ((4, 4, 0, [], []), "n_layers = 0 outside 1 .. 16 (JD_MLP_MAX_LAYERS)"),
]


def _create(capi, in_dim, n_phones, n_layers, width, act, priors=None, spm=3):
    n = max(n_layers, 1)
    ws = [np.zeros(1 << 21, np.float32) for _ in range(min(n, 2))]                 # (large enough for any refused shape read by mistake)
    wp = (C.POINTER(C.c_float) * n)(*[ws[l % len(ws)].ctypes.data_as(C.POINTER(C.c_float)) for l in range(n)])
    pr = np.full(max(n_phones, 1), 1.0 / max(n_phones, 1), np.float32) if priors is None else np.asarray(priors, np.float32)
    wd, ac = np.asarray(width + [0], np.int32), np.asarray(act + [0], np.int32)
    h = C.c_void_p()
    rc = capi.lib().jd_am_create_mlp(C.byref(h), C.c_int32(n_phones), pr.ctypes.data_as(C.POINTER(C.c_float)), C.c_int32(spm), C.c_int32(in_dim),
                                     C.c_int32(n_layers), wd.ctypes.data_as(C.POINTER(C.c_int32)), ac.ctypes.data_as(C.POINTER(C.c_int32)), wp, wp)
    return rc, h, capi.lib().jd_last_error().decode()


@pytest.mark.parametrize("args,text", REFUSALS, ids=[r[1][:24] for r in REFUSALS])
def test_argument_refusals(built, driver, args, text):
    """every refusal with its message: the check itself (driver) and jd_am_create_mlp (JD_EINVAL, nothing created)"""
    from juicer_amd import capi
    in_dim, n_phones, n_layers, width, act = args
    out = subprocess.run([driver, "check", str(in_dim), str(n_phones), str(n_layers)] + [str(w) for w in width] + [str(a) for a in act + [0]][:len(width)],
                         check=True, capture_output=True, text=True).stdout
    assert out.split()[0] != "0" and text in out
    rc, h, msg = _create(capi, in_dim, n_phones, n_layers, width, act)
    assert rc == capi.JD_EINVAL and not h.value
    assert "jd_am_create_mlp" in msg and text in msg


def test_other_refusals(built):
    from juicer_amd import capi
    L = capi.lib()
    rc, h, msg = _create(capi, 4, 4, 1, [4], [], priors=[0.5, 0.0, 0.25, 0.25])
    assert rc == capi.JD_EINVAL and "jd_am_create_mlp: prior 1 is not positive" in msg
    rc, h, msg = _create(capi, 4, 4, 1, [4], [], spm=2)
    assert rc == capi.JD_EINVAL and "statesPerModel <= 2" in msg
    rc, h, msg = _create(capi, 4, 4, 1, [4], [], spm=9)
    assert rc == capi.JD_EINVAL and "more than 8 states" in msg
    assert L.jd_am_create_mlp(None, 4, None, 3, 4, 1, None, None, None, None) == capi.JD_EINVAL
    # the entry points that need a network refuse models without one
    hyb = capi.Models.from_hybrid(mc.priors(0, 4), 3)
    x = np.zeros((1, 4), np.float32)
    for call in (lambda: hyb.mlp_forward_host(x), lambda: hyb.mlp_info(), lambda: hyb.save_mlp("/nonexistent/x"),
                 lambda: hyb.mlp_forward(x)):
        with pytest.raises(capi.JuicerAmdError) as e:
            call()
        assert e.value.code == capi.JD_ESTATE and "no network" in str(e.value)
    m = capi.Models.from_mlp(mc.priors(0, 4), 3, mc.random_net(0, 4, [4], []))
    with pytest.raises(capi.JuicerAmdError) as e:
        m.save_jmbi("/nonexistent/x")
    assert e.value.code == capi.JD_ESTATE and "hybrid" in str(e.value)
    assert L.jd_debug_mlp_activations(m.h, 0, 0, x.ctypes.data_as(C.POINTER(C.c_float)), 1, 1, x.ctypes.data_as(C.POINTER(C.c_float))) == capi.JD_EINVAL
    assert "layer 1 outside [0, 1)" in L.jd_last_error().decode()
    # the device is asked for loudly: no fallback to the host twin
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(capi.JuicerAmdError) as e:
            m.mlp_forward(x)
        assert e.value.code in (capi.JD_ENODEV, capi.JD_EHIP)


def test_jmlp_save_load_save(built, driver, driver_san, tmp_path):
    """the file is the header's layout (restated in mlp_cases.jmlp_bytes); save, load, save is byte-identical; the driver's reader
    and writer agree"""
    from juicer_amd import capi
    layers = mc.random_net(4, 33, [31, 7], [mc.SIGMOID])
    pr = mc.priors(4, 7)
    m = capi.Models.from_mlp(pr, 5, layers)
    a, b, c = [str(tmp_path / n) for n in ("a.jmlp", "b.jmlp", "c.jmlp")]
    m.save_mlp(a)
    raw = open(a, "rb").read()
    assert raw == mc.jmlp_bytes(pr, 5, layers)
    m2 = capi.Models.load_mlp(a)
    m2.save_mlp(b)
    assert open(b, "rb").read() == raw
    assert (m2.vec_size, m2.n_gmms, m2.max_states) == (33, 7, 5) and m2.mlp_info() == m.mlp_info()
    x = mc.random_rows(4, 5, 33)
    assert mc.same_floats(m2.mlp_forward_host(x), m.mlp_forward_host(x))
    for drv in (driver, driver_san):
        out = subprocess.run([drv, "read", a, c], check=True, capture_output=True, text=True).stdout
        assert out.split()[0] == "0" and open(c, "rb").read() == raw


def test_jmlp_malformed_files(built, driver_san, tmp_path):
    from juicer_amd import capi
    layers = mc.random_net(5, 3, [4, 2], [mc.RELU])
    pr = mc.priors(5, 2)
    good = mc.jmlp_bytes(pr, 3, layers)
    bad_act = bytearray(good)
    bad_act[24 + 8 + 4:24 + 8 + 8] = (1).to_bytes(4, "little")              # act[last] != 0
    cases = [("empty", b""), ("magic", b"JMLQ" + good[4:]), ("version", mc.jmlp_bytes(pr, 3, layers, version=2)), ("header", good[:20]),
             ("widths", good[:28]), ("truncated", good[:-1]), ("half", good[:len(good) // 2]), ("longer", good + b"\0"),
             ("act", bytes(bad_act)), ("prior", mc.jmlp_bytes([0.5, -0.5], 3, layers)), ("states", mc.jmlp_bytes(pr, 2, layers)),
             ("layers", good[:20] + (99).to_bytes(4, "little") + good[24:])]
    for name, data in cases:
        p = str(tmp_path / (name + ".jmlp"))
        open(p, "wb").write(data)
        with pytest.raises(capi.JuicerAmdError) as e:
            capi.Models.load_mlp(p)
        assert e.value.code == capi.JD_EFORMAT, name
        if name not in ("prior", "states"):                                  # (those two are the model constructor's refusals)
            out = subprocess.run([driver_san, "read", p], check=True, capture_output=True, text=True).stdout
            assert out.split()[0] != "0", name
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.Models.load_mlp(str(tmp_path / "missing.jmlp"))
    assert e.value.code == capi.JD_EFORMAT


def test_header_constants_against_python(built):
    """no struct crosses the ABI for these models; the constants that do"""
    from juicer_amd import capi
    hdr = open(os.path.join(INCLUDE, "juicer_amd.h")).read()
    for name, val in (("JD_ACT_LINEAR", capi.ACT_LINEAR), ("JD_ACT_RELU", capi.ACT_RELU), ("JD_ACT_SIGMOID", capi.ACT_SIGMOID)):
        assert "#define %s" % name in hdr and int(hdr.split("#define %s" % name)[1].split()[0]) == val
    assert "JD_KERNEL_MLP = 9" in hdr and capi.KERNEL_MLP == 9 and len(capi.KERNEL_NAMES) == 9
    assert (capi.ACT_LINEAR, capi.ACT_RELU, capi.ACT_SIGMOID) == (mc.LINEAR, mc.RELU, mc.SIGMOID)
    for s in ("jd_am_create_mlp", "jd_am_mlp_info", "jd_am_save_mlp", "jd_am_load_mlp", "jd_am_mlp_forward", "jd_am_mlp_forward_host",
              "jd_debug_mlp_activations", "jd_debug_mlp_time"):
        assert s in capi.EXPORTS and hasattr(capi.lib(), s)


@pytest.mark.parametrize("spm", [5, 3])
def test_oracle_certifies_the_decoding_utterances(built, spm):
    """tests/test_gpu_mlp.py::test_decoding relies on decode_certified: at mlp_cases.DECODE_NOISE = 0.05 the CPU oracle certifies
    every utterance of the case (no order-dependent tie) under both beam sets, and finds a hypothesis"""
    from juicer_amd import capi, synth
    from oracle.oracle import OracleAM, OracleDecoder, OracleNet
    assert mc.DECODE_NOISE == 0.05
    am, net, feats, _ = synth.config_hybrid(seed=3 + spm, states_per_model=spm)
    mlp = capi.Models.from_mlp(am.priors, spm, mc.decode_net(am.priors.shape[0], seed=spm))
    oam = OracleAM.from_hybrid(am.priors, spm)
    for kw in mc.DECODE_BEAMS:
        od = OracleDecoder(OracleNet(net), oam, **kw)
        for x in feats:
            post = mlp.mlp_forward_host(x)
            assert od.decode_certified(post).n > 0
