"""bf16 neural acoustic models as far as they can be held without a device: csrc/jd_mlp_bf16.h through tests/mlp_bf16_driver.cpp -
compiled with plain g++, and once more with -fsanitize=address,undefined, as a stand-alone program - and through the C ABI
(jd_am_mlp_to_bf16, jd_am_mlp_precision, jd_am_mlp_forward_host, jd_am_save_mlp), against tests/mlp_bf16_cases.py: the rounding, the
packed layout and the host twin restated from the header's text; and the bf16 side of csrc/jd_score_plan.h."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import mlp_bf16_cases as bc
import mlp_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "juicer_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
K_MLP, K_MLP_TIED, K_MLP_BF16, K_MLP_TIED_BF16 = 9, 10, 11, 12
LDS_CU = 160 * 1024


def build_driver(path, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I", CSRC, "-I", INCLUDE, "-o", path,
                           os.path.join(HERE, "mlp_bf16_driver.cpp")])
    return path


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("mlp_bf16") / "mlp_bf16_driver"), ("-O2",))


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("mlp_bf16_san") / "mlp_bf16_driver_san"),
                        ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def write_net(path, layers, seed=0, spm=3):
    pr = mc.priors(seed, layers[-1][0].shape[0])
    with open(path, "wb") as f:
        f.write(mc.jmlp_bytes(pr, spm, layers))
    return pr


def drv_forward(drv, tmp, layers, x, stop, tied=False, seed=0):
    net, xf, of = str(tmp / "net.jmlp"), str(tmp / "x.f32"), str(tmp / "out.f32")
    write_net(net, layers, seed)
    x = np.ascontiguousarray(x, np.float32)
    x.tofile(xf)
    subprocess.run([drv, "forward", net, xf, str(x.shape[0]), str(stop), "1" if tied else "0", of], check=True)
    return np.fromfile(of, np.float32).reshape(x.shape[0], -1)


def drv_round(drv, tmp, x):
    a, b = str(tmp / "r.in"), str(tmp / "r.out")
    np.ascontiguousarray(x, np.float32).tofile(a)
    subprocess.run([drv, "round", a, b], check=True)
    return np.fromfile(b, np.float32)


def test_limits(driver):
    rows, kg, nt, lds, lds_tied = [int(v) for v in subprocess.run([driver, "limits"], check=True, capture_output=True, text=True).stdout.split()]
    assert (rows, kg, nt) == (bc.ROWS, bc.KG, bc.NT) and rows >= 32
    # two ping-pong buffers of 32 rows of bf16 at the widest layer, the bookkeeping and (tied) the partial chains fit a CU's 160 KB
    assert lds == 2 * 32 * bc.stride_of(mc.MAX_DIM, [mc.MAX_DIM]) * 2 + 2 * 32 * 4 and lds_tied == lds + 32 * 128 * 4 <= LDS_CU
    assert bc.stride_of(mc.MAX_DIM, []) == 1040


def test_round_every_bf16_pattern_and_its_midpoint(driver, driver_san, tmp_path):
    """all 65536 bf16 patterns, and for each the f32 values at, just below and just above the midpoint to its successor: ties to
    even, the carry into the exponent, overflow to inf, +-0, inf and NaN.  The expectation is built here from first principles - a
    bf16 value is itself; below the midpoint rounds down, above it up, the midpoint to the even pattern - and the numpy restatement
    (mlp_bf16_cases.bf16_round) is held to the same."""
    h = np.arange(65536, dtype=np.uint32)
    base = h << 16
    exp_all = (h & 0x7f80) == 0x7f80                       # inf and NaN patterns
    nan = exp_all & ((h & 0x7f) != 0)
    ins, want = [base], [base.copy()]
    fin = ~exp_all                                         # finite: the successor in magnitude is h + 1 (the largest finite's is inf)
    up = (h + 1) << 16
    even = np.where(h & 1, up, base)
    for off, w in ((0x7fff, base), (0x8000, even), (0x8001, up)):
        ins.append((base + off)[fin])
        want.append(w[fin])
    x, w = np.concatenate(ins), np.concatenate(want)
    for drv in (driver, driver_san):
        got = drv_round(drv, tmp_path, x.view(np.float32)).view(np.uint32)
        isn = (x & 0x7fffffff) > 0x7f800000
        assert np.array_equal(got[~isn], w[~isn])
        assert np.all((got[isn] & 0x7fffffff) > 0x7f800000) and not np.any(got[isn] & 0xffff)          # any NaN is a NaN, and a bf16 one
    assert int(nan.sum()) == 2 * 127
    ref = bc.bf16_round(x.view(np.float32)).view(np.uint32)
    assert np.array_equal(ref, drv_round(driver, tmp_path, x.view(np.float32)).view(np.uint32))
    # the named cases, as literals
    f = np.float32
    lit = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, 1.00390625, 1.01171875], f)
    out = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, 1.0, 1.015625], f)
    assert np.array_equal(drv_round(driver, tmp_path, lit).view(np.uint32), out.view(np.uint32))
    big = np.array([0x7f7f8000, 0xff7f8000, 0x7f7f7fff, 0x7f7f0000], np.uint32)       # the midpoint past the largest bf16, +-; just below it; the largest
    assert list(drv_round(driver, tmp_path, big.view(f)).view(np.uint32)) == [0x7f800000, 0xff800000, 0x7f7f0000, 0x7f7f0000]


PACK_SHAPES = [(33, [31, 17, 5], [1, 2]), (1, [1], []), (32, [32, 16], [0]), (31, [33, 15], [2]), (65, [17, 129, 3], [1, 1])]


def test_pack_round_trip_and_zero_padding(driver, driver_san, tmp_path):
    for drv in (driver, driver_san):
        for i, (in_dim, widths, acts) in enumerate(PACK_SHAPES):
            layers = mc.random_net(i, in_dim, widths, acts)
            net = str(tmp_path / "n.jmlp")
            write_net(net, layers)
            files = [str(tmp_path / n) for n in ("wp", "bp", "w2", "b2")]
            subprocess.run([drv, "pack", net] + files, check=True)
            wp = np.fromfile(files[0], np.uint16)
            bp, w2, b2 = [np.fromfile(f, np.float32) for f in files[1:]]
            want_wp, want_bp = bc.packed(layers)
            assert np.array_equal(wp, want_wp) and np.array_equal(bp.view(np.uint32), want_bp.view(np.uint32))
            assert wp.shape[0] == sum(bc.pad32(l[0].shape[0]) * bc.pad32(l[0].shape[1]) for l in layers)
            assert int((wp != 0).sum()) <= sum(l[0].size for l in layers)              # every element that is no weight is +0
            assert np.array_equal(w2.view(np.uint32), np.concatenate([bc.bf16_round(l[0]).ravel() for l in layers]).view(np.uint32))
            assert np.array_equal(b2.view(np.uint32), np.concatenate([l[1] for l in layers]).view(np.uint32))
            out = [int(v) for v in subprocess.run([drv, "dev", net], check=True, capture_output=True, text=True).stdout.split()]
            stride = bc.stride_of(in_dim, widths[:-1])
            assert stride % 128 == 16 and stride >= max([bc.pad32(in_dim)] + [bc.pad32(w) for w in widths[:-1]])
            assert out[:3] == [stride, 2 * 32 * stride * 2 + 256, 2 * 32 * stride * 2 + 256 + 32 * 128 * 4]
            n = len(layers)
            assert out[3:4 + n] == list(np.cumsum([0] + [bc.pad32(l[0].shape[0]) * bc.pad32(l[0].shape[1]) for l in layers]))
            assert out[4 + n:] == list(np.cumsum([0] + [bc.pad32(l[0].shape[0]) for l in layers]))


def test_lds_reads_are_conflict_free():
    """the header's argument for the row padding, counted: a 16-byte read is served in four groups of 16 lanes; lane l reads row
    l & 15 at byte 16 (l >> 4) of a k group; with a row stride of 16 modulo 128 elements every group falls on 16 distinct 16-byte
    slots of the 256-byte LDS row - and with the usual padding of 8 elements (one slot) it does not"""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[l + 32 for l in g] for g in groups]

    def worst(stride):
        return max(16 - len({(((l & 15) * stride * 2 + 16 * (l >> 4)) // 16) % 16 for l in g}) for g in groups)
    for width in (32, 64, 352, 512, 1024):
        assert worst(bc.stride_of(width, [])) == 0
    assert worst(1024 + 8) > 0 and worst(1024) > 0


@pytest.fixture(scope="module")
def seeded():
    """[(layers, rows, tied, the restatement's log posteriors)] over mlp_cases.small_shapes() and tile_shapes(), computed once"""
    out = []
    for i, (in_dim, widths, acts) in enumerate(mc.small_shapes() + mc.tile_shapes()):
        layers = mc.random_net(200 + i, in_dim, widths, acts)
        x = mc.random_rows(200 + i, 3, in_dim)
        out.append((layers, x, i % 2 == 1, bc.forward(layers, x, tied=i % 2 == 1)))
    return out


def test_host_twin_equals_restatement(driver, driver_san, seeded, tmp_path):
    """bit for bit: the log posteriors (serial logZ and, every other case, the 128 chains), the hybrid scores and every layer's
    activations; every hidden activation is a bf16 value; the sanitizer build gives the same and reports nothing"""
    for i, (layers, x, tied, want) in enumerate(seeded):
        got = drv_forward(driver, tmp_path, layers, x, -1, tied, seed=i)
        assert mc.same_floats(got, want), (i, got, want)
        for l in range(len(layers)):
            a = drv_forward(driver, tmp_path, layers, x, l, tied, seed=i)
            assert mc.same_floats(a, bc.forward(layers, x, l)), (i, l)
            if l < len(layers) - 1:
                assert bc.is_bf16(a), (i, l)
        if i % 4 == 0:
            assert mc.same_floats(drv_forward(driver_san, tmp_path, layers, x, -1, tied, seed=i), want), i
            lp = mc.log_priors(mc.priors(i, want.shape[1]))
            assert mc.same_floats(drv_forward(driver, tmp_path, layers, x, -2, tied, seed=i), bc.forward(layers, x, -1, lp, tied)), i


def test_abi_conversion(built, seeded, tmp_path):
    """jd_am_mlp_to_bf16 through the library (no device): the precision of every kind of models, the twin behind
    jd_am_mlp_forward_host and jd_debug_mlp_activations, idempotence, and the file - an ordinary JMLP holding the rounded weights"""
    from juicer_amd import capi
    import mlp_tied_cases as tc
    hdr = open(os.path.join(INCLUDE, "juicer_amd.h")).read()
    assert "JD_KERNEL_MLP_BF16 = 11" in hdr and "JD_KERNEL_MLP_TIED_BF16 = 12" in hdr
    assert (capi.KERNEL_MLP_BF16, capi.KERNEL_MLP_TIED_BF16, capi.MLP_F32, capi.MLP_BF16) == (11, 12, 0, 1)
    for s in ("jd_am_mlp_to_bf16", "jd_am_mlp_precision"):
        assert s in capi.EXPORTS and hasattr(capi.lib(), s)
    assert capi.Models.from_hybrid(mc.priors(0, 4), 3).mlp_precision == -1
    assert capi.Models.from_htk(tc.flat_topology(3)).mlp_precision == -1
    for i, (layers, x, tied, want) in enumerate(seeded[::5]):
        P = layers[-1][0].shape[0]
        pr = mc.priors(i, P)
        if tied:
            top = capi.Models.from_htk(tc.flat_topology(P))
            m = capi.Models.from_mlp_tied(top, pr, layers)
        else:
            m = capi.Models.from_mlp(pr, 3, layers)
        q = m.to_bf16()
        assert (m.mlp_precision, q.mlp_precision) == (capi.MLP_F32, capi.MLP_BF16)
        assert q.mlp_info() == m.mlp_info() and (q.vec_size, q.n_gmms, q.n_hmms, q.max_states) == (m.vec_size, m.n_gmms, m.n_hmms, m.max_states)
        assert mc.same_floats(q.mlp_forward_host(x), want), i
        for l in range(len(layers)):
            assert mc.same_floats(q.mlp_activations(x, l, on_device=False), bc.forward(layers, x, l)), (i, l)
        # src is only read: it still gives the f32 contract's values
        if not tied:
            assert mc.same_floats(m.mlp_forward_host(x), mc.forward(layers, x)), i
        # the file: version 1 or 2, the rounded weights as f32; loading gives f32 models, converting those an equal bf16 model
        a, b, c = [str(tmp_path / n) for n in ("a.jmlp", "b.jmlp", "c.jmlp")]
        q.save_mlp(a)
        assert open(a, "rb").read() == mc.jmlp_bytes(pr, 0 if tied else 3, bc.rounded(layers), version=2 if tied else 1)
        r = capi.Models.load_mlp_tied(top, a) if tied else capi.Models.load_mlp(a)
        assert r.mlp_precision == capi.MLP_F32
        q2, q3 = r.to_bf16(), q.to_bf16()
        q2.save_mlp(b)
        q3.save_mlp(c)
        assert open(b, "rb").read() == open(a, "rb").read() == open(c, "rb").read()
        assert q3.mlp_precision == capi.MLP_BF16
        assert mc.same_floats(q2.mlp_forward_host(x), want) and mc.same_floats(q3.mlp_forward_host(x), want), i


def test_refusals(built):
    from juicer_amd import capi
    import ctypes as C
    L = capi.lib()
    hyb = capi.Models.from_hybrid(mc.priors(0, 4), 3)
    with pytest.raises(capi.JuicerAmdError) as e:
        hyb.to_bf16()
    assert e.value.code == capi.JD_ESTATE and "jd_am_mlp_to_bf16: these models hold no network (jd_am_create_mlp / jd_am_load_mlp make the ones that do)" in str(e.value)
    h = C.c_void_p()
    assert L.jd_am_mlp_to_bf16(None, C.byref(h)) == capi.JD_EINVAL and L.jd_am_mlp_to_bf16(hyb.h, None) == capi.JD_EINVAL
    assert L.jd_am_mlp_precision(None) == -1
    q = capi.Models.from_mlp(mc.priors(0, 4), 3, mc.random_net(0, 4, [4], [])).to_bf16()
    with pytest.raises(capi.JuicerAmdError) as e:
        q.save_jmbi("/nonexistent/x")
    assert e.value.code == capi.JD_ESTATE and "hybrid" in str(e.value)
    x = np.zeros((1, 4), np.float32)
    with pytest.raises(capi.JuicerAmdError) as e:                # JD_SCORE_FAST stays refused, before any device is asked for
        q.score_frames(x, mode=capi.SCORE_FAST)
    assert e.value.code == capi.JD_EINVAL and "JD_SCORE_FAST" in str(e.value)
    import torch
    if not torch.cuda.is_available():                            # the device is asked for loudly: no fallback to the host twin
        with pytest.raises(capi.JuicerAmdError) as e:
            q.mlp_forward(x)
        assert e.value.code in (capi.JD_ENODEV, capi.JD_EHIP)


PLAN_FIELDS = ["D", "G", "hybrid", "mlp", "fast", "n_rows", "max_blocks", "used_row_tiles", "has_list", "n_rt_list", "tied", "bf16"]
PLAN_OUT = ["verdict", "kernel", "tile_rows", "tile_states", "row_tiles", "tiles", "grid", "lds_bytes", "dp"]


def run_plans(driver, cases):
    text = "".join(" ".join(str(int(c[f])) for f in PLAN_FIELDS) + "\n" for c in cases)
    lines = subprocess.run([driver, "plan"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(cases)
    return [dict(zip(PLAN_OUT, (int(v) for v in l.split()))) for l in lines]


def test_score_plan_bf16(driver, driver_san):
    base = dict(D=351, G=3000, hybrid=1, mlp=1, fast=0, n_rows=0, max_blocks=0, used_row_tiles=-1, has_list=0, n_rt_list=0, tied=0, bf16=1)
    cases = [dict(base, n_rows=n, max_blocks=mb, tied=t) for t in (0, 1) for n in (1, 31, 32, 33, 129, 8192) for mb in (0, 1, 3, 1000)]
    for drv in (driver, driver_san):
        for c, p in zip(cases, run_plans(drv, cases)):
            tiles = (c["n_rows"] + 31) // 32
            assert p["verdict"] == 0 and p["kernel"] == (K_MLP_TIED_BF16 if c["tied"] else K_MLP_BF16)
            assert p["tile_rows"] == 32 and p["tile_states"] == 0 and p["row_tiles"] == p["tiles"] == tiles
            assert p["grid"] == (min(tiles, c["max_blocks"]) if c["max_blocks"] else tiles) and p["grid"] >= 1
            # the LDS the kernel is told: the limit of its kind, inside a CU
            assert p["lds_bytes"] == 2 * 32 * 1040 * 2 + 256 + (32 * 128 * 4 if c["tied"] else 0) <= LDS_CU
    assert run_plans(driver, [dict(base, n_rows=0)])[0]["verdict"] == 1
    # bf16 is a property of models with a network: without mlp the field changes nothing
    for kind in (dict(hybrid=0, mlp=0, D=39), dict(hybrid=1, mlp=0)):
        a, b = run_plans(driver, [dict(base, n_rows=500, bf16=0, **kind), dict(base, n_rows=500, bf16=1, **kind)])
        assert a == b


def test_score_plan_is_unchanged_without_bf16(driver):
    """every recorded case of tests/golden/score_plan_golden.json (the plans of the code before jd_score_plan.h existed), and the
    f32 neural kernels, through this driver with bf16 = 0 - tied or not - give what they gave"""
    with open(os.path.join(HERE, "golden", "score_plan_golden.json")) as f:
        doc = json.load(f)
    ins = [dict(zip(doc["fields"], c["in"])) for c in doc["cases"]]
    cases = [dict(D=i["D"], G=i["G"], hybrid=i["hybrid"], mlp=i["mlp"], fast=i["fast"], n_rows=i["n_rows"], max_blocks=i["max_blocks"],
                  used_row_tiles=i["used_row_tiles"], has_list=i["has_list"], n_rt_list=i["n_rt_list"], tied=0, bf16=0) for i in ins]
    assert len(cases) > 50
    for c, rec, p in zip(cases, doc["cases"], run_plans(driver, cases)):
        assert [p["verdict"], p["kernel"], p["grid"], p["lds_bytes"]] == rec["out"][:4], c
    base = dict(D=40, G=3000, hybrid=1, mlp=1, fast=0, n_rows=100, max_blocks=3, used_row_tiles=-1, has_list=0, n_rt_list=0, tied=0, bf16=0)
    p, t = run_plans(driver, [base, dict(base, tied=1)])
    assert (p["kernel"], t["kernel"]) == (K_MLP, K_MLP_TIED) and p["tile_rows"] == t["tile_rows"] == 16 and p["tiles"] == 7 and p["grid"] == 3
    assert p["lds_bytes"] == t["lds_bytes"] == 0


def test_what_bf16_costs(driver, seeded, tmp_path, capsys):
    """The twin against mlp_cases.forward_f64 (float64, true log-sum-exp) on the seeded cases, beside the f32 contract's restatement
    against the same: measured and printed, no pass mark (DESIGN.md 3.5.1 records the figures)."""
    worst_bf16 = worst_f32 = 0.0
    for i, (layers, x, tied, want) in enumerate(seeded):
        ref = mc.forward_f64(layers, x)
        worst_bf16 = max(worst_bf16, float(np.abs(want.astype(np.float64) - ref).max()))
        if i % 3 == 0:
            worst_f32 = max(worst_f32, float(np.abs(mc.forward(layers, x).astype(np.float64) - ref).max()))
    with capsys.disabled():
        print("\nworst |log posterior - float64| over the seeded cases: bf16 twin %.3e, f32 contract %.3e" % (worst_bf16, worst_f32))
    assert np.isfinite(worst_bf16)
