"""Context splicing of neural acoustic models as far as it can be held without a device: csrc/jd_splice.h through
tests/splice_driver.cpp - compiled with plain g++, and once more with -fsanitize=address,undefined, as a stand-alone program - and
through the C ABI (jd_am_mlp_splice, jd_am_mlp_context, jd_am_mlp_forward_host, jd_am_save_mlp), against tests/splice_cases.py: the
window, the spans and the push plan's promises restated from the header's text."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mlp_cases as mc
import mlp_tied_cases as tc
import splice_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "juicer_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
LDS_CU = 160 * 1024


def build_driver(path, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I", CSRC, "-I", INCLUDE, "-o", path,
                           os.path.join(HERE, "splice_driver.cpp")])
    return path


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("splice") / "splice_driver"), ("-O2",))


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("splice_san") / "splice_driver_san"),
                        ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_check(driver, driver_san):
    for drv in (driver, driver_san):
        def chk(in_dim, left, right):
            out = subprocess.run([drv, "check", str(in_dim), str(left), str(right)], check=True, capture_output=True, text=True).stdout.split("\n")
            rc, D = [int(v) for v in out[0].split()]
            return rc, D, out[1]
        assert chk(351, 4, 4)[:2] == (0, 39) and chk(7, 0, 0)[:2] == (0, 7) and chk(6, 2, 3)[:2] == (0, 1) and chk(1024, 8, 7)[:2] == (0, 64)
        rc, _, msg = chk(351, -1, 4)
        assert rc != 0 and "left and right are frames, 0 or more" in msg
        rc, _, msg = chk(351, 4, -2)
        assert rc != 0 and "left and right are frames, 0 or more" in msg
        rc, _, msg = chk(350, 4, 4)
        assert rc != 0 and "in_dim = 350 is not a multiple of left + right + 1 = 9 frames" in msg
        rc, _, msg = chk(4, 3, 3)
        assert rc != 0 and "not a multiple" in msg
        rc, _, msg = chk(8, 2 ** 31 - 1, 2 ** 31 - 1)                        # (the sum does not fit an int: the sanitized build sees it)
        assert rc != 0 and "not a multiple" in msg


def test_gather_is_the_numpy_window(driver, driver_san, tmp_path):
    """one utterance through jd_splice_gather: the clamp at both edges, utterances shorter than either context"""
    for drv in (driver, driver_san):
        for i, (n, D, left, right) in enumerate([(1, 3, 2, 2), (2, 1, 4, 0), (3, 5, 0, 4), (40, 13, 2, 3), (17, 39, 4, 4), (5, 2, 0, 0), (0, 4, 1, 1)]):
            f = sc.raw_frames(i, n, D)
            a, b = str(tmp_path / "f"), str(tmp_path / "x")
            f.tofile(a)
            subprocess.run([drv, "gather", a, str(n), str(D), str(left), str(right), b], check=True)
            got = np.fromfile(b, np.float32).reshape(n, (left + right + 1) * D)
            assert np.array_equal(bits(got), bits(sc.splice(f, left, right)))


def test_push_plan_exhaustively(driver, driver_san, tmp_path):
    """left, right in 0 .. 4, every split of T = 0 .. 12 frames into pushes of 1 .. 5 frames, and each again with an empty push in
    front of every piece and behind the last, then a finish: every frame becomes a row exactly once, in order, with the window
    clamp(t + c - left, 0, T - 1); every window lies inside the staging buffer, and inside the piece of it a chunk sends up; no more
    than left + right frames are kept and held = min(right, pushed) while the stream is open; nothing is held behind the finish."""
    recs, keys = [], []
    for left in range(5):
        for right in range(5):
            for T in range(13):
                for seq in sc.push_sequences(T):
                    recs.append(np.array([left, right, len(seq), *seq], np.int32))
                    keys.append((left, right, T, len(seq)))
    a, m, r = str(tmp_path / "in"), str(tmp_path / "meta"), str(tmp_path / "rows")
    np.concatenate(recs).tofile(a)
    subprocess.run([driver, "push", a, m, r], check=True)
    meta, rows = np.fromfile(m, np.int32).reshape(-1, 11), np.fromfile(r, np.int32)
    keys = np.array(keys, np.int64)
    left, right, T, n_push = keys.T
    assert meta.shape[0] == int((n_push + 1).sum())
    seq = meta[:, 0]
    assert np.array_equal(seq, np.repeat(np.arange(len(keys)), n_push + 1))
    L, R, TT = left[seq], right[seq], T[seq]
    last = np.concatenate([seq[1:] != seq[:-1], [True]])                        # the finish
    pushed, n_front, n_buf, n_keep, held, n_rows, row_first, lowest, highest, bad = meta[:, 1:].T
    assert not bad.any()
    assert np.array_equal(held[~last], np.minimum(R, pushed)[~last]) and not held[last].any()
    assert np.all(n_keep[~last] <= (L + R)[~last]) and np.all(n_front <= L + R) and np.all(n_buf >= n_front)
    assert np.all(lowest[n_rows > 0] >= 0) and np.all(highest[n_rows > 0] < n_buf[n_rows > 0])
    assert np.array_equal(pushed[last], TT[last])
    # the rows of a call follow those of the calls before it: rows are [0, T) in order
    before = np.concatenate([[0], np.cumsum(n_rows)[:-1]])
    first_of_seq = np.concatenate([[True], seq[1:] != seq[:-1]])
    seq_row0 = np.maximum.accumulate(np.where(first_of_seq, before, 0))
    assert np.array_equal(row_first, before - seq_row0)
    # ... with the windows of the definition, as VALUES read from the staging buffer
    at = 0
    for i in range(len(keys)):
        C_ = int(left[i] + right[i] + 1)
        n = int(T[i]) * (C_ + 1)
        got = rows[at:at + n].reshape(int(T[i]), C_ + 1)
        at += n
        want = np.concatenate([np.arange(T[i], dtype=np.int32)[:, None], sc.windows(int(T[i]), int(left[i]), int(right[i]))], axis=1)
        assert np.array_equal(got, want), (keys[i], got, want)
    assert at == rows.shape[0]
    # the sanitized build: the same answers on a slice of the cases (every context, the longest utterance)
    pick = [i for i in range(len(keys)) if T[i] in (0, 1, 12) and i % 7 == 0]
    np.concatenate([recs[i] for i in pick]).tofile(a)
    m2, r2 = str(tmp_path / "meta2"), str(tmp_path / "rows2")
    subprocess.run([driver_san, "push", a, m2, r2], check=True)
    subprocess.run([driver, "push", a, m, r], check=True)
    assert open(m, "rb").read() == open(m2, "rb").read() and open(r, "rb").read() == open(r2, "rb").read()


def test_batch_spans(driver, driver_san):
    """wave_layout plans with several chunks and utterances of length 0, 1 and more than Fc, scattered over the feature buffer: every
    used row's span is its utterance's first and last frame there, whichever chunk the row sits in"""
    cases = [(8, 4, [(0, 0), (0, 1), (1, 30), (40, 8), (100, 9)]), (128, 128, [(5, 300), (305, 1), (306, 0), (400, 129)]),
             (16, 16, [(0, 16), (16, 17), (33, 15)]), (0, 128, [(0, 5), (5, 200)])]
    for drv in (driver, driver_san):
        for fc, tile, utts in cases:
            args = [drv, "wave", str(fc), str(tile), str(len(utts))]
            for s, n in utts:
                args += [str(s), str(n)]
            out = subprocess.run(args, check=True, capture_output=True, text=True).stdout.split("\n")
            n_chunks, Fc = [int(v) for v in out[0].split()]
            longest = max(n for _, n in utts)
            assert n_chunks == max(1, -(-longest // Fc)) and (fc == 0 or (Fc == fc and n_chunks > 1 and longest > Fc))
            t = np.array([[int(v) for v in l.split()] for l in out[1:] if l], np.int64)
            used = t[t[:, 0] >= 0]
            assert used.shape[0] == sum(n for _, n in utts)
            seen = []
            for src, lo, hi in used:
                owner = [(s, n) for s, n in utts if s <= src < s + n]
                assert len(owner) == 1 and (lo, hi) == (owner[0][0], owner[0][0] + owner[0][1] - 1)
                seen.append(src)
            assert sorted(seen) == sorted(f for s, n in utts for f in range(s, s + n))


def test_score_plan_spliced(driver):
    """the spliced kernels are 13 .. 16, on their parents' tiles and grids; the bf16 bound grows by the tile's spans"""
    def plan(n_rows, max_blocks, tied, bf16, spliced):
        out = subprocess.run([driver, "plan", "39", "45", str(n_rows), str(max_blocks), str(int(tied)), str(int(bf16)), str(int(spliced))],
                             check=True, capture_output=True, text=True).stdout.split()
        return [int(v) for v in out]
    for tied in (False, True):
        for bf16 in (False, True):
            for n_rows, mb in ((1, 0), (64, 0), (65, 0), (8192, 7)):
                p, s = plan(n_rows, mb, tied, bf16, False), plan(n_rows, mb, tied, bf16, True)
                assert p[0] == 9 + int(tied) + 2 * int(bf16) and s[0] == 13 + int(tied) + 2 * int(bf16)
                assert s[1:3] == p[1:3] and s[3] == p[3] + (8 * 32 if bf16 else 0) <= LDS_CU


def models_of(kind, shape, seed):
    """(parent, spliced) models of a shape of splice_cases.SHAPES: kind in plain / tied, f32"""
    from juicer_amd import capi
    D, left, right, widths = shape
    layers = sc.parent_layers(shape, seed, tied=kind == "tied")
    if kind == "tied":
        parent = tc.tied_models(layers, seed)[0]
    else:
        parent = capi.Models.from_mlp(mc.priors(seed, widths[-1]), 3, layers)
    return parent, parent.splice(left, right)


@pytest.mark.parametrize("shape", sc.SHAPES[:5], ids=sc.shape_id)
@pytest.mark.parametrize("kind", ["plain", "tied"])
def test_host_twin_equals_parent_on_numpy_splice(built, kind, shape):
    """mlp_forward_host and every layer's activations of a spliced model on raw frames = its parent's on the frames spliced with
    numpy, bit for bit, in f32 and in bf16; splicing then bf16 = bf16 then splicing; vec_size, mlp_info and mlp_context"""
    D, left, right, widths = shape
    parent, spl = models_of(kind, shape, 5)
    assert spl.vec_size == D and parent.vec_size == D * (left + right + 1)
    assert spl.mlp_info() == parent.mlp_info() and spl.mlp_info()[0] == D * (left + right + 1)
    assert spl.mlp_context == (left, right) and parent.mlp_context == (0, 0)
    assert spl.mlp_precision == parent.mlp_precision and spl.n_gmms == parent.n_gmms
    for T in (1, 2, 7):
        f = sc.raw_frames(T, T, D)
        x = sc.splice(f, left, right)
        variants = [("f32", parent, spl), ("splice then bf16", parent.to_bf16(), spl.to_bf16()), ("bf16 then splice", parent.to_bf16(), parent.to_bf16().splice(left, right))]
        for name, p, s in variants:
            assert s.mlp_context == (left, right) and s.vec_size == D and s.mlp_precision == p.mlp_precision
            assert np.array_equal(bits(s.mlp_forward_host(f)), bits(p.mlp_forward_host(x))), (name, T)
            for l in range(len(widths)):
                assert np.array_equal(bits(s.mlp_activations(f, l, on_device=False)), bits(p.mlp_activations(x, l, on_device=False))), (name, T, l)


def test_zero_context_behaves_like_the_parent(built):
    from juicer_amd import capi
    layers = mc.random_net(3, 6, [8, 4], [mc.SIGMOID])
    parent = capi.Models.from_mlp(mc.priors(3, 4), 3, layers)
    s = parent.splice(0, 0)
    x = mc.random_rows(3, 5, 6)
    assert s.vec_size == 6 and s.mlp_context == (0, 0)
    assert np.array_equal(bits(s.mlp_forward_host(x)), bits(parent.mlp_forward_host(x)))
    with pytest.raises(capi.JuicerAmdError) as e:                               # (spliced all the same: a second splice is refused)
        s.splice(0, 0)
    assert e.value.code == capi.JD_EINVAL and "spliced already" in str(e.value)


def test_refusals(built):
    from juicer_amd import capi
    L = capi.lib()
    parent = capi.Models.from_mlp(mc.priors(0, 4), 3, mc.random_net(0, 12, [4], []))
    for m in (capi.Models.from_hybrid(mc.priors(0, 4), 3), capi.Models.from_htk(tc.flat_topology(3))):
        with pytest.raises(capi.JuicerAmdError) as e:
            m.splice(1, 1)
        assert e.value.code == capi.JD_EINVAL and "jd_am_mlp_splice: these models hold no network" in str(e.value)
        with pytest.raises(capi.JuicerAmdError) as e:
            m.mlp_context
        assert e.value.code == capi.JD_EINVAL and "jd_am_mlp_context: these models hold no network" in str(e.value)
    for left, right in ((-1, 1), (1, -1)):
        with pytest.raises(capi.JuicerAmdError) as e:
            parent.splice(left, right)
        assert e.value.code == capi.JD_EINVAL and "context (%d, %d): left and right are frames, 0 or more" % (left, right) in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        parent.splice(2, 2)
    assert e.value.code == capi.JD_EINVAL and "in_dim = 12 is not a multiple of left + right + 1 = 5 frames" in str(e.value)
    s = parent.splice(1, 2)
    for again in (s, s.to_bf16()):
        with pytest.raises(capi.JuicerAmdError) as e:
            again.splice(0, 0)
        assert e.value.code == capi.JD_EINVAL and "spliced already, with context (1, 2)" in str(e.value)
    h = C.c_void_p()
    assert L.jd_am_mlp_splice(None, 1, 1, C.byref(h)) == capi.JD_EINVAL and L.jd_am_mlp_splice(parent.h, 1, 1, None) == capi.JD_EINVAL
    assert L.jd_am_mlp_context(None, None, None) == capi.JD_EINVAL
    # jd_debug_score_rows names the call that takes the spans; that call is a spliced model's alone (both before any device is asked for)
    out = np.zeros((2, 4), np.float32)
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.debug_score_rows(s, np.zeros((2, 3), np.float32), [0, 1], out)
    assert e.value.code == capi.JD_EINVAL and "jd_debug_score_rows_span" in str(e.value) and "spliced" in str(e.value)
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.debug_score_rows(parent, np.zeros((2, 12), np.float32), [0, 1], out, row_lo=[0, 0], row_hi=[1, 1])
    assert e.value.code == capi.JD_EINVAL and "spans are a spliced model's" in str(e.value)
    for lo, hi, what in (([0, -1], [1, 1], "row_lo[1] = -1 outside [0, 2)"), ([0, 0], [1, 2], "row_hi[1] = 2 outside [0, 2)"), ([1, 0], [0, 1], "row_lo[0] = 1 above row_hi[0] = 0")):
        with pytest.raises(capi.JuicerAmdError) as e:
            capi.debug_score_rows(s, np.zeros((2, 3), np.float32), [0, 1], out, row_lo=lo, row_hi=hi)
        assert e.value.code == capi.JD_EINVAL and what in str(e.value)
    for sym in ("jd_am_mlp_splice", "jd_am_mlp_context", "jd_debug_score_rows_span", "jd_stream_held_frames"):
        assert sym in capi.EXPORTS and hasattr(L, sym)
    assert (capi.KERNEL_MLP_SPLICED, capi.KERNEL_MLP_TIED_SPLICED, capi.KERNEL_MLP_BF16_SPLICED, capi.KERNEL_MLP_TIED_BF16_SPLICED) == (13, 14, 15, 16)


def test_save_mlp_writes_the_parents_bytes(built, tmp_path):
    """the ordinary JMLP file of the network, version 1 or 2: the format has no context field, the caller splices again after loading"""
    from juicer_amd import capi
    for kind in ("plain", "tied"):
        parent, s = models_of(kind, sc.SHAPES[3], 9)
        a, b, c = str(tmp_path / "p.jmlp"), str(tmp_path / "s.jmlp"), str(tmp_path / "q.jmlp")
        parent.save_mlp(a)
        s.save_mlp(b)
        assert open(a, "rb").read() == open(b, "rb").read()
        assert open(a, "rb").read()[4:8] == (b"\x02\0\0\0" if kind == "tied" else b"\x01\0\0\0")
        parent.to_bf16().save_mlp(a)
        s.to_bf16().save_mlp(c)
        assert open(a, "rb").read() == open(c, "rb").read()
        r = capi.Models.load_mlp_tied(capi.Models.from_htk(tc.flat_topology(sc.TIED_OUTPUTS)), b) if kind == "tied" else capi.Models.load_mlp(b)
        assert r.mlp_context == (0, 0) and r.vec_size == parent.vec_size
        f = sc.raw_frames(1, 6, sc.SHAPES[3][0])
        assert np.array_equal(bits(r.splice(3, 3).mlp_forward_host(f)), bits(s.mlp_forward_host(f)))
