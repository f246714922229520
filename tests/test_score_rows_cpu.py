"""The cases of tests/score_rows_cases.py themselves, without a GPU: every cell of a case's guarded buffer is classified once, the
unspecified share is within its cap, a case holds the feature it is named for, the expected values stand on a second witness
(float64), every kernel gets its row maps - and what jd_debug_score_rows refuses, it refuses on the host, before it asks for a device."""
import numpy as np
import pytest

import score_rows_cases as sc
from score_rows_cases import CASES, CASE_IDS, UNSPEC, UNTOUCHED, VALUE


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_case_classifies_every_cell_once(built, case):
    cls, want = case.classify()                            # (asserts the cap and that no two scored tiles overlap)
    m = sc.model(case.model_key)
    gr, n, h = case.guard_rows, case.n_rows, case.h
    assert cls.shape == want.shape == case.prefill().shape == (n + 2 * gr, m.G)
    assert gr >= max(h, 1)
    assert np.isin(cls, (UNTOUCHED, VALUE, UNSPEC)).all()
    assert (cls[:gr] == UNTOUCHED).all() and (cls[gr + n:] == UNTOUCHED).all()
    assert (cls == cls[:, :1]).all()                       # a row's cells are of one class
    # row by row, from the definitions (not the builder's slices)
    src = case.row_src
    assert src.min() >= -1 and src.max() < sc.N_FRAMES
    for r in range(n):
        if h == 0:
            scored = True
        elif case.rt_base is not None:
            t = [int(r0) for r0 in case.rt_base if r0 <= r < r0 + h]
            assert len(t) <= 1
            scored = bool(t) and not (case.skip_unused and src[t[0]] < 0)
        else:
            scored = not (case.skip_unused and src[r // h * h] < 0)
        expect = UNTOUCHED if not scored else (VALUE if src[r] >= 0 else UNSPEC)
        assert cls[gr + r, 0] == expect, (case.id, r)
    # the values are the oracle's rows of the source frames; nothing is expected elsewhere
    tab = m.oracle_table()
    for r in np.nonzero(src >= 0)[0][:: max(1, n // 16)]:
        if cls[gr + r, 0] == VALUE:
            assert sc.same_floats(want[gr + r], tab[src[r]])
    assert (want[cls != VALUE] == 0.0).all()
    if n > 1:                                              # (one row may be the NaN frame's) most expected values are finite: the fast mode's share
        assert np.isfinite(want[cls == VALUE]).mean() > 0.5
    # the prefill is no likelihood: NaNs, every cell its own, none of them a NaN an operation makes
    pre = case.prefill().view(np.uint32).ravel()
    assert np.isnan(case.prefill()).all() and np.unique(pre).shape[0] == pre.shape[0]
    assert not np.isin(pre, np.uint32([0x7FC00000, 0xFFC00000])).any()
    assert not np.isin(pre, m.frames.view(np.uint32).ravel()).any()
    # with skip_unused the map keeps the kernels' precondition: a scored tile's used rows are a prefix of it
    if case.skip_unused and h:
        for r0 in ([int(v) for v in case.rt_base] if case.rt_base is not None else range(0, n, h)):
            u = src[r0:min(n, r0 + h)] >= 0
            assert not (np.diff(u.astype(np.int8)) > 0).any(), (case.id, r0)
    # the kernel is the one the models and the mode give
    if case.kernel == sc.K_HYBRID:
        assert m.kind == "hybrid"
    elif case.kernel == sc.K_GENERIC:
        assert m.kind == "synth" and m.D != 39
    elif case.kernel in (sc.K_FAST_16, sc.K_FAST_64):
        assert m.D != 39 and case.mode == sc.SCORE_FAST
    else:
        assert m.D == 39
    # ... and its width follows from the arguments as launch_gmm chooses it
    if case.kernel in sc.LIST_KERNELS:
        n_gt64 = -(-m.G // 64)
        tiles = (case.used_row_tiles if case.used_row_tiles >= 0 else case.row_tiles()) * n_gt64
        assert (tiles < 1024) == (sc.TILE_STATES[case.kernel] == 16), case.id
    assert case.grid() >= 1


@pytest.mark.parametrize("case", [c for c in CASES if c.feature], ids=[c.id for c in CASES if c.feature])
def test_case_holds_its_feature(built, case):
    cls, _ = case.classify()
    gr, n, h, src = case.guard_rows, case.n_rows, case.h, case.row_src
    rows = cls[gr:gr + n, 0]
    if case.feature == "pair":
        # PAIR_FRAME at both rows of a lane (r and r + 64) and, with a second tile, there too
        assert src[5] == src[5 + 64] == sc.PAIR_FRAME
        if n > h:
            assert src[h] == sc.PAIR_FRAME
    elif case.feature == "nan":
        r = 70
        assert src[r] == sc.NAN_FRAME and (src == sc.NAN_FRAME).sum() == 1
        tab = sc.model(case.model_key).oracle_table()
        assert np.isnan(tab[sc.NAN_FRAME]).all()
        for q in (r - 1, r + 1, r - 64, r + 64):
            assert rows[q] == VALUE and np.isfinite(tab[src[q]]).mean() > 0.5 and np.isnan(tab[src[q]]).mean() < 0.05      # (inf - inf states)
    elif case.feature == "holes":
        hh = h or 128
        hole = np.nonzero(rows == UNSPEC)[0]
        assert ((hole % hh) < hh // 2).any() and ((hole % hh) >= hh // 2).any()          # a hole in each lane half
        half = [t for t in range(0, n - hh + 1, hh) if (rows[t + hh // 2:t + hh] == UNSPEC).all() and (rows[t:t + hh // 2 - 4] == VALUE).all()]
        assert half, "no tile whose whole second half is unused"
    elif case.feature == "skipped":
        t = [r0 for r0 in range(0, n, h) if (rows[r0:r0 + h] == UNTOUCHED).all()]
        assert case.skip_unused and t and len(t) < -(-n // h)
        if case.id.endswith("d_skip1"):
            assert t == [h, 3 * h] and n == 5 * h
    elif case.feature == "unused_scored":
        assert not case.skip_unused and n == 5 * h
        assert (rows[h:2 * h] == UNSPEC).all() and (rows[3 * h:4 * h] == UNSPEC).all() and (rows != UNTOUCHED).all()
    elif case.feature in ("unlisted", "cut"):
        assert case.rt_base is not None and (rows == UNTOUCHED).any() and (rows == VALUE).any()
        assert -(-n // h) == 6 and len(case.rt_base) < 6
        if case.feature == "cut":
            last = int(max(case.rt_base))
            assert last + h > n > last and (rows[last:] == VALUE).all()
    else:
        raise AssertionError(case.feature)


def test_every_kernel_gets_its_row_maps(built):
    by_kernel = {}
    for c in CASES:
        by_kernel.setdefault(c.kernel, []).append(c.id.split("-")[-1])
    assert sorted(by_kernel) == list(range(1, 9))                     # the eight kernels
    for k, ids in by_kernel.items():
        if k == sc.K_HYBRID:
            want = ["a1", "a129", "c_skip0", "c_skip1", "c_max_blocks_ignored"]
        else:
            h = sc.TILE_ROWS[k]
            want = ["a%d" % n for n in (1, h - 1, h, h + 1, 2 * h + 1)] + ["b", "c_scattered", "c_tails_skip0", "c_tails_skip1", "d_skip0", "d_skip1",
                                                                           "f_blocks1", "f_blocks3"]
            if k in sc.LIST_KERNELS:
                want += ["e_412", "e_one", "e_cut"]
        assert set(want) <= set(ids), (sc.KERNEL_NAMES[k], sorted(set(want) - set(ids)))
    # the bounded grids: 1, the row tiles, one less than the tiles
    for c in CASES:
        if c.max_blocks and c.kernel != sc.K_HYBRID:
            n_gt = -(-sc.model(c.model_key).G // sc.TILE_STATES[c.kernel])
            assert c.max_blocks in (1, 3, 3 * n_gt - 1) and c.grid() == c.max_blocks
            # the stride: some workgroup scores a tile and then, a step `tile += gridDim.x` on, another (the kernels' skew, from jd_gmm.h)
            n_rt, scored = 3, set(c.scored_tiles())
            per_wg = [sum(((t + t // n_rt) % n_rt) * c.h in scored for t in range(b, n_rt * n_gt, c.grid())) for b in range(c.grid())]
            assert max(per_wg) >= 2, c.id
        elif c.max_blocks:
            assert c.grid() == -(-c.n_rows * sc.N_PHONES // 256) > c.max_blocks            # the hybrid kernel: no bound
    # the random models: every D with every G
    keys = {c.model_key for c in CASES}
    assert {"synth%d_%d" % (D, G) for D in sc.SYNTH_DIMS for G in sc.SYNTH_G} <= keys and {"crafted39", "hybrid"} <= keys
    assert sc.model("synth65_150").am.n_mix.max() > 8 and sc.model("synth65_150").am.n_mix.min() == 1      # two blocks of mixtures, ragged


@pytest.mark.parametrize("D", sc.SYNTH_DIMS)
def test_oracle_tables_stand_on_a_second_witness(built, D):
    """the oracle's finite cells against float64 (tests/indep_viterbi_np.gmm_loglik): within four times the deviation measured"""
    worst = 0.0
    for G in sc.SYNTH_G:
        dev, n_fin = sc.f64_deviation("synth%d_%d" % (D, G))
        print("D %d G %d: %d finite cells, largest relative deviation from float64 %.3e" % (D, G, n_fin, dev))
        assert n_fin == (sc.N_FRAMES - 1) * G                          # every cell but the NaN frame's
        worst = max(worst, dev)
    print("D %d: measured %.3e, recorded %.3e, bound %.3e" % (D, worst, sc.F64_MEASURED[D], sc.F64_BOUND[D]))
    assert sc.F64_BOUND[D] == 4.0 * sc.F64_MEASURED[D] and sc.F64_BOUND[D] < 1e-5
    assert worst <= sc.F64_BOUND[D]


def test_check_buffer_bites():
    """check_buffer on made-up buffers: the expected one passes; a touched guard cell, a value cell left alone, and a value off by
    one float do not"""
    class _M:
        G = 3

        @staticmethod
        def oracle_table():
            return np.arange(sc.N_FRAMES * 3, dtype=np.float32).reshape(sc.N_FRAMES, 3) - 50.0
    case = sc.Case("made-up", "made-up", sc.K_GENERIC, np.asarray([1, 2, -1, 1] + [-1] * 64 + [4], np.int32), skip_unused=1, unspec_cap=1.0)
    real = sc.model
    sc.model = lambda key: _M if key == "made-up" else real(key)
    try:
        cls, want = case.classify()
        good = np.where(cls == VALUE, want, case.prefill())
        good[cls == UNSPEC] = 0.0
        assert sc.check_buffer(case, good, 1e-4)
        gr = case.guard_rows
        for r, g, v in ((0, 0, 1.0), (gr - 1, 2, good[gr, 2]), (gr + 64, 1, 0.0), (gr + 69, 0, -1.0)):       # guards and the skipped tile
            bad = good.copy()
            bad[r, g] = v
            with pytest.raises(AssertionError, match="nothing must be written"):
                sc.check_buffer(case, bad, 1e-4)
        bad = good.copy()
        bad[gr + 1, 1] = case.prefill()[gr + 1, 1]
        with pytest.raises(AssertionError, match="never written"):
            sc.check_buffer(case, bad, 1e-4)
        bad = good.copy()
        bad[gr + 1, 1] = np.nextafter(bad[gr + 1, 1], np.float32(0))
        with pytest.raises(AssertionError, match="differs from the oracle"):
            sc.check_buffer(case, bad, 1e-4)
        bad = good.copy()
        bad[gr + 2, 0] = 123.0                                          # an unused row of a scored tile: anything goes
        assert sc.check_buffer(case, bad, 1e-4)
    finally:
        sc.model = real


def test_bad_arguments_are_refused_on_the_host(built):
    """JD_EINVAL for whatever breaks a kernel's precondition, before a device is asked for (device 99: JD_ENODEV would say it was)"""
    from juicer_amd import capi
    m = sc.model("crafted39")
    gam = m.gpu_models()
    gen = sc.model("synth13_17").gpu_models()
    x13 = sc.model("synth13_17").frames

    def refused(models, frames, src, G, what, **kw):
        out = np.zeros((len(src) + 2 * kw.get("guard_rows", 0), G), np.float32)
        with pytest.raises(capi.JuicerAmdError) as e:
            capi.debug_score_rows(models, frames, np.asarray(src, np.int32), out, device=99, **kw)
        assert e.value.code == capi.JD_EINVAL and what in str(e.value), str(e.value)

    ok = list(range(40)) * 8                                           # 320 rows
    refused(gam, m.frames, [0, 40, 1], 150, "row_src[1]")
    refused(gam, m.frames, [0, -2, 1], 150, "row_src[1]")
    # skip_unused: a used row behind an unused one of its tile - in the first tile, and in a listed one; not where nothing is skipped
    holes = list(ok)
    holes[130] = -1
    refused(gam, m.frames, holes, 150, "behind an unused row", skip_unused=1)
    refused(gam, m.frames, holes, 150, "behind an unused row", skip_unused=1, rt_base=[128], used_row_tiles=1)
    refused(gam, m.frames, [-1] + ok[1:], 150, "behind an unused row", skip_unused=1)
    refused(gen, x13, [0] * 64 + [1, -1, 2], 17, "behind an unused row", skip_unused=1)            # the generic kernel's tiles: 64 rows
    # tile lists
    refused(gam, m.frames, ok, 150, "rt_base[1]", rt_base=[0, 320])
    refused(gam, m.frames, ok, 150, "rt_base[0]", rt_base=[-128])
    refused(gam, m.frames, ok, 150, "overlap", rt_base=[128, 0, 255])
    refused(gam, m.frames, ok, 150, "overlap", rt_base=[128, 128])
    refused(gam, m.frames, ok, 150, "overlap", rt_base=[0, 100], mode=capi.SCORE_FAST)
    refused(gam, m.frames, ok, 150, "bad argument", max_blocks=-1)
    refused(gam, m.frames, ok, 150, "mode", mode=2)
    hyb = sc.model("hybrid")
    refused(hyb.gpu_models(), hyb.frames, ok, sc.N_PHONES, "not for hybrid models", rt_base=[0])
    # ... and what passes these checks goes on to ask for the device
    out = np.zeros((320, 150), np.float32)
    with pytest.raises(capi.JuicerAmdError) as e:
        capi.debug_score_rows(gam, m.frames, np.asarray(holes, np.int32), out, device=99, rt_base=[0, 192])
    assert e.value.code == capi.JD_ENODEV
