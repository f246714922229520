"""logAdd on the device: the primitives of csrc/jd_gmm.h against the host libm and the CPU oracle (tests/test_logadd.py holds
their host twins to the same), then likelihood tables whose cells are CHOSEN - models from prepared arrays (capi.Models.from_flat /
OracleAM.from_flat) scored on frames equal to the means, so that every component's value is its det exactly - through the real
kernels: jd_gmm_kernel39 on both tile widths, the generic jd_gmm_kernel at other D, and jd_gmm_fast39 within its tolerance."""
import numpy as np
import pytest

from logadd_cases import (CUT, INF, LZ, NAN, cancellation_pairs, d_chunks, divergent_pairs, edge_pairs, first_difference,
                          random_pairs, same_floats)

pytestmark = pytest.mark.gpu
RTOL = 1e-4                                               # jd_gmm_fast39's, as tests/test_gpu_fastscore.py holds it


def test_device_log1pe_equals_libm_everywhere(built):
    from juicer_amd import capi
    from oracle.oracle import log1pe_array
    n = bad = wide = 0
    for d in d_chunks():
        lib = log1pe_array(d).view(np.int64)
        bad += int((capi.debug_log1pe(d, capi.LOG1PE_LIBM, 0).view(np.int64) != lib).sum())
        wide = max(wide, int(np.abs(capi.debug_log1pe(d, capi.LOG1PE_TABLE, 0).view(np.int64) - lib).max()))
        n += d.shape[0]
    assert n > 1_100_000_000
    assert bad == 0
    assert wide <= 2                                      # the gate's premise, on the device's own arithmetic


@pytest.mark.parametrize("variant", [0, 1], ids=["generic", "pair"])
@pytest.mark.parametrize("cases", ["divergent", "cancellation", "edges", "random"])
def test_device_log_add_equals_oracle(built, variant, cases):
    from juicer_amd import capi
    from oracle.oracle import log_add_array
    if cases == "divergent":
        x, y, want = divergent_pairs()
        assert same_floats(log_add_array(x, y), want)
    else:
        x, y = {"cancellation": cancellation_pairs, "edges": edge_pairs, "random": random_pairs}[cases]()
        want = log_add_array(x, y)
    got = capi.debug_log_add(x, y, variant, 0)
    assert same_floats(got, want), first_difference(got, want, x, y)


@pytest.mark.parametrize("cases", ["divergent", "cancellation", "edges", "random"])
def test_device_fast_log_add_within_tolerance(built, cases):
    from juicer_amd import capi
    from oracle.oracle import log_add_array
    if cases == "divergent":
        x, y, _ = divergent_pairs()
    else:
        x, y = {"cancellation": cancellation_pairs, "edges": edge_pairs, "random": random_pairs}[cases]()
    want = log_add_array(x, y).astype(np.float64)
    got = capi.debug_log_add(x, y, capi.LOGADD_FAST, 0).astype(np.float64)
    fin = np.isfinite(want)
    assert fin.sum() > 0.5 * fin.shape[0]
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    assert err.max() <= RTOL, (err.max(), first_difference(got[fin].astype(np.float32), want[fin].astype(np.float32), x[fin], y[fin]))


# ---------------------------------------------------------------- crafted tables through the kernels

M_MAX = 24                                                # > 16: a state longer than the 16-mixture chains of the bench models


def _crafted_states(rng):
    """component values (dets) of the states whose cells the test chooses"""
    above, below = np.nextafter(CUT, np.float32(0)), np.nextafter(CUT, np.float32(-INF))
    st = []
    x, y, _ = divergent_pairs()
    st += [[a, b] for a, b in zip(x, y)]                                        # the divergent pairs, both orders
    st += [[0.0, CUT], [0.0, above], [0.0, below], [CUT, 0.0], [above, 0.0],    # d at the cut, one float either side
           [-2.5, -2.5 + CUT], [-2.5 + above, -2.5]]
    st += [[-3.25, -3.25], [0.0, 0.0], [-70.0, -70.0, -70.0], [-1.0] * 17]      # equal components
    st += [[LZ, LZ], [LZ, -5.0], [-5.0, LZ], [LZ, -INF], [-INF, -3.0], [-3.0, -INF], [-INF, -INF], [LZ], [-INF],
           [np.nextafter(LZ, np.float32(0)), LZ]]                               # at or below LOG_ZERO
    st += [[INF, -1.0], [INF, INF], [-1.0, INF]]                                # +inf components: inf, NaN (inf - inf)
    cx, cy = cancellation_pairs(per_binade=8, window=4, seed=7)
    pick = rng.choice(cx.shape[0], 48, replace=False)
    st += [[a, b] for a, b in zip(cx[pick], cy[pick])]                          # results near 0
    st += [list(rng.uniform(-4.0, 0.0, n).astype(np.float32)) for n in (17, 20, M_MAX)]   # long chains, close components
    st += [[0.0], [0.0, 0.0], [0.0] * 5]                                        # det 0: subnormal distances stay visible
    return [np.asarray(s, np.float32) for s in st]


def _crafted_model(D, G, seed):
    """det / mean / ivar / n_mix of G states: the crafted ones first, then random ones of every length 1..M_MAX; means 0"""
    rng = np.random.default_rng(seed)
    st = _crafted_states(rng)
    assert G >= len(st)
    n_mix = np.zeros(G, np.int32)
    det = np.full((G, M_MAX), LZ, np.float32)
    for g in range(G):
        n = 1 + g % (M_MAX if g < 4 * M_MAX else 4)                           # (every length, then short: the oracle's time)
        v = st[g] if g < len(st) else rng.uniform(-60.0, -10.0, n).astype(np.float32)
        n_mix[g] = v.shape[0]
        det[g, :v.shape[0]] = v
    mean = np.zeros((G, M_MAX, D), np.float32)
    ivar = rng.uniform(0.5, 2.0, (G, M_MAX, D)).astype(np.float32)
    return det, mean, ivar, n_mix


def _frames(D, R, seed):
    """rows by kind: 0 the means (every cell its det-made value), 1 random, 2 a NaN feature, 3 a feature whose squared distance
    overflows to inf, 4 every feature 1e-20 (squared distances 1e-40: subnormal; a flushed one would read 0)"""
    rng = np.random.default_rng(seed + 1)
    x = np.zeros((R, D), np.float32)
    for r in range(R):
        k = r % 5
        if k == 1:
            x[r] = rng.normal(0.0, 0.4, D)
        elif k == 2:
            x[r, r % D] = NAN
        elif k == 3:
            x[r, (3 * r) % D] = 1e30
        elif k == 4:
            x[r] = 1e-20
    return x


def _check_table(D, G, R, seed, fast=False):
    from juicer_amd import capi
    from oracle.oracle import OracleAM
    det, mean, ivar, n_mix = _crafted_model(D, G, seed)
    x = _frames(D, R, seed)
    want = OracleAM.from_flat(det, mean, ivar, n_mix).score_frames(x)
    gam = capi.Models.from_flat(det, mean, ivar, n_mix)
    got = gam.score_frames(x)
    bad = np.argwhere(~((np.isnan(got) & np.isnan(want)) | (got.view(np.uint32) == want.view(np.uint32))))
    assert bad.shape[0] == 0, "%d cells differ; first: row %d state %d: %s, oracle %s" % (
        bad.shape[0], bad[0][0], bad[0][1], float(got[tuple(bad[0])]).hex(), float(want[tuple(bad[0])]).hex())
    # the table holds what it was built to hold
    _, _, divergent = divergent_pairs()
    assert same_floats(want[0, :divergent.shape[0]], divergent)
    if R > 2:
        assert np.isnan(want[2]).all()                                      # NaN feature: NaN in every state
    if R > 3:
        assert (want[3, ~(det == INF).any(axis=1)] == LZ).all()           # every distance inf: LOG_ZERO
    if R > 4:
        sub = [g for g in range(G) if n_mix[g] == 1 and det[g, 0] == 0.0][0]
        assert want[4, sub] < 0.0 and want[4, sub] > -np.finfo(np.float32).tiny      # a subnormal cell
    if fast:
        fs = gam.score_frames(x, mode=capi.SCORE_FAST).astype(np.float64)
        w = want.astype(np.float64)
        fin = np.isfinite(w)
        err = np.abs(fs[fin] - w[fin]) / np.maximum(1.0, np.abs(w[fin]))
        assert err.max() <= RTOL, err.max()
    return got


@pytest.mark.parametrize("R", [1, 127, 128, 129])
def test_crafted_table_kernel39_small_tiles(built, R):
    """D = 39, few tiles: jd_gmm_kernel39<GMM_GT_SMALL>; 150 states (not a multiple of 16 or 64)"""
    _check_table(39, 150, R, seed=R, fast=True)


def test_crafted_table_kernel39_wide_tiles(built):
    """D = 39, >= 1024 tiles of 128 rows x 64 states: jd_gmm_kernel39<GMM_GT> (what the decoder's tables run)"""
    G, R = 1043, 60 * 128 + 1
    assert ((R + 127) // 128) * ((G + 63) // 64) >= 1024
    _check_table(39, G, R, seed=5, fast=True)


@pytest.mark.parametrize("D", [1, 13, 40, 64])
@pytest.mark.parametrize("R", [1, 127, 128, 129])
def test_crafted_table_generic_kernel(built, D, R):
    _check_table(D, 131, R, seed=D * 1000 + R)
