"""logAdd on the device: the primitives of csrc/jd_gmm.h against the host libm and the CPU oracle (tests/test_logadd.py holds
their host twins to the same), then likelihood tables whose cells are CHOSEN - models from prepared arrays (capi.Models.from_flat /
OracleAM.from_flat) scored on frames equal to the means, so that every component's value is its det exactly - through the real
kernels: jd_gmm_kernel39 on both tile widths, the generic jd_gmm_kernel at other D, and jd_gmm_fast39 within its tolerance."""
import numpy as np
import pytest

from logadd_cases import (INF, LZ, cancellation_pairs, d_chunks, divergent_pairs, edge_pairs, first_difference, random_pairs,
                          same_floats)
from logadd_cases import crafted_model as _crafted_model, table_frames as _frames      # (shared with tests/score_rows_cases.py)

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
