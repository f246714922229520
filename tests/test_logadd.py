"""logAdd of the exact scoring kernels (csrc/jd_gmm.h) against the host libm and the CPU oracle, through the host twins
compiled from the same source as the device code (jd_debug_log1pe / jd_debug_log_add, device -1).

HTKFlatModels::logAdd (HTKFlatModels.cpp:266-293) rounds x + log(1.0 + expf(d)) to float; near a result of 0 the last bits
of the double log decide that float.  So the kernels' log(1 + e) must be the libm's bit for bit, for EVERY float d in
[-18.42, 0] - a table value within 1-2 ulp is not enough (DIVERGENT pairs).  The exhaustive checks run on all cores."""
import numpy as np
import pytest

from logadd_cases import (DIVERGENT, d_chunks, divergent_pairs, cancellation_pairs, edge_pairs, random_pairs, pool_map,
                          same_floats, first_difference)


def _libm(d):
    from oracle.oracle import log1pe_array
    return log1pe_array(d)


def test_log1pe_replica_equals_libm_everywhere(built):
    """jd_log_libm_impl (glibc's log as the x86-64 libm runs it) on 1 + expf(d): every double equal to the libm's"""
    from juicer_amd import capi

    def bad(d):
        return d.shape[0], int((capi.debug_log1pe(d, capi.LOG1PE_LIBM).view(np.uint64) != _libm(d).view(np.uint64)).sum())
    res = pool_map(bad, d_chunks())
    assert sum(n for n, _ in res) > 1_100_000_000
    assert sum(b for _, b in res) == 0


def test_log1pe_table_within_two_doubles_of_libm(built):
    """the gate's premise: the table value the kernels round first is within 2 doubles (both positive: 2 bit patterns) of the
    libm's everywhere, so [m - 2 ulp, m + 2 ulp] holds the libm's value.  (It does differ, on tens of millions of d.)"""
    from juicer_amd import capi

    def dist(d):
        m = capi.debug_log1pe(d, capi.LOG1PE_TABLE).view(np.int64)
        lib = _libm(d).view(np.int64)
        assert (lib > 0).all() and (m > 0).all()
        return int(np.abs(m - lib).max()), int((m != lib).sum())
    res = pool_map(dist, d_chunks())
    assert max(w for w, _ in res) <= 2
    assert sum(n for _, n in res) > 1_000_000


@pytest.mark.parametrize("variant", [0, 1], ids=["generic", "pair"])
def test_log_add_divergent_pairs(built, variant):
    from juicer_amd import capi
    from oracle.oracle import log_add_array
    x, y, want = divergent_pairs()
    ref = log_add_array(x, y)
    assert same_floats(ref, want), "the oracle (host libm) itself: %s" % first_difference(ref, want, x, y)
    got = capi.debug_log_add(x, y, variant)
    assert same_floats(got, want), first_difference(got, want, x, y)


@pytest.mark.parametrize("variant", [0, 1], ids=["generic", "pair"])
@pytest.mark.parametrize("cases", ["cancellation", "edges", "random"])
def test_log_add_host_twin_equals_oracle(built, variant, cases):
    from juicer_amd import capi
    from oracle.oracle import log_add_array
    x, y = {"cancellation": cancellation_pairs, "edges": edge_pairs, "random": random_pairs}[cases]()
    parts = list(zip(np.array_split(x, 16), np.array_split(y, 16)))
    got = np.concatenate(pool_map(lambda p: capi.debug_log_add(p[0], p[1], variant), parts))
    want = np.concatenate(pool_map(lambda p: log_add_array(p[0], p[1]), parts))
    assert same_floats(got, want), first_difference(got, want, x, y)
    if cases == "cancellation":
        assert (np.abs(want) < 1e-3).mean() > 0.9           # (the sweep is where it claims to be: results near 0)


def test_log_add_nan_and_infinities_follow_the_oracle(built):
    """NaN operands give NaN (expf / log propagate it); inf - inf gives NaN; an infinite maximum returns itself"""
    from juicer_amd import capi
    from oracle.oracle import log_add_array
    from logadd_cases import INF, LZ, NAN
    x = np.float32([NAN, 1.0, NAN, INF, -INF, INF, 5.0, LZ, -INF])
    y = np.float32([1.0, NAN, LZ, INF, -INF, 5.0, -INF, -INF, LZ])
    want = log_add_array(x, y)
    assert np.isnan(want[:5]).all() and want[5] == INF and want[6] == 5.0 and want[7] == LZ and want[8] == LZ
    for variant in (0, 1):
        got = capi.debug_log_add(x, y, variant)
        assert same_floats(got, want), (variant, first_difference(got, want, x, y))


def test_debug_entries_refuse_what_they_cannot_evaluate(built):
    from juicer_amd import capi
    with pytest.raises(capi.JuicerAmdError, match="outside"):
        capi.debug_log1pe(np.float32([-1.0, 0.5]), capi.LOG1PE_LIBM)
    with pytest.raises(capi.JuicerAmdError, match="outside"):
        capi.debug_log1pe(np.float32([np.nan]), capi.LOG1PE_TABLE)
    with pytest.raises(capi.JuicerAmdError, match="device only"):
        capi.debug_log_add(np.float32([0.0]), np.float32([0.0]), capi.LOGADD_FAST)
    assert len(DIVERGENT) == 3
