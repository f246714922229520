"""The histogram pruning's bin (Histogram::addScore, Histogram.cpp:64-100) as the search kernels compute it, through its host
twin compiled from the same source (jd_debug_hist_bin, device -1), against the CPU oracle and a restatement in numpy; and the
oracle's calcThresh (:134-158), which tests/test_gpu_hist.py holds the kernels' one-wave search to, against its restatement.

Scores from a decode never land on the edges these cases are built on: exact halves (where half away from zero and
round-half-even part), the bins' own edges, a cumulative count equal to max_hyps."""
import numpy as np
import pytest

from hist_cases import (BIN_RANGES, addscore_bin, bin_edge_scores, first_mismatch, hist_geometry, legal_nbs,
                        random_scores, stack_groups, threshold_groups)


def test_geometry_matches_the_host_formula():
    """nb of every legal main beam: the 1001 values 1003 .. 2003; a main beam <= 0 gives hist_min -1001"""
    nbs = legal_nbs()
    assert len(nbs) == 1001 + 5
    assert hist_geometry(0.0) == (-1001, 201, 1203) and hist_geometry(1000.0) == (-1801, 201, 2003)
    assert hist_geometry(1e-30)[0] == -801 and hist_geometry(150.0)[0] == -951


@pytest.mark.parametrize("rng_", BIN_RANGES, ids=lambda r: "min%d" % r[0])
def test_hist_bin_edges_host_twin(built, rng_):
    from juicer_amd import capi
    from oracle.oracle import hist_bin_array
    hist_min, hist_max = rng_
    s = bin_edge_scores(hist_min, hist_max)
    want = addscore_bin(s, hist_min, hist_max)
    # the cases are where they claim to be: every class, and exact halves where round-half-even would part from the reference
    assert (want == capi.HIST_BELOW).any() and (want == capi.JD_EHIST).any() and (want == 0).any() and (want == hist_max - hist_min).any()
    d = s.astype(np.float64)
    assert (np.rint(d) != np.trunc(np.where(d < 0, d - 0.5, d + 0.5))).sum() > (hist_max - hist_min) // 2
    ref = hist_bin_array(s, hist_min, hist_max)
    assert first_mismatch(ref, want, lambda i: "oracle s=%r" % s[i]) is None
    got = capi.debug_hist_bin(s, hist_min, hist_max)
    assert first_mismatch(got, want, lambda i: "host twin s=%r (%s)" % (s[i], s[i].view(np.int32))) is None


def test_hist_bin_random_host_twin(built):
    """10^7 scores over [-1300, 300] at the default range [-1001, 201]"""
    from juicer_amd import capi
    from oracle.oracle import hist_bin_array
    hist_min, hist_max = BIN_RANGES[0]
    s = random_scores()
    want = addscore_bin(s, hist_min, hist_max)
    assert (want == capi.HIST_BELOW).any() and (want == capi.JD_EHIST).any()
    assert first_mismatch(hist_bin_array(s, hist_min, hist_max), want, lambda i: "oracle s=%r" % s[i]) is None
    assert first_mismatch(capi.debug_hist_bin(s, hist_min, hist_max), want, lambda i: "host twin s=%r" % s[i]) is None


def test_hist_bin_rejects_bad_arguments(built):
    from juicer_amd import capi
    with pytest.raises(capi.JuicerAmdError):
        capi.debug_hist_bin(np.zeros(3, np.float32), 5, 4)
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 31, -(2.0 ** 31)):           # outside the domain where (int) is defined
        with pytest.raises(capi.JuicerAmdError):
            capi.debug_hist_bin(np.float32([1.0, bad]), -10, 10)


def test_oracle_calc_thresh_equals_restatement(built):
    """jo_hist_thresh_array against the restatement over every legal nb, bin pattern and max_hyps case"""
    from oracle.oracle import hist_thresh_array
    n = at_total = cut = 0
    for nb in legal_nbs():
        hist_min = 201 - nb + 1
        bins, m, names, want = stack_groups(threshold_groups(nb), hist_min)
        got = hist_thresh_array(bins, m, hist_min)
        assert first_mismatch(got, want, lambda i: "nb %d %s max_hyps %d" % (nb, names[i], m[i])) is None
        at_total += int((bins.sum(axis=1, dtype=np.int64) == m).sum())
        cut += int((got > np.float32(hist_min - 0.5)).sum())
        n += m.shape[0]
    # (the cases are where they claim to be: a total equal to max_hyps keeps everything; most cases cut somewhere)
    assert n > 400_000 and at_total > 1000 and cut > n // 2
