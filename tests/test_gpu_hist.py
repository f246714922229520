"""The histogram pruning on the device (tests/test_hist_cpu.py holds the host twin and the oracle to the same cases):
jd_hist_bin, which k_search and the slot kernels call for every emitting token, and hist_threshold, their one-wave
Histogram::calcThresh (64 lanes x K bins, a prefix sum, a ballot), both against the CPU oracle and a restatement.

The thresholds are taken at every nb a legal main beam gives and at 1, 63, 64, 65 and 2048 bins, with max_hyps on the
cumulative count at the first and the last bin of every lane's chunk (every bin for some nb), one either side, and at the
total and one either side - the equality cases a decode reaches only by chance."""
import numpy as np
import pytest

from hist_cases import (BIN_RANGES, FULL_NBS, addscore_bin, bin_edge_scores, first_mismatch, legal_nbs, random_scores,
                        stack_groups, threshold_groups)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rng_", BIN_RANGES, ids=lambda r: "min%d" % r[0])
def test_device_hist_bin_edges(built, rng_):
    from juicer_amd import capi
    hist_min, hist_max = rng_
    s = bin_edge_scores(hist_min, hist_max)
    want = addscore_bin(s, hist_min, hist_max)                          # (= the oracle's: tests/test_hist_cpu.py)
    got = capi.debug_hist_bin(s, hist_min, hist_max, 0)
    assert first_mismatch(got, want, lambda i: "device s=%r (%s)" % (s[i], s[i].view(np.int32))) is None


def test_device_hist_bin_random(built):
    from juicer_amd import capi
    hist_min, hist_max = BIN_RANGES[0]
    s = random_scores()
    want = addscore_bin(s, hist_min, hist_max)
    assert first_mismatch(capi.debug_hist_bin(s, hist_min, hist_max, 0), want, lambda i: "device s=%r" % s[i]) is None


def test_device_hist_threshold_every_nb(built):
    from juicer_amd import capi
    n = 0
    for nb in legal_nbs():
        hist_min = 201 - nb + 1
        bins, m, names, want = stack_groups(threshold_groups(nb), hist_min)    # (the restatement = the oracle: tests/test_hist_cpu.py)
        got = capi.debug_hist_threshold(bins, m, hist_min, 0)
        assert first_mismatch(got, want, lambda i: "device nb %d %s max_hyps %d" % (nb, names[i], m[i])) is None
        n += m.shape[0]
    assert n > 400_000


@pytest.mark.parametrize("nb", FULL_NBS)
def test_device_hist_threshold_single_counts(built, nb):
    """one token in each bin on its own, and two in adjacent bins, with max_hyps 1 and 2: the crossing lands on every bin
    of every lane's chunk in turn"""
    from juicer_amd import capi
    from oracle.oracle import hist_thresh_array
    hist_min = -7
    eye = np.eye(nb, dtype=np.int32)
    pairs = eye + np.roll(eye, 1, axis=1)
    bins = np.concatenate([eye, eye, pairs, pairs, pairs])
    m = np.concatenate([np.full(nb, 1), np.full(nb, 2), np.full(nb, 1), np.full(nb, 2), np.full(nb, 3)]).astype(np.int32)
    want = hist_thresh_array(bins, m, hist_min)
    got = capi.debug_hist_threshold(bins, m, hist_min, 0)
    assert first_mismatch(got, want, lambda i: "case %d max_hyps %d bins %s" % (i, m[i], np.flatnonzero(bins[i]))) is None


def test_device_hist_threshold_rejects_bad_arguments(built):
    from juicer_amd import capi
    ok = np.ones((2, 64), np.int32)
    for bins, m in ((ok, np.int32([1, 0])), (np.ones((1, 2049), np.int32), np.int32([1])), (-ok, np.int32([1, 1]))):
        with pytest.raises(capi.JuicerAmdError):
            capi.debug_hist_threshold(bins, m, 0, 0)
    with pytest.raises(capi.JuicerAmdError):
        capi.debug_hist_threshold(ok, np.int32([1, 1]), 0, -1)              # no host twin

    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 31, -(2.0 ** 31)):           # outside the domain where (int) is defined
        with pytest.raises(capi.JuicerAmdError):
            capi.debug_hist_bin(np.float32([1.0, bad]), -10, 10, 0)
