"""Cases for the histogram pruning of the search kernels (tests/test_hist_cpu.py, tests/test_gpu_hist.py).

The reference prunes with a histogram of the emitting tokens' scores (Histogram.cpp): addScore puts a score in bin
(int)(s -/+ 0.5) - minScore (half away from zero), and calcThresh returns the low edge of the highest bin at which the
count from the top reaches maxN.  Random scores never land on the edges where a kernel would go wrong (exact halves, a
cumulative count equal to max_hyps, a total equal to max_hyps), so the cases here are built on them."""
import numpy as np

HIST_MAX = 201                    # (int)(200.0f + 1.0), whatever the main beam
ULPS = 8


def hist_geometry(main_beam):
    """(hist_min, hist_max, nb) as jd_dec_create computes them (WFSTDecoderLite.cpp:76-82, Histogram.cpp:29-37)."""
    mb = np.float32(main_beam)
    mn = np.float32(-np.float64(mb) - 800.0) if mb > 0 else np.float32(-1000.0)
    hist_min = int(np.float64(mn) - 1.0)           # C's (int) truncates toward zero, as int() does
    return hist_min, HIST_MAX, HIST_MAX - hist_min + 1


def legal_nbs():
    """Every bin count a main beam in (0, 1000] gives (contiguous; checked), and the edges of one wave's 64 lanes."""
    beams = np.concatenate([np.float32([1e-30, 1e-6, 999.9999, 1000.0]), np.arange(1, 4000 * 4 + 1, dtype=np.float64) / 16.0])
    beams = beams[(beams > 0) & (beams <= 1000)]
    nbs = sorted({hist_geometry(b)[2] for b in beams})
    assert nbs == list(range(nbs[0], nbs[-1] + 1)) and nbs[0] == 1003 and nbs[-1] == 2003, (nbs[0], nbs[-1])
    assert hist_geometry(0.0)[2] in nbs
    return nbs + [1, 63, 64, 65, 2048]


# ------------------------------------------------------------------------------------------------ addScore's bin

def addscore_bin(s, hist_min, hist_max):
    """Histogram::addScore :72-80 restated: sc = (int)(s - 0.5) if s < 0 else (int)(s + 0.5), in double; -1 below minScore
    (not counted), -5 above maxScore (the reference's fatal error)."""
    d = np.asarray(s, np.float32).astype(np.float64)
    sc = np.trunc(np.where(d < 0.0, d - 0.5, d + 0.5)).astype(np.int64)
    return np.where(sc > hist_max, -5, np.where(sc < hist_min, -1, sc - hist_min)).astype(np.int32)


def _around(x, ulps=ULPS):
    """every float32 within ulps ulp of each of x (float32), x included"""
    x = np.asarray(x, np.float32)
    up, down = [x], [x]
    for _ in range(ulps):
        up.append(np.nextafter(up[-1], np.float32(np.inf)))
        down.append(np.nextafter(down[-1], np.float32(-np.inf)))
    return np.concatenate(up + down[1:])


def bin_edge_scores(hist_min, hist_max):
    """every float within 8 ulp of every k + 0.5 and every integer k in [hist_min - 2, hist_max + 2] (of both signs of
    zero), subnormals and hist_min / hist_max themselves"""
    k = np.arange(hist_min - 2, hist_max + 3, dtype=np.float64)
    centres = np.concatenate([k, k + 0.5, k - 0.5]).astype(np.float32)
    sub = np.float32([1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38])
    special = np.concatenate([sub, -sub, np.float32([0.0, -0.0, hist_min, hist_max, hist_min - 0.5, hist_max + 0.5])])
    out = np.unique(np.concatenate([_around(centres), special]))
    return np.concatenate([out, np.float32([-0.0])])           # (np.unique folds -0 into +0)


def random_scores(n=10_000_000, seed=2026):
    return np.random.default_rng(seed).uniform(-1300.0, 300.0, n).astype(np.float32)


BIN_RANGES = [hist_geometry(b)[:2] for b in (0.0, 1e-6, 150.0, 1000.0)]    # the default -1001, and nb 1003 / 1153 / 2003


# ------------------------------------------------------------------------------------------------ calcThresh

def calc_thresh(bins, max_hyps, hist_min):
    """Histogram::calcThresh :134-158 restated for one bin array and many maxN: count <= maxN keeps everything (the low edge
    of bin 0), else the low edge of the highest bin i at which the count of bins i .. nb - 1 reaches maxN."""
    bins = np.asarray(bins, np.int64)
    m = np.asarray(max_hyps, np.int64)
    suffix = np.cumsum(bins[::-1])                              # suffix[j] = count of bins nb - 1 - j .. nb - 1
    j = np.searchsorted(suffix, m, side="left")                 # the first j (from the top) where it reaches maxN
    i = bins.shape[0] - 1 - np.minimum(j, bins.shape[0] - 1)
    i = np.where(suffix[-1] <= m, 0, i)
    return (i + hist_min - 0.5).astype(np.float32)


def bin_patterns(nb, rng):
    """dense (every bin counted), sparse, everything in the lowest bin, everything in the highest, nothing"""
    dense = rng.integers(1, 4, nb)
    sparse = np.zeros(nb, np.int64)
    pick = rng.choice(nb, max(1, nb // 50), replace=False)
    sparse[pick] = rng.integers(1, 40, pick.shape[0])
    low = np.zeros(nb, np.int64)
    low[0] = 37
    high = np.zeros(nb, np.int64)
    high[-1] = 41
    return {"dense": dense, "sparse": sparse, "lowest": low, "highest": high, "empty": np.zeros(nb, np.int64)}


def chunk_edges(nb):
    """the first and the last bin (in the scan from the top) of each lane's chunk of K = ceil(nb / 64) bins"""
    K = (nb + 63) // 64
    tops = nb - 1 - K * np.arange(64)
    tops = tops[tops >= 0]
    return np.unique(np.concatenate([tops, np.maximum(tops - (K - 1), 0)]))


def max_hyps_cases(bins, all_bins=False):
    """max_hyps at the cumulative count c_i of the chunk edges' bins (all bins with all_bins) and c_i +- 1, and at the
    total - 1, total, total + 1 - only the kernels' domain, max_hyps >= 1"""
    nb = bins.shape[0]
    suffix = np.cumsum(bins[::-1])[::-1]                        # suffix[i] = c_i, the count of bins i .. nb - 1
    idx = np.arange(nb) if all_bins else chunk_edges(nb)
    c = suffix[idx]
    total = int(suffix[0])
    m = np.unique(np.concatenate([c - 1, c, c + 1, [total - 1, total, total + 1, 1]]))
    return m[m >= 1].astype(np.int32)


FULL_NBS = (1, 63, 64, 65, 1003, 1203, 2003, 2048)              # every c_i here; chunk edges only for the others


def threshold_groups(nb, seed=7):
    """[(pattern, bins of nb, its max_hyps cases)] of one nb"""
    rng = np.random.default_rng(seed * 4096 + nb)
    return [(name, b, max_hyps_cases(b, all_bins=nb in FULL_NBS)) for name, b in bin_patterns(nb, rng).items()]


def stack_groups(groups, hist_min):
    """the groups as one call's cases: (bins n_cases x nb, max_hyps, pattern names, the restatement's thresholds)"""
    nb = groups[0][1].shape[0]
    bins = np.concatenate([np.broadcast_to(b.astype(np.int32), (m.shape[0], nb)) for _, b, m in groups])
    m = np.concatenate([m for _, _, m in groups])
    names = np.concatenate([np.full(m.shape[0], name) for name, _, m in groups])
    want = np.concatenate([calc_thresh(b, m, hist_min) for _, b, m in groups])
    return bins, m, names, want


def first_mismatch(got, want, what):
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    if bad.size == 0:
        return None
    i = bad[0]
    return "%d of %d differ; first: %s -> got %r, want %r" % (bad.size, got.shape[0], what(i), got[i], want[i])
