"""Inputs of HTKFlatModels::logAdd (HTKFlatModels.cpp:266-293) where an implementation goes wrong, shared by
tests/test_logadd.py (host twins) and tests/test_gpu_logadd.py (the device).  logAdd(x, y) = max + log(1.0 + expf(d)),
d = min - max, log in double, x returned when d < -18.42 (a double compare)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LZ = np.float32(-3.4028234663852886e38)                  # Torch3 LOG_ZERO = -FLT_MAX
CUT = np.float32(-18.42)                                  # the float nearest the cut: below it (-18.4200000763 < -18.42)
INF, NAN = np.float32(np.inf), np.float32(np.nan)

# (x, y, the reference's logAdd): pairs whose float result the libm's last double bits decide - a table-and-polynomial
# log(1 + e) within 1-2 ulp of the libm's gives the neighbouring float on them
DIVERGENT = [
    ("-0x1p-4", "-0x1.66df2cp+1", "-0x1.3aaed6p-21"),
    ("-0x1.000002p-4", "-0x1.66df2cp+1", "-0x1.3eaed6p-21"),
    ("-0x1.00c0e4p-3", "-0x1.11bb68p+1", "-0x1.439588p-33"),
]


def f32(h):
    return np.float32(float.fromhex(h))


def divergent_pairs():
    x = np.array([f32(a) for a, _, _ in DIVERGENT] + [f32(b) for _, b, _ in DIVERGENT], np.float32)
    y = np.array([f32(b) for _, b, _ in DIVERGENT] + [f32(a) for a, _, _ in DIVERGENT], np.float32)
    want = np.array([f32(c) for _, _, c in DIVERGENT] * 2, np.float32)
    return x, y, want


def all_d():
    """every float d in [-18.42, 0]: -0.0 up to the cut's float (bit patterns of negative floats grow with the magnitude), and +0.0"""
    a = int(np.float32(-0.0).view(np.uint32))
    b = int(CUT.view(np.uint32))
    return a, b


def d_chunks(n_chunks=128):
    a, b = all_d()
    edges = np.linspace(a, b + 1, n_chunks + 1).astype(np.int64)
    for i in range(n_chunks):
        yield np.arange(edges[i], edges[i + 1], dtype=np.uint32).view(np.float32)
    yield np.array([0.0], np.float32)


def pool_map(fn, items, workers=None):
    """fn over items on a thread pool (the ctypes calls drop the GIL): the exhaustive checks on all cores"""
    workers = workers or min(8, os.cpu_count() or 1)
    with ThreadPoolExecutor(workers) as ex:
        return list(ex.map(fn, items))


def cancellation_pairs(per_binade=4096, window=64, seed=0):
    """x in every binade of [-1, -2^-20] (both ends and random floats between), y within `window` floats of the y at which
    logAdd(x, y) crosses 0 (y0 = log(1 - exp(x))): the results are near 0, where the last bits of log(1 + e) reach the float.
    Both argument orders."""
    rng = np.random.default_rng(seed)
    xs = []
    for e in range(-20, 0):
        lo, hi = int(np.float32(-(2.0 ** e)).view(np.uint32)), int(np.float32(-(2.0 ** (e + 1))).view(np.uint32))
        xs.append(np.array([lo, hi - 1], np.uint32))
        xs.append(rng.integers(lo, hi, per_binade, dtype=np.uint32))
    x = np.concatenate(xs).view(np.float32)
    y0 = np.log(-np.expm1(x.astype(np.float64))).astype(np.float32)
    # floats around y0 (negative: bit patterns grow with the magnitude)
    off = np.arange(-window, window + 1, dtype=np.int64)
    yy = (y0.view(np.uint32).astype(np.int64)[:, None] + off[None, :]).astype(np.uint32).view(np.float32)
    xx = np.broadcast_to(x[:, None], yy.shape)
    x1, y1 = xx.ravel().copy(), yy.ravel().copy()
    return np.concatenate([x1, y1]), np.concatenate([y1, x1])


def edge_pairs():
    """the cut (d at the cut's float, one float either side), d = 0, LOG_ZERO, +-inf and NaN operands, signed zeros"""
    below, above = np.nextafter(CUT, np.float32(-np.inf)), np.nextafter(CUT, np.float32(0))
    xs, ys = [], []
    for x in np.float32([0.0, -0.0, 1.0, -1.0, 0.5, -2.75, 37.5, -60.0, -1024.0, 4096.0]):
        for d in (below, CUT, above, np.float32(-18.0), np.float32(-1e-7), np.float32(-0.0), np.float32(0.0)):
            y = np.float32(x + d)
            xs += [x, y]
            ys += [y, x]
    v = np.float32([0.0, -1.5, -87.25, 3.0e38, -3.0e38, 1e-30, -1e-42])
    specials = [LZ, np.nextafter(LZ, np.float32(0)), -INF, INF, NAN]
    for a in specials:
        for b in list(specials) + list(v):
            xs += [a, b]
            ys += [b, a]
    return np.array(xs, np.float32), np.array(ys, np.float32)


def random_pairs(n=1 << 20, seed=1):
    """log-likelihood-like operands (what the kernels' tables hold) and pairs close to each other"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-200.0, 10.0, n).astype(np.float32)
    d = -np.abs(rng.standard_normal(n) * 6.0).astype(np.float32)
    return x, (x + d).astype(np.float32)


def same_floats(a, b):
    """bit for bit, except that any NaN equals any NaN (payloads are not part of logAdd's contract)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def first_difference(a, b, x, y):
    na, nb = np.isnan(a), np.isnan(b)
    bad = np.nonzero((na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32))))[0]
    if bad.shape[0] == 0:
        return "none"
    i = bad[0]
    return "%d differ; first: logAdd(%s, %s) = %s, want %s" % (bad.shape[0], float(x[i]).hex(), float(y[i]).hex(),
                                                               float(a[i]).hex(), float(b[i]).hex())


# ---------------------------------------------------------------- crafted likelihood tables (tests/test_gpu_logadd.py, tests/score_rows_cases.py)

M_MAX = 24                                                # > 16: a state longer than the 16-mixture chains of the bench models


def crafted_states(rng):
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


def crafted_model(D, G, seed):
    """det / mean / ivar / n_mix of G states: the crafted ones first, then random ones of every length 1..M_MAX; means 0"""
    rng = np.random.default_rng(seed)
    st = crafted_states(rng)
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


def table_frames(D, R, seed):
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
