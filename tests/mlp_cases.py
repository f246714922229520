"""Neural acoustic models (csrc/jd_mlp.h): the forward pass restated with libm's OWN fmaf, expf and log (ctypes on libm.so.6 - Python
3.10 has no math.fma and numpy has none), logAdd restated the way tests/logadd_cases.py describes it, the JMLP file and the packed
weights restated from the header's text, and the networks and rows the CPU and GPU tests share."""
import ctypes as C
import struct

import numpy as np

LINEAR, RELU, SIGMOID = 0, 1, 2
LZ = np.float32(-3.4028234663852886e38)
MAX_DIM, MAX_LAYERS, ROWS = 1024, 16, 16                  # jd_mlp.h: the limits and the kernel's row tile

_m = C.CDLL("libm.so.6")
_m.fmaf.restype = C.c_float
_m.fmaf.argtypes = [C.c_float] * 3
_m.expf.restype = C.c_float
_m.expf.argtypes = [C.c_float]
_m.log.restype = C.c_double
_m.log.argtypes = [C.c_double]
_m.logf.restype = C.c_float
_m.logf.argtypes = [C.c_float]


def fmaf(a, b, c):
    return np.float32(_m.fmaf(float(a), float(b), float(c)))


def expf(x):
    return np.float32(_m.expf(float(x)))


def log_priors(p):
    """HTKModels.cpp:183: log(float), libm's logf (numpy's float32 log is another implementation)"""
    return np.array([_m.logf(float(v)) for v in np.asarray(p, np.float32)], np.float32)


def log_add(a, c):
    """HTKFlatModels::logAdd (HTKFlatModels.cpp:266-293): max + log(1.0 + expf(min - max)), the log in double, rounded once; the
    maximum itself when the difference is below -18.42 (a double compare)"""
    a, c = np.float32(a), np.float32(c)
    x, y = (c, a) if a < c else (a, c)
    with np.errstate(all="ignore"):
        d = np.float32(y - x)
    if float(d) < -18.42:
        return x
    if np.isnan(d):
        return d
    return np.float32(float(x) + _m.log(1.0 + float(expf(d))))


def forward_row(layers, x, stop_layer=-1, log_prior=None):
    """layers [(w [out, in], b [out], act)]; stop_layer >= 0: the activations behind it (raw logits for the last); -1: the log
    posteriors, or the hybrid scores when log_prior is given"""
    cur = [np.float32(v) for v in x]
    n = len(layers)
    for l, (w, b, act) in enumerate(layers):
        nxt = []
        for j in range(w.shape[0]):
            y = np.float32(b[j])
            for k in range(w.shape[1]):
                y = fmaf(cur[k], w[j, k], y)
            if l < n - 1:
                if act == RELU:
                    y = y if y > 0 else np.float32(0.0)
                elif act == SIGMOID:
                    with np.errstate(all="ignore"):
                        y = np.float32(np.float32(1.0) / np.float32(np.float32(1.0) + expf(np.float32(-y))))
            nxt.append(y)
        cur = nxt
        if l == stop_layer:
            return np.array(cur, np.float32)
    lz = LZ
    for z in cur:
        lz = log_add(lz, z)
    with np.errstate(all="ignore"):
        out = [np.float32(z - lz) for z in cur]
        if log_prior is not None:
            out = [np.float32(v - p) for v, p in zip(out, log_prior)]
    return np.array(out, np.float32)


def forward(layers, x, stop_layer=-1, log_prior=None):
    return np.stack([forward_row(layers, r, stop_layer, log_prior) for r in np.asarray(x, np.float32)])


def forward_f64(layers, x):
    """the same network in float64 with a true log-sum-exp: what the f32 contract costs is measured against this"""
    a = np.asarray(x, np.float64)
    n = len(layers)
    for l, (w, b, act) in enumerate(layers):
        a = a @ w.astype(np.float64).T + b.astype(np.float64)
        if l < n - 1:
            if act == RELU:
                a = np.maximum(a, 0.0)
            elif act == SIGMOID:
                a = 1.0 / (1.0 + np.exp(-a))
    m = a.max(axis=1, keepdims=True)
    return a - (m + np.log(np.exp(a - m).sum(axis=1, keepdims=True)))


def same_floats(a, b):
    """bit for bit, except that any NaN equals any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def random_net(seed, in_dim, widths, acts, scale=1.0):
    """weights ~ N(0, scale / sqrt(K)), biases ~ N(0, 0.5); acts: one per HIDDEN layer"""
    rng = np.random.default_rng(seed)
    layers, k = [], in_dim
    for l, n in enumerate(widths):
        w = (rng.standard_normal((n, k)) * scale / np.sqrt(k)).astype(np.float32)
        b = (rng.standard_normal(n) * 0.5).astype(np.float32)
        layers.append((w, b, acts[l] if l < len(widths) - 1 else LINEAR))
        k = n
    return layers


def random_rows(seed, n, in_dim):
    return np.random.default_rng(seed + 77).standard_normal((n, in_dim)).astype(np.float32)


def priors(seed, n):
    p = np.random.default_rng(seed + 5).uniform(0.5, 2.0, n)
    return (p / p.sum()).astype(np.float32)


def small_shapes():
    """(in_dim, widths, acts): in_dim in {1, 2, 33}, widths in {1, 31, 32, 33}, 1 to 3 layers, every activation"""
    out = []
    acts = (LINEAR, RELU, SIGMOID)
    i = 0
    for in_dim in (1, 2, 33):
        for wlast in (1, 31, 32, 33):
            for n_layers in (1, 2, 3):
                hidden = [(31, 32, 33, 1)[(i + h) % 4] for h in range(n_layers - 1)]
                out.append((in_dim, hidden + [wlast], [acts[(i + h) % 3] for h in range(n_layers - 1)]))
                i += 1
    return out


# ---- crafted rows: (name, layers, rows, expected, what) with `what` = -1 (log posteriors) or a layer; expected entries None = NaN
def crafted():
    f = np.float32
    cs = []
    # chain order: products 2^24, 1, -2^24 in that k order from bias 0 give 0 (2^24 + 1 rounds back to 2^24); any other order gives 1
    w = np.array([[2.0 ** 24, 1.0, -(2.0 ** 24)]], f)
    cs.append(("chain order", [(w, np.zeros(1, f), LINEAR)], np.ones((1, 3), f), np.array([[0.0]], f), 0))
    # fusion: x w = (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 exactly; minus (1 + 2^-11) it is 2^-24 fused, 0 when the product is rounded first
    v = f(1.0 + 2.0 ** -12)
    cs.append(("fusion", [(np.array([[v]], f), np.array([-(1.0 + 2.0 ** -11)], f), LINEAR)], np.array([[v]], f), np.array([[2.0 ** -24]], f), 0))
    # a sigmoid whose expf overflows: expf(100) = inf, 1 / (1 + inf) = 0; and one at the other end: expf(-200) = 0, 1 / 1 = 1
    sg = [(np.array([[1.0], [1.0]], f), np.zeros(2, f), SIGMOID), (np.eye(2, dtype=f), np.zeros(2, f), LINEAR)]
    cs.append(("sigmoid overflow", sg, np.array([[-100.0], [200.0]], f), np.array([[0.0, 0.0], [1.0, 1.0]], f), 0))
    # the logAdd cut: logits 0 and -19 are more than 18.42 apart, so logZ is 0 exactly and the log posteriors are the logits;
    # at -18 they are not: logZ = (float)(0.0 + log(1.0 + expf(-18))) (that row's expectation is computed, not a literal)
    cut = [(np.array([[1.0], [0.0]], f), np.zeros(2, f), LINEAR)]
    lz18 = np.float32(_m.log(1.0 + float(expf(f(-18.0)))))
    cs.append(("logAdd cut", cut, np.array([[-19.0], [19.0], [-18.0]], f),
               np.array([[-19.0, 0.0], [0.0, -19.0], [f(-18.0) - lz18, f(0.0) - lz18]], f), -1))
    # a NaN input row is NaN in that row and nowhere else
    nn = [(np.array([[1.0, 2.0], [3.0, -1.0]], f), np.zeros(2, f), SIGMOID), (np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], f), np.zeros(3, f), LINEAR)]
    x = np.array([[0.0, 0.0], [np.nan, 1.0], [0.0, 0.0]], f)
    cs.append(("NaN row", nn, x, np.array([[0.5, 0.5, 1.0], [np.nan] * 3, [0.5, 0.5, 1.0]], f), 1))
    return cs


# ---- the JMLP file and the packed weights, from the text of jd_mlp.h
def jmlp_bytes(priors_, states_per_model, layers, version=1, magic=b"JMLP"):
    n = len(layers)
    out = magic + struct.pack("<I", version)
    out += struct.pack("<4i", len(priors_), states_per_model, layers[0][0].shape[1], n)
    out += struct.pack("<%di" % n, *[l[0].shape[0] for l in layers])
    out += struct.pack("<%di" % n, *([int(l[2]) for l in layers[:-1]] + [0]))
    out += np.asarray(priors_, "<f4").tobytes()
    for w, b, _ in layers:
        out += np.ascontiguousarray(w, "<f4").tobytes() + np.asarray(b, "<f4").tobytes()
    return out


def pad16(n):
    return (n + 15) // 16 * 16


def packed(layers):
    """(weights, biases) as jd_mlp_pack lays them out: w_off[l] + (((j / 16) (Kp / 16) + k / 16) 64 + ((k % 4) 16 + j % 16)) 4 + (k % 16) / 4"""
    wp, bp = [], []
    for w, b, _ in layers:
        N, K = w.shape
        Np, Kp = pad16(N), pad16(K)
        t = np.zeros(Np * Kp, np.float32)
        j, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
        t[(((j // 16) * (Kp // 16) + k // 16) * 64 + ((k % 4) * 16 + j % 16)) * 4 + (k % 16) // 4] = w
        wp.append(t)
        bb = np.zeros(Np, np.float32)
        bb[:N] = b
        bp.append(bb)
    return np.concatenate(wp), np.concatenate(bp)


# ---- the decoding case: synth.config_hybrid's log-posterior vectors as INPUT FEATURES (in_dim = n_phones) of a network that
# passes them through a ReLU pair plus seeded noise, so that the spoken phone stays favoured
DECODE_NOISE = 0.05


def decode_net(n_phones, seed, noise=DECODE_NOISE):
    """W1 = [I; -I] + noise N with ReLU, W2 = [I, -I] + noise N, no biases"""
    rng = np.random.default_rng(seed)
    eye = np.eye(n_phones)
    w1 = (np.vstack([eye, -eye]) + noise * rng.standard_normal((2 * n_phones, n_phones))).astype(np.float32)
    w2 = (np.hstack([eye, -eye]) + noise * rng.standard_normal((n_phones, 2 * n_phones))).astype(np.float32)
    return [(w1, np.zeros(2 * n_phones, np.float32), RELU), (w2, np.zeros(n_phones, np.float32), LINEAR)]


DECODE_BEAMS = (dict(main_beam=200.0), dict(main_beam=150.0, max_hyps=100))


# ---- shapes that straddle the kernel's tiles (16 rows; k groups of 16 inputs; n tiles of 16 outputs taken in pairs, eight tiles
# per turn of a workgroup's four waves, so a ninth and a seventeenth tile start another turn): (in_dim, widths, acts)
def tile_shapes():
    return [
        (15, [15, 15], [SIGMOID]), (16, [16, 16], [RELU]), (17, [17, 17], [SIGMOID]),
        (31, [31, 33], [LINEAR]), (32, [32, 31], [SIGMOID]), (33, [33, 32], [RELU]),
        (47, [127, 129, 45], [SIGMOID, RELU]), (64, [128, 143, 144], [RELU, SIGMOID]), (5, [145, 257, 7], [SIGMOID, SIGMOID]),
    ]


def limit_shapes():
    """one case at each stated limit: the widest input, the widest layer (hidden and last), the most layers"""
    return [
        (MAX_DIM, [9], []), (7, [MAX_DIM, 5], [SIGMOID]), (3, [MAX_DIM], []), (MAX_DIM, [MAX_DIM, MAX_DIM], [RELU]),
        (6, [9, 8, 7, 9, 8, 7, 9, 8, 7, 9, 8, 7, 9, 8, 7, 6], [SIGMOID, RELU, LINEAR] * 5),
    ]


TILE_ROWS = (1, ROWS - 1, ROWS, ROWS + 1, 4 * ROWS + 1)
