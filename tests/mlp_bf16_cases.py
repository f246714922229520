"""bf16 neural acoustic models (csrc/jd_mlp_bf16.h) restated from the header's text: the rounding on the bits with numpy, the packed
index formula, the host twin as a float64 loop over k ascending (vectorised over the outputs), the device's bound, and the networks
the CPU and GPU tests share.  tests/mlp_cases.py supplies libm's expf, logAdd, the seeded networks and the shapes."""
import numpy as np

import mlp_cases as mc

ROWS, KG, NT = 32, 32, 16                                 # jd_mlp_bf16.h: JD_MLP_BF16_ROWS, JD_MLP_BF16_KG, JD_MLP_BF16_NT
LZ_CHAINS = 128
F32, BF16 = 0, 1
TILE_ROWS = (1, ROWS - 1, ROWS, ROWS + 1, 4 * ROWS + 1)


def bf16_round(x):
    """nearest value with 8 significant bits, ties to even, on the bits: a NaN stays a NaN (quiet bit set), everything else is
    u + 0x7fff + (bit 16 of u), the low 16 bits dropped - the carry runs into the exponent, past the largest into inf"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
    r = np.where(nan, (u >> 16) | 0x40, r)
    return (r.astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def is_bf16(x):
    return not np.any(np.ascontiguousarray(x, np.float32).view(np.uint32) & 0xffff)


def pad32(n):
    return (n + 31) // 32 * 32


def stride_of(in_dim, hidden_widths):
    """the widest of in_dim and the hidden widths padded to the k group, then to 16 modulo 128"""
    w = max([pad32(in_dim)] + [pad32(v) for v in hidden_widths])
    return w + (16 - w % 128) % 128


def packed(layers):
    """(weights as 16-bit patterns, biases) as jd_mlp_bf16_pack lays them out:
    w_off[l] + ((j / 16) (Kp / 32) + k / 32) 512 + (((k % 32) / 8) 16 + j % 16) 8 + k % 8, Kp and Np padded to 32, padding +0"""
    wp, bp = [], []
    for w, b, _ in layers:
        N, K = w.shape
        Np, Kp = pad32(N), pad32(K)
        t = np.zeros(Np * Kp, np.uint16)
        j, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
        t[((j // 16) * (Kp // 32) + k // 32) * 512 + (((k % 32) // 8) * 16 + j % 16) * 8 + k % 8] = (bf16_round(w).view(np.uint32) >> 16).astype(np.uint16)
        wp.append(t)
        bb = np.zeros(Np, np.float32)
        bb[:N] = b
        bp.append(bb)
    return np.concatenate(wp), np.concatenate(bp)


def rounded(layers):
    return [(bf16_round(w), b, a) for w, b, a in layers]


def linear_f64(w, b, xh):
    """(the double sums [n, N] from the bias, k ascending; S = |b| + sum |x w| [n, N]) of bf16 operands xh [n, K] and weights w [N, K]"""
    w64, x64 = bf16_round(w).astype(np.float64), np.asarray(xh, np.float64)
    s = np.repeat(b.astype(np.float64)[None, :], x64.shape[0], axis=0)
    S = np.abs(s)
    for k in range(w64.shape[1]):
        p = x64[:, k:k + 1] * w64[None, :, k]
        s = s + p
        S = S + np.abs(p)
    return s, S


def activate(y, act):
    """jd_mlp_forward_row's RELU / SIGMOID on float32 y [n, N], libm's expf"""
    y = np.asarray(y, np.float32)
    if act == mc.RELU:
        return np.where(y > 0, y, np.float32(0.0)).astype(np.float32)
    if act == mc.SIGMOID:
        with np.errstate(all="ignore"):
            e = np.array([mc.expf(np.float32(-v)) for v in y.ravel()], np.float32).reshape(y.shape)
            return (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float32)
    return y


def logz_row(z, tied):
    """logZ of one row of logits with mlp_cases.log_add: the serial chain, or 128 interleaved chains and the chain of the partials"""
    lz = mc.LZ
    if tied:
        for c in range(min(LZ_CHAINS, len(z))):
            p = mc.LZ
            for v in z[c::LZ_CHAINS]:
                p = mc.log_add(p, v)
            lz = mc.log_add(lz, p)
    else:
        for v in z:
            lz = mc.log_add(lz, v)
    return lz


def logpost_rows(z, tied):
    z = np.asarray(z, np.float32)
    with np.errstate(all="ignore"):
        return np.stack([(r - logz_row(r, tied)).astype(np.float32) for r in z])


def forward(layers, x, stop_layer=-1, log_prior=None, tied=False):
    """the host twin restated: operands rounded, double sums, f32 activations rounded again, f32 logits, logZ as ever"""
    cur = bf16_round(np.asarray(x, np.float32))
    n = len(layers)
    for l, (w, b, act) in enumerate(layers):
        with np.errstate(all="ignore"):
            y = linear_f64(w, b, cur)[0].astype(np.float32)
        if l < n - 1:
            y = bf16_round(activate(y, act))
        cur = y
        if l == stop_layer:
            return cur
    out = logpost_rows(cur, tied)
    if log_prior is not None:
        with np.errstate(all="ignore"):
            out = (out - np.asarray(log_prior, np.float32)[None, :]).astype(np.float32)
    return out


def bound(K, S):
    """2 (K + 1) 2^-23 S: any order of K + 1 terms, faithful or truncating per addition, and a block-aligned truncating adder"""
    return 2.0 * (K + 1) * 2.0 ** -23 * S


# ---- exact integer networks: whatever the summation order, the logits are the integer product
def int_layer(seed, N, K):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, (N, K)).astype(np.float32), rng.integers(-8, 9, N).astype(np.float32)


def int_rows(seed, n, K):
    return np.random.default_rng(seed + 1).integers(-8, 9, (n, K)).astype(np.float32)


def int_logits(w, b, x):
    """(in float64, where integers of this size are exact and the product is a library call)"""
    z = x.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)[None, :]
    assert (np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T).max() + np.abs(b).max() < 2 ** 24        # every partial sum, any order
    return z.astype(np.float32)


def asym_layer(N, K):
    """W[j][k] = ((7 j + 3 k) mod 251) - 125: no symmetry between outputs and inputs; bf16-exact (|W| <= 125)"""
    j, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    return (((7 * j + 3 * k) % 251) - 125).astype(np.float32), np.zeros(N, np.float32)


INT_KS = (KG - 1, KG, KG + 1, 2 * KG + 1)
INT_NS = (NT - 1, NT, NT + 1, 8 * NT + 1, 16 * NT + 1)


def relu2_net(seed, K, H, N):
    """two layers, RELU between: first-layer weights in {-1, 0, 1} with at most 32 non-zeros a row, so that with inputs in [-8, 8]
    the hidden values stay within +-256 + bias and are bf16-exact (integers below 2^8 ... the bias is 0); the second layer is an
    integer layer"""
    rng = np.random.default_rng(seed)
    w1 = np.zeros((H, K), np.float32)
    for j in range(H):
        idx = rng.choice(K, size=min(K, 31), replace=False)
        w1[j, idx] = rng.integers(-1, 2, idx.shape[0])
    w2, b2 = int_layer(seed + 9, N, H)
    return [(w1, np.zeros(H, np.float32), mc.RELU), (w2, b2, mc.LINEAR)]


def relu2_logits(layers, x):
    (w1, b1, _), (w2, b2, _) = layers
    h = np.maximum(x.astype(np.int64) @ w1.astype(np.int64).T, 0)
    assert h.max() <= 256                                  # every integer up to 256 is a bf16 value
    return int_logits(w2, b2, h.astype(np.float32))
