// jd_mlp_bf16.h - bf16 neural acoustic models (jd_am_mlp_to_bf16): the rounding, the packing of the weights for jd_mlp_bf16_kernel /
// jd_mlp_tied_bf16_kernel (jd_mlp_bf16_kernel.h), the kernels' LDS, and the HOST TWIN jd_mlp_bf16_forward_row, which defines the
// reference value the device is held to.  Pure: no HIP, no device, no library state - tests/mlp_bf16_driver.cpp includes it under
// plain g++.  The network, its limits, its file and the logZ definitions are jd_mlp.h's; reduced precision is a property of the
// MODEL (made from an f32 one), never a decoder mode: JD_SCORE_FAST stays refused for it as for every hybrid model.
//
// jd_bf16_round(float): the nearest value with 8 significant bits (bf16: f32's sign and exponent, 7 stored mantissa bits), ties to
// even, returned as a float whose low 16 bits are zero.  A value that rounds past the largest bf16 (0x7f7f0000 = 3.3895e38) becomes
// +-inf; +-0 and +-inf map to themselves; a NaN stays a NaN (quiet).  f32 SUBNORMAL inputs are outside the contract: this function
// rounds them like any other value, a device may flush them to zero.
//
// Numerics (jd_mlp_bf16_forward_row; a row's result depends on that row alone):
//   operand   every layer's input is x^ = jd_bf16_round(x) - the caller's features too; the weights are w^ = jd_bf16_round(w), which a
//             bf16 model holds in mlp_w as floats.  Biases and log priors stay f32.
//   linear    y[j] = (float)(bias[j] + sum_k x^[k] w^[j][k]): the sum in DOUBLE, k ascending, from the bias.  A product of two bf16
//             values has 16 significant bits: it is exact in f32 and in double, so y is the correctly rounded sum for practical purposes.
//   RELU / SIGMOID   jd_mlp_forward_row's, in f32 (jd_mlp.h), on y.
//   hidden    the activation handed to the next layer - and returned by jd_debug_mlp_activations - is jd_bf16_round of it.
//   output    the last layer's logits stay f32; logZ, z - logZ and - log_prior are jd_mlp.h's, bit for bit: the serial logAdd chain for
//             phone models, JD_MLP_LZ_CHAINS = 128 interleaved chains for tied ones.
// The DEVICE is not held bit for bit to the twin in the linear part: the order and the intermediate rounding of the sums inside a
// bf16 MFMA are not documented.  What it is held to (tests/test_gpu_mlp_bf16.py):
//   linear    |device pre-activation - the twin's double sum| <= 2 (K + 1) 2^-23 S,  S = |bias| + sum_k |x^[k] w^[j][k]|.
//             (K + 1) 2^-23 S bounds any order of the K + 1 terms with a faithful or truncating rounding per addition; the factor 2
//             covers an adder that aligns a block's products to its largest exponent and truncates.  Derived, not measured.
//   given the logits      the log posteriors equal, bit for bit, the logZ chain over the device's own logits.
//   given bf16            a hidden activation the device hands on is a bf16 value: the operand of layer l is what
//                         jd_debug_mlp_activations(on_device = 1, layer l - 1) returned.
//   row independence      bit for bit: K is split into k groups of 32 and accumulated in ascending order from the bias, one
//                         accumulator per output, for every launch, grid and batch.
//   SIGMOID   the kernel runs the bit-exact jd_mlp_expf and a float division, as the f32 kernel does: the hidden layers are a small
//             part of the pass beside the output layer, and with it a hidden activation differs from the twin's only through the
//             linear bound (Lipschitz 1/4; 1 for RELU and LINEAR) and the half-ulp bf16 rounding, 2^-8 relative.
//
// Tile and LDS.  A workgroup takes JD_MLP_BF16_ROWS = 32 rows (two MFMA row tiles) through all layers; the activations are bf16 in two
// ping-pong buffers [32][stride].  The matrix instruction is v_mfma_f32_16x16x32_bf16: lane l holds A[row l & 15][k = 8 (l >> 4) + e]
// and B[k = 8 (l >> 4) + e][col l & 15], e = 0 .. 7, so in natural k order a lane's A operand of a k group of JD_MLP_BF16_KG = 32
// inputs is ONE 16-byte read at row (l & 15), byte 64 kg + 16 (l >> 4).  stride = the widest of in_dim and the layers held in LDS, padded
// to the k group, then to 16 modulo 128 elements (32 bytes modulo 256): a 16-byte LDS read is served in four groups of 16 lanes -
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 - so a group reads all 16 rows, eight at one 16-byte column and eight at
// the next.  The LDS is 16 slots of 16 bytes wide; with a row stride of 2 slots modulo 16 the rows 0-3, 12-15 fall on eight distinct
// even slots and the rows 4-11, one column further, on the eight odd ones: no conflict.  (A stride of 1 slot modulo 16, the usual
// padding, puts row 12 and row 11 + one column on the same slot; no odd stride is free of such a pair.)
//   1024 wide: stride 1040, 2 x 32 x 1040 x 2 B = 130 KB, + 256 B of bookkeeping; tied + 32 x 128 x 4 B = 16 KB of partial chains.
// The last layer's logits are f32 and do not live in LDS (32 x 1024 floats = 128 KB): both kernels keep them in the tile's own rows
// of the table and normalise in place, as jd_mlp_tied_kernel does.  The limits are jd_mlp.h's, unchanged.
//
// Packing (jd_mlp_bf16_pack; jd_mlp_bf16_unpack is its inverse).  A layer's K is padded to Kp = 32 ceil(K / 32), its N to
// Np = 32 ceil(N / 32) (n tiles of JD_MLP_BF16_NT = 16 outputs come in pairs); the packed weight of output j, input k is the
// 16-bit element
//   w_off[l] + ((j / 16) (Kp / 32) + k / 32) 512 + (((k % 32) / 8) 16 + j % 16) 8 + k % 8
// so that a lane's B fragment of an (n tile, k group) is one 16-byte load and a wave's is 1 KB contiguous.  The padding is +0, in
// the weights, the biases (padded to Np) and the activations: no -0 trick is needed where nothing is held bit for bit to a chain,
// and a padded product is (+0) (+0).
#ifndef JD_MLP_BF16_H
#define JD_MLP_BF16_H

#include "jd_mlp.h"

#ifndef JD_MLP_F32
#define JD_MLP_F32 0
#define JD_MLP_BF16 1
#endif
#define JD_MLP_BF16_ROWS 32         // rows of a workgroup's tile: two MFMA row tiles
#define JD_MLP_BF16_NT 16           // outputs of an n tile (the MFMA's N)
#define JD_MLP_BF16_KG 32           // inputs of a k group (the MFMA's K)

static JD_MLP_HD uint32_t jd_bf16_f2u(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
static JD_MLP_HD float jd_bf16_u2f(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }
// the bf16 nearest to x, ties to even, as its 16 bits
static JD_MLP_HD uint16_t jd_bf16_bits(float x)
{
    const uint32_t u = jd_bf16_f2u(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);       // a NaN: quiet, never rounded into inf
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                        // (a carry out of the mantissa is the next exponent; past the largest, inf)
}
static JD_MLP_HD float jd_bf16_round(float x) { return jd_bf16_u2f((uint32_t)jd_bf16_bits(x) << 16); }

static inline int jd_mlp_pad32(int n) { return (n + 31) / 32 * 32; }
// what the bf16 kernels are told: jd_mlp.h's JdMlpDev with stride, w_off in 16-bit ELEMENTS and b_off padded to 32
// (tied: the last layer's outputs do not widen the stride; they never live in LDS for either kind)
static inline JdMlpDev jd_mlp_bf16_dev(const JdMlpDesc &d)
{
    JdMlpDev m;
    memset(&m, 0, sizeof m);
    m.in_dim = d.in_dim; m.n_layers = d.n_layers;
    m.base_dim = d.in_dim;
    int widest = jd_mlp_pad32(d.in_dim);
    for (int l = 0; l < d.n_layers; ++l) {
        m.width[l] = d.width[l]; m.act[l] = d.act[l];
        m.w_off[l + 1] = m.w_off[l] + (uint32_t)jd_mlp_pad32(d.width[l]) * (uint32_t)jd_mlp_pad32(jd_mlp_k(d, l));
        m.b_off[l + 1] = m.b_off[l] + (uint32_t)jd_mlp_pad32(d.width[l]);
        if (l < d.n_layers - 1 && jd_mlp_pad32(d.width[l]) > widest) widest = jd_mlp_pad32(d.width[l]);
    }
    m.stride = widest + ((16 - widest % 128) + 128) % 128;        // 16 modulo 128 elements: see above
    return m;
}
// two activation buffers of bf16, the tile's row_src entries and its rows' logZ
static inline size_t jd_mlp_bf16_lds_bytes(const JdMlpDev &m) { return (size_t)2 * JD_MLP_BF16_ROWS * m.stride * 2 + (size_t)2 * JD_MLP_BF16_ROWS * 4; }
// jd_mlp_tied_bf16_kernel's: the same, and the tile's partial chains [32][JD_MLP_LZ_CHAINS]
static inline size_t jd_mlp_tied_bf16_lds_bytes(const JdMlpDev &m) { return jd_mlp_bf16_lds_bytes(m) + (size_t)JD_MLP_BF16_ROWS * JD_MLP_LZ_CHAINS * 4; }
#define JD_MLP_BF16_LDS_MAX ((size_t)2 * JD_MLP_BF16_ROWS * (JD_MLP_MAX_DIM + 16) * 2 + (size_t)2 * JD_MLP_BF16_ROWS * 4)
#define JD_MLP_TIED_BF16_LDS_MAX (JD_MLP_BF16_LDS_MAX + (size_t)JD_MLP_BF16_ROWS * JD_MLP_LZ_CHAINS * 4)

// packed weight (output j, input k) of a layer padded to Kp inputs, relative to the layer's w_off
static inline size_t jd_mlp_bf16_w_index(int Kp, int j, int k)
{
    const size_t nt = (size_t)(j / JD_MLP_BF16_NT), kg = (size_t)(k / JD_MLP_BF16_KG);
    const int kk = k % JD_MLP_BF16_KG, lane = (kk / 8) * 16 + j % JD_MLP_BF16_NT;
    return ((nt * (size_t)(Kp / JD_MLP_BF16_KG) + kg) * 64 + (size_t)lane) * 8 + (size_t)(kk % 8);
}
// w / b: the layers' [out][in] weights (rounded here) and biases one after the other
static inline void jd_mlp_bf16_pack(const JdMlpDesc &d, const float *w, const float *b, std::vector<uint16_t> &wp, std::vector<float> &bp)
{
    const JdMlpDev m = jd_mlp_bf16_dev(d);
    wp.assign(m.w_off[d.n_layers], (uint16_t)0);
    bp.assign(m.b_off[d.n_layers], 0.0f);
    for (int l = 0; l < d.n_layers; ++l) {
        const int K = jd_mlp_k(d, l), Kp = jd_mlp_pad32(K), N = d.width[l];
        const float *wl = w + jd_mlp_w_begin(d, l), *bl = b + jd_mlp_b_begin(d, l);
        for (int j = 0; j < N; ++j) {
            for (int k = 0; k < K; ++k) wp[m.w_off[l] + jd_mlp_bf16_w_index(Kp, j, k)] = jd_bf16_bits(wl[(size_t)j * K + k]);
            bp[m.b_off[l] + j] = bl[j];
        }
    }
}
static inline void jd_mlp_bf16_unpack(const JdMlpDesc &d, const uint16_t *wp, const float *bp, std::vector<float> &w, std::vector<float> &b)
{
    const JdMlpDev m = jd_mlp_bf16_dev(d);
    w.assign(jd_mlp_w_begin(d, d.n_layers), 0.0f);
    b.assign(jd_mlp_b_begin(d, d.n_layers), 0.0f);
    for (int l = 0; l < d.n_layers; ++l) {
        const int K = jd_mlp_k(d, l), Kp = jd_mlp_pad32(K), N = d.width[l];
        float *wl = w.data() + jd_mlp_w_begin(d, l), *bl = b.data() + jd_mlp_b_begin(d, l);
        for (int j = 0; j < N; ++j) {
            for (int k = 0; k < K; ++k) wl[(size_t)j * K + k] = jd_bf16_u2f((uint32_t)wp[m.w_off[l] + jd_mlp_bf16_w_index(Kp, j, k)] << 16);
            bl[j] = bp[m.b_off[l] + j];
        }
    }
}

// ---- the host twin.  Arguments as jd_mlp_forward_row's; w holds ROUNDED weights (a bf16 model's mlp_w) - weights that are not
// bf16 values are rounded as they are read, so the result is the same either way.
template <class M>
static inline void jd_mlp_bf16_forward_row(const JdMlpDesc &d, const float *w, const float *b, const float *log_prior, const float *x, int stop_layer,
                                           float *out, const M &math, bool tied = false)
{
    std::vector<float> cur((size_t)d.in_dim), nxt;
    for (int k = 0; k < d.in_dim; ++k) cur[(size_t)k] = jd_bf16_round(x[k]);
    for (int l = 0; l < d.n_layers; ++l) {
        const int K = jd_mlp_k(d, l), N = d.width[l];
        const bool last = l == d.n_layers - 1;
        const float *wl = w + jd_mlp_w_begin(d, l), *bl = b + jd_mlp_b_begin(d, l);
        nxt.assign((size_t)N, 0.0f);
        for (int j = 0; j < N; ++j) {
            double s = (double)bl[j];
            for (int k = 0; k < K; ++k) s += (double)cur[(size_t)k] * (double)jd_bf16_round(wl[(size_t)j * K + k]);
            float y = (float)s;
            if (!last) {
                if (d.act[l] == JD_ACT_RELU) y = y > 0.0f ? y : 0.0f;
                else if (d.act[l] == JD_ACT_SIGMOID) y = 1.0f / (1.0f + math.exp(-y));
                y = jd_bf16_round(y);
            }
            nxt[(size_t)j] = y;
        }
        cur.swap(nxt);
        if (l == stop_layer) { memcpy(out, cur.data(), (size_t)N * sizeof(float)); return; }
    }
    const int P = d.width[d.n_layers - 1];
    float lz = JD_MLP_LOG_ZERO;
    if (tied) {
        const int C = P < JD_MLP_LZ_CHAINS ? P : JD_MLP_LZ_CHAINS;
        for (int c = 0; c < C; ++c) {
            float p = JD_MLP_LOG_ZERO;
            for (int j = c; j < P; j += JD_MLP_LZ_CHAINS) p = math.log_add(p, cur[(size_t)j]);
            lz = math.log_add(lz, p);
        }
    } else
        for (int j = 0; j < P; ++j) lz = math.log_add(lz, cur[(size_t)j]);
    for (int j = 0; j < P; ++j) {
        const float lp = cur[(size_t)j] - lz;
        out[j] = log_prior ? lp - log_prior[j] : lp;
    }
}
template <class M>
static inline void jd_mlp_bf16_forward_host(const JdMlpDesc &d, const float *w, const float *b, const float *log_prior, const float *x, int n,
                                            int stop_layer, float *out, const M &math, bool tied = false)
{
    const int ow = stop_layer >= 0 ? d.width[stop_layer] : d.width[d.n_layers - 1];
    for (int r = 0; r < n; ++r) jd_mlp_bf16_forward_row(d, w, b, log_prior, x + (size_t)r * d.in_dim, stop_layer, out + (size_t)r * ow, math, tied);
}
#endif
