// jd_mlp.h - neural acoustic models (jd_am_create_mlp): the network as plain data, its limits and argument check, the packing of
// its weights for jd_mlp_kernel (jd_mlp_kernel.h), the JMLP file, and the HOST TWIN jd_mlp_forward_host, which defines the numerics
// the kernel is held to bit for bit.  Pure: no HIP, no device, no library state - tests/mlp_driver.cpp includes it under plain g++.
//
// The model.  in_dim inputs, n_layers >= 1 fully connected layers of widths width[l]; the last width is n_phones.  Weights are
// [layer][out][in] row-major with one bias per output.  A HIDDEN layer l < n_layers - 1 ends in act[l] (JD_ACT_LINEAR / JD_ACT_RELU /
// JD_ACT_SIGMOID); the last layer's outputs are the logits z of a log-softmax, and what the search reads is the hybrid score
// (HTKFlatModels.cpp:190-222)  ll[j] = (z[j] - logZ) - log(prior[j]).
//
// Numerics (jd_mlp_forward_row; a row's result depends on that row alone - never on the batch it sits in or on a tile shape):
//   linear    y[j] = fmaf(x[K-1], w[j][K-1], ... fmaf(x[0], w[j][0], bias[j])): ONE chain per output, k ascending, from the bias.
//             gfx950's f32-input MFMA is such a chain with one rounding per product, so the kernel may not split K or reorder.
//   RELU      y > 0 ? y : 0                      (a NaN becomes 0)
//   SIGMOID   1.0f / (1.0f + expf(-y))           float division; expf as glibc's (overflow gives inf and the result 0)
//   output    logZ = logAdd chain over z[0], z[1], ... from JD_LOG_ZERO (HTKFlatModels::logAdd with its -18.42 cut: the function the
//             GMM kernels add mixtures with); logpost[j] = z[j] - logZ; ll[j] = logpost[j] - log_prior[j], one float operation each.
// The two functions the chain needs come in as a policy M { float exp(float); float log_add(float, float); }: the library passes
// the bit-exact replicas of jd_gmm.h (jd_am_mlp_forward_host), a g++ driver passes libm itself - tests/test_expf.py and
// tests/test_logadd.py hold the two equal.
//
// Limits, from the kernel's LDS budget (gfx950: 160 KB a CU).  A workgroup takes a tile of JD_MLP_ROWS = 16 rows through all layers
// with two ping-pong activation buffers of 16 x (widest padded layer + 4) floats: 2 x 16 x 1028 x 4 B = 128.5 KB at the limit, plus
// 128 B of row bookkeeping.
//   JD_MLP_MAX_DIM     1024   in_dim and every width (1 .. 1024)
//   JD_MLP_MAX_LAYERS  16     (a kernel argument holds the layer table)
// A network beyond them is JD_EINVAL with a message that names the limit.
//
// Packing (jd_mlp_pack; jd_mlp_unpack is its inverse).  The kernel multiplies with v_mfma_f32_16x16x4_f32: lane l of a wave holds
// A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15] of a k-step of 4.  A layer's K is padded to Kp = 16 ceil(K / 16) (FOUR k-steps:
// one 16-byte load per lane), its N to Np = 16 ceil(N / 16); the packed weight of output j, input k sits at
//   w_off[l] + (((j / 16) (Kp / 16) + k / 16) 64 + ((k % 4) 16 + j % 16)) 4 + (k % 16) / 4
// so that a wave's load of one (n tile, k group) is 1 KB contiguous, and the padding is +0.0f.  Biases are padded to Np with 0.
// The ACTIVATIONS' padding in LDS is -0.0f: a padded step is then fmaf(-0, +0, c) = c for every c, a -0 included.
//
// TIED models (jd_am_create_mlp_tied: one output per tied state - senone - of an HMM set of any topology).  Layers, activations
// and the linear chain are the same; two things differ:
//   limits    the LAST width is 1 .. JD_MLP_MAX_OUT = 16384 (in_dim and the hidden widths stay 1 .. JD_MLP_MAX_DIM): the output
//             layer's logits do not live in LDS (16 x 16384 floats = 1 MB) but in the tile's own rows of the likelihood table, so
//             that the LDS holds the widest of in_dim and the HIDDEN layers, plus the partials below.
//   output    logZ over several thousand outputs is not one serial chain.  JD_MLP_LZ_CHAINS = 128 - a constant: never a function
//             of rows, launch, grid, device or network - interleaved partial chains
//               p[c] = logAdd chain from JD_MLP_LOG_ZERO over z[c], z[c + 128], z[c + 256], ...  (ascending)   for c < min(128, P)
//               logZ = logAdd chain from JD_MLP_LOG_ZERO over p[0], p[1], ...                    (ascending; empty chains, c >= P,
//                      are not combined)
//             then logpost[j] = z[j] - logZ and ll[j] = logpost[j] - log_prior[j], one float operation each, as above.
//             (128: a workgroup's four waves cover 8 n tiles of 16 outputs a turn, so chain j mod 128 belongs to one wave, which
//             meets its elements in ascending order and keeps the partial in a register beside the accumulator.)
// jd_mlp_forward_row / jd_mlp_forward_host take the model kind as their last argument (false: the serial chain, bit for bit as ever).
//
// JMLP file (little-endian, no padding; jd_am_save_mlp / jd_am_load_mlp):
//   char   magic[4] = "JMLP"
//   u32    version = 1
//   i32    n_phones, states_per_model, in_dim, n_layers
//   i32    width[n_layers]
//   i32    act[n_layers]            (act[n_layers - 1] = 0)
//   f32    priors[n_phones]         (as given to jd_am_create_mlp, not their logarithms)
//   per layer l:  f32 weight[width[l]][K_l], f32 bias[width[l]]        (K_0 = in_dim, K_l = width[l - 1])
// A file that ends early, carries another magic or version, describes a network the check refuses, or is longer than its header
// says is JD_EFORMAT.
// Version 2 is a TIED model's network (jd_am_save_mlp on such a model / jd_am_load_mlp_tied): the same layout with
// states_per_model = 0 and n_phones = the number of outputs (tied states), up to JD_MLP_MAX_OUT.  It holds no topology: the loader
// is given the HMM set.  Each loader refuses the other's version and names the loader that reads it.
#ifndef JD_MLP_H
#define JD_MLP_H

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#ifndef JD_ACT_LINEAR
#define JD_ACT_LINEAR 0
#define JD_ACT_RELU 1
#define JD_ACT_SIGMOID 2
#endif

#define JD_MLP_MAX_DIM 1024
#define JD_MLP_MAX_LAYERS 16
#define JD_MLP_MAX_OUT 16384        // the last width of a TIED model (jd_am_create_mlp_tied): its logits live in the likelihood table
#define JD_MLP_LZ_CHAINS 128        // a tied model's logZ: interleaved partial chains (a constant of the numerics)
#define JD_MLP_ROWS 16              // rows of a workgroup's tile (the MFMA's M)
#define JD_MLP_NT 16                // outputs of an n tile (the MFMA's N)
#define JD_MLP_KG 16                // inputs of a k group: four k-steps of 4
#define JD_MLP_LDS_PAD 4            // floats behind a row of activations in LDS (row stride 4 mod 16)
#define JD_MLP_LOG_ZERO (-3.402823466e+38f)

struct JdMlpDesc {
    int32_t in_dim = 0, n_layers = 0;
    int32_t width[JD_MLP_MAX_LAYERS] = {};
    int32_t act[JD_MLP_MAX_LAYERS] = {};          // act[n_layers - 1] = JD_ACT_LINEAR
};

static inline int jd_mlp_pad16(int n) { return (n + 15) / 16 * 16; }
static inline int jd_mlp_k(const JdMlpDesc &d, int l) { return l == 0 ? d.in_dim : d.width[l - 1]; }
// elements of the unpacked weights / biases in front of layer l (l = n_layers: in all)
static inline size_t jd_mlp_w_begin(const JdMlpDesc &d, int l)
{
    size_t n = 0;
    for (int i = 0; i < l; ++i) n += (size_t)d.width[i] * jd_mlp_k(d, i);
    return n;
}
static inline size_t jd_mlp_b_begin(const JdMlpDesc &d, int l)
{
    size_t n = 0;
    for (int i = 0; i < l; ++i) n += (size_t)d.width[i];
    return n;
}

// 0, or what is wrong with the description (msg names the limit)
// (tied: the models of jd_am_create_mlp_tied - the last width is bounded by JD_MLP_MAX_OUT and n_phones counts tied states)
static inline int jd_mlp_check(const JdMlpDesc &d, int n_phones, char *msg, size_t cap, bool tied = false)
{
    if (d.n_layers < 1 || d.n_layers > JD_MLP_MAX_LAYERS) {
        snprintf(msg, cap, "n_layers = %d outside 1 .. %d (JD_MLP_MAX_LAYERS)", d.n_layers, JD_MLP_MAX_LAYERS);
        return 1;
    }
    if (d.in_dim < 1 || d.in_dim > JD_MLP_MAX_DIM) {
        snprintf(msg, cap, "in_dim = %d outside 1 .. %d (JD_MLP_MAX_DIM: the activations of a 16-row tile stay in LDS)", d.in_dim, JD_MLP_MAX_DIM);
        return 2;
    }
    for (int l = 0; l < d.n_layers; ++l) {
        if (tied && l == d.n_layers - 1) {
            if (d.width[l] < 1 || d.width[l] > JD_MLP_MAX_OUT) {
                snprintf(msg, cap, "width[%d] = %d outside 1 .. %d (JD_MLP_MAX_OUT: the last width of a tied model)", l, d.width[l], JD_MLP_MAX_OUT);
                return 3;
            }
        } else if (d.width[l] < 1 || d.width[l] > JD_MLP_MAX_DIM) {
            snprintf(msg, cap, "width[%d] = %d outside 1 .. %d (JD_MLP_MAX_DIM: the activations of a 16-row tile stay in LDS)", l, d.width[l], JD_MLP_MAX_DIM);
            return 3;
        }
        if (l < d.n_layers - 1 && d.act[l] != JD_ACT_LINEAR && d.act[l] != JD_ACT_RELU && d.act[l] != JD_ACT_SIGMOID) {
            snprintf(msg, cap, "act[%d] = %d is none of JD_ACT_LINEAR (0), JD_ACT_RELU (1), JD_ACT_SIGMOID (2)", l, d.act[l]);
            return 4;
        }
    }
    if (d.act[d.n_layers - 1] != JD_ACT_LINEAR) {
        snprintf(msg, cap, "act[%d] = %d: the last layer's outputs are the logits of the log-softmax (JD_ACT_LINEAR)", d.n_layers - 1, d.act[d.n_layers - 1]);
        return 5;
    }
    if (d.width[d.n_layers - 1] != n_phones) {
        if (tied) snprintf(msg, cap, "the last width, %d, is not the topology's number of tied states, n_gmm = %d", d.width[d.n_layers - 1], n_phones);
        else snprintf(msg, cap, "the last width, %d, is not n_phones = %d", d.width[d.n_layers - 1], n_phones);
        return 6;
    }
    return 0;
}

// ---- what the kernel is told (a kernel argument) and its LDS
struct JdMlpDev {
    int32_t in_dim, n_layers, stride;             // stride: floats of an activation row in LDS
    int32_t width[JD_MLP_MAX_LAYERS], act[JD_MLP_MAX_LAYERS];
    uint32_t w_off[JD_MLP_MAX_LAYERS + 1], b_off[JD_MLP_MAX_LAYERS + 1];      // packed; [n_layers]: the sizes
    int32_t base_dim, left, right;                // spliced models (jd_splice.h): the frames' size and the context; else in_dim, 0, 0
};
// (tied: jd_mlp_tied_kernel's - the last layer's outputs are not held in LDS and do not widen the stride)
static inline JdMlpDev jd_mlp_dev(const JdMlpDesc &d, bool tied = false)
{
    JdMlpDev m;
    memset(&m, 0, sizeof m);
    m.in_dim = d.in_dim; m.n_layers = d.n_layers;
    m.base_dim = d.in_dim;
    int widest = jd_mlp_pad16(d.in_dim);
    for (int l = 0; l < d.n_layers; ++l) {
        m.width[l] = d.width[l]; m.act[l] = d.act[l];
        m.w_off[l + 1] = m.w_off[l] + (uint32_t)jd_mlp_pad16(d.width[l]) * (uint32_t)jd_mlp_pad16(jd_mlp_k(d, l));
        m.b_off[l + 1] = m.b_off[l] + (uint32_t)jd_mlp_pad16(d.width[l]);
        if (!(tied && l == d.n_layers - 1) && jd_mlp_pad16(d.width[l]) > widest) widest = jd_mlp_pad16(d.width[l]);
    }
    m.stride = widest + JD_MLP_LDS_PAD;
    return m;
}
// two activation buffers, the tile's row_src entries and its rows' logZ
static inline size_t jd_mlp_lds_bytes(const JdMlpDev &m) { return ((size_t)2 * JD_MLP_ROWS * m.stride + 2 * JD_MLP_ROWS) * 4; }
#define JD_MLP_LDS_MAX ((size_t)(2 * JD_MLP_ROWS * (JD_MLP_MAX_DIM + JD_MLP_LDS_PAD) + 2 * JD_MLP_ROWS) * 4)
// jd_mlp_tied_kernel's (m = jd_mlp_dev(d, true)): the same, and the tile's partial chains [16][JD_MLP_LZ_CHAINS]
static inline size_t jd_mlp_tied_lds_bytes(const JdMlpDev &m) { return jd_mlp_lds_bytes(m) + (size_t)JD_MLP_ROWS * JD_MLP_LZ_CHAINS * 4; }
#define JD_MLP_TIED_LDS_MAX (JD_MLP_LDS_MAX + (size_t)JD_MLP_ROWS * JD_MLP_LZ_CHAINS * 4)

// where input k of an activation row sits in LDS: a k group's 16 values k-step-minor, so that a lane's four k-steps (k = 4 e + q,
// e = 0 .. 3, for its q = lane >> 4) are one 16-byte read
#ifdef __HIPCC__
#define JD_MLP_HD __host__ __device__ inline
#else
#define JD_MLP_HD inline
#endif
static JD_MLP_HD int jd_mlp_act_pos(int k) { return (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3); }
// packed weight (output j, input k) of a layer padded to Kp inputs, relative to the layer's w_off
static inline size_t jd_mlp_w_index(int Kp, int j, int k)
{
    const size_t nt = (size_t)(j / JD_MLP_NT), kg = (size_t)(k / JD_MLP_KG);
    const int kk = k % JD_MLP_KG, lane = (kk & 3) * 16 + j % JD_MLP_NT;
    return ((nt * (size_t)(Kp / JD_MLP_KG) + kg) * 64 + (size_t)lane) * 4 + (size_t)(kk >> 2);
}

// w / b: the layers' [out][in] weights and biases one after the other
static inline void jd_mlp_pack(const JdMlpDesc &d, const float *w, const float *b, std::vector<float> &wp, std::vector<float> &bp)
{
    const JdMlpDev m = jd_mlp_dev(d);
    wp.assign(m.w_off[d.n_layers], 0.0f);
    bp.assign(m.b_off[d.n_layers], 0.0f);
    for (int l = 0; l < d.n_layers; ++l) {
        const int K = jd_mlp_k(d, l), Kp = jd_mlp_pad16(K), N = d.width[l];
        const float *wl = w + jd_mlp_w_begin(d, l), *bl = b + jd_mlp_b_begin(d, l);
        for (int j = 0; j < N; ++j) {
            for (int k = 0; k < K; ++k) wp[m.w_off[l] + jd_mlp_w_index(Kp, j, k)] = wl[(size_t)j * K + k];
            bp[m.b_off[l] + j] = bl[j];
        }
    }
}
static inline void jd_mlp_unpack(const JdMlpDesc &d, const float *wp, const float *bp, std::vector<float> &w, std::vector<float> &b)
{
    const JdMlpDev m = jd_mlp_dev(d);
    w.assign(jd_mlp_w_begin(d, d.n_layers), 0.0f);
    b.assign(jd_mlp_b_begin(d, d.n_layers), 0.0f);
    for (int l = 0; l < d.n_layers; ++l) {
        const int K = jd_mlp_k(d, l), Kp = jd_mlp_pad16(K), N = d.width[l];
        float *wl = w.data() + jd_mlp_w_begin(d, l), *bl = b.data() + jd_mlp_b_begin(d, l);
        for (int j = 0; j < N; ++j) {
            for (int k = 0; k < K; ++k) wl[(size_t)j * K + k] = wp[m.w_off[l] + jd_mlp_w_index(Kp, j, k)];
            bl[j] = bp[m.b_off[l] + j];
        }
    }
}

// ---- the host twin.  One row x[in_dim].  stop_layer in [0, n_layers): out[width[stop_layer]] = the activations behind that layer
// (the raw logits for the last).  stop_layer = -1: out[n_phones] = the log posteriors (log_prior null) or the hybrid scores.
// tied: logZ by JD_MLP_LZ_CHAINS interleaved partial chains (the models of jd_am_create_mlp_tied), else the one serial chain.
template <class M>
static inline void jd_mlp_forward_row(const JdMlpDesc &d, const float *w, const float *b, const float *log_prior, const float *x, int stop_layer,
                                      float *out, const M &math, bool tied = false)
{
    std::vector<float> cur(x, x + d.in_dim), nxt;
    for (int l = 0; l < d.n_layers; ++l) {
        const int K = jd_mlp_k(d, l), N = d.width[l];
        const float *wl = w + jd_mlp_w_begin(d, l), *bl = b + jd_mlp_b_begin(d, l);
        nxt.assign((size_t)N, 0.0f);
        for (int j = 0; j < N; ++j) {
            float y = bl[j];
            for (int k = 0; k < K; ++k) y = fmaf(cur[(size_t)k], wl[(size_t)j * K + k], y);
            if (l < d.n_layers - 1) {
                if (d.act[l] == JD_ACT_RELU) y = y > 0.0f ? y : 0.0f;
                else if (d.act[l] == JD_ACT_SIGMOID) y = 1.0f / (1.0f + math.exp(-y));
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
// n rows of x [n][in_dim]; out [n][width[stop_layer]] / [n][n_phones]
template <class M>
static inline void jd_mlp_forward_host(const JdMlpDesc &d, const float *w, const float *b, const float *log_prior, const float *x, int n,
                                       int stop_layer, float *out, const M &math, bool tied = false)
{
    const int ow = stop_layer >= 0 ? d.width[stop_layer] : d.width[d.n_layers - 1];
    for (int r = 0; r < n; ++r) jd_mlp_forward_row(d, w, b, log_prior, x + (size_t)r * d.in_dim, stop_layer, out + (size_t)r * ow, math, tied);
}

// ---- the JMLP file as bytes
struct JdMlpFile {
    JdMlpDesc d;
    int32_t n_phones = 0, states_per_model = 0;
    std::vector<float> priors, w, b;              // [n_phones]; the layers' weights / biases one after the other
    bool tied = false;                            // version 2: a tied model's network (states_per_model = 0, n_phones = the outputs)
};
static inline void jd_mlp_file_write(const JdMlpFile &f, std::vector<unsigned char> &out)
{
    out.clear();
    auto put = [&](const void *p, size_t n) { const unsigned char *c = (const unsigned char *)p; out.insert(out.end(), c, c + n); };
    const uint32_t version = f.tied ? 2 : 1;
    put("JMLP", 4); put(&version, 4);
    put(&f.n_phones, 4); put(&f.states_per_model, 4); put(&f.d.in_dim, 4); put(&f.d.n_layers, 4);
    put(f.d.width, 4 * (size_t)f.d.n_layers); put(f.d.act, 4 * (size_t)f.d.n_layers);
    put(f.priors.data(), 4 * f.priors.size());
    for (int l = 0; l < f.d.n_layers; ++l) {
        put(f.w.data() + jd_mlp_w_begin(f.d, l), 4 * (size_t)f.d.width[l] * jd_mlp_k(f.d, l));
        put(f.b.data() + jd_mlp_b_begin(f.d, l), 4 * (size_t)f.d.width[l]);
    }
}
// 0, or what is wrong with the bytes (tied: the reader of version 2, jd_am_load_mlp_tied's; else of version 1)
static inline int jd_mlp_file_read(const unsigned char *p, size_t n, JdMlpFile &f, char *msg, size_t cap, bool tied = false)
{
    size_t at = 0;
    auto get = [&](void *q, size_t k) { if (n - at < k) return false; memcpy(q, p + at, k); at += k; return true; };
    char magic[4]; uint32_t version = 0;
    if (!get(magic, 4) || memcmp(magic, "JMLP", 4) != 0) { snprintf(msg, cap, "not a JMLP file (magic)"); return 1; }
    if (!get(&version, 4) || (version != 1 && version != 2)) { snprintf(msg, cap, "JMLP version %u (this build reads 1 and 2)", version); return 2; }
    if (version == 2 && !tied) { snprintf(msg, cap, "JMLP version 2: a tied-state network without a topology (jd_am_load_mlp_tied reads it beside an HMM set)"); return 2; }
    if (version == 1 && tied) { snprintf(msg, cap, "JMLP version 1: a phone network with its own topology (jd_am_load_mlp reads it)"); return 2; }
    f = JdMlpFile();
    f.tied = tied;
    if (!get(&f.n_phones, 4) || !get(&f.states_per_model, 4) || !get(&f.d.in_dim, 4) || !get(&f.d.n_layers, 4)) { snprintf(msg, cap, "JMLP header truncated"); return 3; }
    if (f.d.n_layers < 1 || f.d.n_layers > JD_MLP_MAX_LAYERS || f.n_phones < 1 || f.n_phones > (tied ? JD_MLP_MAX_OUT : JD_MLP_MAX_DIM) ||
        (tied && f.states_per_model != 0)) {
        snprintf(msg, cap, "JMLP header: n_layers = %d, n_phones = %d", f.d.n_layers, f.n_phones);
        return 4;
    }
    if (!get(f.d.width, 4 * (size_t)f.d.n_layers) || !get(f.d.act, 4 * (size_t)f.d.n_layers)) { snprintf(msg, cap, "JMLP header truncated"); return 3; }
    char why[200];
    if (jd_mlp_check(f.d, f.n_phones, why, sizeof why, tied)) { snprintf(msg, cap, "JMLP header: %s", why); return 4; }
    f.priors.resize((size_t)f.n_phones);
    f.w.resize(jd_mlp_w_begin(f.d, f.d.n_layers));
    f.b.resize(jd_mlp_b_begin(f.d, f.d.n_layers));
    bool ok = get(f.priors.data(), 4 * f.priors.size());
    for (int l = 0; ok && l < f.d.n_layers; ++l)
        ok = get(f.w.data() + jd_mlp_w_begin(f.d, l), 4 * (size_t)f.d.width[l] * jd_mlp_k(f.d, l)) && get(f.b.data() + jd_mlp_b_begin(f.d, l), 4 * (size_t)f.d.width[l]);
    if (!ok) { snprintf(msg, cap, "JMLP file truncated: %zu bytes", n); return 5; }
    if (at != n) { snprintf(msg, cap, "JMLP file of %zu bytes, its header describes %zu", n, at); return 6; }
    return 0;
}
#endif
