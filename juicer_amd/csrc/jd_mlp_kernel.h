// jd_mlp_kernel.h - the forward pass of a neural acoustic model on the device (included by jd_device.hip behind jd_gmm.h; gfx950 only):
// jd_mlp_kernel takes a tile of JD_MLP_ROWS = 16 rows of a likelihood table through ALL layers of the network - linear layers on
// v_mfma_f32_16x16x4_f32, activations, log-softmax, minus the log priors - and writes only its rows of the table.  The numerics are
// jd_mlp_forward_row's (jd_mlp.h), bit for bit.
//
// Fused because launch_gmm has no memory of its own: it is called with one shared AmDevBuf on several streams at once, and a layer's
// activations in global memory would be shared by the launches in flight.  They live in LDS: two buffers [16][stride] that the
// layers fill in turn, stride = the widest padded layer + 4 floats.
//
// A workgroup is four waves.  A wave takes PAIRS of n tiles (16 outputs each) of a layer: two independent accumulators keep the
// MFMA's issue rate (32 cycles issue, 40 dependent), and both share the A operand.  Per k group of 16 inputs a lane reads 16 bytes of
// activations from LDS (jd_mlp_act_pos: its four k-steps side by side) and 16 bytes of each tile's packed weights from memory
// (jd_mlp_w_index: 1 KB contiguous per wave), two k groups ahead of their use, then issues four MFMAs per tile; C-in of the first is
// the bias.  K is never split and a chain never reordered: the result is the k-ascending fmaf chain whatever the tile or the batch.
// Padded inputs are -0 in the activations and +0 in the weights (a padded step leaves every c as it is), padded outputs are not stored.
//
// The logits of the last layer land in LDS; lane r of the first wave runs row r's logAdd chain (serial by definition: no tree), and
// all threads write (z - logZ) - log_prior, coalesced.  A row with row_src < 0 is written as 0.0f (as jd_hybrid_kernel does); a tile
// whose rows are all unused does no arithmetic.  The grid strides over the row tiles (launch_gmm's max_blocks).
//
// jd_mlp_tied_kernel, at the end of this file, is the same pass for the models of jd_am_create_mlp_tied: an output layer of up to
// 16384 tied states whose logits live in the tile's rows of the table, and logZ by 128 interleaved chains.
//
// SPLICED models (jd_am_mlp_splice, jd_splice.h).  Each kernel is a template over SPL; jd_mlp_kernel / jd_mlp_tied_kernel name the
// SPL = false instantiations - the code of an unspliced model, which reads neither `span` nor the context - and jd_mlp_spliced_kernel /
// jd_mlp_tied_spliced_kernel the SPL = true ones, which differ in the input stage alone (jd_mlp_stage_spliced): the tile keeps its
// rows' spans beside ssrc and fills the first activation buffer with C = left + right + 1 pieces of D = base_dim values each, piece c
// of a row from frame jd_splice_frame(row_src, c, left, span).  The layout in LDS is the one layer 0 expects.
#pragma once

typedef float jd_mlp_f4 __attribute__((ext_vector_type(4)));

// glibc's expf with its special cases around jd_expf_impl (e_expf.c: NaN, +-inf, overflow above 0x1.62e42ep6, zero below -0x1.9fe368p6)
__host__ __device__ __forceinline__ float jd_mlp_expf(float x, const unsigned long long *tab)
{
    if (!(x <= 0x1.62e42ep6f)) return x > 0.0f ? __builtin_inff() : x + x;
    if (x < -0x1.9fe368p6f) return 0.0f;
    return jd_expf_impl(x, tab);
}
// the policy of jd_mlp_forward_row on the host: the replicas the kernel runs
struct JdMlpHostMath {
    JdLogTab tab[129];
    JdMlpHostMath() { jd_fill_logtab(tab); }
    float exp(float x) const { return jd_mlp_expf(x, jd_exp2f_tab_host); }
    float log_add(float a, float c) const { return jd_log_add_impl(a, c, tab, jd_exp2f_tab_host, jd_log_tab_host); }
};

#define JD_MLP_OUT_LL 0             // out [n_rows][n_phones]: (z - logZ) - log_prior; 0.0f for unused rows
#define JD_MLP_OUT_LOGPOST 1        // z - logZ
#define JD_MLP_OUT_LAYER 2          // out [n_rows][width[layer]]: the activations behind `layer` (raw logits for the last)

__device__ __forceinline__ float jd_mlp_activate(float y, int act)
{
    if (act == JD_ACT_RELU) return y > 0.0f ? y : 0.0f;
    if (act == JD_ACT_SIGMOID) return 1.0f / (1.0f + jd_mlp_expf(-y, jd_exp2f_tab));
    return y;
}

// an accumulator tile (column lane & 15, rows 4 (lane >> 4) + reg) into the next layer's operand / the logits
__device__ __forceinline__ void jd_mlp_store_tile(const jd_mlp_f4 acc, int nt, int N, int act, bool last, float *dst, int S, int lane)
{
    const int j = nt * JD_MLP_NT + (lane & 15), q = lane >> 4;
    const int col = last ? j : jd_mlp_act_pos(j);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const float v = acc[reg];
        if (last) { if (j < N) dst[(4 * q + reg) * S + col] = v; }
        else dst[(4 * q + reg) * S + col] = (j < N) ? jd_mlp_activate(v, act) : -0.0f;
    }
}

// The chains of one n tile (TWO: of a pair) over a layer's KG k groups: c = fma(a[k], b[k], c), k ascending.  ap: the lane's
// activations (16 bytes a k group, 64 bytes apart), w0 / w1: its packed weights (16 bytes a k group, 1 KB apart).  The operands
// of the next JD_MLP_CH k groups are requested before the current ones are multiplied, so that a wave waits for memory once a layer
// and not once a k group; a request behind the last k group repeats the last one (in bounds) and is not used.
#define JD_MLP_CH 2
template <bool TWO>
__device__ __forceinline__ void jd_mlp_chain(const jd_mlp_f4 *__restrict__ ap, const jd_mlp_f4 *__restrict__ w0, const jd_mlp_f4 *__restrict__ w1,
                                             int KG, jd_mlp_f4 &c0, jd_mlp_f4 &c1)
{
    jd_mlp_f4 a[JD_MLP_CH], b0[JD_MLP_CH], b1[JD_MLP_CH], an[JD_MLP_CH], b0n[JD_MLP_CH], b1n[JD_MLP_CH];
#pragma unroll
    for (int i = 0; i < JD_MLP_CH; ++i) {
        const int k = min(i, KG - 1);
        a[i] = ap[k * 4]; b0[i] = w0[k * 64];
        if (TWO) b1[i] = w1[k * 64];
    }
    for (int kg0 = 0; kg0 < KG; kg0 += JD_MLP_CH) {
#pragma unroll
        for (int i = 0; i < JD_MLP_CH; ++i) {
            const int k = min(kg0 + JD_MLP_CH + i, KG - 1);
            an[i] = ap[k * 4]; b0n[i] = w0[k * 64];
            if (TWO) b1n[i] = w1[k * 64];
        }
#pragma unroll
        for (int i = 0; i < JD_MLP_CH; ++i) {
            if (kg0 + i < KG) {                                        // (wave-uniform)
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b0[i].x, c0, 0, 0, 0);
                if (TWO) c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b1[i].x, c1, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b0[i].y, c0, 0, 0, 0);
                if (TWO) c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b1[i].y, c1, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b0[i].z, c0, 0, 0, 0);
                if (TWO) c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b1[i].z, c1, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b0[i].w, c0, 0, 0, 0);
                if (TWO) c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b1[i].w, c1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < JD_MLP_CH; ++i) { a[i] = an[i]; b0[i] = b0n[i]; if (TWO) b1[i] = b1n[i]; }
    }
}

// The input stage of a spliced tile: pieces outside, d inside - a wave takes a piece (row r, frame c of its window: wave-uniform, one
// division a piece and none an element), its lanes the piece's D contiguous values.  An unused row is 0.0f and reads nothing; the
// padding behind in_dim is -0 as ever.  sspan: the tile's spans (LDS).  (D, left, right, K by value: the kernel's argument m stays in
// the kernel-argument segment - a reference to it would make a private copy)
__device__ __forceinline__ void jd_mlp_stage_spliced(const float *__restrict__ feats, const int *ssrc, const JdSpan *sspan, int D, int left, int right,
                                                     int K, float *buf0, int S, int tid, int lane, int wid)
{
    const int C = left + right + 1, pad = ((K + 15) & ~15) - K;
    for (int p = wid; p < JD_MLP_ROWS * C; p += 4) {                   // (wave-uniform)
        const int r = p / C, c = p - r * C;
        const int src = ssrc[r];
        float *dst = buf0 + r * S;
        if (src >= 0) {
            const float *f = feats + (size_t)jd_splice_frame(src, c, left, sspan[r]) * D;
            for (int d = lane; d < D; d += 64) dst[jd_mlp_act_pos(c * D + d)] = f[d];
        } else
            for (int d = lane; d < D; d += 64) dst[jd_mlp_act_pos(c * D + d)] = 0.0f;
    }
    for (int e = tid; e < JD_MLP_ROWS * pad; e += 256) {
        const int r = e / pad, k = K + (e - r * pad);
        buf0[r * S + jd_mlp_act_pos(k)] = -0.0f;
    }
}

template <bool SPL>
__global__ __launch_bounds__(256) void jd_mlp_kernel_t(const float *__restrict__ feats, const int *__restrict__ row_src, int n_rows,
                                                       const float *__restrict__ wp, const float *__restrict__ bp,
                                                       const float *__restrict__ log_prior, const JdLogTab *__restrict__ logtab,
                                                       const JdMlpDev m, float *__restrict__ out, int out_mode, int layer,
                                                       const JdSpan *__restrict__ span)
{
    extern __shared__ __align__(16) char smem[];
    const int S = m.stride;
    float *buf0 = (float *)smem, *buf1 = buf0 + JD_MLP_ROWS * S;      // [16][S] each
    int *ssrc = (int *)(buf1 + JD_MLP_ROWS * S);                       // [16] the tile's row_src (-1 behind n_rows)
    float *slz = (float *)(ssrc + JD_MLP_ROWS);                        // [16] logZ
    JdSpan *sspan = (JdSpan *)(slz + JD_MLP_ROWS);                     // SPL: [16] the tile's spans
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int P = m.width[m.n_layers - 1];
    const int n_rt = (n_rows + JD_MLP_ROWS - 1) / JD_MLP_ROWS;
    for (int rt = blockIdx.x; rt < n_rt; rt += gridDim.x) {
        const int r0 = rt * JD_MLP_ROWS;
        __syncthreads();                                               // the previous tile's readers are done
        if (tid < JD_MLP_ROWS) ssrc[tid] = (r0 + tid < n_rows) ? row_src[r0 + tid] : -1;
        if (SPL && tid < JD_MLP_ROWS && r0 + tid < n_rows) sspan[tid] = span[r0 + tid];
        __syncthreads();
        bool any = false;
#pragma unroll
        for (int r = 0; r < JD_MLP_ROWS; ++r) any |= ssrc[r] >= 0;
        if (!any) {                                                    // (workgroup-uniform)
            if (out_mode == JD_MLP_OUT_LL)
                for (int e = tid; e < JD_MLP_ROWS * P; e += 256) {
                    const int r = e / P;
                    if (r0 + r < n_rows) out[(size_t)(r0 + r) * P + (e - r * P)] = 0.0f;
                }
            continue;
        }
        if (SPL) jd_mlp_stage_spliced(feats, ssrc, sspan, m.base_dim, m.left, m.right, m.in_dim, buf0, S, tid, lane, wid);
        else {   // the input rows, padded with -0 to the k group
            const int K = m.in_dim, Kp = (K + 15) & ~15;
            for (int e = tid; e < JD_MLP_ROWS * Kp; e += 256) {
                const int r = e / Kp, k = e - r * Kp;
                const int src = ssrc[r];
                buf0[r * S + jd_mlp_act_pos(k)] = (k < K) ? (src >= 0 ? feats[(size_t)src * K + k] : 0.0f) : -0.0f;
            }
        }
        __syncthreads();
        float *in = buf0, *nx = buf1;
        bool done = false;
        for (int l = 0; l < m.n_layers && !done; ++l) {
            const int K = l ? m.width[l - 1] : m.in_dim, KG = (K + 15) >> 4, N = m.width[l], n_nt = (N + 15) >> 4;
            const bool last = l == m.n_layers - 1;
            const int act = m.act[l];
            const float *B = bp + m.b_off[l];
            const jd_mlp_f4 *W = (const jd_mlp_f4 *)(wp + m.w_off[l]) + lane;          // (n tile, k group): 64 lanes x 16 bytes
            const jd_mlp_f4 *ap = (const jd_mlp_f4 *)(in + (lane & 15) * S + 4 * (lane >> 4));
            for (int nt0 = wid * 2; nt0 < n_nt; nt0 += 8) {                            // (wave-uniform)
                const bool two = nt0 + 1 < n_nt;
                const float bias0 = B[nt0 * JD_MLP_NT + (lane & 15)];
                const float bias1 = two ? B[(nt0 + 1) * JD_MLP_NT + (lane & 15)] : 0.0f;
                jd_mlp_f4 c0 = {bias0, bias0, bias0, bias0}, c1 = {bias1, bias1, bias1, bias1};
                const jd_mlp_f4 *w0 = W + (size_t)nt0 * KG * 64;
                if (two) jd_mlp_chain<true>(ap, w0, w0 + (size_t)KG * 64, KG, c0, c1);
                else jd_mlp_chain<false>(ap, w0, w0, KG, c0, c1);
                jd_mlp_store_tile(c0, nt0, N, act, last, nx, S, lane);
                if (two) jd_mlp_store_tile(c1, nt0 + 1, N, act, last, nx, S, lane);
            }
            __syncthreads();
            if (out_mode == JD_MLP_OUT_LAYER && l == layer) {
                for (int e = tid; e < JD_MLP_ROWS * N; e += 256) {
                    const int r = e / N, j = e - r * N;
                    if (r0 + r < n_rows) out[(size_t)(r0 + r) * N + j] = nx[r * S + (last ? j : jd_mlp_act_pos(j))];
                }
                done = true;
            }
            float *t = in; in = nx; nx = t;
        }
        if (done) continue;
        // `in` holds the logits [16][S], plain order
        if (tid < JD_MLP_ROWS) {
            float lz = LZ;
            for (int j = 0; j < P; ++j) lz = jd_log_add(lz, in[tid * S + j], logtab);
            slz[tid] = lz;
        }
        __syncthreads();
        for (int e = tid; e < JD_MLP_ROWS * P; e += 256) {
            const int r = e / P, j = e - r * P;
            if (r0 + r < n_rows) {
                const float lp = in[r * S + j] - slz[r];
                out[(size_t)(r0 + r) * P + j] = (ssrc[r] < 0) ? 0.0f : (out_mode == JD_MLP_OUT_LL ? lp - log_prior[j] : lp);
            }
        }
    }
}

// ---- tied models (jd_am_create_mlp_tied): the same tile of 16 rows through the same hidden layers - ping-pong activations in LDS,
// jd_mlp_chain, K never split - and an OUTPUT layer of up to JD_MLP_MAX_OUT = 16384 tied states, whose logits do not fit in LDS
// (16 x 16384 floats = 1 MB).  They go to the tile's own rows of `out`: those rows are this launch's alone (launch_gmm keeps no
// memory of its own), and the same workgroup normalises them in place.  m = jd_mlp_dev(desc, true): its stride covers in_dim and the
// hidden widths; during the output layer only the layer's input buffer is read.
//
// logZ (jd_mlp.h: JD_MLP_LZ_CHAINS = 128 interleaved partial chains, then the chain of the partials).  A workgroup's four waves
// cover 8 n tiles = 128 outputs a turn: wave w takes tiles 2 w + 8 t and 2 w + 1 + 8 t, so a lane's two accumulator columns are
// always outputs j = 32 w + (lane & 15) (+ 16) mod 128 - chains that belong to this lane alone, met in ascending order.  The partials
// of its 4 rows x 2 chains stay in registers beside the accumulators, one logAdd per logit as it leaves the MFMA; outputs at or
// beyond P are not added and a chain c >= P stays empty.  The partials go to LDS [16][128], lane r of the first wave runs row r's chain
// over them (128 steps: serial by definition), and all threads read the tile's logits back and write (z - logZ) - log_prior.
// The logits are kept in memory whatever the width: the result does not depend on where they were held.
static constexpr auto jd_mlp_kernel = jd_mlp_kernel_t<false>;
static constexpr auto jd_mlp_spliced_kernel = jd_mlp_kernel_t<true>;

template <bool SPL>
__global__ __launch_bounds__(256) void jd_mlp_tied_kernel_t(const float *__restrict__ feats, const int *__restrict__ row_src, int n_rows,
                                                            const float *__restrict__ wp, const float *__restrict__ bp,
                                                            const float *__restrict__ log_prior, const JdLogTab *__restrict__ logtab,
                                                            const JdMlpDev m, float *out, int out_mode, int layer,
                                                            const JdSpan *__restrict__ span)
{
    extern __shared__ __align__(16) char smem[];
    const int S = m.stride;
    float *buf0 = (float *)smem, *buf1 = buf0 + JD_MLP_ROWS * S;      // [16][S] each
    int *ssrc = (int *)(buf1 + JD_MLP_ROWS * S);                       // [16] the tile's row_src (-1 behind n_rows)
    float *slz = (float *)(ssrc + JD_MLP_ROWS);                        // [16] logZ
    float *sp = slz + JD_MLP_ROWS;                                     // [16][JD_MLP_LZ_CHAINS] the partial chains
    JdSpan *sspan = (JdSpan *)(sp + JD_MLP_ROWS * JD_MLP_LZ_CHAINS);   // SPL: [16] the tile's spans
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = m.n_layers, P = m.width[L - 1];
    const int n_rt = (n_rows + JD_MLP_ROWS - 1) / JD_MLP_ROWS;
    for (int rt = blockIdx.x; rt < n_rt; rt += gridDim.x) {
        const int r0 = rt * JD_MLP_ROWS;
        const int rows = min(JD_MLP_ROWS, n_rows - r0);                // the tile's rows inside the table: nothing behind them is touched
        __syncthreads();                                               // the previous tile's readers are done
        if (tid < JD_MLP_ROWS) ssrc[tid] = (tid < rows) ? row_src[r0 + tid] : -1;
        if (SPL && tid < rows) sspan[tid] = span[r0 + tid];
        __syncthreads();
        bool any = false;
#pragma unroll
        for (int r = 0; r < JD_MLP_ROWS; ++r) any |= ssrc[r] >= 0;
        if (!any) {                                                    // (workgroup-uniform)
            if (out_mode == JD_MLP_OUT_LL)
                for (int r = 0; r < rows; ++r)
                    for (int j = tid; j < P; j += 256) out[(size_t)(r0 + r) * P + j] = 0.0f;
            continue;
        }
        if (SPL) jd_mlp_stage_spliced(feats, ssrc, sspan, m.base_dim, m.left, m.right, m.in_dim, buf0, S, tid, lane, wid);
        else {   // the input rows, padded with -0 to the k group
            const int K = m.in_dim, Kp = (K + 15) & ~15;
            for (int e = tid; e < JD_MLP_ROWS * Kp; e += 256) {
                const int r = e / Kp, k = e - r * Kp;
                const int src = ssrc[r];
                buf0[r * S + jd_mlp_act_pos(k)] = (k < K) ? (src >= 0 ? feats[(size_t)src * K + k] : 0.0f) : -0.0f;
            }
        }
        __syncthreads();
        float *in = buf0, *nx = buf1;
        bool done = false;
        for (int l = 0; l < L - 1 && !done; ++l) {                     // the hidden layers, as jd_mlp_kernel runs them
            const int K = l ? m.width[l - 1] : m.in_dim, KG = (K + 15) >> 4, N = m.width[l], n_nt = (N + 15) >> 4;
            const int act = m.act[l];
            const float *B = bp + m.b_off[l];
            const jd_mlp_f4 *W = (const jd_mlp_f4 *)(wp + m.w_off[l]) + lane;
            const jd_mlp_f4 *ap = (const jd_mlp_f4 *)(in + (lane & 15) * S + 4 * (lane >> 4));
            for (int nt0 = wid * 2; nt0 < n_nt; nt0 += 8) {                            // (wave-uniform)
                const bool two = nt0 + 1 < n_nt;
                const float bias0 = B[nt0 * JD_MLP_NT + (lane & 15)];
                const float bias1 = two ? B[(nt0 + 1) * JD_MLP_NT + (lane & 15)] : 0.0f;
                jd_mlp_f4 c0 = {bias0, bias0, bias0, bias0}, c1 = {bias1, bias1, bias1, bias1};
                const jd_mlp_f4 *w0 = W + (size_t)nt0 * KG * 64;
                if (two) jd_mlp_chain<true>(ap, w0, w0 + (size_t)KG * 64, KG, c0, c1);
                else jd_mlp_chain<false>(ap, w0, w0, KG, c0, c1);
                jd_mlp_store_tile(c0, nt0, N, act, false, nx, S, lane);
                if (two) jd_mlp_store_tile(c1, nt0 + 1, N, act, false, nx, S, lane);
            }
            __syncthreads();
            if (out_mode == JD_MLP_OUT_LAYER && l == layer) {
                for (int e = tid; e < JD_MLP_ROWS * N; e += 256) {
                    const int r = e / N, j = e - r * N;
                    if (r < rows) out[(size_t)(r0 + r) * N + j] = nx[r * S + jd_mlp_act_pos(j)];
                }
                done = true;
            }
            float *t = in; in = nx; nx = t;
        }
        if (done) continue;
        {   // the output layer: logits to the tile's rows of out, the partial chains in registers
            const int K = L > 1 ? m.width[L - 2] : m.in_dim, KG = (K + 15) >> 4, n_nt = (P + 15) >> 4;
            const float *B = bp + m.b_off[L - 1];
            const jd_mlp_f4 *W = (const jd_mlp_f4 *)(wp + m.w_off[L - 1]) + lane;
            const jd_mlp_f4 *ap = (const jd_mlp_f4 *)(in + (lane & 15) * S + 4 * (lane >> 4));
            const int col = lane & 15, q = lane >> 4;
            const bool raw = out_mode == JD_MLP_OUT_LAYER;             // (layer = L - 1: the raw logits are the result)
            float pz0[4] = {LZ, LZ, LZ, LZ}, pz1[4] = {LZ, LZ, LZ, LZ};
            for (int nt0 = wid * 2; nt0 < n_nt; nt0 += 8) {                            // (wave-uniform)
                const bool two = nt0 + 1 < n_nt;
                const int j0 = nt0 * JD_MLP_NT + col, j1 = j0 + JD_MLP_NT;
                const float bias0 = B[j0];                                             // (biases are padded to the n tile)
                const float bias1 = two ? B[j1] : 0.0f;
                jd_mlp_f4 c0 = {bias0, bias0, bias0, bias0}, c1 = {bias1, bias1, bias1, bias1};
                const jd_mlp_f4 *w0 = W + (size_t)nt0 * KG * 64;
                if (two) jd_mlp_chain<true>(ap, w0, w0 + (size_t)KG * 64, KG, c0, c1);
                else jd_mlp_chain<false>(ap, w0, w0, KG, c0, c1);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int r = 4 * q + reg;
                    if (j0 < P) {
                        if (r < rows) out[(size_t)(r0 + r) * P + j0] = c0[reg];
                        if (!raw) pz0[reg] = jd_log_add(pz0[reg], c0[reg], logtab);
                    }
                    if (two && j1 < P) {
                        if (r < rows) out[(size_t)(r0 + r) * P + j1] = c1[reg];
                        if (!raw) pz1[reg] = jd_log_add(pz1[reg], c1[reg], logtab);
                    }
                }
            }
            if (raw) continue;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                sp[(4 * q + reg) * JD_MLP_LZ_CHAINS + wid * 32 + col] = pz0[reg];
                sp[(4 * q + reg) * JD_MLP_LZ_CHAINS + wid * 32 + 16 + col] = pz1[reg];
            }
        }
        __syncthreads();                                               // the partials (LDS) are there
        if (tid < JD_MLP_ROWS) {
            const int C = min(P, JD_MLP_LZ_CHAINS);
            float lz = LZ;
            for (int c = 0; c < C; ++c) lz = jd_log_add(lz, sp[tid * JD_MLP_LZ_CHAINS + c], logtab);
            slz[tid] = lz;
        }
        // This barrier is also what makes the tile's logits - written to `out` by other lanes of this workgroup - visible to the reads
        // below: __syncthreads() is a workgroup-scope release / acquire fence around s_barrier (every wave waits for its own stores,
        // vmcnt(0), before it arrives), and a workgroup's waves share one CU and its vector L1, which writes through.  Nothing wider
        // is needed: no other workgroup reads or writes these rows during the launch.
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const float lz = slz[r];
            const bool unused = ssrc[r] < 0;
            float *o = out + (size_t)(r0 + r) * P;
            for (int j = tid; j < P; j += 256) {
                const float lp = o[j] - lz;
                o[j] = unused ? 0.0f : (out_mode == JD_MLP_OUT_LL ? lp - log_prior[j] : lp);
            }
        }
    }
}

static constexpr auto jd_mlp_tied_kernel = jd_mlp_tied_kernel_t<false>;
static constexpr auto jd_mlp_tied_spliced_kernel = jd_mlp_tied_kernel_t<true>;
