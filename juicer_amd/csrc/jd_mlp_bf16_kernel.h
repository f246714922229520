// jd_mlp_bf16_kernel.h - the forward pass of a bf16 neural acoustic model (jd_am_mlp_to_bf16) on the device (included by jd_device.hip
// behind jd_mlp_kernel.h; gfx950 only): jd_mlp_bf16_kernel for phone models, jd_mlp_tied_bf16_kernel for tied ones - the two
// instantiations of jd_mlp_bf16_kernel_t<TIED>, which differ in the logZ stage alone.  A workgroup takes a
// tile of JD_MLP_BF16_ROWS = 32 rows of a likelihood table through ALL layers - linear layers on v_mfma_f32_16x16x32_bf16, activations,
// log-softmax, minus the log priors - and writes only its rows of the table.  The numerics contract, the tile, the LDS layout with the
// choice of its row padding and the packing of the weights are jd_mlp_bf16.h's.
//
// Fused for jd_mlp_kernel's reason: launch_gmm has no memory of its own.  The activations live in LDS as bf16, two buffers
// [32][stride] that the layers fill in turn, in natural k order: a lane's A operand of a k group of 32 inputs is one 16-byte read.
//
// A workgroup is four waves.  A wave takes PAIRS of n tiles (16 outputs each; the packing pads N to 32, so there is always a pair)
// for BOTH row tiles of 16: four independent accumulators, two A reads and two B loads per k group - every weight is fetched once for
// 32 rows, half the bytes of an f32 weight for twice the rows of jd_mlp_kernel's tile.  Per k group a lane reads 2 x 16 bytes of
// activations from LDS and 16 bytes of each n tile's packed weights from memory (1 KB contiguous per wave), JD_MLP_BF16_CH k groups ahead
// of their use, then issues four MFMAs; C-in of the first is the bias.  One accumulator per output, k groups ascending, for every
// launch: a row's result depends on that row alone.  Every padded activation and weight is a written +0.
//
// An accumulator leaves as activation -> jd_bf16_round -> 16 bits in LDS (hidden layers), or as an f32 logit in the tile's own rows
// of `out` (the last layer: 32 x 1024 floats do not fit in LDS beside the buffers).  Those rows are this launch's alone, and the same
// workgroup normalises them in place: the serial logAdd chain (lane r of the first wave runs row r's) for phone models, for tied
// ones jd_mlp_tied_kernel's 128 interleaved chains - wave w takes n tiles 2 w + 8 t and 2 w + 1 + 8 t, so a lane's two accumulator
// columns are outputs 32 w + (lane & 15) (+ 16) modulo 128, chains that belong to this lane alone and meet their elements in ascending
// order; the partials of its 8 rows x 2 chains stay in registers, go to LDS [32][128], and lane r of the first wave chains them.
// A row with row_src < 0 is written 0.0f; a tile without a used row does no arithmetic; rows at or behind n_rows are never touched.
//
// SPLICED models (jd_am_mlp_splice, jd_splice.h): the SPL = true instantiations, jd_mlp_bf16_spliced_kernel / jd_mlp_tied_bf16_spliced_kernel,
// differ in the input stage alone, as jd_mlp_kernel.h's do: the tile keeps its rows' spans beside ssrc and gathers C pieces of D values a
// row, rounded to bf16 as they land.  The SPL = false ones read neither `span` nor the context.
#pragma once

typedef __bf16 jd_mlp_bf8 __attribute__((ext_vector_type(8)));
#define JD_MLP_BF16_CH 4           // k groups requested ahead: 4 x 2 KB of weights in flight per wave (one wave per SIMD: nothing else hides memory)

// The sums of a PAIR of n tiles for both row tiles over a layer's KG k groups.  a0 / a1: the lane's activations of the two row
// tiles (16 bytes a k group, 64 bytes apart), w0 / w1: its packed weights of the two n tiles (16 bytes a k group, 1 KB apart).
// c[2 mt + nt].  The operands of the next JD_MLP_BF16_CH k groups are requested before the current ones are multiplied (jd_mlp_chain); a
// request behind the last k group repeats the last one (in bounds) and is not used.
__device__ __forceinline__ void jd_mlp_bf16_chain(const jd_mlp_bf8 *__restrict__ a0, const jd_mlp_bf8 *__restrict__ a1,
                                                  const jd_mlp_bf8 *__restrict__ w0, const jd_mlp_bf8 *__restrict__ w1, int KG, jd_mlp_f4 (&c)[4])
{
    jd_mlp_bf8 x0[JD_MLP_BF16_CH], x1[JD_MLP_BF16_CH], b0[JD_MLP_BF16_CH], b1[JD_MLP_BF16_CH], x0n[JD_MLP_BF16_CH], x1n[JD_MLP_BF16_CH], b0n[JD_MLP_BF16_CH], b1n[JD_MLP_BF16_CH];
#pragma unroll
    for (int i = 0; i < JD_MLP_BF16_CH; ++i) {
        const int k = min(i, KG - 1);
        x0[i] = a0[k * 4]; x1[i] = a1[k * 4]; b0[i] = w0[k * 64]; b1[i] = w1[k * 64];
    }
    for (int kg0 = 0; kg0 < KG; kg0 += JD_MLP_BF16_CH) {
#pragma unroll
        for (int i = 0; i < JD_MLP_BF16_CH; ++i) {
            const int k = min(kg0 + JD_MLP_BF16_CH + i, KG - 1);
            x0n[i] = a0[k * 4]; x1n[i] = a1[k * 4]; b0n[i] = w0[k * 64]; b1n[i] = w1[k * 64];
        }
#pragma unroll
        for (int i = 0; i < JD_MLP_BF16_CH; ++i) {
            if (kg0 + i < KG) {                                        // (wave-uniform)
                c[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x0[i], b0[i], c[0], 0, 0, 0);
                c[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x0[i], b1[i], c[1], 0, 0, 0);
                c[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x1[i], b0[i], c[2], 0, 0, 0);
                c[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x1[i], b1[i], c[3], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < JD_MLP_BF16_CH; ++i) { x0[i] = x0n[i]; x1[i] = x1n[i]; b0[i] = b0n[i]; b1[i] = b1n[i]; }
    }
}

// (one body, two kernels: jd_mlp_bf16_kernel and jd_mlp_tied_bf16_kernel are its instantiations, named at the end of this file.  m is
// the kernel's own argument - read from the kernel-argument segment with scalar loads, not through a private copy)
template <bool TIED, bool SPL>
__global__ __launch_bounds__(256) void jd_mlp_bf16_kernel_t(const float *__restrict__ feats, const int *__restrict__ row_src, int n_rows,
                                                            const unsigned short *__restrict__ wp, const float *__restrict__ bp,
                                                            const float *__restrict__ log_prior, const JdLogTab *__restrict__ logtab,
                                                            const JdMlpDev m, float *out, int out_mode, int layer,
                                                            const JdSpan *__restrict__ span)
{
    extern __shared__ __align__(16) char smem[];
    constexpr int R = JD_MLP_BF16_ROWS;
    const int S = m.stride;                                            // 16-bit elements; 16 modulo 128
    unsigned short *buf0 = (unsigned short *)smem, *buf1 = buf0 + R * S;              // [32][S] each
    int *ssrc = (int *)(buf1 + R * S);                                 // [32] the tile's row_src (-1 behind n_rows)
    float *slz = (float *)(ssrc + R);                                  // [32] logZ
    float *sp = slz + R;                                               // TIED: [32][JD_MLP_LZ_CHAINS] the partial chains
    JdSpan *sspan = (JdSpan *)(TIED ? sp + R * JD_MLP_LZ_CHAINS : sp); // SPL: [32] the tile's spans
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, q = lane >> 4;
    const int L = m.n_layers, P = m.width[L - 1];
    const int n_rt = (n_rows + R - 1) / R;
    for (int rt = blockIdx.x; rt < n_rt; rt += gridDim.x) {
        const int r0 = rt * R;
        const int rows = min(R, n_rows - r0);                          // the tile's rows inside the table: nothing behind them is touched
        __syncthreads();                                               // the previous tile's readers are done
        if (tid < R) ssrc[tid] = (tid < rows) ? row_src[r0 + tid] : -1;
        if (SPL && tid < rows) sspan[tid] = span[r0 + tid];
        __syncthreads();
        bool any = false;
#pragma unroll
        for (int r = 0; r < R; ++r) any |= ssrc[r] >= 0;
        if (!any) {                                                    // (workgroup-uniform)
            if (out_mode == JD_MLP_OUT_LL)
                for (int r = 0; r < rows; ++r)
                    for (int j = tid; j < P; j += 256) out[(size_t)(r0 + r) * P + j] = 0.0f;
            continue;
        }
        if (SPL) {   // pieces outside, d inside (jd_mlp_stage_spliced): a wave takes a piece, its lanes the piece's D contiguous values
            const int D = m.base_dim, left = m.left, C = left + m.right + 1, K = m.in_dim, pad = ((K + 31) & ~31) - K;
            for (int p = wid; p < R * C; p += 4) {                     // (wave-uniform)
                const int r = p / C, c = p - r * C;
                const int src = ssrc[r];
                unsigned short *dst = buf0 + r * S + c * D;
                if (src >= 0) {
                    const float *f = feats + (size_t)jd_splice_frame(src, c, left, sspan[r]) * D;
                    for (int d = lane; d < D; d += 64) dst[d] = jd_bf16_bits(f[d]);
                } else
                    for (int d = lane; d < D; d += 64) dst[d] = (unsigned short)0;
            }
            for (int e = tid; e < R * pad; e += 256) {
                const int r = e / pad;
                buf0[r * S + K + (e - r * pad)] = (unsigned short)0;
            }
        } else {   // the input rows as bf16, padded with +0 to the k group; an unused row is +0 throughout
            const int K = m.in_dim, Kp = (K + 31) & ~31;
            for (int e = tid; e < R * Kp; e += 256) {
                const int r = e / Kp, k = e - r * Kp;
                const int src = ssrc[r];
                buf0[r * S + k] = (k < K && src >= 0) ? jd_bf16_bits(feats[(size_t)src * K + k]) : (unsigned short)0;
            }
        }
        __syncthreads();
        unsigned short *in = buf0, *nx = buf1;
        bool done = false;
        for (int l = 0; l < L - 1 && !done; ++l) {                     // the hidden layers
            const int K = l ? m.width[l - 1] : m.in_dim, KG = (K + 31) >> 5, N = m.width[l], n_nt = ((N + 31) >> 5) * 2;
            const int act = m.act[l];
            const float *B = bp + m.b_off[l];
            const jd_mlp_bf8 *W = (const jd_mlp_bf8 *)(wp + m.w_off[l]) + lane;       // (n tile, k group): 64 lanes x 16 bytes
            const jd_mlp_bf8 *a0 = (const jd_mlp_bf8 *)(in + col * S + 8 * q), *a1 = (const jd_mlp_bf8 *)(in + (16 + col) * S + 8 * q);
            for (int nt0 = wid * 2; nt0 < n_nt; nt0 += 8) {                           // (wave-uniform)
                const int j0 = nt0 * JD_MLP_BF16_NT + col, j1 = j0 + JD_MLP_BF16_NT;
                const float bias0 = B[j0], bias1 = B[j1];                             // (biases are padded to the pair)
                jd_mlp_f4 c[4] = {{bias0, bias0, bias0, bias0}, {bias1, bias1, bias1, bias1}, {bias0, bias0, bias0, bias0}, {bias1, bias1, bias1, bias1}};
                const jd_mlp_bf8 *w0 = W + (size_t)nt0 * KG * 64;
                jd_mlp_bf16_chain(a0, a1, w0, w0 + (size_t)KG * 64, KG, c);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int r = 16 * mt + 4 * q + reg;
                        nx[r * S + j0] = (j0 < N) ? jd_bf16_bits(jd_mlp_activate(c[2 * mt][reg], act)) : (unsigned short)0;
                        nx[r * S + j1] = (j1 < N) ? jd_bf16_bits(jd_mlp_activate(c[2 * mt + 1][reg], act)) : (unsigned short)0;
                    }
            }
            __syncthreads();
            if (out_mode == JD_MLP_OUT_LAYER && l == layer) {
                for (int e = tid; e < R * N; e += 256) {
                    const int r = e / N, j = e - r * N;
                    if (r < rows) out[(size_t)(r0 + r) * N + j] = jd_bf16_u2f((uint32_t)nx[r * S + j] << 16);
                }
                done = true;
            }
            unsigned short *t = in; in = nx; nx = t;
        }
        if (done) continue;
        const bool raw = out_mode == JD_MLP_OUT_LAYER;                 // (layer = L - 1: the raw logits are the result)
        {   // the output layer: logits to the tile's rows of out; TIED: the partial chains in registers
            const int K = L > 1 ? m.width[L - 2] : m.in_dim, KG = (K + 31) >> 5, n_nt = ((P + 31) >> 5) * 2;
            const float *B = bp + m.b_off[L - 1];
            const jd_mlp_bf8 *W = (const jd_mlp_bf8 *)(wp + m.w_off[L - 1]) + lane;
            const jd_mlp_bf8 *a0 = (const jd_mlp_bf8 *)(in + col * S + 8 * q), *a1 = (const jd_mlp_bf8 *)(in + (16 + col) * S + 8 * q);
            float pz[4][4] = {{LZ, LZ, LZ, LZ}, {LZ, LZ, LZ, LZ}, {LZ, LZ, LZ, LZ}, {LZ, LZ, LZ, LZ}};       // [2 mt + nt][reg]
            for (int nt0 = wid * 2; nt0 < n_nt; nt0 += 8) {                           // (wave-uniform)
                const int j0 = nt0 * JD_MLP_BF16_NT + col, j1 = j0 + JD_MLP_BF16_NT;
                const float bias0 = B[j0], bias1 = B[j1];
                jd_mlp_f4 c[4] = {{bias0, bias0, bias0, bias0}, {bias1, bias1, bias1, bias1}, {bias0, bias0, bias0, bias0}, {bias1, bias1, bias1, bias1}};
                const jd_mlp_bf8 *w0 = W + (size_t)nt0 * KG * 64;
                jd_mlp_bf16_chain(a0, a1, w0, w0 + (size_t)KG * 64, KG, c);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int r = 16 * mt + 4 * q + reg;
                        if (j0 < P) {
                            if (r < rows) out[(size_t)(r0 + r) * P + j0] = c[2 * mt][reg];
                            if (TIED && !raw) pz[2 * mt][reg] = jd_log_add(pz[2 * mt][reg], c[2 * mt][reg], logtab);
                        }
                        if (j1 < P) {
                            if (r < rows) out[(size_t)(r0 + r) * P + j1] = c[2 * mt + 1][reg];
                            if (TIED && !raw) pz[2 * mt + 1][reg] = jd_log_add(pz[2 * mt + 1][reg], c[2 * mt + 1][reg], logtab);
                        }
                    }
            }
            if (raw) continue;
            if (TIED) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int r = 16 * mt + 4 * q + reg;
                        sp[r * JD_MLP_LZ_CHAINS + wid * 32 + col] = pz[2 * mt][reg];
                        sp[r * JD_MLP_LZ_CHAINS + wid * 32 + 16 + col] = pz[2 * mt + 1][reg];
                    }
            }
        }
        // This barrier makes the partials (LDS) and the tile's logits - written to `out` by other lanes of this workgroup - visible to
        // the reads below: __syncthreads() is a workgroup-scope release / acquire fence around the barrier (every wave waits for its
        // own stores before it arrives), and a workgroup's waves share one CU and its vector L1, which writes through.  Nothing wider
        // is needed: no other workgroup reads or writes these rows during the launch (jd_mlp_tied_kernel).
        __syncthreads();
        if (tid < rows) {
            float lz = LZ;
            if (TIED) {
                const int C = min(P, JD_MLP_LZ_CHAINS);
                for (int c = 0; c < C; ++c) lz = jd_log_add(lz, sp[tid * JD_MLP_LZ_CHAINS + c], logtab);
            } else {
                const float *o = out + (size_t)(r0 + tid) * P;
                for (int j = 0; j < P; ++j) lz = jd_log_add(lz, o[j], logtab);
            }
            slz[tid] = lz;
        }
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

static constexpr auto jd_mlp_bf16_kernel = jd_mlp_bf16_kernel_t<false, false>;
static constexpr auto jd_mlp_tied_bf16_kernel = jd_mlp_bf16_kernel_t<true, false>;
static constexpr auto jd_mlp_bf16_spliced_kernel = jd_mlp_bf16_kernel_t<false, true>;
static constexpr auto jd_mlp_tied_bf16_spliced_kernel = jd_mlp_bf16_kernel_t<true, true>;
