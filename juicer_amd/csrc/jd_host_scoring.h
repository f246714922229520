// jd_host_scoring.h - the host side of the companion scoring kernels (included by jd_device.hip): the model parameters on the device,
// launch_gmm - the launch of what jd_score_plan.h plans: which kernel (jd_gmm_kernel39, the default; jd_gmm_fast39 / jd_gmm_fast,
// jd_dec_set_scoring's option; the generic and the hybrid kernel; jd_mlp_kernel for the models of jd_am_create_mlp, jd_mlp_tied_kernel for
// those of jd_am_create_mlp_tied, their bf16 kernels, and the spliced flavours of the four for jd_am_mlp_splice's models, whose rows carry
// a span beside row_src - jd_splice.h), its tiles, grid and
// LDS are decided there, on plain data, and tested on the CPU - jd_am_score_frames, jd_am_mlp_forward.  Reference: HTKFlatModels::calcGMMOutput + logAdd, src/HTKFlatModels.cpp:190-293.
#pragma once

// hybrid scoring (HTKFlatModels.cpp:190-222): output = x[model] - log prior; rows as in the GMM kernels
__global__ void jd_hybrid_kernel(const float *__restrict__ feats, const int *__restrict__ row_src, int n_rows,
                                 const float *__restrict__ log_prior, int G, float *__restrict__ ll)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n_rows * G) return;
    const int r = (int)(i / G), g = (int)(i - (long long)r * G);
    const int src = row_src[r];
    ll[i] = (src >= 0) ? feats[(size_t)src * G + g] - log_prior[g] : 0.0f;
}

struct AmDevBuf {
    float *par = nullptr, *det = nullptr; int *n_mix = nullptr;
    float *par_fast = nullptr;      // jd_dec_set_scoring(JD_SCORE_FAST): [g][m][DP][2] = (sqrt(ivar), -mean sqrt(ivar)), made when first asked for
                                    // (DP = jd_fast_dp(D): D = 39 as it is, every other D padded with (0, 0) to jd_gmm_fast's chunk)
    int fast = 0;                   // launch_gmm scores with jd_gmm_fast39 (D = 39) / jd_gmm_fast
    float *log_prior = nullptr;
    float *mlp_w = nullptr, *mlp_b = nullptr;   // jd_am_create_mlp's models: the packed network (jd_mlp_pack)
    unsigned short *mlp_wq = nullptr;           // jd_am_mlp_to_bf16's: the weights packed as bf16 (jd_mlp_bf16_pack; mlp_w is null, mlp_b padded to 32)
    JdLogTab *logtab = nullptr;
    int device = -1;
};

static int upload_am_gmm(const jd_am *a, AmDevBuf &b)
{
    const size_t gm = (size_t)a->n_gmm * a->max_mix, D = (size_t)a->D;
    if (!a->tied) {                                                    // (tied hybrid models hold no Gaussians, placeholders neither: jd_host.cpp)
        std::vector<float> par(gm * D * 2);
        for (size_t i = 0; i < gm; ++i)
            for (size_t j = 0; j < D; ++j) {
                par[(i * D + j) * 2] = a->mean[i * D + j];
                par[(i * D + j) * 2 + 1] = a->ivar[i * D + j];
            }
        HIPCHK(hipMalloc(&b.par, par.size() * sizeof(float)));
        HIPCHK(hipMalloc(&b.det, gm * sizeof(float)));
        HIPCHK(hipMalloc(&b.n_mix, (size_t)a->n_gmm * sizeof(int)));
        HIPCHK(hipMemcpy(b.par, par.data(), par.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b.det, a->det.data(), gm * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b.n_mix, a->n_mix.data(), (size_t)a->n_gmm * sizeof(int), hipMemcpyHostToDevice));
    }
    {   // the table of jd_log1pe_table (both exact kernels)
        std::vector<JdLogTab> t(129);
        jd_fill_logtab(t.data());
        HIPCHK(hipMalloc(&b.logtab, t.size() * sizeof(JdLogTab)));
        HIPCHK(hipMemcpy(b.logtab, t.data(), t.size() * sizeof(JdLogTab), hipMemcpyHostToDevice));
    }
    if (a->hybrid) {
        HIPCHK(hipMalloc(&b.log_prior, a->log_prior.size() * sizeof(float)));
        HIPCHK(hipMemcpy(b.log_prior, a->log_prior.data(), a->log_prior.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (a->mlp && a->mlp_precision == JD_MLP_BF16) {
        HIPCHK(hipMalloc(&b.mlp_wq, a->mlp_wq.size() * sizeof(unsigned short)));
        HIPCHK(hipMalloc(&b.mlp_b, a->mlp_bp.size() * sizeof(float)));
        HIPCHK(hipMemcpy(b.mlp_wq, a->mlp_wq.data(), a->mlp_wq.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b.mlp_b, a->mlp_bp.data(), a->mlp_bp.size() * sizeof(float), hipMemcpyHostToDevice));
        const int span_b = (int)jd_splice_lds_bytes(JD_MLP_BF16_ROWS);
        if (a->mlp_spliced && a->tied) HIPCHK(hipFuncSetAttribute((const void *)jd_mlp_tied_bf16_spliced_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)JD_MLP_TIED_BF16_LDS_MAX + span_b));
        else if (a->mlp_spliced) HIPCHK(hipFuncSetAttribute((const void *)jd_mlp_bf16_spliced_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)JD_MLP_BF16_LDS_MAX + span_b));
        else if (a->tied) HIPCHK(hipFuncSetAttribute((const void *)jd_mlp_tied_bf16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)JD_MLP_TIED_BF16_LDS_MAX));
        else HIPCHK(hipFuncSetAttribute((const void *)jd_mlp_bf16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)JD_MLP_BF16_LDS_MAX));
    } else if (a->mlp) {
        HIPCHK(hipMalloc(&b.mlp_w, a->mlp_wp.size() * sizeof(float)));
        HIPCHK(hipMalloc(&b.mlp_b, a->mlp_bp.size() * sizeof(float)));
        HIPCHK(hipMemcpy(b.mlp_w, a->mlp_wp.data(), a->mlp_wp.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b.mlp_b, a->mlp_bp.data(), a->mlp_bp.size() * sizeof(float), hipMemcpyHostToDevice));
        // (above 64 KB of dynamic LDS a kernel has to be told; per device, and the same value every time)
        const int span_b = (int)jd_splice_lds_bytes(JD_MLP_ROWS);
        if (a->mlp_spliced && a->tied) HIPCHK(hipFuncSetAttribute((const void *)jd_mlp_tied_spliced_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)JD_MLP_TIED_LDS_MAX + span_b));
        else if (a->mlp_spliced) HIPCHK(hipFuncSetAttribute((const void *)jd_mlp_spliced_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)JD_MLP_LDS_MAX + span_b));
        else {
            HIPCHK(hipFuncSetAttribute((const void *)jd_mlp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)JD_MLP_LDS_MAX));
            if (a->tied) HIPCHK(hipFuncSetAttribute((const void *)jd_mlp_tied_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)JD_MLP_TIED_LDS_MAX));
        }
    }
    return JD_OK;
}

// the parameters of the scoring option (jd_gmm.h: jd_gmm_fast39, jd_gmm_fast): par is [gm][jd_fast_dp(D)][2], zero behind dimension D (jd_score_plan.h)
static void prep_par_fast(const float *mean, const float *ivar, size_t gm, size_t D, std::vector<float> &par)
{
    const size_t DP = (size_t)jd_fast_dp((int)D);
    par.assign(gm * DP * 2, 0.0f);
    for (size_t i = 0; i < gm; ++i)
        for (size_t j = 0; j < D; ++j) {
            const double s = sqrt((double)ivar[i * D + j]);
            par[(i * DP + j) * 2] = (float)s;
            par[(i * DP + j) * 2 + 1] = (float)(-(double)mean[i * D + j] * s);
        }
}
static int upload_am_fast(const jd_am *a, AmDevBuf &b)
{
    if (b.par_fast) return JD_OK;
    std::vector<float> par;
    prep_par_fast(a->mean.data(), a->ivar.data(), (size_t)a->n_gmm * a->max_mix, (size_t)a->D, par);
    HIPCHK(hipMalloc(&b.par_fast, par.size() * sizeof(float)));
    HIPCHK(hipMemcpy(b.par_fast, par.data(), par.size() * sizeof(float), hipMemcpyHostToDevice));
    return JD_OK;
}

static void free_am_gmm(AmDevBuf &b)
{
    if (b.par) (void)hipFree(b.par);
    if (b.par_fast) (void)hipFree(b.par_fast);
    if (b.det) (void)hipFree(b.det);
    if (b.n_mix) (void)hipFree(b.n_mix);
    if (b.logtab) (void)hipFree(b.logtab);
    if (b.log_prior) (void)hipFree(b.log_prior);
    if (b.mlp_w) (void)hipFree(b.mlp_w);
    if (b.mlp_b) (void)hipFree(b.mlp_b);
    if (b.mlp_wq) (void)hipFree(b.mlp_wq);
    b = AmDevBuf();
}

static_assert(sizeof(JdLogTab) == SCORE_LOGTAB_BYTES, "gmm39_lds (jd_score_plan.h) counts jd_gmm_kernel39's copy of the table");

// which kernel a launch_gmm call ran and on what grid (jd_score_kernel of juicer_amd.h; 0 / 0: nothing was launched)
struct GmmLaunch { int kernel = JD_KERNEL_NONE; unsigned grid = 0; };

// The plan of a scoring launch for these models on this device (jd_score_plan.h): the kernel, its tiles, the grid, the LDS
static bool am_fast(const AmDevBuf &b) { return b.fast && b.par_fast; }                   // launch_gmm scores with jd_gmm_fast39 / jd_gmm_fast
static ScorePlan gmm_plan(const jd_am *a, const AmDevBuf &b, int n_rows, int max_blocks = 0, int used_row_tiles = -1, bool has_list = false,
                          int n_rt_list = 0)
{
    return score_plan(ScorePlanIn{a->D, a->n_gmm, a->hybrid, a->mlp, am_fast(b), n_rows, max_blocks, used_row_tiles, has_list, n_rt_list,
                                  a->mlp && a->tied, a->mlp && a->mlp_precision == JD_MLP_BF16, a->mlp && a->mlp_spliced});
}

// jd_mlp_kernel - for tied models jd_mlp_tied_kernel - on rows [0, n_rows), on the plan's grid: d_out as out_mode says (JD_MLP_OUT_LL: the likelihood table)
// d_span: the rows' spans (jd_splice.h) for a spliced model - its kernels are the spliced flavours of the same four - and null for every other
static void launch_mlp(const jd_am *a, const AmDevBuf &b, const float *d_feats, const int *d_row_src, int n_rows, float *d_out, hipStream_t st,
                       unsigned grid, int out_mode, int layer, const JdSpan *d_span)
{
    const bool spl = a->mlp_spliced;
    if (a->mlp_precision == JD_MLP_BF16) {                             // (jd_am_mlp_to_bf16's models: the kernels of 32-row tiles)
        JdMlpDev m = jd_mlp_bf16_dev(a->mlp_desc);
        if (spl) m = jd_splice_dev(m, a->mlp_left, a->mlp_right);
        const size_t span_b = spl ? jd_splice_lds_bytes(JD_MLP_BF16_ROWS) : 0;
        const auto kernel = a->tied ? (spl ? jd_mlp_tied_bf16_spliced_kernel : jd_mlp_tied_bf16_kernel) : (spl ? jd_mlp_bf16_spliced_kernel : jd_mlp_bf16_kernel);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), (a->tied ? jd_mlp_tied_bf16_lds_bytes(m) : jd_mlp_bf16_lds_bytes(m)) + span_b, st, d_feats, d_row_src,
                           n_rows, b.mlp_wq, b.mlp_b, b.log_prior, b.logtab, m, d_out, out_mode, layer, d_span);
        return;
    }
    const size_t span_b = spl ? jd_splice_lds_bytes(JD_MLP_ROWS) : 0;
    if (a->tied) {
        JdMlpDev m = jd_mlp_dev(a->mlp_desc, true);
        if (spl) m = jd_splice_dev(m, a->mlp_left, a->mlp_right);
        const auto kernel = spl ? jd_mlp_tied_spliced_kernel : jd_mlp_tied_kernel;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), jd_mlp_tied_lds_bytes(m) + span_b, st, d_feats, d_row_src, n_rows, b.mlp_w, b.mlp_b, b.log_prior,
                           b.logtab, m, d_out, out_mode, layer, d_span);
        return;
    }
    JdMlpDev m = jd_mlp_dev(a->mlp_desc);
    if (spl) m = jd_splice_dev(m, a->mlp_left, a->mlp_right);
    const auto kernel = spl ? jd_mlp_spliced_kernel : jd_mlp_kernel;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), jd_mlp_lds_bytes(m) + span_b, st, d_feats, d_row_src, n_rows, b.mlp_w, b.mlp_b, b.log_prior, b.logtab,
                       m, d_out, out_mode, layer, d_span);
}

// max_blocks > 0 bounds the grid (the kernel strides over the tiles): next to the search, a
// chip-filling scoring launch holds every wave slot for milliseconds and the latency-bound search
// kernels, which need slots for microseconds at a time, all but stop (measured: 25 ms of
// scoring cost the search 20 ms).  A bounded grid scores in the background instead.
// skip_unused: row_src marks unused rows with -1 in whole-tile runs (decode_wave's stream slots).
// used_row_tiles >= 0: the row tiles that are not skipped (else: all of them)
// rt_base (device, or null) / n_rt_list: score these row tiles (first rows) only - the kernels of 128-row tiles (D = 39; jd_gmm_fast)
// info (or null): what was launched (jd_debug_score_rows)
// (hybrid models: all of rows [0, n_rows), whatever the other arguments say - but for max_blocks, which bounds jd_mlp_kernel's grid)
// d_span (device): span[r] beside d_row_src[r] for a spliced model (jd_splice.h), null for every other
static int launch_gmm(const jd_am *a, const AmDevBuf &b, const float *d_feats, const int *d_row_src, int n_rows,
                      float *d_ll, hipStream_t st, int max_blocks = 0, int skip_unused = 0, int used_row_tiles = -1,
                      const int *rt_base = nullptr, int n_rt_list = 0, GmmLaunch *info = nullptr, const JdSpan *d_span = nullptr)
{
    if (info) *info = GmmLaunch();
    if ((a->mlp && a->mlp_spliced) != (d_span != nullptr))
        return jd_fail(JD_EINVAL, "launch_gmm: the rows' spans are a spliced model's (jd_am_mlp_splice), and such a model's launch needs them");
    const ScorePlan p = gmm_plan(a, b, n_rows, max_blocks, used_row_tiles, rt_base != nullptr, n_rt_list);
    if (p.verdict == SCORE_PLAN_NOTHING) return JD_OK;
    if (p.verdict == SCORE_PLAN_LIST) return jd_fail(JD_EINVAL, "launch_gmm: tile lists are the D = 39 kernel's");
#define GMM_LAUNCH(kernel, ...) hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(256), p.lds_bytes, st, d_feats, d_row_src, n_rows, __VA_ARGS__)
#define GMM_ARGS(par) par, b.det, b.n_mix, a->n_gmm, a->max_mix
    switch (p.kernel) {
    case JD_KERNEL_MLP:
    case JD_KERNEL_MLP_BF16:
    case JD_KERNEL_MLP_TIED_BF16:
    case JD_KERNEL_MLP_SPLICED:
    case JD_KERNEL_MLP_TIED_SPLICED:
    case JD_KERNEL_MLP_BF16_SPLICED:
    case JD_KERNEL_MLP_TIED_BF16_SPLICED:
    case JD_KERNEL_MLP_TIED: launch_mlp(a, b, d_feats, d_row_src, n_rows, d_ll, st, p.grid, JD_MLP_OUT_LL, 0, d_span); break;
    case JD_KERNEL_HYBRID: GMM_LAUNCH(jd_hybrid_kernel, b.log_prior, a->n_gmm, d_ll); break;
    case JD_KERNEL_GMM_FAST39_16: GMM_LAUNCH(jd_gmm_fast39<GMM_GT_SMALL>, GMM_ARGS(b.par_fast), d_ll, skip_unused, rt_base, n_rt_list); break;
    case JD_KERNEL_GMM_FAST39_64: GMM_LAUNCH(jd_gmm_fast39<GMM_GT>, GMM_ARGS(b.par_fast), d_ll, skip_unused, rt_base, n_rt_list); break;
    case JD_KERNEL_GMM_FAST_16: GMM_LAUNCH(jd_gmm_fast<GMM_GT_SMALL>, GMM_ARGS(b.par_fast), a->D, p.dp, d_ll, skip_unused, rt_base, n_rt_list); break;
    case JD_KERNEL_GMM_FAST_64: GMM_LAUNCH(jd_gmm_fast<GMM_GT>, GMM_ARGS(b.par_fast), a->D, p.dp, d_ll, skip_unused, rt_base, n_rt_list); break;
    case JD_KERNEL_GMM39_16: GMM_LAUNCH(jd_gmm_kernel39<GMM_GT_SMALL>, GMM_ARGS(b.par), d_ll, skip_unused, b.logtab, rt_base, n_rt_list); break;
    case JD_KERNEL_GMM39_64: GMM_LAUNCH(jd_gmm_kernel39<GMM_GT>, GMM_ARGS(b.par), d_ll, skip_unused, b.logtab, rt_base, n_rt_list); break;
    case JD_KERNEL_GMM_GENERIC: GMM_LAUNCH(jd_gmm_kernel<0>, GMM_ARGS(b.par), a->D, d_ll, skip_unused, b.logtab); break;
    default: return jd_fail(JD_EINVAL, "launch_gmm: no kernel %d", p.kernel);
    }
#undef GMM_ARGS
#undef GMM_LAUNCH
    HIPCHK(hipGetLastError());
    if (info) { info->kernel = p.kernel; info->grid = p.grid; }
    return JD_OK;
}

// Workgroups of the scoring kernel launch_gmm chooses for a large launch that a CU holds, as the runtime counts them for the kernel
// alone; *per_cu = 0 where the kernel is not one of 128-row tiles (hybrid models, exact scoring of D != 39)
static int gmm_tiles128_occupancy(const jd_am *a, const AmDevBuf &b, int *per_cu)
{
    *per_cu = 0;
    const ScoreLarge large = score_plan_large(a->D, a->hybrid, a->mlp, am_fast(b));   // (none for either kind of neural models)
    const void *kernel = nullptr;
    switch (large.kernel) {
    case JD_KERNEL_GMM_FAST39_64: kernel = (const void *)jd_gmm_fast39<GMM_GT>; break;
    case JD_KERNEL_GMM_FAST_64: kernel = (const void *)jd_gmm_fast<GMM_GT>; break;
    case JD_KERNEL_GMM39_64: kernel = (const void *)jd_gmm_kernel39<GMM_GT>; break;
    default: return JD_OK;
    }
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kernel, 256, large.lds_bytes));
    return JD_OK;
}

static int check_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return jd_fail(JD_ENODEV, "no HIP device available (%s); juicer_amd has no CPU fallback",
                       e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return jd_fail(JD_ENODEV, "HIP device %d out of range (have %d)", device, n);
    HIPCHK(hipSetDevice(device));
    return JD_OK;
}

// What a stand-alone scoring call holds on the device: the model's parameters and the call's own buffers.  Freed when the call is
// left, whichever way (an early return of HIPCHK included).
struct ScoreBufs {
    AmDevBuf b;
    float *d_x = nullptr, *d_ll = nullptr;
    int *d_src = nullptr, *d_list = nullptr;
    JdSpan *d_span = nullptr;       // a spliced model's rows (else null)
    ScoreBufs() = default;
    ScoreBufs(const ScoreBufs &) = delete;
    ScoreBufs &operator=(const ScoreBufs &) = delete;
    ~ScoreBufs()
    {
        free_am_gmm(b);
        if (d_x) (void)hipFree(d_x);
        if (d_ll) (void)hipFree(d_ll);
        if (d_src) (void)hipFree(d_src);
        if (d_list) (void)hipFree(d_list);
        if (d_span) (void)hipFree(d_span);
    }
    // frames [n_frames][D] and a row map [n_rows] (row_src; null: the identity) go up, beside room for n_out floats of output;
    // for a spliced model the rows' spans {row_lo[r], row_hi[r]} too (null: the frames are ONE utterance, {0, n_frames - 1})
    int upload_rows(const jd_am *a, const float *frames, int n_frames, const int *row_src, int n_rows, size_t n_out, const int *row_lo = nullptr,
                    const int *row_hi = nullptr)
    {
        if (a->mlp && a->mlp_spliced) {
            std::vector<JdSpan> span((size_t)n_rows, JdSpan{0, std::max(0, n_frames - 1)});
            if (row_lo) for (int r = 0; r < n_rows; ++r) span[(size_t)r] = JdSpan{row_lo[r], row_hi[r]};
            HIPCHK(hipMalloc(&d_span, std::max<size_t>(span.size(), 1) * sizeof(JdSpan)));
            if (n_rows > 0) HIPCHK(hipMemcpy(d_span, span.data(), span.size() * sizeof(JdSpan), hipMemcpyHostToDevice));
        }
        const size_t D = (size_t)a->D;
        std::vector<int> identity;
        if (!row_src) {
            identity.resize((size_t)n_rows);
            std::iota(identity.begin(), identity.end(), 0);
            row_src = identity.data();
        }
        HIPCHK(hipMalloc(&d_x, std::max<size_t>((size_t)n_frames, 1) * D * sizeof(float)));
        HIPCHK(hipMalloc(&d_ll, n_out * sizeof(float)));
        HIPCHK(hipMalloc(&d_src, (size_t)n_rows * sizeof(int)));
        if (n_frames > 0) HIPCHK(hipMemcpy(d_x, frames, (size_t)n_frames * D * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_src, row_src, (size_t)n_rows * sizeof(int), hipMemcpyHostToDevice));
        return JD_OK;
    }
};

// One launch_gmm call on buffers of its own (the device is set): frames [n_frames][D] and row_src [n_rows] (null: the identity) go up, with the tile list
// rt_base [n_rt] (or null) and - prefilled - the caller's out [(guard_rows + n_rows + guard_rows)][G]; the table is written `guard_rows`
// rows into the buffer, and the whole buffer comes back.  The arguments are the caller's to check (jd_debug_score_rows does).
// (row_lo / row_hi: a spliced model's spans; null: the frames are one utterance)
static int score_rows_on_device(const jd_am *a, int mode, const float *frames, int n_frames, const int *row_src, int n_rows, int skip_unused,
                                int max_blocks, int used_row_tiles, const int *rt_base, int n_rt, int guard_rows, bool prefilled, float *out,
                                GmmLaunch *info, const int *row_lo = nullptr, const int *row_hi = nullptr)
{
    ScoreBufs s;
    int rc = upload_am_gmm(a, s.b);
    if (rc) return rc;
    if (mode == JD_SCORE_FAST) { rc = upload_am_fast(a, s.b); if (rc) return rc; s.b.fast = 1; }
    const size_t G = (size_t)a->n_gmm, n_out = ((size_t)n_rows + 2 * (size_t)guard_rows) * G;
    rc = s.upload_rows(a, frames, n_frames, row_src, n_rows, n_out, row_lo, row_hi);
    if (rc) return rc;
    if (prefilled) HIPCHK(hipMemcpy(s.d_ll, out, n_out * sizeof(float), hipMemcpyHostToDevice));
    if (rt_base) {
        HIPCHK(hipMalloc(&s.d_list, (size_t)n_rt * sizeof(int)));
        HIPCHK(hipMemcpy(s.d_list, rt_base, (size_t)n_rt * sizeof(int), hipMemcpyHostToDevice));
    }
    rc = launch_gmm(a, s.b, s.d_x, s.d_src, n_rows, s.d_ll + (size_t)guard_rows * G, 0, max_blocks, skip_unused, used_row_tiles, s.d_list,
                    rt_base ? n_rt : 0, info, s.d_span);
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, s.d_ll, n_out * sizeof(float), hipMemcpyDeviceToHost));
    return JD_OK;
}

static int score_frames_mode(const jd_am *a, int32_t device, int32_t mode, const float *frames, int32_t n_frames, float *out);
extern "C" int jd_am_score_frames(const jd_am *a, int32_t device, const float *frames, int32_t n_frames,
                                  float *out)
{
    return score_frames_mode(a, device, JD_SCORE_EXACT, frames, n_frames, out);
}
extern "C" int jd_am_score_frames_mode(const jd_am *a, int32_t device, int32_t mode, const float *frames, int32_t n_frames,
                                       float *out)
{
    return score_frames_mode(a, device, mode, frames, n_frames, out);
}
static int score_frames_mode(const jd_am *a, int32_t device, int32_t mode, const float *frames, int32_t n_frames, float *out)
{
    if (!a || !frames || !out || n_frames < 0) return jd_fail(JD_EINVAL, "jd_am_score_frames: bad argument");
    if (mode != JD_SCORE_EXACT && mode != JD_SCORE_FAST) return jd_fail(JD_EINVAL, "jd_am_score_frames_mode: mode %d (JD_SCORE_EXACT or JD_SCORE_FAST)", mode);
    // (the text of the days when the option served D = 39 alone, kept for its callers: GMM models of every D are served, hybrid ones are not)
    if (mode == JD_SCORE_FAST && a->hybrid) return jd_fail(JD_EINVAL, "JD_SCORE_FAST: 39-dimensional GMM models only");
    int rc = check_device(device);
    if (rc) return rc;
    if (n_frames == 0) return JD_OK;
    return score_rows_on_device(a, mode, frames, n_frames, nullptr, n_frames, 0, 0, -1, nullptr, 0, 0, false, out, nullptr);
}

// What the kernels take for granted of a launch's rows (host arrays): every row_src entry in [-1, n_frames); a tile list's entries in
// [0, n_rows) and their tiles apart; with skip_unused, the valid rows of every scored tile a prefix of it (jd_gmm.h: jd_gmm_kernel -
// the tile's first row decides).  No device is needed.
static int check_score_rows(const jd_am *a, int mode, int n_frames, const int *row_src, int n_rows, int skip_unused, const int *rt_base, int n_rt)
{
    for (int r = 0; r < n_rows; ++r)
        if (row_src[r] < -1 || row_src[r] >= n_frames)
            return jd_fail(JD_EINVAL, "jd_debug_score_rows: row_src[%d] = %d outside [-1, %d)", r, row_src[r], n_frames);
    const int h = score_plan_tile_rows(a->D, a->hybrid, a->mlp, mode == JD_SCORE_FAST);   // (0: no tiles as far as skip_unused and lists go)
    if (h == 0) {                                                      // (launch_gmm scores every row of a hybrid model and would ignore the list)
        if (rt_base) return jd_fail(JD_EINVAL, "jd_debug_score_rows: tile lists are not for hybrid models (jd_hybrid_kernel has no tiles)");
        return JD_OK;
    }
    std::vector<int> first;                                            // the scored tiles' first rows
    if (rt_base) {
        for (int t = 0; t < n_rt; ++t) {
            if (rt_base[t] < 0 || rt_base[t] >= n_rows) return jd_fail(JD_EINVAL, "jd_debug_score_rows: rt_base[%d] = %d outside [0, %d)", t, rt_base[t], n_rows);
            first.push_back(rt_base[t]);
        }
        std::sort(first.begin(), first.end());
        for (size_t t = 1; t < first.size(); ++t)
            if (first[t] - first[t - 1] < h) return jd_fail(JD_EINVAL, "jd_debug_score_rows: the listed tiles at rows %d and %d overlap", first[t - 1], first[t]);
    } else
        for (int r0 = 0; r0 < n_rows; r0 += h) first.push_back(r0);
    if (skip_unused)
        for (const int r0 : first) {
            bool hole = false;
            for (int r = r0; r < std::min(n_rows, r0 + h); ++r) {
                if (row_src[r] < 0) hole = true;
                else if (hole) return jd_fail(JD_EINVAL, "jd_debug_score_rows: skip_unused, and row %d is used behind an unused row of its tile (first row %d)", r, r0);
            }
        }
    return JD_OK;
}

// launch_gmm with a caller's own arguments, as the decoder's paths call it (include/juicer_amd.h); jd_debug_score_rows_span: the same
// with the rows' spans, a spliced model's (row_lo / row_hi null: any other model's)
static int debug_score_rows(const jd_am *a, int32_t device, int32_t mode, const float *frames, int32_t n_frames, const int32_t *row_src,
                            int32_t n_rows, int32_t skip_unused, int32_t max_blocks, int32_t used_row_tiles, const int32_t *rt_base,
                            int32_t n_rt, int32_t guard_rows, float *out, int32_t *kernel, int32_t *grid, const int32_t *row_lo, const int32_t *row_hi);
extern "C" int jd_debug_score_rows(const jd_am *a, int32_t device, int32_t mode, const float *frames, int32_t n_frames, const int32_t *row_src,
                                   int32_t n_rows, int32_t skip_unused, int32_t max_blocks, int32_t used_row_tiles, const int32_t *rt_base,
                                   int32_t n_rt, int32_t guard_rows, float *out, int32_t *kernel, int32_t *grid)
{
    if (a && a->mlp && a->mlp_spliced) {
        if (kernel) *kernel = JD_KERNEL_NONE;
        if (grid) *grid = 0;
        return jd_fail(JD_EINVAL, "jd_debug_score_rows: these models are spliced (jd_am_mlp_splice) and a row needs its span: jd_debug_score_rows_span takes it");
    }
    return debug_score_rows(a, device, mode, frames, n_frames, row_src, n_rows, skip_unused, max_blocks, used_row_tiles, rt_base, n_rt, guard_rows, out, kernel,
                            grid, nullptr, nullptr);
}
extern "C" int jd_debug_score_rows_span(const jd_am *a, int32_t device, int32_t mode, const float *frames, int32_t n_frames, const int32_t *row_src,
                                        const int32_t *row_lo, const int32_t *row_hi, int32_t n_rows, int32_t skip_unused, int32_t max_blocks,
                                        int32_t used_row_tiles, const int32_t *rt_base, int32_t n_rt, int32_t guard_rows, float *out, int32_t *kernel,
                                        int32_t *grid)
{
    if (kernel) *kernel = JD_KERNEL_NONE;
    if (grid) *grid = 0;
    if (!a || !(a->mlp && a->mlp_spliced))
        return jd_fail(JD_EINVAL, "jd_debug_score_rows_span: spans are a spliced model's (jd_am_mlp_splice); jd_debug_score_rows serves every other");
    if (n_rows > 0 && (!row_lo || !row_hi)) return jd_fail(JD_EINVAL, "jd_debug_score_rows_span: bad argument");
    for (int r = 0; r < n_rows; ++r) {
        if (row_src && row_src[r] < 0) continue;                       // (an unused row's span is not read)
        if (row_lo[r] < 0 || row_lo[r] >= n_frames) return jd_fail(JD_EINVAL, "jd_debug_score_rows_span: row_lo[%d] = %d outside [0, %d)", r, row_lo[r], n_frames);
        if (row_hi[r] < 0 || row_hi[r] >= n_frames) return jd_fail(JD_EINVAL, "jd_debug_score_rows_span: row_hi[%d] = %d outside [0, %d)", r, row_hi[r], n_frames);
        if (row_lo[r] > row_hi[r]) return jd_fail(JD_EINVAL, "jd_debug_score_rows_span: row_lo[%d] = %d above row_hi[%d] = %d", r, row_lo[r], r, row_hi[r]);
    }
    return debug_score_rows(a, device, mode, frames, n_frames, row_src, n_rows, skip_unused, max_blocks, used_row_tiles, rt_base, n_rt, guard_rows, out, kernel,
                            grid, row_lo, row_hi);
}
static int debug_score_rows(const jd_am *a, int32_t device, int32_t mode, const float *frames, int32_t n_frames, const int32_t *row_src,
                            int32_t n_rows, int32_t skip_unused, int32_t max_blocks, int32_t used_row_tiles, const int32_t *rt_base,
                            int32_t n_rt, int32_t guard_rows, float *out, int32_t *kernel, int32_t *grid, const int32_t *row_lo, const int32_t *row_hi)
{
    if (kernel) *kernel = JD_KERNEL_NONE;
    if (grid) *grid = 0;
    if (!a || !out || n_frames < 0 || n_rows < 0 || (n_frames > 0 && !frames) || (n_rows > 0 && !row_src) || max_blocks < 0 || guard_rows < 0 ||
        (rt_base ? n_rt < 1 : n_rt != 0))
        return jd_fail(JD_EINVAL, "jd_debug_score_rows: bad argument");
    if (mode != JD_SCORE_EXACT && mode != JD_SCORE_FAST) return jd_fail(JD_EINVAL, "jd_debug_score_rows: mode %d (JD_SCORE_EXACT or JD_SCORE_FAST)", mode);
    if (mode == JD_SCORE_FAST && a->hybrid) return jd_fail(JD_EINVAL, "jd_debug_score_rows: JD_SCORE_FAST is for GMM models");
    if ((long long)n_rows + 2LL * guard_rows > INT32_MAX) return jd_fail(JD_EINVAL, "jd_debug_score_rows: too many rows");
    int rc = check_score_rows(a, mode, n_frames, row_src, n_rows, skip_unused, rt_base, n_rt);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    if (n_rows == 0) return JD_OK;
    GmmLaunch info;
    rc = score_rows_on_device(a, mode, frames, n_frames, row_src, n_rows, skip_unused, max_blocks, used_row_tiles, rt_base, n_rt, guard_rows, true,
                              out, &info, row_lo, row_hi);
    if (rc) return rc;
    if (kernel) *kernel = info.kernel;
    if (grid) *grid = (int32_t)info.grid;
    return JD_OK;
}

// ---- the forward pass of jd_am_create_mlp's models on its own (include/juicer_amd.h): the kernel's and the host twin's
static int mlp_on_device(const jd_am *a, int device, const float *frames, int n_frames, int out_mode, int layer, float *out)
{
    int rc = check_device(device);
    if (rc) return rc;
    if (n_frames == 0) return JD_OK;
    ScoreBufs s;
    rc = upload_am_gmm(a, s.b);
    if (rc) return rc;
    const size_t W = (size_t)(out_mode == JD_MLP_OUT_LAYER ? a->mlp_desc.width[layer] : a->n_gmm);
    rc = s.upload_rows(a, frames, n_frames, nullptr, n_frames, (size_t)n_frames * W);
    if (rc) return rc;
    launch_mlp(a, s.b, s.d_x, s.d_src, n_frames, s.d_ll, 0, gmm_plan(a, s.b, n_frames).grid, out_mode, layer, s.d_span);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, s.d_ll, (size_t)n_frames * W * sizeof(float), hipMemcpyDeviceToHost));
    return JD_OK;
}
static int mlp_args(const jd_am *a, const float *frames, int32_t n_frames, const float *out, const char *who)
{
    if (!a || !out || n_frames < 0 || (n_frames > 0 && !frames)) return jd_fail(JD_EINVAL, "%s: bad argument", who);
    if (!a->mlp) return jd_fail(JD_ESTATE, "%s: these models hold no network (jd_am_create_mlp / jd_am_load_mlp make the ones that do)", who);
    return JD_OK;
}
extern "C" int jd_am_mlp_forward(const jd_am *a, int32_t device, const float *frames, int32_t n_frames, float *logpost)
{
    const int rc = mlp_args(a, frames, n_frames, logpost, "jd_am_mlp_forward");
    return rc ? rc : mlp_on_device(a, device, frames, n_frames, JD_MLP_OUT_LOGPOST, 0, logpost);
}
extern "C" int jd_am_mlp_forward_host(const jd_am *a, const float *frames, int32_t n_frames, float *logpost)
{
    const int rc = mlp_args(a, frames, n_frames, logpost, "jd_am_mlp_forward_host");
    if (rc) return rc;
    const JdMlpHostMath math;
    if (a->mlp_spliced)                                                // (the frames are one utterance: jd_splice.h)
        jd_splice_forward_host(a->mlp_desc, a->mlp_left, a->mlp_right, a->mlp_precision == JD_MLP_BF16, a->mlp_w.data(), a->mlp_b.data(), nullptr, frames, n_frames,
                               -1, logpost, math, a->tied);
    else if (a->mlp_precision == JD_MLP_BF16) jd_mlp_bf16_forward_host(a->mlp_desc, a->mlp_w.data(), a->mlp_b.data(), nullptr, frames, n_frames, -1, logpost, math, a->tied);
    else jd_mlp_forward_host(a->mlp_desc, a->mlp_w.data(), a->mlp_b.data(), nullptr, frames, n_frames, -1, logpost, math, a->tied);
    return JD_OK;
}
extern "C" int jd_debug_mlp_activations(const jd_am *a, int32_t device, int32_t on_device, const float *frames, int32_t n_frames, int32_t layer,
                                        float *out)
{
    const int rc = mlp_args(a, frames, n_frames, out, "jd_debug_mlp_activations");
    if (rc) return rc;
    if (layer < 0 || layer >= a->mlp_desc.n_layers)
        return jd_fail(JD_EINVAL, "jd_debug_mlp_activations: layer %d outside [0, %d)", layer, a->mlp_desc.n_layers);
    if (on_device) return mlp_on_device(a, device, frames, n_frames, JD_MLP_OUT_LAYER, layer, out);
    const JdMlpHostMath math;
    if (a->mlp_spliced)
        jd_splice_forward_host(a->mlp_desc, a->mlp_left, a->mlp_right, a->mlp_precision == JD_MLP_BF16, a->mlp_w.data(), a->mlp_b.data(), nullptr, frames, n_frames,
                               layer, out, math, a->tied);
    else if (a->mlp_precision == JD_MLP_BF16) jd_mlp_bf16_forward_host(a->mlp_desc, a->mlp_w.data(), a->mlp_b.data(), nullptr, frames, n_frames, layer, out, math, a->tied);
    else jd_mlp_forward_host(a->mlp_desc, a->mlp_w.data(), a->mlp_b.data(), nullptr, frames, n_frames, layer, out, math, a->tied);
    return JD_OK;
}

// launch_gmm's MLP branch timed with events: warmup launches, then ms[iters], one launch each on n_frames rows (frames [n_frames][in_dim])
extern "C" int jd_debug_mlp_time(const jd_am *a, int32_t device, const float *frames, int32_t n_frames, int32_t max_blocks, int32_t warmup,
                                 int32_t iters, float *ms)
{
    int rc = mlp_args(a, frames, n_frames, ms, "jd_debug_mlp_time");
    if (rc) return rc;
    if (n_frames < 1 || warmup < 0 || iters < 1 || max_blocks < 0) return jd_fail(JD_EINVAL, "jd_debug_mlp_time: bad argument");
    rc = check_device(device);
    if (rc) return rc;
    ScoreBufs s;
    rc = upload_am_gmm(a, s.b);
    if (rc) return rc;
    rc = s.upload_rows(a, frames, n_frames, nullptr, n_frames, (size_t)n_frames * a->n_gmm);
    if (rc) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return jd_fail(JD_EHIP, "jd_debug_mlp_time: hipEventCreate"); }
    for (int i = 0; i < warmup + iters && rc == JD_OK; ++i) {
        bool ok = hipEventRecord(e0, 0) == hipSuccess;
        rc = launch_gmm(a, s.b, s.d_x, s.d_src, n_frames, s.d_ll, 0, max_blocks, 0, -1, nullptr, 0, nullptr, s.d_span);
        float t = 0.0f;
        ok = ok && rc == JD_OK && hipEventRecord(e1, 0) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess;
        if (rc == JD_OK && !ok) rc = jd_fail(JD_EHIP, "jd_debug_mlp_time: timing a launch failed");
        if (i >= warmup) ms[i - warmup] = t;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return rc;
}
