// jd_score_plan.h - what a scoring launch is, as a function of plain data (no HIP, no models: compiled and tested on the CPU,
// tests/test_score_plan_cpu.py, tests/test_mlp_tied_cpu.py): which of the scoring kernels (jd_gmm.h, jd_mlp_kernel.h, jd_hybrid_kernel) serves the models and
// the option, its tile, how many tiles the rows make, the grid and the dynamic LDS.  launch_gmm (jd_host_scoring.h) turns the
// result into the launch; gmm_tiles128_occupancy and check_score_rows ask it for the kernel of a large launch and for the tile's
// rows; the pipeline's piece bounds (jd_pipe.h: pipe_piece_bounds) take the tile constants and the threshold from here.
// The tile constants of the kernels themselves are defined here, once: jd_device.hip includes this header in front of jd_gmm.h.
#pragma once

#include <algorithm>
#include <cstddef>

#include "../../include/juicer_amd.h"   // JD_KERNEL_* (by its place: jd_pipe.h's includers search csrc alone)
#include "jd_mlp.h"            // JD_MLP_ROWS: the rows of jd_mlp_kernel's tile
#include "jd_mlp_bf16.h"       // JD_MLP_BF16_ROWS: the rows of jd_mlp_bf16_kernel's tile, and its LDS
#include "jd_splice.h"         // jd_splice_lds_bytes: what a spliced kernel's tile keeps beside it

#define GMM_ROWS 64             // stream-frames per tile of jd_gmm_kernel<0> (one per lane)
#define GMM_GT 64               // tied states per GMM workgroup (16 per wave)
#define GMM_GT_SMALL 16         // ... of a launch with few rows (the kernels of 128-row tiles)
#define GMM_ROWS2 128           // stream-frames per tile of jd_gmm_kernel39 / jd_gmm_fast39 / jd_gmm_fast (two per lane)
#define GMM_FAST_DC 8           // jd_gmm_fast: dimensions of a chunk (the parameters are padded to it)
#define GMM_FAST_DS 64          // ... and of the slab of the tile in LDS
#define SCORE_SMALL_BELOW 1024  // a launch of fewer tiles of GMM_GT states than this is one of GMM_GT_SMALL-state tiles
#define SCORE_LOGTAB_BYTES 16   // sizeof(JdLogTab) (jd_gmm.h: two doubles)

// the parameters of the scoring option (jd_gmm.h: jd_gmm_fast39, jd_gmm_fast): par is [gm][jd_fast_dp(D)][2], zero behind dimension D
static inline int jd_fast_dp(int D) { return D == 39 ? 39 : (D + GMM_FAST_DC - 1) / GMM_FAST_DC * GMM_FAST_DC; }

// dynamic LDS of the kernels of 128-row tiles, and of jd_gmm_kernel<0> (dp = D | 1)
static inline size_t gmm39_lds() { return 130 * (size_t)SCORE_LOGTAB_BYTES + 32 * sizeof(unsigned long long) + (size_t)GMM_ROWS2 * std::max(39, GMM_GT + 1) * sizeof(float); }
static inline size_t gmm_fast39_lds() { return (size_t)GMM_ROWS2 * std::max(39, GMM_GT + 1) * sizeof(float); }
static inline size_t gmm_fast_lds() { return (size_t)GMM_ROWS2 * (GMM_FAST_DS + 1) * sizeof(float); }
static inline size_t gmm_generic_lds(int dp) { return (size_t)(GMM_ROWS * dp + GMM_ROWS * (GMM_GT + 1)) * sizeof(float); }

// The kernel of the models and the option, whatever the rows: its flavours of GMM_GT and of GMM_GT_SMALL states (the same where
// there is one), the tile, the LDS.  fast: the option is on and its parameters are there.
struct ScoreKernels {
    int kernel = JD_KERNEL_NONE, kernel_small = JD_KERNEL_NONE;
    int tile_rows = 0;                    // 0: jd_hybrid_kernel has no tiles
    bool state_tiles = false;             // tiles of rows x states (the GMM kernels); else every row is scored whole
    bool tiles128 = false;                // ... of GMM_ROWS2 rows: two widths, skip lists
    size_t lds_bytes = 0;                 // (jd_mlp_kernel / jd_mlp_tied_kernel: the network's, jd_mlp.h: jd_mlp_lds_bytes / jd_mlp_tied_lds_bytes)
    int dp = 0;                           // jd_gmm_fast: jd_fast_dp(D); jd_gmm_kernel<0>: D | 1
};
// (tied: jd_am_create_mlp_tied's models among those with a network - jd_mlp_tied_kernel; bf16: jd_am_mlp_to_bf16's among those -
// jd_mlp_bf16_kernel / jd_mlp_tied_bf16_kernel, tiles of JD_MLP_BF16_ROWS rows; lds_bytes is then the bound the kernel is told,
// JD_MLP_BF16_LDS_MAX / JD_MLP_TIED_BF16_LDS_MAX, and the launch takes the network's own, jd_mlp_bf16.h;
// spliced: jd_am_mlp_splice's among those with a network - the spliced flavour of the same kernel, the same tile, and the tile's spans
// behind the bf16 bound)
static inline ScoreKernels score_kernels(int D, bool hybrid, bool mlp, bool fast, bool tied = false, bool bf16 = false, bool spliced = false)
{
    ScoreKernels k;
    if (mlp && bf16) {
        if (spliced) k.kernel = k.kernel_small = tied ? JD_KERNEL_MLP_TIED_BF16_SPLICED : JD_KERNEL_MLP_BF16_SPLICED;
        else k.kernel = k.kernel_small = tied ? JD_KERNEL_MLP_TIED_BF16 : JD_KERNEL_MLP_BF16;
        k.tile_rows = JD_MLP_BF16_ROWS;
        k.lds_bytes = (tied ? JD_MLP_TIED_BF16_LDS_MAX : JD_MLP_BF16_LDS_MAX) + (spliced ? jd_splice_lds_bytes(JD_MLP_BF16_ROWS) : 0);
        return k;
    }
    if (mlp) {
        if (spliced) k.kernel = k.kernel_small = tied ? JD_KERNEL_MLP_TIED_SPLICED : JD_KERNEL_MLP_SPLICED;
        else k.kernel = k.kernel_small = tied ? JD_KERNEL_MLP_TIED : JD_KERNEL_MLP;
        k.tile_rows = JD_MLP_ROWS;
        return k;
    }
    if (hybrid) { k.kernel = k.kernel_small = JD_KERNEL_HYBRID; return k; }
    k.state_tiles = true;
    k.tiles128 = D == 39 || fast;
    k.tile_rows = k.tiles128 ? GMM_ROWS2 : GMM_ROWS;
    if (D == 39 && fast) { k.kernel = JD_KERNEL_GMM_FAST39_64; k.kernel_small = JD_KERNEL_GMM_FAST39_16; k.lds_bytes = gmm_fast39_lds(); }
    else if (fast) { k.kernel = JD_KERNEL_GMM_FAST_64; k.kernel_small = JD_KERNEL_GMM_FAST_16; k.lds_bytes = gmm_fast_lds(); k.dp = jd_fast_dp(D); }
    else if (D == 39) { k.kernel = JD_KERNEL_GMM39_64; k.kernel_small = JD_KERNEL_GMM39_16; k.lds_bytes = gmm39_lds(); }
    else { k.kernel = k.kernel_small = JD_KERNEL_GMM_GENERIC; k.dp = D | 1; k.lds_bytes = gmm_generic_lds(k.dp); }
    return k;
}

// The kernel launch_gmm chooses for a LARGE launch and its LDS; JD_KERNEL_NONE where it is not one of 128-row tiles (hybrid and
// neural models, exact scoring of D != 39)
struct ScoreLarge { int kernel = JD_KERNEL_NONE; size_t lds_bytes = 0; };
static inline ScoreLarge score_plan_large(int D, bool hybrid, bool mlp, bool fast)
{
    const ScoreKernels k = score_kernels(D, hybrid, mlp, fast);
    return k.tiles128 ? ScoreLarge{k.kernel, k.lds_bytes} : ScoreLarge();
}

// The rows of a tile as far as skip_unused and tile lists go (check_score_rows): 0 for the kernels that score every row whole
static inline int score_plan_tile_rows(int D, bool hybrid, bool mlp, bool fast)
{
    const ScoreKernels k = score_kernels(D, hybrid, mlp, fast);
    return k.state_tiles ? k.tile_rows : 0;
}

struct ScorePlanIn {
    int D, n_gmm;
    bool hybrid, mlp;                     // jd_am_create_hybrid's models / those with a network (which are hybrid too)
    bool fast;                            // jd_dec_set_scoring(JD_SCORE_FAST) and its parameters are on the device
    int n_rows;
    int max_blocks;                       // > 0 bounds the grid (the kernels stride over the tiles); not jd_hybrid_kernel's
    int used_row_tiles;                   // >= 0: the row tiles that are not skipped (else: all of them)
    bool has_list; int n_rt_list;         // score the listed row tiles only (the kernels of 128-row tiles)
    bool tied = false;                    // mlp, and the network's outputs are tied states (jd_am_create_mlp_tied): jd_mlp_tied_kernel
    bool bf16 = false;                    // mlp, and the model is a bf16 one (jd_am_mlp_to_bf16): jd_mlp_bf16_kernel / jd_mlp_tied_bf16_kernel
    bool spliced = false;                 // mlp, and the model is a spliced one (jd_am_mlp_splice): the spliced flavour of its kernel
};

enum ScorePlanVerdict {
    SCORE_PLAN_OK = 0,
    SCORE_PLAN_NOTHING,                   // n_rows <= 0: nothing to launch
    SCORE_PLAN_LIST,                      // a tile list, and the kernel is not one of 128-row tiles
};

struct ScorePlan {                        // (what follows the point a verdict other than ok was reached stays 0)
    ScorePlanVerdict verdict = SCORE_PLAN_OK;
    int kernel = JD_KERNEL_NONE;
    int tile_rows = 0;                    // 0: jd_hybrid_kernel; 16: jd_mlp_kernel, jd_mlp_tied_kernel; 32: their bf16 kernels (spliced or not); 64 or 128
    int tile_states = 0;                  // 16 or 64; 0: no state tiles
    long long row_tiles = 0, tiles = 0;   // jd_hybrid_kernel: no row tiles, and its tiles are blocks of 256 cells
    unsigned grid = 0;
    size_t lds_bytes = 0;
    int dp = 0;
};

static inline ScorePlan score_plan(const ScorePlanIn &in)
{
    ScorePlan p;
    if (in.n_rows <= 0) { p.verdict = SCORE_PLAN_NOTHING; return p; }
    const ScoreKernels k = score_kernels(in.D, in.hybrid, in.mlp, in.fast, in.tied, in.bf16, in.spliced);
    const int max_blocks = in.max_blocks;
    // (hybrid models: all of rows [0, n_rows), whatever the other arguments say - but for max_blocks, which bounds the grid of
    // jd_mlp_kernel and jd_mlp_tied_kernel and of their bf16 kernels)
    if (in.mlp) {
        const int tiles = (in.n_rows + k.tile_rows - 1) / k.tile_rows;
        p.kernel = k.kernel;
        p.row_tiles = p.tiles = tiles;
        p.grid = (unsigned)((max_blocks > 0 && tiles > max_blocks) ? max_blocks : tiles);
    } else if (in.hybrid) {
        const long long n = (long long)in.n_rows * in.n_gmm;
        p.kernel = k.kernel;
        p.tiles = (n + 255) / 256;
        p.grid = (unsigned)((n + 255) / 256);
    } else {
        if (in.has_list && !k.tiles128) { p.verdict = SCORE_PLAN_LIST; return p; }
        const long long row_tiles = in.has_list ? in.n_rt_list : (in.n_rows + k.tile_rows - 1) / k.tile_rows;
        long long tiles = row_tiles * ((in.n_gmm + GMM_GT - 1) / GMM_GT);
        // few rows (a streaming push, a tick of the broker): tiles of 16 states, four times as many and a quarter as long
        const bool small_tiles = k.tiles128 && (in.used_row_tiles >= 0 ? (long long)in.used_row_tiles * ((in.n_gmm + GMM_GT - 1) / GMM_GT) : tiles) < SCORE_SMALL_BELOW;
        if (small_tiles) tiles = row_tiles * ((in.n_gmm + GMM_GT_SMALL - 1) / GMM_GT_SMALL);
        p.tile_states = small_tiles ? GMM_GT_SMALL : GMM_GT;
        p.row_tiles = row_tiles; p.tiles = tiles;
        p.grid = (unsigned)((max_blocks > 0 && tiles > max_blocks) ? max_blocks : tiles);
        p.kernel = small_tiles ? k.kernel_small : k.kernel;
    }
    p.tile_rows = k.tile_rows; p.lds_bytes = k.lds_bytes; p.dp = k.dp;
    return p;
}
