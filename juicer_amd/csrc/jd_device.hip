// jd_device.hip - gfx950 (MI355X) kernels + decoder runtime of juicer_amd.
//
// Two kernels make up the hot path (reference: WFSTDecoderLite::processFrame,
// src/WFSTDecoderLite.cpp:311-372, and HTKFlatModels::calcGMMOutput,
// src/HTKFlatModels.cpp:226-262):
//
//  jd_gmm_kernel     companion kernel.  Diagonal-GMM log-likelihood of every
//                    tied state for a tile of 64 stream-frames.  One lane owns
//                    one frame (its 39-dim vector staged through LDS into
//                    registers); the tied state is wave-uniform, so its
//                    mean/inverse-variance stream arrives through the scalar
//                    cache and the per-lane work is pure VALU in the
//                    reference's operation order (no FMA contraction, no MFMA:
//                    elementwise + reduction).  The log-sum-exp over mixtures is
//                    the reference's sequential logAdd chain, evaluated per lane.
//
//  k_search          persistent token-passing search (jd_search.h): every utterance
//                    stream is served by a cluster of workgroups that runs all
//                    frames of a chunk without returning to the host.  Per frame:
//                    (A) HMM-internal propagation over the active arc instances
//                    with beam / histogram pruning and ballot compaction into
//                    wave-owned list segments, (X) frontier expansion over the CSR
//                    arc table iterated to epsilon/tee closure, with 64-bit
//                    atomic-max Viterbi recombination into per-arc keys and
//                    word-boundary Path records appended to a device arena.
//
// The host runtime below asks HIP, calls a pure function, allocates and uploads: what the kernels see of the graph and the
// models is decided in jd_prep.h, the sizes and the layout of the stream arenas and of a wave's likelihood tables in
// jd_arena.h, the cluster plan of a launch in jd_plan.h - plain data in, plain data out, each tested on the CPU.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see build.py).
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <cerrno>
#include <numeric>
#include <queue>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <limits>
#include <mutex>
#include <vector>

#include "jd_internal.h"
#include "jd_prep.h"            // LZ, the device arc's flags, XState; the graph preparation of jd_dec_create
#include "jd_arena.h"           // the sizes and the layout of the stream arenas (ensure_arenas), a wave's likelihood tables (WavePlan, plan_wave)
#include "jd_ahead.h"           // working ahead: the queue of announced batches, tables and banks, decode_wave's decisions
#include "jd_pipe.h"            // batches through the resident slot kernel: the mailbox record, the slot pipeline's bookkeeping and pump decisions
#include "jd_push.h"            // the streaming interface: a stream's record, argument checks, PARTIAL_DECODING's schedule, packing, k_partial_many's layout
#include "jd_best.h"            // the current best hypothesis of live streams: k_best_many's layout, what a reply means, the word projection
#include "jd_final.h"           // the end-of-utterance view of live streams: k_final_many's layout, what a reply means, the word projection
#include "jd_score_plan.h"      // a scoring launch: the kernel, its tiles, grid and LDS (launch_gmm); the scoring kernels' tile constants (GMM_*)

#define HIST_MAX_BINS 2048

struct __align__(16) Tok { float score, ac, lm; int path; };
struct __align__(16) PathRec { int prev, frame, label, model; float score, ac, lm, pad1; };   // model: in-label, model-level output only (else 0)

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return jd_fail(JD_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                           __FILE__, __LINE__);                                              \
    } while (0)

// ------------------------------------------------------------------ device utils

__device__ __forceinline__ unsigned f2o(float f)
{
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float o2f(unsigned o)
{
    unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    return __uint_as_float(u);
}
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int rank_in(unsigned long long bal)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
}

// ------------------------------------------------------------------- scoring kernels
#include "jd_gmm.h"
#include "jd_mlp_kernel.h"      // neural acoustic models: the fused forward pass (jd_mlp.h: the network as data, the host twin)
#include "jd_mlp_bf16_kernel.h" // ... and of their bf16 form (jd_mlp_bf16.h: the contract, the packing, the twin)

// --------------------------------------------------------------- search kernels
#include "jd_search.h"

// ------------------------------------------- Path collection, partial trace, finish, launch helpers
#include "jd_gc.h"
#include "jd_resident.h"
#include "jd_slot.h"

// --------------------------------------------------------------- host runtime

#include "jd_host_scoring.h"

#define JD_MAX_DEVICES 64
static std::mutex g_search_mu[JD_MAX_DEVICES];     // one persistent search launch at a time per device (launch_search)
static std::atomic<long long> g_search_turn[JD_MAX_DEVICES];  // counts the holders of the lock: who gives it up for a waiter sees the waiter take it
static std::atomic<int> g_search_waiters[JD_MAX_DEVICES];   // ... and who waits for it (a resident kernel makes room: jd_res_should_yield)

// ... and across PROCESSES: the reference's way of using several cores is several processes over split file lists
// (doc/userman/juicer_userman.tex:584), and two of them pointed at one GPU would each get part of the CUs for their
// persistent launch and spin at their cluster barriers until the 30 s time-out.  An advisory file lock per device -
// named after its PCI bus id, so that every process means the same GPU whatever its visible-device order - is held
// from the dispatch of a search launch to its completion: the processes take turns launch by launch (a launch is
// milliseconds) and both finish.  JD_GPU_LOCK=0 switches it off, JD_GPU_LOCK_DIR moves the files (default /tmp); a
// lock file that cannot be opened leaves the launch unguarded, as before.
struct GpuFileLock {
    int fd = -2;                                   // -2: not tried yet, -1: unavailable
    std::mutex mu;
};
static GpuFileLock g_gpu_lock[JD_MAX_DEVICES];
static int gpu_lock_fd(int device)
{
    GpuFileLock &L = g_gpu_lock[(size_t)std::min(std::max(device, 0), JD_MAX_DEVICES - 1)];
    std::lock_guard<std::mutex> lk(L.mu);
    if (L.fd != -2) return L.fd;
    L.fd = -1;
    const char *off = getenv("JD_GPU_LOCK");
    if (off && atoi(off) == 0) return -1;
    char bus[64] = "";
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char *p = bus; *p; ++p) if (*p == ':' || *p == '/') *p = '_';
    const char *dir = getenv("JD_GPU_LOCK_DIR");
    char path[512];
    snprintf(path, sizeof path, "%s/juicer_amd.gpu-%s.lock", dir && *dir ? dir : "/tmp", bus);
    L.fd = open(path, O_RDWR | O_CREAT | O_CLOEXEC, 0666);
    return L.fd;
}
struct GpuLockGuard {
    int fd;
    explicit GpuLockGuard(int device) : fd(gpu_lock_fd(device)) { if (fd >= 0) while (flock(fd, LOCK_EX) != 0 && errno == EINTR) { } }
    ~GpuLockGuard() { if (fd >= 0) (void)flock(fd, LOCK_UN); }
};

// The stream arenas of a decoder are ONE slab, and the slab of a destroyed decoder is kept (one per device, the
// largest) for the next decoder on that device: what a decoder's set-up costs is the driver clearing the bytes it
// hands out (25-60 GB/s, tools/alloc_probe.py - seconds for the default 70 % of a 288 GB device, every time a
// decoder follows another one), and nothing in the arenas needs to be clear except what ensure_arenas clears itself.
// JD_ARENA_CACHE=0 switches it off; jd_release_cached_memory gives the slab back.
struct ArenaSlab { void *p = nullptr; size_t bytes = 0; };
static std::mutex g_slab_mu;
static ArenaSlab g_slab[JD_MAX_DEVICES];
static size_t slab_cached_bytes(int device)
{
    std::lock_guard<std::mutex> lk(g_slab_mu);
    return (device >= 0 && device < JD_MAX_DEVICES) ? g_slab[device].bytes : 0;
}
static int slab_take(int device, size_t bytes, ArenaSlab *out)
{
    {
        std::lock_guard<std::mutex> lk(g_slab_mu);
        if (device >= 0 && device < JD_MAX_DEVICES && g_slab[device].p) {
            ArenaSlab &c = g_slab[device];
            if (c.bytes >= bytes) { *out = c; c = ArenaSlab(); return JD_OK; }
            (void)hipFree(c.p);                                        // too small: its bytes go towards the new one
            c = ArenaSlab();
        }
    }
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, std::max<size_t>(bytes, 256));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return jd_fail(e == hipErrorOutOfMemory ? JD_ENOMEM : JD_EHIP, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    }
    out->p = q; out->bytes = std::max<size_t>(bytes, 256);
    return JD_OK;
}
static void slab_give(int device, ArenaSlab sl)
{
    if (!sl.p) return;
    const char *e = getenv("JD_ARENA_CACHE");
    const bool keep = !(e && atoi(e) == 0) && device >= 0 && device < JD_MAX_DEVICES;
    std::lock_guard<std::mutex> lk(g_slab_mu);
    if (keep && g_slab[device].bytes < sl.bytes) std::swap(g_slab[device], sl);
    if (sl.p) (void)hipFree(sl.p);
}
extern "C" int jd_release_cached_memory(int32_t device)
{
    if (device < 0 || device >= JD_MAX_DEVICES) return jd_fail(JD_EINVAL, "jd_release_cached_memory: bad device");
    ArenaSlab sl;
    { std::lock_guard<std::mutex> lk(g_slab_mu); std::swap(sl, g_slab[device]); }
    if (sl.p) { if (hipSetDevice(device) != hipSuccess) return jd_fail(JD_EHIP, "hipSetDevice(%d) failed", device); (void)hipFree(sl.p); }
    return JD_OK;
}

struct HostResult {
    std::vector<int32_t> label, time;
    std::vector<float> score, ac, lm;
    // model-level output (jd_dec_set_output_level): the whole record chain, newest first (jd_dec_model_result)
    int32_t m_n = -1;
    std::vector<int32_t> m_model, m_label, m_time;
    std::vector<float> m_score, m_ac, m_lm;
    float m_tot[3] = {0.0f, 0.0f, 0.0f};
};

// A batch announced with jd_dec_prefetch_scores: scored on the scoring stream WHILE the batch before it is searched
// (the blocks of the scoring kernel take the CUs that clusters of the persistent search leave as their streams end).
// What is decided about it is decided in jd_ahead.h (AheadEntry); here, the events around its scoring (SCORED: the table is d_ll[buf]).
struct Prefetch : AheadEntry {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void drop_events() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); ev0 = ev1 = nullptr; }
    void drop() { drop_events(); state = AHEAD_NONE; feats = nullptr; bank = -1; }
};

struct jd_dec {
    const jd_net *net = nullptr;
    const jd_am *am = nullptr;
    int device = 0, max_streams = 0, block_size = 5;
    DecConst C{};
    AmDevBuf amb;
    // device copies of static data
    int *d_row_ptr = nullptr; JdArc *d_arcs = nullptr; float *d_fin_w = nullptr; int *d_aux = nullptr;
    XState *d_xst = nullptr;              // per state: the decoder's arc order (DecConst::xst)
    int *d_se32 = nullptr;
    float *d_hmm_tee = nullptr, *d_trP = nullptr, *d_hmm_tmax0 = nullptr, *d_lrt = nullptr;
    int *d_pcount = nullptr;               // per state: Path objects of the reference per arriving token (DecConst::pcount)
    std::vector<int> state_new;           // the decoder's own numbering of the states: state_new[network state] (empty: the network's)
    // per-stream state
    StreamDev *d_streams = nullptr;
    StreamCtl *d_ctl = nullptr;
    std::vector<StreamDev> h_streams;          // host mirror (arena pointers)
    std::vector<void *> allocs;
    ArenaSlab slab;                       // the stream arenas (ensure_arenas)
    bool arenas_ready = false;
    int64_t cap_slots = 0, cap_paths = 0, cap_items = 0, cap_new = 0;
    int64_t slots_hint = 0;               // jd_dec_set_max_alloc_models
    int res_cap = 8192;
    int *d_res = nullptr;                 // result arena, see ensure_arenas
    int *d_res_model = nullptr;           // ... the records' models beside it, [stream][res_cap] (model-level output)
    bool models = false;                  // model-level output (jd_dec_set_output_level): the search kernels' MDL flavour
    int n_cus = 256;
    // search launches: one 512-thread workgroup per CU, a cluster of them per stream
    int max_cw = MAXCW;                   // upper bound of workgroups per stream cluster (JD_CW overrides)
    int weighted = 1;                     // size the clusters by the work ahead of each stream (JD_WEIGHTED=0: uniform)
    int rebalance = 1;                    // cut a launch short and plan the rest anew when part of the grid idles (JD_REBALANCE=0: off)
    double rebalance_frac = 0.2;          // ... this part (JD_REBALANCE_FRAC)
    double rebalance_min_us = 4000.0;     // ... and only launches predicted to last this long (JD_REBALANCE_MIN_US; 0 in tests)
    double model_a_us = 10.0, model_b_us = 360.0;   // cost model of a stream-frame: a + b / workgroups (launch_search), as fitted in round 2
    double pf_gmm_weight = 1.35;          // scoring beside a search is priced at this times its CU-time on its own (the CUs come late,
                                          // and piecemeal; JD_PF_GMM_WEIGHT)
    int plan_min_cw = 2;                  // greedy plan: workgroups every stream starts with (JD_PLAN_MIN_CW)
    int plan_mode = 0;                    // 0: round 2's constants + bisection; 1: measured curve (model2_*) + greedy whole workgroups (JD_PLAN)
    double model2_a_us = 24.6, model2_b_us = 61.4;   // ... as measured in round 3 (JD_MODEL2_A / JD_MODEL2_B)
    // b was fitted at configs[1]'s load (23.7 k instances + arcs per stream-frame); it scales with the load,
    // which a decoder learns from the batches it has decoded (first batch: as fitted)
    double load_scale = 1.0, load_sum = 0.0, load_frames = 0.0;
    int4 *d_work = nullptr; int work_cap = 0;
    unsigned *d_cells = nullptr; size_t cells_words = 0;   // diagnostics (jd_dec_debug_cells): a bit per cell of the likelihood slab
    int *d_status = nullptr; int *h_status = nullptr;
    bool xl_ok = true;                    // XCD-local launches allowed (JD_XCD_LOCAL=0 or one failed placement check switch them off)
    double xl_slack = 1.04;               // ... when the packed plan is predicted to end no later than this times the unpacked one (JD_XL_SLACK)
    long long *d_dbg = nullptr, *d_dbg_buf = nullptr;   // in-kernel cycle accounting (jd_dec_debug_trace): in use / allocated
    // chunked pipeline
    int Fc = 128;                         // frames per scoring chunk of the streaming API (jd_stream_push)
    int Fw_env = 0;                       // JD_FC: frames per chunk of the batch path (0 = as long as the longest utterance)
    float *d_ll_slab = nullptr;           // the three likelihood tables (ensure_slab)
    float *d_ll[3] = {nullptr, nullptr, nullptr};
    size_t ll_cap = 0;                    // floats per table
    int *d_row_src[3] = {nullptr, nullptr, nullptr}; size_t row_src_cap[3] = {0, 0, 0};   // row -> source frame tables, one per likelihood table
    // spliced models (jd_splice.h): the rows' spans beside them, and the host's copy a transfer reads (else null / empty)
    JdSpan *d_row_span[3] = {nullptr, nullptr, nullptr}; size_t row_span_cap[3] = {0, 0, 0};
    std::vector<JdSpan> h_row_span[3];
    int *d_T = nullptr;
    hipStream_t s_gmm = nullptr, s_search = nullptr;
    unsigned *h_park = nullptr; int *d_park = nullptr;   // jd_park_kernel's words (host-mapped state; arrival counts and quotas by XCD)
    // scoring one batch ahead (jd_dec_prefetch_scores): the table of the NEXT batch is scored while this one is searched
    std::deque<Prefetch> pf_q;            // the batches ahead, in the order announced: scored, started ("two batches in flight"), or neither yet
    int fg_buf = FG_NONE;                 // the table(s) the wave being decoded uses (or FG_NONE, FG_BOTH)
    int fg_bank = -1;                     // >= 0: the wave being decoded runs on this bank of streams and the batch behind it may be
                                          // started beside it
    int pipeline = 1;                     // two batches in flight (JD_PIPELINE=0: off)
    bool bg_ran = false;                  // the last launch_search advanced streams of the batch behind, too
    double bg_wait_us = 1000.0;           // how long the start of a launch waits for the table of the batch behind (JD_BG_WAIT_US)
    double last_wave_ms = 0.0;            // wall time of the last wave decoded (what a scoring beside the next one has to fit)
    int score_reserve = -1;               // CUs left to the scoring beside a launch with two batches in flight: -1 by its cost (JD_SCORE_RESERVE)
    int reserve_now = 0;                  // ... of the launch under way
    int bg_rebalance = 0;                 // re-plan a launch that runs two batches (JD_BG_REBALANCE)
    double bg_max_load = 4.0;             // two batches in flight up to this load_scale (JD_BG_MAX_LOAD)
    double bg_weight = 0.5;               // the plan counts this part of the frames a stream of the batch behind has ahead (JD_BG_WEIGHT)
    int fg_cw_cap = 8, bg_cw_cap = 4;     // two batches in flight: largest cluster of the running batch / of the batch behind (JD_FG_CW, JD_BG_CW)
    bool pf_armed = false;                // decode_wave: the coming launch_search may start the announced scorings
    bool pf_retry = false;                // decode_wave: this wave is being decoded again - what was scored beside its first attempt stays
    int pf_rebalance = -1;                // re-planning a launch beside which a table is scored: -1 by the measured ratio (launch_search),
                                          // JD_PF_REBALANCE=0: never while the scoring runs, =1: like any other launch
    double gmm_ms_per_row = 0.0, search_ms_per_frame = 0.0;   // measured on this decoder's last waves (scoring on its own / search)
    int *h_resident = nullptr, *d_resident = nullptr; int launch_seq = 0;   // host-mapped word: k_search's last workgroup has started
    // streaming API state: a record per stream (jd_push.h)
    std::vector<PushStream> push;
    // PARTIAL_DECODING (WFSTDecoderLite.h:199-205), streaming API
    int partial_interval = 0;                  // partialTraceInterval
    int *d_partial_out = nullptr;
    // ... k_partial_many's buffers (trace_partial_many): [int4 work list][{found, n} heads][staging], for max_streams entries, on the
    // device and pinned on the host
    int *d_pmany = nullptr, *h_pmany = nullptr;
    // ... and k_best_many's (jd_streams_best; best_layout, jd_best.h), with the launches and device-to-host copies those calls have made
    int *d_best = nullptr, *h_best = nullptr;
    int64_t best_launches = 0, best_copies = 0;
    // ... k_final_many's (jd_streams_final; final_layout, jd_final.h), with its launches and device-to-host copies
    int *d_final = nullptr, *h_final = nullptr;
    int64_t final_launches = 0, final_copies = 0;
    // ... and k_partial_many_models' (jd_streams_trace_models; partial_models_layout, jd_push.h) with the per-stream area the model lists
    // are exported into, [stream][model, label, time, score, ac, lm][res_cap]
    int *d_pmm = nullptr, *h_pmm = nullptr, *d_pmm_area = nullptr;
    // ... k_partial's export of the model-level list of the same traces (PushStream::partial_m, jd_stream_partial_models),
    // [model, label, time, score, ac, lm][res_cap] (model-level output only, allocated with d_res_model)
    int *d_partial_model = nullptr;
    bool return_on_collect = false, collected_now = false;   // jd_stream_push: launch_search comes back after a collection by the count rule
    float *d_push = nullptr; size_t push_cap = 0;
    char *h_stage = nullptr; size_t stage_cap = 0;     // pinned staging of jd_streams_push
    bool xch_forced = false;               // JD_XCH given (development)
    struct Resident *res = nullptr;        // the resident search kernel of a broker (jd_res_*), or null
    std::recursive_mutex res_mu;           // jd_res_stop / jd_res_start (the broker's worker) against jd_res_finish (its finisher thread)
    long long res_yield_turn = -1;             // the lock's turn count when the resident kernel last made room for a waiter
    std::vector<hipStream_t> res_old_streams;   // search streams the resident kernel gave up (jd_res_start)
    struct Pipe *pipe = nullptr;           // batches through the resident kernel, utterance by utterance (jd_pipe_*; JD_PIPELINE=3)
    bool pipe_mode = false;
    bool pipe_on = false;                  // Pipe::on (for the code in front of the struct)
    int pipe_depth = 8;                    // likelihood tables = batches announced and not handed back, at most (jd_dec_set_pipeline)
    int pipe_slots = 0;                    // one-workgroup slots of the resident kernel (0: max_streams)
    // jd_dec_pipeline_stats: cumulative over the decoder's life
    long long pipe_frames_searched = 0;    // stream-frames the slots have advanced, as reported command by command
    long long pipe_utts_through = 0, pipe_rows_scored = 0, pipe_batches_back = 0, pipe_collections = 0;
    long long pipe_busy_ticks = 0;         // the slots' own clocks on their commands (100 MHz)
    double pipe_on_us = 0.0;               // wall time the resident kernel has been on the device for the pipeline
    const float *res_ll = nullptr;         // the likelihood slab the resident kernel reads (null: the broker's stream buffers)
    // results
    std::vector<HostResult> results;
    jd_timing timing{};
    // lazily composed networks (jd_lazy_enter / jd_lazy_leave): a stream of the last fetch ran out of graph room;
    // streams of the streaming API that are inside an utterance
    bool lazy_failed = false;
    std::vector<char> lazy_in;
    // a stream whose last launch ended in an error, or never reported back (a wave that returned early, a push that
    // failed and was not followed by a finish): its per-state and per-arc words may be anything - wiped before its next init
    std::vector<char> stream_dirty;
    bool occupancy_ok = false;            // k_search fits a CU the way launch_search's grid assumes (checked at the first launch)
};

template <typename T>
static int dmalloc(jd_dec *d, T **p, size_t n)
{
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return jd_fail(e == hipErrorOutOfMemory ? JD_ENOMEM : JD_EHIP, "hipMalloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
    }
    d->allocs.push_back(q);
    *p = (T *)q;
    return JD_OK;
}

template <typename T>
static int dupload(jd_dec *d, T **p, const T *src, size_t n)
{
    int rc = dmalloc(d, p, n);
    if (rc) return rc;
    HIPCHK(hipMemcpy(*p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return JD_OK;
}

// A buffer that is replaced by a larger one of n elements (what it held is not kept; pinned: host memory): free, forget pointer and
// capacity, allocate, remember the capacity - a failed allocation leaves no pointer behind
template <typename T>
static int dregrow(T **p, size_t *cap, size_t n, bool pinned)
{
    if (*p) (void)(pinned ? hipHostFree(*p) : hipFree(*p));
    *p = nullptr; *cap = 0;
    if (pinned) HIPCHK(hipHostMalloc((void **)p, n * sizeof(T)));
    else HIPCHK(hipMalloc((void **)p, n * sizeof(T)));
    *cap = n;
    return JD_OK;
}

static void res_free_fwd(jd_dec *d);
static void pipe_free_fwd(jd_dec *d);
static void pipe_drain(jd_dec *d);
static int pipe_announce(jd_dec *d, int n_utts, const float *d_feats, const int64_t *offs, int *taken);
static int pipe_decode(jd_dec *d, int n_utts, const float *d_feats, const int64_t *offs, jd_hyp *out, int *handled);
extern "C" void jd_dec_destroy(jd_dec *d)
{
    if (!d) return;
    (void)hipSetDevice(d->device);
    pipe_drain(d);
    pipe_free_fwd(d);
    if (d->res) { (void)jd_res_stop(d); res_free_fwd(d); }
    (void)hipDeviceSynchronize();
    for (char in : d->lazy_in) if (in) jd_lazy_leave(d->net, 1);      // (utterances the caller never finished)
    for (void *p : d->allocs) (void)hipFree(p);
    slab_give(d->device, d->slab);
    d->slab = ArenaSlab();
    free_am_gmm(d->amb);
    if (d->d_ll_slab) (void)hipFree(d->d_ll_slab);
    if (d->d_cells) (void)hipFree(d->d_cells);
    for (int i = 0; i < 3; ++i)
        if (d->d_row_src[i]) (void)hipFree(d->d_row_src[i]);
    for (Prefetch &F : d->pf_q) F.drop();
    d->pf_q.clear();
    if (d->h_resident) (void)hipHostFree(d->h_resident);
    if (d->d_push) (void)hipFree(d->d_push);
    for (int i = 0; i < 3; ++i) if (d->d_row_span[i]) (void)hipFree(d->d_row_span[i]);
    if (d->h_stage) (void)hipHostFree(d->h_stage);
    if (d->h_pmany) (void)hipHostFree(d->h_pmany);
    if (d->h_best) (void)hipHostFree(d->h_best);
    if (d->h_final) (void)hipHostFree(d->h_final);
    if (d->h_pmm) (void)hipHostFree(d->h_pmm);
    if (d->d_work) (void)hipFree(d->d_work);
    if (d->h_status) (void)hipHostFree(d->h_status);
    if (d->s_gmm) (void)hipStreamDestroy(d->s_gmm);
    if (d->s_search) (void)hipStreamDestroy(d->s_search);
    if (d->h_park) (void)hipHostFree(d->h_park);
    if (d->d_park) (void)hipFree(d->d_park);
    for (hipStream_t st : d->res_old_streams) (void)hipStreamDestroy(st);
    delete d;
}

// ---- jd_dec_create, step by step.  What the search kernels see of the graph and the models is decided in jd_prep.h (pure, tested on
// the CPU: tests/test_prep_cpu.py); the steps here read the knobs, say what was decided (JD_VERBOSE) and upload it.  A step that fails
// returns its code and jd_dec_create destroys the decoder.

static int dec_check_args(jd_dec **out, const jd_net *net, const jd_am *am, float main_beam, int32_t max_hyps, int32_t block_size,
                          int32_t device, int32_t max_streams, PrepHist *hist)
{
    if (!out || !net || !am) return jd_fail(JD_EINVAL, "jd_dec_create: null argument");
    if (block_size < 1 || block_size > 20)      // HTKFlatModels::setBlockSize, HTKFlatModels.cpp:311-312
        return jd_fail(JD_EINVAL, "HTKFlatModels::setBlockSize fnBlock should be in [1, 20]");
    if (max_streams < 1) return jd_fail(JD_EINVAL, "jd_dec_create: max_streams < 1");
    if (net->max_in > am->n_hmm)
        return jd_fail(JD_EINVAL, "network input label %d exceeds the number of HMMs %d", net->max_in, am->n_hmm);
    if (am->max_n > JD_MAXN) return jd_fail(JD_EINVAL, "HMMs with more than %d states unsupported", JD_MAXN);
    if (am->n_hmm >= SOLE_FLAG || am->n_tm > 0x1fffff)                    // (the flag bits of a device arc's in-label and of a record's header)
        return jd_fail(JD_EINVAL, "more than %d HMMs or %d transition matrices unsupported", SOLE_FLAG - 1, 0x1fffff);
    if ((int64_t)net->n_states * (int64_t)sizeof(StateRec) > 0xf0000000LL)   // (32-bit byte offsets of the buffer descriptor)
        return jd_fail(JD_EINVAL, "networks with more than %lld states unsupported", (long long)(0xf0000000LL / (int64_t)sizeof(StateRec)));
    int rc = check_device(device);
    if (rc) return rc;
    *hist = prep_hist(main_beam, max_hyps);
    if (hist->hist_nbins > HIST_MAX_BINS)
        return jd_fail(JD_EINVAL, "mainBeam %.1f needs %d histogram bins (> %d supported)", main_beam, hist->hist_nbins, HIST_MAX_BINS);
    if (net->lazy_dev && net->lazy_device != device)
        return jd_fail(JD_EINVAL, "jd_dec_create: the lazily composed network lives on device %d, not %d", net->lazy_device, device);
    return JD_OK;
}

// the development knobs of the preparation (docs/DEV_KNOBS.md), as jd_prep.h takes them
static PrepKnobs dec_prep_knobs()
{
    PrepKnobs k;
    if (const char *e = jd_dev_env("JD_RENUMBER")) k.renumber = atoi(e) != 0;
    if (jd_dev_env("JD_NO_XSORT")) k.xsort = 0;
    if (jd_dev_env("JD_NO_SOLE")) k.sole = 0;
    if (const char *e = jd_dev_env("JD_XCUT")) k.xcut = atoi(e) != 0;
    if (const char *e = jd_dev_env("JD_SREC_SPLIT")) k.srec_split = std::max(0, std::min(2, atoi(e)));
    if (jd_dev_env("JD_NO_LR")) k.no_lr = 1;
    return k;
}

// The graph as the kernels see it: the decoder's own state numbering, arc order and arc flags, the layout of the per-state words, the
// final weights.  A lazily composed network has no graph of its own to prepare: joint records unless the knob says otherwise, no XState.
static int dec_upload_graph(jd_dec *d, const PrepKnobs &knobs, const std::vector<float> &tmax0)
{
    const jd_net *net = d->net;
    DecConst &C = d->C;
    const bool lazy = net->lazy_dev != nullptr, verbose = getenv("JD_VERBOSE") != nullptr;
    int rc;
    PrepNumbering N;
    if (!lazy) {
        N = prep_renumber(*net, knobs.renumber);
        if (N.tried && verbose) fprintf(stderr, "state numbers: %s\n", N.same ? "the network's (already along its chains)" : "the decoder's own (a state, the chains behind its arcs side by side)");
    }
    const std::vector<int32_t> &row_ptr_h = N.state_new.empty() ? net->row_ptr : N.row_ptr;
    const std::vector<JdArc> &arcs_h = N.state_new.empty() ? net->arcs : N.arcs;
    if (!lazy) {
        if ((rc = dupload(d, &d->d_row_ptr, row_ptr_h.data(), row_ptr_h.size()))) return rc;
        const PrepArcs A = prep_arcs(row_ptr_h, arcs_h, net->n_states, *d->am, tmax0, knobs);
        if (verbose) fprintf(stderr, "exit tokens that recombine with nobody: those of %lld of %lld model arcs (the only arc into their state)\n", (long long)A.n_sole, (long long)A.n_model);
        if ((rc = dupload(d, &d->d_arcs, A.arcs.data(), A.arcs.size()))) return rc;
        if ((rc = dupload(d, &d->d_xst, A.xst.data(), A.xst.size()))) return rc;
        C.xcut = A.xcut;
        if (verbose) fprintf(stderr, "arc order: %lld of %lld model arcs in sorted rows (<= %d arcs), %d states; k_search cuts walks: %d\n",
                             (long long)A.n_sorted, (long long)A.n_model_all, XSORT_MAX_ROW, net->n_states, C.xcut);
    }
    const PrepSrec S = prep_srec_layout(row_ptr_h, arcs_h, net->n_states, net->n_arcs, knobs.srec_split);
    C.srec_stride = S.stride; C.srec_arr = S.arr; C.srec_estride = S.estride; C.srec_par = S.par;
    if (verbose) fprintf(stderr, "per-state words: %s (%lld of %lld arcs lead to the next state number)\n",
                         S.split == 2 ? "split (bids | arrival keys of either frame parity)" : S.split ? "split (bids | arrival keys)" : "joint records",
                         (long long)S.n_next, (long long)net->n_arcs);
    if (!lazy) {
        if (N.state_new.empty()) rc = dupload(d, &d->d_fin_w, net->fin_w.data(), net->fin_w.size());
        else {
            const std::vector<float> fw = permute_by_state(N.state_new, net->fin_w);
            rc = dupload(d, &d->d_fin_w, fw.data(), fw.size());
        }
        if (rc) return rc;
    }
    d->state_new = std::move(N.state_new);
    return JD_OK;
}

static int dec_upload_models(jd_dec *d, const PrepModels &M)
{
    const jd_am *am = d->am;
    int rc;
    if ((rc = dupload(d, &d->d_hmm_tee, am->hmm_tee.data(), am->hmm_tee.size()))) return rc;
    if ((rc = dupload(d, &d->d_hmm_tmax0, M.tmax0.data(), M.tmax0.size()))) return rc;     // (phase X, hopeless candidates)
    if ((rc = dupload(d, &d->d_trP, am->trP.data(), am->trP.size()))) return rc;
    if ((rc = dupload(d, &d->d_se32, M.se32.data(), M.se32.size()))) return rc;
    if ((rc = upload_am_gmm(am, d->amb))) return rc;
    if ((rc = dupload(d, &d->d_aux, M.aux.data(), M.aux.size()))) return rc;
    if (!M.lrt.empty() && (rc = dupload(d, &d->d_lrt, M.lrt.data(), M.lrt.size()))) return rc;
    return JD_OK;
}

// what the kernels are handed of all that (the pruning windows and the histogram's range are set before the uploads)
static void dec_fill_const(jd_dec *d)
{
    const jd_net *net = d->net;
    const jd_am *am = d->am;
    DecConst &C = d->C;
    C.row_ptr = d->d_row_ptr; C.arcs = d->d_arcs; C.fin_w = d->d_fin_w; C.init_state = d->state_new.empty() ? net->init : d->state_new[(size_t)net->init]; C.n_states = net->n_states;
    C.xst = d->d_xst;
    C.G = am->n_gmm; C.max_n = am->max_n; C.n_tm = am->n_tm;
    C.hmm_tee = d->d_hmm_tee; C.n_hmm = am->n_hmm; C.hmm_tmax0 = d->d_hmm_tmax0;
    C.lazy = (const LazyDev *)net->lazy_dev; C.aux_h = d->d_aux;
    C.trP = d->d_trP; C.se32 = d->d_se32;
    C.lrt = d->d_lrt;
}

// the planner's and the pipeline's development knobs (docs/DEV_KNOBS.md)
static void dec_read_planner_knobs(jd_dec *d)
{
    if (const char *e = jd_dev_env("JD_CW")) { const int v = atoi(e); if (v >= 1 && v <= MAXCW) d->max_cw = v; }   // development
    if (const char *e = jd_dev_env("JD_WEIGHTED")) d->weighted = atoi(e) != 0;
    if (const char *e = jd_dev_env("JD_REBALANCE")) d->rebalance = atoi(e) != 0;
    if (const char *e = jd_dev_env("JD_REBALANCE_FRAC")) { const double v = atof(e); if (v > 0.0 && v < 1.0) d->rebalance_frac = v; }
    if (const char *e = jd_dev_env("JD_REBALANCE_MIN_US")) d->rebalance_min_us = atof(e);
    if (const char *e = jd_dev_env("JD_MODEL_A")) d->model_a_us = atof(e);
    if (const char *e = jd_dev_env("JD_MODEL_B")) d->model_b_us = atof(e);
    if (const char *e = jd_dev_env("JD_PLAN")) d->plan_mode = atoi(e) != 0;
    if (const char *e = jd_dev_env("JD_PLAN_MIN_CW")) d->plan_min_cw = std::max(1, atoi(e));
    if (const char *e = jd_dev_env("JD_PF_GMM_WEIGHT")) d->pf_gmm_weight = atof(e);
    if (const char *e = jd_dev_env("JD_MODEL2_A")) d->model2_a_us = atof(e);
    if (const char *e = jd_dev_env("JD_MODEL2_B")) d->model2_b_us = atof(e);
    if (const char *e = jd_dev_env("JD_XCD_LOCAL")) d->xl_ok = atoi(e) != 0;                      // development
    if (const char *e = jd_dev_env("JD_XL_SLACK")) { const double v = atof(e); if (v >= 1.0 && v <= 10.0) d->xl_slack = v; }
    // arena capacities: 0 = sized from the free HBM when the arenas are allocated (ensure_arenas)
    d->cap_slots = d->cap_items = d->cap_paths = d->cap_new = 0;
    if (const char *e = jd_dev_env("JD_PF_REBALANCE")) d->pf_rebalance = atoi(e) != 0;                // development
    if (const char *e = jd_dev_env("JD_PIPELINE")) { d->pipeline = atoi(e) != 0; d->pipe_mode = atoi(e) == 3; }
    if (const char *e = jd_dev_env("JD_PIPE_DEPTH")) { const int v = atoi(e); if (v >= 2 && v <= 32) d->pipe_depth = v; }
    if (const char *e = jd_dev_env("JD_BG_WAIT_US")) d->bg_wait_us = atof(e);
    if (const char *e = jd_dev_env("JD_SCORE_RESERVE")) d->score_reserve = atoi(e);
    if (const char *e = jd_dev_env("JD_BG_REBALANCE")) d->bg_rebalance = atoi(e) != 0;
    if (const char *e = jd_dev_env("JD_BG_WEIGHT")) d->bg_weight = atof(e);
    if (const char *e = jd_dev_env("JD_BG_MAX_LOAD")) d->bg_max_load = atof(e);
    if (const char *e = jd_dev_env("JD_FG_CW")) d->fg_cw_cap = std::max(1, atoi(e));
    if (const char *e = jd_dev_env("JD_BG_CW")) d->bg_cw_cap = std::max(1, atoi(e));
    if (const char *e = jd_dev_env("JD_RES_CAP")) { const int v = atoi(e); if (v >= 16 && v <= (1 << 20)) d->res_cap = v; }   // (tests)
}

// the two HIP streams, the host-mapped "resident" word and the per-stream host state
static int dec_create_streams(jd_dec *d)
{
    hipError_t e;
    // the search stream has the highest priority, the scoring stream the lowest: when a table is scored while a search
    // runs (jd_dec_prefetch_scores) a search launch that needs CUs gets them before further scoring blocks do
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if ((e = hipStreamCreateWithPriority(&d->s_gmm, hipStreamNonBlocking, prio_lo)) != hipSuccess ||
        (e = hipStreamCreateWithPriority(&d->s_search, hipStreamNonBlocking, prio_hi)) != hipSuccess)
        return jd_fail(JD_EHIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    if ((e = hipHostMalloc((void **)&d->h_resident, 64, hipHostMallocMapped)) != hipSuccess ||
        (e = hipHostGetDevicePointer((void **)&d->d_resident, d->h_resident, 0)) != hipSuccess)
        return jd_fail(JD_EHIP, "hipHostMalloc failed: %s", hipGetErrorString(e));
    *d->h_resident = 0;
    const size_t n = (size_t)d->max_streams;
    d->push.assign(n, PushStream());
    d->lazy_in.assign(n, 0);
    d->stream_dirty.assign(n, 0);
    d->results.resize(n);
    return JD_OK;
}

extern "C" int jd_dec_create(jd_dec **out, const jd_net *net, const jd_am *am, float start_beam, float main_beam,
                             float end_beam, float word_beam, int32_t max_hyps, int32_t block_size,
                             int32_t device, int32_t max_streams)
{
    PrepHist hist;
    int rc = dec_check_args(out, net, am, main_beam, max_hyps, block_size, device, max_streams, &hist);
    if (rc) return rc;
    jd_dec *d = new jd_dec();
    d->net = net; d->am = am; d->device = device; d->max_streams = max_streams; d->block_size = block_size;
    // development: frames per chunk of a batch
    if (const char *e = jd_dev_env("JD_FC")) { const int v = atoi(e); if (v >= 16 && v <= 65536) d->Fw_env = v; }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) d->n_cus = prop.multiProcessorCount;
    }
    DecConst &C = d->C;
    C.start_win = start_beam; C.emit_win = main_beam; C.end_win = end_beam; C.word_win = word_beam;
    C.max_hyps = max_hyps;
    C.x_chunks = 2;
    if (const char *e = jd_dev_env("JD_XCH")) { const int v = atoi(e); if (v >= 1 && v <= 16) { C.x_chunks = v; d->xch_forced = true; } }   // development
    C.exp = 0; C.path_rule = 0; C.pcount = nullptr;
    if (const char *e = jd_dev_env("JD_EXP")) C.exp = atoi(e);                                                    // development
    C.hist_min = hist.hist_min; C.hist_max = hist.hist_max; C.hist_nbins = hist.hist_nbins;
    const PrepKnobs knobs = dec_prep_knobs();
    const PrepModels M = prep_models(*am, knobs);
    if ((rc = dec_upload_graph(d, knobs, M.tmax0)) || (rc = dec_upload_models(d, M))) { jd_dec_destroy(d); return rc; }
    dec_fill_const(d);
    dec_read_planner_knobs(d);
    if ((rc = dec_create_streams(d))) { jd_dec_destroy(d); return rc; }
    *out = d;
    return JD_OK;
}

extern "C" int jd_dec_set_capacity(jd_dec *d, int64_t max_slots, int64_t max_paths, int64_t max_items)
{
    if (!d) return jd_fail(JD_EINVAL, "jd_dec_set_capacity: null");
    if (d->arenas_ready) return jd_fail(JD_ESTATE, "jd_dec_set_capacity: arenas already allocated");
    if (max_slots > 0) d->cap_slots = max_slots;
    if (max_paths > 0) d->cap_paths = max_paths;
    if (max_items > 0) d->cap_items = max_items;
    return JD_OK;
}

// setMaxAllocModels (WFSTDecoderLite.cpp:807-820): same argument convention - below 100 a percentage
// of the network's transitions, 100..7999 a memory limit in MB, from 8000 a number of instances.  In the
// reference it is a SOFT limit: it is compared with the NetInst objects the pools have handed out, and when there
// are more they are all dropped between two utterances (:164-169) - a cap on what stays cached, never a
// reason for a decode to fail.  Here instance memory is one arena of records per stream that every utterance
// reuses wholesale, so nothing is cached from one utterance to the next and there is nothing to drop: the value
// is validated and kept as a hint that can only RAISE the arena above its automatic size (a caller who asks
// for room for more instances gets it), never lower it.  A hard capacity is jd_dec_set_capacity's business.
extern "C" int jd_dec_set_max_alloc_models(jd_dec *d, int32_t max_alloc_models)
{
    if (!d || max_alloc_models <= 0) return jd_fail(JD_EINVAL, "setMaxAllocModels: maxAllocModels > 0");
    if (d->arenas_ready) return jd_fail(JD_ESTATE, "jd_dec_set_max_alloc_models: arenas already allocated");
    int64_t n;
    // (a lazily composed network's n_arcs is the capacity it may grow into: the most it can ever hold)
    if (max_alloc_models < 100) n = d->net->n_arcs * max_alloc_models / 100;                        // :809-811
    // :812-814, sizeof(NetInst) + sizeof(Token) * nStatePools
    else if (max_alloc_models < 8000) n = (int64_t)max_alloc_models * 1024 * 1024 / (40 + 24 * (int64_t)d->am->max_n);
    else n = max_alloc_models;                                                                       // :815-817
    d->slots_hint = std::min<int64_t>(n, d->net->n_arcs + 65536);      // (one instance per arc at most)
    return JD_OK;
}

// reset a stream's per-state records: no bids, no arrivals; the CSR row of the state (row_ptr == nullptr: a lazy
// graph, rows live elsewhere)
__global__ void jd_reset_srec_kernel(StateRec *srec, const int *row_ptr, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        (void)row_ptr;
        srec[i] = StateRec{0ULL, 0ULL, {0ULL, 0ULL}};
    }
}
static void reset_srec(StateRec *srec, const int *d_row_ptr, int64_t n_states)
{
    hipLaunchKernelGGL(jd_reset_srec_kernel, dim3((unsigned)((n_states + 255) / 256)), dim3(256), 0, 0, srec, d_row_ptr, (long long)n_states);
}

// ---- ensure_arenas, step by step.  How large the arenas are and where each piece lies is decided in jd_arena.h (pure, tested on the
// CPU: tests/test_arena_cpu.py); the steps below ask HIP for the memory there is, call it, allocate and clear.

// what jd_arena.h has to know of the kernels' structs (the literals: what tests/arena_driver.cpp is run with - a struct that grows
// fails the build here instead of moving the recorded capacities)
static ArenaSizes arena_sizes()
{
    static_assert(RecLayout<3>::REC_BYTES == 80 && RecLayout<6>::REC_BYTES == 144, "tests/golden/arena_golden.json: rec_bytes");
    static_assert(sizeof(PathRec) == 32 && sizeof(Tok) == 16 && sizeof(int4) == 16 && sizeof(StateRec) == 32, "tests/golden/arena_golden.json: sizes");
    static_assert(sizeof(int2) == 8 && sizeof(GcState) == 4 * 68, "tests/golden/arena_golden.json: newl, gc_words");
    static_assert(TOT_N == 10 && MAXW == 512 && HIST_MAX_BINS == 2048 && SW == 8, "tests/golden/arena_golden.json: tot_n, maxw, hist_bins, sw");
    return ArenaSizes{RecLayout<3>::REC_BYTES, RecLayout<6>::REC_BYTES, sizeof(PathRec), sizeof(Tok), sizeof(int4), sizeof(StateRec),
                      (int)(sizeof(GcState) / 4), TOT_N, MAXW, HIST_MAX_BINS, SW};
}

// what arena_caps was given and how many fit passes it ran: ensure_arenas' JD_VERBOSE line
struct ArenaAttempt { ArenaIn in{}; int passes = 0; };

// the capacities of a stream's arenas (arena_caps) from the free memory and the cached slab, into d and d->C
static int arenas_pick_caps(jd_dec *d, double mem_fraction, ArenaAttempt *att)
{
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    ArenaIn &in = att->in;
    in = ArenaIn{free_b, slab_cached_bytes(d->device), mem_fraction, d->max_streams, d->net->n_arcs, d->net->n_states,
                 d->Fc, d->am->n_gmm, d->am->max_n, d->cap_slots, d->cap_items, d->cap_paths, d->slots_hint, arena_sizes()};
    ArenaCaps caps;
    arena_caps(in, &caps);
    att->passes = caps.passes;
    d->cap_slots = caps.cap_slots; d->cap_items = caps.cap_items; d->cap_paths = caps.cap_paths;
    if (caps.status == ARENA_TOO_LARGE)
        return jd_fail(JD_EINVAL, "arena capacity too large (instance records and frontier items are addressed "
                       "with 32-bit byte offsets: at most %lld / %lld records)", (long long)caps.lim_rec, (long long)caps.lim_item);
    d->cap_new = caps.cap_new;
    d->C.cap_slots = (unsigned)d->cap_slots; d->C.cap_items = (unsigned)d->cap_items; d->C.cap_new = (unsigned)d->cap_new;
    d->C.cap_paths = (int)d->cap_paths;
    d->C.gc_threshold = (int)caps.gc_threshold;
    return JD_OK;
}

// the result arena of all streams (and, for model-level output, the records' models beside it)
static int arenas_alloc_results(jd_dec *d)
{
    const size_t B = (size_t)d->max_streams;
    int rc = dmalloc(d, &d->d_res, B * 5 * d->res_cap);
    if (rc) return rc;
    if (d->models) {                                                   // (model-level output only; else jd_dec_set_output_level)
        rc = dmalloc(d, &d->d_res_model, B * d->res_cap);
        if (rc) return rc;
        rc = dmalloc(d, &d->d_partial_model, (size_t)6 * d->res_cap);
        if (rc) return rc;
    }
    return JD_OK;
}

// ONE slab for all streams (slab_take: the previous decoder's when there is one), a stream's share carved up into
// 256-byte aligned pieces (arena_layout).  What a decoder's set-up costs is the BYTES the driver has to clear:
// 25-60 GB/s (tools/alloc_probe.py), i.e. seconds for the default 70 % of a 288 GB device.
static int arenas_take_and_carve(jd_dec *d)
{
    const int B = d->max_streams;
    size_t off[AR_N];
    const ArenaDims dims = {d->cap_slots, d->cap_items, d->cap_paths, d->cap_new, d->net->n_arcs, d->net->n_states, d->am->max_n, arena_sizes()};
    const size_t stream_bytes = arena_layout(dims, off);               // (the same for every stream)
    const int rc = slab_take(d->device, stream_bytes * (size_t)B, &d->slab);
    if (rc) return rc;
    d->h_streams.assign((size_t)B, StreamDev());
    for (int s = 0; s < B; ++s) {
        StreamDev &S = d->h_streams[(size_t)s];
        memset(&S, 0, sizeof S);
        char *blk = (char *)d->slab.p + (size_t)s * stream_bytes;
        S.rec = (int *)(blk + off[AR_REC]);
        S.live = (unsigned char *)(blk + off[AR_LIVE]);
        S.srec = (StateRec *)(blk + off[AR_SREC]);
        S.items = (int4 *)(blk + off[AR_ITEMS]);
        S.newl = (int2 *)(blk + off[AR_NEWL]);
        S.dirtyl = (int *)(blk + off[AR_DIRTYL]);
        S.tot = (int *)(blk + off[AR_TOT]);
        S.item_end = (int *)(blk + off[AR_ITEM_END]);
        S.paths = (PathRec *)(blk + off[AR_PATHS]);
        S.paths2 = (PathRec *)(blk + off[AR_PATHS2]);
        S.gc_idx = (int *)(blk + off[AR_GC_IDX]);
        S.gc_state = (int *)(blk + off[AR_GC_STATE]);
        S.hist = (int *)(blk + off[AR_HIST]);
        // the five result arrays of all streams live in one arena [stream][array][res_cap]:
        // fetch_results brings a whole wave back with a single strided copy
        int *base = d->d_res + (size_t)s * 5 * d->res_cap;
        S.res_label = base; S.res_time = base + d->res_cap;
        S.res_score = (float *)(base + 2 * (size_t)d->res_cap); S.res_ac = (float *)(base + 3 * (size_t)d->res_cap);
        S.res_lm = (float *)(base + 4 * (size_t)d->res_cap);
        S.res_cap = d->res_cap;
    }
    return JD_OK;
}

// nothing in the arenas needs to be clear except the per-arc and per-state words and the waves' counts
static int arenas_clear(jd_dec *d)
{
    for (const StreamDev &S : d->h_streams) {
        HIPCHK(hipMemset(S.live, 0, (size_t)d->net->n_arcs));          // per arc: no instance
        reset_srec(S.srec, d->d_row_ptr, d->net->n_states);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemset(S.hist, 0, 2 * HIST_MAX_BINS * sizeof(int)));
        HIPCHK(hipMemset(S.tot, 0, TOT_N * MAXW * sizeof(int)));
        HIPCHK(hipMemset(S.item_end, 0, MAXW * sizeof(int)));
    }
    return JD_OK;
}

// the streams' arena pointers, frame counts and control blocks on the device, and the status words
static int arenas_alloc_ctl(jd_dec *d)
{
    const size_t B = (size_t)d->max_streams;
    int rc = dmalloc(d, &d->d_streams, B);
    if (rc) return rc;
    HIPCHK(hipMemcpy(d->d_streams, d->h_streams.data(), B * sizeof(StreamDev), hipMemcpyHostToDevice));
    rc = dmalloc(d, &d->d_T, B);
    if (rc) return rc;
    rc = dmalloc(d, &d->d_ctl, B);
    if (rc) return rc;
    rc = dmalloc(d, &d->d_status, 8);
    if (rc) return rc;
    HIPCHK(hipMemset(d->d_status, 0, 8 * sizeof(int)));
    HIPCHK(hipHostMalloc((void **)&d->h_status, 8 * sizeof(int)));
    std::vector<StreamCtl> hc(B);
    memset(hc.data(), 0, hc.size() * sizeof(StreamCtl));
    for (auto &c : hc) {
        c.needs_init = 1; c.best_emit = LZ;
        c.best_final.score = LZ; c.best_final.ac = LZ; c.best_final.lm = LZ; c.best_final.path = -1;
    }
    HIPCHK(hipMemcpy(d->d_ctl, hc.data(), hc.size() * sizeof(StreamCtl), hipMemcpyHostToDevice));
    return JD_OK;
}

static int ensure_slab(jd_dec *d, size_t floats);
static int ensure_arenas_try(jd_dec *d, double mem_fraction, ArenaAttempt *att)
{
    int rc = check_device(d->device);
    if (rc) return rc;
    if ((rc = arenas_pick_caps(d, mem_fraction, att)) || (rc = arenas_alloc_results(d)) || (rc = arenas_take_and_carve(d)) ||
        (rc = arenas_clear(d)) || (rc = arenas_alloc_ctl(d)))
        return rc;
    rc = ensure_slab(d, (size_t)d->Fc * d->am->n_gmm);                // streaming API: one stream, one chunk
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    d->arenas_ready = true;
    return JD_OK;
}

// The default capacities take 70% of the device's free memory.  When that cannot be had - another
// process on the same GPU sized itself at the same moment - the defaults are halved, up to three times.
static int ensure_arenas(jd_dec *d)
{
    if (d->arenas_ready) return JD_OK;
    const auto t_start = std::chrono::steady_clock::now();
    ArenaAttempt att;                                                  // (the last attempt's: the one that succeeded, when one did)
    struct Report { jd_dec *d; const ArenaAttempt *att; std::chrono::steady_clock::time_point t0;
        ~Report() { if (getenv("JD_VERBOSE")) fprintf(stderr, "arenas: slots %lld, items %lld, Path records %lld per stream x %d streams in %.3f s "
                                                      "(free %zu, cached %zu bytes, fraction %.17g, %d fit passes)\n",
                                                      (long long)d->cap_slots, (long long)d->cap_items, (long long)d->cap_paths, d->max_streams,
                                                      std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(),
                                                      att->in.free_bytes, att->in.cached_bytes, att->in.mem_fraction, att->passes); } } report{d, &att, t_start};
    const int64_t u_slots = d->cap_slots, u_items = d->cap_items, u_paths = d->cap_paths;   // <= 0: not set by the caller
    double frac = 0.7;
    for (int attempt = 0;; ++attempt) {
        const size_t mark = d->allocs.size();
        const int rc = ensure_arenas_try(d, frac, &att);
        if (rc == JD_OK) return JD_OK;
        for (size_t i = mark; i < d->allocs.size(); ++i) (void)hipFree(d->allocs[i]);
        d->allocs.resize(mark);
        slab_give(d->device, d->slab);
        d->slab = ArenaSlab();
        if (d->h_status) { (void)hipHostFree(d->h_status); d->h_status = nullptr; }
        if (d->d_ll_slab) { (void)hipFree(d->d_ll_slab); d->d_ll_slab = nullptr; d->ll_cap = 0; for (int i = 0; i < 3; ++i) d->d_ll[i] = nullptr; }
        d->d_res = nullptr; d->d_res_model = nullptr; d->d_partial_model = nullptr; d->d_streams = nullptr; d->d_T = nullptr; d->d_ctl = nullptr; d->d_status = nullptr;
        (void)hipGetLastError();
        if (rc != JD_ENOMEM || attempt == 3 || (u_slots > 0 && u_items > 0 && u_paths > 0)) return rc;
        d->cap_slots = u_slots; d->cap_items = u_items; d->cap_paths = u_paths; d->cap_new = 0;
        frac *= 0.5;
    }
}

// After an error the lists a stream's next init would clean up from cannot be trusted (stale bids, arrival keys or
// instance flags would silently drop tokens of later utterances): everything per state and per arc is wiped.
static int wipe_stream(jd_dec *d, int s)
{
    const StreamDev &S = d->h_streams[(size_t)s];
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(S.live, 0, (size_t)d->net->n_arcs));
    reset_srec(S.srec, d->d_row_ptr, d->net->n_states);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemset(S.tot, 0, TOT_N * MAXW * sizeof(int)));
    HIPCHK(hipMemset(S.item_end, 0, MAXW * sizeof(int)));
    HIPCHK(hipMemset(S.hist, 0, 2 * HIST_MAX_BINS * sizeof(int)));
    HIPCHK(hipDeviceSynchronize());
    d->stream_dirty[(size_t)s] = 0;
    return JD_OK;
}

// mark streams [s0, s0+n) for re-initialisation (IDecoder::init)
static int mark_init(jd_dec *d, int s0, int n, hipStream_t st)
{
    for (int s = s0; s < s0 + n; ++s)
        if (d->stream_dirty[(size_t)s]) { const int rc = wipe_stream(d, s); if (rc) return rc; }
    hipLaunchKernelGGL(jd_mark_init_kernel, dim3((n + 63) / 64), dim3(64), 0, st, d->d_ctl, s0, n);
    HIPCHK(hipGetLastError());
    return JD_OK;
}

// results -> out[out_idx[i]] (out_idx == nullptr: out[out0 + i]): of streams [s0, s0+n), or - resn_v != null - of the virtual
// result slots [s0, s0+n) the batch pipeline exported them to (ctl_v / resn_v / res_v: their control blocks, word counts and
// result arrays; slot_of: the streams they ran on, for the messages and the dirty marks)
// A stream's device-side error word (StreamCtl::error) as the library's code + message
static int report_stream_error(jd_dec *d, int s_i, int error, int frame, int lst_nw)
{
    if (error == JD_EHIST) return jd_fail(JD_EHIST, "Histogram::addScore - score > maxScore (stream %d)", s_i);
    if (error == JDE_BARRIER)
        return jd_fail(JD_EHIP, "stream %d: a workgroup of the search cluster did not arrive at a barrier (frame %d)", s_i, frame);
    if (error == JDE_LAZY_INV)
        return jd_fail(JD_EHIP, "stream %d: internal error - a token reached a composed state that has not been expanded (frame %d)", s_i, frame);
    if (error == JDE_GEOM)
        return jd_fail(JD_ESTATE, "stream %d: the slot kernel was given a stream in the middle of an utterance (frame %d) whose lists were written by a "
                       "cluster of %d wave segments, not its own %d: the utterance is lost, the stream is reset by its next jd_stream_init", s_i, frame,
                       lst_nw, SW);
    if (error == JDE_LAZY) {
        d->lazy_failed = true;
        LazyDev L;
        int why = 0;
        if (hipMemcpy(&L, d->net->lazy_dev, sizeof L, hipMemcpyDeviceToHost) == hipSuccess)
            (void)hipMemcpy(&why, L.err, sizeof why, hipMemcpyDeviceToHost);
        return jd_fail(JD_ENOMEM, "stream %d: the lazily composed network ran out of %s at frame %d (capacity %d states, %lld arcs): "
                       "what was being decoded at once needs a network with larger max_states / max_arcs", s_i,
                       why == 1 ? "states" : why == 2 ? "arcs"
                                : "stack closing a state (epsilon / tee arcs more than a hundred deep, or a cycle of them)",
                       frame, d->net->n_states, (long long)d->net->n_arcs);
    }
    const char *what = error == JDE_SLOTS ? "instance slots" : error == JDE_ITEMS ? "frontier items"
                     : error == JDE_PATHS ? "Path records" : error == JDE_NEW ? "newly entered arcs" : "arena";
    const long long cap = error == JDE_SLOTS ? d->cap_slots : error == JDE_ITEMS ? d->cap_items : error == JDE_NEW ? d->cap_new : d->cap_paths;
    return jd_fail(JD_ENOMEM, "stream %d: device arena overflow at frame %d: %s (capacity %lld, split over %d wave segments); raise it with "
                   "jd_dec_set_capacity", s_i, frame, what, cap, error == JDE_PATHS ? 1 : std::max(lst_nw, 1));
}

// the model array of the finish kernels: model-level output only
static int *res_model_of(jd_dec *d) { return d->models ? d->d_res_model : nullptr; }

// resm_v: the virtual slots' model arrays (model-level output; with resn_v)
static int fetch_results_from(jd_dec *d, const StreamCtl *ctl_v, const int *resn_v, const int *res_v, const int *slot_of, int s0, int n,
                              jd_hyp *out, int out0, const int *out_idx, const int *resm_v = nullptr)
{
    std::vector<StreamDev> hs((size_t)n);
    std::vector<StreamCtl> hc((size_t)n);
    if (resn_v) {
        std::vector<int> rn((size_t)n);
        HIPCHK(hipMemcpy(rn.data(), resn_v + s0, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) hs[(size_t)i].res_n = rn[(size_t)i];
        HIPCHK(hipMemcpy(hc.data(), ctl_v + s0, (size_t)n * sizeof(StreamCtl), hipMemcpyDeviceToHost));
    } else {
        HIPCHK(hipMemcpy(hs.data(), d->d_streams + s0, (size_t)n * sizeof(StreamDev), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hc.data(), d->d_ctl + s0, (size_t)n * sizeof(StreamCtl), hipMemcpyDeviceToHost));
    }
    const int *res_base = resn_v ? res_v : d->d_res;
    int first_err = JD_OK;
    int kmax = 0;
    for (int i = 0; i < n; ++i) kmax = std::max(kmax, std::min(hs[(size_t)i].res_n, d->res_cap));
    std::vector<int> hres((size_t)n * 5 * std::max(kmax, 0));
    if (kmax > 0)                                                      // rows = (stream, array), first kmax words of each
        HIPCHK(hipMemcpy2D(hres.data(), (size_t)kmax * 4, res_base + (size_t)s0 * 5 * d->res_cap, (size_t)d->res_cap * 4,
                           (size_t)kmax * 4, (size_t)n * 5, hipMemcpyDeviceToHost));
    const int *resm_base = resn_v ? resm_v : d->d_res_model;
    std::vector<int> hmod;
    if (d->models && kmax > 0) {
        hmod.resize((size_t)n * kmax);
        HIPCHK(hipMemcpy2D(hmod.data(), (size_t)kmax * 4, resm_base + (size_t)s0 * d->res_cap, (size_t)d->res_cap * 4,
                           (size_t)kmax * 4, (size_t)n, hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < n; ++i) {
        const StreamDev &S = hs[(size_t)i];
        const StreamCtl &K = hc[(size_t)i];
        const int s_i = slot_of ? slot_of[i] : s0 + i;                  // the stream it ran on
        const int oi = out_idx ? out_idx[i] : out0 + i;
        HostResult &R = d->results[(size_t)oi];
        jd_hyp &H = out[oi];
        memset(&H, 0, sizeof H);
        if (K.error && first_err == JD_OK) first_err = report_stream_error(d, s_i, K.error, K.frame, K.lst_nw);
        if (K.error) d->stream_dirty[(size_t)(s_i)] = 1;            // arenas may be inconsistent after an abort: wiped before the next init
        H.stats.n_frames = K.frame;
        H.stats.tot_active_emit_hyps = K.st[ST_EMIT];
        H.stats.tot_active_end_hyps = K.st[ST_END];
        H.stats.tot_active_models = K.st[ST_MODELS];
        H.stats.tot_proc_emit_hyps = K.st[ST_PEMIT];
        H.stats.tot_proc_end_hyps = K.st[ST_PEND];
        H.stats.tot_arcs_visited = K.st[ST_ARCS];
        H.stats.tot_paths = K.st[ST_PATHS];
        H.stats.tot_insts_in = K.st[ST_INSTS];
        H.stats.tot_recs_read = K.st[ST_RECS]; H.stats.tot_new_attached = K.st[ST_NEWL]; H.stats.tot_recs_written = K.st[ST_SURV]; H.stats.tot_entry_items = K.st[ST_KEYS];
        H.stats.tot_items_expanded = K.st[ST_XITEMS]; H.stats.tot_arcs_walked = K.st[ST_WALK]; H.stats.tot_closure_items = K.st[ST_CLOS]; H.stats.tot_bids_placed = K.st[ST_BIDS];
        d->load_sum += (double)K.st[ST_INSTS] + (double)K.st[ST_ARCS]; d->load_frames += (double)K.frame;
        H.stats.ties = 0;
        int k = S.res_n;
        if (k > d->res_cap) {
            if (first_err == JD_OK)
                first_err = d->models ? jd_fail(JD_ENOMEM, "stream %d: the model-level result has %d entries (> %d, the result capacity)", s_i, k, d->res_cap)
                                      : jd_fail(JD_ENOMEM, "stream %d: hypothesis has %d words (> %d)", s_i, k, d->res_cap);
            k = d->res_cap;
        }
        if (d->models) {
            // model-level output: the chain as it is (entry 0 and the totals carry the final-state weight) ...
            const size_t km = (size_t)std::max(k, 0);
            const int *row = hres.data() + (size_t)i * 5 * kmax;
            R.m_n = S.res_n < 0 ? -1 : k;
            R.m_model.assign(km ? hmod.data() + (size_t)i * kmax : nullptr, km ? hmod.data() + (size_t)i * kmax + km : nullptr);
            R.m_label.assign(row, row + km); R.m_time.assign(row + kmax, row + kmax + km);
            R.m_score.assign((const float *)(row + 2 * (size_t)kmax), (const float *)(row + 2 * (size_t)kmax) + km);
            R.m_ac.assign((const float *)(row + 3 * (size_t)kmax), (const float *)(row + 3 * (size_t)kmax) + km);
            R.m_lm.assign((const float *)(row + 4 * (size_t)kmax), (const float *)(row + 4 * (size_t)kmax) + km);
            if (km) { R.m_tot[0] = K.best_final.score; R.m_tot[1] = K.best_final.ac; R.m_tot[2] = K.best_final.lm; }
            else { R.m_tot[0] = LZ; R.m_tot[1] = LZ; R.m_tot[2] = LZ; }
            // ... and the word result word mode gives: its labelled entries, the first of them with the final-state weight
            int w = 0;
            for (size_t j = 0; j < km; ++j)
                if (R.m_label[j] != 0) {
                    int *rw = hres.data() + (size_t)i * 5 * kmax;
                    for (int a = 0; a < 5; ++a) rw[(size_t)a * kmax + w] = rw[(size_t)a * kmax + j];
                    ++w;
                }
            if (w > 0) {
                float *rf = (float *)(hres.data() + (size_t)i * 5 * kmax);
                rf[2 * (size_t)kmax] = K.best_final.score; rf[3 * (size_t)kmax] = K.best_final.ac; rf[4 * (size_t)kmax] = K.best_final.lm;
            }
            if (S.res_n >= 0) k = w;
        } else R.m_n = -1;
        H.n = S.res_n < 0 ? -1 : k;
        const size_t kk = (size_t)std::max(k, 0);
        R.label.resize(kk); R.time.resize(kk); R.score.resize(kk); R.ac.resize(kk); R.lm.resize(kk);
        if (kk) {
            const int *row = hres.data() + (size_t)i * 5 * kmax;
            memcpy(R.label.data(), row, kk * 4); memcpy(R.time.data(), row + kmax, kk * 4);
            memcpy(R.score.data(), row + 2 * (size_t)kmax, kk * 4); memcpy(R.ac.data(), row + 3 * (size_t)kmax, kk * 4);
            memcpy(R.lm.data(), row + 4 * (size_t)kmax, kk * 4);
        }
        H.label = R.label.data(); H.time = R.time.data();
        H.score = R.score.data(); H.ac = R.ac.data(); H.lm = R.lm.data();
        if (kk) { H.tot_score = K.best_final.score; H.tot_ac = K.best_final.ac; H.tot_lm = K.best_final.lm; }
        else { H.tot_score = LZ; H.tot_ac = LZ; H.tot_lm = LZ; }      // DecHyp() defaults, DecHypHistPool.h
    }
    return first_err;
}
static int fetch_results(jd_dec *d, int s0, int n, jd_hyp *out, int out0, const int *out_idx = nullptr)
{
    return fetch_results_from(d, nullptr, nullptr, nullptr, nullptr, s0, n, out, out0, out_idx);
}

#include "jd_host_launch.h"

// Lay a wave of nb <= max_streams utterances out in likelihood tables (jd_arena.h: wave_layout, from the free memory)
static int plan_wave(jd_dec *d, int nb, const int64_t *ustart, const int64_t *ulen, WavePlan &P)
{
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const WaveStatus st = wave_layout(WaveIn{nb, ustart, ulen, free_b, d->ll_cap, d->am->n_gmm, d->Fw_env, GMM_ROWS2}, &P);
    switch (st.code) {
    case WAVE_OK: return JD_OK;
    case WAVE_BAD_LENGTH: return jd_fail(JD_EINVAL, "utterance %d: bad frame count", st.utt);
    case WAVE_CHUNK_ROWS: return jd_fail(JD_EINVAL, "more than 2^31 frames in one chunk");
    case WAVE_BATCH_FRAMES: return jd_fail(JD_EINVAL, "more than 2^31 frames in one batch");
    }
    return jd_fail(JD_EINVAL, "plan_wave: internal error");
}

// The likelihood tables: THREE of one size in one allocation (a search launch addresses the table of every stream it
// advances as a row of that slab: SearchArgs::ll + slot * G), each with its row -> source frame table.  Three, because
// three batches can be under way at once ("two batches in flight" below): the one the caller is waiting for, the one
// behind it whose utterances are already being searched, and the one behind that whose table is being scored.
// Growing the slab loses what is in it: only when nothing scored ahead is waiting (the callers see to that).
static int ensure_slab(jd_dec *d, size_t floats)
{
    if (floats <= d->ll_cap) return JD_OK;
    if (d->d_cells) { (void)hipFree(d->d_cells); d->d_cells = nullptr; d->cells_words = 0; }   // (the diagnostics bitmap is as long as the slab)
    if (d->d_ll_slab) (void)hipFree(d->d_ll_slab);
    d->d_ll_slab = nullptr; d->ll_cap = 0;
    for (int i = 0; i < 3; ++i) d->d_ll[i] = nullptr;
    const size_t G = (size_t)d->am->n_gmm;
    floats = (floats + G - 1) / G * G;                                 // whole rows: a table starts at a row of the slab
    hipError_t e = hipMalloc(&d->d_ll_slab, 3 * floats * sizeof(float));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return jd_fail(e == hipErrorOutOfMemory ? JD_ENOMEM : JD_EHIP, "hipMalloc of %zu bytes (likelihood tables) failed: %s",
                       3 * floats * sizeof(float), hipGetErrorString(e));
    }
    d->ll_cap = floats;
    for (int i = 0; i < 3; ++i) d->d_ll[i] = d->d_ll_slab + (size_t)i * floats;
    return JD_OK;
}
static int ensure_rows(jd_dec *d, int i, size_t rows)
{
    if (rows > d->row_src_cap[i]) {
        if (d->d_row_src[i]) (void)hipFree(d->d_row_src[i]);
        d->d_row_src[i] = nullptr; d->row_src_cap[i] = 0;
        HIPCHK(hipMalloc(&d->d_row_src[i], rows * sizeof(int)));
        d->row_src_cap[i] = rows;
    }
    if (d->am->mlp_spliced && rows > d->row_span_cap[i]) {
        if (d->d_row_span[i]) (void)hipFree(d->d_row_span[i]);
        d->d_row_span[i] = nullptr; d->row_span_cap[i] = 0;
        HIPCHK(hipMalloc(&d->d_row_span[i], rows * sizeof(JdSpan)));
        d->row_span_cap[i] = rows;
    }
    return JD_OK;
}
// a spliced model's spans beside row table i (from entry `at`); null for every other model: what launch_gmm takes
static const JdSpan *row_span(const jd_dec *d, int i, size_t at = 0) { return d->am->mlp_spliced ? d->d_row_span[i] + at : nullptr; }
// ... of a wave's plan, sent behind its row table on stream st (splice_wave_spans; nothing to do for any other model)
static hipError_t send_wave_spans(jd_dec *d, int i, const WavePlan &P, const int64_t *ustart, hipStream_t st)
{
    if (!d->am->mlp_spliced) return hipSuccess;
    splice_wave_spans(P, ustart, &d->h_row_span[i]);
    return hipMemcpyAsync(d->d_row_span[i], d->h_row_span[i].data(), P.n_rows_all * sizeof(JdSpan), hipMemcpyHostToDevice, st);
}
// table i holds `floats`, its row table `rows` entries (grown, never shrunk)
static int ensure_table(jd_dec *d, int i, size_t floats, size_t rows)
{
    int rc = ensure_slab(d, floats);
    if (rc) return rc;
    return ensure_rows(d, i, rows);
}
static long long table_row0(const jd_dec *d, int buf) { return (long long)buf * (long long)(d->ll_cap / (size_t)d->am->n_gmm); }

// Forget what was scored, searched or announced ahead (the scoring stream is drained first: a table being written is
// not re-used; utterances whose search had been started are simply started again when their batch is decoded)
static void pipe_drain(jd_dec *d);
static void pf_discard(jd_dec *d)
{
    pipe_drain(d);
    if (ahead_any_scored(d->pf_q)) (void)hipStreamSynchronize(d->s_gmm);
    for (Prefetch &F : d->pf_q) F.drop();
    d->pf_q.clear();
}
// ... what has been scored ahead only: the announcements stay (they are scored again, beside the next search)
static void pf_discard_scored(jd_dec *d)
{
    if (ahead_any_scored(d->pf_q)) (void)hipStreamSynchronize(d->s_gmm);
    for (Prefetch &F : d->pf_q) { F.drop_events(); F.state = AHEAD_ANNOUNCED; F.bank = -1; }
}

// Start the scoring of the batches that have been announced and not scored yet, each into a table nobody holds.  Called
// by launch_search right behind the dispatch of a persistent search launch, once that launch is resident: the scoring
// kernel's blocks then only ever get the CUs that clusters of the search have left.
static int pf_launch(jd_dec *d)
{
    const size_t G = (size_t)d->am->n_gmm;
    for (Prefetch &F : d->pf_q) {
        if (F.state != AHEAD_ANNOUNCED) continue;
        // Scoring ahead is an optimisation: a batch that cannot be scored now (no table free, a table larger than the
        // slab - which cannot grow while tables are in use) is scored when it is decoded, as ever.
        const int buf = ahead_free_table(d->pf_q, d->fg_buf);
        if (buf < 0 || F.plan.max_rows * G > d->ll_cap) break;
        if (ensure_rows(d, buf, F.plan.n_rows_all) != JD_OK) { (void)hipGetLastError(); break; }
        if (hipEventCreate(&F.ev0) != hipSuccess || hipEventCreate(&F.ev1) != hipSuccess) { (void)hipGetLastError(); F.drop_events(); break; }
        if (hipMemcpyAsync(d->d_row_src[buf], F.plan.row_src.data(), F.plan.n_rows_all * sizeof(int), hipMemcpyHostToDevice, d->s_gmm) != hipSuccess ||
            send_wave_spans(d, buf, F.plan, F.ustart.data(), d->s_gmm) != hipSuccess ||
            hipEventRecord(F.ev0, d->s_gmm) != hipSuccess ||
            launch_gmm(d->am, d->amb, F.feats, d->d_row_src[buf], F.plan.chunk_rows[0], d->d_ll[buf], d->s_gmm, 0, true, -1, nullptr, 0, nullptr,
                       row_span(d, buf)) != JD_OK ||
            hipEventRecord(F.ev1, d->s_gmm) != hipSuccess) {
            (void)hipGetLastError(); F.drop_events(); break;
        }
        F.buf = buf; F.state = AHEAD_SCORED;
    }
    HIPCHK(hipMemsetAsync(d->d_status + 4, 0, sizeof(int), d->s_gmm)); // (behind the scoring, if any: the search may be re-planned again)
    return JD_OK;
}
static bool pf_wants_scoring(const jd_dec *d) { return ahead_wants_scoring(d->pf_q, d->fg_buf, (size_t)d->am->n_gmm, d->ll_cap); }
static bool pf_scoring_in_flight(const jd_dec *d)
{
    for (const Prefetch &F : d->pf_q)
        if (F.state == AHEAD_SCORED && F.ev1 && hipEventQuery(F.ev1) != hipSuccess) { (void)hipGetLastError(); return true; }
    return false;
}

// Announce a wave (jd_ahead.h: ahead_admits, ahead_enqueue): it is scored beside the next search launch that leaves a table free.
// front: in front of what the caller announced (the waves of one call).
static int pf_announce(jd_dec *d, int nb, const float *d_feats, const int64_t *ustart, const int64_t *ulen, bool front = false)
{
    if (!ahead_admits(nb, d->max_streams, d->pf_q.size())) return JD_OK;
    Prefetch F;
    F.ustart.assign(ustart, ustart + nb);
    F.ulen.assign(ulen, ulen + nb);
    const int rc = plan_wave(d, nb, F.ustart.data(), F.ulen.data(), F.plan);
    if (rc) return rc;
    (void)ahead_enqueue(d->pf_q, std::move(F), d_feats, nb, front);
    return JD_OK;
}

// ---- two batches in flight.  A batch of 64 utterances lasts as long as its longest one - a chain of ~1150 dependent
// frames - while the clusters of the shorter ones are through after half of that: whatever the plan, workgroup-time is
// burnt waiting.  What a stream of batches allows: the utterances of the batch BEHIND the one the caller
// is waiting for are started beside it, one workgroup each (no cluster barrier at all), on stream slots of their own
// (the decoder's streams are two banks of max_streams / 2) - when that batch's turn comes its utterances are hundreds
// of frames in, and the step is that much shorter.  It takes a table scored one batch earlier, i.e. announcements
// that run two batches ahead of the decode (jd_dec_prefetch_scores twice before the first decode, once per decode
// afterwards).  Nothing changes for a caller who does not announce, announces one ahead, or fills more than half of
// the streams with one batch; results cannot depend on any of it (streams never interact).
// The batch behind the running one, if its table is there: its unfinished streams as work items for the launch that is
// being planned (started - initialised, frame counts set - the first time round).  heads: those of every stream (read_heads),
// as of now (only read for a batch that has been started before).
static int pf_background(jd_dec *d, int fg_bank, const std::vector<StreamHead> *heads, hipStream_t st, std::vector<int2> *work, std::vector<double> *left)
{
    work->clear(); left->clear();
    const AheadBg step = ahead_bg_step(d->pf_q, d->pipeline != 0, d->C.lazy != nullptr, d->load_scale, d->bg_max_load, d->max_streams);
    if (step == AHEAD_BG_NONE || (step == AHEAD_BG_GO_ON && !heads)) return JD_OK;
    Prefetch &F = d->pf_q.front();
    const int B = d->max_streams / 2;
    if (step == AHEAD_BG_START) {
        // its table was scored beside the search before this one and is about ready: worth a moment (JD_BG_WAIT_US)
        const auto tq0 = std::chrono::steady_clock::now();
        while (hipEventQuery(F.ev1) != hipSuccess) {
            (void)hipGetLastError();
            const double waited_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tq0).count();
            if (waited_us > d->bg_wait_us) return JD_OK;              // still being scored
        }
        F.bank = fg_bank ^ 1;
        const int s0 = F.bank * B;
        int rc = mark_init(d, s0, F.nb, st);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(d->d_T + s0, F.plan.T.data(), (size_t)F.nb * sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(jd_set_T_kernel, dim3((F.nb + 63) / 64), dim3(64), 0, st, d->d_ctl, s0, F.nb, d->d_T + s0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));                              // (plan.T may move with the queue)
        heads = nullptr;                                               // (just started: every utterance, all its frames)
    }
    ahead_bg_work(F, F.bank * B, table_row0(d, F.buf), heads, work, left);
    return JD_OK;
}

// ---- decode_wave, step by step.  One wave on its way through the steps: what was decided (jd_ahead.h) and what the next steps need.
struct Wave {
    int nb; const float *feats; const int64_t *ustart, *ulen;
    Prefetch me;                               // the announced batch this wave turned out to be (claim.mine); dropped on every way out
    WavePlan plan_local;
    AheadClaim claim{}; AheadPlace place{}; AheadNeed need{}; AheadTake take{};
    int b0 = 0;                                // its table (in chunks: b0 and b0 ^ 1, alternately)
    std::vector<int> frame0;                   // where its streams stand (a batch started ahead: hundreds of frames in)
    struct Events {                            // a chunk's scoring, begin and end (destroyed on every way out, error paths included)
        std::vector<hipEvent_t> v;
        ~Events() { for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e); }
    } gs, ge;
    const WavePlan &P() const { return claim.mine ? me.plan : plan_local; }
    ~Wave() { me.drop(); }
};

// claim: is this wave the one at the head of the batches ahead (jd_dec_prefetch_scores)?  An announcement speaks of a batch
// BEHIND the decode that follows it (a stream of equal batches announces the very batch it is about to decode).
static void wave_claim(jd_dec *d, Wave &W)
{
    W.claim = ahead_claim(d->pf_q, W.feats, W.nb, W.ustart, W.ulen, d->pf_retry);
    if (W.claim.mine) { W.me = std::move(d->pf_q.front()); d->pf_q.pop_front(); }
    if (W.claim.drop) pf_discard(d);
}
// place: its bank of streams, and what becomes of a batch ahead that is in its way
static void wave_place(jd_dec *d, Wave &W)
{
    W.place = ahead_place(d->pf_q, W.P().n_chunks, W.nb, d->max_streams, d->pipeline != 0, d->C.lazy != nullptr, W.claim.mine, W.me.bank);
    if (W.place.discard) pf_discard(d);
    if (W.place.unbank) for (Prefetch &Q : d->pf_q) Q.bank = -1;
}
// tables: a single-chunk wave sits in one of the three - the one it was scored into ahead, or a free one; chunks alternate between 0 and 1
static int wave_tables(jd_dec *d, Wave &W)
{
    const WavePlan &P = W.P();
    const bool chunked = P.n_chunks > 1;
    if (W.claim.mine && !chunked) { W.b0 = W.me.buf; return JD_OK; }
    W.need = ahead_table_need(d->pf_q, P.max_rows, (size_t)d->am->n_gmm, d->ll_cap, chunked);
    if (W.need.drop_scored) pf_discard_scored(d);
    const int rc = ensure_slab(d, W.need.floats);
    if (rc) return rc;
    W.take = ahead_table_take(d->pf_q, chunked);
    if (W.take.discard) pf_discard(d);
    W.b0 = W.take.table;
    return ensure_rows(d, W.b0, P.n_rows_all);
}
// start its streams, or - its utterances have been started beside the batch before - see where they stand
static int wave_start_or_resume(jd_dec *d, Wave &W)
{
    const int nb = W.nb, s0 = W.place.s0;
    W.frame0.assign((size_t)nb, 0);
    if (!W.place.resumed) {
        HIPCHK(hipMemcpyAsync(d->d_T + s0, W.P().T.data(), (size_t)nb * sizeof(int), hipMemcpyHostToDevice, d->s_search));
        const int rc = mark_init(d, s0, nb, d->s_search);
        if (rc) return rc;
        hipLaunchKernelGGL(jd_set_T_kernel, dim3((nb + 63) / 64), dim3(64), 0, d->s_search, d->d_ctl, s0, nb, d->d_T + s0);
        HIPCHK(hipGetLastError());
        return JD_OK;
    }
    std::vector<StreamHead> head;
    const int rc = read_heads(d, s0, nb, &head, nullptr);
    if (rc) return rc;
    for (int u = 0; u < nb; ++u) { W.frame0[(size_t)u] = head[(size_t)u].frame; d->timing.ahead_frames += head[(size_t)u].frame; }
    return JD_OK;
}
// Scoring runs one chunk ahead of the search on its own stream.  launch_search returns when its
// chunk is through (it synchronises to learn whether a stream stopped for garbage collection),
// so by the time chunk c+1 is scored into buffer (c+1)&1 the search of chunk c-1 has left it.
static int wave_score_chunk(jd_dec *d, Wave &W, int c)
{
    const WavePlan &P = W.P();
    HIPCHK(hipEventRecord(W.gs.v[(size_t)c], d->s_gmm));
    // (a later chunk is launched while the previous one is searched: k_search holds every CU's
    // registers, so its workgroups start as the search's clusters finish - they fill the tail)
    if (P.chunk_rows[(size_t)c] == 0) { HIPCHK(hipEventRecord(W.ge.v[(size_t)c], d->s_gmm)); return JD_OK; }
    const int r = launch_gmm(d->am, d->amb, W.feats, d->d_row_src[W.b0] + P.chunk_row0[(size_t)c], P.chunk_rows[(size_t)c], d->d_ll[W.b0 ^ (c & 1)],
                             d->s_gmm, 0, true, -1, nullptr, 0, nullptr, row_span(d, W.b0, P.chunk_row0[(size_t)c]));
    if (r) return r;
    HIPCHK(hipEventRecord(W.ge.v[(size_t)c], d->s_gmm));
    return JD_OK;
}
// search chunk c, once its scores are there (and the next chunk's scoring is under way)
static int wave_search_chunk(jd_dec *d, Wave &W, int c, double *waited_ms, long long *frames_here)
{
    const WavePlan &P = W.P();
    const int G = d->am->n_gmm, s0 = W.place.s0, c0 = c * P.Fc, c1 = (c + 1) * P.Fc;
    auto failed = [&](int rc) { for (int u = 0; u < W.nb; ++u) d->stream_dirty[(size_t)(s0 + u)] = 1; return rc; };   // (nobody looks at the streams' error words)
    const auto tw0 = std::chrono::steady_clock::now();
    HIPCHK(hipEventSynchronize(W.ge.v[(size_t)c]));
    *waited_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
    int rc = JD_OK;
    if (c + 1 < P.n_chunks) { rc = wave_score_chunk(d, W, c + 1); if (rc) return rc; }
    std::vector<int2> work;
    std::vector<double> weight;
    // (k_search reads row  slot + (f - c0)  of the slab)
    *frames_here += ahead_chunk_work(P, c, s0, table_row0(d, W.b0 ^ (c & 1)), W.frame0, &work, &weight);
    const float *ll = d->d_ll_slab;
    if (ahead_probe_applies(d->load_scale, d->weighted != 0, c, P, W.place.resumed)) {
        const std::vector<double> wp = ahead_probe_weights(weight);
        rc = launch_search(d, work, ll, (long long)G, c0, c0 + AHEAD_PROBE_FRAMES, d->s_search, &wp);
        if (rc) return failed(rc);
        if (d->load_scale == 1.0) { rc = learn_load(d, work); if (rc) return rc; }
        ahead_probe_rest(P, c, s0, &work, &weight);
    }
    d->pf_armed = P.n_chunks == 1;                                     // batches ahead are scored / started beside this launch
    d->fg_bank = W.place.pipe ? W.place.bank : -1;
    rc = launch_search(d, work, ll, (long long)G, c0, c1, d->s_search, &weight);
    d->pf_armed = false; d->fg_bank = -1;
    return rc ? failed(rc) : JD_OK;
}
// what scoring (on its own) and search cost on this decoder (launch_search's choice when a table is scored ahead), and the counters
static void wave_timing(jd_dec *d, const Wave &W, double wall_ms, double waited_ms, long long frames_here, double gmm_before, double search_before)
{
    const WavePlan &P = W.P();
    d->timing.total_ms += wall_ms;
    d->last_wave_ms = wall_ms;
    long long rows = 0;
    for (int c = 0; c < P.n_chunks; ++c) {
        float gms = 0.0f;
        if (hipEventElapsedTime(&gms, W.gs.v[(size_t)c], W.ge.v[(size_t)c]) == hipSuccess) d->timing.gmm_ms += gms;
        rows += P.chunk_rows[(size_t)c];
    }
    d->timing.gmm_wait_ms += waited_ms;
    d->timing.gmm_launches += P.n_chunks;
    d->timing.prefetched += W.claim.mine ? 1 : 0;
    if (!W.claim.mine && rows > 0 && d->timing.gmm_ms > gmm_before) d->gmm_ms_per_row = (d->timing.gmm_ms - gmm_before) / (double)rows;
    // (a launch that also advanced the batch behind: its frames are not known here - the estimate stays)
    if (frames_here > 0 && d->timing.search_ms > search_before && !d->bg_ran)
        d->search_ms_per_frame = (d->timing.search_ms - search_before) / (double)frames_here;
    d->bg_ran = false;
    for (int u = 0; u < W.nb; ++u) d->timing.search_frames += P.T[(size_t)u];
    d->timing.gmm_frames = d->timing.search_frames;
    d->timing.gmm_states = d->am->n_gmm;
}

// Decode one wave of nb <= max_streams utterances held in device memory.
// Stream u decodes frames [ustart[u], ustart[u] + ulen[u]) of d_feats.  *s0_out: the first stream it ran on.
static int decode_wave(jd_dec *d, int nb, const float *d_feats, const int64_t *ustart, const int64_t *ulen,
                       hipStream_t user_stream, int *s0_out)
{
    const double gmm_before = d->timing.gmm_ms, search_before = d->timing.search_ms;
    const bool verbose = getenv("JD_VERBOSE") != nullptr;
    const std::string q_before = verbose ? ahead_describe(d->pf_q, d_feats, nb, ustart, ulen) : std::string();
    const size_t cap_before = d->ll_cap;
    Wave W{nb, d_feats, ustart, ulen};
    wave_claim(d, W);
    int rc = JD_OK;
    if (!W.claim.mine) { rc = plan_wave(d, nb, ustart, ulen, W.plan_local); if (rc) return rc; }
    const WavePlan &P = W.P();
    const int n_chunks = P.n_chunks;
    wave_place(d, W);
    if (s0_out) *s0_out = W.place.s0;
    rc = wave_tables(d, W);
    if (verbose)                                                       // (tests/test_gpu_ahead_inputs.py reads it)
        fprintf(stderr, "ahead: q %s retry %d nb %d n_chunks %d max_rows %zu streams %d pipeline %d lazy %d G %d ll_cap %zu -> mine %d drop %d pipe %d "
                "resumed %d discard %d unbank %d bank %d s0 %d need %zu drop_scored %d table %d none_free %d\n", q_before.c_str(), d->pf_retry ? 1 : 0,
                nb, n_chunks, P.max_rows, d->max_streams, d->pipeline != 0, d->C.lazy != nullptr, d->am->n_gmm, cap_before, W.claim.mine, W.claim.drop,
                W.place.pipe, W.place.resumed, W.place.discard, W.place.unbank, W.place.bank, W.place.s0, W.need.floats, W.need.drop_scored, W.b0,
                W.take.discard);
    if (rc) return rc;
    d->fg_buf = n_chunks == 1 ? W.b0 : FG_BOTH;
    struct FgGuard { jd_dec *d; ~FgGuard() { d->fg_buf = FG_NONE; } } fg_guard{d};
    // the caller's features may have been produced asynchronously on its stream (NULL = the
    // default stream): the decoder's own streams are non-blocking, so order against it explicitly
    HIPCHK(hipStreamSynchronize(user_stream));
    if (!W.claim.mine) {
        HIPCHK(hipMemcpyAsync(d->d_row_src[W.b0], P.row_src.data(), P.n_rows_all * sizeof(int), hipMemcpyHostToDevice, d->s_gmm));
        HIPCHK(send_wave_spans(d, W.b0, P, ustart, d->s_gmm));
    }
    rc = wave_start_or_resume(d, W);
    if (rc) return rc;
    W.gs.v.assign((size_t)n_chunks, nullptr); W.ge.v.assign((size_t)n_chunks, nullptr);
    if (W.claim.mine) {                                                // the scoring's own events (Events destroys them)
        W.gs.v[0] = W.me.ev0; W.ge.v[0] = W.me.ev1;
        W.me.ev0 = W.me.ev1 = nullptr;
    } else
        for (int c = 0; c < n_chunks; ++c) { HIPCHK(hipEventCreate(&W.gs.v[(size_t)c])); HIPCHK(hipEventCreate(&W.ge.v[(size_t)c])); }
    const auto w0 = std::chrono::steady_clock::now();
    if (!W.claim.mine) { rc = wave_score_chunk(d, W, 0); if (rc) return rc; }
    double waited_ms = 0.0;
    long long frames_here = 0;
    for (int c = 0; c < n_chunks; ++c) { rc = wave_search_chunk(d, W, c, &waited_ms, &frames_here); if (rc) return rc; }
    hipLaunchKernelGGL(jd_finish_kernel, dim3((nb + 63) / 64), dim3(64), 0, d->s_search, d->d_ctl, d->d_streams, W.place.s0, nb, res_model_of(d));
    HIPCHK(hipGetLastError());
    if (!ahead_any_scored(d->pf_q)) HIPCHK(hipStreamSynchronize(d->s_gmm));   // (a table being scored ahead is waited for by the wave that uses it)
    HIPCHK(hipStreamSynchronize(d->s_search));
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    wave_timing(d, W, wall_ms, waited_ms, frames_here, gmm_before, search_before);
    return JD_OK;
}

extern "C" int jd_decode_batch_device(jd_dec *d, int32_t n_utts, const float *d_feats, const int64_t *offs,
                                      void *hip_stream, jd_hyp *out)
{
    if (!d || !offs || !out || n_utts < 0) return jd_fail(JD_EINVAL, "jd_decode_batch_device: bad argument");
    int rc = check_device(d->device);
    if (rc) return rc;
    {   // the oldest batch of the pipeline (JD_PIPELINE=3)?
        int handled = 0;
        rc = pipe_decode(d, n_utts, d_feats, offs, out, &handled);
        if (rc || handled) return rc;
        // ... or more utterances than streams, nothing announced: through the pipeline's slots as well - a stream takes the next
        // utterance the moment its own is through, where the waves below end with their longest one
        if (d->pipe_mode && n_utts > (d->pipe_slots > 0 ? d->pipe_slots : d->max_streams) && !d->pipe_on) {
            HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));     // the features are there
            int taken = 0;
            rc = pipe_announce(d, n_utts, d_feats, offs, &taken);
            if (rc) return rc;
            if (taken) {
                rc = pipe_decode(d, n_utts, d_feats, offs, out, &handled);
                if (rc || handled) return rc;
            }
        }
    }
    rc = ensure_arenas(d);
    if (rc) return rc;
    if ((size_t)n_utts > d->results.size()) d->results.resize((size_t)n_utts);
    d->timing = jd_timing();
    int first_err = JD_OK;
    // More utterances than streams: successive waves, formed from the utterances sorted by length (jd_ahead.h)
    const std::vector<int> order = ahead_wave_order(offs, n_utts, d->max_streams);
    std::vector<int64_t> ustart((size_t)d->max_streams), ulen((size_t)d->max_streams);
    std::vector<int64_t> nstart((size_t)d->max_streams), nlen((size_t)d->max_streams);
    // the batch takes every stream over: utterances of the streaming interface that were never finished leave the
    // (lazily composed) network now - before the first jd_lazy_enter, which starts a new arena generation only when
    // nobody is inside, or a full network would fail this call and, the release below never reached, every later one
    for (int s = 0; s < d->max_streams; ++s) {
        d->push[(size_t)s].taken_over();
        if (d->lazy_in[(size_t)s]) { d->lazy_in[(size_t)s] = 0; jd_lazy_leave(d->net, 1); }
    }
    // Scoring ahead inside the batch: every wave but the last announces the wave behind it, whose table is then scored
    // beside this wave's search (pf_launch); what the caller announced (the batches behind this one) rides on the last wave.
    const bool waves = n_utts > d->max_streams;
    std::deque<Prefetch> callers;
    if (waves) {
        // (a batch of several waves is never itself one of the announced ones: what has been worked ahead goes)
        if (ahead_any_worked(d->pf_q)) pf_discard(d);
        callers.swap(d->pf_q);
    }
    // (on an error way out nothing scored or announced ahead survives: the caller may free the features next)
    struct Restore {
        jd_dec *d; std::deque<Prefetch> &p; bool ok;
        ~Restore() { for (Prefetch &F : p) F.drop(); if (!ok) pf_discard(d); }
    } callers_guard{d, callers, false};
    for (int u0 = 0; u0 < n_utts; u0 += d->max_streams) {
        const int nb = ahead_wave_slice(offs, order, u0, d->max_streams, ustart.data(), ulen.data());
        const int nn = waves ? ahead_wave_slice(offs, order, u0 + nb, d->max_streams, nstart.data(), nlen.data()) : 0;
        if (nn > 0) {
            rc = pf_announce(d, nn, d_feats, nstart.data(), nlen.data());
            if (rc) return rc;
        } else if (waves) {
            for (Prefetch &F : callers) d->pf_q.push_back(std::move(F));
            callers.clear();
        }
        struct RetryGuard { jd_dec *d; ~RetryGuard() { d->pf_retry = false; } } retry_guard{d};
        for (int attempt = 0;; ++attempt) {
            // (lazily composed networks: the wave's utterances enter the network - which starts a new arena generation
            // when nobody is inside an utterance and it is nearly full, or has run out of room)
            bool net_failed = false;
            rc = jd_lazy_enter(d->net, nb, &net_failed);
            if (rc) return rc;
            if (net_failed) {
                jd_lazy_leave(d->net, nb);
                return jd_fail(JD_ENOMEM, "the lazily composed network has run out of room and utterances of other decoders are inside it: "
                               "it starts again when they are through (capacity %d states, %lld arcs)", d->net->n_states, (long long)d->net->n_arcs);
            }
            d->lazy_failed = false;
            const jd_timing t_before = d->timing;                      // (a wave that is decoded twice counts once)
            const double ls_before = d->load_sum, lf_before = d->load_frames;
            int s0 = 0;
            rc = decode_wave(d, nb, d_feats, ustart.data(), ulen.data(), (hipStream_t)hip_stream, &s0);
            const int rf = rc ? rc : fetch_results(d, s0, nb, out, 0, order.data() + u0);
            jd_lazy_leave(d->net, nb);
            if (rc) return rc;
            // out of graph room under way: once more - jd_lazy_enter gives the wave a fresh generation to itself
            if (d->lazy_failed && attempt == 0) {
                d->timing = t_before; d->load_sum = ls_before; d->load_frames = lf_before;
                // (what was scored ahead beside attempt 0 belongs to the waves BEHIND this one: the retry, which matches no
                // announced table, must not drop it)
                d->pf_retry = true;
                continue;
            }
            d->pf_retry = false;
            if (rf && first_err == JD_OK) first_err = rf;
            break;
        }
    }
    d->load_scale = ahead_load_update(d->load_scale, d->load_sum, d->load_frames);   // the load this batch had -> the next batch's cluster sizes
    if (d->load_frames > 0.0) d->load_sum = d->load_frames = 0.0;
    callers_guard.ok = true;
    return first_err;
}

extern "C" int jd_dec_prefetch_scores(jd_dec *d, int32_t n_utts, const float *d_feats, const int64_t *offs, void *hip_stream)
{
    if (!d || n_utts < 0 || (n_utts > 0 && (!d_feats || !offs))) return jd_fail(JD_EINVAL, "jd_dec_prefetch_scores: bad argument");
    int rc = check_device(d->device);
    if (rc) return rc;
    if (n_utts == 0) { pf_discard(d); return JD_OK; }                  // nothing: what was scored or announced ahead is dropped
    // what cannot be scored ahead is scored when it is decoded, as ever: more utterances than streams (several waves,
    // formed by length: jd_decode_batch_device scores each of them beside the wave before it), a table cut into chunks
    if (d->pipe_mode) {   // JD_PIPELINE=3: the batch goes through the resident kernel, utterance by utterance (any number of them)
        HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));         // the features are there
        int taken = 0;
        rc = pipe_announce(d, n_utts, d_feats, offs, &taken);
        if (rc || taken) return rc;
    }
    if (n_utts > d->max_streams) return JD_OK;
    HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));             // the features are there
    std::vector<int64_t> ulen((size_t)n_utts);
    for (int u = 0; u < n_utts; ++u) ulen[(size_t)u] = offs[u + 1] - offs[u];
    return pf_announce(d, n_utts, d_feats, offs, ulen.data());
}

extern "C" int jd_decode_batch(jd_dec *d, int32_t n_utts, const float *const *feats, const int32_t *n_frames,
                               jd_hyp *out)
{
    if (!d || !feats || !n_frames || !out || n_utts < 0) return jd_fail(JD_EINVAL, "jd_decode_batch: bad argument");
    int rc = check_device(d->device);
    if (rc) return rc;
    const int D = d->am->D;
    std::vector<int64_t> offs((size_t)n_utts + 1, 0);
    for (int u = 0; u < n_utts; ++u) {
        if (n_frames[u] < 0) return jd_fail(JD_EINVAL, "jd_decode_batch: negative frame count");
        offs[(size_t)u + 1] = offs[(size_t)u] + n_frames[u];
    }
    float *d_feats = nullptr;
    HIPCHK(hipMalloc(&d_feats, std::max<size_t>((size_t)offs[(size_t)n_utts] * D, 1) * sizeof(float)));
    for (int u = 0; u < n_utts; ++u)
        if (n_frames[u] > 0)
            HIPCHK(hipMemcpy(d_feats + (size_t)offs[(size_t)u] * D, feats[u], (size_t)n_frames[u] * D * sizeof(float),
                             hipMemcpyHostToDevice));
    rc = jd_decode_batch_device(d, n_utts, d_feats, offs.data(), nullptr, out);
    (void)hipFree(d_feats);
    return rc;
}

// ---- streaming API: IDecoder::init / processFrame / finish for one stream

#include "jd_host_stream.h"
#include "jd_host_paths.h"         // jd_debug_paths: the collection and the partial trace on a described state

// Diagnostics: per-workgroup cycle accounting of k_search (100 MHz wall clock): for every
// workgroup of the grid {work lists A, phase A, workgroup wait, cluster barrier, work lists X, phase X,
// workgroup wait, cluster barriers, frames} (thread 0's timeline), summed over the launches since it
// was enabled.  enable >= 0 switches it on (and clears it), < 0 off;
// fetch (1024 x 16 int64, may be NULL) receives the current sums.
extern "C" int jd_dec_debug_trace(jd_dec *d, int32_t enable, int64_t *fetch)
{
    if (!d) return jd_fail(JD_EINVAL, "jd_dec_debug_trace: null");
    const size_t n = (size_t)1024 * 16;
    static_assert(sizeof(long long) == sizeof(int64_t), "");
    if (fetch && d->d_dbg) {
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(fetch, d->d_dbg, n * sizeof(long long), hipMemcpyDeviceToHost));
    } else if (fetch) memset(fetch, 0, n * sizeof(int64_t));
    if (enable >= 0 && !fetch) {
        if (!d->d_dbg_buf) {                                           // (one buffer per decoder, kept when tracing is switched off)
            long long *p = nullptr;
            HIPCHK(hipMalloc(&p, n * sizeof(long long)));
            d->allocs.push_back(p);
            d->d_dbg_buf = p;
        }
        d->d_dbg = d->d_dbg_buf;
        HIPCHK(hipMemset(d->d_dbg, 0, n * sizeof(long long)));
    } else if (enable < 0) d->d_dbg = nullptr;
    return JD_OK;
}

// Test hook for the bit-exactness claim of jd_expf: evaluates it for x[0..n) on HIP device
// `device`, or - device == -1 - its host twin compiled from the same source.
__global__ void jd_debug_expf_kernel(const float *x, long long n, float *out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = jd_expf(x[i]);
}
extern "C" int jd_debug_expf(int32_t device, const float *x, int64_t n, float *out)
{
    if (!x || !out || n < 0) return jd_fail(JD_EINVAL, "jd_debug_expf: bad argument");
    if (device == -1) {
        for (int64_t i = 0; i < n; ++i) out[i] = jd_expf_impl(x[i], jd_exp2f_tab_host);
        return JD_OK;
    }
    int rc = check_device(device);
    if (rc) return rc;
    float *dx = nullptr, *dy = nullptr;
    HIPCHK(hipMalloc(&dx, std::max<size_t>((size_t)n, 1) * sizeof(float)));
    HIPCHK(hipMalloc(&dy, std::max<size_t>((size_t)n, 1) * sizeof(float)));
    HIPCHK(hipMemcpy(dx, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    if (n) hipLaunchKernelGGL(jd_debug_expf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, (long long)n, dy);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dy, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    (void)hipFree(dx); (void)hipFree(dy);
    return JD_OK;
}

// Test hooks for logAdd (HTKFlatModels.cpp:266-293), jd_debug_expf's companions; device == -1 runs the host twins compiled
// from the same source.  jd_debug_log1pe: out[i] = log(1.0 + (double)expf(d[i])) in double, d[i] in [-19, 0] - variant 0
// jd_log_libm_impl (the libm's value), 1 jd_log1pe_table (the table value the gate rounds).  jd_debug_log_add: out[i] =
// logAdd(x[i], y[i]) - variant 0 jd_log_add (the generic kernel's), 1 jd_log_add2x2 (jd_gmm_kernel39's: elements 2j and 2j + 1
// are one call's pair), 2 jd_log_add_fast (jd_gmm_fast39's; device only).
__global__ void jd_debug_log1pe_kernel(const float *d, long long n, int variant, const JdLogTab *tab, double *out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double e = (double)jd_expf(d[i]);
    out[i] = variant ? jd_log1pe_table(e, tab) : jd_log_libm_impl(1.0 + e, jd_log_tab);
}
__global__ void jd_debug_log_add_kernel(const float *x, const float *y, long long n, int variant, const JdLogTab *tab, float *out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (variant == 1) {
        const long long j = 2 * i;
        if (j >= n) return;
        float a0 = x[j], a1 = (j + 1 < n) ? x[j + 1] : a0;
        const float c0 = y[j], c1 = (j + 1 < n) ? y[j + 1] : c0;
        jd_log_add2x2(a0, a1, c0, c1, tab, jd_exp2f_tab);                 // NaN: jd_gmm_kernel39 scores the cell again
        out[j] = (a0 != a0) ? jd_log_add(x[j], c0, tab) : a0;
        if (j + 1 < n) out[j + 1] = (a1 != a1) ? jd_log_add(x[j + 1], c1, tab) : a1;
        return;
    }
    if (i < n) out[i] = variant ? jd_log_add_fast(x[i], y[i]) : jd_log_add(x[i], y[i], tab);
}
static int debug_upload_logtab(JdLogTab **d_tab)
{
    JdLogTab t[129];
    jd_fill_logtab(t);
    HIPCHK(hipMalloc(d_tab, sizeof t));
    HIPCHK(hipMemcpy(*d_tab, t, sizeof t, hipMemcpyHostToDevice));
    return JD_OK;
}
extern "C" int jd_debug_log1pe(int32_t device, int32_t variant, const float *d, int64_t n, double *out)
{
    if (!d || !out || n < 0 || (variant != 0 && variant != 1)) return jd_fail(JD_EINVAL, "jd_debug_log1pe: bad argument");
    for (int64_t i = 0; i < n; ++i)
        if (!(d[i] >= -19.0f && d[i] <= 0.0f)) return jd_fail(JD_EINVAL, "jd_debug_log1pe: d[%lld] outside [-19, 0]", (long long)i);
    if (device == -1) {
        JdLogTab t[129];
        jd_fill_logtab(t);
        for (int64_t i = 0; i < n; ++i) {
            const double e = (double)jd_expf_impl(d[i], jd_exp2f_tab_host);
            out[i] = variant ? jd_log1pe_table(e, t) : jd_log_libm_impl(1.0 + e, jd_log_tab_host);
        }
        return JD_OK;
    }
    int rc = check_device(device);
    if (rc) return rc;
    float *dd = nullptr;
    double *dy = nullptr;
    JdLogTab *dt = nullptr;
    rc = debug_upload_logtab(&dt);
    if (rc) return rc;
    HIPCHK(hipMalloc(&dd, std::max<size_t>((size_t)n, 1) * sizeof(float)));
    HIPCHK(hipMalloc(&dy, std::max<size_t>((size_t)n, 1) * sizeof(double)));
    HIPCHK(hipMemcpy(dd, d, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    if (n) hipLaunchKernelGGL(jd_debug_log1pe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dd, (long long)n, (int)variant, dt, dy);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dy, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipFree(dd); (void)hipFree(dy); (void)hipFree(dt);
    return JD_OK;
}
extern "C" int jd_debug_log_add(int32_t device, int32_t variant, const float *x, const float *y, int64_t n, float *out)
{
    if (!x || !y || !out || n < 0 || variant < 0 || variant > 2) return jd_fail(JD_EINVAL, "jd_debug_log_add: bad argument");
    if (device == -1) {
        if (variant == 2) return jd_fail(JD_EINVAL, "jd_debug_log_add: jd_log_add_fast has no host twin (device only)");
        JdLogTab t[129];
        jd_fill_logtab(t);
        if (variant == 0)
            for (int64_t i = 0; i < n; ++i) out[i] = jd_log_add_impl(x[i], y[i], t, jd_exp2f_tab_host, jd_log_tab_host);
        else
            for (int64_t j = 0; j < n; j += 2) {
                float a0 = x[j], a1 = (j + 1 < n) ? x[j + 1] : a0;
                const float c0 = y[j], c1 = (j + 1 < n) ? y[j + 1] : c0;
                jd_log_add2x2(a0, a1, c0, c1, t, jd_exp2f_tab_host);
                out[j] = (a0 != a0) ? jd_log_add_impl(x[j], c0, t, jd_exp2f_tab_host, jd_log_tab_host) : a0;
                if (j + 1 < n) out[j + 1] = (a1 != a1) ? jd_log_add_impl(x[j + 1], c1, t, jd_exp2f_tab_host, jd_log_tab_host) : a1;
            }
        return JD_OK;
    }
    int rc = check_device(device);
    if (rc) return rc;
    float *dx = nullptr, *dy = nullptr, *dz = nullptr;
    JdLogTab *dt = nullptr;
    rc = debug_upload_logtab(&dt);
    if (rc) return rc;
    const size_t bytes = std::max<size_t>((size_t)n, 1) * sizeof(float);
    HIPCHK(hipMalloc(&dx, bytes));
    HIPCHK(hipMalloc(&dy, bytes));
    HIPCHK(hipMalloc(&dz, bytes));
    HIPCHK(hipMemcpy(dx, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dy, y, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    if (n) hipLaunchKernelGGL(jd_debug_log_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, dy, (long long)n, (int)variant, dt, dz);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dz, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(dz); (void)hipFree(dt);
    return JD_OK;
}

// Test hooks for the histogram pruning of the search kernels (Histogram.cpp:64-100 / 134-158).  jd_debug_hist_bin: out[i] =
// jd_hist_bin(s[i], hist_min, hist_max) - the bin, JD_HIST_BELOW (-1) or JD_EHIST; device == -1 runs the host twin.
// jd_debug_hist_threshold: out[c] = hist_threshold over bins[c * nb .. c * nb + nb) with max_hyps[c], one wave per case,
// the very function k_search and the slot kernels call (device only: it is a wave-parallel search).
__global__ void jd_debug_hist_bin_kernel(const float *s, long long n, int hist_min, int hist_max, int *out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = jd_hist_bin(s[i], hist_min, hist_max);
}
__global__ void __launch_bounds__(64) jd_debug_hist_threshold_kernel(const int *bins, int nb, const int *max_hyps, int hist_min, float *out)
{
    __shared__ int sh_hist[HIST_MAX_BINS];
    const int lane = threadIdx.x;
    const size_t c = blockIdx.x;
    for (int b = lane; b < nb; b += 64) sh_hist[b] = bins[c * (size_t)nb + b];
    __syncthreads();
    DecConst C;
    memset(&C, 0, sizeof C);
    C.max_hyps = max_hyps[c]; C.hist_min = hist_min; C.hist_nbins = nb;
    const float th = hist_threshold(C, sh_hist, lane);
    if (lane == 0) out[c] = th;
}
extern "C" int jd_debug_hist_bin(int32_t device, const float *s, int64_t n, int32_t hist_min, int32_t hist_max, int32_t *out)
{
    if (!s || !out || n < 0 || hist_min > hist_max) return jd_fail(JD_EINVAL, "jd_debug_hist_bin: bad argument");
    for (int64_t i = 0; i < n; ++i)                          // (int)(s -+ 0.5) is defined, and equal on host and device, only here
        if (!(s[i] > -2147483648.0f && s[i] < 2147483648.0f)) return jd_fail(JD_EINVAL, "jd_debug_hist_bin: s[%lld] not in (-2^31, 2^31)", (long long)i);
    if (device == -1) {
        for (int64_t i = 0; i < n; ++i) out[i] = jd_hist_bin(s[i], hist_min, hist_max);
        return JD_OK;
    }
    int rc = check_device(device);
    if (rc) return rc;
    float *ds = nullptr;
    int *dy = nullptr;
    HIPCHK(hipMalloc(&ds, std::max<size_t>((size_t)n, 1) * sizeof(float)));
    HIPCHK(hipMalloc(&dy, std::max<size_t>((size_t)n, 1) * sizeof(int)));
    HIPCHK(hipMemcpy(ds, s, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    if (n) hipLaunchKernelGGL(jd_debug_hist_bin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ds, (long long)n,
                              (int)hist_min, (int)hist_max, dy);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dy, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(ds); (void)hipFree(dy);
    return JD_OK;
}
extern "C" int jd_debug_hist_threshold(int32_t device, const int32_t *bins, int64_t n_cases, int32_t nb, const int32_t *max_hyps,
                                       int32_t hist_min, float *out)
{
    if (!bins || !max_hyps || !out || n_cases < 0 || n_cases > INT32_MAX || nb < 1 || nb > HIST_MAX_BINS)
        return jd_fail(JD_EINVAL, "jd_debug_hist_threshold: bad argument");
    if (device == -1) return jd_fail(JD_EINVAL, "jd_debug_hist_threshold: hist_threshold has no host twin (device only)");
    for (int64_t c = 0; c < n_cases; ++c) {                // the kernels' domain: max_hyps > 0, counts that fit an int
        if (max_hyps[c] < 1) return jd_fail(JD_EINVAL, "jd_debug_hist_threshold: max_hyps[%lld] < 1", (long long)c);
        int64_t total = 0;
        for (int b = 0; b < nb; ++b) {
            const int32_t v = bins[c * nb + b];
            if (v < 0) return jd_fail(JD_EINVAL, "jd_debug_hist_threshold: negative count in case %lld", (long long)c);
            total += v;
        }
        if (total > INT32_MAX) return jd_fail(JD_EINVAL, "jd_debug_hist_threshold: case %lld counts more than INT32_MAX", (long long)c);
    }
    int rc = check_device(device);
    if (rc) return rc;
    int *db = nullptr, *dm = nullptr;
    float *dy = nullptr;
    const size_t nc = std::max<size_t>((size_t)n_cases, 1);
    HIPCHK(hipMalloc(&db, nc * (size_t)nb * sizeof(int)));
    HIPCHK(hipMalloc(&dm, nc * sizeof(int)));
    HIPCHK(hipMalloc(&dy, nc * sizeof(float)));
    HIPCHK(hipMemcpy(db, bins, (size_t)n_cases * (size_t)nb * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dm, max_hyps, (size_t)n_cases * sizeof(int), hipMemcpyHostToDevice));
    if (n_cases) hipLaunchKernelGGL(jd_debug_hist_threshold_kernel, dim3((unsigned)n_cases), dim3(64), 0, 0, db, (int)nb, dm, (int)hist_min, dy);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dy, (size_t)n_cases * sizeof(float), hipMemcpyDeviceToHost));
    (void)hipFree(db); (void)hipFree(dm); (void)hipFree(dy);
    return JD_OK;
}

// Diagnostics: what part of a likelihood table does the search read?  (SURVEY.md 8d's Ug: the reference scores a tied
// state only when a token that passed the emit threshold asks for it, WFSTDecoderLite.cpp:409-411; here every state of
// every frame is scored.)  enable != 0: the slab's bitmap is cleared and every cell phase A adds to a token is marked from
// the next launch on; enable == 0: the marks are counted against the cells of the last decode's frames and marking stops.
__global__ void jd_popcount_kernel(const unsigned *w, size_t n, unsigned long long *out)
{
    unsigned long long acc = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) acc += (unsigned)__popc(w[i]);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}
extern "C" int jd_dec_debug_cells(jd_dec *d, int32_t enable, int64_t *cells_read, int64_t *cells_total)
{
    if (!d) return jd_fail(JD_EINVAL, "jd_dec_debug_cells: null");
    int rc = check_device(d->device);
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    if (enable) {
        if (d->ll_cap == 0) return jd_fail(JD_ESTATE, "jd_dec_debug_cells: decode a batch first (the tables are sized by it)");
        const size_t words = (3 * d->ll_cap + 31) / 32 + 2;
        if (!d->d_cells || d->cells_words != words) {
            if (d->d_cells) (void)hipFree(d->d_cells);
            d->d_cells = nullptr;
            HIPCHK(hipMalloc(&d->d_cells, words * sizeof(unsigned)));
            d->cells_words = words;
        }
        HIPCHK(hipMemset(d->d_cells, 0, words * sizeof(unsigned)));
        return JD_OK;
    }
    unsigned long long n = 0;
    if (d->d_cells) {
        unsigned long long *dn = (unsigned long long *)d->d_cells;      // (the first two words: the counter)
        HIPCHK(hipMemset(dn, 0, sizeof(unsigned long long)));
        hipLaunchKernelGGL(jd_popcount_kernel, dim3(1024), dim3(256), 0, 0, d->d_cells + 2, d->cells_words - 2, dn);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(&n, dn, sizeof n, hipMemcpyDeviceToHost));
        (void)hipFree(d->d_cells);
        d->d_cells = nullptr; d->cells_words = 0;
    }
    if (cells_read) *cells_read = (int64_t)n;
    if (cells_total) *cells_total = (int64_t)d->timing.search_frames * d->am->n_gmm;
    return JD_OK;
}

int jd_dec_spliced(const jd_dec *d) { return d && d->am->mlp_spliced ? 1 : 0; }
extern "C" int jd_dec_info(const jd_dec *d, int32_t *max_streams, int32_t *vec_size)
{
    if (!d) return jd_fail(JD_EINVAL, "jd_dec_info: null");
    if (max_streams) *max_streams = d->max_streams;
    if (vec_size) *vec_size = d->am->D;
    return JD_OK;
}

extern "C" int jd_dec_last_timing(const jd_dec *d, jd_timing *out)
{
    if (!d || !out) return jd_fail(JD_EINVAL, "jd_dec_last_timing: null");
    *out = d->timing;
    return JD_OK;
}
