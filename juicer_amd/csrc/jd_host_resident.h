// jd_host_resident.h - host side of the search kernels that STAY on the device (included by jd_device.hip; not a translation unit of
// its own: it lives in jd_device.hip's TU because the kernels it launches are templates of that TU).
//
//   * Resident: the mailbox protocol of jd_resident.h / jd_slot.h (commands in host-mapped words, ready numbers counted up on the side
//     stream, reports, the host heartbeat) - jd_res_start / _stop / _post / _poll / _collect / _finish, driven by jd_broker.cpp; the
//     kernel's geometry is jd_plan.h's plan_resident, jd_res_start the steps that bring it onto the device;
//   * Pipe: batches through the resident slot kernel utterance by utterance (jd_dec_set_pipeline: JD_FLOW_RESIDENT) - pipe_announce,
//     pipe_pump, pipe_decode, jd_dec_quiesce, jd_dec_pipeline_stats.  What they DECIDE - the record of a stream's mailbox, which slot
//     takes which utterance, the commands, the ready numbers, the scoring pieces, the watchdog, the drain - is jd_pipe.h (no HIP,
//     tested on the CPU); here are the launches, event queries, mailbox accesses and statistics those decisions ask for;
//   * at the end, the setters that drop what the pipeline holds: jd_dec_set_output_level / _get_output_level, jd_dec_model_result,
//     jd_dec_set_scoring.
// The launch-per-call paths (one batch, two batches in flight, re-planning, the streaming calls) stay in jd_device.hip.
#pragma once

// ------------------------------------------------------------------------------------------------------------------
// The resident search kernel (jd_resident.h) and its host side: what jd_broker.cpp drives instead of ticks.
// While it runs it owns the device's search lock (this process) and the GPU's file lock (other processes); nothing here
// allocates or frees device memory or synchronises the device - either would wait for the kernel.
#define RES_RING 256
#define RES_RING_W 2048
// (ResStream, the protocol as the host sees it for one stream, and its two transitions - a command, a report: jd_pipe.h)
struct Resident {
    bool on = false;
    int n = 0, Cw = 0, rows = 0;                       // streams [0, n), workgroups per cluster, rows per likelihood buffer
    bool slot = false;                                 // one workgroup per stream: the slot kernel (jd_slot.h), SLOT_WG_PER_CU of them per CU
    ResMail *d_mail = nullptr;
    ResPost *h_post = nullptr;                         // host-mapped: the commands
    ResDone *h_done = nullptr;                         // host-mapped: the reports
    unsigned *h_beat = nullptr;                        // host-mapped: counted up whenever the host looks after the kernel (k_resident: beat)
    unsigned *d_ready = nullptr;                       // per stream: how far the side stream has come for it
    std::vector<ResStream> stream;
    int *h_ring = nullptr, *d_ring = nullptr;          // row-tile lists of the scoring launches (RES_RING slots of RES_RING_W)
    int ring_turn = 0;
    float *d_feat = nullptr, *d_ll = nullptr;          // [n][2][rows] x D / x G
    int *d_src = nullptr;
    char *h_stage = nullptr;                           // pinned: the features of every buffer, [n][2][rows] x D
    long long run_ticks = 0;                           // (statistics) what the clusters spent on their commands, 100 MHz ticks
    long long n_collect = 0;                           // (statistics) Path collections between commands
    std::unique_lock<std::mutex> search_lock;
    GpuLockGuard *process_lock = nullptr;
    std::chrono::steady_clock::time_point t_start;     // when the kernel was last started (jd_dec_pipeline_stats: time on the device)
    hipStream_t st = nullptr;                          // the stream the kernel runs on (the decoder's search stream, or its CU-masked slot stream)
};

static void res_free(jd_dec *d);
static ExportDst pipe_export_dst(const jd_dec *d);      // (the pipeline's virtual result slots, below: what k_slot is started with)
static void res_free_fwd(jd_dec *d) { res_free(d); }
static void res_free(jd_dec *d)
{
    Resident *R = d->res;
    if (!R) return;
    if (R->d_mail) (void)hipFree(R->d_mail);
    if (R->h_post) (void)hipHostFree(R->h_post);
    if (R->h_done) (void)hipHostFree(R->h_done);
    if (R->h_beat) (void)hipHostFree(R->h_beat);
    if (R->d_ready) (void)hipFree(R->d_ready);
    if (R->h_ring) (void)hipHostFree(R->h_ring);
    if (R->d_ring) (void)hipFree(R->d_ring);
    if (R->d_feat) (void)hipFree(R->d_feat);
    if (R->d_ll) (void)hipFree(R->d_ll);
    if (R->d_src) (void)hipFree(R->d_src);
    if (R->h_stage) (void)hipHostFree(R->h_stage);
    delete R;
    d->res = nullptr;
}

// pred() every sleep_us until it holds or ms are over; whether it held
template <class Pred>
static bool wait_until(Pred pred, double ms, int sleep_us)
{
    const auto t0 = std::chrono::steady_clock::now();
    while (!pred()) {
        if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() >= ms) return false;
        std::this_thread::sleep_for(std::chrono::microseconds(sleep_us));
    }
    return true;
}

// a workgroup of streams [0, n) has left the kernel (no command for 5 s, an exit request, a lost workgroup)
static bool res_any_left(const Resident *R, int n)
{
    for (int s = 0; s < n; ++s)
        if (__atomic_load_n(&R->h_done[s].left, __ATOMIC_ACQUIRE) != 0) return true;
    return false;
}

// the report of stream s's command, if it is in
static bool res_harvest(jd_dec *d, int s)
{
    Resident *R = d->res;
    ResStream &S = R->stream[s];
    if (!S.busy) return true;
    if (!res_stream_answered(S, __atomic_load_n(&R->h_done[s].seq, __ATOMIC_ACQUIRE))) return false;
    const int advanced = res_stream_report(S, R->h_done[s].frame, R->h_done[s].error, R->h_done[s].exported);
    if (d->pipe_on) {                                                  // (jd_dec_pipeline_stats: frames the slot has advanced)
        d->pipe_frames_searched += advanced;
        d->pipe_busy_ticks += R->h_done[s].run_ticks;
    }
    // (a stream that failed on the device - an arena overflow, a lost workgroup - may hold anything: wiped before its next init,
    // whether or not anybody fetches its result)
    if (S.err_done != 0) d->stream_dirty[(size_t)s] = 1;
    R->run_ticks += R->h_done[s].run_ticks;
    d->push[(size_t)s].T = S.T_done;
    return true;
}

int jd_res_stop(jd_dec *d)
{
    if (!d) return JD_OK;
    std::lock_guard<std::recursive_mutex> guard(d->res_mu);            // (a finish that is being fetched goes first)
    if (!d->res || !d->res->on) return JD_OK;
    Resident *R = d->res;
    for (int s = 0; s < R->n; ++s) __atomic_store_n(&R->h_post[s].exit_req, 1, __ATOMIC_RELEASE);
    hipError_t e = hipStreamSynchronize(R->st ? R->st : d->s_search);  // (it also leaves by itself after RES_IDLE_TICKS)
    (void)hipStreamSynchronize(d->s_gmm);
    // (a cluster takes a command that is there before it looks at the exit request: whatever was posted is through)
    bool lost = false;
    for (int s = 0; s < R->n; ++s)
        if (!res_harvest(d, s)) {
            R->stream[s].busy = false;
            // a command the cluster never saw (it left by itself - idle for 5 s - just before the word was written) has not been
            // started: the stream stands where its last report says, short of what was posted, and whoever drives it posts the
            // rest again (the same way as behind a Path collection).  Anything else is a lost workgroup.
            if (!__atomic_load_n(&R->h_done[s].left, __ATOMIC_ACQUIRE)) { lost = true; d->stream_dirty[(size_t)s] = 1; }
        }
    R->on = false;
    if (d->pipe_on) d->pipe_on_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - R->t_start).count();
    delete R->process_lock; R->process_lock = nullptr;
    if (R->search_lock.owns_lock()) R->search_lock.unlock();
    if (e != hipSuccess) return jd_fail(JD_EHIP, "the resident search kernel did not end: %s", hipGetErrorString(e));
    if (lost) return jd_fail(JD_EHIP, "the resident search kernel ended with a command unanswered");
    return JD_OK;
}

// ---- jd_res_start, step by step

// The flavours of the kernels that stay on the device (the counterparts of jd_host_launch.h's search_kernel / slot_kernel; they are
// here and in this order because a template kernel's place in the device code object is where the translation unit first names it,
// and the object stays as it has been): k_slot (jd_slot.h: HMM size class, word / model-level output) ...
typedef void (*SlotMailboxKernel)(SearchArgs, const ResPost *, const unsigned *, ResDone *, const unsigned *, unsigned *, ExportDst);
static SlotMailboxKernel slot_mailbox_kernel(bool ne3, bool mdl)
{
    static const SlotMailboxKernel tab[4] = { k_slot<3, true>, k_slot<3, false>, k_slot<6, true>, k_slot<6, false> };
    return tab[(ne3 ? 0 : 2) + (mdl ? 0 : 1)];
}
// ... and k_resident (jd_resident.h: HMM size class, agent-scope / XCD-local memory model, word / model-level output)
typedef void (*ResidentKernel)(SearchArgs, const ResPost *, ResMail *, const unsigned *, ResDone *, int, const unsigned *);
static ResidentKernel resident_kernel(bool ne3, bool xl, bool mdl)
{
    static const ResidentKernel tab[8] = {
        k_resident<3, false, true>, k_resident<3, false, false>, k_resident<6, false, true>, k_resident<6, false, false>,
        k_resident<3, true, true>, k_resident<6, true, true>, k_resident<3, true, false>, k_resident<6, true, false>,
    };
    return tab[xl ? 4 + (mdl ? 0 : 2) + (ne3 ? 0 : 1) : (ne3 ? 0 : 2) + (mdl ? 0 : 1)];
}

static int res_knob(const char *name) { const char *e = jd_dev_env(name); return e ? atoi(e) : -1; }   // development; -1: unset

// the kernel's geometry (jd_plan.h: plan_resident) from the decoder and the development knobs
static ResPlanOut res_plan(const jd_dec *d, int n_streams, int rows_per_buf)
{
    ResPlanIn in;
    in.n_cus = d->n_cus; in.n_streams = n_streams; in.rows_per_buf = rows_per_buf;
    in.max_cw = d->max_cw; in.cap_slots = d->cap_slots; in.cap_items = d->cap_items;
    in.pipeline = d->res_ll != nullptr;
    in.free_cus = res_knob("JD_RES_FREE_CUS"); in.slot = res_knob("JD_RES_SLOT"); in.xl = res_knob("JD_RES_XL"); in.keep_se = res_knob("JD_SLOT_KEEP_SE");
    in.sw = SW; in.wg_per_cu = WG_PER_CU; in.slot_wg_per_cu = SLOT_WG_PER_CU; in.gmm_rows2 = GMM_ROWS2; in.res_ring_w = RES_RING_W;
    return plan_resident(in);
}

static int res_fill(jd_dec *d, Resident *R, int n_streams, int rows)
{
    const int D = d->am->D, G = d->am->n_gmm;
    // (jd_res_stage_many lists a buffer's row tiles by first row, (2 s + buf) rows + 128 t: a buffer of whole tiles - plan_resident
    // rounds what jd_res_start is given - or a listed tile would write the next buffer's rows)
    if (rows < 1 || rows % GMM_ROWS2 != 0) return jd_fail(JD_EINVAL, "jd_res_start: %d rows per buffer, not whole scoring tiles of %d", rows, GMM_ROWS2);
    R->n = n_streams; R->rows = rows;
    const size_t tr = (size_t)n_streams * 2 * rows;
    if (hipMalloc(&R->d_mail, (size_t)n_streams * sizeof(ResMail)) != hipSuccess ||
        hipHostMalloc((void **)&R->h_post, (size_t)n_streams * sizeof(ResPost), hipHostMallocMapped) != hipSuccess ||
        hipHostMalloc((void **)&R->h_done, (size_t)n_streams * sizeof(ResDone), hipHostMallocMapped) != hipSuccess ||
        hipHostMalloc((void **)&R->h_beat, 64, hipHostMallocMapped) != hipSuccess ||
        hipMalloc(&R->d_ready, (size_t)n_streams * sizeof(unsigned)) != hipSuccess ||
        hipHostMalloc((void **)&R->h_ring, (size_t)RES_RING * RES_RING_W * sizeof(int)) != hipSuccess ||
        hipMalloc(&R->d_ring, (size_t)RES_RING * RES_RING_W * sizeof(int)) != hipSuccess ||
        hipMalloc(&R->d_feat, tr * D * sizeof(float)) != hipSuccess || hipMalloc(&R->d_ll, tr * G * sizeof(float)) != hipSuccess ||
        hipMalloc(&R->d_src, tr * sizeof(int)) != hipSuccess ||
        hipHostMalloc((void **)&R->h_stage, tr * D * sizeof(float)) != hipSuccess)
        return jd_fail(JD_ENOMEM, "jd_res_start: no memory for %d streams x 2 x %d rows", n_streams, rows);
    *R->h_beat = 0u;
    R->stream.resize((size_t)n_streams);
    for (int t = 0; t < n_streams; ++t) R->stream[t].reset(&d->push[(size_t)t].T);
    std::vector<int> ident(tr);            // the row table of every scoring launch: row r of the table is row r of the features
    for (size_t r = 0; r < tr; ++r) ident[r] = (int)r;
    HIPCHK(hipMemcpy(R->d_src, ident.data(), ident.size() * sizeof(int), hipMemcpyHostToDevice));
    return JD_OK;
}

// d->res for n_streams streams and buffers of `rows` rows: the whole of it, or none (and the code)
static int res_alloc(jd_dec *d, int n_streams, int rows)
{
    d->res = new Resident();
    const int rc = res_fill(d, d->res, n_streams, rows);
    if (rc) res_free(d);
    return rc;
}

// the kernel is about to start: an empty mailbox, and the numbers of both sides begin again (ResStream::reset)
static void res_reset(Resident *R)
{
    memset(R->h_done, 0, (size_t)R->n * sizeof(ResDone));
    memset(R->h_post, 0, (size_t)R->n * sizeof(ResPost));
    for (int s = 0; s < R->n; ++s) R->h_post[s].vslot = -1;
    for (ResStream &S : R->stream) S.reset(nullptr);
}

// all the kernel's workgroups have to be resident at once: asked of the runtime for the kernel the plan chose
static int res_occupancy(const jd_dec *d, const Resident *R)
{
    const bool ne3 = d->am->max_n <= 5;
    int per_cu = 0;
    // (k_resident: asked of the agent-scope flavour, XL = false, even where the XCD-local one is what is launched - as it has
    // always been; the two differ in the scope of their memory operations.  Known, and not changed here.)
    const void *kf = R->slot ? (const void *)slot_mailbox_kernel(ne3, d->models) : (const void *)resident_kernel(ne3, false, d->models);
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kf, SNT, 0));
    const int need = R->slot ? SLOT_WG_PER_CU : WG_PER_CU;
    if (per_cu < need)
        return jd_fail(R->slot ? JD_EINVAL : JD_EHIP, "%s: %d workgroup(s) per CU fit, %d streams on %d CUs need %d", R->slot ? "k_slot" : "k_resident",
                       per_cu, R->n, d->n_cus, need);
    return JD_OK;
}

// The locks the kernel owns while it is on the device - the device's search lock, the GPU's file lock - go back when
// jd_res_start is left without it (R->on is not set), whichever way.
struct ResLocks {
    Resident *R;
    ~ResLocks()
    {
        if (R->on) return;
        delete R->process_lock; R->process_lock = nullptr;
        if (R->search_lock.owns_lock()) R->search_lock.unlock();
    }
};

struct ResLaunch {                                     // what an attempt to start the kernel takes, the same for every attempt
    SearchArgs A;
    bool ne3, xl;
    int park_cus, park_fill;                           // (slots) CUs parked while the grid is dealt, and the slots that find room beside them
    ExportDst E;                                       // (slots) the pipeline's virtual result slots, or nulls
    hipEvent_t ev_side = nullptr, ev_null = nullptr;   // behind the probes on the side stream and the null stream
    ~ResLaunch() { if (ev_side) (void)hipEventDestroy(ev_side); if (ev_null) (void)hipEventDestroy(ev_null); }
};

static int res_launch_init(jd_dec *d, const Resident *R, const ResPlanOut &P, ResLaunch *L)
{
    SearchArgs &A = L->A;
    memset(&A, 0, sizeof A);
    A.C = d->C; A.ctl = d->d_ctl; A.streams = d->d_streams; A.work = nullptr; A.n_work = R->n; A.Cw = R->Cw; A.n_slots = 0;
    A.ll = d->res_ll ? d->res_ll : R->d_ll; A.ll_stride = (long long)d->am->n_gmm; A.f0 = 0; A.f_end = 0x7fffffff;
    A.status = d->d_status; A.dbg = d->d_dbg; A.cells = nullptr; A.resident = nullptr; A.rebalance_at = 0; A.n_prio = 0;   // (dbg: jd_dec_debug_trace)
    L->ne3 = d->am->max_n <= 5; L->xl = P.xl;
    L->park_cus = P.park_cus; L->park_fill = P.park_fill;
    L->E = pipe_export_dst(d);
    if (L->park_cus > 0 && !d->h_park) {                               // (jd_park_kernel's words; without them nothing is parked)
        if (hipHostMalloc((void **)&d->h_park, 64, hipHostMallocMapped) != hipSuccess || hipMalloc(&d->d_park, 64 * sizeof(int)) != hipSuccess) {
            (void)hipGetLastError();
            L->park_cus = 0;
        }
    }
    HIPCHK(hipEventCreateWithFlags(&L->ev_side, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&L->ev_null, hipEventDisableTiming));
    return JD_OK;
}

// Where the slots go.  A grid of at most one workgroup per CU is dealt one per CU, and that is what the pipeline wants: a slot's eight
// waves take two of a SIMD's four wave slots and half its registers, the scoring kernel's waves (127 VGPRs, no LDS) take the other half
// of the SAME CU - a search that waits for memory beside arithmetic that does not: 256 slots on 256 CUs 18.1 ms per configs[1] batch,
// against 21.5 with the slots two per CU on half the chip and the scoring on the other half (jd_slot.h: jd_park_kernel, which is how
// such a split is made: JD_SLOT_KEEP_SE = CUs per shader engine the slots get, development), 19.1 with 272 and 21.1 with 304 slots
// dealt over all CUs (the CUs that hold two slots have no room for the scoring).
static void park_and_launch_slots(jd_dec *d, Resident *R, const ResLaunch &L)
{
    bool parked = false;
    if (L.park_cus > 0) {
        // the CUs of every XCD that the slots are NOT to get: parked until the slots are on theirs
        d->h_park[0] = d->h_park[1] = d->h_park[2] = d->h_park[3] = d->h_park[4] = 0u;
        if (hipMemsetAsync(d->d_park, 0, 64 * sizeof(int), d->s_gmm) == hipSuccess) {
            hipLaunchKernelGGL(jd_park_kernel, dim3((unsigned)d->n_cus), dim3(64), 0, d->s_gmm, (unsigned *)d->d_park, L.park_cus / 32, d->h_park);
            parked = hipGetLastError() == hipSuccess;
        }
        if (parked)
            wait_until([&] { return __atomic_load_n(&d->h_park[0], __ATOMIC_ACQUIRE) + __atomic_load_n(&d->h_park[1], __ATOMIC_ACQUIRE) >= (unsigned)d->n_cus; },
                       50.0, 20);
    }
    unsigned *started = parked ? d->h_park + 4 : nullptr;
    hipLaunchKernelGGL(slot_mailbox_kernel(L.ne3, d->models), dim3((unsigned)R->n), dim3(SNT), 0, R->st, L.A, R->h_post, R->d_ready, R->h_done, R->h_beat,
                       started, L.E);
    if (!parked) return;
    // every slot is on its CU (or 100 ms are over): the parked CUs are the scoring's
    const auto tp = std::chrono::steady_clock::now();
    wait_until([&] { return __atomic_load_n(&d->h_park[4], __ATOMIC_ACQUIRE) >= (unsigned)L.park_fill; }, 100.0, 20);
    if (getenv("JD_VERBOSE"))
        fprintf(stderr, "k_slot: %u CUs parked (%u left free), %u of %d slots on their CUs after %.2f ms\n", d->h_park[0], d->h_park[1], d->h_park[4], R->n,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count());
    __atomic_store_n(&d->h_park[2], 1u, __ATOMIC_RELEASE);
}

// HIP maps streams onto a few hardware queues, and whatever is queued BEHIND a kernel that stays waits until it leaves:
// the side stream's scoring, the null stream's copies back.  Which queue a stream gets is the runtime's business
// (tools/resident_alias_probe.py: one fresh stream in fourteen lands behind the kernel), so the kernel is started, a
// small kernel is sent down the side stream and the null stream, and if either has not come back in 150 ms the
// resident kernel leaves again (jd_res_start: it comes back on a NEW search stream - a few times, then it is an error).
// One attempt.  *clear: the kernel is on the device and neither stream is queued behind it.
static hipError_t launch_and_probe(jd_dec *d, Resident *R, const ResLaunch &L, bool *clear)
{
    hipLaunchKernelGGL(jd_res_reset_kernel, dim3((R->n + 63) / 64), dim3(64), 0, R->st, d->d_ctl, R->d_mail, R->d_ready, R->n);
    __atomic_fetch_add(R->h_beat, 1u, __ATOMIC_RELEASE);
    if (R->slot) park_and_launch_slots(d, R, L);
    else
        hipLaunchKernelGGL(resident_kernel(L.ne3, L.xl, d->models), dim3((unsigned)(R->n * R->Cw)), dim3(SNT), 0, R->st, L.A, R->h_post, R->d_mail, R->d_ready,
                           R->h_done, R->Cw, R->h_beat);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ReadyList none; none.n = 0;
    hipLaunchKernelGGL(jd_res_ready_kernel, dim3(1), dim3(64), 0, d->s_gmm, R->d_ready, none);
    (void)hipEventRecord(L.ev_side, d->s_gmm);
    hipLaunchKernelGGL(jd_res_ready_kernel, dim3(1), dim3(64), 0, (hipStream_t)0, R->d_ready, none);
    (void)hipEventRecord(L.ev_null, (hipStream_t)0);
    *clear = wait_until([&] { return hipEventQuery(L.ev_side) == hipSuccess && hipEventQuery(L.ev_null) == hipSuccess; }, 150.0, 200);
    if (*clear) return hipSuccess;
    // behind the kernel: it leaves (the exit word) and what waited for it runs
    for (int t = 0; t < R->n; ++t) __atomic_store_n(&R->h_post[t].exit_req, 1, __ATOMIC_RELEASE);
    (void)hipStreamSynchronize(R->st);
    (void)hipEventSynchronize(L.ev_side); (void)hipEventSynchronize(L.ev_null);
    res_reset(R);
    return hipSuccess;
}

// the search stream is made anew (for the kernel's next attempt)
static bool fresh_search_stream(jd_dec *d, Resident *R)
{
    hipStream_t fresh = nullptr;
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (hipStreamCreateWithPriority(&fresh, hipStreamNonBlocking, prio_hi) != hipSuccess) return false;
    d->res_old_streams.push_back(d->s_search);                         // (destroyed with the decoder: somebody may still hold it)
    d->s_search = fresh; R->st = fresh;
    return true;
}

// streams [0, n_streams) of the decoder, likelihood buffers of rows_per_buf rows (two per stream)
int jd_res_start(jd_dec *d, int n_streams, int rows_per_buf)
{
    if (!d || n_streams < 1 || n_streams > d->max_streams || rows_per_buf < 1) return jd_fail(JD_EINVAL, "jd_res_start: bad argument");
    std::lock_guard<std::recursive_mutex> guard(d->res_mu);
    if (d->net->lazy_dev || d->partial_interval > 0) return jd_fail(JD_ESTATE, "jd_res_start: not with a lazily composed network / partial traces");
    int rc = check_device(d->device);
    if (rc) return rc;
    rc = ensure_arenas(d);
    if (rc) return rc;
    if (!d->pipe_on) pf_discard(d);                      // (not when the batch pipeline's kernel comes back: jd_dec_quiesce)
    const ResPlanOut P = res_plan(d, n_streams, rows_per_buf);
    if (d->res && (d->res->n != n_streams || d->res->rows != P.rows)) { if (d->res->on) { rc = jd_res_stop(d); if (rc) return rc; } res_free(d); }
    if (!d->res) {
        // (the limits bind where a Resident is made: one that exists has passed them)
        if (P.verdict == RES_PLAN_LIMITS) return jd_fail(JD_EINVAL, "jd_res_start: at most 1024 streams and %d row tiles per scoring launch", RES_RING_W);
        rc = res_alloc(d, n_streams, P.rows);
        if (rc) return rc;
    }
    Resident *R = d->res;
    if (R->on) return JD_OK;
    R->Cw = P.Cw; R->slot = P.slot;
    rc = res_occupancy(d, R);
    if (rc) return rc;
    if (P.verdict == RES_PLAN_CLUSTERS) return jd_fail(JD_EINVAL, "jd_res_start: %d streams do not fit the device", n_streams);
    if (P.verdict == RES_PLAN_SLOTS)
        return jd_fail(JD_EINVAL, "jd_res_start: %d one-workgroup slots do not fit the device (%d CUs x %d workgroups of k_slot resident at once)",
                       n_streams, d->n_cus, SLOT_WG_PER_CU);
    res_reset(R);
    const size_t dev_i = dev_index(d);
    if (d->res_yield_turn >= 0) {
        // this kernel has just made room for somebody who waits for the device (jd_res_yield): a mutex hands itself to
        // whoever asks first, which may well be the one who let go - so it asks only once the waiter has had its turn
        wait_until([&] { return g_search_turn[dev_i].load() != d->res_yield_turn || g_search_waiters[dev_i].load() <= 0; }, 500.0, 100);
        d->res_yield_turn = -1;
    }
    R->search_lock = lock_search(dev_i);
    R->process_lock = new GpuLockGuard(d->device);
    const ResLocks locks{R};
    ResLaunch L;
    rc = res_launch_init(d, R, P, &L);
    if (rc) return rc;
    R->st = d->s_search;
    hipError_t e = hipSuccess;
    bool clear = false;
    for (int attempt = 0; attempt < 8 && !clear; ++attempt) {
        e = launch_and_probe(d, R, L, &clear);
        if (e != hipSuccess || clear) break;
        if (!fresh_search_stream(d, R)) { e = hipErrorUnknown; break; }
        if (getenv("JD_VERBOSE")) fprintf(stderr, "k_resident: the side stream or the null stream was queued behind it - a new search stream (%d)\n", attempt + 1);
    }
    if (e != hipSuccess) return jd_fail(JD_EHIP, "k_resident: %s", hipGetErrorString(e));
    if (!clear) return jd_fail(JD_EHIP, "k_resident: no search stream whose hardware queue the side stream and the null stream do not share");
    R->on = true;
    R->t_start = std::chrono::steady_clock::now();
    if (getenv("JD_VERBOSE")) fprintf(stderr, "%s: %d streams, clusters of %d workgroups, %d rows per buffer%s\n", R->slot ? "k_slot" : "k_resident", R->n, R->Cw, R->rows,
                                      L.park_cus > 0 ? " (the other CUs parked while its grid was dealt)" : "");
    return JD_OK;
}

int jd_res_cluster(const jd_dec *d) { return (d && d->res) ? d->res->Cw : 0; }
// the kernel leaves for somebody who waits for the device, and comes back behind them (jd_res_start)
int jd_res_yield(jd_dec *d)
{
    if (!d || !d->res || !d->res->on) return JD_OK;
    d->res_yield_turn = g_search_turn[dev_index(d)].load();
    return jd_res_stop(d);
}
// somebody else of this process waits for the device's search lock (another decoder's launch, another broker's kernel)
int jd_res_should_yield(const jd_dec *d)
{
    return (d && d->res && d->res->on) ? g_search_waiters[dev_index(d)].load() > 0 : 0;
}
long long jd_res_run_us(const jd_dec *d) { return (d && d->res) ? d->res->run_ticks / 100 : 0; }
long long jd_res_collections(const jd_dec *d) { return (d && d->res) ? d->res->n_collect : 0; }

// "the side stream has come this far" for these streams: a new ready number each, behind everything enqueued so far
static int res_bump(jd_dec *d, int n, const int *streams)
{
    Resident *R = d->res;
    for (int i0 = 0; i0 < n; i0 += 64) {
        ReadyList L;
        L.n = std::min(64, n - i0);
        for (int i = 0; i < L.n; ++i) { const int s = streams[i0 + i]; L.s[i] = s; L.id[i] = ++R->stream[s].rid; }
        hipLaunchKernelGGL(jd_res_ready_kernel, dim3(1), dim3(64), 0, d->s_gmm, R->d_ready, L);
        HIPCHK(hipGetLastError());
    }
    return JD_OK;
}

// IDecoder::init of stream s (idle): recognitionStart runs with the stream's next command
int jd_res_init(jd_dec *d, int s)
{
    std::lock_guard<std::recursive_mutex> guard(d->res_mu);            // (the wipe of a failed stream stops and starts the kernel)
    Resident *R = d->res;
    if (!R || !R->on || s < 0 || s >= R->n) return jd_fail(JD_ESTATE, "jd_res_init: no resident kernel for stream %d", s);
    if (d->stream_dirty[(size_t)s]) {                                  // (after an error: the wipe synchronises the device)
        int rc = jd_res_stop(d);
        if (rc) return rc;
        rc = wipe_stream(d, s);
        if (rc) return rc;
        rc = jd_res_start(d, R->n, R->rows);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(jd_mark_init_kernel, dim3(1), dim3(64), 0, d->s_gmm, d->d_ctl, s, 1);
    HIPCHK(hipGetLastError());
    d->push[(size_t)s].begin();
    R->stream[s].T_posted = 0; R->stream[s].T_done = 0; R->stream[s].err_done = 0;
    return res_bump(d, 1, &s);
}

// Frames of n streams into their likelihood buffers bufs[i] (0 / 1, free): an upload per stream from the buffer's own
// pinned staging region, ONE scoring launch over the row tiles concerned (asynchronous, on the side stream), and the
// streams' ready numbers behind it
int jd_res_stage_many(jd_dec *d, int n, const int *streams, const int *bufs, const float *const *frames, const int *n_frames)
{
    Resident *R = d->res;
    if (!R || !R->on) return jd_fail(JD_ESTATE, "jd_res_stage_many: no resident kernel");
    const int D = d->am->D;
    const size_t tr = (size_t)R->n * 2 * R->rows;
    int *list = R->h_ring + (size_t)R->ring_turn * RES_RING_W;
    int *d_list = R->d_ring + (size_t)R->ring_turn * RES_RING_W;
    int nt = 0, ns = 0;
    std::vector<int> who;
    for (int i = 0; i < n; ++i) {
        const int s = streams[i], buf = bufs[i], nf = n_frames[i];
        if (s < 0 || s >= R->n || (buf != 0 && buf != 1) || nf < 0 || nf > R->rows || (nf > 0 && !frames[i]))
            return jd_fail(JD_EINVAL, "jd_res_stage_many: bad argument");
        if (nf == 0) continue;
        const size_t r0 = ((size_t)s * 2 + (size_t)buf) * (size_t)R->rows;
        float *hf = (float *)R->h_stage + r0 * D;
        memcpy(hf, frames[i], (size_t)nf * D * sizeof(float));
        HIPCHK(hipMemcpyAsync(R->d_feat + r0 * D, hf, (size_t)nf * D * sizeof(float), hipMemcpyHostToDevice, d->s_gmm));
        for (int t = 0; t < (nf + GMM_ROWS2 - 1) / GMM_ROWS2; ++t) list[nt++] = (int)r0 + t * GMM_ROWS2;
        who.push_back(s);
        ++ns;
    }
    if (ns == 0) return JD_OK;
    R->ring_turn = (R->ring_turn + 1) % RES_RING;
    HIPCHK(hipMemcpyAsync(d_list, list, (size_t)nt * sizeof(int), hipMemcpyHostToDevice, d->s_gmm));
    // (a tile's rows behind the chunk's last frame are scored too - whatever the buffer holds there - and read by nobody)
    const int rc = launch_gmm(d->am, d->amb, R->d_feat, R->d_src, (int)tr, R->d_ll, d->s_gmm, 0, 0, nt, d_list, nt);
    if (rc) return rc;
    return res_bump(d, ns, who.data());
}

// The command "frames up to T, likelihood rows from `slot`" for stream s: the host's record of it, and the command itself - a word
// in host-mapped memory (the cluster's first workgroup polls it), behind the ready number the stream has now.
// init: the command begins an utterance.  vslot (the pipeline's slots): the command ends one - ResPost::vslot.
static void res_command(Resident *R, int s, int T, int slot, bool init, int vslot = -1)
{
    const ResCommand C = res_stream_command(R->stream[s], T, slot, init, vslot);
    __atomic_fetch_add(R->h_beat, 1u, __ATOMIC_RELAXED);               // (a sign of life: k_resident's `beat`)
    ResPost &P = R->h_post[s];
    P.T = C.T;
    P.init = C.init;
    P.vslot = C.vslot;
    P.ready_id = C.ready_id;
    __atomic_store_n(&P.word, C.word, __ATOMIC_RELEASE);
}

// The command "frames up to T + n_frames are scored in buffer buf" for stream s (idle), behind what has been staged
int jd_res_post(jd_dec *d, int s, int buf, int n_frames)
{
    Resident *R = d->res;
    if (!R || !R->on || s < 0 || s >= R->n) return jd_fail(JD_ESTATE, "jd_res_post: no resident kernel for stream %d", s);
    const int T0 = R->stream[s].T_done;
    const long long slot = ((long long)s * 2 + buf) * R->rows - T0;    // (k_search reads row  slot + f: see jd_streams_push)
    res_command(R, s, T0 + n_frames, (int)slot, false);
    return JD_OK;
}

// Where stream s stands: *idle = its last command is through (then *frame = frames processed, *error = StreamCtl::error,
// *stopped = it stopped short of what was posted - a Path collection is due: jd_res_collect)
int jd_res_poll(jd_dec *d, int s, int *idle, int *frame, int *error, int *stopped)
{
    Resident *R = d->res;
    if (!R || !R->on || s < 0 || s >= R->n) return jd_fail(JD_ESTATE, "jd_res_poll: no resident kernel for stream %d", s);
    __atomic_fetch_add(R->h_beat, 1u, __ATOMIC_RELAXED);               // (a sign of life: k_resident's `beat`)
    const bool through = res_harvest(d, s);
    const ResStream &S = R->stream[s];
    *idle = through ? 1 : 0;
    if (frame) *frame = S.T_done;
    if (error) *error = S.err_done;
    if (stopped) *stopped = (through && S.err_done == 0 && S.T_done < S.T_posted) ? 1 : 0;
    if (through) return JD_OK;
    if (__atomic_load_n(&R->h_done[s].left, __ATOMIC_ACQUIRE))
        return jd_fail(JD_ESTATE, "the resident search kernel has ended (no command for 5 s, or a lost workgroup)");
    return JD_OK;
}

// the device-side error a poll reported for stream s, as the library's code (jd_last_error() has the text)
int jd_res_stream_error(jd_dec *d, int s, int dev_error, int frame)
{
    return report_stream_error(d, s, dev_error, frame, 1);
}

// collectPaths for stream s (idle, stopped), then the rest of its command again
int jd_res_collect(jd_dec *d, int s)
{
    Resident *R = d->res;
    if (!R || !R->on || s < 0 || s >= R->n) return jd_fail(JD_ESTATE, "jd_res_collect: no resident kernel for stream %d", s);
    launch_gc(d->C, d->d_ctl, d->d_streams, nullptr, 1, s, d->am->max_n <= 5, std::max(8, d->n_cus / 6), d->s_gmm);
    HIPCHK(hipGetLastError());
    R->n_collect += 1;
    if (d->pipe_on) d->pipe_collections += 1;
    // (the command waits for the collection: the ready number first - the word carries the one the stream has THEN)
    const int rc = res_bump(d, 1, &s);
    if (rc) return rc;
    const ResStream &S = R->stream[s];
    res_command(R, s, S.T_posted, S.slot_posted, S.init_pending, S.vslot_posted);   // (an utterance's first command says again that it is)
    return JD_OK;
}

// IDecoder::finish of stream s (idle, every frame it was given processed)
int jd_res_finish(jd_dec *d, int s, jd_hyp *out)
{
    // (the broker's finisher thread, beside its worker: the kernel is neither stopped nor started while a result is fetched -
    // a stop wipes device state and synchronises the device - and this thread's launches go to the decoder's device)
    std::lock_guard<std::recursive_mutex> guard(d->res_mu);
    int rc0 = check_device(d->device);
    if (rc0) return rc0;
    Resident *R = d->res;
    if (!R || !R->on || s < 0 || s >= R->n || !out) return jd_fail(JD_ESTATE, "jd_res_finish: no resident kernel for stream %d", s);
    hipLaunchKernelGGL(jd_finish_kernel, dim3(1), dim3(64), 0, d->s_gmm, d->d_ctl, d->d_streams, s, 1, res_model_of(d));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(d->s_gmm));
    std::vector<jd_hyp> tmp((size_t)d->max_streams);
    const int rc = fetch_results(d, s, 1, tmp.data(), s);
    *out = tmp[(size_t)s];
    return rc;
}


// ------------------------------------------------------------------------------------------------------------------
// Batches through the resident kernel, UTTERANCE BY UTTERANCE (JD_PIPELINE=3).  A batch lasts as long as its longest
// utterance; with two batches in flight (above) the streams of a bank still wait for their bank to be handed back.  Here
// every stream is a slot of the resident kernel with ONE workgroup: announced batches (jd_dec_prefetch_scores, up to
// pipe_depth of them) are scored whole into a table of their own, their utterances queue up, and a slot whose utterance is
// through takes the next one at once - its result exported to a virtual result slot first (jd_finish_export_kernel) - so
// that no workgroup waits for anybody.  jd_decode_batch_device of the OLDEST announced batch waits until its utterances are
// through and hands them back; it is also what keeps the slots fed (the pump runs inside the calls - no thread).  Results
// are those of any other path; what changes is that a batch takes as long as its longest utterance on one workgroup.
// What is decided about them is decided in jd_pipe.h (PipeState: the queue of batches, the slots, the pieces); here, what is on the device.
static_assert(sizeof(ExportList().slot) / sizeof(int) == PIPE_EXPORTS, "pipe_export_add fills jd_gc.h's ExportList");
struct Pipe : PipeState {
    bool on = false;
    float *d_ll = nullptr;                             // K tables
    int *d_ident = nullptr;                            // row r is frame r of the batch's features
    StreamCtl *d_vctl = nullptr; int *d_vresn = nullptr, *d_vres = nullptr;   // K x max_batch virtual result slots
    int *d_vres_model = nullptr;                       // ... their models (model-level output)
    std::chrono::steady_clock::time_point t_on;        // (statistics)
    hipEvent_t ev_piece[2] = { nullptr, nullptr };     // behind the scoring pieces that are out; the oldest is ev_piece[piece_turn]
    std::vector<hipEvent_t> ev_batch;                  // per table: behind the last piece of the batch that has it
};
static ExportDst pipe_export_dst(const jd_dec *d)
{
    const Pipe *P = d->pipe;
    if (!P || !d->res_ll) return ExportDst{ nullptr, nullptr, nullptr, nullptr, 0 };
    return ExportDst{ P->d_vctl, P->d_vresn, P->d_vres, d->models ? P->d_vres_model : nullptr, d->res_cap };
}

static void pipe_free(jd_dec *d);
static void pipe_free_fwd(jd_dec *d) { pipe_free(d); }
static void pipe_free(jd_dec *d)
{
    Pipe *P = d->pipe;
    if (!P) return;
    if (P->d_ll) (void)hipFree(P->d_ll);
    if (P->d_ident) (void)hipFree(P->d_ident);
    if (P->d_vctl) (void)hipFree(P->d_vctl);
    if (P->d_vresn) (void)hipFree(P->d_vresn);
    if (P->d_vres) (void)hipFree(P->d_vres);
    if (P->d_vres_model) (void)hipFree(P->d_vres_model);
    for (hipEvent_t e : P->ev_piece) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : P->ev_batch) if (e) (void)hipEventDestroy(e);
    delete P;
    d->pipe = nullptr;
}

// everything in flight is dropped (the batches concerned are decoded from scratch when their turn comes), the kernel leaves
static void pipe_drain(jd_dec *d)
{
    Pipe *P = d->pipe;
    if (!P || !P->on) return;
    (void)jd_res_stop(d);                                              // (running utterances run out first)
    if (getenv("JD_VERBOSE") && d->res) {                              // development: how busy the slots were
        const double wall_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - P->t_on).count();
        fprintf(stderr, "pipeline: %d slots for %.1f ms, busy %.1f %% of it on %lld frames (%.1f us per frame on the slot's clock)\n", P->n_slots,
                wall_us / 1e3, 100.0 * (double)(d->res->run_ticks / 100) / (wall_us * P->n_slots), P->frames_done,
                P->frames_done ? (double)(d->res->run_ticks / 100) / (double)P->frames_done : 0.0);
    }
    P->on = false; d->pipe_on = false;                                 // (jd_res_stop has synchronised the side stream)
    d->res_ll = nullptr;
    pipe_drain_reset(*P, &d->stream_dirty);                            // (streams left in the middle of an utterance, or failed: dirty)
}

// the results of the slots in EL to their virtual result slots (jd_finish_export_kernel, on the side stream); EL is empty afterwards
static int pipe_export(jd_dec *d, ExportList *EL)
{
    Pipe *P = d->pipe;
    if (EL->n == 0) return JD_OK;
    hipLaunchKernelGGL(jd_finish_export_kernel, dim3((unsigned)EL->n), dim3(64), 0, d->s_gmm, d->d_ctl, d->d_streams, *EL, P->d_vctl, P->d_vresn,
                       P->d_vres, d->res_cap, d->models ? P->d_vres_model : nullptr);
    HIPCHK(hipGetLastError());
    EL->n = 0;
    return JD_OK;
}

// The pump's steps, pipe_announce, pipe_decode and pipe_drain have a twin in tests/pipe_driver.cpp - the same calls into jd_pipe.h in the
// same order, the device replaced by a model - which is what tests/test_pipe_cpu.py holds to the recorded behaviour: a change to the order
// or the arguments of the calls here is made there too.
// The pump, step 1 (jd_pipe.h: pipe_harvest): the reports that are in - a collection, the next frames, or the utterance is through
static int pump_harvest(jd_dec *d)
{
    Pipe *P = d->pipe;
    Resident *R = d->res;
    ExportList EL; EL.n = 0;
    for (int s = 0; s < P->n_slots; ++s) {
        if (!pipe_slot_occupied(*P, s) || !res_harvest(d, s)) continue;
        const ResStream &S = R->stream[s];
        PipeBatch &B = pipe_slot_batch(*P, s);
        const int ui = P->slot_utt[(size_t)s];
        const PipeHarvest h = pipe_harvest(S, B.u[(size_t)ui], pipe_vslot(*P, B, ui), P->chunk, P->decouple);
        if (h.act == PIPE_COLLECT) {
            const int rc = jd_res_collect(d, s);
            if (rc) return rc;
        } else if (h.act == PIPE_NEXT) {
            res_command(R, s, h.T, h.row_slot, false, h.vslot);
            B.n_commands += 1;
        } else {
            if (h.kexport) {
                pipe_harvest_kexport(*P, s);
                if (pipe_export_add(&EL, s, pipe_vslot(*P, B, ui))) { const int rc = pipe_export(d, &EL); if (rc) return rc; }
            }
            pipe_harvest_through(*P, s, h, S.T_done);
            d->pipe_utts_through += 1;
        }
    }
    return pipe_export(d, &EL);
}

// The pump, step 3 (jd_pipe.h: pipe_piece_next): the pieces that are through, then the next ones - each with its event, and behind a
// batch's last piece the event of its table.  The ready numbers this pump call enqueued (steps 1 and 2) are in front of the new piece.
static int pump_score(jd_dec *d)
{
    Pipe *P = d->pipe;
    pipe_pieces_retire(*P, [&](int e) { return hipEventQuery(P->ev_piece[e]) == hipSuccess; });
    for (PipePiece p = pipe_piece_next(*P); p.batch >= 0; p = pipe_piece_next(*P)) {
        const float *feats = P->q[(size_t)p.batch].feats;
        const int rc = launch_gmm(d->am, d->amb, feats + p.feat_row * (size_t)d->am->D, P->d_ident, (int)p.rows, P->d_ll + p.base_row * (size_t)d->am->n_gmm,
                                  d->s_gmm);
        if (rc) return rc;
        HIPCHK(hipEventRecord(P->ev_piece[p.event], d->s_gmm));
        pipe_piece_launched(*P, p); d->pipe_rows_scored += (long long)p.rows;
        if (p.last) HIPCHK(hipEventRecord(P->ev_batch[(size_t)p.table], d->s_gmm));
    }
    return JD_OK;
}

// The pump, step 2 (jd_pipe.h: pipe_refill): free slots take the next queued utterances - new ready numbers where they are needed
// (behind the exports and every scoring launch enqueued so far), then each utterance's first command
static int pump_refill(jd_dec *d)
{
    Pipe *P = d->pipe;
    Resident *R = d->res;
    std::vector<PipeAssign> who;
    std::vector<int> bump;
    pipe_refill(*P, [&](int t) { return hipEventQuery(P->ev_batch[(size_t)t]) == hipSuccess; }, &who);
    if (who.empty()) return JD_OK;
    for (const PipeAssign &a : who) if (a.bump) bump.push_back(a.slot);
    if (!bump.empty()) {
        const int rc = res_bump(d, (int)bump.size(), bump.data());
        if (rc) return rc;
    }
    for (const PipeAssign &a : who) {
        const PipeFirst c = pipe_refill_command(*P, a);
        res_stream_begin(R->stream[a.slot]);
        res_command(R, a.slot, c.T, c.row_slot, true, c.vslot);
        P->q[(size_t)a.batch].n_commands += 1;
    }
    return JD_OK;
}

// slots whose utterance is through -> their results exported, the slots free; free slots -> the next queued utterances
static int pipe_pump(jd_dec *d)
{
    Pipe *P = d->pipe;
    Resident *R = d->res;
    if (R->h_beat) __atomic_fetch_add(R->h_beat, 1u, __ATOMIC_RELAXED);   // (a sign of life: k_resident's `beat`)
    // the kernel has gone by itself: nobody gave it a command for 5 s (a caller that was away between two calls) - seen
    // BEFORE anything is posted to it: the reports are all in, and it comes back like behind jd_dec_quiesce
    if (R->on && res_any_left(R, P->n_slots)) { const int rc = jd_res_stop(d); if (rc) return rc; }
    if (!R->on) {                                                      // (after jd_dec_quiesce: the kernel comes back, the slots go on where they were)
        const int rc = jd_res_start(d, P->n_slots, GMM_ROWS2);
        if (rc) return rc;
    }
    int rc = pump_harvest(d);
    if (!rc) rc = pump_refill(d);
    if (!rc) rc = pump_score(d);
    return rc;
}

// The decoder's work on the device comes to rest: a search kernel of its own that stays on the device (the batch pipeline)
// lets the commands that are running run out (PIPE_CHUNK frames at most) and leaves; nothing that is announced or under
// way is lost - the kernel comes back with the next call and the slots go on where they were.  What a caller needs before
// a device-wide synchronisation (hipDeviceSynchronize, torch.cuda.synchronize) while batches are announced.
extern "C" int jd_dec_quiesce(jd_dec *d)
{
    if (!d) return jd_fail(JD_EINVAL, "jd_dec_quiesce: null");
    if (d->pipe && d->pipe->on && d->res && d->res->on) {
        int rc = check_device(d->device);
        if (rc) return rc;
        rc = jd_res_stop(d);
        if (rc) return rc;
    }
    return JD_OK;
}

// How batches that follow each other share the chip (include/juicer_amd.h).  Whatever is announced or under way under the old
// setting is dropped: results never depend on announcements, the batches concerned are decoded from scratch when their turn comes.
extern "C" int jd_dec_set_pipeline(jd_dec *d, int32_t mode, int32_t depth, int32_t slots)
{
    if (!d) return jd_fail(JD_EINVAL, "jd_dec_set_pipeline: null");
    if (mode != JD_FLOW_SERIAL && mode != JD_FLOW_TWO_IN_FLIGHT && mode != JD_FLOW_RESIDENT)
        return jd_fail(JD_EINVAL, "jd_dec_set_pipeline: mode %d (JD_FLOW_SERIAL, JD_FLOW_TWO_IN_FLIGHT or JD_FLOW_RESIDENT)", mode);
    if (mode == JD_FLOW_RESIDENT) {
        const PipeSetting S = pipe_setting(depth, slots, d->max_streams, d->n_cus, SLOT_WG_PER_CU, d->net->lazy_dev ? true : false, d->am->hybrid ? true : false);
        depth = S.depth; slots = S.slots;
        if (S.verdict == PIPE_SET_DEPTH) return jd_fail(JD_EINVAL, "jd_dec_set_pipeline: depth %d (2..32 batches announced and not handed back)", depth);
        if (S.verdict == PIPE_SET_SLOTS) return jd_fail(JD_EINVAL, "jd_dec_set_pipeline: %d slots, the decoder has %d streams", slots, d->max_streams);
        if (S.verdict == PIPE_SET_DEVICE)
            return jd_fail(JD_EINVAL, "jd_dec_set_pipeline: %d slots, but the device holds %d at once (%d CUs x %d workgroups of the slot kernel); "
                           "one per CU (%d) is what leaves the scoring room beside them", slots, d->n_cus * SLOT_WG_PER_CU, d->n_cus, SLOT_WG_PER_CU, d->n_cus);
        if (S.verdict == PIPE_SET_NOT_WITH)
            return jd_fail(JD_ESTATE, "jd_dec_set_pipeline: JD_FLOW_RESIDENT not with a lazily composed network / hybrid scoring");
    }
    if (d->res && d->res->on && !d->pipe_on) return jd_fail(JD_ESTATE, "jd_dec_set_pipeline: a broker drives this decoder's resident kernel");
    int rc = check_device(d->device);
    if (rc) return rc;
    pipe_drain(d);
    pipe_free(d);
    pf_discard(d);
    d->pipeline = mode != JD_FLOW_SERIAL;
    d->pipe_mode = mode == JD_FLOW_RESIDENT;
    if (d->pipe_mode) { d->pipe_depth = depth; d->pipe_slots = slots; }
    return JD_OK;
}

extern "C" int jd_dec_pipeline_stats(const jd_dec *d, jd_pipe_stats *out)
{
    if (!d || !out) return jd_fail(JD_EINVAL, "jd_dec_pipeline_stats: null");
    memset(out, 0, sizeof *out);
    out->mode = d->pipe_mode ? JD_FLOW_RESIDENT : (d->pipeline ? JD_FLOW_TWO_IN_FLIGHT : JD_FLOW_SERIAL);
    out->depth = d->pipe_mode ? d->pipe_depth : 0;
    out->slots = d->pipe_mode ? (d->pipe ? d->pipe->n_slots : (d->pipe_slots > 0 ? d->pipe_slots : d->max_streams)) : 0;
    out->resident = (d->pipe_on && d->res && d->res->on) ? 1 : 0;
    out->batches_announced = d->pipe ? (int32_t)d->pipe->q.size() : 0;
    out->frames_searched = d->pipe_frames_searched; out->utts_through = d->pipe_utts_through; out->rows_scored = d->pipe_rows_scored;
    out->batches_back = d->pipe_batches_back; out->collections = d->pipe_collections;
    out->slot_busy_us = (double)d->pipe_busy_ticks / 100.0;
    out->on_us = d->pipe_on_us;
    if (out->resident) out->on_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - d->res->t_start).count();
    return JD_OK;
}

// Rows per scoring launch (jd_plan.h: plan_piece_rows, between jd_pipe.h's pipe_piece_bounds): the piece whose last round of
// workgroups is fullest, with what the runtime says of the slot kernel and of the scoring kernel on a CU.  (The kernels of 128-row
// tiles; the others plan nothing: PIPE_PIECE_ROWS0.)
static_assert(PLAN_PIECE_TILE == GMM_ROWS2, "plan_piece_rows counts the scoring kernels' row tiles");
static int pipe_plan_piece(const jd_dec *d, const Pipe *P, size_t *planned)
{
    int occ_gmm = 0, occ_slot = 0;
    const int rc = gmm_tiles128_occupancy(d->am, d->amb, &occ_gmm);
    if (rc) return rc;
    if (occ_gmm <= 0) return JD_OK;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_slot, (const void *)slot_mailbox_kernel(d->am->max_n <= 5, d->models), SNT, 0));
    const int wgs = plan_resident_scoring_wgs(d->n_cus, P->n_slots, occ_slot, occ_gmm);
    const PipePieceBounds b = pipe_piece_bounds(d->am->n_gmm, GMM_GT, GMM_GT_SMALL, GMM_ROWS2);
    *planned = (size_t)plan_piece_rows(b.groups, wgs, b.lo, b.hi);
    if (getenv("JD_VERBOSE"))
        fprintf(stderr, "pipeline: pieces of %zu rows (%d state groups, %d scoring workgroups resident beside %d slots: %d + %d per CU alone)\n",
                *planned, b.groups, wgs, P->n_slots, occ_slot, occ_gmm);
    return JD_OK;
}

// sized (jd_pipe.h: pipe_size, pipe_size_piece), then its events, tables and virtual result slots
static int pipe_fill(jd_dec *d, Pipe *P, int n_utts, size_t rows)
{
    const int G = d->am->n_gmm;
    const PipeSizeIn in{d->pipe_depth, d->pipe_slots, d->max_streams, n_utts, rows, GMM_ROWS2, res_knob("JD_PIPE_CHUNK"), res_knob("JD_PIPE_DECOUPLE")};
    const size_t V = pipe_size(*P, in);
    size_t planned = 0;
    if (P->decouple) { const int rc = pipe_plan_piece(d, P, &planned); if (rc) return rc; }
    const int piece_knob = res_knob("JD_PIPE_PIECE");
    P->piece_rows = pipe_size_piece(planned, piece_knob, GMM_ROWS2);
    if (getenv("JD_VERBOSE"))
        fprintf(stderr, "pipe: size depth %d slots %d streams %d utts %d rows %zu tile %d chunk %d decouple %d planned %zu piece %d -> K %d max_batch %d "
                "n_slots %d chunk %d decouple %d max_out %d piece_rows %zu table_rows %zu vslots %zu\n", in.depth, in.pipe_slots, in.max_streams, in.n_utts,
                in.rows, in.tile, in.chunk_knob, in.decouple_knob, planned, piece_knob, P->K, P->max_batch, P->n_slots, P->chunk, (int)P->decouple,
                P->max_out, P->piece_rows, P->table_rows, V);
    P->ev_batch.assign((size_t)P->K, nullptr);
    for (hipEvent_t &e : P->ev_piece) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return jd_fail(JD_EHIP, "hipEventCreate failed");
    for (hipEvent_t &e : P->ev_batch) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return jd_fail(JD_EHIP, "hipEventCreate failed");
    if (hipMalloc(&P->d_ll, (size_t)P->K * P->table_rows * G * sizeof(float)) != hipSuccess ||
        hipMalloc(&P->d_ident, P->table_rows * sizeof(int)) != hipSuccess ||
        hipMalloc(&P->d_vctl, V * sizeof(StreamCtl)) != hipSuccess || hipMalloc(&P->d_vresn, V * sizeof(int)) != hipSuccess ||
        hipMalloc(&P->d_vres, V * 5 * (size_t)d->res_cap * sizeof(int)) != hipSuccess ||
        (d->models && hipMalloc(&P->d_vres_model, V * (size_t)d->res_cap * sizeof(int)) != hipSuccess)) {
        (void)hipGetLastError();
        return jd_fail(JD_ENOMEM, "jd_dec_prefetch_scores: no memory for %d likelihood tables of %zu rows", d->pipe_depth, rows);
    }
    std::vector<int> ident(P->table_rows);
    for (size_t r = 0; r < P->table_rows; ++r) ident[r] = (int)r;
    HIPCHK(hipMemcpy(P->d_ident, ident.data(), ident.size() * sizeof(int), hipMemcpyHostToDevice));
    return JD_OK;
}

// d->pipe for batches like this one (n_utts utterances, `rows` frames): the whole of it, or none (and the code)
static int pipe_alloc(jd_dec *d, int n_utts, size_t rows)
{
    d->pipe = new Pipe();
    const int rc = pipe_fill(d, d->pipe, n_utts, rows);
    if (rc) pipe_free(d);
    return rc;
}

// jd_dec_prefetch_scores in pipe mode: 1 = taken, 0 = not this way (the caller goes on with the usual announcement)
static int pipe_announce(jd_dec *d, int n_utts, const float *d_feats, const int64_t *offs, int *taken)
{
    *taken = 0;
    if (!pipe_takes(d->pipe_mode, d->net->lazy_dev ? true : false, d->partial_interval > 0, d->am->hybrid ? true : false, n_utts)) return JD_OK;
    const size_t rows = (size_t)(offs[n_utts] - offs[0]);
    if (d->pipe && pipe_outgrown(*d->pipe, n_utts, rows)) {            // a larger batch than the tables were made for: the pipeline starts again
        pipe_drain(d);
        pipe_free(d);
    }
    int rc = check_device(d->device);
    if (rc) return rc;
    if (!d->pipe) {
        rc = ensure_arenas(d);
        if (rc) return rc;
        if (d->res && d->res->on) return JD_OK;                        // (a broker owns the resident kernel)
        rc = pipe_alloc(d, n_utts, rows);
        if (rc) return rc;
    }
    Pipe *P = d->pipe;
    if (pipe_full(*P))
        return jd_fail(JD_ESTATE, "jd_dec_prefetch_scores: %d batches are announced and not decoded - the pipeline is %d deep (JD_PIPE_DEPTH)",
                       (int)P->q.size(), P->K);
    if (!P->on) {
        pf_discard(d);                                                 // (what the other way of working ahead holds)
        for (int s = 0; s < P->n_slots; ++s)
            if (d->stream_dirty[(size_t)s]) { rc = wipe_stream(d, s); if (rc) return rc; }
        d->res_ll = P->d_ll;
        rc = jd_res_start(d, P->n_slots, GMM_ROWS2);
        if (rc) { d->res_ll = nullptr; return rc; }
        P->on = true; d->pipe_on = true;
        pipe_started(*P); P->t_on = std::chrono::steady_clock::now(); d->res->run_ticks = 0;
    }
    const bool verbose = getenv("JD_VERBOSE") != nullptr;
    const std::string used = verbose ? pipe_list(P->K, [&](int t) { return P->table_used[(size_t)t]; }) : std::string();
    const PipeBatch &B = pipe_enqueue(*P, d_feats, n_utts, offs);
    if (verbose)
        fprintf(stderr, "pipe: announce K %d table_rows %zu used %s T %s -> table %d row0 %s order %s\n", P->K, P->table_rows, used.c_str(),
                pipe_list(B.n, [&](int u) { return B.u[(size_t)u].T; }).c_str(), B.table, pipe_list(B.n, [&](int u) { return B.u[(size_t)u].row0; }).c_str(),
                pipe_list(B.n, [&](int k) { return B.order[(size_t)k]; }).c_str());
    *taken = 1;
    return pipe_pump(d);
}

// jd_decode_batch_device in pipe mode: 1 = handled (the oldest announced batch, handed back), 0 = not this way
static int pipe_decode(jd_dec *d, int n_utts, const float *d_feats, const int64_t *offs, jd_hyp *out, int *handled)
{
    *handled = 0;
    Pipe *P = d->pipe;
    if (!P || !P->on || P->q.empty()) return JD_OK;
    if (!pipe_is_head(*P, d_feats, n_utts, offs)) { pipe_drain(d); return JD_OK; }   // not the announced one: as if nothing had been announced
    const auto w0 = std::chrono::steady_clock::now();
    PipeWatch W;
    for (;;) {
        const int rc = pipe_pump(d);
        if (rc) { pipe_drain(d); return rc; }
        if (pipe_head_done(*P)) break;
        if (pipe_watch_stuck(W, P->frames_done, std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - w0).count())) {
            pipe_drain(d);
            return jd_fail(JD_EHIP, "the batch pipeline has not finished an utterance for 30 s");
        }
        if (d->res->on && res_any_left(d->res, P->n_slots)) {
            // the kernel has gone by itself: nobody gave it a command for 5 s (a caller that was away between two calls) - the
            // reports are taken and it comes back like behind jd_dec_quiesce; a command that was never answered is a lost workgroup
            const int rs = jd_res_stop(d);
            if (rs || pipe_watch_gives_up(W)) {
                pipe_drain(d);
                return rs ? rs : jd_fail(JD_EHIP, "the resident search kernel keeps ending under a batch");
            }
            continue;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    const PipeBatch &F = P->q.front();
    if (pipe_head_needs_sync(*P)) HIPCHK(hipStreamSynchronize(d->s_gmm));      // (the kernel's exports)
    std::vector<int> slot_of;
    pipe_head_slots(*P, &slot_of);
    if ((size_t)n_utts > d->results.size()) d->results.resize((size_t)n_utts);
    d->timing = jd_timing();
    const int rc = fetch_results_from(d, P->d_vctl, P->d_vresn, P->d_vres, slot_of.data(), pipe_vslot(*P, F, 0), n_utts, out, 0, nullptr,
                                      P->d_vres_model);
    for (int u = 0; u < n_utts; ++u) d->timing.search_frames += F.u[(size_t)u].T;
    d->timing.gmm_frames = d->timing.search_frames; d->timing.gmm_states = d->am->n_gmm;
    d->timing.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    d->timing.search_ms = d->timing.total_ms; d->timing.search_launches = 0; d->timing.cluster_wgs = 1; d->timing.prefetched = 1;
    d->load_sum = d->load_frames = 0.0;
    if (getenv("JD_VERBOSE"))
        fprintf(stderr, "pipe: back serial %lld table %d utts %d commands %d pieces %d -> %d\n", P->serial0, F.table, F.n, F.n_commands, F.n_pieces, rc);
    d->pipe_batches_back += 1;
    if (pipe_pop(*P)) pipe_drain(d);                                   // nothing announced behind it: the kernel leaves the device
    *handled = 1;
    return rc;
}

// ------------------------------------------------------------------------------------------------------------------
// Setters that drop what the pipeline holds (they are here for pipe_drain / pipe_free; nothing else of them is about the
// resident kernel): the output level and its results, the way the likelihood tables are scored.
// What a decode returns (include/juicer_amd.h): words, or words and the model-level chain.  The search kernels come in a flavour
// for each (MDL): the resident pipeline's kernel leaves, and whatever is announced under the old setting is dropped.
extern "C" int jd_dec_set_output_level(jd_dec *d, int32_t level)
{
    if (!d) return jd_fail(JD_EINVAL, "jd_dec_set_output_level: null");
    if (level != JD_OUTPUT_WORDS && level != (JD_OUTPUT_WORDS | JD_OUTPUT_MODELS))
        return jd_fail(JD_EINVAL, "jd_dec_set_output_level: level %d (JD_OUTPUT_WORDS or JD_OUTPUT_WORDS | JD_OUTPUT_MODELS)", level);
    const bool m = (level & JD_OUTPUT_MODELS) != 0;
    if (m == d->models) return JD_OK;
    if (d->res && d->res->on && !d->pipe_on) return jd_fail(JD_ESTATE, "jd_dec_set_output_level: a broker drives this decoder's resident kernel");
    if (m && d->partial_interval > 0)
        return jd_fail(JD_EINVAL, "jd_dec_set_output_level: partial traces (jd_dec_set_partial_interval) are not available with model-level output");
    // (an utterance under way keeps the records of the level it began with: its result would mix the two)
    for (int s = 0; s < d->max_streams; ++s)
        if (d->push[(size_t)s].started && d->push[(size_t)s].open)
            return jd_fail(JD_ESTATE, "jd_dec_set_output_level: stream %d has an utterance under way (frames pushed since its jd_stream_init, "
                           "no jd_stream_finish yet) - between utterances only", s);
    int rc = check_device(d->device);
    if (rc) return rc;
    pipe_drain(d);
    pipe_free(d);                                                      // (its result slots are sized for the level)
    pf_discard(d);
    if (m && d->arenas_ready && !d->d_res_model) {
        rc = dmalloc(d, &d->d_res_model, (size_t)d->max_streams * d->res_cap);
        if (rc) return rc;
    }
    if (m && d->arenas_ready && !d->d_partial_model) {
        rc = dmalloc(d, &d->d_partial_model, (size_t)6 * d->res_cap);
        if (rc) return rc;
    }
    d->models = m;
    d->occupancy_ok = false;                                           // (asked again for the flavours it now launches)
    for (HostResult &R : d->results) R.m_n = -1;
    return JD_OK;
}

extern "C" int jd_dec_get_output_level(const jd_dec *d, int32_t *level)
{
    if (!d || !level) return jd_fail(JD_EINVAL, "jd_dec_get_output_level: null");
    *level = JD_OUTPUT_WORDS | (d->models ? JD_OUTPUT_MODELS : 0);
    return JD_OK;
}

extern "C" int jd_dec_model_result(jd_dec *d, int32_t i, jd_model_hyp *out)
{
    if (!d || !out || i < 0 || (size_t)i >= d->results.size()) return jd_fail(JD_EINVAL, "jd_dec_model_result: bad argument");
    if (!d->models) return jd_fail(JD_ESTATE, "jd_dec_model_result: the decoder's output level is JD_OUTPUT_WORDS");
    const HostResult &R = d->results[(size_t)i];
    memset(out, 0, sizeof *out);
    out->n = R.m_n;
    out->model = R.m_model.data(); out->label = R.m_label.data(); out->time = R.m_time.data();
    out->score = R.m_score.data(); out->ac = R.m_ac.data(); out->lm = R.m_lm.data();
    out->tot_score = R.m_tot[0]; out->tot_ac = R.m_tot[1]; out->tot_lm = R.m_tot[2];
    return JD_OK;
}

// How the likelihood tables are scored (include/juicer_amd.h).  Whatever was scored or announced under the other setting is dropped.
extern "C" int jd_dec_set_scoring(jd_dec *d, int32_t mode)
{
    if (!d) return jd_fail(JD_EINVAL, "jd_dec_set_scoring: null");
    if (mode != JD_SCORE_EXACT && mode != JD_SCORE_FAST) return jd_fail(JD_EINVAL, "jd_dec_set_scoring: mode %d (JD_SCORE_EXACT or JD_SCORE_FAST)", mode);
    if (mode == JD_SCORE_FAST && d->am->hybrid)                        // (today's text: GMM models of every D are served since)
        return jd_fail(JD_EINVAL, "jd_dec_set_scoring: JD_SCORE_FAST serves 39-dimensional GMM models (this decoder's: D = %d%s)", d->am->D,
                       ", hybrid");
    if (d->res && d->res->on && !d->pipe_on) return jd_fail(JD_ESTATE, "jd_dec_set_scoring: a broker drives this decoder's resident kernel");
    int rc = check_device(d->device);
    if (rc) return rc;
    if ((d->amb.fast != 0) == (mode == JD_SCORE_FAST)) return JD_OK;
    pipe_drain(d);
    pf_discard(d);
    if (mode == JD_SCORE_FAST) { rc = upload_am_fast(d->am, d->amb); if (rc) return rc; }
    d->amb.fast = mode == JD_SCORE_FAST ? 1 : 0;
    return JD_OK;
}
