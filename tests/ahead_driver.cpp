// ahead_driver.cpp - runs the decisions of working ahead (juicer_amd/csrc/jd_ahead.h) over lines read from stdin, for
// tests/test_ahead_cpu.py and tests/test_gpu_ahead_inputs.py: one line in, one line of integers out (tests/ahead_cases.py writes the
// lines and names the columns).  Doubles are read with strtod (the golden's are hex floats) and printed as their 64 bits.
//
// Single decisions: free_table wants rows any announce_one claim place need take chunk probe bg clip reserve hold waves load wave.
// Scripts: `reset` makes a model decoder - the queue, fg_buf, ll_cap - and `announce`, `announce-none`, `decode` are what
// jd_dec_prefetch_scores and jd_decode_batch_device do to it, every HIP call replaced by what the line says the device reported:
//   decode feats n_utts ulen[n_utts] can_launch table_ready can_grow n_heads {frame error}[n_heads]
// can_launch: how many scorings pf_launch gets enqueued per launch; table_ready: the head's table is there when pf_background asks;
// can_grow: ensure_slab succeeds; heads: of every stream, as read_heads would find them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <sstream>

#include "jd_ahead.h"

struct I2 { int x, y; };
struct Head { int frame, error; };
typedef std::deque<AheadEntry> Queue;
static const float g_feats[8] = {0};                                  // feature buffers are told apart by address: &g_feats[id]

struct In {
    std::istringstream s;
    long long i() { long long v = 0; if (!(s >> v)) { fprintf(stderr, "ahead_driver: short line\n"); exit(2); } return v; }
    double f() { std::string t; if (!(s >> t)) { fprintf(stderr, "ahead_driver: short line\n"); exit(2); } return strtod(t.c_str(), nullptr); }
    std::vector<int64_t> vec(int n) { std::vector<int64_t> v((size_t)n); for (int64_t &x : v) x = i(); return v; }
};
static void out_bits(double v) { unsigned long long b; memcpy(&b, &v, sizeof b); printf(" %llu", b); }
static WavePlan layout(int nb, const int64_t *ustart, const int64_t *ulen, size_t ll_cap, int G, int fc_env, int tile)
{
    WavePlan P;
    if (wave_layout(WaveIn{nb, ustart, ulen, (size_t)1 << 40, ll_cap, G, fc_env, tile}, &P).code != WAVE_OK) { fprintf(stderr, "ahead_driver: bad wave\n"); exit(2); }
    return P;
}
static std::vector<int64_t> starts(const std::vector<int64_t> &ulen)
{
    std::vector<int64_t> s(ulen.size(), 0);
    for (size_t u = 1; u < ulen.size(); ++u) s[u] = s[u - 1] + ulen[u - 1];
    return s;
}
static void print_items(const std::vector<I2> &work, const std::vector<double> &w)
{
    printf(" %zu", work.size());
    for (size_t k = 0; k < work.size(); ++k) printf(" %d %d %lld", work[k].x, work[k].y, (long long)w[k]);
}

// ---- single decisions
static void run_queue_predicate(const std::string &cmd, In &in)
{
    // free_table fg n {state buf} | wants fg G ll_cap n {state buf max_rows} | rows n {state rows} | any n {state bank}
    const int fg = (cmd == "free_table" || cmd == "wants") ? (int)in.i() : 0;
    const size_t G = cmd == "wants" ? (size_t)in.i() : 1, ll_cap = cmd == "wants" ? (size_t)in.i() : 0;
    Queue q((size_t)in.i());
    for (AheadEntry &F : q) {
        F.state = (AheadState)in.i();
        if (cmd == "any") F.bank = (int)in.i();
        else if (cmd == "rows") F.plan.chunk_rows.assign(1, (int)in.i());
        else F.buf = (int)in.i();
        if (cmd == "wants") F.plan.max_rows = (size_t)in.i();
    }
    if (cmd == "free_table") printf("%d", ahead_free_table(q, fg));
    else if (cmd == "wants") printf("%d", (int)ahead_wants_scoring(q, fg, G, ll_cap));
    else if (cmd == "rows") printf("%lld", (long long)ahead_scoring_rows(q));
    else printf("%d %d %d", (int)ahead_any_scored(q), (int)ahead_any_started(q), (int)ahead_any_worked(q));
}
static void run_announce_one(In &in)
{
    // announce_one max_streams front queued fc_env nb ulen[nb] -> admitted n_chunks enqueued queue_size position (-1: not there)
    const int max_streams = (int)in.i(), front = (int)in.i(), queued = (int)in.i(), fc_env = (int)in.i(), nb = (int)in.i();
    const std::vector<int64_t> ulen = in.vec(std::max(nb, 0)), ustart = starts(ulen);
    Queue q((size_t)queued);
    const bool admitted = ahead_admits(nb, max_streams, q.size());
    int n_chunks = 0, enq = 0, pos = -1;
    if (admitted) {
        AheadEntry F;
        F.ustart = ustart; F.ulen = ulen;
        F.plan = layout(nb, ustart.data(), ulen.data(), 0, 2, fc_env, 128);
        n_chunks = F.plan.n_chunks;
        enq = ahead_enqueue(q, std::move(F), &g_feats[1], nb, front != 0);
        for (size_t k = 0; k < q.size(); ++k) if (q[k].feats == &g_feats[1]) pos = (int)k;
    }
    printf("%d %d %d %zu %d", (int)admitted, n_chunks, enq, q.size(), pos);
}
static void run_claim(In &in)
{
    // claim retry feats nb ustart[nb] ulen[nb] n {state bank feats nb ustart[] ulen[]} -> mine drop
    const int retry = (int)in.i(), feats = (int)in.i(), nb = (int)in.i();
    const std::vector<int64_t> ustart = in.vec(nb), ulen = in.vec(nb);
    Queue q((size_t)in.i());
    for (AheadEntry &F : q) {
        F.state = (AheadState)in.i(); F.bank = (int)in.i(); F.feats = &g_feats[in.i()]; F.nb = (int)in.i();
        F.ustart = in.vec(F.nb); F.ulen = in.vec(F.nb);
    }
    const AheadClaim c = ahead_claim(q, &g_feats[feats], nb, ustart.data(), ulen.data(), retry != 0);
    printf("%d %d", (int)c.mine, (int)c.drop);
}
static void print_place(const AheadPlace &p) { printf("%d %d %d %d %d %d", (int)p.pipe, (int)p.resumed, (int)p.discard, (int)p.unbank, p.bank, p.s0); }
static void run_place(In &in)
{
    // place n_chunks nb max_streams pipeline lazy mine my_bank n {state bank} -> pipe resumed discard unbank bank s0
    const int n_chunks = (int)in.i(), nb = (int)in.i(), max_streams = (int)in.i(), pipeline = (int)in.i(), lazy = (int)in.i(), mine = (int)in.i(),
              my_bank = (int)in.i();
    Queue q((size_t)in.i());
    for (AheadEntry &F : q) { F.state = (AheadState)in.i(); F.bank = (int)in.i(); }
    print_place(ahead_place(q, n_chunks, nb, max_streams, pipeline != 0, lazy != 0, mine != 0, my_bank));
}
static void run_need_take(const std::string &cmd, In &in)
{
    // need max_rows G ll_cap chunked n {max_rows} -> floats drop_scored | take chunked n {state buf} -> table discard
    size_t max_rows = 0, G = 1, ll_cap = 0;
    if (cmd == "need") { max_rows = (size_t)in.i(); G = (size_t)in.i(); ll_cap = (size_t)in.i(); }
    const int chunked = (int)in.i();
    Queue q((size_t)in.i());
    for (AheadEntry &F : q) {
        if (cmd == "need") F.plan.max_rows = (size_t)in.i();
        else { F.state = (AheadState)in.i(); F.buf = (int)in.i(); }
    }
    if (cmd == "need") { const AheadNeed n = ahead_table_need(q, max_rows, G, ll_cap, chunked != 0); printf("%zu %d", n.floats, (int)n.drop_scored); }
    else { const AheadTake t = ahead_table_take(q, chunked != 0); printf("%d %d", t.table, (int)t.discard); }
}
static void run_chunk(const std::string &cmd, In &in)
{
    // chunk c s0 row0 fc_env nb T[nb] frame0[nb] -> frames n {stream row weight}
    // probe load_scale weighted resumed s0 fc_env nb T[nb] -> applies, and when it does: n {stream row probe_weight} n {stream row weight} of the rest
    const double load_scale = cmd == "probe" ? in.f() : 1.0;
    const int weighted = cmd == "probe" ? (int)in.i() : 1, resumed = cmd == "probe" ? (int)in.i() : 0;
    const int c = cmd == "chunk" ? (int)in.i() : 0, s0 = (int)in.i();
    const long long row0 = cmd == "chunk" ? in.i() : 0;
    const int fc_env = (int)in.i(), nb = (int)in.i();
    const std::vector<int64_t> T = in.vec(nb), ustart = starts(T);
    std::vector<int> frame0((size_t)nb, 0);
    if (cmd == "chunk") for (int &f : frame0) f = (int)in.i();
    const WavePlan P = layout(nb, ustart.data(), T.data(), 0, 2, fc_env, 128);
    std::vector<I2> work; std::vector<double> weight;
    const long long frames = ahead_chunk_work(P, c, s0, row0, frame0, &work, &weight);
    if (cmd == "chunk") { printf("%lld", frames); print_items(work, weight); return; }
    const bool applies = ahead_probe_applies(load_scale, weighted != 0, c, P, resumed != 0);
    printf("%d", (int)applies);
    if (!applies) return;
    print_items(work, ahead_probe_weights(weight));
    ahead_probe_rest(P, c, s0, &work, &weight);
    print_items(work, weight);
}
// pf_background on the head of q: the step, and the work it gives (table_ready: what the event wait found)
static AheadBg background(Queue &q, bool pipeline, bool lazy, double load_scale, double bg_max_load, int max_streams, bool table_ready, int fg_bank,
                          size_t rows_per_table, const std::vector<Head> *heads, std::vector<I2> *work, std::vector<double> *left)
{
    work->clear(); left->clear();
    const AheadBg step = ahead_bg_step(q, pipeline, lazy, load_scale, bg_max_load, max_streams);
    if (step == AHEAD_BG_NONE || (step == AHEAD_BG_GO_ON && !heads)) return step;
    AheadEntry &F = q.front();
    if (step == AHEAD_BG_START) {
        if (!table_ready) return step;
        F.bank = fg_bank ^ 1;
        heads = nullptr;
    }
    ahead_bg_work(F, F.bank * (max_streams / 2), (long long)F.buf * (long long)rows_per_table, heads, work, left);
    return step;
}
static void run_bg(In &in)
{
    // bg pipeline lazy load_scale bg_max_load max_streams table_ready fg_bank rows_per_table have_heads n_heads {frame error}
    //    n(0|1) {state bank buf nb n_chunks T[nb]} -> step bank n {stream row left}
    const int pipeline = (int)in.i(), lazy = (int)in.i();
    const double load_scale = in.f(), bg_max_load = in.f();
    const int max_streams = (int)in.i(), ready = (int)in.i(), fg_bank = (int)in.i();
    const size_t rows_per_table = (size_t)in.i();
    const int have_heads = (int)in.i();
    std::vector<Head> heads((size_t)in.i());
    for (Head &h : heads) { h.frame = (int)in.i(); h.error = (int)in.i(); }
    Queue q((size_t)in.i());
    for (AheadEntry &F : q) {
        F.state = (AheadState)in.i(); F.bank = (int)in.i(); F.buf = (int)in.i(); F.nb = (int)in.i();
        const int n_chunks = (int)in.i();
        const std::vector<int64_t> T = in.vec(F.nb), ustart = starts(T);
        F.plan = layout(F.nb, ustart.data(), T.data(), 0, 2, 0, 128);
        F.plan.n_chunks = n_chunks;
    }
    std::vector<I2> work; std::vector<double> left;
    const AheadBg step = background(q, pipeline != 0, lazy != 0, load_scale, bg_max_load, max_streams, ready != 0, fg_bank, rows_per_table,
                                    have_heads ? &heads : nullptr, &work, &left);
    printf("%d %d", (int)step, q.empty() ? -1 : q.front().bank);
    print_items(work, left);
}
static void run_waves(In &in)
{
    // waves max_streams n_utts len[n_utts] -> order[n_utts] n_waves, per wave: nb {ustart ulen}[nb] nn (utterances of the wave announced beside it)
    const int max_streams = (int)in.i(), n_utts = (int)in.i();
    std::vector<int64_t> offs((size_t)n_utts + 1, 0);
    for (int u = 0; u < n_utts; ++u) offs[(size_t)u + 1] = offs[(size_t)u] + in.i();
    const std::vector<int> order = ahead_wave_order(offs.data(), n_utts, max_streams);
    for (int o : order) printf("%d ", o);
    printf("%d", (n_utts + max_streams - 1) / max_streams);
    std::vector<int64_t> ustart((size_t)max_streams), ulen((size_t)max_streams), ns((size_t)max_streams), nl((size_t)max_streams);
    for (int u0 = 0; u0 < n_utts; u0 += max_streams) {
        const int nb = ahead_wave_slice(offs.data(), order, u0, max_streams, ustart.data(), ulen.data());
        printf(" %d", nb);
        for (int k = 0; k < nb; ++k) printf(" %lld %lld", (long long)ustart[(size_t)k], (long long)ulen[(size_t)k]);
        printf(" %d", n_utts > max_streams ? ahead_wave_slice(offs.data(), order, u0 + nb, max_streams, ns.data(), nl.data()) : 0);
    }
}

// ---- what decode_wave decides about one wave, applied to a queue (the order of jd_device.hip's steps)
struct WaveDecisions { AheadClaim claim; AheadPlace place; AheadNeed need; AheadTake take; int b0; AheadEntry me; };
static void discard(Queue &q) { q.clear(); }
static void discard_scored(Queue &q) { for (AheadEntry &F : q) { F.state = AHEAD_ANNOUNCED; F.bank = -1; } }
// before the slab is grown ...
static void decide_before_slab(Queue &q, WaveDecisions &W, const float *feats, int nb, const int64_t *ustart, const int64_t *ulen, bool retry,
                               const WavePlan *plan, int max_streams, bool pipeline, bool lazy, size_t G, size_t ll_cap)
{
    W.need = AheadNeed{0, false}; W.take = AheadTake{0, false};
    W.claim = ahead_claim(q, feats, nb, ustart, ulen, retry);
    if (W.claim.mine) { W.me = std::move(q.front()); q.pop_front(); }
    if (W.claim.drop) discard(q);
    const WavePlan &P = W.claim.mine && !plan ? W.me.plan : *plan;
    W.place = ahead_place(q, P.n_chunks, nb, max_streams, pipeline, lazy, W.claim.mine, W.me.bank);
    if (W.place.discard) discard(q);
    if (W.place.unbank) for (AheadEntry &F : q) F.bank = -1;
    if (W.claim.mine && P.n_chunks == 1) { W.b0 = W.me.buf; return; }
    W.need = ahead_table_need(q, P.max_rows, G, ll_cap, P.n_chunks > 1);
    if (W.need.drop_scored) discard_scored(q);
}
// ... and after it
static void decide_after_slab(Queue &q, WaveDecisions &W, int n_chunks)
{
    if (W.claim.mine && n_chunks == 1) return;
    W.take = ahead_table_take(q, n_chunks > 1);
    if (W.take.discard) discard(q);
    W.b0 = W.take.table;
}
static void print_decisions(const WaveDecisions &W)
{
    printf("%d %d ", (int)W.claim.mine, (int)W.claim.drop);
    print_place(W.place);
    printf(" %zu %d %d %d", W.need.floats, (int)W.need.drop_scored, W.b0, (int)W.take.discard);
}
static void run_wave(In &in)
{
    // wave queue retry nb n_chunks max_rows max_streams pipeline lazy G ll_cap -> mine drop pipe resumed discard unbank bank s0 need drop_scored
    // table none_free.  The inputs of a decoder's "ahead:" line (JD_VERBOSE); queue: "state,buf,bank,nb,max_rows,same;..." or "-"
    std::string desc;
    in.s >> desc;
    const int retry = (int)in.i(), nb = (int)in.i();
    WavePlan P;
    P.n_chunks = (int)in.i(); P.max_rows = (size_t)in.i();
    const int max_streams = (int)in.i(), pipeline = (int)in.i(), lazy = (int)in.i();
    const size_t G = (size_t)in.i(), ll_cap = (size_t)in.i();
    const std::vector<int64_t> zero((size_t)nb, 0);
    Queue q;
    for (char &ch : desc) if (ch == ',' || ch == ';') ch = ' ';
    std::istringstream ds(desc == "-" ? "" : desc);
    for (long long st, buf, bank, n, rows, same; ds >> st >> buf >> bank >> n >> rows >> same;) {
        AheadEntry F;
        F.state = (AheadState)st; F.buf = (int)buf; F.bank = (int)bank; F.nb = (int)n; F.plan.max_rows = (size_t)rows;
        F.feats = &g_feats[same ? 0 : 1];
        F.ustart.assign((size_t)n, 0); F.ulen.assign((size_t)n, 0);
        q.push_back(std::move(F));
    }
    WaveDecisions W{};
    // (a claimed entry's plan is the wave's: the line gives the wave's n_chunks and max_rows either way)
    decide_before_slab(q, W, &g_feats[0], nb, zero.data(), zero.data(), retry != 0, &P, max_streams, pipeline != 0, lazy != 0, G, ll_cap);
    decide_after_slab(q, W, P.n_chunks);
    print_decisions(W);
}

// ---- scripts
struct Model {
    int max_streams = 0, pipeline = 1, lazy = 0, G = 1, tile = 128, nwg_all = 16;
    double load_scale = 1.0, bg_max_load = 4.0;
    size_t ll_cap = 0;
    Queue pf_q;
    int fg_buf = FG_NONE;
    int next_feats = 0;
};
static void print_queue(const Model &m)
{
    printf(" %zu", m.pf_q.size());
    for (const AheadEntry &F : m.pf_q) printf(" %d %d %d %d %d", (int)F.state, F.buf, F.bank, F.nb, (int)(F.feats - g_feats));
}
static void model_announce(Model &m, int nb, const float *feats, const int64_t *ustart, const int64_t *ulen)
{
    if (!ahead_admits(nb, m.max_streams, m.pf_q.size())) return;
    AheadEntry F;
    F.ustart.assign(ustart, ustart + nb); F.ulen.assign(ulen, ulen + nb);
    F.plan = layout(nb, F.ustart.data(), F.ulen.data(), m.ll_cap, m.G, 0, m.tile);
    (void)ahead_enqueue(m.pf_q, std::move(F), feats, nb, false);
}
struct Report { int can_launch, table_ready, can_grow; std::vector<Head> heads; };
// decode_wave: prints  ok mine drop pipe resumed discard unbank bank s0 need drop_scored table none_free n_chunks, per chunk
// n_work frames probe wants bg_step n_bg clipped launched, then gmm_synced; returns false when the slab could not grow
static bool model_wave(Model &m, int nb, const float *feats, const int64_t *ustart, const int64_t *ulen, const Report &r)
{
    WaveDecisions W{};
    WavePlan plan_local;
    const bool mine = ahead_claim(m.pf_q, feats, nb, ustart, ulen, false).mine;
    if (!mine) plan_local = layout(nb, ustart, ulen, m.ll_cap, m.G, 0, m.tile);
    decide_before_slab(m.pf_q, W, feats, nb, ustart, ulen, false, mine ? nullptr : &plan_local, m.max_streams, m.pipeline != 0, m.lazy != 0, (size_t)m.G,
                       m.ll_cap);
    const WavePlan &P = mine ? W.me.plan : plan_local;
    const bool ok = W.need.floats <= m.ll_cap || r.can_grow;
    if (ok && W.need.floats > m.ll_cap) m.ll_cap = (W.need.floats + (size_t)m.G - 1) / (size_t)m.G * (size_t)m.G;
    if (ok) decide_after_slab(m.pf_q, W, P.n_chunks);
    printf(" %d ", (int)ok);
    print_decisions(W);
    printf(" %d", P.n_chunks);
    if (!ok) return false;
    m.fg_buf = P.n_chunks == 1 ? W.b0 : FG_BOTH;
    std::vector<int> frame0((size_t)nb, 0);
    if (W.place.resumed) for (int u = 0; u < nb; ++u) frame0[(size_t)u] = r.heads[(size_t)(W.place.s0 + u)].frame;
    const size_t rows_per_table = m.ll_cap / (size_t)m.G;
    for (int c = 0; c < P.n_chunks; ++c) {
        std::vector<I2> work, bg; std::vector<double> weight, left;
        const long long frames = ahead_chunk_work(P, c, W.place.s0, (long long)(W.b0 ^ (c & 1)) * (long long)rows_per_table, frame0, &work, &weight);
        const bool probe = ahead_probe_applies(m.load_scale, true, c, P, W.place.resumed);
        if (probe) ahead_probe_rest(P, c, W.place.s0, &work, &weight);  // (the probe's own launch is not armed: nothing ahead is touched)
        // launch_search, first round: armed for a single chunk, on the wave's bank
        const bool armed = P.n_chunks == 1;
        const int fg_bank = W.place.pipe ? W.place.bank : -1;
        const bool wants = ahead_wants_scoring(m.pf_q, m.fg_buf, (size_t)m.G, m.ll_cap);
        int step = AHEAD_BG_NONE, clipped = 0, launched = 0;
        if (fg_bank >= 0 && !work.empty()) {
            const bool started = !m.pf_q.empty() && m.pf_q.front().bank >= 0;
            step = background(m.pf_q, m.pipeline != 0, m.lazy != 0, m.load_scale, m.bg_max_load, m.max_streams, r.table_ready != 0, fg_bank, rows_per_table,
                              started ? &r.heads : nullptr, &bg, &left);
            clipped = ahead_bg_clipped((int)bg.size(), (int)work.size(), m.nwg_all);
        }
        if (armed && wants && !work.empty())
            for (AheadEntry &F : m.pf_q) {                             // pf_launch
                if (F.state != AHEAD_ANNOUNCED) continue;
                const int buf = ahead_free_table(m.pf_q, m.fg_buf);
                if (buf < 0 || F.plan.max_rows * (size_t)m.G > m.ll_cap || launched >= r.can_launch) break;
                F.buf = buf; F.state = AHEAD_SCORED; ++launched;
            }
        printf(" %zu %lld %d %d %d %zu %d %d", work.size(), frames, (int)probe, (int)wants, step, bg.size(), clipped, launched);
    }
    printf(" %d", (int)!ahead_any_scored(m.pf_q));
    m.fg_buf = FG_NONE;
    return true;
}
// jd_decode_batch_device: n_waves, per wave {model_wave's line, the queue}
static void model_decode(Model &m, const float *feats, const std::vector<int64_t> &len, const Report &r)
{
    const int n_utts = (int)len.size();
    std::vector<int64_t> offs((size_t)n_utts + 1, 0);
    for (int u = 0; u < n_utts; ++u) offs[(size_t)u + 1] = offs[(size_t)u] + len[(size_t)u];
    const std::vector<int> order = ahead_wave_order(offs.data(), n_utts, m.max_streams);
    std::vector<int64_t> ustart((size_t)m.max_streams), ulen((size_t)m.max_streams), ns((size_t)m.max_streams), nl((size_t)m.max_streams);
    const bool waves = n_utts > m.max_streams;
    Queue callers;
    if (waves) {
        if (ahead_any_worked(m.pf_q)) discard(m.pf_q);
        callers.swap(m.pf_q);
    }
    printf("%d", (n_utts + m.max_streams - 1) / m.max_streams);
    for (int u0 = 0; u0 < n_utts; u0 += m.max_streams) {
        const int nb = ahead_wave_slice(offs.data(), order, u0, m.max_streams, ustart.data(), ulen.data());
        const int nn = waves ? ahead_wave_slice(offs.data(), order, u0 + nb, m.max_streams, ns.data(), nl.data()) : 0;
        if (nn > 0) model_announce(m, nn, feats, ns.data(), nl.data());
        else if (waves) { for (AheadEntry &F : callers) m.pf_q.push_back(std::move(F)); callers.clear(); }
        const bool ok = model_wave(m, nb, feats, ustart.data(), ulen.data(), r);
        if (!ok) { m.fg_buf = FG_NONE; discard(m.pf_q); }               // (the error way out: nothing ahead survives)
        print_queue(m);
        if (!ok) return;
    }
}
static void run_script(const std::string &cmd, In &in, Model &m)
{
    if (cmd == "reset") {
        // reset max_streams pipeline lazy G tile nwg_all load_scale bg_max_load ll_cap
        m = Model();
        m.max_streams = (int)in.i(); m.pipeline = (int)in.i(); m.lazy = (int)in.i(); m.G = (int)in.i(); m.tile = (int)in.i(); m.nwg_all = (int)in.i();
        m.load_scale = in.f(); m.bg_max_load = in.f(); m.ll_cap = (size_t)in.i();
        printf("0");
    } else if (cmd == "announce-none") {
        discard(m.pf_q);
        printf("0");
    } else {
        const float *feats = &g_feats[in.i()];
        const std::vector<int64_t> len = in.vec((int)in.i());
        if (cmd == "announce") {                                       // jd_dec_prefetch_scores
            if ((int)len.size() <= m.max_streams) { const std::vector<int64_t> s = starts(len); model_announce(m, (int)len.size(), feats, s.data(), len.data()); }
            printf("0");
        } else {
            Report r;
            r.can_launch = (int)in.i(); r.table_ready = (int)in.i(); r.can_grow = (int)in.i();
            r.heads.resize((size_t)in.i());
            for (Head &h : r.heads) { h.frame = (int)in.i(); h.error = (int)in.i(); }
            model_decode(m, feats, len, r);
            return;
        }
    }
    print_queue(m);
}

int main()
{
    Model model;
    for (std::string line; std::getline(std::cin, line);) {
        if (line.empty()) continue;
        In in{std::istringstream(line)};
        std::string cmd;
        in.s >> cmd;
        if (cmd == "free_table" || cmd == "wants" || cmd == "rows" || cmd == "any") run_queue_predicate(cmd, in);
        else if (cmd == "announce_one") run_announce_one(in);
        else if (cmd == "claim") run_claim(in);
        else if (cmd == "place") run_place(in);
        else if (cmd == "need" || cmd == "take") run_need_take(cmd, in);
        else if (cmd == "chunk" || cmd == "probe") run_chunk(cmd, in);
        else if (cmd == "bg") run_bg(in);
        else if (cmd == "clip") { const int a = (int)in.i(), b = (int)in.i(), c = (int)in.i(); printf("%d", (int)ahead_bg_clipped(a, b, c)); }
        else if (cmd == "reserve") {
            const int sr = (int)in.i(); const double g = in.f(), l = in.f(), rows = in.f(); const int nwg = (int)in.i();
            printf("%d", ahead_reserve(sr, g, l, rows, nwg));
        } else if (cmd == "hold") {
            const int pr = (int)in.i(); const double g = in.f(), rows = in.f(), s = in.f(), fr = in.f();
            printf("%d", (int)ahead_hold_replan(pr, g, rows, s, fr));
        } else if (cmd == "waves") run_waves(in);
        else if (cmd == "load") { const double a = in.f(), b = in.f(), c = in.f(); printf("0"); out_bits(ahead_load_update(a, b, c)); }
        else if (cmd == "wave") run_wave(in);
        else if (cmd == "reset" || cmd == "announce" || cmd == "announce-none" || cmd == "decode") run_script(cmd, in, model);
        else { fprintf(stderr, "ahead_driver: unknown command %s\n", cmd.c_str()); return 2; }
        printf("\n");
    }
    return 0;
}
