// arena_driver.cpp - runs arena_caps / arena_layout and wave_layout (juicer_amd/csrc/jd_arena.h) over cases read from stdin, for
// tests/test_arena_cpu.py and tests/test_gpu_arena_inputs.py.  Input: the number of cases, then per case one of
//   caps free_bytes cached_bytes mem_fraction B n_arcs n_states Fc n_gmm max_n cap_slots cap_items cap_paths slots_hint
//        rec_bytes_small rec_bytes_large path_rec tok item state_rec gc_words tot_n maxw hist_bins sw
//   wave nb free_bytes ll_cap G fc_env tile ustart[nb] ulen[nb]
// (mem_fraction: whatever strtod reads - the golden's are hex floats).  Output, one line of integers per case:
//   caps: status passes cap_slots cap_items cap_paths cap_new gc_threshold bytes_per_stream off[AR_N], and when the status is not 0 the
//         two addressing limits behind them (everything from cap_new to off[] is 0 then)
//   wave: code utt, and when the code is 0:  nb Fc n_chunks maxT max_rows n_rows_all T[nb] chunk_row0[n_chunks + 1] row_off[n_chunks * nb]
//         chunk_rows[n_chunks] row_src[n_rows_all]   (utt: the utterance of a bad length, else -1)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "jd_arena.h"

static bool rd(long long *v) { return scanf("%lld", v) == 1; }
static bool rdu(unsigned long long *v) { return scanf("%llu", v) == 1; }

static int run_caps()
{
    unsigned long long free_b, cached_b;
    char frac[64];
    long long v[21];
    if (!rdu(&free_b) || !rdu(&cached_b) || scanf("%63s", frac) != 1) return 2;
    for (long long &x : v) if (!rd(&x)) return 2;
    ArenaIn in;
    in.free_bytes = (size_t)free_b; in.cached_bytes = (size_t)cached_b; in.mem_fraction = strtod(frac, nullptr);
    in.B = (int)v[0]; in.n_arcs = v[1]; in.n_states = v[2]; in.Fc = (int)v[3]; in.n_gmm = (int)v[4]; in.max_n = (int)v[5];
    in.cap_slots = v[6]; in.cap_items = v[7]; in.cap_paths = v[8]; in.slots_hint = v[9];
    in.z = ArenaSizes{v[10], v[11], (size_t)v[12], (size_t)v[13], (size_t)v[14], (size_t)v[15], (int)v[16], (int)v[17], (int)v[18], (int)v[19], (int)v[20]};
    if (in.B < 1) return 2;
    ArenaCaps caps;
    arena_caps(in, &caps);
    size_t off[AR_N] = {0}, bytes = 0;
    if (caps.status == ARENA_OK)
        bytes = arena_layout(ArenaDims{caps.cap_slots, caps.cap_items, caps.cap_paths, caps.cap_new, in.n_arcs, in.n_states, in.max_n, in.z}, off);
    printf("%d %d %lld %lld %lld %lld %lld %zu", (int)caps.status, caps.passes, (long long)caps.cap_slots, (long long)caps.cap_items,
           (long long)caps.cap_paths, (long long)caps.cap_new, (long long)caps.gc_threshold, bytes);
    for (size_t o : off) printf(" %zu", o);
    if (caps.status != ARENA_OK) printf(" %lld %lld", (long long)caps.lim_rec, (long long)caps.lim_item);
    printf("\n");
    return 0;
}

static int run_wave()
{
    long long nb, G, fc_env, tile;
    unsigned long long free_b, ll_cap;
    if (!rd(&nb) || !rdu(&free_b) || !rdu(&ll_cap) || !rd(&G) || !rd(&fc_env) || !rd(&tile) || nb < 0) return 2;
    std::vector<int64_t> ustart((size_t)nb), ulen((size_t)nb);
    for (int64_t &x : ustart) { long long t; if (!rd(&t)) return 2; x = t; }
    for (int64_t &x : ulen) { long long t; if (!rd(&t)) return 2; x = t; }
    WavePlan P;
    const WaveStatus st = wave_layout(WaveIn{(int)nb, ustart.data(), ulen.data(), (size_t)free_b, (size_t)ll_cap, (int)G, (int)fc_env, (int)tile}, &P);
    printf("%d %d", (int)st.code, st.utt);
    if (st.code == WAVE_OK) {
        printf(" %d %d %d %d %zu %zu", P.nb, P.Fc, P.n_chunks, P.maxT, P.max_rows, P.n_rows_all);
        for (int x : P.T) printf(" %d", x);
        for (size_t x : P.chunk_row0) printf(" %zu", x);
        for (int x : P.row_off) printf(" %d", x);
        for (int x : P.chunk_rows) printf(" %d", x);
        for (int x : P.row_src) printf(" %d", x);
    }
    printf("\n");
    return 0;
}

int main()
{
    long long n_cases = 0;
    if (!rd(&n_cases)) return 2;
    for (long long c = 0; c < n_cases; ++c) {
        char kind[16];
        if (scanf("%15s", kind) != 1) return 2;
        const int rc = !strcmp(kind, "caps") ? run_caps() : !strcmp(kind, "wave") ? run_wave() : 2;
        if (rc) return rc;
    }
    return 0;
}
