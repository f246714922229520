// prep_driver.cpp - runs the graph and model preparation of jd_dec_create (juicer_amd/csrc/jd_prep.h) over cases read from stdin, in
// jd_dec_create's order, for tests/test_prep_cpu.py.  Floats travel as the decimal value of their 32 bits.
// Input:  n_nets, then per network   n_states init n_arcs | row_ptr[n_states + 1] | n_arcs x {to w in out} | fin_w[n_states]
//         n_ams, then per model set  n_hmm max_n n_tm | hmm_n[n_hmm] | hmm_tm[n_hmm] | hmm_tee[n_hmm] | hmm_gmm[n_hmm * max_n] | tm_n[n_tm] |
//                                    trP[n_tm * max_n * max_n] | se[n_tm * max_n * 2]
//         n_cases, then per case     net am renumber xsort sole xcut srec_split no_lr main_beam max_hyps      (knobs: -1 unset)
// Output: a line "consts ..." with the build's constants, then per case one line of name=value pairs: every scalar, and sha256_NAME of
// each array's raw little-endian bytes.  With the argument "arrays" every array follows its case's line in full: "NAME n v v v ...".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "jd_prep.h"

static bool rd(long long *v) { return scanf("%lld", v) == 1; }
static long long need()
{
    long long v = 0;
    if (!rd(&v)) { fprintf(stderr, "prep_driver: short input\n"); exit(2); }
    return v;
}
static float need_f()
{
    const uint32_t u = (uint32_t)need();
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// SHA-256 (FIPS 180-4), of a byte string held in memory
static std::string sha256(const void *data, size_t n)
{
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
        0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
        0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
        0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
        0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
        0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    std::vector<unsigned char> m((const unsigned char *)data, (const unsigned char *)data + n);
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    for (int i = 7; i >= 0; --i) m.push_back((unsigned char)(((unsigned long long)n * 8) >> (8 * i)));
    auto rotr = [](uint32_t x, int r) { return (x >> r) | (x << (32 - r)); };
    for (size_t off = 0; off < m.size(); off += 64) {
        uint32_t w[64];
        for (int i = 0; i < 16; ++i)
            w[i] = (uint32_t)m[off + 4 * i] << 24 | (uint32_t)m[off + 4 * i + 1] << 16 | (uint32_t)m[off + 4 * i + 2] << 8 | (uint32_t)m[off + 4 * i + 3];
        for (int i = 16; i < 64; ++i)
            w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; ++i) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    char out[65];
    for (int i = 0; i < 8; ++i) snprintf(out + 8 * i, 9, "%08x", h[i]);
    return out;
}

// what one case comes to: scalars in the order they are printed, arrays as 32-bit words
struct Out {
    std::vector<std::pair<const char *, long long>> scalars;
    std::vector<std::pair<const char *, std::vector<uint32_t>>> arrays;
    template <typename T> void array(const char *name, const std::vector<T> &v)
    {
        static_assert(sizeof(T) % 4 == 0, "whole words");
        std::vector<uint32_t> w(v.size() * (sizeof(T) / 4));
        if (!w.empty()) memcpy(w.data(), v.data(), w.size() * 4);
        arrays.push_back({name, std::move(w)});
    }
};

// jd_dec_create's preparation, in its order (jd_device.hip: jd_dec_create, dec_upload_graph; jd_host_stream.h: jd_dec_set_partial_interval)
static Out run_case(const jd_net &net, const jd_am &am, const PrepKnobs &knobs, float main_beam, int max_hyps)
{
    Out o;
    const PrepHist H = prep_hist(main_beam, max_hyps);
    const PrepModels M = prep_models(am, knobs);
    PrepNumbering N = prep_renumber(net, knobs.renumber);
    const std::vector<int32_t> &row_ptr = N.state_new.empty() ? net.row_ptr : N.row_ptr;
    const std::vector<JdArc> &arcs = N.state_new.empty() ? net.arcs : N.arcs;
    const PrepArcs A = prep_arcs(row_ptr, arcs, net.n_states, am, M.tmax0, knobs);
    const PrepSrec S = prep_srec_layout(row_ptr, arcs, net.n_states, net.n_arcs, knobs.srec_split);
    const std::vector<float> fin_w = N.state_new.empty() ? net.fin_w : permute_by_state(N.state_new, net.fin_w);
    std::vector<int> pcount;
    const bool acyclic = closure_path_counts(&net, &am, pcount);
    if (!N.state_new.empty()) pcount = permute_by_state(N.state_new, pcount);
    o.scalars = {{"n_next_net", N.n_next_net}, {"renumber_tried", N.tried}, {"renumber_same", N.same}, {"renumbered", !N.state_new.empty()},
                 {"init_state", N.state_new.empty() ? net.init : N.state_new[(size_t)net.init]},
                 {"n_sole", A.n_sole}, {"n_model", A.n_model}, {"n_sorted", A.n_sorted}, {"n_model_all", A.n_model_all}, {"xcut", A.xcut},
                 {"srec_stride", S.stride}, {"srec_arr", S.arr}, {"srec_estride", S.estride}, {"srec_par", S.par}, {"split", S.split}, {"n_next", S.n_next},
                 {"AI", M.AI}, {"all_lr", !M.lrt.empty()}, {"hist_min", H.hist_min}, {"hist_max", H.hist_max}, {"hist_nbins", H.hist_nbins},
                 {"acyclic", acyclic}};
    o.array("state_new", N.state_new);
    o.array("row_ptr", row_ptr);
    o.array("arcs", A.arcs);
    o.array("xst", A.xst);
    o.array("fin_w", fin_w);
    o.array("tmax0", M.tmax0);
    o.array("se32", M.se32);
    o.array("aux", M.aux);
    o.array("lrt", M.lrt);
    o.array("pcount", pcount);
    return o;
}

int main(int argc, char **argv)
{
    const bool arrays = argc > 1 && strcmp(argv[1], "arrays") == 0;
    std::vector<std::unique_ptr<jd_net>> nets((size_t)need());
    for (auto &pn : nets) {
        pn.reset(new jd_net());
        jd_net &n = *pn;
        n.n_states = (int)need(); n.init = (int)need(); n.n_arcs = need();
        n.row_ptr.resize((size_t)n.n_states + 1);
        for (int32_t &x : n.row_ptr) x = (int32_t)need();
        n.arcs.resize((size_t)n.n_arcs);
        for (JdArc &a : n.arcs) { a.to = (int)need(); a.w = need_f(); a.in = (int)need(); a.out = (int)need(); n.max_in = std::max(n.max_in, a.in); }
        n.fin_w.resize((size_t)n.n_states);
        for (float &x : n.fin_w) x = need_f();
        bool ok = n.init >= 0 && n.init < n.n_states && n.row_ptr[0] == 0 && n.row_ptr.back() == n.n_arcs;
        for (int q = 0; q < n.n_states && ok; ++q) ok = n.row_ptr[(size_t)q] <= n.row_ptr[(size_t)q + 1];
        for (const JdArc &a : n.arcs) ok = ok && a.to >= 0 && a.to < n.n_states && a.in >= 0;
        if (!ok) { fprintf(stderr, "prep_driver: bad network\n"); return 2; }
    }
    std::vector<jd_am> ams((size_t)need());
    for (jd_am &a : ams) {
        a.n_hmm = (int)need(); a.max_n = (int)need(); a.n_tm = (int)need();
        if (a.n_hmm < 1 || a.max_n < 1 || a.max_n > JD_MAXN || a.n_tm < 1) { fprintf(stderr, "prep_driver: bad model set\n"); return 2; }
        a.hmm_n.resize((size_t)a.n_hmm); a.hmm_tm.resize((size_t)a.n_hmm); a.hmm_tee.resize((size_t)a.n_hmm);
        a.hmm_gmm.resize((size_t)a.n_hmm * a.max_n); a.tm_n.resize((size_t)a.n_tm);
        a.trP.resize((size_t)a.n_tm * a.max_n * a.max_n); a.se.resize((size_t)a.n_tm * a.max_n * 2);
        for (int32_t &x : a.hmm_n) { x = (int32_t)need(); if (x < 0 || x > a.max_n) return 2; }
        for (int32_t &x : a.hmm_tm) { x = (int32_t)need(); if (x < 0 || x >= a.n_tm) return 2; }
        for (float &x : a.hmm_tee) x = need_f();
        for (int32_t &x : a.hmm_gmm) x = (int32_t)need();
        for (int32_t &x : a.tm_n) { x = (int32_t)need(); if (x < 0 || x > a.max_n) return 2; }
        for (float &x : a.trP) x = need_f();
        for (int16_t &x : a.se) x = (int16_t)need();
    }
    printf("consts XSORT_MAX_ROW=%d XNCAND=%d TRP_LDS_MAX=%d JD_MAXN=%d\n", XSORT_MAX_ROW, XNCAND, TRP_LDS_MAX, JD_MAXN);
    const long long n_cases = need();
    for (long long c = 0; c < n_cases; ++c) {
        const long long ni = need(), ai = need();
        PrepKnobs k;
        k.renumber = (int)need(); k.xsort = (int)need(); k.sole = (int)need(); k.xcut = (int)need(); k.srec_split = (int)need(); k.no_lr = (int)need();
        const float main_beam = need_f();
        const int max_hyps = (int)need();
        if (ni < 0 || ni >= (long long)nets.size() || ai < 0 || ai >= (long long)ams.size() || nets[(size_t)ni]->max_in > ams[(size_t)ai].n_hmm) {
            fprintf(stderr, "prep_driver: bad case\n");
            return 2;
        }
        const Out o = run_case(*nets[(size_t)ni], ams[(size_t)ai], k, main_beam, max_hyps);
        for (const auto &s : o.scalars) printf("%s=%lld ", s.first, s.second);
        for (const auto &a : o.arrays) printf("sha256_%s=%s ", a.first, sha256(a.second.data(), a.second.size() * 4).c_str());
        printf("\n");
        if (arrays)
            for (const auto &a : o.arrays) {
                printf("%s %zu", a.first, a.second.size());
                for (uint32_t w : a.second) printf(" %u", w);
                printf("\n");
            }
    }
    return 0;
}
