// best_driver.cpp - juicer_amd/csrc/jd_best.h on the CPU (tests/test_best_cpu.py): one decision per input line, integers in, integers
// out (floats travel as their bits).  No HIP, no device: what jd_host_stream.h does between these decisions is copies and one launch.
//   request s                         -> the four words of the stream's request
//   layout M n i                      -> head_at per words reply_words(n) BEST_STAGE_AT(n, i) BEST_HEAD BEST_FIELDS BEST_SHARE
//   reply found n_records res_cap     -> BestReply
//   none frame                        -> the nine words of the head of a stream without a hypothesis
//   check M {started T resident}xM n s_1 .. s_n -> verdict stream |ss| ss.. at..
//   stage n cap l_1 .. l_n            -> a share of the staging area filled by the layout's own index expression (record k: model
//                                        100 + k, label l_k, time 200 + k, score / ac / lm the floats 300 + k, 400 + k, 500 + k),
//                                        taken, then read back with capacity cap: n_models, 6 x min(cap, n) words, n_words, 5 x min(cap, n_words)
//   rows n cap with_models l_1 .. l_n -> the same records through the result arrays [label, time, score, ac, lm][n] (+ the model row)
//   life                              -> a stream's record: |best| and resident after a fill, init(), begin(), taken_over(), init()
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "jd_best.h"

static int32_t fbits(float f) { int32_t v; memcpy(&v, &f, 4); return v; }

static void read_back(const PushModels &M, int cap)
{
    std::vector<int32_t> a((size_t)cap + 1, -7), b(a), c(a);
    std::vector<float> x((size_t)cap + 1, -7.0f), y(x), z(x);
    int32_t n = -1;
    best_models(M, cap, &n, a.data(), b.data(), c.data(), x.data(), y.data(), z.data());
    const int k = cap < n ? cap : n;
    printf("%d", n);
    for (int i = 0; i < k; ++i) printf(" %d", a[(size_t)i]);
    for (int i = 0; i < k; ++i) printf(" %d", b[(size_t)i]);
    for (int i = 0; i < k; ++i) printf(" %d", c[(size_t)i]);
    for (int i = 0; i < k; ++i) printf(" %d", fbits(x[(size_t)i]));
    for (int i = 0; i < k; ++i) printf(" %d", fbits(y[(size_t)i]));
    for (int i = 0; i < k; ++i) printf(" %d", fbits(z[(size_t)i]));
    // (nothing behind the capacity is written)
    if (a[(size_t)cap] != -7 || b[(size_t)cap] != -7 || c[(size_t)cap] != -7 || x[(size_t)cap] != -7.0f || y[(size_t)cap] != -7.0f || z[(size_t)cap] != -7.0f) printf(" OVERRUN");
    std::fill(b.begin(), b.end(), -7); std::fill(c.begin(), c.end(), -7);
    std::fill(x.begin(), x.end(), -7.0f); std::fill(y.begin(), y.end(), -7.0f); std::fill(z.begin(), z.end(), -7.0f);
    int32_t nw = -1;
    best_words(M, cap, &nw, b.data(), c.data(), x.data(), y.data(), z.data());
    const int kw = cap < nw ? cap : nw;
    printf(" %d", nw);
    for (int i = 0; i < kw; ++i) printf(" %d", b[(size_t)i]);
    for (int i = 0; i < kw; ++i) printf(" %d", c[(size_t)i]);
    for (int i = 0; i < kw; ++i) printf(" %d", fbits(x[(size_t)i]));
    for (int i = 0; i < kw; ++i) printf(" %d", fbits(y[(size_t)i]));
    for (int i = 0; i < kw; ++i) printf(" %d", fbits(z[(size_t)i]));
    if (b[(size_t)cap] != -7 || c[(size_t)cap] != -7 || x[(size_t)cap] != -7.0f || y[(size_t)cap] != -7.0f || z[(size_t)cap] != -7.0f) printf(" OVERRUN");
    // ... and every output may be null
    int32_t n2 = -1, nw2 = -1;
    best_models(M, cap, &n2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    best_words(M, cap, &nw2, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (n2 != n || nw2 != nw) printf(" NULLS");
    printf("\n");
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "request") {
            int s; in >> s;
            const BestRequest r = best_request(s);
            int32_t w[4];
            static_assert(sizeof r == sizeof w, "a request is four words");
            memcpy(w, &r, sizeof w);
            printf("%d %d %d %d\n", w[0], w[1], w[2], w[3]);
        } else if (cmd == "layout") {
            int M, n, i; in >> M >> n >> i;
            const BestLayout Y = best_layout(M);
            printf("%zu %zu %zu %zu %zu %d %d %d\n", Y.head_at, Y.per, Y.words, Y.reply_words(n), BEST_STAGE_AT(n, i), BEST_HEAD, BEST_FIELDS, BEST_SHARE);
        } else if (cmd == "reply") {
            int found, n, cap; in >> found >> n >> cap;
            printf("%d\n", (int)best_reply(found, n, cap));
        } else if (cmd == "none") {
            int frame; in >> frame;
            const BestHead h = best_none(frame);
            int32_t w[9];
            memcpy(w, &h, sizeof w);
            for (int k = 0; k < 9; ++k) printf(k ? " %d" : "%d", w[k]);
            printf("\n");
        } else if (cmd == "check") {
            int M; in >> M;
            std::vector<PushStream> S((size_t)M);
            for (PushStream &P : S) in >> P.started >> P.T >> P.resident;
            int n; in >> n;
            std::vector<int32_t> ss((size_t)n);
            for (int32_t &s : ss) in >> s;
            std::vector<int> live, at;
            const BestCheck c = best_check(S, n, ss.data(), &live, &at);
            printf("%d %d %zu", (int)c.verdict, c.stream, live.size());
            for (int s : live) printf(" %d", s);
            for (int a : at) printf(" %d", a);
            printf("\n");
        } else if (cmd == "stage" || cmd == "rows") {
            int n, cap, with_models = 1; in >> n >> cap;
            if (cmd == "rows") in >> with_models;
            std::vector<int32_t> lab((size_t)n);
            for (int32_t &l : lab) in >> l;
            PushModels M;
            M.model.assign(3, 9); M.label.assign(3, 9); M.time.assign(3, 9); M.score.assign(3, 9.0f); M.ac.assign(3, 9.0f); M.lm.assign(3, 9.0f);   // (an older list)
            if (cmd == "stage") {
                // two entries' worth of a reply; the share under test is entry 1's of 2
                std::vector<int32_t> reply(best_layout(2).reply_words(2), -1);
                int32_t *st = reply.data() + BEST_STAGE_AT(2, 1);
                for (int k = 0; k < n; ++k) {
                    st[BEST_STAGE_WORD(0, k)] = 100 + k; st[BEST_STAGE_WORD(1, k)] = lab[(size_t)k]; st[BEST_STAGE_WORD(2, k)] = 200 + k;
                    st[BEST_STAGE_WORD(3, k)] = fbits(300.0f + k); st[BEST_STAGE_WORD(4, k)] = fbits(400.0f + k); st[BEST_STAGE_WORD(5, k)] = fbits(500.0f + k);
                }
                best_take_stage(M, n, st);
            } else {
                std::vector<int32_t> rows(5 * (size_t)n + 1, -1), mrow((size_t)n + 1, -1);
                for (int k = 0; k < n; ++k) {
                    mrow[(size_t)k] = 100 + k;
                    rows[(size_t)k] = lab[(size_t)k]; rows[(size_t)n + k] = 200 + k;
                    rows[2 * (size_t)n + k] = fbits(300.0f + k); rows[3 * (size_t)n + k] = fbits(400.0f + k); rows[4 * (size_t)n + k] = fbits(500.0f + k);
                }
                best_take_rows(M, n, rows.data(), with_models ? mrow.data() : nullptr);
            }
            read_back(M, cap);
        } else if (cmd == "life") {
            PushStream P;
            auto fill = [&]() { best_resize(P.best, 5); };
            fill();
            printf("%zu %d", P.best.label.size(), P.resident);
            P.init(); printf(" %zu %d", P.best.label.size(), P.resident);
            fill(); P.begin(); printf(" %zu %d", P.best.label.size(), P.resident);
            P.taken_over(); printf(" %zu %d", P.best.label.size(), P.resident);
            P.begin(); P.init(); printf(" %zu %d", P.best.label.size(), P.resident);
            best_clear(P.best); printf(" %zu %zu\n", P.best.model.size() + P.best.label.size() + P.best.time.size(), P.best.score.size() + P.best.ac.size() + P.best.lm.size());
        } else {
            printf("?\n");
        }
    }
    return 0;
}
