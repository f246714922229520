// final_driver.cpp - juicer_amd/csrc/jd_final.h and the model-trace decisions of jd_push.h on the CPU (tests/test_final_cpu.py): one
// decision per input line, integers in, integers out (floats travel as their bits).  No HIP, no device.
//   request s                          -> the four words of the stream's request
//   layout M n i                       -> head_at per words reply_words(n) FINAL_STAGE_AT(n, i) FINAL_HEAD FINAL_FIELDS FINAL_SHARE FINAL_THREADS
//   reply found n_records res_cap      -> FinalReply
//   none frame                         -> the seven words of the head of a stream without a final hypothesis
//   check M {started T resident}xM n s_1 .. s_n -> verdict stream |ss| ss.. at..
//   stage n cap l_1 .. l_n             -> a share of the staging area filled by the layout's own index expression (record k: model
//                                         100 + k, label l_k, time 200 + k, score / ac / lm the floats 300 + k, 400 + k, 500 + k),
//                                         taken, then read back with capacity cap: n_models, 6 x min(cap, n) words, n_words, 5 x
//                                         min(cap, n_words) words - the word list's newest entry with the totals 7, 8, 9 (floats)
//   rows n cap with_models l_1 .. l_n  -> the same records through the result arrays [label, time, score, ac, lm][n] (+ the model row)
//   life                               -> a stream's record: |fin| and the totals' sum after a fill, init()
//   pm_request have have_m last        -> the four words of a model trace's request of stream 5 whose lists have these lengths
//   pm_layout M n i                    -> head_at per words reply_words(n) PM_STAGE_AT(n, i) PM_STAGE_WORD(0, 0) PM_STAGE_WORD(5, PM_SHARE - 1) PM_HEAD PM_SHARE area(M, 100)
//   pm_reply found n nm have have_m res_cap -> PartialModelsReply
//   pm_take have n have_m nm           -> lists of have / have_m older entries (word k: label 10 + k, time 20 + k; record k: fields
//                                         1000 f + k), extended from a share filled by the layout's own expressions (entry 1 of 2), read back
//   pm_arrays n nm                     -> the same lists whole from the device arrays' images
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "jd_final.h"

static int32_t fbits(float f) { int32_t v; memcpy(&v, &f, 4); return v; }

static void read_back(const PushModels &M, int cap)
{
    std::vector<int32_t> a((size_t)cap + 1, -7), b(a), c(a);
    std::vector<float> x((size_t)cap + 1, -7.0f), y(x), z(x);
    int32_t n = -1;
    final_models(M, cap, &n, a.data(), b.data(), c.data(), x.data(), y.data(), z.data());
    const int k = cap < n ? cap : n;
    printf("%d", n);
    for (int i = 0; i < k; ++i) printf(" %d", a[(size_t)i]);
    for (int i = 0; i < k; ++i) printf(" %d", b[(size_t)i]);
    for (int i = 0; i < k; ++i) printf(" %d", c[(size_t)i]);
    for (int i = 0; i < k; ++i) printf(" %d", fbits(x[(size_t)i]));
    for (int i = 0; i < k; ++i) printf(" %d", fbits(y[(size_t)i]));
    for (int i = 0; i < k; ++i) printf(" %d", fbits(z[(size_t)i]));
    if (a[(size_t)cap] != -7 || b[(size_t)cap] != -7 || c[(size_t)cap] != -7 || x[(size_t)cap] != -7.0f || y[(size_t)cap] != -7.0f || z[(size_t)cap] != -7.0f) printf(" OVERRUN");
    std::fill(b.begin(), b.end(), -7); std::fill(c.begin(), c.end(), -7);
    std::fill(x.begin(), x.end(), -7.0f); std::fill(y.begin(), y.end(), -7.0f); std::fill(z.begin(), z.end(), -7.0f);
    const float tot[3] = {7.0f, 8.0f, 9.0f};
    int32_t nw = -1;
    final_words(M, tot, cap, &nw, b.data(), c.data(), x.data(), y.data(), z.data());
    const int kw = cap < nw ? cap : nw;
    printf(" %d", nw);
    for (int i = 0; i < kw; ++i) printf(" %d", b[(size_t)i]);
    for (int i = 0; i < kw; ++i) printf(" %d", c[(size_t)i]);
    for (int i = 0; i < kw; ++i) printf(" %d", fbits(x[(size_t)i]));
    for (int i = 0; i < kw; ++i) printf(" %d", fbits(y[(size_t)i]));
    for (int i = 0; i < kw; ++i) printf(" %d", fbits(z[(size_t)i]));
    if (b[(size_t)cap] != -7 || c[(size_t)cap] != -7 || x[(size_t)cap] != -7.0f || y[(size_t)cap] != -7.0f || z[(size_t)cap] != -7.0f) printf(" OVERRUN");
    int32_t n2 = -1, nw2 = -1;
    final_models(M, cap, &n2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    final_words(M, tot, cap, &nw2, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (n2 != n || nw2 != nw) printf(" NULLS");
    printf("\n");
}

static void print_stream(const PushStream &P)
{
    printf("%zu", P.partial_label.size());
    for (size_t k = 0; k < P.partial_label.size(); ++k) printf(" %d %d", P.partial_label[k], P.partial_time[k]);
    const PushModels &M = P.partial_m;
    printf(" %zu", M.model.size());
    for (size_t k = 0; k < M.model.size(); ++k) printf(" %d %d %d %d %d %d", M.model[k], M.label[k], M.time[k], fbits(M.score[k]), fbits(M.ac[k]), fbits(M.lm[k]));
    if (M.label.size() != M.model.size() || M.time.size() != M.model.size() || M.score.size() != M.model.size() || M.ac.size() != M.model.size() ||
        M.lm.size() != M.model.size() || P.partial_time.size() != P.partial_label.size())
        printf(" RAGGED");
    printf("\n");
}
// record k's field f, as an int word (fields 3 .. 5 travel as floats)
static int32_t pm_word(int f, int k) { return f < 3 ? 1000 * f + k : fbits((float)(1000 * f + k)); }
static void older(PushStream *P, int have, int have_m)
{
    for (int k = 0; k < have; ++k) { P->partial_label.push_back(10 + k); P->partial_time.push_back(20 + k); }
    partial_models_resize(P->partial_m, (size_t)have_m);
    for (int k = 0; k < have_m; ++k) {
        P->partial_m.model[(size_t)k] = k; P->partial_m.label[(size_t)k] = 1000 + k; P->partial_m.time[(size_t)k] = 2000 + k;
        P->partial_m.score[(size_t)k] = (float)(3000 + k); P->partial_m.ac[(size_t)k] = (float)(4000 + k); P->partial_m.lm[(size_t)k] = (float)(5000 + k);
    }
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
            const FinalRequest r = final_request(s);
            int32_t w[4];
            static_assert(sizeof r == sizeof w, "a request is four words");
            memcpy(w, &r, sizeof w);
            printf("%d %d %d %d\n", w[0], w[1], w[2], w[3]);
        } else if (cmd == "layout") {
            int M, n, i; in >> M >> n >> i;
            const FinalLayout Y = final_layout(M);
            printf("%zu %zu %zu %zu %zu %d %d %d %d\n", Y.head_at, Y.per, Y.words, Y.reply_words(n), FINAL_STAGE_AT(n, i), FINAL_HEAD, FINAL_FIELDS, FINAL_SHARE, FINAL_THREADS);
        } else if (cmd == "reply") {
            int found, n, cap; in >> found >> n >> cap;
            printf("%d\n", (int)final_reply(found, n, cap));
        } else if (cmd == "none") {
            int frame; in >> frame;
            const FinalHead h = final_none(frame);
            int32_t w[7];
            memcpy(w, &h, sizeof w);
            for (int k = 0; k < 7; ++k) printf(k ? " %d" : "%d", w[k]);
            printf("\n");
        } else if (cmd == "check") {
            int M; in >> M;
            std::vector<PushStream> S((size_t)M);
            for (PushStream &P : S) in >> P.started >> P.T >> P.resident;
            int n; in >> n;
            std::vector<int32_t> ss((size_t)n);
            for (int32_t &s : ss) in >> s;
            std::vector<int> live, at;
            const BestCheck c = final_check(S, n, ss.data(), &live, &at);
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
                std::vector<int32_t> reply(final_layout(2).reply_words(2), -1);
                int32_t *st = reply.data() + FINAL_STAGE_AT(2, 1);
                for (int k = 0; k < n; ++k) {
                    st[FINAL_STAGE_WORD(0, k)] = 100 + k; st[FINAL_STAGE_WORD(1, k)] = lab[(size_t)k]; st[FINAL_STAGE_WORD(2, k)] = 200 + k;
                    st[FINAL_STAGE_WORD(3, k)] = fbits(300.0f + k); st[FINAL_STAGE_WORD(4, k)] = fbits(400.0f + k); st[FINAL_STAGE_WORD(5, k)] = fbits(500.0f + k);
                }
                final_take_stage(M, n, st);
            } else {
                std::vector<int32_t> rows(5 * (size_t)n + 1, -1), mrow((size_t)n + 1, -1);
                for (int k = 0; k < n; ++k) {
                    mrow[(size_t)k] = 100 + k;
                    rows[(size_t)k] = lab[(size_t)k]; rows[(size_t)n + k] = 200 + k;
                    rows[2 * (size_t)n + k] = fbits(300.0f + k); rows[3 * (size_t)n + k] = fbits(400.0f + k); rows[4 * (size_t)n + k] = fbits(500.0f + k);
                }
                final_take_rows(M, n, rows.data(), with_models ? mrow.data() : nullptr);
            }
            read_back(M, cap);
        } else if (cmd == "life") {
            PushStream P;
            best_resize(P.fin, 5); P.fin_tot[0] = 1.0f; P.fin_tot[1] = 2.0f; P.fin_tot[2] = 3.0f;
            printf("%zu %d", P.fin.label.size(), (int)(P.fin_tot[0] + P.fin_tot[1] + P.fin_tot[2]));
            P.init();
            printf(" %zu %d\n", P.fin.model.size() + P.fin.label.size() + P.fin.time.size() + P.fin.score.size() + P.fin.ac.size() + P.fin.lm.size(),
                   (int)(P.fin_tot[0] + P.fin_tot[1] + P.fin_tot[2]));
        } else if (cmd == "pm_request") {
            int have, have_m, last; in >> have >> have_m >> last;
            PushStream P;
            older(&P, have, have_m);
            if (have) P.partial_time.back() = last;
            const PartialModelsRequest r = partial_models_request(P, 5);
            int32_t w[4];
            static_assert(sizeof r == sizeof w, "a request is four words");
            memcpy(w, &r, sizeof w);
            printf("%d %d %d %d\n", w[0], w[1], w[2], w[3]);
        } else if (cmd == "pm_layout") {
            int M, n, i; in >> M >> n >> i;
            const PartialModelsLayout Y = partial_models_layout(M);
            printf("%zu %zu %zu %zu %zu %zu %zu %d %d %zu\n", Y.head_at, Y.per, Y.words, Y.reply_words(n), PM_STAGE_AT(n, i), PM_STAGE_WORD(0, 0),
                   PM_STAGE_WORD(PM_FIELDS - 1, PM_SHARE - 1), PM_HEAD, PM_SHARE, partial_models_area_words(M, 100));
        } else if (cmd == "pm_reply") {
            int found, n, nm, have, have_m, cap; in >> found >> n >> nm >> have >> have_m >> cap;
            printf("%d\n", (int)partial_models_reply(found, n, nm, have, have_m, cap));
        } else if (cmd == "pm_take") {
            int have, n, have_m, nm; in >> have >> n >> have_m >> nm;
            PushStream P;
            older(&P, have, have_m);
            std::vector<int32_t> reply(partial_models_layout(2).reply_words(2), -1);
            int32_t *st = reply.data() + PM_STAGE_AT(2, 1);
            for (int k = have; k < n; ++k) { st[2 * (k - have)] = 10 + k; st[2 * (k - have) + 1] = 20 + k; }
            for (int k = have_m; k < nm; ++k)
                for (int f = 0; f < PM_FIELDS; ++f) st[PM_STAGE_WORD(f, k - have_m)] = pm_word(f, k);
            partial_models_take(P, have, n, have_m, nm, st);
            print_stream(P);
        } else if (cmd == "pm_arrays") {
            int n, nm; in >> n >> nm;
            PushStream P;
            older(&P, 2, 3);
            std::vector<int32_t> words(2 * (size_t)n + 1, -1), rows((size_t)PM_FIELDS * (size_t)nm + 1, -1);
            for (int k = 0; k < n; ++k) { words[(size_t)k] = 10 + k; words[(size_t)n + k] = 20 + k; }
            for (int f = 0; f < PM_FIELDS; ++f)
                for (int k = 0; k < nm; ++k) rows[(size_t)f * nm + k] = pm_word(f, k);
            partial_models_take_arrays(P, n, words.data(), nm, rows.data());
            print_stream(P);
        } else {
            printf("?\n");
        }
    }
    return 0;
}
