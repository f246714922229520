// Stand-alone driver for the body of jd_debug_cl_label_sets (jd_label_sets_csr, juicer_amd/csrc/jd_labelsets.h): plain host C++, no device and no library -
// tests/test_compose_sets_cpu.py compiles it with g++ and compares what it prints with the Python sets; built with
// -fsanitize=address,undefined it is the sanitizer run of the set computation.
//   stdin:  n_states init n_arcs cap, then n_states final flags (0 / 1), then n_arcs lines "src dst in out" sorted by src
//   stdout: the return code and n_total, then (on success) one line per state: mayfin, then the labels of S(c)
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "jd_labelsets.h"

int jd_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return code;
}
const char *jd_dev_env(const char *name) { return getenv(name); }

int main()
{
    int S = 0, init = 0;
    long long n_arcs = 0, cap = 0;
    if (scanf("%d %d %lld %lld", &S, &init, &n_arcs, &cap) != 4 || S < 1 || n_arcs < 0) return 2;
    jd_net net;
    net.n_states = S; net.init = init; net.n_arcs = n_arcs;
    net.fin_w.assign((size_t)S, std::numeric_limits<float>::infinity());
    for (int c = 0; c < S; ++c) { int f = 0; if (scanf("%d", &f) != 1) return 2; if (f) net.fin_w[(size_t)c] = 0.0f; }
    net.row_ptr.assign((size_t)S + 1, 0);
    int last = 0;
    for (long long a = 0; a < n_arcs; ++a) {
        int src, dst, in, out;
        if (scanf("%d %d %d %d", &src, &dst, &in, &out) != 4 || src < last || src >= S || dst < 0 || dst >= S) return 2;
        last = src;
        net.arcs.push_back(JdArc{dst, 0.0f, in, out});
        ++net.row_ptr[(size_t)src + 1];
    }
    for (int c = 0; c < S; ++c) net.row_ptr[(size_t)c + 1] += net.row_ptr[(size_t)c];
    std::vector<int64_t> row((size_t)S + 1, 0);
    std::vector<int32_t> labels((size_t)(cap > 0 ? cap : 1));
    std::vector<uint8_t> mayfin((size_t)S, 0);
    int64_t total = -1;
    const int rc = jd_label_sets_csr(&net, row.data(), labels.data(), cap, &total, mayfin.data());
    printf("%d %lld\n", rc, (long long)total);
    if (rc) return 0;
    for (int c = 0; c < S; ++c) {
        printf("%d", (int)mayfin[(size_t)c]);
        for (int64_t i = row[(size_t)c]; i < row[(size_t)c + 1]; ++i) printf(" %d", labels[(size_t)i]);
        printf("\n");
    }
    return 0;
}
