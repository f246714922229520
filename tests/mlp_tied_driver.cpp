// mlp_tied_driver.cpp - the TIED side of csrc/jd_mlp.h under plain g++ (tests/test_mlp_tied_cpu.py): the host twin of a tied
// model (logZ by JD_MLP_LZ_CHAINS interleaved chains) with libm's own expf and log as its policy, the argument check with the
// tied limit, the JMLP reader for either version, the tied kernel's layer table, and the scoring plan of a tied model.
//   forward NET X N STOP OUT     NET: a JMLP VERSION 2 file; X: N x in_dim raw floats; STOP >= 0: the activations behind that layer,
//                                -1: the log posteriors, -2: the hybrid scores (minus logf(prior)); OUT: raw floats
//   check TIED IN_DIM N_OUT N_LAYERS WIDTH.. ACT..     prints the check's code and message
//   read TIED NET [OUT]          prints the reader's code and message (TIED: 1 reads version 2, 0 version 1); code 0: writes it again
//   dev NET                      prints the tied stride and LDS bytes, then the untied ones
//   plan TIED N_GMM N_ROWS MAX_BLOCKS     prints kernel, grid, tile_rows of a neural model's plan
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "jd_score_plan.h"

struct LibmMath {
    float exp(float x) const { return expf(x); }
    // HTKFlatModels::logAdd, HTKFlatModels.cpp:266-293
    float log_add(float x, float y) const
    {
        if (x < y) { const float t = x; x = y; y = t; }
        const float d = y - x;
        if (d < -18.42) return x;
        return (float)(x + log(1.0 + expf(d)));
    }
};

static bool slurp(const char *path, std::vector<unsigned char> &b)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    unsigned char chunk[4096];
    size_t n;
    b.clear();
    while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) b.insert(b.end(), chunk, chunk + n);
    fclose(f);
    return true;
}
static bool spill(const char *path, const void *p, size_t n)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}
static int load(const char *path, bool tied, JdMlpFile &f, char *msg, size_t cap)
{
    std::vector<unsigned char> b;
    if (!slurp(path, b)) { snprintf(msg, cap, "cannot read %s", path); return -1; }
    return jd_mlp_file_read(b.data(), b.size(), f, msg, cap, tied);
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    char msg[400] = "";
    JdMlpFile f;
    if (cmd == "check") {
        if (argc < 6) return 2;
        JdMlpDesc d;
        const bool tied = atoi(argv[2]) != 0;
        d.in_dim = atoi(argv[3]);
        const int n_out = atoi(argv[4]);
        d.n_layers = atoi(argv[5]);
        if (d.n_layers < 1 || d.n_layers > JD_MLP_MAX_LAYERS || argc != 6 + 2 * d.n_layers) return 2;
        for (int l = 0; l < d.n_layers; ++l) { d.width[l] = atoi(argv[6 + l]); d.act[l] = atoi(argv[6 + d.n_layers + l]); }
        const int rc = jd_mlp_check(d, n_out, msg, sizeof msg, tied);
        printf("%d %s\n", rc, msg);
        return 0;
    }
    if (cmd == "plan" && argc == 6) {
        ScorePlanIn in{9, atoi(argv[3]), true, true, false, atoi(argv[4]), atoi(argv[5]), -1, false, 0};
        in.tied = atoi(argv[2]) != 0;
        const ScorePlan p = score_plan(in);
        printf("%d %u %d %d %d\n", p.kernel, p.grid, p.tile_rows, score_plan_tile_rows(9, true, true, false),
               score_plan_large(9, true, true, false).kernel);
        return 0;
    }
    if (cmd == "read") {
        if (argc < 4) return 2;
        const int rc = load(argv[3], atoi(argv[2]) != 0, f, msg, sizeof msg);
        printf("%d %s\n", rc, msg);
        if (rc == 0 && argc > 4) {
            std::vector<unsigned char> b;
            jd_mlp_file_write(f, b);
            if (!spill(argv[4], b.data(), b.size())) return 3;
        }
        return 0;
    }
    if (argc < 3) return 2;
    const int rc = load(argv[2], true, f, msg, sizeof msg);
    if (rc) { fprintf(stderr, "%s\n", msg); return 3; }
    if (cmd == "forward" && argc == 7) {
        const int n = atoi(argv[4]), stop = atoi(argv[5]);
        std::vector<unsigned char> xb;
        if (!slurp(argv[3], xb) || xb.size() != (size_t)n * f.d.in_dim * 4) return 3;
        std::vector<float> x((size_t)n * f.d.in_dim + 1), lp((size_t)f.n_phones);
        memcpy(x.data(), xb.data(), xb.size());
        for (int j = 0; j < f.n_phones; ++j) lp[(size_t)j] = std::log(f.priors[(size_t)j]);
        const int ow = stop >= 0 ? f.d.width[stop] : f.n_phones;
        std::vector<float> out((size_t)n * ow + 1);
        jd_mlp_forward_host(f.d, f.w.data(), f.b.data(), stop == -2 ? lp.data() : nullptr, x.data(), n, stop < 0 ? -1 : stop, out.data(), LibmMath(), true);
        return spill(argv[6], out.data(), (size_t)n * ow * 4) ? 0 : 3;
    }
    if (cmd == "dev") {
        const JdMlpDev t = jd_mlp_dev(f.d, true), u = jd_mlp_dev(f.d);
        printf("%d %zu %d %zu\n", t.stride, jd_mlp_tied_lds_bytes(t), u.stride, jd_mlp_lds_bytes(u));
        return 0;
    }
    return 2;
}
