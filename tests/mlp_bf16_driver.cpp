// mlp_bf16_driver.cpp - csrc/jd_mlp_bf16.h and the bf16 side of csrc/jd_score_plan.h under plain g++ (tests/test_mlp_bf16_cpu.py):
// the rounding, the host twin with libm's own expf and log as its policy, the packing and its inverse, the kernels' layer table,
// the scoring plan.
//   round IN OUT                 IN: raw floats; OUT: jd_bf16_round of each, raw floats
//   forward NET X N STOP TIED OUT    NET: a JMLP file (version 1); X: N x in_dim raw floats; STOP >= 0: the activations behind that layer,
//                                -1: the log posteriors, -2: the hybrid scores; TIED: 1 = logZ by 128 interleaved chains; OUT: raw floats.
//                                The file's weights are rounded first, as jd_am_mlp_to_bf16 does.
//   pack NET WP BP W2 B2         the packed weights (16-bit) / biases, and what unpacking them gives (floats)
//   dev NET                      prints stride, LDS bytes, LDS bytes tied, then w_off[0 .. n_layers] and b_off[0 .. n_layers]
//   plan D N_GMM HYBRID MLP FAST N_ROWS MAX_BLOCKS USED_ROW_TILES HAS_LIST N_RT_LIST TIED BF16
//                                prints verdict kernel tile_rows tile_states row_tiles tiles grid lds_bytes dp
//   limits                       prints JD_MLP_BF16_ROWS JD_MLP_BF16_KG JD_MLP_BF16_NT JD_MLP_BF16_LDS_MAX JD_MLP_TIED_BF16_LDS_MAX
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "jd_mlp_bf16.h"
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

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "limits") {
        printf("%d %d %d %zu %zu\n", JD_MLP_BF16_ROWS, JD_MLP_BF16_KG, JD_MLP_BF16_NT, (size_t)JD_MLP_BF16_LDS_MAX, (size_t)JD_MLP_TIED_BF16_LDS_MAX);
        return 0;
    }
    if (cmd == "round" && argc == 4) {
        std::vector<unsigned char> b;
        if (!slurp(argv[2], b) || b.size() % 4) return 3;
        std::vector<float> x(b.size() / 4 + 1);
        memcpy(x.data(), b.data(), b.size());
        for (size_t i = 0; i < b.size() / 4; ++i) x[i] = jd_bf16_round(x[i]);
        return spill(argv[3], x.data(), b.size()) ? 0 : 3;
    }
    if (cmd == "plan") {                                               // one case a line of standard input, one plan a line
        int v[12];
        while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11) == 12) {
            ScorePlanIn in{v[0], v[1], v[2] != 0, v[3] != 0, v[4] != 0, v[5], v[6], v[7], v[8] != 0, v[9], v[10] != 0, v[11] != 0};
            const ScorePlan p = score_plan(in);
            printf("%d %d %d %d %lld %lld %u %zu %d\n", (int)p.verdict, p.kernel, p.tile_rows, p.tile_states, p.row_tiles, p.tiles, p.grid, p.lds_bytes, p.dp);
        }
        return 0;
    }
    if (argc < 3) return 2;
    char msg[400] = "";
    JdMlpFile f;
    {
        std::vector<unsigned char> b;
        if (!slurp(argv[2], b) || jd_mlp_file_read(b.data(), b.size(), f, msg, sizeof msg)) { fprintf(stderr, "%s: %s\n", argv[2], msg); return 3; }
    }
    if (cmd == "forward" && argc == 8) {
        const int n = atoi(argv[4]), stop = atoi(argv[5]);
        const bool tied = atoi(argv[6]) != 0;
        std::vector<unsigned char> xb;
        if (!slurp(argv[3], xb) || xb.size() != (size_t)n * f.d.in_dim * 4) return 3;
        std::vector<float> x((size_t)n * f.d.in_dim + 1), lp((size_t)f.n_phones);
        memcpy(x.data(), xb.data(), xb.size());
        for (int j = 0; j < f.n_phones; ++j) lp[(size_t)j] = std::log(f.priors[(size_t)j]);
        for (float &w : f.w) w = jd_bf16_round(w);
        const int ow = stop >= 0 ? f.d.width[stop] : f.n_phones;
        std::vector<float> out((size_t)n * ow + 1);
        jd_mlp_bf16_forward_host(f.d, f.w.data(), f.b.data(), stop == -2 ? lp.data() : nullptr, x.data(), n, stop < 0 ? -1 : stop, out.data(), LibmMath(), tied);
        return spill(argv[7], out.data(), (size_t)n * ow * 4) ? 0 : 3;
    }
    if (cmd == "pack" && argc == 7) {
        std::vector<uint16_t> wp;
        std::vector<float> bp, w2, b2;
        jd_mlp_bf16_pack(f.d, f.w.data(), f.b.data(), wp, bp);
        jd_mlp_bf16_unpack(f.d, wp.data(), bp.data(), w2, b2);
        return spill(argv[3], wp.data(), wp.size() * 2) && spill(argv[4], bp.data(), bp.size() * 4) && spill(argv[5], w2.data(), w2.size() * 4) &&
                       spill(argv[6], b2.data(), b2.size() * 4) ? 0 : 3;
    }
    if (cmd == "dev") {
        const JdMlpDev m = jd_mlp_bf16_dev(f.d);
        printf("%d %zu %zu", m.stride, jd_mlp_bf16_lds_bytes(m), jd_mlp_tied_bf16_lds_bytes(m));
        for (int l = 0; l <= f.d.n_layers; ++l) printf(" %u", m.w_off[l]);
        for (int l = 0; l <= f.d.n_layers; ++l) printf(" %u", m.b_off[l]);
        printf("\n");
        return 0;
    }
    return 2;
}
