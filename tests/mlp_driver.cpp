// mlp_driver.cpp - csrc/jd_mlp.h under plain g++ (tests/test_mlp_cpu.py): the host twin with libm's own expf and log as its
// policy, the packing and its inverse, the argument check, the JMLP reader and writer, the kernel's layer table.
//   forward NET X N STOP OUT     NET: a JMLP file; X: N x in_dim raw floats; STOP >= 0: the activations behind that layer, -1: the log
//                                posteriors, -2: the hybrid scores (minus logf(prior)); OUT: raw floats
//   pack NET WP BP W2 B2         the packed weights / biases, and what unpacking them gives
//   check IN_DIM N_PHONES N_LAYERS WIDTH.. ACT..     prints the check's code and message
//   read NET OUT                 prints the reader's code and message; code 0: writes the file again to OUT
//   dev NET                      prints stride, LDS bytes, then w_off[0 .. n_layers] and b_off[0 .. n_layers]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "jd_mlp.h"

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
static int load(const char *path, JdMlpFile &f, char *msg, size_t cap)
{
    std::vector<unsigned char> b;
    if (!slurp(path, b)) { snprintf(msg, cap, "cannot read %s", path); return -1; }
    return jd_mlp_file_read(b.data(), b.size(), f, msg, cap);
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    char msg[400] = "";
    JdMlpFile f;
    if (cmd == "check") {
        if (argc < 5) return 2;
        JdMlpDesc d;
        d.in_dim = atoi(argv[2]);
        const int n_phones = atoi(argv[3]);
        d.n_layers = atoi(argv[4]);
        const int n = d.n_layers < 0 ? 0 : d.n_layers > JD_MLP_MAX_LAYERS ? JD_MLP_MAX_LAYERS : d.n_layers;
        if (argc != 5 + 2 * n && !(d.n_layers > JD_MLP_MAX_LAYERS || d.n_layers < 1)) return 2;
        for (int l = 0; l < n && 5 + n + l < argc; ++l) { d.width[l] = atoi(argv[5 + l]); d.act[l] = atoi(argv[5 + n + l]); }
        const int rc = jd_mlp_check(d, n_phones, msg, sizeof msg);
        printf("%d %s\n", rc, msg);
        return 0;
    }
    if (argc < 3) return 2;
    const int rc = load(argv[2], f, msg, sizeof msg);
    if (cmd == "read") {
        printf("%d %s\n", rc, msg);
        if (rc == 0 && argc > 3) {
            std::vector<unsigned char> b;
            jd_mlp_file_write(f, b);
            if (!spill(argv[3], b.data(), b.size())) return 3;
        }
        return 0;
    }
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
        jd_mlp_forward_host(f.d, f.w.data(), f.b.data(), stop == -2 ? lp.data() : nullptr, x.data(), n, stop < 0 ? -1 : stop, out.data(), LibmMath());
        return spill(argv[6], out.data(), (size_t)n * ow * 4) ? 0 : 3;
    }
    if (cmd == "pack" && argc == 7) {
        std::vector<float> wp, bp, w2, b2;
        jd_mlp_pack(f.d, f.w.data(), f.b.data(), wp, bp);
        jd_mlp_unpack(f.d, wp.data(), bp.data(), w2, b2);
        return spill(argv[3], wp.data(), wp.size() * 4) && spill(argv[4], bp.data(), bp.size() * 4) && spill(argv[5], w2.data(), w2.size() * 4) &&
                       spill(argv[6], b2.data(), b2.size() * 4) ? 0 : 3;
    }
    if (cmd == "dev") {
        const JdMlpDev m = jd_mlp_dev(f.d);
        printf("%d %zu", m.stride, jd_mlp_lds_bytes(m));
        for (int l = 0; l <= f.d.n_layers; ++l) printf(" %u", m.w_off[l]);
        for (int l = 0; l <= f.d.n_layers; ++l) printf(" %u", m.b_off[l]);
        printf("\n");
        return 0;
    }
    return 2;
}
