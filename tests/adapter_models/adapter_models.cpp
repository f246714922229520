// Drives include/juicer_amd_decoder.hpp's stand-alone GpuWFSTDecoder through the reference's serial protocol
// (init / processFrame with 20 rows of look-ahead / finish, DecoderSingleTest.cpp:259-324) and writes the DecHypHist
// chain finish() returns, record for record.  Test infrastructure (tests/test_gpu_model_harness.py).
//   adapter_models FSM MMF OUT MODEL_LEVEL MAIN_BEAM UTT.jdf...
// OUT, per utterance: int32 n_records, float32 hyp score / ac / lm, then per record (newest first) int32 type, int32 id
// (DHHTYPE: state, LABDHHTYPE: label), int32 time, float32 score, ac, lm (0 for a label record); n_records = -1: no hyp.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "juicer_amd.h"
#include "juicer_amd_decoder.hpp"

static void die(const char *what) { fprintf(stderr, "adapter_models: %s: %s\n", what, jd_last_error()); exit(1); }

int main(int argc, char **argv)
{
    if (argc < 7) { fprintf(stderr, "usage: adapter_models FSM MMF OUT MODEL_LEVEL MAIN_BEAM UTT.jdf...\n"); return 2; }
    jd_net *net = 0;
    jd_am *am = 0;
    if (jd_net_load_fsm(&net, argv[1], 0, 0, 1.0f, 0.0f)) die("jd_net_load_fsm");
    if (jd_am_load_mmf(&am, argv[2])) die("jd_am_load_mmf");
    FILE *o = fopen(argv[3], "wb");
    if (!o) { fprintf(stderr, "adapter_models: cannot write %s\n", argv[3]); return 1; }
    const bool models = atoi(argv[4]) != 0;
    const int D = jd_am_vec_size(am);
    {
        JuicerAmd::GpuWFSTDecoder dec(net, am, 0.0f, (float)atof(argv[5]), 0.0f, 0.0f, 0);
        if (dec.modelLevelOutput()) { fprintf(stderr, "adapter_models: model-level output is on by default\n"); return 1; }
        dec.setModelLevelOutput(models);
        if (dec.modelLevelOutput() != models) { fprintf(stderr, "adapter_models: modelLevelOutput() does not follow the setting\n"); return 1; }
        for (int a = 6; a < argc; ++a) {
            FILE *f = fopen(argv[a], "rb");
            int32_t hdr[2] = {0, 0};
            if (!f || fread(hdr, 4, 2, f) != 2 || hdr[1] != D) { fprintf(stderr, "adapter_models: bad feature file %s\n", argv[a]); return 1; }
            const int T = hdr[0];
            std::vector<float> x((size_t)T * D);
            if (T && fread(&x[0], 4, x.size(), f) != x.size()) { fprintf(stderr, "adapter_models: short %s\n", argv[a]); return 1; }
            fclose(f);
            std::vector<float *> rows((size_t)T);
            for (int t = 0; t < T; ++t) rows[(size_t)t] = &x[(size_t)t * D];
            dec.init();
            int nFrames = 0, nData = T < 20 ? T : 20;
            while (nData > 0) {
                dec.processFrame(&rows[(size_t)nFrames], nFrames, nData);
                ++nFrames;
                if (nFrames + nData - 1 >= T) --nData;
            }
            JuicerAmd::DecHyp *hyp = dec.finish();
            int32_t n = 0;
            for (JuicerAmd::DecHypHist *h = hyp ? hyp->hist : 0; h; h = h->prev) ++n;
            if (!hyp) n = -1;
            const float tot[3] = {hyp ? hyp->score : 0.0f, hyp ? hyp->acousticScore : 0.0f, hyp ? hyp->lmScore : 0.0f};
            fwrite(&n, 4, 1, o);
            fwrite(tot, 4, 3, o);
            for (JuicerAmd::DecHypHist *h = hyp ? hyp->hist : 0; h; h = h->prev) {
                int32_t r[3] = {h->type, h->state, h->time};
                float s[3] = {h->score, h->acousticScore, h->lmScore};
                if (h->type == LABDHHTYPE) {
                    const JuicerAmd::LabDecHypHist *l = reinterpret_cast<const JuicerAmd::LabDecHypHist *>(h);
                    r[1] = l->label; r[2] = 0; s[0] = s[1] = s[2] = 0.0f;
                } else if (h->type != DHHTYPE) { fprintf(stderr, "adapter_models: record type %d\n", (int)h->type); return 1; }
                fwrite(r, 4, 3, o);
                fwrite(s, 4, 3, o);
            }
        }
    }
    fclose(o);
    jd_am_destroy(am);
    jd_net_destroy(net);
    return 0;
}
