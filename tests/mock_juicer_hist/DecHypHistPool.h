// Own-written stand-in for the *declarations* of Juicer's src/DecHypHistPool.h (:10-11 include guard, :38-56
// DecHypHist / LabDecHypHist, :106-107 record types, :146-165 DecHyp): enough for a compile-only check that
// include/juicer_amd_decoder.hpp's in-tree branch uses Juicer's own LabDecHypHist for model-level output.
// Test infrastructure only.
#ifndef DECHYPHISTPOOL_INC
#define DECHYPHISTPOOL_INC
#include <cfloat>
#include <cstddef>
#ifndef real
#define real float
#endif
#ifndef LOG_ZERO
#define LOG_ZERO (-FLT_MAX)
#endif
#define DHHTYPE 1
#define LABDHHTYPE 2
namespace Juicer {
struct DecHypHist {
    unsigned char type; int nConnect; DecHypHist *prev;
    int state; int time; real score; real acousticScore; real lmScore;
};
struct LabDecHypHist {
    unsigned char type; int nConnect; DecHypHist *prev;
    int label;
};
class DecHyp {
public:
    DecHypHist *hist; int state; real score, acousticScore, lmScore;
    char nLabelsNR; int labelsNR[2];
    DecHyp() : hist(NULL), state(-1), score(LOG_ZERO), acousticScore(LOG_ZERO), lmScore(LOG_ZERO), nLabelsNR(0) {}
    virtual ~DecHyp() {}
};
}
#endif
