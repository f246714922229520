// Own-written stand-in for the *declarations* of Juicer's src/Decoder.h (:8 include guard, :13-31 IDecoder) and
// src/WFSTLattice.h (:20, :52), with the record types from the DecHypHistPool.h stand-in beside it.  Test
// infrastructure only (tests/test_model_output_cpu.py).
#ifndef DECODER_H
#define DECODER_H
#include "DecHypHistPool.h"
namespace Juicer {
class WFSTLattice;
class IDecoder {
public:
    virtual ~IDecoder() {}
    virtual bool modelLevelOutput() = 0;
    virtual WFSTLattice *getLattice() = 0;
    virtual void init() = 0;
    virtual void processFrame(float **inputVec, int currFrame_, int nFrames) = 0;
    virtual DecHyp *finish() = 0;
};
}
#endif
