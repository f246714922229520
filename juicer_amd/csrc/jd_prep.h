// jd_prep.h - how the search kernels see the graph and the models, as a function of plain data (no HIP, no environment, nothing
// printed: compiled and tested on the CPU, tests/test_prep_cpu.py): the decoder's own state numbering, the device arc table with its
// flags, its arc order and the per-state record that goes with it, the layout of a stream's per-state words, the tables phase A reads
// by HMM and by transition matrix, the histogram's range.  jd_dec_create (jd_device.hip) reads the development knobs into PrepKnobs,
// runs these in the order they stand here and uploads what they return.
// At the top, what the host code and the kernels must agree on: the flag bits of a device arc, XState, xcand(), LZ.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "jd_internal.h"

#ifdef __HIPCC__
#define JD_HD __host__ __device__ __forceinline__
#else
#define JD_HD inline
#endif

#define LZ (-3.402823466e+38f)       // LOG_ZERO
#define TEE_FLAG 0x40000000          // bit 30 of the device arc's in-label: the arc's HMM is a tee model
#define SOLE_FLAG 0x20000000         // bit 29: the arc is the ONLY arc that leads to its destination state (prep_arcs) - see REC_SOLE
#define ARC_FLAGS (TEE_FLAG | SOLE_FLAG)
#define TRP_LDS_MAX 4096             // floats of transition tables cached in LDS (else read from HBM)

// per-state STATIC record of the decoder's own copy of the graph (shared by the streams; prep_arcs).  The decoder keeps the
// arcs of a state in an order of its own: first the arcs every arrival has to walk (epsilon inputs, tee models: n_always of
// them), then the arcs that enter a model, by DESCENDING w + tmax (arc weight + the model's largest entry transition) - the
// quantity phase X's "hopeless candidate" test runs on.  An arrival of score s can only enter the arcs of a PREFIX of that order;
// k[] samples the order at the positions xcand() so that an item finds an upper bound of its prefix from this one record instead
// of looking at every arc: the slot kernel (jd_slot.h: phase X) does not walk the arcs behind it at all.  What the walk did for
// them besides is accounted from here: n_model (arcs that carry a model, tee models included) less the instance flags set in the
// state's row (StreamDev::live: one byte per arc, a row's flags side by side) gives the arcs entered without an instance, wmax the
// best entry-token candidate.  (k_search walks every arc, in this order, and does not read this record.)
#define XNCAND 12
struct alignas(64) XState { int n_always, n_entry; float wmax; int n_model; float k[XNCAND]; };
JD_HD constexpr int xcand(int i)
{
    return i == 0 ? 0 : i == 1 ? 1 : i == 2 ? 2 : i == 3 ? 3 : i == 4 ? 4 : i == 5 ? 6 : i == 6 ? 8 : i == 7 ? 12 : i == 8 ? 16 : i == 9 ? 24 : i == 10 ? 32 : 64;
}
// collectPaths' count trigger (WFSTDecoderLite.cpp:360-362): nPath / nPathNew > 12 and nPath > 10000, with the IEEE float
// division of the reference (nPathNew = 0 before the first collection: the ratio is +inf).  The counts are this
// reference's where DecConst::pcount is there (n_paths_ref / path_new_ref: a Path per labelled propagateToken call, winner
// or not, and what collectPaths keeps), else this build's own records - at most the reference's, which also creates
// records for tokens that lose their state's recombination.  The kernels ask it before a frame, the host behind a stream's
// last frame of a launch (jd_push.h).
JD_HD bool path_rule_fires(int n_path, int n_path_new)
{
    return n_path > 10000 && (float)n_path / (float)n_path_new > 12.0f;
}
// k_partial_many's staging share: (label, frame) pairs per entry of a launch (jd_gc.h says why 32; the host's side: jd_push.h)
#define PARTIAL_SHARE 32
// Only rows the cut can apply to - up to 57 arcs, jd_slot.h: the flags of a longer row do not fit an item's loads - change their
// order: the long rows of trigram-shaped graphs keep the file's, which the searches of such graphs are 2-3 % faster on (measured on
// the north-star graph).
#define XSORT_MAX_ROW 57

// The development knobs of the preparation as plain data: -1 = unset.  renumber 0 / 1: never / always the decoder's own state
// numbering; xsort 0: the file's arc order; sole 0: no arc is flagged SOLE; xcut 0 / 1: k_search's prefix walk off / on; srec_split
// 0 / 1 / 2: the per-state words joint / split / split by parity; no_lr 1: the general path for left-to-right models.
struct PrepKnobs { int renumber = -1, xsort = -1, sole = -1, xcut = -1, srec_split = -1, no_lr = -1; };

// arcs that lead to the next state number
inline int64_t prep_count_next(const std::vector<int32_t> &row_ptr, const std::vector<JdArc> &arcs, int n_states)
{
    int64_t n = 0;
    for (int q = 0; q < n_states; ++q)
        for (int b = row_ptr[(size_t)q]; b < row_ptr[(size_t)q + 1]; ++b) n += arcs[(size_t)b].to == q + 1;
    return n;
}

// "index it by the decoder's own state numbers": out[state_new[q]] = v[q]
template <typename T>
std::vector<T> permute_by_state(const std::vector<int> &state_new, const std::vector<T> &v)
{
    std::vector<T> out(v.size());
    for (size_t q = 0; q < v.size(); ++q) out[(size_t)state_new[q]] = v[q];
    return out;
}

// The decoder's OWN numbering of the states.  A stream's per-state words (jd_search.h: StateRec) are gathered by state number, eight
// arrival keys to a 64-byte line, so which states are neighbours in NUMBER decides how many lines a frame fetches - and tokens
// move along chains.  The numbering: a state, then, arc by arc, the chain of one-arc states behind each of its arcs (the phones of
// a word, one state after the other; the chains that leave one state side by side, as their instances are attached in the same
// frame); the states the chains END in - the ones with a choice to make - get their number there and take their turn first come,
// first served.  That is how a lexicon written chain after chain is laid out already, and such a network keeps its numbering; one
// numbered by its composition (jd_net_compose: canonical, breadth first) gets this one.  State numbers never leave the device and
// nothing breaks a tie by them (the frontier item's number does): results are bit-identical.  Measured on the composed configs[4]
// graph (k frames/s, tools/r6_run21-24.sh): the network's numbers 36.7, along the chains of first model arcs 36.7 (round 6's first
// attempt), depth first 41.3, blocks of 16 filled breadth first 43.5, this 45.0; on the bench's generated graphs it equals the
// generator's own order (129.8 / 129.1 k, 5.60 / 5.65 k), every other order loses 1-4 % to it.
// (knob: 1 / 0 - always / never.)
struct PrepNumbering {
    std::vector<int> state_new;          // state_new[network state]; empty: the network's numbering is kept - the rule or the knob
                                         // says no, or the new numbering equals the old
    std::vector<int32_t> row_ptr;        // the network in the decoder's numbering (empty with state_new)
    std::vector<JdArc> arcs;
    int64_t n_next_net = 0;              // arcs of the network that lead to the next state number
    bool tried = false, same = false;    // the numbering was made; ... and came out as the network's
};
inline PrepNumbering prep_renumber(const jd_net &net, int knob)
{
    PrepNumbering N;
    const int ns = net.n_states;
    N.n_next_net = prep_count_next(net.row_ptr, net.arcs, ns);
    N.tried = ns > 0 && (knob >= 0 ? knob != 0 : 4 * N.n_next_net < (int64_t)net.n_arcs);
    if (!N.tried) return N;
    std::vector<int> new_of((size_t)ns, -1), old_of((size_t)ns);
    int next = 0;
    auto take = [&](int q) { new_of[(size_t)q] = next; old_of[(size_t)next] = q; ++next; };
    std::vector<int> pend;                                         // numbered states whose arcs are still to be followed, in the order they were met
    for (int pass = 0; pass < 2; ++pass)                           // (from the initial state; then whatever it does not reach, in the network's order)
        for (int s0 = pass == 0 ? net.init : 0; s0 < (pass == 0 ? net.init + 1 : ns); ++s0) {
            if (new_of[(size_t)s0] >= 0) continue;
            take(s0);
            pend.clear(); pend.push_back(s0);
            for (size_t ph = 0; ph < pend.size(); ++ph) {
                const int q = pend[ph];
                for (int b = net.row_ptr[(size_t)q]; b < net.row_ptr[(size_t)q + 1]; ++b) {
                    int t = net.arcs[(size_t)b].to;
                    while (new_of[(size_t)t] < 0 && net.row_ptr[(size_t)t + 1] - net.row_ptr[(size_t)t] == 1) {
                        take(t);
                        t = net.arcs[(size_t)net.row_ptr[(size_t)t]].to;
                    }
                    if (new_of[(size_t)t] < 0) { take(t); pend.push_back(t); }
                }
            }
        }
    N.same = true;
    for (int q = 0; q < ns && N.same; ++q) N.same = new_of[(size_t)q] == q;
    if (N.same) return N;
    N.row_ptr.assign((size_t)ns + 1, 0);
    for (int n = 0; n < ns; ++n) N.row_ptr[(size_t)n + 1] = N.row_ptr[(size_t)n] + (net.row_ptr[(size_t)old_of[(size_t)n] + 1] - net.row_ptr[(size_t)old_of[(size_t)n]]);
    N.arcs.resize(net.arcs.size());
    for (int n = 0; n < ns; ++n) {
        const int q = old_of[(size_t)n], r0 = net.row_ptr[(size_t)q], r1 = net.row_ptr[(size_t)q + 1];
        for (int b = r0; b < r1; ++b) {
            JdArc a = net.arcs[(size_t)b];
            a.to = new_of[(size_t)a.to];
            N.arcs[(size_t)N.row_ptr[(size_t)n] + (size_t)(b - r0)] = a;
        }
    }
    N.state_new.swap(new_of);
    return N;
}

// What phase A and phase X read by HMM and by transition matrix.
struct PrepModels {
    std::vector<float> tmax0;            // largest log transition probability out of the entry state of every HMM (phase X, hopeless candidates)
    std::vector<int> se32;               // [tm][state]: first | last << 16 of the predecessors (SEIndex)
    int AI = 4;                          // ints per HMM of aux
    std::vector<int> aux;                // the instance template
    std::vector<float> lrt;              // left-to-right topologies only (else empty): per transition matrix a_1.., s_1..
};
inline PrepModels prep_models(const jd_am &am, const PrepKnobs &knobs)
{
    PrepModels M;
    M.tmax0.assign((size_t)am.n_hmm, LZ);
    for (int h = 0; h < am.n_hmm; ++h) {
        const float *t0 = am.trP.data() + (size_t)am.hmm_tm[(size_t)h] * am.max_n * am.max_n;
        for (int j = 0; j < am.hmm_n[(size_t)h]; ++j) M.tmax0[(size_t)h] = std::max(M.tmax0[(size_t)h], t0[j]);
    }
    M.se32.resize((size_t)am.n_tm * am.max_n);
    for (size_t i = 0; i < M.se32.size(); ++i)
        M.se32[i] = ((int)am.se[i * 2] & 0xffff) | ((int)am.se[i * 2 + 1] << 16);
    // instance template: what phase A needs to attach an instance (attachNetInst :751-774), by HMM -
    // {nStates | transMat << 8, g0, g1, g2} (+ {g3, g4, g5, 0}): one hop behind the arc record's label, but the
    // table is a few tens of KB (L2 hits) where a per-arc copy was a second random 64-byte sector per new
    // instance and 16-32 B per arc of HBM (measured: same speed at configs[1], +0.5 % in the heavy legs)
    const int AI = M.AI = (am.max_n <= 5) ? 4 : 8;
    M.aux.assign((size_t)am.n_hmm * AI, 0);
    for (int hm = 0; hm < am.n_hmm; ++hm) {
        const int n = am.hmm_n[(size_t)hm];
        int *a = M.aux.data() + (size_t)hm * AI;
        a[0] = n | (am.hmm_tm[(size_t)hm] << 8);
        for (int j = 1; j < n - 1 && j <= (AI == 4 ? 3 : 6); ++j)
            a[j] = am.hmm_gmm[(size_t)hm * am.max_n + j];
    }
    // Plain left-to-right topologies (every emitting state entered from its predecessor and itself,
    // the exit state from the last emitting state - createTrPandSEIndex, HTKModels.cpp:2330-2390,
    // gives SEIndex[j] = {j-1, j+1}): phase A then needs a_k = log P(k-1 -> k), s_k = log P(k -> k) only
    const int MNn = am.max_n, NEn = (MNn <= 5) ? 3 : 6, LRW = (NEn == 3) ? 8 : 16;
    bool all_lr = (size_t)am.n_tm * LRW <= TRP_LDS_MAX;
    for (int t = 0; t < am.n_tm && all_lr; ++t) {
        const int n = am.tm_n[(size_t)t];
        if (n < 3) all_lr = false;
        for (int j = 1; j < n && all_lr; ++j) {
            const int st = am.se[((size_t)t * MNn + j) * 2], en = am.se[((size_t)t * MNn + j) * 2 + 1];
            if (j < n - 1 ? (st != j - 1 || en != j + 1) : (st != n - 2 || en != n - 1)) all_lr = false;
        }
    }
    for (int h = 0; h < am.n_hmm && all_lr; ++h)
        if (am.hmm_n[(size_t)h] != am.tm_n[(size_t)am.hmm_tm[(size_t)h]]) all_lr = false;
    if (knobs.no_lr == 1) all_lr = false;                                        // development: force the general path
    if (all_lr) {
        M.lrt.assign((size_t)am.n_tm * LRW, LZ);
        for (int t = 0; t < am.n_tm; ++t) {
            const float *tp = am.trP.data() + (size_t)t * MNn * MNn;
            const int n = am.tm_n[(size_t)t];
            for (int k = 1; k <= n - 1; ++k) M.lrt[(size_t)t * LRW + k - 1] = tp[(k - 1) * MNn + k];          // a_k
            for (int k = 1; k <= n - 2; ++k) M.lrt[(size_t)t * LRW + NEn + k] = tp[k * MNn + k];              // s_k
        }
    }
    return M;
}

// The device arc table, from the network's (or the decoder's own numbering of it).
//   TEE_FLAG   bit 30 of the in-label marks arcs whose HMM is a tee model.
//   the order  The decoder's OWN order of a state's arcs (XState): what every arrival walks first, then the arcs that enter a
//              model by descending w + tmax - phase X of the slot kernel walks a prefix of those.  Arc numbers never leave the
//              device (results carry labels, times and scores), and every arc has an instance of its own, so the order changes no
//              score; it can change which of two EQUAL-scored tokens a state keeps (the frontier item's number breaks the tie), which
//              the reference's own traversal order decides no better (tests: decode_certified).  (knob xsort 0: the file's order.)
//   SOLE_FLAG  (jd_search.h: REC_SOLE) the arc that enters a model and is the only arc of the table that leads to its destination -
//              its exit tokens recombine with nobody.  THE INVARIANT the kernels rely on: SOLE_FLAG is set if and only if (knob sole
//              0 aside: then never) all three hold -
//                1. the arc enters a model (its in-label is not 0),
//                2. the model is not a tee model (a tee model's pass-through arrives beside its exit token),
//                3. the destination has in-degree 1, counted over ALL arcs of this table - epsilon and tee arcs, arcs from the same
//                   source state and self-loops included.
//              k_search replaces the arrival's atomic max by a plain store for such arcs (the slot kernel keeps the atomic), and
//              their exit tokens place no bid.  Nothing on the device checks it: whatever adds another way INTO a state - arcs
//              composed lazily (jd_lazy.h: they never carry the flag), a start token put back into a running search - has to count
//              here, or recombination is lost without a sound.  tests/test_prep_cpu.py::test_prep_invariants asserts it.
//   xcut       k_search takes the cut where it pays - graphs whose rows are short throughout, like configs[1]'s: 99.7 % of its model
//              arcs sit in sorted rows, two batches in flight gain 10 % - and not where a few long rows carry the traffic:
//              trigram-shaped graphs have 85-87 % of their arcs in short rows, yet configs[3] loses 4 % to the item stage's extra
//              loads and the north-star graph gains nothing.
struct PrepArcs {
    std::vector<JdArc> arcs;
    std::vector<XState> xst;
    int64_t n_sorted = 0, n_model_all = 0;   // model arcs in sorted rows / of all rows, tee models included
    int64_t n_sole = 0, n_model = 0;         // arcs flagged SOLE / that carry a model
    int xcut = 0;
};
inline PrepArcs prep_arcs(const std::vector<int32_t> &row_ptr, const std::vector<JdArc> &arcs, int n_states, const jd_am &am,
                          const std::vector<float> &tmax0, const PrepKnobs &knobs)
{
    PrepArcs P;
    std::vector<JdArc> &darcs = P.arcs;
    darcs = arcs;
    for (JdArc &a : darcs)
        if (a.in > 0 && am.hmm_tee[(size_t)a.in - 1] > LZ) a.in |= TEE_FLAG;
    const bool xsort = knobs.xsort != 0;
    P.xst.resize((size_t)n_states);
    std::vector<std::pair<float, JdArc>> ent;
    for (int q = 0; q < n_states; ++q) {
        const int r0 = row_ptr[(size_t)q], r1 = row_ptr[(size_t)q + 1];
        XState &X = P.xst[(size_t)q];
        X.n_always = 0; X.n_entry = 0; X.wmax = LZ; X.n_model = 0;
        for (int i = 0; i < XNCAND; ++i) X.k[i] = LZ;
        ent.clear();
        const bool sort_row = xsort && r1 - r0 <= XSORT_MAX_ROW;
        int at = r0;
        for (int b = r0; b < r1; ++b) {
            const JdArc a = darcs[(size_t)b];
            const int inl = a.in & ~TEE_FLAG;
            if (inl != 0) { ++X.n_model; X.wmax = std::max(X.wmax, a.w); }
            if (sort_row && inl != 0 && !(a.in & TEE_FLAG)) ent.push_back({a.w + tmax0[(size_t)inl - 1], a});
            else darcs[(size_t)at++] = a;                          // (in place: `at` never passes b)
        }
        X.n_always = at - r0;
        std::stable_sort(ent.begin(), ent.end(), [](const std::pair<float, JdArc> &x, const std::pair<float, JdArc> &y) { return x.first > y.first; });
        X.n_entry = (int)ent.size();
        for (size_t i = 0; i < ent.size(); ++i) darcs[(size_t)at + i] = ent[i].second;
        for (int i = 0; i < XNCAND; ++i) if (xcand(i) < X.n_entry) X.k[i] = ent[(size_t)xcand(i)].first;
    }
    std::vector<int> indeg((size_t)n_states, 0);
    for (const JdArc &a : darcs) ++indeg[(size_t)a.to];
    const bool sole_on = knobs.sole != 0;
    for (JdArc &a : darcs)
        if ((a.in & ~TEE_FLAG) != 0) { ++P.n_model; if (sole_on && indeg[(size_t)a.to] == 1 && !(a.in & TEE_FLAG)) { a.in |= SOLE_FLAG; ++P.n_sole; } }
    for (const XState &X : P.xst) { P.n_sorted += X.n_entry; P.n_model_all += X.n_model; }
    P.xcut = (xsort && P.n_model_all > 0 && 20 * P.n_sorted >= 19 * P.n_model_all) ? 1 : 0;
    if (knobs.xcut >= 0) P.xcut = (knobs.xcut != 0 && xsort) ? 1 : 0;
    return P;
}

// The layout of a stream's per-state words (jd_search.h: StateRec): split - the arrival keys of all states in an array of their own,
// four states to a 64-byte line - where the graph's numbering puts the states of a chain side by side (an arc to the NEXT state
// number: the lexicon chains of a composed C.L.G written state after state - 42 % of the arcs of the bench graphs), joint where it
// does not (a graph numbered by its composition: what neighbours in number have in common is nothing, and every exit token would
// pay a second line).  (knob: 0 / 1 / 2.)  row_ptr and arcs in the decoder's numbering; both empty for a lazily composed network,
// whose n_states / n_arcs are capacities: joint records unless the knob says otherwise.
struct PrepSrec {
    unsigned stride = 32, arr = 16, estride = 32, par = 8;   // DecConst::srec_stride / srec_arr / srec_estride / srec_par
    int split = 0;                       // 0 joint, 1 split (both parities of a state together), 2 split by parity
    int64_t n_next = 0;                  // arcs that lead to the next state number
};
inline PrepSrec prep_srec_layout(const std::vector<int32_t> &row_ptr, const std::vector<JdArc> &arcs, int n_states, int64_t n_arcs, int knob)
{
    PrepSrec S;
    const bool have = !row_ptr.empty();
    if (have) S.n_next = prep_count_next(row_ptr, arcs, n_states);
    S.split = (have && n_arcs > 0 && 4 * S.n_next >= n_arcs) ? 2 : 0;
    if (knob >= 0) S.split = std::min(2, knob);
    const unsigned ns = (unsigned)n_states;
    S.stride = S.split ? 16u : 32u;
    S.arr = S.split ? 16u * ns : 16u;
    S.estride = S.split == 2 ? 8u : (S.split ? 16u : 32u);
    S.par = S.split == 2 ? 8u * ns : 8u;
    return S;
}

// The histogram's range (WFSTDecoderLite.cpp:76-82, Histogram.cpp:29-37); all 0 without histogram pruning.
struct PrepHist { int hist_min = 0, hist_max = 0, hist_nbins = 0; };
inline PrepHist prep_hist(float main_beam, int max_hyps)
{
    PrepHist H;
    if (max_hyps > 0) {
        float mn = (main_beam > 0.0) ? (float)(-main_beam - 800.0) : -1000.0f;
        H.hist_min = (int)(mn - 1.0);
        H.hist_max = (int)(200.0f + 1.0);
        H.hist_nbins = H.hist_max - H.hist_min + 1;
    }
    return H;
}

// The Path objects WFSTDecoderLite::propagateToken creates behind ONE token that arrives at state q (:497-509 inside
// the recursion of :533-541 and :583-599): one per labelled epsilon arc and per labelled arc of a tee model that leaves
// q, plus what arrives behind each of those arcs - with multiplicity, the recursion does not recombine.  Static as
// long as nothing prunes inside the closure, i.e. with the end and word beams off (the thresholds of :538, :591-596 are
// LOG_ZERO then).  Saturates at 2^20 (the rule's own mark is 10000).  false: the label-less part of the graph has a
// cycle (the reference would not come back from it).
inline bool closure_path_counts(const jd_net *net, const jd_am *am, std::vector<int> &P)
{
    const int nS = net->n_states;
    P.assign((size_t)nS, -1);
    std::vector<char> open((size_t)nS, 0);
    std::vector<std::pair<int, int>> stack;                           // (state, next arc)
    auto passes = [&](const JdArc &a) { return a.in == 0 || am->hmm_tee[(size_t)a.in - 1] > LZ; };
    for (int q0 = 0; q0 < nS; ++q0) {
        if (P[(size_t)q0] >= 0) continue;
        stack.assign(1, std::make_pair(q0, net->row_ptr[(size_t)q0]));
        open[(size_t)q0] = 1;
        while (!stack.empty()) {
            const int q = stack.back().first;
            int &a = stack.back().second;
            bool descended = false;
            for (; a < net->row_ptr[(size_t)q + 1]; ++a) {
                const JdArc &arc = net->arcs[(size_t)a];
                if (!passes(arc) || P[(size_t)arc.to] >= 0) continue;
                if (open[(size_t)arc.to]) return false;
                open[(size_t)arc.to] = 1;
                stack.push_back(std::make_pair(arc.to, net->row_ptr[(size_t)arc.to]));
                descended = true;
                break;
            }
            if (descended) continue;
            long long sum = 0;
            for (int b = net->row_ptr[(size_t)q]; b < net->row_ptr[(size_t)q + 1]; ++b) {
                const JdArc &arc = net->arcs[(size_t)b];
                if (passes(arc)) sum += (arc.out != 0 ? 1 : 0) + P[(size_t)arc.to];
            }
            P[(size_t)q] = (int)std::min<long long>(sum, 1 << 20);
            open[(size_t)q] = 0;
            stack.pop_back();
        }
    }
    return true;
}
