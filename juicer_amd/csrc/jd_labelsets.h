// jd_labelsets.h - exact label-set look-ahead of C.L (JD_LOOKAHEAD_SETS): host code only, plain C++ (no HIP), so
// that it can be compiled and tested without a device (tests/labelsets_driver.cpp).  Included by jd_compose.hip.  Everything
// in here is static: any number of translation units may include it.
//
// S(c) is the set of output labels on the first label-carrying arcs reachable from C.L state c through arcs without
// an output label (the reference: WFSTLabelPushingNetwork's label sets, WFSTNetwork.cpp:1505-2590).  cl_lookahead
// (jd_compose.hip) bounds S(c) by an interval of the caller's word numbers, which is exact only when the words are
// numbered in the lexicon tree's depth-first order.  Here the words are RELABELLED that way internally - a word's
// number is the order in which a depth-first walk from the initial state first meets it - so that the set of a tree
// node whose words occur nowhere else is one interval again, whatever numbers the caller gave them; what is left
// (a word with two pronunciations sits in two subtrees, shared suffixes) is kept as a sorted LIST per state:
//   lo[c], hi[c]   smallest and largest label of S(c), internal numbering (lo > hi: empty; {1, 0x7fffffff} and
//                  full[c]: "every label" - c lies on a cycle of label-less arcs or reaches one)
//   set_row / set_lab   CSR over the states: the sorted labels of the states whose set is NOT all of [lo, hi];
//                  an empty row says the interval is the set
// The relabelling is applied to C.L's output labels and to a private copy of G's input labels (fwd[]); G's output
// labels, which are what the composed graph carries, stay, so nothing outside the composition sees it.
#ifndef JD_LABELSETS_H
#define JD_LABELSETS_H

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <limits>
#include <utility>
#include <vector>

#include "jd_internal.h"

// The lists of all states together hold at most this many labels (4 bytes each on the device: 1 GiB, the size of
// the arc arena a lazily composed network gets by default, and within what an int32 CSR row can address); beyond
// it the computation fails with JD_ENOMEM instead of falling back to intervals.  (JD_LA_SET_MAX, a development
// knob, lowers it for the tests.)
#define JD_LA_SET_MAX (1LL << 28)

struct JdLabelSets {
    std::vector<int32_t> fwd, back;          // caller's label -> internal label (0 -> 0), and back
    std::vector<int32_t> lo, hi;             // per state, internal numbering
    std::vector<uint8_t> full, mayfin;       // per state: every label / a final C.L state is reachable without a label
    std::vector<int32_t> set_row, set_lab;   // lists (see above)
    std::vector<int32_t> multi;              // per state: index into runs, -1 if the set is one interval (or empty / full)
    std::vector<std::vector<std::pair<int32_t, int32_t>>> runs;   // the sets that are not one interval, as sorted disjoint runs
};

// max_label: the largest label the relabelling has to cover besides C.L's own (G's largest input label)
static int jd_label_sets(const jd_net *cl, int32_t max_label, int64_t max_list, JdLabelSets &R)
{
    const int S = cl->n_states;
    for (const JdArc &a : cl->arcs) {
        if (a.out < 0) return jd_fail(JD_EINVAL, "label-set look-ahead: negative output label %d in C.L", a.out);
        max_label = std::max(max_label, a.out);
    }
    if (max_label >= 0x7fffffff) return jd_fail(JD_EINVAL, "label-set look-ahead: labels are limited to 2^31 - 2");
    R.fwd.assign((size_t)max_label + 1, 0);
    R.full.assign((size_t)S, 0);
    // depth first from the initial state (then from whatever it does not reach): word numbers in the order of first
    // meeting, the states in post-order, and the states that see a label-less arc back into the walk's own stack
    std::vector<int32_t> post;
    post.reserve((size_t)S);
    {
        std::vector<char> st((size_t)S, 0);                            // 0 new, 1 on the stack, 2 done
        std::vector<std::pair<int, int>> stack;                        // (state, next arc)
        int32_t next = 0;
        for (int k = -1; k < S; ++k) {
            const int r = k < 0 ? cl->init : k;
            if (r < 0 || r >= S || st[(size_t)r]) continue;
            stack.push_back({r, cl->row_ptr[(size_t)r]});
            st[(size_t)r] = 1;
            while (!stack.empty()) {
                const int c = stack.back().first;
                int &a = stack.back().second;
                if (a == cl->row_ptr[(size_t)c + 1]) { st[(size_t)c] = 2; post.push_back(c); stack.pop_back(); continue; }
                const JdArc &arc = cl->arcs[(size_t)a];
                if (arc.out != 0) { if (!R.fwd[(size_t)arc.out]) R.fwd[(size_t)arc.out] = ++next; ++a; }
                else if (st[(size_t)arc.to] == 2) ++a;
                else if (st[(size_t)arc.to] == 1) { R.full[(size_t)c] = 1; ++a; }   // cycle of label-less arcs
                else { st[(size_t)arc.to] = 1; stack.push_back({arc.to, cl->row_ptr[(size_t)arc.to]}); }   // (a stays)
            }
        }
        for (int32_t x = 1; x <= max_label; ++x)                       // labels C.L does not have: behind the others
            if (!R.fwd[(size_t)x]) R.fwd[(size_t)x] = ++next;
        R.back.assign((size_t)max_label + 1, 0);
        for (int32_t x = 1; x <= max_label; ++x) R.back[(size_t)R.fwd[(size_t)x]] = x;
    }
    // "every label" spreads to every ancestor of a cycle state; the same sweeps find the states that reach a FINAL
    // C.L state through label-less arcs (LA_MAYFIN, jd_lazy.h).  Post-order: one sweep settles everything acyclic.
    R.mayfin.assign((size_t)S, 0);
    for (int c = 0; c < S; ++c) R.mayfin[(size_t)c] = cl->fin_w[(size_t)c] < std::numeric_limits<float>::infinity();
    for (bool changed = true; changed;) {
        changed = false;
        for (const int32_t c : post)
            for (int a = cl->row_ptr[(size_t)c]; a < cl->row_ptr[(size_t)c + 1]; ++a) {
                const JdArc &arc = cl->arcs[(size_t)a];
                if (arc.out != 0) continue;
                if (R.full[(size_t)arc.to] && !R.full[(size_t)c]) { R.full[(size_t)c] = 1; changed = true; }
                if (R.mayfin[(size_t)arc.to] && !R.mayfin[(size_t)c]) { R.mayfin[(size_t)c] = 1; changed = true; }
            }
    }
    // the sets, children first: a state that is not full reaches no cycle, so its children's sets are complete
    R.lo.assign((size_t)S, 0x7fffffff);
    R.hi.assign((size_t)S, 0);
    R.multi.assign((size_t)S, -1);
    R.runs.clear();
    int64_t total = 0;
    std::vector<std::pair<int32_t, int32_t>> tmp, merged;
    for (const int32_t c : post) {
        if (R.full[(size_t)c]) { R.lo[(size_t)c] = 1; R.hi[(size_t)c] = 0x7fffffff; continue; }
        tmp.clear();
        for (int a = cl->row_ptr[(size_t)c]; a < cl->row_ptr[(size_t)c + 1]; ++a) {
            const JdArc &arc = cl->arcs[(size_t)a];
            if (arc.out != 0) { const int32_t x = R.fwd[(size_t)arc.out]; tmp.push_back({x, x}); continue; }
            const size_t t = (size_t)arc.to;
            if (R.multi[t] >= 0) tmp.insert(tmp.end(), R.runs[(size_t)R.multi[t]].begin(), R.runs[(size_t)R.multi[t]].end());
            else if (R.lo[t] <= R.hi[t]) tmp.push_back({R.lo[t], R.hi[t]});
        }
        if (tmp.empty()) continue;
        std::sort(tmp.begin(), tmp.end());
        merged.clear();
        for (const auto &r : tmp) {
            if (!merged.empty() && r.first <= merged.back().second + 1) merged.back().second = std::max(merged.back().second, r.second);
            else merged.push_back(r);
        }
        R.lo[(size_t)c] = merged.front().first;
        R.hi[(size_t)c] = merged.back().second;
        if (merged.size() > 1) {
            for (const auto &r : merged) total += (int64_t)r.second - r.first + 1;
            if (total > max_list)
                return jd_fail(JD_ENOMEM, "label-set look-ahead: the label lists of C.L's states hold more than %lld labels "
                                          "(the bound, JD_LA_SET_MAX); interval look-ahead (no JD_LOOKAHEAD_SETS) has no such limit",
                               (long long)max_list);
            R.multi[(size_t)c] = (int32_t)R.runs.size();
            R.runs.push_back(merged);
        }
    }
    R.set_row.assign((size_t)S + 1, 0);
    R.set_lab.clear();
    R.set_lab.reserve((size_t)total);
    for (int c = 0; c < S; ++c) {
        if (R.multi[(size_t)c] >= 0)
            for (const auto &r : R.runs[(size_t)R.multi[(size_t)c]])
                for (int32_t x = r.first; x <= r.second; ++x) R.set_lab.push_back(x);
        R.set_row[(size_t)c + 1] = (int32_t)R.set_lab.size();
    }
    return JD_OK;
}

static int64_t jd_label_sets_bound()
{
    if (const char *e = jd_dev_env("JD_LA_SET_MAX")) { const long long v = atoll(e); if (v >= 0 && v <= JD_LA_SET_MAX) return v; }
    return JD_LA_SET_MAX;
}

// The body of jd_debug_cl_label_sets (the exported function is in jd_compose.hip; tests/labelsets_driver.cpp calls this one):
// S(c) of every C.L state as sorted CSR in the CALLER's label numbering - a state with "every label" gets the single entry -1 -
// and mayfin[c] (may be NULL).  *n_total = entries in all; when that is more than cap the call fails with JD_ENOMEM (n_total
// is set, row_ptr and labels are not written).
static int jd_label_sets_csr(const jd_net *cl, int64_t *row_ptr, int32_t *labels, int64_t cap, int64_t *n_total, uint8_t *mayfin)
{
    if (!cl || !row_ptr || !n_total || (!labels && cap > 0)) return jd_fail(JD_EINVAL, "jd_debug_cl_label_sets: null argument");
    if (cl->lazy_dev) return jd_fail(JD_EINVAL, "jd_debug_cl_label_sets: not for a lazily composed network");
    JdLabelSets R;
    const int rc = jd_label_sets(cl, 0, jd_label_sets_bound(), R);
    if (rc) return rc;
    const int S = cl->n_states;
    int64_t total = 0;
    for (int c = 0; c < S; ++c) {
        if (R.full[(size_t)c]) total += 1;
        else if (R.multi[(size_t)c] >= 0) total += R.set_row[(size_t)c + 1] - R.set_row[(size_t)c];
        else if (R.lo[(size_t)c] <= R.hi[(size_t)c]) total += (int64_t)R.hi[(size_t)c] - R.lo[(size_t)c] + 1;
    }
    *n_total = total;
    if (total > cap) return jd_fail(JD_ENOMEM, "jd_debug_cl_label_sets: %lld labels in all, room for %lld", (long long)total, (long long)cap);
    int64_t n = 0;
    for (int c = 0; c < S; ++c) {
        row_ptr[c] = n;
        if (R.full[(size_t)c]) labels[n++] = -1;
        else {
            const int64_t first = n;
            if (R.multi[(size_t)c] >= 0)
                for (int32_t i = R.set_row[(size_t)c]; i < R.set_row[(size_t)c + 1]; ++i) labels[n++] = R.back[(size_t)R.set_lab[(size_t)i]];
            else
                for (int64_t x = R.lo[(size_t)c]; x <= R.hi[(size_t)c]; ++x) labels[n++] = R.back[(size_t)x];
            std::sort(labels + first, labels + n);
        }
        if (mayfin) mayfin[c] = R.mayfin[(size_t)c];
    }
    row_ptr[S] = n;
    return JD_OK;
}

#endif
