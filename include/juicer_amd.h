/*
 * juicer_amd.h - C ABI of the MI355X-native WFST Viterbi decoder.
 *
 * This is the drop-in boundary for ONE path of idiap/juicer: the
 * WFSTDecoderLite token-passing search + HTKFlatModels diagonal-GMM scoring,
 * behind Juicer's IDecoder / DecoderBatchTest seam.  Every entry point cites
 * the reference interface it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - Every function that can fail returns 0 on success or a negative JD_E*
 *     code; jd_last_error() returns a human readable message for the calling
 *     thread's most recent failure.  (The reference calls Torch3 error() =
 *     print + exit(); a library must not exit, so the same conditions are
 *     reported as codes instead.)
 *   - All "host" pointers are only read during the call; nothing is retained.
 *   - There is NO CPU fallback: if no gfx950 device / HIP runtime is usable
 *     jd_dec_create() fails with JD_ENODEV.
 */
#ifndef JUICER_AMD_H
#define JUICER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JD_OK        0
#define JD_EINVAL   -1   /* bad argument                                        */
#define JD_ENODEV   -2   /* no usable HIP device                                */
#define JD_EHIP     -3   /* HIP runtime call failed                             */
#define JD_ENOMEM   -4   /* a device arena (slots/paths/frontier) overflowed     */
#define JD_EHIST    -5   /* Histogram::addScore - score > maxScore
                            (Histogram.cpp:78-79 is fatal in the reference)     */
#define JD_ESTATE   -6   /* call order violated (e.g. push before init)          */
#define JD_EFORMAT  -7   /* text loader: malformed FSM / MMF input               */

/* LOG_ZERO of the reference: Torch3 defines it as -FLT_MAX (not -inf). */
#define JD_LOG_ZERO (-3.402823466e+38f)

typedef struct jd_net jd_net;   /* replaces Juicer::WFSTNetwork  (WFSTNetwork.h:110-245)   */
typedef struct jd_am  jd_am;    /* replaces Juicer::HTKFlatModels (HTKFlatModels.h)         */
typedef struct jd_dec jd_dec;   /* replaces Juicer::WFSTDecoderLite (WFSTDecoderLite.h:77) */

/* ------------------------------------------------------------------ network */

/*
 * Build a network from arcs in FSM *file order* with the raw file weights,
 * applying the load-time arithmetic of WFSTNetwork::WFSTNetwork(text)
 * (WFSTNetwork.cpp:371-616):
 *     weight = (float)(-w_file * lm_scale); if (out > 0) weight += ins_penalty
 *     final weight = (float)(-w_file * lm_scale)
 *     initial state = source state of the first arc
 * Arcs of one source state must be contiguous (getTransitions(),
 * WFSTNetwork.cpp:709-721, returns "first arc + count"); JD_EFORMAT otherwise.
 * in/out labels are integers; 0 is epsilon; in-label i>0 selects HMM i-1
 * (WFSTDecoderLite.cpp:754).  Auxiliary symbols must already be removed.
 */
int jd_net_create_arcs(jd_net **out, int64_t n_arcs,
                       const int32_t *from, const int32_t *to,
                       const int32_t *in, const int32_t *outl,
                       const float *w_file,
                       int32_t n_final, const int32_t *fstate, const float *fweight_file,
                       float lm_scale, float ins_penalty);

/*
 * Build a network from an already prepared CSR (weights are used as given,
 * i.e. they are the reference's in-memory transitions[].weight values).
 * row_ptr has n_states+1 entries.
 */
int jd_net_create_csr(jd_net **out, int32_t n_states, int32_t init_state,
                      const int32_t *row_ptr, const int32_t *to, const float *w,
                      const int32_t *in, const int32_t *outl,
                      int32_t n_final, const int32_t *fstate, const float *fweight);

/* AT&T text FSM file (WFSTNetwork.cpp:403-560); symbol files are optional and
 * only used for the range checks of WFSTNetwork.cpp:566-584. */
int jd_net_load_fsm(jd_net **out, const char *fsm_path, const char *insyms_path,
                    const char *outsyms_path, float lm_scale, float ins_penalty);

/* Juicer's binary network cache "<fsm>.bin" (JWNT), which juicer.cpp:854-866 prefers over the
 * text FSM when it exists: WFSTNetwork(lmScale, insPenalty) + readBinary (WFSTNetwork.cpp:333-359,
 * 1228-1365).  Arc weights are stored without scale and penalty and get `w *= lm_scale`, then
 * `+= ins_penalty` on arcs with an output label; final-state weights are used as stored.
 * Embedded alphabets are skipped (auxiliary '#' symbols are an error, as for the text loader). */
int jd_net_load_jwnt(jd_net **out, const char *path, float lm_scale, float ins_penalty);
/* WFSTNetwork::writeBinary (WFSTNetwork.cpp:1106-1225, juicer.cpp:879-882 -writeBinaryFiles):
 * takes the penalty and the scale the network was built with off the arc weights again;
 * no alphabets are written. */
int jd_net_save_jwnt(const jd_net *n, const char *path);

/* Read back the prepared CSR (host copies; any pointer may be NULL) - used by parity tests.
 * fin_w has n_states entries, +inf for non-final states. */
int jd_net_get_csr(const jd_net *n, int32_t *row_ptr, int32_t *to, float *w, int32_t *in, int32_t *outl,
                   float *fin_w);

int64_t jd_net_num_arcs(const jd_net *n);     /* WFSTNetwork::getNumTransitions */
int32_t jd_net_num_states(const jd_net *n);   /* WFSTNetwork::getNumStates      */
int32_t jd_net_init_state(const jd_net *n);   /* WFSTNetwork::getInitState      */
void    jd_net_destroy(jd_net *n);

/*
 * Dynamic composition, first step (WFSTOnTheFlyDecoder, juicer.cpp:594-598): C.L and G
 * are handed over apart - cl loaded like the reference's clNetwork (scale 1.0, juicer.cpp:933-940), g like
 * its gNetwork (lmScaleFactor; arcs of a state sorted by input label, one per label, the back-off
 * epsilon first: WFSTSortedInLabelNetwork, WFSTNetwork.cpp:2693-2710) - and composed ON THE DEVICE into
 * an ordinary network for jd_dec_create: reachable (C.L state, G state) pairs only, G advanced by a
 * binary search for the C.L arc's output label (WFSTOnTheFlyDecoder.cpp:3106-3159), back-off epsilons
 * taken right after a word only (WFSTOnTheFlyDecoder.cpp:1590-1622), lexicon branches that hold no word
 * the G state has an arc for left out (label look-ahead, WFSTNetwork.cpp:1505-2590, on label intervals:
 * tight when words are numbered in the lexicon tree's depth-first order).  Exact definition and the
 * state / arc numbering: csrc/jd_compose.hip.  max_states / max_arcs bound the result (0: a default
 * derived from the inputs); JD_ENOMEM names the one that was too small.  There is no CPU path.
 * pushing: the reference's -pushing (doLabelAndWeightPushing, juicer.cpp:240, 931-935) is JD_PUSH_WEIGHTS |
 * JD_PUSH_LABELS.  JD_PUSH_WEIGHTS: the best grammar weight reachable below a lexicon-tree node is paid on the way
 * into it, so the beam prunes on it; path totals are the same up to float association.  JD_PUSH_LABELS: C.L is
 * composed with its output labels pushed towards the initial state (jd_net_push_labels).
 * JD_LOOKAHEAD_SETS (a third bit of `pushing`, free to combine with the other two; off by default, and without it
 * every result is what it was before the bit existed): the look-ahead works on label SETS, as the reference's does,
 * instead of intervals of the caller's word numbers.  S(c) is the set of output labels on the first label-carrying
 * arcs reachable from C.L state c through arcs without an output label.  With the bit, a label-less arc
 * c -i:eps-> c' is followed at grammar state g iff g has an arc whose input label is in S(c') (or a final C.L state
 * is reachable from c' without a label and g is final - unchanged), and JD_PUSH_WEIGHTS pays the best weight among
 * g's arcs with a label in S(c), 0 if there is none.  States on a cycle of label-less arcs, and their ancestors, keep
 * "every label".  The composed network then does not depend on how the words are numbered: vocabularies numbered by
 * spelling and words with several pronunciations get the graph a depth-first numbering of a pure tree gets from the
 * intervals.  Costs host time (the sets) and device memory for the label lists of the states whose set is no interval
 * under the internal renumbering; those lists hold at most 2^28 labels in all (JD_ENOMEM names the bound).
 */
#define JD_PUSH_WEIGHTS 1
#define JD_PUSH_LABELS 2
#define JD_LOOKAHEAD_SETS 4
int jd_net_compose(jd_net **out, const jd_net *cl, const jd_net *g, int32_t device,
                   int64_t max_states, int64_t max_arcs, int32_t pushing);

/*
 * Label pushing on a C.L transducer (the reference: WFSTLabelPushingNetwork gives every transition the set of output
 * labels that can follow it, WFSTNetwork.cpp:1643-1764, and the on-the-fly decoder takes the G transition as soon as
 * the set is one label): every output label moves towards the initial state, up to the first arc behind which it is
 * the only label that can follow.  The result has the same states, arcs and weights and accepts the same label
 * sequences at the same costs; a hypothesis' word-end times become the frames in which its words were identified.
 * Host code (no device needed); exact rule: csrc/jd_compose.hip, cl_push_labels.  n_moved (may be NULL): labels moved.
 */
int jd_net_push_labels(jd_net **out, const jd_net *cl, int64_t *n_moved);

/*
 * Diagnostics / tests (host code, no device): the label sets S(c) of JD_LOOKAHEAD_SETS for every state of a C.L
 * transducer, as CSR - row_ptr[n_states + 1], labels[cap] - sorted, in the caller's label numbering; a state with
 * "every label" gets the single entry -1.  mayfin[n_states] (may be NULL): a final state is reachable from c through
 * label-less arcs.  *n_total = the number of entries; JD_ENOMEM (with *n_total set) when cap is too small, or when
 * the sets that are no interval under the internal renumbering hold more than 2^28 labels (the bound of the option).
 */
int jd_debug_cl_label_sets(const jd_net *cl, int64_t *row_ptr, int32_t *labels, int64_t cap, int64_t *n_total, uint8_t *mayfin);

/*
 * Diagnostics / tests (host code, no device): the look-ahead INTERVALS the composition uses without JD_LOOKAHEAD_SETS,
 * for every state of a C.L transducer - lo[n_states], hi[n_states]: the smallest and largest output label of the first
 * label-carrying arcs reachable from c through label-less arcs, in the caller's numbering (lo = 2^31 - 1, hi = 0: none;
 * lo = 1, hi = 2^31 - 1: "every label", c lies on a cycle of label-less arcs or reaches one) - and mayfin[n_states] as
 * above.
 */
int jd_debug_cl_lookahead(const jd_net *cl, int32_t *lo, int32_t *hi, uint8_t *mayfin);

/*
 * Dynamic composition proper (WFSTOnTheFlyDecoder: C.L o G expanded where the search goes, never as a
 * whole): the network this returns holds only its start state; decoders created on it expand a composed
 * state - same expansion step as jd_net_compose, one state at a time - when a token first enters an arc
 * that leads to it (csrc/jd_lazy.h).  What has been expanded stays, shared by every decoder and stream on
 * the network, so later utterances find most of what they need.  `am` says which input labels are tee
 * models; max_states / max_arcs are the room the network may grow into (0: 2^22 states, 2^24 arcs;
 * see jd_net_lazy_set_high_water for what happens when it fills up).  The decoder must be created on the same device; the
 * network has no arc table to read back (jd_net_get_csr / jd_net_save_jwnt refuse it).  Results are those
 * of decoding on jd_net_compose's network (pushing: as there, applied arc by arc as states are expanded).
 * There is no CPU path.
 */
int jd_net_create_lazy(jd_net **out, const jd_net *cl, const jd_net *g, const jd_am *am, int32_t device,
                       int64_t max_states, int64_t max_arcs, int32_t pushing);
/* Bounded look-ahead memory (the reference: an LRU cache of composed transitions, WFSTOnTheFlyDecoder.h:210-371).
 * Eviction here is by arena GENERATION: when an utterance (or batch) begins while no stream of any decoder on the
 * network is inside one, and the arena is past its high-water mark - `fraction` of either capacity, default 0.9 -
 * or has run out of room, everything expanded so far is dropped and the arena starts again from the start state.
 * A batch that runs out of room under way is decoded again on a fresh generation, so JD_ENOMEM means ONE batch
 * needs more than the capacities; it is never a sticky state of the network.  jd_net_lazy_generation counts the
 * generations begun so far (0: nothing has been dropped yet). */
int jd_net_lazy_set_high_water(jd_net *n, double fraction);
int jd_net_lazy_generation(const jd_net *n, int64_t *generation);
/* The same by hand: forget everything expanded so far.  JD_ESTATE while a stream of a decoder on the network is
 * inside an utterance. */
int jd_net_lazy_reset(jd_net *n);
/* composed states and arcs materialised so far */
int jd_net_lazy_size(const jd_net *n, int64_t *states, int64_t *arcs);

/* ---------------------------------------------------------- acoustic models */

/*
 * Build models from HTK-level parameters, applying the load-time arithmetic of
 * HTKModels::addVarVec (HTKModels.cpp:835-870), addGMM (:600-676),
 * addTransMatrix (:873-974), addHMM tee detection (:581-593),
 * createTrPandSEIndex (:2330-2390) and HTKFlatModels::init
 * (HTKFlatModels.cpp:94-177):
 *     det  = -0.5*(D*LOG_2_PI + sum_k logf(var_k))  [float accumulation] + logf(weight)
 *     ivar = (float)(1.0/var)
 *     trP[i][j] = logf(a_ij) if a_ij > 0 else LOG_ZERO; SEIndex; teeWeight
 * Layout: weight[n_gmm*max_mix], mean/var[n_gmm*max_mix*D] (component major),
 * n_mix[n_gmm]; hmm_nstates[n_hmm] (incl. entry+exit), hmm_gmm[n_hmm*max_n]
 * (gmm id per state, -1 for entry/exit), hmm_tm[n_hmm]; tm_nstates[n_tm],
 * transp[n_tm*max_n*max_n] row-major a_ij.
 */
int jd_am_create_htk(jd_am **out, int32_t D, int32_t n_gmm, int32_t max_mix,
                     const int32_t *n_mix, const float *weight,
                     const float *mean, const float *var,
                     int32_t n_hmm, int32_t max_n, const int32_t *hmm_nstates,
                     const int32_t *hmm_gmm, const int32_t *hmm_tm,
                     int32_t n_tm, const int32_t *tm_nstates, const float *transp);

/*
 * Build models from the PREPARED arrays of a loaded HTKFlatModels / HTKModels object - what
 * `WFSTDecoderLite(network, models, ...)` (WFSTDecoderLite.h:81-89) is handed by juicer.cpp:577-586:
 * det = fDets, mean = fMeans, ivar = fVars (inverse variances) of HTKFlatModels.h:48-52 re-laid as
 * [n_gmm][max_mix] / [n_gmm][max_mix][D]; hmm_tee[h] = getTeeLogProb(h) (Models.h:61); trP[t] =
 * getTransMat(h) rows (Models.h:63, [n_tm][max_n][max_n], LOG_ZERO where there is no transition),
 * se[t][j] = getSEIndex(h)[j] (Models.h:64, [n_tm][max_n][2]).  Nothing is recomputed.
 * include/juicer_amd_decoder.hpp's exact-signature constructor fills these from an IModels*.
 */
int jd_am_create_flat(jd_am **out, int32_t D, int32_t n_gmm, int32_t max_mix, const int32_t *n_mix,
                      const float *det, const float *mean, const float *ivar,
                      int32_t n_hmm, int32_t max_n, const int32_t *hmm_nstates,
                      const int32_t *hmm_gmm, const int32_t *hmm_tm, const float *hmm_tee,
                      int32_t n_tm, const int32_t *tm_nstates, const float *trP, const int16_t *se);

/* HTK MMF text (HTKModels::Load, HTKModels.cpp:221-282): the subset the reference's
 * flex/bison front-end accepts (htkparse.l.lpp:21-268, htkparse.y.ypp:113-147,414-685):
 * ~o, ~v (ignored), ~s, ~t, ~h with shared or inline states / <TRANSP>, <NUMMIXES>/<MIXTURE>
 * or the implicit single mixture, optional <GCONST>.  HMM index = order of the ~h macros. */
int jd_am_load_mmf(jd_am **out, const char *mmf_path);
/* HTKModels::Load(phonesListFName, priorsFName, statesPerModel) (HTKModels.cpp:74-218): hybrid ANN / HMM
 * models - one HMM per phone, states_per_model states each (entry and exit included), one shared
 * transition matrix (1.0 into the first emitting state, 0.5 / 0.5 self loop / forward); the feature vector
 * holds one log posterior per phone and an emitting state scores x[phone] - log(prior[phone])
 * (HTKModels.cpp:481-512, HTKFlatModels.cpp:190-222).  priors: n_phones values as read from the priors
 * file (the phone list only gives names). */
int jd_am_create_hybrid(jd_am **out, int32_t n_phones, const float *priors, int32_t states_per_model);

/* Neural acoustic models: jd_am_create_hybrid's models (same topology, same priors, same refusals: JD_FLOW_RESIDENT, JD_SCORE_FAST,
 * jd_am_save_jmbi, tile lists) with the NETWORK that yields the log posteriors, so that the caller pushes feature vectors of in_dim
 * values (jd_am_vec_size) and the device runs the forward pass: a fused kernel behind every scoring call of every entry point
 * (batches, streaming pushes, jd_streams_push, the broker, jd_multi_*, the C++ adapter).  n_layers >= 1 fully connected layers;
 * width[n_layers], the last equal to n_phones; act[n_layers - 1]: the HIDDEN layers' activations (NULL when n_layers == 1);
 * weight[l]: [width[l]][K_l] row-major with K_0 = in_dim, K_l = width[l - 1]; bias[l]: [width[l]].  The outputs of the last layer
 * are the logits z of a log-softmax, and an emitting state of phone j scores (z[j] - logZ) - log(prior[j]).
 * Numerics (csrc/jd_mlp.h defines them, jd_am_mlp_forward_host runs them on the host, and the device equals it bit for bit): a
 * linear output is ONE fmaf chain from the bias, k ascending; RELU y > 0 ? y : 0; SIGMOID 1.0f / (1.0f + expf(-y)); logZ is the
 * chain of HTKFlatModels::logAdd over z[0], z[1], ... from JD_LOG_ZERO.  A row's result depends on that row alone.
 * Limits (JD_EINVAL names the one exceeded): in_dim and every width 1 .. 1024, 1 .. 16 layers.  Context splicing is the caller's. */
#define JD_ACT_LINEAR  0
#define JD_ACT_RELU    1
#define JD_ACT_SIGMOID 2
int jd_am_create_mlp(jd_am **out, int32_t n_phones, const float *priors, int32_t states_per_model, int32_t in_dim,
                     int32_t n_layers, const int32_t *width, const int32_t *act, const float *const *weight,
                     const float *const *bias);
/* The network's shape: width[n_layers] and act[n_layers] (the last act is JD_ACT_LINEAR) - up to 16 entries; any pointer may be
 * NULL.  JD_ESTATE for models without a network. */
int jd_am_mlp_info(const jd_am *a, int32_t *in_dim, int32_t *n_layers, int32_t *width, int32_t *act);
/* A network and its priors as a file of this project's own (little-endian): "JMLP", u32 version 1, i32 n_phones,
 * states_per_model, in_dim, n_layers, i32 width[n_layers], i32 act[n_layers] (the last 0), f32 priors[n_phones], then per layer
 * f32 weight[width][K], f32 bias[width].  Loading a file that is truncated, malformed or longer than its header says: JD_EFORMAT. */
int jd_am_save_mlp(const jd_am *a, const char *path);
int jd_am_load_mlp(jd_am **out, const char *path);
/* The forward pass on its own.  frames: n_frames x in_dim; logpost: n_frames x n_phones log posteriors z - logZ (no priors) - from
 * HIP device `device`, and from the host twin (needs no device). */
int jd_am_mlp_forward(const jd_am *a, int32_t device, const float *frames, int32_t n_frames, float *logpost);
int jd_am_mlp_forward_host(const jd_am *a, const float *frames, int32_t n_frames, float *logpost);
/* ... and a layer of it, to place a mismatch: out = n_frames x width[layer], the activations behind layer `layer` (the raw logits
 * for the last).  on_device != 0: the kernel's, from HIP device `device`; 0: the host twin's (device is ignored). */
int jd_debug_mlp_activations(const jd_am *a, int32_t device, int32_t on_device, const float *frames, int32_t n_frames, int32_t layer,
                             float *out);
/* ... and its time: the scoring launch of these models (launch_gmm's branch, max_blocks as there) on n_frames rows, `warmup` launches
 * unmeasured, then ms[iters] - one launch each between two events.  tools/mlp_bench.py. */
int jd_debug_mlp_time(const jd_am *a, int32_t device, const float *frames, int32_t n_frames, int32_t max_blocks, int32_t warmup,
                      int32_t iters, float *ms);

/* TIED hybrid and neural models: what a large-vocabulary hybrid ANN / HMM recogniser has - a context-dependent HMM set of any
 * topology whose emitting states are tied to a few thousand states (senones), and one network output per tied state.
 * `topology` is any set of GMM models (jd_am_load_mmf, jd_am_load_jmbi, jd_am_create_htk / _flat); it is only read during the call.
 * The new models take its HMMs, their state tying (which tied state an emitting state scores with), the transition matrices with
 * their tee models, the HMM names, jd_am_num_gmms and jd_am_max_states - and none of its Gaussians (jd_am_max_mix is 1, and
 * jd_am_get_flat fills det alone: there are no means or variances, placeholders neither).  priors: one per tied state
 * (jd_am_num_gmms(topology) values); an emitting state tied to g scores logpost[g] - log(priors[g]).  They are hybrid models: what
 * hybrid models refuse (JD_FLOW_RESIDENT, JD_SCORE_FAST, jd_am_save_jmbi, tile lists) these refuse.  JD_EINVAL, naming the argument:
 * a NULL argument, a `topology` that is itself hybrid or neural, a prior that is not positive.
 * jd_am_create_hybrid_tied: the caller pushes vectors of jd_am_num_gmms log posteriors (jd_am_vec_size = jd_am_num_gmms).
 * jd_am_create_mlp_tied: jd_am_create_mlp's arguments for the network; the caller pushes vectors of in_dim features.  in_dim and
 * the hidden widths 1 .. 1024, the LAST width = jd_am_num_gmms(topology), 1 .. 16384 (JD_MLP_MAX_OUT).  jd_am_mlp_info,
 * jd_am_mlp_forward(_host), jd_debug_mlp_activations, jd_debug_mlp_time, jd_am_score_frames and jd_debug_score_rows serve them.
 * Numerics: layers as above.  logZ is NOT one serial chain over thousands of outputs but (csrc/jd_mlp.h) 128 interleaved partial
 * chains - p[c] = the logAdd chain from JD_LOG_ZERO over z[c], z[c + 128], ... for c < min(128, P) - and the logAdd chain over
 * p[0], p[1], ...; a constant of the numerics, whatever the rows, the launch or the device.  Host twin and device agree bit for bit.
 * jd_am_save_mlp on such models writes JMLP version 2 - the same layout with states_per_model = 0 and n_phones = the number of
 * outputs; no topology - which jd_am_load_mlp_tied reads beside a topology (JD_EINVAL when the outputs are not its tied states).
 * Each loader answers the other's version with JD_EFORMAT and the name of the loader that reads it. */
int jd_am_create_hybrid_tied(jd_am **out, const jd_am *topology, const float *priors);
int jd_am_create_mlp_tied(jd_am **out, const jd_am *topology, const float *priors, int32_t in_dim, int32_t n_layers,
                          const int32_t *width, const int32_t *act, const float *const *weight, const float *const *bias);
int jd_am_load_mlp_tied(jd_am **out, const jd_am *topology, const char *path);

/* bf16 neural models: reduced precision is a property of the MODEL, not a decoder mode.  jd_am_mlp_to_bf16 makes, from models with
 * a network (plain or tied; `src` is only read), new models of the same kind - same topology, priors, names and limits - whose
 * weights are src's rounded to bf16 (round to nearest even); biases and log priors stay f32.  Every entry point serves them with no
 * mode set (batches, scoring ahead, streaming pushes, jd_streams_push, the broker, jd_multi_*, the C++ adapter), on their own kernels
 * (bf16 matrix instructions, 32-row tiles, half the weight bytes); what hybrid models refuse they refuse, JD_SCORE_FAST included.
 * Converting a bf16 model again gives an equal model.  JD_EINVAL for a NULL argument, JD_ESTATE for models without a network.
 * Numerics (csrc/jd_mlp_bf16.h defines them; jd_am_mlp_forward_host and jd_debug_mlp_activations(on_device = 0) run the host twin):
 * every layer's input - the caller's features too - is rounded to bf16; a linear output is (float)(bias + sum_k x[k] w[k]) with the
 * sum in double; RELU / SIGMOID as above in f32; a hidden activation is rounded to bf16 (jd_debug_mlp_activations returns that
 * value: the low 16 bits of each float are zero); the logits stay f32, and logZ, z - logZ and - log(prior) are exactly those above.
 * The DEVICE is held to the twin by a bound in the linear part - |device - double sum| <= 2 (K + 1) 2^-23 (|bias| + sum_k |x[k] w[k]|):
 * the order and rounding of the sums inside a bf16 matrix instruction are not documented - and bit for bit in the rest: the log
 * posteriors are the logZ chain over the device's own logits, a hidden activation handed on is the bf16 value
 * jd_debug_mlp_activations(on_device = 1) returns, and a row's result depends on that row alone, whatever the batch or the launch
 * (pushes equal batches).  jd_am_save_mlp on a bf16 model writes an ordinary JMLP file (version 1 or 2) holding the rounded
 * weights as f32: loading it gives f32 models, converting those gives back equal bf16 models.  jd_am_mlp_info is unchanged.
 * jd_am_mlp_precision: JD_MLP_F32, JD_MLP_BF16, or -1 for models without a network. */
#define JD_MLP_F32  0
#define JD_MLP_BF16 1
int jd_am_mlp_to_bf16(const jd_am *src, jd_am **out);
int32_t jd_am_mlp_precision(const jd_am *a);

/* SPLICED neural models: the window of frames that a hybrid network takes is gathered on the device, in the input stage of the
 * network's kernel.  Splicing is a property of the MODEL, like bf16: jd_am_mlp_splice makes, from models with a network (plain or
 * tied, f32 or bf16; `src` is only read), new models with the same network, topology, priors and precision whose feature vectors
 * are single FRAMES of D = in_dim / C values, C = left + right + 1.  The network's input for frame t of an utterance of T frames is
 *   x[c D + d] = frame[clamp(t + c - left, 0, T - 1)][d]     c = 0 .. C - 1
 * - the oldest frame first, the first and the last frame repeated at the edges - and after the gather the arithmetic is the parent's:
 * a spliced model on raw frames gives, BIT FOR BIT (host twin and device, f32 and bf16), what its parent gives on the same frames
 * spliced by the caller.  Splicing and jd_am_mlp_to_bf16 commute.  (0, 0) is accepted and behaves like the parent.
 * JD_EINVAL, naming the cause: models without a network, a negative left or right, an in_dim that is no multiple of C, models
 * that are spliced already.
 * jd_am_vec_size and jd_dec_info report D; jd_am_mlp_info still reports the network's in_dim.  jd_am_mlp_context: (left, right),
 * (0, 0) for an unspliced network, JD_EINVAL for models without one.  jd_am_save_mlp writes the ordinary JMLP file of the network
 * (version 1 or 2): the format has no context field, the caller splices again after loading.
 * What serves them: jd_am_mlp_forward(_host), jd_debug_mlp_activations, jd_debug_mlp_time and jd_am_score_frames (the frames of a
 * call are ONE utterance), jd_debug_score_rows_span, jd_decode_batch(_device) in the default flow and in JD_FLOW_SERIAL with or
 * without jd_dec_prefetch_scores (an utterance is frames [ustart, ustart + ulen) of the buffer: windows clamp to it), jd_multi_*,
 * and jd_stream_init / _push / _finish for one stream, hence the C++ adapter.  A live stream holds back the last `right` frames
 * pushed: a frame is scored and searched once `right` more have arrived (a push may search nothing), jd_stream_finish searches the
 * rest with the right edge clamped, and every count of frames the streaming calls report - chunks, PARTIAL_DECODING's schedule,
 * times in traces, jd_streams_best / _final - is one of SEARCHED frames.  jd_stream_held_frames: frames pushed and not yet searched
 * (0 for every other kind of model).
 * Refused with JD_EINVAL, naming splicing: jd_streams_push with a stream of such a decoder, jd_broker_create on one, and
 * jd_debug_score_rows (jd_debug_score_rows_span takes the spans); JD_FLOW_RESIDENT refuses them as it does every hybrid model. */
int jd_am_mlp_splice(const jd_am *src, int32_t left, int32_t right, jd_am **out);
int jd_am_mlp_context(const jd_am *a, int32_t *left, int32_t *right);

/* Juicer's binary model cache "<mmf>.bin" (JMBI), preferred by juicer.cpp:778-784:
 * HTKModels::readBinary (HTKModels.cpp:1110-1233) + HTKFlatModels::init.  The derived values in
 * the file (sumLogVarPlusNObsLog2Pi, logCompWeights, transition logProbs) are used as stored. */
int jd_am_load_jmbi(jd_am **out, const char *path);
/* HTKModels::output(fName, true) (HTKModels.cpp:1044-1105, juicer.cpp:791-795). */
int jd_am_save_jmbi(const jd_am *a, const char *path);

int32_t jd_am_num_hmms(const jd_am *a);       /* IModels::getNumHMMs       (Models.h:57) */
int32_t jd_am_num_gmms(const jd_am *a);
int32_t jd_am_vec_size(const jd_am *a);       /* IModels::getInputVecSize  (Models.h:60) */
int32_t jd_am_max_states(const jd_am *a);
int32_t jd_am_max_mix(const jd_am *a);
int32_t jd_am_num_transmats(const jd_am *a);
/* topology read-back: hmm_nstates[n_hmm], hmm_gmm[n_hmm*max_states], hmm_tm[n_hmm], n_mix[n_gmm] */
int jd_am_get_topology(const jd_am *a, int32_t *hmm_nstates, int32_t *hmm_gmm, int32_t *hmm_tm, int32_t *n_mix);
/* Read back prepared parameters (host copies) - used by parity tests. */
int jd_am_get_flat(const jd_am *a, float *det, float *mean, float *ivar);
int jd_am_get_trans(const jd_am *a, float *trP, int16_t *se, float *tee);
void jd_am_destroy(jd_am *a);

/* ------------------------------------------------------------------ decoder */

typedef struct jd_stats {          /* WFSTDecoderLite.cpp:231-241 + build counters */
    int32_t n_frames;
    int64_t tot_active_emit_hyps;  /* totalActiveEmitHyps */
    int64_t tot_active_end_hyps;   /* totalActiveEndHyps  */
    int64_t tot_active_models;     /* totalActiveModels   */
    int64_t tot_proc_emit_hyps;    /* totalProcEmitHyps   */
    int64_t tot_proc_end_hyps;     /* totalProcEndHyps    */
    /* work the GPU path actually did: at most the reference's figures (only the best tokens
     * per destination state are expanded) and, with the inline closure, slightly run-dependent */
    int64_t tot_arcs_visited;      /* out-arcs visited by propagateToken (A)      */
    int64_t tot_paths;             /* Path records created (Wd)                    */
    int64_t tot_insts_in;          /* instances processed by internal propagation (Mdl) */
    int64_t ties;                  /* equal-score recombinations seen (oracle only; 0 on GPU) */
    /* what the kernels really touched - the figures above are the REFERENCE's counts (tot_insts_in includes candidates that
     * never become a record here, tot_arcs_visited the arcs a prefix walk accounts for without reading them); these price
     * the bytes the DESIGN moves (bench.py: roofline.design_bytes_per_launch): */
    int64_t tot_recs_read;         /* phase A: instance records read */
    int64_t tot_new_attached;      /* phase A: newly entered arcs taken up from the new-arc list (attachNetInst) */
    int64_t tot_recs_written;      /* phase A: records written to the next frame's list */
    int64_t tot_entry_items;       /* phase A: entry tokens pulled (the winning frontier item is gathered) */
    int64_t tot_items_expanded;    /* phase X: frontier items taken up (exit tokens, closure items, slices) */
    int64_t tot_arcs_walked;       /* phase X: arc records loaded */
    int64_t tot_closure_items;     /* phase X: closure items written (epsilon / tee arcs followed) */
    int64_t tot_bids_placed;       /* phase A: exit tokens that bid for their destination state - those of an arc that is the only
                                    * arc into its state recombine with nobody and place none (csrc/jd_search.h: REC_SOLE) */
} jd_stats;

/*
 * 1-best result: the DecHyp / DecHypHist chain of recognitionFinish()
 * (WFSTDecoderLite.cpp:262-308, DecHypHistPool.h:38-49,146-165) flattened to
 * arrays in CHAIN order: index 0 is hyp->hist (the newest word), index n-1 the
 * oldest.  label = DecHypHist::state (= output label = word id + 1), time =
 * DecHypHist::time.  Entry 0 and the totals carry the final-state weight.
 * n == -1 means "no token survived" (the reference returns NULL + warning).
 * Storage is owned by the decoder and valid until the next init of that stream.
 */
typedef struct jd_hyp {
    int32_t  n;
    const int32_t *label;
    const int32_t *time;
    const float   *score;
    const float   *ac;
    const float   *lm;
    float tot_score, tot_ac, tot_lm;
    jd_stats stats;
} jd_hyp;

/*
 * WFSTDecoderLite::WFSTDecoderLite(network, models, phoneStartPruneWin,
 * emitPruneWin, phoneEndPruneWin, wordPruneWin, maxEmitHyps)
 * (WFSTDecoderLite.h:81-89).  A window is enabled iff > 0; max_hyps == 0
 * disables the histogram (WFSTDecoderLite.cpp:76-82).  block_size mirrors
 * IModels::setBlockSize (1..20, juicer.cpp:255); it never changes results.
 * device = HIP device ordinal; max_streams = utterances decoded concurrently.
 * Like the reference's decoder (juicer.cpp:647-652) a decoder does not own its network or models: both must
 * outlive it - jd_dec_destroy still talks to the network (utterances of the streaming interface that were never
 * finished leave a lazily composed network there).
 */
int jd_dec_create(jd_dec **out, const jd_net *net, const jd_am *am,
                  float start_beam, float main_beam, float end_beam, float word_beam,
                  int32_t max_hyps, int32_t block_size, int32_t device, int32_t max_streams);
void jd_dec_destroy(jd_dec *d);

/* Per-stream arena capacities, in records (call before the first init; 0 keeps the default).
 * Defaults are taken from the free HBM when the arenas are first allocated: 70 % of it is split
 * over max_streams, each stream's share going 50/20/30 to instance records (80 B, two lists),
 * frontier items and Path records, never below 2^19 / 2^21 / 2^21 and never above what the
 * graph can need (one instance per arc).  An overflow is reported as JD_ENOMEM naming the arena. */
int jd_dec_set_capacity(jd_dec *d, int64_t max_slots, int64_t max_paths, int64_t max_items);
/* The stream arenas of a decoder are one slab of device memory; jd_dec_destroy keeps the largest one per device
 * for the next decoder created there (a decoder's set-up time is the driver clearing the memory it hands out:
 * seconds for the default sizes).  This gives the cached slab of `device` back to the driver (also: environment
 * JD_ARENA_CACHE=0 never keeps one). */
int jd_release_cached_memory(int32_t device);
/* WFSTDecoderLite::setMaxAllocModels (WFSTDecoderLite.cpp:807-820; environment variable
 * MaxAllocModels, default 10, :73-74), same argument convention: < 100 a percentage of the network's
 * transitions, 100..7999 a memory limit in MB (of 40 + 24 * maxNStates bytes per instance), otherwise
 * a number of instances.  A SOFT limit, as in the reference, which drops its cached NetInst objects
 * between utterances when more than this many are allocated (:164-169) and never fails a decode
 * because of it: here nothing is cached between utterances (one arena of records per stream, reused
 * wholesale), so the value can only RAISE that arena above its automatic size, never lower it - a
 * hard capacity is jd_dec_set_capacity's max_slots.  Before the first decode. */
int jd_dec_set_max_alloc_models(jd_dec *d, int32_t max_alloc_models);

/* IDecoder::init() (Decoder.h:26) for stream s. */
int jd_stream_init(jd_dec *d, int32_t s);
/* IDecoder::processFrame() x n_frames (Decoder.h:27): frames is n_frames x D
 * contiguous HOST floats; the look-ahead rows of the reference protocol
 * (DecoderSingleTest.cpp:267-295) carry no information beyond the frames
 * themselves, so the adapter folds them into pushes. */
int jd_stream_push(jd_dec *d, int32_t s, const float *frames, int32_t n_frames);
/* A stream of SPLICED models (jd_am_mlp_splice) holds the last `right` frames back until their windows are there: *held = the frames
 * pushed to stream s and not yet searched (jd_stream_finish searches them); 0 for every other kind of model. */
int jd_stream_held_frames(jd_dec *d, int32_t s, int32_t *held);
/* IDecoder::finish() (Decoder.h:28). */
int jd_stream_finish(jd_dec *d, int32_t s, jd_hyp *out);
/* jd_stream_push for several streams at once (each at most once per call): ONE scoring launch and ONE search launch
 * for all of them - the streams may sit at different frames.  With partial traces (jd_dec_set_partial_interval > 0) the
 * rows are still scored once and the streams then advance in rounds: a round is one search launch that ends, stream by
 * stream, at the frame after which the reference collects (either trigger), one collection launch and one trace launch
 * (k_partial_many) for all the streams whose collection or trace is due - every stream's collections, traces and lists
 * are what jd_stream_push calls with the same frames give, and the two calls may be mixed.  A stream that fails on the
 * device is left out of the later rounds (jd_stream_finish reports it), the others go on. */
int jd_streams_push(jd_dec *d, int32_t n, const int32_t *streams, const float *const *frames, const int32_t *n_frames);
/* max_streams / feature vector size of a decoder */
int jd_dec_info(const jd_dec *d, int32_t *max_streams, int32_t *vec_size);

/* ------------------------------------------------------------------ many IDecoder instances on one decoder
 *
 * The reference's harness decodes serially through ONE IDecoder (DecoderBatchTest.cpp:738-771 ->
 * DecoderSingleTest.cpp:259-324) and scales out as independent processes over split file lists
 * (doc/userman/juicer_userman.tex:584).  A broker lets N such serial callers - threads of one process - share the
 * streams of one decoder: each drives its own client with init / push / finish.  Up to 64 clients are served by a search
 * kernel that STAYS on the device while there is work (csrc/jd_resident.h): every client's stream has a cluster of
 * workgroups of its own there, the worker thread scores a client's frames as they come (one launch per round for all
 * the clients that brought some) and hands them to the cluster as soon as it is through with the chunk before - every
 * stream at its own pace; init, the Path collections and finish are small kernels beside it.  The kernel leaves the
 * device after 3 ms without work and comes back with the next request; while it is there, other search launches on the
 * device (this process: they wait for it; other processes: the file lock) and anything that synchronises the whole
 * device wait for that.  More than 64 clients, a lazily composed network, partial traces
 * (jd_dec_set_partial_interval > 0 before jd_broker_create; jd_broker_partial), or JD_BROKER_RESIDENT=0: a worker that turns
 * what has been pushed since its last TICK into one scoring launch and one search launch over all the streams concerned
 * (jd_streams_push).  The decoder must not be used directly while a broker owns it; clients may be driven from
 * different threads, one thread per client at a time.  jd_hyp arrays stay valid until the client's next init.
 * Environment: JD_BROKER_TICK_FRAMES (frames of one client per chunk / tick, default 256 / 192), JD_BROKER_COALESCE_US
 * (ticks: how long one waits for the other open clients' frames, default 300). */
typedef struct jd_broker jd_broker;
typedef struct jd_broker_stats {
    int64_t ticks, frames, stream_ticks;           /* launches, frames, streams summed over ticks */
    int64_t us_idle, us_coalesce;                  /* worker thread: waiting for work; waiting for the other clients' frames */
    int64_t us_init, us_push, us_finish;           /* ... inside jd_stream_init / jd_streams_push / jd_stream_finish */
    int64_t us_search;                             /* of us_push: the search launches (device time) */
    int64_t resident;                              /* > 0: the worker drives the resident search kernel, clusters of this many workgroups.
                                                      A "tick" is then one stream's chunk, and: us_search = the time from its post to its
                                                      report, us_coalesce = the time its cluster spent on it (device clock), us_init = the
                                                      NUMBER of Path collections between chunks, us_idle = what the cluster waited for the
                                                      next chunk of the same utterance, us_push = the staging calls, us_finish = the result
                                                      fetches */
} jd_broker_stats;
int jd_broker_create(jd_broker **out, jd_dec *dec, int32_t n_clients);   /* n_clients <= the decoder's max_streams */
void jd_broker_destroy(jd_broker *b);                                    /* (the decoder is the caller's to destroy, afterwards) */
int jd_broker_open(jd_broker *b, int32_t *client);
int jd_broker_close(jd_broker *b, int32_t client);
int jd_broker_init(jd_broker *b, int32_t client);                                              /* IDecoder::init */
/* IDecoder::processFrame x n: returns once the frames are taken */
int jd_broker_push(jd_broker *b, int32_t client, const float *frames, int32_t n_frames);
int jd_broker_finish(jd_broker *b, int32_t client, jd_hyp *out);                               /* IDecoder::finish */
int jd_broker_get_stats(jd_broker *b, jd_broker_stats *out);

/*
 * PARTIAL_DECODING (WFSTDecoderLite.cpp:822-896, compiled in by src/CMakeLists.txt:5): the Path
 * records every open hypothesis of a stream has converged into - the part of the result that can
 * no longer change - collected in the decoder's partialPaths list (WFSTDecoderLite.h:199-205).
 *
 * jd_dec_set_partial_interval = setPartialDecodeOptions (:892-896; the reference takes the value
 * from the environment variable PartialTraceInterval, :116-119; 0 = off, the default).  With an
 * interval > 0 jd_stream_push traces on the reference's schedule - together with a path
 * collection, if f - lastPartialTraceFrame > interval (:362-368) - and jd_stream_finish completes
 * the list from the best token (:245-251).  A collection runs after frame f under the reference's
 * two triggers (:362): f - lastPathCollectFrame > 100, or nPath / nPathNew > 12 with nPath > 10000.
 * The first is exact.  The second counts Path objects: the reference creates one per labelled
 * propagateToken call (:497-509), i.e. for every exit token and every labelled epsilon / tee arc of the
 * closure behind it, whether or not the token then wins its entry state, and keeps what the tokens of its
 * active instances reach (:703-745).  With the end and word beams off (the CLI's default) those are static
 * properties of the graph, and the decoder counts them without writing the losers: the collections then run
 * after the reference's own frames (tests: equal to the oracle's frame by frame, counts included).  With
 * an end or word beam, or a lazily composed network, the rule runs on this build's own records - at most
 * the reference's, so it fires no earlier - an approximation.  The schedule decides when a trace is
 * taken, never what a trace at a given frame finds.
 * jd_streams_push keeps the same schedule for every one of its streams.  Under a broker the interval is set before
 * jd_broker_create (the decoder is not to be used directly while a broker owns it) and the lists are read with
 * jd_broker_partial.
 * jd_stream_collect_info: collections of the stream's utterance so far and lastPathCollectFrame.
 * jd_stream_path_counts: nPath and nPathNew as the trigger reads them, *exact = 1 when they are the reference's.
 *
 * jd_stream_partial returns the stream's partialPaths - (output label, frame) of each record,
 * oldest first; *n is the full length, at most cap entries are written - after, if trace_now != 0,
 * running tracePartialPath (:824-868) on the frame the stream has reached (*found = its return
 * value).  Streaming API only: a batch returns whole results, and the list recognitionFinish
 * ends up with is the hypothesis itself (jd_hyp.label / .time, newest first).
 */
int jd_dec_set_partial_interval(jd_dec *d, int32_t interval);
int jd_stream_collect_info(jd_dec *d, int32_t s, int32_t *n_collections, int32_t *last_collect_frame);
int jd_stream_path_counts(jd_dec *d, int32_t s, int32_t *n_path, int32_t *n_path_new, int32_t *exact);
/* Diagnostics / tests (host only): per state, the Path objects WFSTDecoderLite::propagateToken creates behind ONE token that
 * arrives there with the end and word beams off - one per labelled epsilon arc and per labelled arc of a tee model that
 * leaves the state, plus what arrives behind each of those arcs, with multiplicity (:497-509 inside :533-541, :583-599);
 * saturated at 2^20.  out[n_states]; *acyclic = 0: the label-less part of the graph has a cycle, the counts are not used. */
int jd_debug_closure_path_counts(const jd_net *net, const jd_am *am, int32_t *out, int32_t *acyclic);
int jd_stream_partial(jd_dec *d, int32_t s, int32_t trace_now, int32_t cap, int32_t *n,
                      int32_t *labels, int32_t *times, int32_t *found);
/* tracePartialPath now (:824-868) on each of the n listed streams, each at the frame it has reached: jd_stream_partial(s,
 * trace_now = 1) for a list - ONE kernel launch (a workgroup per stream) and one fetch instead of a launch and three
 * copies per stream.  found[i] (found may be NULL) = the return value of stream i's trace; the lists are then read with
 * jd_stream_partial(s, 0, ...).  Each stream may be listed once (JD_EINVAL).  Word level only: JD_ESTATE on a decoder with
 * JD_OUTPUT_MODELS, where the single-stream calls remain. */
int jd_streams_trace(jd_dec *d, int32_t n, const int32_t *streams, int32_t *found);
/* the interval jd_dec_set_partial_interval set (0: off) */
int jd_dec_get_partial_interval(const jd_dec *d, int32_t *interval);
/* The partialPaths of a broker's client as of the worker's last tick - after jd_broker_finish the complete list (the
 * hypothesis, oldest first) - with jd_stream_partial's conventions: *n is the full length, at most cap entries are
 * written (labels / times may be NULL).  Empty from the client's jd_broker_init on.  The schedule is the interval's
 * (set with jd_dec_set_partial_interval BEFORE jd_broker_create; such a broker runs the tick worker,
 * jd_broker_stats.resident = 0): there is no trace_now through a broker.  Only the worker touches the decoder; this call
 * reads the copy it leaves with the client after every tick. */
int jd_broker_partial(jd_broker *b, int32_t client, int32_t cap, int32_t *n, int32_t *labels, int32_t *times);

/*
 * DecoderBatchTest::run() inner loop (DecoderBatchTest.cpp:738-771) for a
 * batch: decodes n_utts utterances (n_utts may exceed max_streams; they are
 * processed in waves of max_streams).  feats[u] = n_frames[u] x D host floats.
 */
int jd_decode_batch(jd_dec *d, int32_t n_utts, const float *const *feats,
                    const int32_t *n_frames, jd_hyp *out);

/*
 * Same, with features already resident in device memory (bench path: inputs
 * in HBM before the timed region).  d_feats is one device buffer holding all
 * utterances back to back; offs[u] is the frame offset of utterance u
 * (n_utts+1 entries).  hip_stream is a hipStream_t (or NULL for the default
 * stream).  Results are valid after the call returns (it synchronises).
 */
int jd_decode_batch_device(jd_dec *d, int32_t n_utts, const float *d_feats,
                           const int64_t *offs, void *hip_stream, jd_hyp *out);

/*
 * Scoring one batch ahead.  The reference scores and searches in turn (HTKFlatModels::calcOutput is
 * called from the search, src/HTKFlatModels.cpp:190-262; its two-thread organisation overlaps them on
 * two cores).  Here the batch path scores a whole batch's likelihood table and then searches it with a
 * persistent kernel whose clusters leave their CUs as their utterances end; announcing the NEXT batch
 * (same arguments as the jd_decode_batch_device call that will decode it; at most max_streams
 * utterances) before decoding the current one lets the scoring kernel of that next batch run on the
 * CUs the current search leaves idle, into a second table.  The announced decode then finds its table
 * scored.  The device buffer of the announced batch must stay valid and unchanged until that decode
 * (offs is copied); a decode with other arguments simply drops the table - results never depend on the
 * announcement.  n_utts = 0 drops whatever was announced or scored ahead.  Calling this is optional.
 * Announcements queue up, in the order of the decodes to come (at most three; one more is not taken), and
 * SEARCHING ahead follows from scoring ahead: a batch lasts as long as its longest utterance while the clusters of
 * its shorter ones are long through, so when the batch BEHIND the one being decoded has its table already - it was
 * announced two decodes ahead - and each of the two fills at most half of the decoder's streams, its utterances are
 * started beside the running batch, one workgroup each, on the other half of the streams; when its turn comes they
 * are hundreds of frames in (jd_timing.ahead_frames) and the call is that much shorter.  A stream of batches gets
 * this with two announcements before its first decode and one before every later one (jd_dec_set_pipeline(d, JD_FLOW_SERIAL, 0, 0) switches it off).
 * While the scoring runs the search launch is not re-planned under way when the scoring is a sizeable part
 * of the step (measured on the decoder's last batches: from a tenth of the search on), so that its blocks find
 * CUs; else it is slotted in at the re-planning cuts.
 */
int jd_dec_prefetch_scores(jd_dec *d, int32_t n_utts, const float *d_feats,
                           const int64_t *offs, void *hip_stream);

/*
 * The same loop sharded over the GPUs of ONE node from C++ (no Python, no torchrun): one decoder
 * and one host thread per device, utterances dealt by length (longest first, each to the device
 * with the fewest frames so far), no data-path collective, and ONE RCCL all-gather (over xGMI) of
 * padded 1-best records at the end - a record is as long as the batch's longest hypothesis; results
 * come back in the caller's utterance order.  An utterance that fails leaves an empty hypothesis,
 * the others are returned and the call reports the first error.  devices == NULL means devices
 * 0 .. n_devices-1.  RCCL is loaded with dlopen on first use.  jd_hyp storage is owned by the
 * jd_multi and valid until its next decode.
 */
typedef struct jd_multi jd_multi;
int jd_multi_create(jd_multi **out, const jd_net *net, const jd_am *am,
                    float start_beam, float main_beam, float end_beam, float word_beam,
                    int32_t max_hyps, int32_t block_size, int32_t n_devices, const int32_t *devices,
                    int32_t max_streams_per_device);
/* the same over lazily composed networks (jd_net_create_lazy), one per device, owned by the jd_multi: every
 * device expands the part of C.L o G its own utterances reach */
int jd_multi_create_lazy(jd_multi **out, const jd_net *cl, const jd_net *g, const jd_am *am,
                         int64_t max_states, int64_t max_arcs, int32_t pushing,
                         float start_beam, float main_beam, float end_beam, float word_beam,
                         int32_t max_hyps, int32_t block_size, int32_t n_devices, const int32_t *devices,
                         int32_t max_streams_per_device);
int jd_multi_decode_batch(jd_multi *m, int32_t n_utts, const float *const *feats,
                          const int32_t *n_frames, jd_hyp *out);
void jd_multi_destroy(jd_multi *m);

/* Timing of the most recent jd_decode_batch*() (HIP events on the decoder's own streams): total
 * duration of the GMM-kernel launches, of the k_search launches (the persistent search kernel:
 * one launch per chunk of frames, repeated when a stream had to stop for Path garbage
 * collection), wall time of the call. */
typedef struct jd_timing {
    double gmm_ms, search_ms, total_ms;
    double gmm_wait_ms;       /* host time spent waiting for scores the search needed next      */
    int32_t gmm_launches, search_launches;
    int32_t relaunches;       /* k_search launches repeated after an in-chunk garbage collection */
    int32_t cluster_wgs;      /* workgroups (1024 threads) per stream cluster in the last launch */
    int64_t gmm_frames;       /* stream-frames scored                           */
    int64_t gmm_states;       /* tied states scored per frame                    */
    int64_t search_frames;    /* stream-frames decoded                          */
    int32_t prefetched;       /* waves whose table had been scored ahead (jd_dec_prefetch_scores): their gmm_ms is the
                                 span of that scoring beside the previous search, and gmm_wait_ms what was left of it */
    int32_t ahead_frames;     /* frames of this batch that had been searched beside the batch before it ("two batches in
                                 flight": announcements two batches ahead, a batch on at most half of the streams) */
    int32_t slot_launches;    /* of search_launches: launches of the slot kernel (csrc/jd_slot.h: one workgroup per stream, two per
                                 CU - batches of more streams than the chip has CUs) */
    int32_t trace_launches;   /* partial-trace kernel launches (k_partial, k_partial_many, k_partial_many_models), cumulative over the streaming calls as
                                 search_ms is: a jd_streams_push round traces all its due streams with one */
} jd_timing;
int jd_dec_last_timing(const jd_dec *d, jd_timing *out);

/*
 * How batches that follow each other share the chip - the decoder's counterpart of the reference's constructor-time
 * configuration (WFSTDecoderLite.h:81-89; its harness decodes list entry after list entry, DecoderBatchTest.cpp:738-771).
 * Results never depend on it.  Call it any time between two decodes; whatever is announced or under way is dropped.
 *   JD_FLOW_SERIAL         one batch on the chip at a time (an announced batch is still SCORED beside the running search).
 *   JD_FLOW_TWO_IN_FLIGHT  (default) the batch behind the running one is started beside it when its table is there:
 *                          announcements two batches ahead, each batch on at most half of the decoder's streams.
 *   JD_FLOW_RESIDENT       announced batches go through a search kernel that STAYS on the device, utterance by utterance:
 *                          every stream is a slot of one workgroup that takes the next queued utterance the moment its
 *                          own is through; the scoring runs beside them.  depth = batches announced and not yet handed
 *                          back, at most (2..32; 0 = by the slots: 8, or slots / 32 + 2 - a likelihood table each); slots =
 *                          one-workgroup slots (1..max_streams; 0 = max_streams): a slot is half a CU and the slots are dealt
 *                          one per CU while there are CUs - the scoring kernel's workgroups take the other half of the
 *                          same CUs, so as many slots as the device has CUs is the count to ask for.
 *                          jd_decode_batch_device must be called for the batches in the order they
 *                          were announced (anything else drops what is under way and decodes the usual way); a batch
 *                          larger than the decoder's slots goes through them without any announcement.  See
 *                          jd_dec_quiesce for what the resident kernel means for the rest of the process.
 *                          Not with lazily composed networks, hybrid scoring or PARTIAL_DECODING (those decode the
 *                          usual way).
 */
#define JD_FLOW_SERIAL         0
#define JD_FLOW_TWO_IN_FLIGHT  1
#define JD_FLOW_RESIDENT       3
int jd_dec_set_pipeline(jd_dec *d, int32_t mode, int32_t depth, int32_t slots);

/*
 * How the likelihood tables are scored - an OPTION beside the default, for a caller that wants throughput over bit equality.
 *   JD_SCORE_EXACT  (default) HTKFlatModels::calcGMMOutput + logAdd with the reference's own roundings (src/HTKFlatModels.cpp:226-293: no
 *                   contraction, the host libm's expf, log(1 + e) in double): every log-likelihood equals the reference's bit for bit.
 *   JD_SCORE_FAST   fused multiply-add distance on pre-scaled parameters and an fp32 logAdd on the hardware's exp / log: a log-likelihood
 *                   moves by ~1e-5 of its magnitude; hypotheses keep their words and times on every fixture of the test suite and their
 *                   scores stay within 1e-4 relative (what BASELINE.json's north_star asks of the path; tests/test_gpu_fastscore.py).
 *                   GMM models of every vector size (hybrid models: refused).  At D = 39 the table costs 0.4 of the exact one
 *                   (csrc/jd_gmm.h: jd_gmm_fast39); every other D is scored by jd_gmm_fast (the same arithmetic, D at run time; DESIGN.md
 *                   3.5 has its measured cost and deviation per D; tests/test_gpu_fastscore_anyd.py).
 * Call it between two decodes; whatever was scored or announced ahead is dropped.  jd_am_score_frames_mode: jd_am_score_frames with the option.
 */
#define JD_SCORE_EXACT 0
#define JD_SCORE_FAST  1
int jd_dec_set_scoring(jd_dec *d, int32_t mode);
int jd_am_score_frames_mode(const jd_am *a, int32_t device, int32_t mode, const float *frames, int32_t n_frames, float *out);

/* Model-level output (IDecoder::modelLevelOutput; basicCore's WFSTDecoder::extendModelEndState): besides the words, which HMM
 * (model) the best path passed and in which frames.
 *   JD_OUTPUT_WORDS                      the default: jd_hyp, the 1-best word chain
 *   JD_OUTPUT_WORDS | JD_OUTPUT_MODELS   the same jd_hyp - bit for bit what word output gives, the search is the same - and a
 *                                        jd_model_hyp beside it (jd_dec_model_result)
 * A jd_model_hyp entry per arc with an in-label (a model) the best path traversed, tee models included (zero frames), and per
 * epsilon-input arc with a word label (model 0); newest first, like jd_hyp:
 *   model  in-label = HMM index + 1 (0: a word label on an epsilon-input arc)
 *   label  word id + 1 when the same arc carries a word label, else 0
 *   time   the frame the token left the model (a word's end frame in jd_hyp); a segment starts at the next entry's time
 *          (frame 0 for the oldest)
 *   score / ac / lm  the token's there; entry 0 and the totals with the final state's weight, as in jd_hyp.
 * The search kernels write a Path record for every model the best paths pass: more records, more collections on heavy graphs.
 * Set between utterances: refused (JD_ESTATE) while a stream has frames pushed since its jd_stream_init and no jd_stream_finish
 * yet.  The result arrays of model-level output are allocated when it is first switched on.  Not with partial traces (jd_dec_set_partial_interval > 0; jd_stream_partial / jd_stream_partial_models with trace_now work, the first
 * gives words, the second models), not under a broker (jd_broker_create refuses such a decoder; set it before creating one), and jd_multi_* decode
 * words only.  jd_dec_model_result: result i of the decoder's last jd_stream_finish (i = the stream) or jd_decode_batch /
 * jd_decode_batch_device (i = the utterance); valid until the next decode, finish or jd_dec_set_output_level.  n = -1: no result
 * (as in jd_hyp); n is capped by the result capacity (8192 entries), a longer chain fails the decode with JD_ENOMEM.
 */
#define JD_OUTPUT_WORDS  1
#define JD_OUTPUT_MODELS 2
typedef struct jd_model_hyp {
    int32_t  n;
    const int32_t *model;
    const int32_t *label;
    const int32_t *time;
    const float   *score;
    const float   *ac;
    const float   *lm;
    float tot_score, tot_ac, tot_lm;
} jd_model_hyp;
int jd_dec_set_output_level(jd_dec *d, int32_t level);
int jd_dec_get_output_level(const jd_dec *d, int32_t *level);
int jd_dec_model_result(jd_dec *d, int32_t i, jd_model_hyp *out);
/* The models' names, for printing phones (HTKModels::getHMMName / PhoneLookup::getModelStr): *name = the name of HMM i (HMM
 * index i = in-label i + 1), as jd_am_load_mmf (the ~h name) or jd_am_load_jmbi (the JMHM record's name) read it - "" for an
 * unnamed record of a file whose other records have names; NULL when the model set has no names (jd_am_create_htk / _flat /
 * _hybrid, a JMBI file without names).  The string lives as long as a.  jd_am_save_jmbi writes the names back.
 * JD_EINVAL: a null handle or i outside [0, jd_am_num_hmms). */
int jd_am_hmm_name(const jd_am *a, int32_t i, const char **name);
/* jd_stream_partial's trace at model level (JD_OUTPUT_MODELS; JD_ESTATE on a word-level decoder): the same trace_now, the same
 * trace, and the list of the last trace that found something - every record of the chain from the root up to the record the
 * word list ends at, model records and word records alike, OLDEST first, entries as in jd_model_hyp (no final-state weight:
 * the utterance has not ended).  A trace through either call updates both lists: the word list is this list's entries with a
 * label, and its last entry carries a word.  *n = the length (copied up to cap; any output pointer may be NULL).  A chain
 * longer than the result capacity fails the trace with JD_ENOMEM.  Explicit traces only: jd_dec_set_partial_interval > 0
 * stays refused at model level. */
int jd_stream_partial_models(jd_dec *d, int32_t s, int32_t trace_now, int32_t cap, int32_t *n,
                             int32_t *model, int32_t *label, int32_t *time, float *score, float *ac, float *lm,
                             int32_t *found);

/* The CURRENT BEST hypothesis of live streams: what the decoder believes right now, beside the converged prefix the partial
 * traces give (jd_stream_partial).  After the last frame pushed to a stream, the best token is the emitting-state token with
 * the highest score among the active arc instances (HMM states 1 .. nStates - 2 with a score above LOG_ZERO; entry tokens
 * pending at states have not been scored on a frame and do not count).  Equal scores: the lowest arc in the decoder's own arc
 * order, then the lowest HMM state - a rule that does not depend on the run.  The hypothesis is the token's Path chain, OLDEST
 * first: on a word-level decoder every record carries a word label; at model level (JD_OUTPUT_MODELS) it is every record of
 * the chain with the fields of jd_model_hyp, and the word list is its entries with a label.  Nothing carries a final-state
 * weight: the utterance has not ended.  Unstable by nature - every call may revise the whole list.
 * jd_streams_best runs the search for the n listed streams, each at the frame it has reached, with ONE kernel launch (a
 * workgroup per stream) and ONE device-to-host copy that brings the heads and every chain of up to 64 records; a longer chain
 * is read from the stream's result arrays afterwards.  out[i] is stream i's head; the lists stay with the decoder and are read
 * with jd_stream_best_words / jd_stream_best_models, which only read that host copy, with jd_stream_partial's conventions (*n
 * the full length, at most cap entries written, any output pointer may be NULL; empty from jd_stream_init on and after a call
 * that found nothing).  jd_stream_best_models: JD_ESTATE on a word-level decoder; jd_stream_best_words works at both levels.
 * Anywhere between a stream's jd_stream_init and its jd_stream_finish, mixed freely with jd_stream_push, jd_streams_push,
 * jd_stream_partial* and jd_streams_trace, under a trace interval and on a lazily composed network; it only reads the
 * stream's state and never changes what those calls or jd_stream_finish return.
 * JD_EINVAL: a null handle or list, n < 0, a stream outside the decoder's range or listed twice.  JD_ESTATE: a listed stream
 * before its jd_stream_init; a decoder whose resident kernel a broker drives.  JD_ENOMEM: a chain longer than the result
 * capacity - that stream's entry says found = 0 and its list is empty, the other entries are delivered, and the first such
 * error is returned.
 * jd_dec_best_stats: the kernel launches and device-to-host copies these calls have made (cumulative).
 * Out of scope: the broker (jd_broker_* offers the converged prefix only), the batch calls, jd_multi_* and the resident
 * kernels. */
typedef struct jd_best {
    int32_t found;        /* 0: the stream has no live emitting token (no frame yet, a failed stream, everything pruned) */
    int32_t frame;        /* the frame the stream has reached (frames pushed)                                           */
    int32_t n_words;      /* records with a word label on the chain                                                     */
    int32_t n_records;    /* all records on the chain (= n_words on a word-level decoder)                               */
    int32_t model;        /* in-label of the arc the token is inside (HMM index + 1)                                    */
    int32_t state;        /* its HMM state, 1 .. nStates - 2                                                            */
    float score, ac, lm;  /* the token's                                                                                */
} jd_best;
int jd_streams_best(jd_dec *d, int32_t n, const int32_t *streams, jd_best *out);
int jd_stream_best_words(jd_dec *d, int32_t s, int32_t cap, int32_t *n, int32_t *label, int32_t *time,
                         float *score, float *ac, float *lm);
int jd_stream_best_models(jd_dec *d, int32_t s, int32_t cap, int32_t *n, int32_t *model, int32_t *label,
                          int32_t *time, float *score, float *ac, float *lm);
int jd_dec_best_stats(const jd_dec *d, int64_t *launches, int64_t *copies);

/* The END-OF-UTTERANCE view of live streams: the hypothesis jd_stream_finish would return if the utterance ended now, read
 * without ending it.  The decoder keeps bestFinalToken behind every frame (WFSTDecoderLite.cpp:513-520): the best token in a
 * final state, its score with the final-state weight.  found follows jd_stream_finish's rule - that token's score is above
 * LOG_ZERO and the stream has processed a frame.  The hypothesis is the token's Path chain, OLDEST first like every other live
 * list; the newest (last) entry carries the token's own score / ac / lm with the final weight (:293-300).  Reversed, the lists
 * are entry for entry and bit for bit the jd_hyp (jd_stream_final_words, at both output levels: at model level the labelled
 * entries, the newest of which carries the totals as in jd_hyp) or the jd_model_hyp (jd_stream_final_models) that
 * jd_stream_finish would return after the same frames, and the head's score / ac / lm are the totals of a non-empty result
 * (jd_stream_finish reports LOG_ZERO totals for an empty one; the head says the token's).
 * jd_streams_final serves the n listed streams, each at the frame it has reached, with ONE kernel launch (a workgroup per
 * stream) and ONE device-to-host copy that brings the heads and every chain of up to 64 records; a longer chain is read from
 * the stream's result arrays afterwards.  out[i] is stream i's head; the lists stay with the decoder and are read with
 * jd_stream_final_words / jd_stream_final_models, which only read that host copy, with jd_stream_partial's conventions (*n the
 * full length, at most cap entries written, any output pointer may be NULL; empty from jd_stream_init on and after a call that
 * found nothing).  jd_stream_final_models: JD_ESTATE on a word-level decoder.
 * Non-destructive: allowed wherever jd_streams_best is, mixed freely with the push, trace and best calls, under a trace
 * interval and on a lazily composed network; it never changes what a later call returns.  Taken behind the same frame,
 * jd_best.score and jd_final.score are under the same normalisation; the rule that compares them (an endpointer's) is the
 * caller's.
 * JD_EINVAL: a null handle or list, n < 0, a stream outside the decoder's range or listed twice.  JD_ESTATE: a listed stream
 * before its jd_stream_init; a stream, or a decoder, whose resident kernel a broker drives.  JD_ENOMEM: a chain longer than
 * the result capacity - that stream's entry says found = 0 and its list is empty, the other entries are delivered, and the
 * first such error is returned.
 * jd_dec_final_stats: the kernel launches and device-to-host copies these calls have made (cumulative). */
typedef struct jd_final {
    int32_t found;        /* 0: no token is in a final state behind the last frame pushed (also: no frame yet, a failed stream) */
    int32_t frame;        /* frames pushed                                                                                     */
    int32_t n_words;      /* records with a word label on the chain                                                            */
    int32_t n_records;    /* all records on the chain (= n_words on a word-level decoder); 0 is possible with found = 1        */
    float score, ac, lm;  /* bestFinalToken's, final-state weight included: jd_hyp.tot_score / tot_ac / tot_lm of that finish    */
} jd_final;
int jd_streams_final(jd_dec *d, int32_t n, const int32_t *streams, jd_final *out);
int jd_stream_final_words(jd_dec *d, int32_t s, int32_t cap, int32_t *n, int32_t *label, int32_t *time,
                          float *score, float *ac, float *lm);
int jd_stream_final_models(jd_dec *d, int32_t s, int32_t cap, int32_t *n, int32_t *model, int32_t *label,
                           int32_t *time, float *score, float *ac, float *lm);
int jd_dec_final_stats(const jd_dec *d, int64_t *launches, int64_t *copies);

/* jd_stream_partial_models(s, trace_now = 1) for a list of streams of a MODEL-level decoder (each once), each at the frame it
 * has reached: one kernel launch (a workgroup per stream) and one device-to-host copy, as jd_streams_trace is for
 * jd_stream_partial.  found[i] (found may be NULL) is stream i's trace's result; the lists are read afterwards with
 * jd_stream_partial_models(s, 0, ...) and jd_stream_partial(s, 0, ...) - both are updated, as by a single-stream trace.
 * Counts once per call in jd_timing.trace_launches.  JD_ESTATE on a word-level decoder (its counterpart there is
 * jd_streams_trace); otherwise jd_streams_trace's argument rules.  A list longer than the result capacity fails that stream
 * alone (JD_ENOMEM; the first such error is returned).  Explicit traces only: jd_dec_set_partial_interval stays refused at
 * model level. */
int jd_streams_trace_models(jd_dec *d, int32_t n, const int32_t *streams, int32_t *found);

/* What JD_FLOW_RESIDENT has done so far (cumulative over the decoder's life; a bench reads it on either side of its
 * timed region: frames_searched is what the slots really advanced in between, whatever was announced or handed back). */
typedef struct jd_pipe_stats {
    int32_t mode, depth, slots;
    int32_t resident;            /* the kernel is on the device right now                                     */
    int32_t batches_announced;   /* announced and not yet handed back                                         */
    int32_t pad0;
    int64_t frames_searched;     /* stream-frames the slots have advanced (their own reports, command by command) */
    int64_t utts_through;        /* utterances whose result has been exported                                 */
    int64_t rows_scored;         /* likelihood rows whose scoring has been enqueued                           */
    int64_t batches_back;        /* batches handed back by jd_decode_batch_device                              */
    int64_t collections;         /* Path collections between commands                                         */
    double slot_busy_us;         /* sum over the slots of their own clocks on their commands                  */
    double on_us;                /* wall time the resident kernel has been on the device                      */
} jd_pipe_stats;
int jd_dec_pipeline_stats(const jd_dec *d, jd_pipe_stats *out);

/* The decoder's work on the device comes to rest: with JD_FLOW_RESIDENT (announced batches go through a search kernel that stays
 * on the device, utterance by utterance: jd_dec_prefetch_scores up to `depth` batches ahead) that kernel lets the
 * commands that are running run out (128 frames at most) and leaves; nothing announced or under way is lost - it comes back
 * with the next call.  What a caller needs before a device-wide synchronisation while batches are announced - and before
 * it puts work of its own on OTHER streams of the device: HIP maps streams onto a few hardware queues, and a kernel that
 * is queued behind the resident one waits until it leaves (tools/resident_alias_probe.py: one fresh stream in fourteen;
 * by itself the kernel leaves after 5 s without a command, and the decode that follows says so).  The same holds while a
 * broker's resident kernel has work (it leaves after 3 ms without). */
int jd_dec_quiesce(jd_dec *d);

/* Diagnostics: per-workgroup cycle accounting of k_search (100 MHz wall clock).  enable >= 0 with
 * fetch == NULL switches it on and clears it, enable < 0 switches it off; with fetch != NULL
 * (1024 x 16 int64) the sums so far are copied out: per workgroup of the grid (thread 0's timeline)
 * {work lists A, phase A, workgroup wait, cluster barrier 1, work lists X, phase X, workgroup wait,
 *  cluster barriers of X, frames, ...}. */
int jd_dec_debug_trace(jd_dec *d, int32_t enable, int64_t *fetch);
/* Diagnostics: what part of a batch's likelihood table does the search read?  The reference scores a tied state only when
 * a token that passed the emit threshold asks for it (WFSTDecoderLite.cpp:409-411); this build scores every state of
 * every frame.  enable != 0: from the next decode on every cell (frame, tied state) whose value is added to a token is
 * marked; enable == 0: *cells_read = the marks, *cells_total = frames x tied states of the last decode, marking stops. */
int jd_dec_debug_cells(jd_dec *d, int32_t enable, int64_t *cells_read, int64_t *cells_total);

/*
 * Companion kernel on its own: HTKFlatModels::calcGMMOutput
 * (HTKFlatModels.cpp:226-262) for every tied state of every frame.
 * frames: n_frames x D host floats; out: n_frames x n_gmm host floats.
 */
int jd_am_score_frames(const jd_am *a, int32_t device, const float *frames,
                       int32_t n_frames, float *out);

/* Test hook behind the bit-exactness of logAdd (HTKFlatModels.cpp:266-293 calls expf on a float):
 * the kernels' own expf for x[0..n), evaluated on HIP device `device`, or by its host twin
 * (same source) when device == -1.  tests/test_expf.py compares both with the host libm. */
int jd_debug_expf(int32_t device, const float *x, int64_t n, float *out);
/* ... and of the rest of logAdd.  jd_debug_log1pe: log(1.0 + (double)expf(d[i])) in double for d[i] in [-19, 0]; variant 0 =
 * the kernels' replica of the host libm's log, 1 = the table value they round first.  jd_debug_log_add: logAdd(x[i], y[i]);
 * variant 0 = the generic kernel's, 1 = jd_gmm_kernel39's pairwise step (elements 2j and 2j + 1 are one pair), 2 = the
 * JD_SCORE_FAST kernel's (device only).  tests/test_logadd.py compares them with the host libm and the CPU oracle. */
int jd_debug_log1pe(int32_t device, int32_t variant, const float *d, int64_t n, double *out);
int jd_debug_log_add(int32_t device, int32_t variant, const float *x, const float *y, int64_t n, float *out);
/* ... and of the scoring kernels' tile loops: launch_gmm (csrc/jd_host_scoring.h) called once with the caller's own arguments, the
 * way the decoder's paths call it - the batch path with a packed row map and skip_unused, the resident side with a tile list - and
 * not only the way jd_am_score_frames does.  frames: n_frames x D.  row_src[r] in [-1, n_frames): the frame row r of the table is
 * scored from, -1 = unused.  skip_unused: a tile whose first row is unused is not scored.  max_blocks > 0 bounds the grid.
 * used_row_tiles >= 0 stands for the row tiles in the choice between the kernels of 16 and of 64 tied states per tile.  rt_base
 * (n_rt first rows) or NULL (n_rt = 0): score the 128-row tiles that begin at these rows only.  out: (guard_rows + n_rows +
 * guard_rows) x n_gmm floats, PREFILLED by the caller; it goes to the device as it is, the table is written behind the first
 * guard_rows rows, and the whole buffer comes back - whatever the launch did not write still holds the prefill.  *kernel = the
 * kernel launch_gmm chose (jd_score_kernel), *grid = its workgroups (either may be NULL).
 * Refused with JD_EINVAL before anything is launched: a row_src entry outside [-1, n_frames); with skip_unused, a scored tile
 * whose used rows are not a prefix of it (the kernels let the tile's first row decide); a list entry outside [0, n_rows); listed
 * tiles that overlap; a tile list for hybrid models (launch_gmm would ignore it); and, launch_gmm's own refusal, a tile list for exact
 * scoring of D != 39.  Tile rows: 128 at D = 39
 * and with JD_SCORE_FAST, 64 for exact scoring of any other D, none for hybrid models (which ignore skip_unused; those with a network,
 * jd_am_create_mlp and jd_am_create_mlp_tied, included: the 16-row tiles of jd_mlp_kernel / jd_mlp_tied_kernel - 32-row tiles of
 * jd_mlp_bf16_kernel / jd_mlp_tied_bf16_kernel for jd_am_mlp_to_bf16's models - are their own affair, and rows with row_src = -1 are
 * written as 0.0f).
 * tests/test_gpu_score_rows.py holds every cell of the buffer to tests/score_rows_cases.py. */
typedef enum jd_score_kernel {
    JD_KERNEL_NONE = 0,            /* nothing was launched                                  */
    JD_KERNEL_GMM_GENERIC = 1,     /* jd_gmm_kernel<0>: exact, D != 39, 64-row tiles        */
    JD_KERNEL_GMM39_16 = 2,        /* jd_gmm_kernel39<16>                                   */
    JD_KERNEL_GMM39_64 = 3,        /* jd_gmm_kernel39<64>                                   */
    JD_KERNEL_GMM_FAST39_16 = 4,   /* jd_gmm_fast39<16>                                     */
    JD_KERNEL_GMM_FAST39_64 = 5,   /* jd_gmm_fast39<64>                                     */
    JD_KERNEL_GMM_FAST_16 = 6,     /* jd_gmm_fast<16>                                       */
    JD_KERNEL_GMM_FAST_64 = 7,     /* jd_gmm_fast<64>                                       */
    JD_KERNEL_HYBRID = 8,          /* jd_hybrid_kernel                                      */
    JD_KERNEL_MLP = 9,             /* jd_mlp_kernel: jd_am_create_mlp's models, 16-row tiles */
    JD_KERNEL_MLP_TIED = 10,       /* jd_mlp_tied_kernel: jd_am_create_mlp_tied's, 16-row tiles */
    JD_KERNEL_MLP_BF16 = 11,       /* jd_mlp_bf16_kernel: jd_am_mlp_to_bf16 of jd_am_create_mlp's models, 32-row tiles */
    JD_KERNEL_MLP_TIED_BF16 = 12,  /* jd_mlp_tied_bf16_kernel: jd_am_mlp_to_bf16 of jd_am_create_mlp_tied's, 32-row tiles */
    JD_KERNEL_MLP_SPLICED = 13,            /* jd_mlp_spliced_kernel: jd_am_mlp_splice of a model that runs JD_KERNEL_MLP */
    JD_KERNEL_MLP_TIED_SPLICED = 14,       /* jd_mlp_tied_spliced_kernel: ... JD_KERNEL_MLP_TIED */
    JD_KERNEL_MLP_BF16_SPLICED = 15,       /* jd_mlp_bf16_spliced_kernel: ... JD_KERNEL_MLP_BF16 */
    JD_KERNEL_MLP_TIED_BF16_SPLICED = 16   /* jd_mlp_tied_bf16_spliced_kernel: ... JD_KERNEL_MLP_TIED_BF16 */
} jd_score_kernel;
int jd_debug_score_rows(const jd_am *a, int32_t device, int32_t mode, const float *frames, int32_t n_frames, const int32_t *row_src,
                        int32_t n_rows, int32_t skip_unused, int32_t max_blocks, int32_t used_row_tiles, const int32_t *rt_base,
                        int32_t n_rt, int32_t guard_rows, float *out, int32_t *kernel, int32_t *grid);
/* ... for SPLICED models (jd_am_mlp_splice), whose rows carry a span beside row_src: row r's window is the frames
 * clamp(row_src[r] + c - left, row_lo[r], row_hi[r]), c = 0 .. left + right - its utterance's bounds in `frames` (n_frames x D raw
 * frames).  Each row_lo / row_hi entry of a used row is checked against [0, n_frames), and row_lo <= row_hi; the other arguments and
 * refusals are jd_debug_score_rows', which itself refuses spliced models and names this call.  JD_EINVAL for any other model. */
int jd_debug_score_rows_span(const jd_am *a, int32_t device, int32_t mode, const float *frames, int32_t n_frames, const int32_t *row_src,
                             const int32_t *row_lo, const int32_t *row_hi, int32_t n_rows, int32_t skip_unused, int32_t max_blocks,
                             int32_t used_row_tiles, const int32_t *rt_base, int32_t n_rt, int32_t guard_rows, float *out, int32_t *kernel,
                             int32_t *grid);
/* ... and of the histogram pruning (Histogram.cpp:64-100 / 134-158).  jd_debug_hist_bin: the search kernels' bin of s[i]
 * (jd_hist_bin: s rounded half away from zero in double, minus hist_min), -1 when it falls below hist_min, JD_EHIST above
 * hist_max; device -1 runs the host twin; every s[i] must lie in (-2^31, 2^31) (no NaN, no infinity: JD_EINVAL).  jd_debug_hist_threshold: the kernels' one-wave calcThresh (hist_threshold) for
 * each case c over the counts bins[c * nb .. c * nb + nb) of bins hist_min .. hist_min + nb - 1, nb in [1, 2048], with
 * max_hyps[c] >= 1; device only.  tests/test_hist_cpu.py and tests/test_gpu_hist.py compare them with the CPU oracle. */
int jd_debug_hist_bin(int32_t device, const float *s, int64_t n, int32_t hist_min, int32_t hist_max, int32_t *out);
int jd_debug_hist_threshold(int32_t device, const int32_t *bins, int64_t n_cases, int32_t nb, const int32_t *max_hyps,
                            int32_t hist_min, float *out);
/* ... and of the Path collection and the PARTIAL_DECODING trace (csrc/jd_gc.h) on a state the CALLER describes instead of
 * one a search left behind: one to four streams - Path arenas, flags and counters, instance records by writer wave, the
 * last frame's frontier items and dirty lists, arrival keys, bestFinalToken's Path - over a tiny CSR graph, and up to eight
 * operations: a collection (launch_gc itself, on a work list or on one stream, with G workgroups per stream, gc_threshold and
 * path_rule as given), a trace of one stream (k_partial, word or model level) and a trace of several (k_partial_many).
 * desc is a list of n_desc int32 words whose grammar stands at the top of csrc/jd_paths.h; it is validated BEFORE any device
 * call, and what could lead a kernel out of an arena is JD_EINVAL: a prev[q] outside [-1, q), a token's, an item's or
 * bestFinalToken's path outside [-1, n_paths), an arrival key that names an item not written, a dirty or source state outside
 * the graph, per-wave counts beyond make_geo's segments, n_paths above the arena's capacity, an arena above 2^18 records, G
 * outside 1 .. 32, NE other than 3 or 6, res_cap < 1, more than four streams.  What comes back in out (same header: per stream
 * its counters, GcState words, the Path arena now current, the path of every token slot and of every item; per trace its
 * out words, result arrays and model row, prefilled with the description's sentinel): *n_out words, at most out_cap - too
 * small an out_cap is JD_ENOMEM with *n_out set to what is needed, before any device call as well.  Device only; needs no
 * jd_dec, network or model, and allocates and frees what it uses.  tests/test_gpu_paths.py compares every word that comes back
 * with tests/paths_ref.py. */
int jd_debug_paths(int32_t device, const int32_t *desc, int64_t n_desc, int32_t *out, int64_t out_cap, int64_t *n_out);

const char *jd_last_error(void);
const char *jd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* JUICER_AMD_H */
