"""The model-level twin of tests/indep_viterbi_np.py - test infrastructure, not product code.

The same float64 full-trellis Viterbi (no active lists, no pruning, its own GMM evaluation through indep_viterbi_np.gmm_loglik),
whose back-pointers keep every MODEL boundary besides the words: a record {model, label, frame, score, lm} is made whenever a
token leaves an arc with an in-label (through the model's exit state, or through its tee transition within the frame) and
whenever it crosses an epsilon-input arc with an output label (model 0).  This is what basicCore's extendModelEndState records
(one DHHTYPE entry per model, the word label on the same arc), restated from the recurrences alone; score is the token's there,
lm the sum of the arc weights it has crossed (ac = score - lm).  Its word projection (records with a label) is
indep_viterbi_np.viterbi's result."""
import numpy as np

from indep_viterbi_np import NEG, _best_per_key


class _Hist:
    """records {model, label, frame, score, lm, previous record}, appended in blocks"""
    def __init__(self):
        self.cols = [[] for _ in range(6)]
        self.n = 0

    def add(self, model, label, time, score, lm, prev):
        k = len(label)
        ids = np.arange(self.n, self.n + k, dtype=np.int64)
        for c, v in zip(self.cols, (model, label, np.full(k, time), score, lm, prev)):
            c.append(np.asarray(v))
        self.n += k
        return ids

    def chain(self, h):
        if self.n == 0 or h < 0:
            return []
        M, L, Tm, S, LM, P = (np.concatenate(c) for c in self.cols)
        out = []
        while h >= 0:
            out.append((int(M[h]), int(L[h]), int(Tm[h]), float(S[h]), float(LM[h])))
            h = int(P[h])
        return out[::-1]


def viterbi_models(net, am, ll, lm_scale=1.0, ins_penalty=0.0):
    """Returns (total score, total lm, [(model, label, frame, score, lm), ...] oldest first) or None when no token ends in a
    final state.  model = in-label (HMM index + 1; 0: an epsilon-input arc with a word label), label = output label (0: none)."""
    src, dst, il, ol = (np.asarray(a, np.int64) for a in (net.src, net.dst, net.ilab, net.olab))
    w = -net.w_file.astype(np.float64) * lm_scale + np.where(ol > 0, ins_penalty, 0.0)
    nS = int(max(net.n_states, src.max() + 1, dst.max() + 1))
    fin = np.full(nS, NEG)
    fin[np.asarray(net.fstate, np.int64)] = -np.asarray(net.fweight_file, np.float64) * lm_scale
    init = int(src[0])
    MN = am.max_n
    with np.errstate(divide="ignore"):
        logA = np.where(am.transp > 0, np.log(np.maximum(am.transp.astype(np.float64), 1e-300)), NEG)
    T = ll.shape[0]
    marc = np.nonzero(il > 0)[0]
    earc = np.nonzero(il == 0)[0]
    hm = il[marc] - 1
    n_st = am.hmm_nstates[hm].astype(np.int64)
    A = logA[am.hmm_tm[hm]]
    jj = np.arange(MN)[None, :]
    emitting = (jj >= 1) & (jj <= n_st[:, None] - 2)
    gm = np.where(emitting, am.hmm_gmm[hm], 0).astype(np.int64)
    A_exit = np.take_along_axis(A, (n_st - 1)[:, None, None].repeat(MN, axis=1), axis=2)[:, :, 0]
    A_in = np.where(emitting[:, None, :] & (jj[:, :, None] <= n_st[:, None, None] - 2), A, NEG)
    tee = np.full(am.n_hmm, NEG)
    for h in range(am.n_hmm):
        n = int(am.hmm_nstates[h]); a = am.transp[am.hmm_tm[h]]
        sucs = [j for j in range(n) if a[0, j] > 0]
        if (n - 1) in sucs[1:]:
            tee[h] = np.log(float(a[0, n - 1]))
    tee_arc = marc[tee[hm] > NEG / 2]
    tee_w = tee[il[tee_arc] - 1]
    c_arc = np.concatenate([earc, tee_arc]); c_w = np.concatenate([w[earc], w[tee_arc] + tee_w])
    H = _Hist()

    def expand(a_state, a_score, a_lm, a_hist, t):
        sb = np.full(nS, NEG); slm = np.zeros(nS); sh = np.full(nS, -1, np.int64)
        k = _best_per_key(a_state, a_score)
        sb[a_state[k]] = a_score[k]; slm[a_state[k]] = a_lm[k]; sh[a_state[k]] = a_hist[k]
        changed = np.zeros(nS, bool); changed[a_state[k]] = True
        for _ in range(nS + 1):
            use = changed[src[c_arc]]
            if not use.any():
                break
            ca, cw = c_arc[use], c_w[use]
            cand = sb[src[ca]] + cw
            k = _best_per_key(dst[ca], cand)
            k = k[cand[k] > sb[dst[ca[k]]]]
            changed[:] = False
            if k.shape[0] == 0:
                break
            win = ca[k]
            hist = sh[src[win]].copy()
            lm = slm[src[win]] + w[win]
            rec = (il[win] != 0) | (ol[win] != 0)                       # a tee model passed, or a word label crossed
            if rec.any():
                hist[rec] = H.add(il[win[rec]], ol[win[rec]], t, cand[k][rec], lm[rec], hist[rec])
            sb[dst[win]] = cand[k]; slm[dst[win]] = lm; sh[dst[win]] = hist
            changed[dst[win]] = True
        return sb, slm, sh

    sb, slm, sh = expand(np.array([init]), np.array([0.0]), np.array([0.0]), np.array([-1], np.int64), 0)
    S = np.full((marc.shape[0], MN), NEG); Sh = np.full((marc.shape[0], MN), -1, np.int64); Slm = np.zeros((marc.shape[0], MN))
    best = None
    for t in range(T):
        ok = sb[src[marc]] > NEG / 2
        S[:, 0] = np.where(ok, sb[src[marc]] + w[marc], NEG); Sh[:, 0] = np.where(ok, sh[src[marc]], -1)
        Slm[:, 0] = np.where(ok, slm[src[marc]] + w[marc], 0.0)
        cand = S[:, :, None] + A_in
        bi = cand.argmax(axis=1)
        bs = np.take_along_axis(cand, bi[:, None, :], axis=1)[:, 0, :]
        alive = emitting & (bs > NEG / 2)
        new = np.where(alive, bs + ll[t][gm], NEG)
        newh = np.where(alive, np.take_along_axis(Sh, bi, axis=1), -1)
        newlm = np.where(alive, np.take_along_axis(Slm, bi, axis=1), 0.0)
        exc = np.where(emitting, new + A_exit, NEG)
        ei = exc.argmax(axis=1)
        r = np.arange(exc.shape[0])
        ex, exh, exlm = exc[r, ei], newh[r, ei], newlm[r, ei]
        S, Sh, Slm = new, newh, newlm
        out = np.nonzero(ex > NEG / 2)[0]
        a_arc = marc[out]
        hist = H.add(il[a_arc], ol[a_arc], t, ex[out], exlm[out], exh[out])     # every model exit is a record
        sb, slm, sh = expand(dst[a_arc], ex[out], exlm[out], hist, t)
        if t == T - 1:
            f = np.where((sb > NEG / 2) & (fin > NEG / 2), sb + fin, NEG)
            q = int(f.argmax())
            if f[q] > NEG / 2:
                best = (float(f[q]), float(slm[q] + fin[q]), H.chain(int(sh[q])))
    return best


def word_projection(res):
    """viterbi_models' result as indep_viterbi_np.viterbi's: (total score, [(label, frame), ...])"""
    if res is None:
        return None
    return res[0], [(lab, t) for (_m, lab, t, _s, _l) in res[2] if lab != 0]
