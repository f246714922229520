"""The CURRENT BEST hypothesis by the float64 full-trellis Viterbi of tests/indep_viterbi_models.py - test infrastructure, not
product code.

The same recurrences and the same records (a record whenever a token leaves an arc with an in-label or crosses an epsilon-input
arc with an output label), looked at BEHIND chosen frames instead of at the end: after frame t the best token is the argmax over
all (arc, emitting state) cells of the trellis, its hypothesis the record chain its back-pointer holds.  Entry cells (state 0)
are no candidates: they have not been scored on a frame.  Beside the argmax the margin to the best cell with ANOTHER record
chain is returned - the distance a float32 search may close - and the margin to the best other cell whatever its chain."""
import numpy as np

from indep_viterbi_np import NEG, _best_per_key, gmm_loglik  # noqa: F401  (gmm_loglik: for the callers)
from indep_viterbi_models import _Hist


def viterbi_best(net, am, ll, frames, lm_scale=1.0, ins_penalty=0.0):
    """frames: numbers of frames pushed (1 .. T) to look behind.  Returns {f: dict or None} with, for the best emitting cell after
    frame f - 1: score, lm, model (the arc's in-label), state, chain [(model, label, frame, score, lm), ...] oldest first, margin
    (score minus the best score among cells whose record chain differs; inf: none) and cell_margin (... among all other cells)."""
    want = set(int(f) for f in frames)
    src, dst, il, ol = (np.asarray(a, np.int64) for a in (net.src, net.dst, net.ilab, net.olab))
    w = -net.w_file.astype(np.float64) * lm_scale + np.where(ol > 0, ins_penalty, 0.0)
    nS = int(max(net.n_states, src.max() + 1, dst.max() + 1))
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

    def look(S, Sh, Slm):
        flat = np.where(emitting, S, NEG).ravel()
        b = int(flat.argmax())
        if flat[b] <= NEG / 2:
            return None
        a, j = divmod(b, MN)
        chain = H.chain(int(Sh[a, j]))
        ids = [(m, lab, t) for (m, lab, t, _s, _l) in chain]
        order = np.argsort(-flat, kind="stable")
        margin, cell_margin = np.inf, np.inf
        for o in order[1:]:
            if flat[o] <= NEG / 2:
                break
            cell_margin = min(cell_margin, flat[b] - flat[o])
            a2, j2 = divmod(int(o), MN)
            if Sh[a2, j2] == Sh[a, j]:
                continue
            if [(m, lab, t) for (m, lab, t, _s, _l) in H.chain(int(Sh[a2, j2]))] != ids:
                margin = float(flat[b] - flat[o])
                break
        return dict(score=float(flat[b]), lm=float(Slm[a, j]), model=int(il[marc[a]]), state=int(j), chain=chain,
                    margin=float(margin), cell_margin=float(cell_margin))

    sb, slm, sh = expand(np.array([init]), np.array([0.0]), np.array([0.0]), np.array([-1], np.int64), 0)
    S = np.full((marc.shape[0], MN), NEG); Sh = np.full((marc.shape[0], MN), -1, np.int64); Slm = np.zeros((marc.shape[0], MN))
    out = {}
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
        if t + 1 in want:
            out[t + 1] = look(S, Sh, Slm)
        if t + 1 >= max(want):
            break
        outs = np.nonzero(ex > NEG / 2)[0]
        a_arc = marc[outs]
        hist = H.add(il[a_arc], ol[a_arc], t, ex[outs], exlm[outs], exh[outs])     # every model exit is a record
        sb, slm, sh = expand(dst[a_arc], ex[outs], exlm[outs], hist, t)
    return out
