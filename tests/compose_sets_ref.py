"""Label-SET look-ahead (JD_LOOKAHEAD_SETS, include/juicer_amd.h) written a second time in plain Python - TEST
INFRASTRUCTURE for csrc/jd_labelsets.h and the set paths of csrc/jd_compose.hip / jd_lazy.h.  Nothing here uses
compose_ref.py's interval code: the sets are Python sets, grown by a naive fix-point, and the composition tests
membership in them.

  label_sets      S(c) for every C.L state: the output labels of the first label-carrying arcs reachable through arcs
                  without an output label; None = "every label" (the state lies on a cycle of label-less arcs or
                  reaches one); and mayfin[c]: a final C.L state is reachable through label-less arcs
  compose_sets    C.L o G by the definition at the top of jd_compose.hip with S(c) in place of [lo(c), hi(c)]: the
                  arrays jd_net_get_csr returns, in the (c, f, g) numbering
  permute_words   the same pair of networks with the words renumbered (C.L's output labels and G's INPUT labels; G's
                  output labels - what a composed graph and a hypothesis carry - stay)
  add_variants    C.L with a second pronunciation, in another subtree, for some words: their sets are contiguous under
                  no numbering

label_sets / compose_sets take csr() dictionaries of capi.Network objects (the weights as the loaders scaled them),
permute_words / add_variants take and return synth.SynthNet objects.
"""
import dataclasses

import numpy as np

INF = np.float32(np.inf)


def _rows(cl):
    S = len(cl["row_ptr"]) - 1
    return [[(int(cl["olab"][a]), int(cl["to"][a])) for a in range(int(cl["row_ptr"][c]), int(cl["row_ptr"][c + 1]))] for c in range(S)]


def label_sets(cl):
    rows = _rows(cl)
    S = len(rows)
    less = [[t for (o, t) in rows[c] if o == 0] for c in range(S)]
    # "every label": on a label-less cycle, or an ancestor of such a state
    full = [False] * S
    for c in range(S):
        seen, todo = set(), list(less[c])
        while todo:
            x = todo.pop()
            if x == c:
                full[c] = True
                break
            if x not in seen:
                seen.add(x)
                todo.extend(less[x])
    sets = [set(o for (o, _) in rows[c] if o != 0) for c in range(S)]
    mayfin = [bool(np.isfinite(cl["fin_w"][c])) for c in range(S)]
    changed = True
    while changed:
        changed = False
        for c in range(S):
            for t in less[c]:
                if full[t] and not full[c]:
                    full[c] = changed = True
                if mayfin[t] and not mayfin[c]:
                    mayfin[c] = changed = True
                if not sets[t] <= sets[c]:
                    sets[c] |= sets[t]
                    changed = True
    return [None if full[c] else sets[c] for c in range(S)], mayfin


def compose_sets(cl, cl_init, g, g_init, pushing=False):
    sets, mayfin = label_sets(cl)
    G = []                                               # per G state: label -> (output label, destination, weight), epsilon first
    for s in range(len(g["row_ptr"]) - 1):
        row = {}
        for a in range(int(g["row_ptr"][s]), int(g["row_ptr"][s + 1])):
            assert int(g["ilab"][a]) not in row
            row[int(g["ilab"][a])] = (int(g["olab"][a]), int(g["to"][a]), np.float32(g["w"][a]))
        G.append(row)

    def hits(gs, c):
        """the weights of the arcs of G state gs whose label is in S(c)"""
        if sets[c] is None:
            return [v[2] for l, v in G[gs].items() if l != 0]
        return [G[gs][l][2] for l in sets[c] if l in G[gs]]

    def potential(gs, c):
        ws = hits(gs, c)
        return max(ws) if ws else np.float32(0.0)

    start = (cl_init, 1, g_init)                         # (c, f, g): the canonical order
    arcs_of, fin_of, todo = {}, {}, [start]
    seen = {start}
    while todo:
        c, f, gs = k = todo.pop()
        out = []
        p_src = np.float32(potential(gs, c)) if (pushing and not f) else np.float32(0.0)
        if f and 0 in G[gs]:
            o, t, ww = G[gs][0]
            out.append(((c, 1, t), ww, 0, o))
        for a in range(int(cl["row_ptr"][c]), int(cl["row_ptr"][c + 1])):
            x, t, ww, i = int(cl["olab"][a]), int(cl["to"][a]), np.float32(cl["w"][a]), int(cl["ilab"][a])
            if x == 0:
                if hits(gs, t) or (mayfin[t] and np.isfinite(g["fin_w"][gs])):
                    if pushing:
                        ww = np.float32(np.float32(ww + np.float32(potential(gs, t))) - p_src)
                    out.append(((t, 0, gs), ww, i, 0))
            elif x in G[gs]:
                o, t2, wg = G[gs][x]
                w2 = np.float32(ww + wg)
                out.append(((t, 1, t2), np.float32(w2 - p_src) if pushing else w2, i, o))
        arcs_of[k] = out
        fc, fg = np.float32(cl["fin_w"][c]), np.float32(g["fin_w"][gs])
        fin_of[k] = INF
        if np.isfinite(fc) and np.isfinite(fg):
            fin_of[k] = np.float32(np.float32(fc + fg) - p_src) if pushing else np.float32(fc + fg)
        for (dk, _, _, _) in out:
            if dk not in seen:
                seen.add(dk)
                todo.append(dk)
    keys = sorted(seen)
    idx = {k: n for n, k in enumerate(keys)}
    row_ptr, to, w, il, ol = [0], [], [], [], []
    for k in keys:
        for (dk, ww, i, o) in arcs_of[k]:
            to.append(idx[dk]); w.append(ww); il.append(i); ol.append(o)
        row_ptr.append(len(to))
    return dict(n_states=len(keys), init=idx[start], row_ptr=np.asarray(row_ptr, np.int32), to=np.asarray(to, np.int32),
                w=np.asarray(w, np.float32), ilab=np.asarray(il, np.int32), olab=np.asarray(ol, np.int32),
                fin_w=np.asarray([fin_of[k] for k in keys], np.float32), keys=keys)   # (keys: what each state is, (c, f, g))


def random_perm(cl, g, seed):
    """a random renumbering of the words of (cl, g): perm[old label] = new label, perm[0] = 0"""
    from juicer_amd import synth
    return synth.random_word_permutation(cl, g, seed)


def permute_words(cl, g, perm):
    """C.L's output labels and G's input labels renumbered by perm; G's output labels stay (synth.permute_words, which
    tools/compose_sets_bench.py uses too)"""
    from juicer_amd import synth
    return synth.permute_words(cl, g, perm)


def dfs_numbering(cl, cl_init):
    """{label: n}: the n-th word a depth-first walk from the initial state (arcs in their order; then from the states it did not
    reach) meets first - the internal word numbering of csrc/jd_labelsets.h, under which a set is an interval or a list"""
    rows = [[(int(cl["olab"][a]), int(cl["to"][a])) for a in range(int(cl["row_ptr"][c]), int(cl["row_ptr"][c + 1]))]
            for c in range(len(cl["row_ptr"]) - 1)]
    num, seen = {}, set()
    for r in [cl_init] + list(range(len(rows))):
        if r in seen:
            continue
        seen.add(r)
        stack = [(r, 0)]
        while stack:
            c, a = stack.pop()
            if a == len(rows[c]):
                continue
            stack.append((c, a + 1))
            o, t = rows[c][a]
            if o != 0:
                num.setdefault(o, len(num) + 1)
            elif t not in seen:
                seen.add(t)
                stack.append((t, 0))
    return num


def add_variants(cl, am, words, seed, host=None):
    """For every word in `words` (0-based, as in cl.prons): one more arc carrying its label, from a tree node on ANOTHER
    word's pronunciation - one that starts with a different model - to where word arcs end.  The variant shares that
    word's prefix and ends in the last model of its own first pronunciation.  host: the other word is this one for every
    variant, and the node the one behind its first model (a first-level node that collects all the variants)."""
    rng = np.random.default_rng(seed)
    child = {(int(s), int(i)): int(d) for s, d, i, o in zip(cl.src, cl.dst, cl.ilab, cl.olab) if o == 0}
    word_end = {int(o): int(d) for d, o in zip(cl.dst, cl.olab) if o != 0}
    V = cl.n_words
    src, dst, il, ol, wf = list(cl.src), list(cl.dst), list(cl.ilab), list(cl.olab), list(cl.w_file)
    for w in words:
        others = [v for v in range(V) if cl.prons[v][0] != cl.prons[w][0] and len(cl.prons[v]) >= 2]
        v = others[int(rng.integers(0, len(others)))] if host is None else host
        assert cl.prons[v][0] != cl.prons[w][0]
        nd = 0
        for hm in cl.prons[v][:int(rng.integers(1, len(cl.prons[v]))) if host is None else 1]:
            nd = child[(nd, int(hm) + 1)]
        assert nd != 0
        src.append(nd); dst.append(word_end[w + 1]); il.append(int(cl.prons[w][-1]) + 1); ol.append(w + 1)
        wf.append(float(rng.uniform(0.0, 1.0)))
    order = np.argsort(np.asarray(src), kind="stable")
    A = lambda x, dt: np.asarray(x, dtype=dt)[order]
    return dataclasses.replace(cl, src=A(src, np.int32), dst=A(dst, np.int32), ilab=A(il, np.int32), olab=A(ol, np.int32),
                               w_file=A(wf, np.float32))
