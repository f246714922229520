"""Tied neural acoustic models (jd_am_create_mlp_tied, csrc/jd_mlp.h): logZ restated from the header's text on the CPU oracle's
logAdd (oracle.oracle.log_add_array, the host libm's) - 128 interleaved partial chains, then the chain of the partials -, the serial
chain it must be told apart from, topologies of any number of tied states, and the networks, tyings and shapes the CPU and GPU
tests share.  tests/mlp_cases.py supplies the rest (networks, rows, priors, the JMLP bytes)."""
import numpy as np

import mlp_cases as mc

LZ = mc.LZ
LZ_CHAINS = 128                                           # jd_mlp.h: JD_MLP_LZ_CHAINS
MAX_OUT = 16384                                           # jd_mlp.h: JD_MLP_MAX_OUT

# the widths of the definition test (CPU) and of the device test (GPU): either side of an n-tile pair (16, 32), of the 8-tile turn
# and the 128 chains (127 .. 130, 255, 257), of the old LDS limit (1024, 1025, 1040), and one that is no multiple of anything
LOGZ_WIDTHS = (1, 15, 127, 128, 129, 257, 1025, 2063)
DEVICE_WIDTHS = (1, 15, 16, 17, 127, 128, 129, 130, 255, 257, 1024, 1025, 1040, 2063)
DEVICE_HIDDEN = (1, 16, 33)
DEVICE_ROWS = (1, 15, 16, 17, 33)


def logz_tied(z):
    """z [n, P] float32 -> logZ [n]: p[c] = the logAdd chain from LZ over z[c], z[c + 128], ... (c < min(128, P)), then the logAdd
    chain from LZ over p[0], p[1], ...; chains c >= P are empty and not combined"""
    from oracle.oracle import log_add_array
    z = np.ascontiguousarray(z, np.float32)
    n, P = z.shape
    p = np.full((n, LZ_CHAINS), LZ, np.float32)
    for t in range(0, P, LZ_CHAINS):                       # step t of every chain at once: element c + t
        seg = np.ascontiguousarray(z[:, t:t + LZ_CHAINS])
        w = seg.shape[1]
        p[:, :w] = log_add_array(np.ascontiguousarray(p[:, :w]).ravel(), seg.ravel()).reshape(n, w)
    lz = np.full(n, LZ, np.float32)
    for c in range(min(LZ_CHAINS, P)):
        lz = log_add_array(lz, np.ascontiguousarray(p[:, c]))
    return lz


def logz_serial(z):
    """the one chain over z[0], z[1], ... (the phone models' logZ)"""
    from oracle.oracle import log_add_array
    z = np.ascontiguousarray(z, np.float32)
    lz = np.full(z.shape[0], LZ, np.float32)
    for j in range(z.shape[1]):
        lz = log_add_array(lz, np.ascontiguousarray(z[:, j]))
    return lz


def logpost_of(z, lz):
    with np.errstate(all="ignore"):
        return (np.asarray(z, np.float32) - np.asarray(lz, np.float32)[:, None]).astype(np.float32)


def forward_f64(layers, x):
    return mc.forward_f64(layers, x)


# ---- topologies
def flat_topology(n_gmm, states=3):
    """a SynthAM of n_gmm tied states, one HMM of `states` states per tied state, D = 1: the least that carries n_gmm outputs"""
    from juicer_amd import synth
    hg = np.full((n_gmm, states), -1, np.int32)
    hg[:, 1:states - 1] = np.arange(n_gmm, dtype=np.int32)[:, None]
    tp = np.zeros((1, states, states), np.float32)
    tp[0, 0, 1] = 1.0
    for i in range(1, states - 1):
        tp[0, i, i] = tp[0, i, i + 1] = 0.5
    return synth.SynthAM(D=1, n_gmm=n_gmm, max_mix=1, n_mix=np.ones(n_gmm, np.int32), weight=np.ones((n_gmm, 1), np.float32),
                         mean=np.zeros((n_gmm, 1, 1), np.float32), var=np.ones((n_gmm, 1, 1), np.float32), n_hmm=n_gmm, max_n=states,
                         hmm_nstates=np.full(n_gmm, states, np.int32), hmm_gmm=hg, hmm_tm=np.zeros(n_gmm, np.int32), n_tm=1,
                         tm_nstates=np.full(1, states, np.int32), transp=tp)


def tied_models(layers, seed=0):
    """capi models of a network over flat_topology(its outputs), and the priors"""
    from juicer_amd import capi
    P = layers[-1][0].shape[0]
    pr = mc.priors(seed, P)
    return capi.Models.from_mlp_tied(capi.Models.from_htk(flat_topology(P)), pr, layers), pr


def net_for(P, hidden=(16,), in_dim=9, seed=0, scale=1.0):
    acts = [(mc.SIGMOID, mc.RELU, mc.LINEAR)[i % 3] for i in range(len(hidden))]
    return mc.random_net(seed, in_dim, list(hidden) + [P], acts, scale)


# ---- the oracle anchor for tying: synth.config_hybrid's graph over 30 one-per-phone HMMs, whose emitting states are TIED to 22
# states: HMMs h and h + 22 (h < 8) share one, so 16 of the 30 HMMs share theirs with another
ANCHOR_PHONES, ANCHOR_TIED = 30, 22


def anchor_tying():
    t = np.arange(ANCHOR_PHONES, dtype=np.int32) % ANCHOR_TIED
    shared = sum(1 for h in range(ANCHOR_PHONES) if (t == t[h]).sum() > 1)
    assert ANCHOR_TIED < ANCHOR_PHONES and 3 * shared >= ANCHOR_PHONES
    return t


def anchor_topology(spm):
    """config_hybrid's topology (jd_am_create_hybrid: one transition matrix, 1.0 into the first emitting state, 0.5 / 0.5) as
    GMM-style arrays, all emitting states of HMM h tied to state t(h)"""
    from juicer_amd import synth
    t = anchor_tying()
    H, G = ANCHOR_PHONES, ANCHOR_TIED
    hg = np.full((H, spm), -1, np.int32)
    hg[:, 1:spm - 1] = t[:, None]
    tp = np.zeros((1, spm, spm), np.float32)
    tp[0, 0, 1] = 1.0
    for i in range(1, spm - 1):
        tp[0, i, i] = tp[0, i, i + 1] = 0.5
    return synth.SynthAM(D=1, n_gmm=G, max_mix=1, n_mix=np.ones(G, np.int32), weight=np.ones((G, 1), np.float32),
                         mean=np.zeros((G, 1, 1), np.float32), var=np.ones((G, 1, 1), np.float32), n_hmm=H, max_n=spm,
                         hmm_nstates=np.full(H, spm, np.int32), hmm_gmm=hg, hmm_tm=np.zeros(H, np.int32), n_tm=1,
                         tm_nstates=np.full(1, spm, np.int32), transp=tp)


def anchor_net(seed, noise=mc.DECODE_NOISE):
    """mlp_cases.decode_net with a tied output layer: W1 = [I; -I] + noise N with ReLU (the phone log posteriors pass through),
    W2 = T [I, -I] + noise N, T [tied, phone] the MEAN over the phones tied to a state; no biases"""
    rng = np.random.default_rng(seed)
    n, t = ANCHOR_PHONES, anchor_tying()
    eye = np.eye(n)
    T = np.zeros((ANCHOR_TIED, n))
    T[t, np.arange(n)] = 1.0
    T /= T.sum(axis=1, keepdims=True)
    w1 = (np.vstack([eye, -eye]) + noise * rng.standard_normal((2 * n, n))).astype(np.float32)
    w2 = (T @ np.hstack([eye, -eye]) + noise * rng.standard_normal((ANCHOR_TIED, 2 * n))).astype(np.float32)
    return [(w1, np.zeros(2 * n, np.float32), mc.RELU), (w2, np.zeros(ANCHOR_TIED, np.float32), mc.LINEAR)]


def anchor_case(spm):
    """(topology SynthAM, graph, utterances [T, 30], tied priors [22], layers, the tying) - seeds chosen so that the CPU oracle
    certifies every utterance under mlp_cases.DECODE_BEAMS (tests/test_mlp_tied_cpu.py asserts it)"""
    from juicer_amd import synth
    _, net, feats, _ = synth.config_hybrid(seed=3 + spm, states_per_model=spm)
    return anchor_topology(spm), net, feats, mc.priors(40 + spm, ANCHOR_TIED), anchor_net(seed=spm), anchor_tying()


def anchor_oracle_inputs(logpost, priors, tying):
    """what the oracle's hybrid decoder (one output per HMM) is fed: x'[:, h] = logpost[:, t(h)], priors'[h] = priors[t(h)] - it
    then computes x'[h] - log(priors'[h]), the tied models' own float operations"""
    return np.ascontiguousarray(np.asarray(logpost, np.float32)[:, tying]), np.asarray(priors, np.float32)[tying]


# ---- arbitrary topology: synth.make_models_mixed (1 to 6 emitting states, a tee model, real state tying) under a graph of
# indep_cases' kind; the network's inputs are the frames' normalised GMM log-likelihoods (so that paths stay well apart), passed
# through mlp_cases.decode_net
def mixed_case():
    from juicer_amd import synth
    import indep_viterbi_np as iv
    am, net, feats, _ = synth.config_mixed(seed=23, n_utts=2, n_words=120, n_succ=5)
    xs = []
    for x in feats:
        ll = iv.gmm_loglik(am, x)
        m = ll.max(axis=1, keepdims=True)
        xs.append((ll - (m + np.log(np.exp(ll - m).sum(axis=1, keepdims=True)))).astype(np.float32))
    return am, net, xs, mc.priors(9, am.n_gmm), mc.decode_net(am.n_gmm, seed=9, noise=0.01)


# ---- crafted rows through the tied path: (name, layers, rows, expected log posteriors; None = NaN)
def crafted():
    f = np.float32
    cs = []
    P = 130                                                # two elements in chains 0 and 1, one in the others
    eye = [(np.eye(P, dtype=f), np.zeros(P, f), mc.LINEAR)]
    # a NaN row is NaN in that row and nowhere else
    x = np.zeros((3, P), f)
    x[1, 5] = np.nan
    lz0 = logz_tied(np.zeros((1, P), f))[0]
    cs.append(("NaN row", eye, x, np.stack([np.full(P, f(0.0) - lz0, f), np.full(P, np.nan, f), np.full(P, f(0.0) - lz0, f)])))
    # one logit dominates past the -18.42 cut, in its partial chain and in the chain of the partials: logZ is that logit exactly
    x = np.full((1, P), -30.0, f)
    x[0, 129] = 50.0
    want = x - f(50.0)
    cs.append(("dominant logit", eye, x, want.astype(f)))
    # all-equal logits: the log posteriors are one value, -logZ of the zeros by the definition
    x = np.full((2, P), 3.5, f)
    lz = logz_tied(x)
    cs.append(("all equal", eye, x, logpost_of(x, lz)))
    return cs
