"""Context splicing of neural acoustic models (csrc/jd_splice.h), restated with numpy from the header's text: the window, the
spans of utterances that lie back to back, the push plan's promises - and the shapes, utterances and row maps the CPU and GPU tests share."""
import numpy as np

import mlp_cases as mc


def splice(frames, left, right):
    """x[t, c D + d] = frames[clamp(t + c - left, 0, T - 1), d], c = 0 .. left + right: ONE utterance [T, D] -> [T, (left + right + 1) D]"""
    frames = np.ascontiguousarray(frames, np.float32)
    T, D = frames.shape
    C = left + right + 1
    if T == 0:
        return np.zeros((0, C * D), np.float32)
    idx = np.clip(np.arange(T)[:, None] + np.arange(C)[None, :] - left, 0, T - 1)
    return np.ascontiguousarray(frames[idx].reshape(T, C * D))


def windows(T, left, right):
    """[T, C] the frames of every row's window"""
    C = left + right + 1
    return np.clip(np.arange(T)[:, None] + np.arange(C)[None, :] - left, 0, max(T - 1, 0)).astype(np.int32)


def utterance_spans(lengths):
    """utterances back to back: (first frame, last frame) of the utterance of every frame, and the utterances' first frames"""
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    lo = np.concatenate([np.full(n, starts[u], np.int32) for u, n in enumerate(lengths)]) if len(lengths) else np.zeros(0, np.int32)
    hi = np.concatenate([np.full(n, starts[u] + n - 1, np.int32) for u, n in enumerate(lengths)]) if len(lengths) else np.zeros(0, np.int32)
    return lo.astype(np.int32), hi.astype(np.int32), starts


def splice_utterances(frames, lengths, left, right):
    """every utterance spliced on its own, back to back again"""
    _, _, starts = utterance_spans(lengths)
    return np.concatenate([splice(frames[starts[u]:starts[u] + n], left, right) for u, n in enumerate(lengths)])


# ---- the GPU shapes: (D, left, right, widths); hidden activations alternate
SHAPES = [
    (1, 1, 1, [5, 3]),                  # the smallest case
    (13, 2, 0, [20, 7]), (13, 0, 3, [20, 7]),       # one-sided contexts
    (5, 3, 3, [24, 9]),                 # 35 inputs: pieces straddle the 16- and 32-input k groups
    (39, 4, 4, [48, 45]),               # the real shape
    (64, 8, 7, [32, 10]),               # 1024 inputs: the limit
]
TIED_OUTPUTS = 300                      # more than the 128 logZ chains
# utterances back to back: boundaries inside a 16-row and a 32-row tile, utterances shorter than either context
UTTERANCES = [1, 2, 3, 40, 1, 17]


def shape_id(s):
    return "D%d-%d+%d-%s" % (s[0], s[1], s[2], "-".join(str(w) for w in s[3]))


def parent_layers(shape, seed, tied=False):
    D, left, right, widths = shape
    widths = list(widths[:-1]) + [TIED_OUTPUTS] if tied else list(widths)
    acts = [(mc.SIGMOID, mc.RELU)[i % 2] for i in range(len(widths) - 1)]
    return mc.random_net(seed, D * (left + right + 1), widths, acts)


def raw_frames(seed, n, D):
    return np.random.default_rng(seed + 4242).standard_normal((n, D)).astype(np.float32)


def row_maps(n_frames, seed):
    """(name, row_src) over frames [0, n_frames): the identity; a permutation with -1 holes whose length is no multiple of a tile"""
    rng = np.random.default_rng(seed)
    ident = np.arange(n_frames, dtype=np.int32)
    perm = rng.permutation(n_frames).astype(np.int32)
    perm = np.concatenate([perm, rng.integers(0, n_frames, 9).astype(np.int32)])      # 64 + 9 rows: neither 16 nor 32 divides it
    perm[rng.choice(perm.shape[0], 11, replace=False)] = -1
    perm[32:48] = -1                                                                    # a 16-row tile without a used row
    return [("identity", ident), ("permuted", perm)]


# ---- the push plan: every composition of T into parts of 1 .. max_part, and each again with an empty push in front of every part
def compositions(T, max_part):
    if T == 0:
        yield ()
        return
    for p in range(1, min(max_part, T) + 1):
        for rest in compositions(T - p, max_part):
            yield (p,) + rest


def push_sequences(T, max_part=5):
    for c in compositions(T, max_part):
        yield c
        z = []
        for p in c:
            z += [0, p]
        yield tuple(z + [0])
