"""Cases for jd_debug_score_rows (include/juicer_amd.h): launch_gmm called as the decoder's paths call it - a row map with repeats and
unused (-1) rows, skip_unused, a bounded grid, a tile list, the choice between the tiles of 16 and of 64 tied states - and, for every cell
of the guarded output buffer, what the launch must leave there.  Pure numpy plus the CPU oracle: tests/test_score_rows_cpu.py checks the
cases themselves without a GPU, tests/test_gpu_score_rows.py runs them through the kernels.

A cell (row, tied state) of the buffer [(guard + n_rows + guard)][G] is exactly one of
  UNTOUCHED    guard rows; rows of a tile that is not scored (not listed, or dropped because skip_unused is set and its first row is
               unused).  The cell still holds the prefill pattern, bit for bit.
  VALUE        a row with a source frame inside a scored tile: OracleAM.score_frames(frames[row_src[r]])[g] - bit for bit under
               JD_SCORE_EXACT (any NaN equals any NaN), within RTOL relative under JD_SCORE_FAST where the oracle's cell is finite - and
               never the prefill pattern.  Rows that share a source frame hold identical bits.
  UNSPECIFIED  an unused row inside a scored tile: nobody reads it.  At most UNSPEC_CAP of the cells of rows [0, n_rows) - except the
               case the row map `d` exists for with skip_unused = 0: two of five tiles are unused and scored all the same (2 / 5).

Tile rows: 64 for jd_gmm_kernel<0>, 128 for jd_gmm_kernel39 / jd_gmm_fast39 / jd_gmm_fast, none for jd_hybrid_kernel (every row with a source
is a VALUE row there, whatever skip_unused says).

Where the cases differ from a literal reading of what was asked for, and why:
  * row map c under skip_unused = 1: the entry refuses a scored tile whose used rows are not a prefix of it (the kernels' stated
    precondition), so the holes there are TAILS - a tile used up to four rows before its lane-half boundary (a hole in each lane half and
    the whole second half unused), a last tile with an unused tail - while skip_unused = 0 takes scattered holes.
  * row map f: 3 row tiles x as many state tiles as the kernel's width makes of 150 states (3 at 64 states per tile, 10 at 16).  The
    hybrid kernel has no tiles and launch_gmm bounds no grid for it: its "f" is row map c with max_blocks = 1, which must change nothing.

The oracle is not the only witness of the expected values: on the random models its finite cells are held to the float64
tests/indep_viterbi_np.gmm_loglik.  Largest relative deviation |oracle - float64| / max(1, |float64|) MEASURED on the CPU (40 frames x the
models below, all G), per vector size; the asserted bound is FOUR TIMES that (float32 sums of 13 to 65 terms vary with the data):"""
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np

from logadd_cases import crafted_model, same_floats, table_frames

F64_MEASURED = {13: 3.309e-07, 40: 3.837e-07, 65: 5.278e-07}
F64_BOUND = {D: 4.0 * m for D, m in F64_MEASURED.items()}

UNTOUCHED, VALUE, UNSPEC = 0, 1, 2
UNSPEC_CAP = 0.25
N_FRAMES = 40
NAN_FRAME, PAIR_FRAME = 2, 7                              # the frame with a NaN feature; the frame of a lane's two rows
CLEAN = [0, 1, 5, 6, 10, 11, 15, 16]                      # crafted table: rows of kind 0 / 1 (the means, random) - no NaN feature, no overflow
SYNTH_DIMS, SYNTH_G = [13, 40, 65], [1, 17, 65, 150]
SYNTH_MAX_MIX = 11                                        # > GMM_FAST_MB = 8: two blocks of mixtures, the second short or empty
N_PHONES = 40

# the kernels (capi.KERNEL_*, jd_score_kernel of include/juicer_amd.h)
(K_NONE, K_GENERIC, K_GMM39_16, K_GMM39_64, K_FAST39_16, K_FAST39_64, K_FAST_16, K_FAST_64, K_HYBRID) = range(9)
KERNEL_NAMES = ["none", "jd_gmm_kernel<0>", "jd_gmm_kernel39<16>", "jd_gmm_kernel39<64>", "jd_gmm_fast39<16>", "jd_gmm_fast39<64>",
                "jd_gmm_fast<16>", "jd_gmm_fast<64>", "jd_hybrid_kernel"]
TILE_ROWS = {K_GENERIC: 64, K_GMM39_16: 128, K_GMM39_64: 128, K_FAST39_16: 128, K_FAST39_64: 128, K_FAST_16: 128, K_FAST_64: 128, K_HYBRID: 0}
TILE_STATES = {K_GENERIC: 64, K_GMM39_16: 16, K_GMM39_64: 64, K_FAST39_16: 16, K_FAST39_64: 64, K_FAST_16: 16, K_FAST_64: 64}
FAST_KERNELS = (K_FAST39_16, K_FAST39_64, K_FAST_16, K_FAST_64)
LIST_KERNELS = (K_GMM39_16, K_GMM39_64, K_FAST39_16, K_FAST39_64, K_FAST_16, K_FAST_64)
SCORE_EXACT, SCORE_FAST = 0, 1


# ---------------------------------------------------------------------------------------------------------------- models

def ragged_models(D, G):
    """synth.make_models with 1..SYNTH_MAX_MIX mixtures per state (both ends present where G allows), weights renormalised"""
    from juicer_amd import synth
    seed = 1000 * D + G
    am = synth.make_models(seed, n_gmm=G, n_hmm=max(4, G // 3), n_mix=SYNTH_MAX_MIX, D=D, n_tm=4)
    rng = np.random.default_rng(seed + 77)
    am.n_mix = rng.integers(1, SYNTH_MAX_MIX + 1, size=G).astype(np.int32)
    am.n_mix[0] = SYNTH_MAX_MIX
    if G > 1:
        am.n_mix[1] = 1
    w = am.weight.astype(np.float64) * (np.arange(SYNTH_MAX_MIX)[None, :] < am.n_mix[:, None])
    am.weight = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    am.weight[am.n_mix == 1, 0] = 1.0
    return am


def synth_frames(am):
    """frames near the models (a component's mean plus noise of its own variance); frame NAN_FRAME has a NaN feature"""
    rng = np.random.default_rng(am.D * 31 + am.n_gmm)
    g = rng.integers(0, am.n_gmm, size=N_FRAMES)
    x = (am.mean[g, 0] + rng.normal(0.0, 1.0, size=(N_FRAMES, am.D)) * np.sqrt(am.var[g, 0])).astype(np.float32)
    x[NAN_FRAME, NAN_FRAME % am.D] = np.nan
    return x


@dataclass
class Model:
    key: str
    kind: str                     # "crafted" (capi.Models.from_flat), "synth" (from_htk), "hybrid" (from_hybrid)
    D: int
    G: int
    frames: np.ndarray            # [N_FRAMES][D]
    args: tuple                   # what the constructors take
    am: object = None             # synth: the SynthAM (tests/indep_viterbi_np.gmm_loglik reads it)

    def oracle_table(self):
        """OracleAM.score_frames of the N_FRAMES frames, [N_FRAMES][G] (computed once)"""
        return _oracle_table(self.key)

    def gpu_models(self):
        from juicer_amd import capi
        if self.kind == "crafted":
            return capi.Models.from_flat(*self.args)
        if self.kind == "synth":
            return capi.Models.from_htk(self.am)
        return capi.Models.from_hybrid(*self.args)


@functools.lru_cache(maxsize=None)
def model(key):
    """"crafted39" - the crafted D = 39 table of tests/test_gpu_logadd.py (150 states, chains of up to 24 mixtures; the five row kinds of
    table_frames: frame 2 has a NaN feature, frame 3 overflows); "synth<D>_<G>"; "hybrid" - 40 phones, log-posterior frames"""
    if key == "crafted39":
        det, mean, ivar, n_mix = crafted_model(39, 150, seed=11)
        return Model(key, "crafted", 39, 150, table_frames(39, N_FRAMES, seed=11), (det, mean, ivar, n_mix))
    if key == "hybrid":
        rng = np.random.default_rng(4)
        pri = rng.uniform(0.5, 2.0, size=N_PHONES)
        logit = rng.normal(size=(N_FRAMES, N_PHONES))
        logit[np.arange(N_FRAMES), rng.integers(0, N_PHONES, N_FRAMES)] += 4.0
        x = (logit - np.log(np.exp(logit).sum(axis=1, keepdims=True))).astype(np.float32)
        return Model(key, "hybrid", N_PHONES, N_PHONES, x, ((pri / pri.sum()).astype(np.float32), 5))
    D, G = (int(v) for v in key[len("synth"):].split("_"))
    am = ragged_models(D, G)
    return Model(key, "synth", D, G, synth_frames(am), (), am)


@functools.lru_cache(maxsize=None)
def _oracle_table(key):
    from oracle.oracle import OracleAM
    m = model(key)
    if m.kind == "crafted":
        o = OracleAM.from_flat(*m.args)
    elif m.kind == "synth":
        o = OracleAM(m.am)
    else:
        o = OracleAM.from_hybrid(*m.args)
    t = o.score_frames(m.frames)
    assert t.shape == (N_FRAMES, m.G)
    t.setflags(write=False)
    return t


# ---------------------------------------------------------------------------------------------------------------- cases

@dataclass
class Case:
    id: str
    model_key: str
    kernel: int
    row_src: np.ndarray
    skip_unused: int = 0
    max_blocks: int = 0
    used_row_tiles: int = -1
    rt_base: Optional[np.ndarray] = None
    feature: str = ""             # what the case is named for (tests/test_score_rows_cpu.py looks for it in the case)
    unspec_cap: float = UNSPEC_CAP

    @property
    def mode(self):
        return SCORE_FAST if self.kernel in FAST_KERNELS else SCORE_EXACT

    @property
    def h(self):
        return TILE_ROWS[self.kernel]

    @property
    def n_rows(self):
        return int(self.row_src.shape[0])

    @property
    def guard_rows(self):
        """a tile's rows on either side: a store that ignores n_rows, or a tile one too far, lands in the guard and not outside the buffer"""
        return self.h or 4

    def scored_tiles(self):
        """first rows of the tiles the launch scores (tile kernels)"""
        h = self.h
        first = [int(r) for r in self.rt_base] if self.rt_base is not None else list(range(0, self.n_rows, h))
        if self.skip_unused:
            first = [r0 for r0 in first if self.row_src[r0] >= 0]
        return first

    def row_tiles(self):
        """the row tiles the launch goes through, skipped ones included"""
        return len(self.rt_base) if self.rt_base is not None else -(-self.n_rows // self.h)

    def grid(self):
        """the workgroups launch_gmm asks for"""
        G = model(self.model_key).G
        if self.kernel == K_HYBRID:
            return -(-self.n_rows * G // 256)
        tiles = self.row_tiles() * -(-G // TILE_STATES[self.kernel])
        return min(tiles, self.max_blocks) if self.max_blocks > 0 else tiles

    def prefill(self):
        """[(guard + n_rows + guard)][G] float32 of bit patterns no likelihood can take, every cell its own: NaNs with the sign bit, payload
        bit 21 and the cell's number below it (the kernels' own NaNs are the canonical one or a frame's)"""
        G = model(self.model_key).G
        n = (self.n_rows + 2 * self.guard_rows) * G
        bits = np.uint32(0xFFE00000) | (np.arange(n, dtype=np.uint32) & np.uint32(0x1FFFFF))
        return bits.view(np.float32).reshape(-1, G)

    def classify(self):
        """(cls [(guard + n_rows + guard)][G] of UNTOUCHED / VALUE / UNSPEC, want - the same shape, the oracle's value in the VALUE cells)"""
        m = model(self.model_key)
        gr, n = self.guard_rows, self.n_rows
        row_cls = np.full(n + 2 * gr, UNTOUCHED, np.int8)
        hits = np.zeros(n, np.int32)                                  # how many scored tiles hold the row: once at the most
        src = self.row_src
        if self.kernel == K_HYBRID:
            hits += 1
            row_cls[gr:gr + n] = np.where(src >= 0, VALUE, UNSPEC)
        else:
            for r0 in self.scored_tiles():
                r1 = min(n, r0 + self.h)
                hits[r0:r1] += 1
                row_cls[gr + r0:gr + r1] = np.where(src[r0:r1] >= 0, VALUE, UNSPEC)
        assert hits.max() <= 1, "%s: scored tiles overlap" % self.id
        cls = np.repeat(row_cls[:, None], m.G, axis=1)
        want = np.zeros((n + 2 * gr, m.G), np.float32)
        used = src >= 0
        want[gr:gr + n][used] = m.oracle_table()[src[used]]
        want[cls != VALUE] = 0.0
        unspec = float((cls[gr:gr + n] == UNSPEC).mean()) if n else 0.0
        assert unspec <= self.unspec_cap + 1e-12, "%s: %.3f of the cells unspecified" % (self.id, unspec)
        return cls, want


def check_buffer(case, got, rtol):
    """the three cell classes of `got` (what jd_debug_score_rows brought back); raises AssertionError with the first offending cell"""
    cls, want = case.classify()
    pre = case.prefill()
    assert got.shape == pre.shape and got.dtype == np.float32
    gb, pb = got.view(np.uint32), pre.view(np.uint32)
    gr = case.guard_rows

    def where(bad):
        r, g = np.argwhere(bad)[0]
        return "%d cells; first: buffer row %d (table row %d, source %s) state %d: got %s, want %s" % (
            int(bad.sum()), r, r - gr, case.row_src[r - gr] if 0 <= r - gr < case.n_rows else "-", g, float(got[r, g]).hex(), float(want[r, g]).hex())

    bad = (cls == UNTOUCHED) & (gb != pb)
    assert not bad.any(), "%s: written where nothing must be written: %s" % (case.id, where(bad))
    val = cls == VALUE
    bad = val & (gb == pb)
    assert not bad.any(), "%s: never written: %s" % (case.id, where(bad))
    if case.mode == SCORE_EXACT:
        bad = val & ~((np.isnan(got) & np.isnan(want)) | (gb == want.view(np.uint32)))
        assert not bad.any(), "%s: differs from the oracle: %s" % (case.id, where(bad))
    else:
        fin = val & np.isfinite(want)                                  # (most of them: tests/test_score_rows_cpu.py)
        w = want.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs(got.astype(np.float64) - w) / np.maximum(1.0, np.abs(w))
        bad = fin & ~(err <= rtol)
        assert not bad.any(), "%s: beyond %g relative: %s" % (case.id, rtol, where(bad))
    # rows that share a source frame: identical bits
    src = case.row_src
    row_val = val[gr:gr + case.n_rows, 0] if case.n_rows else np.zeros(0, bool)
    firsts = {}
    for r in np.nonzero(row_val)[0]:
        f = int(src[r])
        if f in firsts:
            assert np.array_equal(gb[gr + r], gb[gr + firsts[f]]), "%s: rows %d and %d of frame %d differ" % (case.id, firsts[f], r, f)
        else:
            firsts[f] = int(r)
    return True


def _wide_urt(G):
    """a used_row_tiles at which launch_gmm takes the tiles of 64 states (>= 1024 of them)"""
    return -(-1024 // -(-G // 64))


def _random_map(rng, n, clean_only=False):
    if clean_only:
        return np.asarray(CLEAN, np.int32)[rng.integers(0, len(CLEAN), n)]
    return rng.integers(0, N_FRAMES, n).astype(np.int32)


def _maps(h, n_gt, rng):
    """the row maps a-d and f of a tile kernel of h rows per tile: (id, row_src, skip_unused, max_blocks list or None, feature, cap)"""
    out = []
    half = h // 2
    # a. random with repeats; PAIR_FRAME at both rows of a lane (r, r + 64) and once more in another tile
    for n in (1, h - 1, h, h + 1, 2 * h + 1):
        src = _random_map(rng, n)
        for r in (5, 5 + 64, h):
            if r < n:
                src[r] = PAIR_FRAME
        out.append(("a%d" % n, src, 0, None, "pair" if n > 5 + 64 else "", UNSPEC_CAP))
    # b. the NaN frame at one row, clean frames on either side and a lane half away; nowhere else
    n = 200
    src = _random_map(rng, n, clean_only=True)
    src[70] = NAN_FRAME
    out.append(("b", src, 0, None, "nan", UNSPEC_CAP))
    # c. holes.  skip_unused = 0: scattered, and the whole second half of tile 1
    n = 2 * h + 40
    src = _random_map(rng, n)
    src[[3, 17, half + 9, h - 1, 2 * h + 2]] = -1
    src[h + half:2 * h] = -1
    out.append(("c_scattered", src, 0, None, "holes", UNSPEC_CAP))
    # ... skip_unused = 1: tails (the entry refuses anything else) - tile 1 used up to 4 rows before its second half, the last tile's tail
    src = _random_map(rng, n)
    src[h + half - 4:2 * h] = -1
    src[2 * h + 36:] = -1
    for skip in (0, 1):
        out.append(("c_tails_skip%d" % skip, src.copy(), skip, None, "holes", UNSPEC_CAP))
    # d. five tiles, the second and the fourth unused
    src = _random_map(rng, 5 * h)
    src[h:2 * h] = -1
    src[3 * h:4 * h] = -1
    out.append(("d_skip1", src.copy(), 1, None, "skipped", UNSPEC_CAP))
    out.append(("d_skip0", src.copy(), 0, None, "unused_scored", 0.4))
    # f. a bounded grid over 3 row tiles x n_gt state groups with one row tile skipped.  The kernels take row tile (tile + gt) % n_rt of
    # state group gt = tile / n_rt; under max_blocks = n_rt n_gt - 1 only workgroup 0 takes a second stride step, from tile 0 (row tile 0)
    # to the last tile.  The skipped row tile is the one that is neither, so that BOTH are scored (row tile 2 at 3 state groups, 1 at 10) -
    # tests/test_score_rows_cpu.py holds every bounded case to "some workgroup scores two tiles"
    n_rt = 3
    last = (n_rt * n_gt - 1 + n_gt - 1) % n_rt
    skipped = [t for t in range(n_rt) if t not in (0, last)][-1]
    src = _random_map(rng, n_rt * h)
    src[skipped * h:(skipped + 1) * h] = -1
    out.append(("f", src, 1, "bounds", "skipped", UNSPEC_CAP))
    return out


def _build_cases():
    cases = []
    rng = np.random.default_rng(2024)

    def tile_kernel(model_key, kernel, with_lists, only=None):
        G = model(model_key).G
        h = TILE_ROWS[kernel]
        urt = _wide_urt(G) if (kernel in LIST_KERNELS and TILE_STATES[kernel] == 64) else -1
        name = "%s-%s" % (KERNEL_NAMES[kernel], model_key)
        for mid, src, skip, bounds, feat, cap in _maps(h, -(-G // TILE_STATES[kernel]), rng):
            if only is not None and mid not in only:
                continue
            if bounds is None:
                cases.append(Case("%s-%s" % (name, mid), model_key, kernel, src, skip, 0, urt, None, feat, cap))
            else:
                n_rt, n_gt = 3, -(-G // TILE_STATES[kernel])
                for mb in sorted({1, n_rt, n_rt * n_gt - 1}):
                    cases.append(Case("%s-%s_blocks%d" % (name, mid, mb), model_key, kernel, src.copy(), skip, mb, urt, None, feat, cap))
        if not with_lists:
            return
        # e. tile lists over a six-tile table; the small kernels get the number of listed tiles, as jd_res_stage_many passes it
        for lid, n, lst in (("e_412", 6 * h, [4 * h, 1 * h, 2 * h]), ("e_one", 6 * h, [3 * h]), ("e_cut", 5 * h + 37, [5 * h, 2 * h])):
            src = _random_map(rng, n)
            cases.append(Case("%s-%s" % (name, lid), model_key, kernel, src, 0, 0, urt if urt >= 0 else len(lst), np.asarray(lst, np.int32),
                              "cut" if lid == "e_cut" else "unlisted"))

    for k in (K_GMM39_16, K_GMM39_64, K_FAST39_16, K_FAST39_64):
        tile_kernel("crafted39", k, True)
    for D in SYNTH_DIMS:
        for k in (K_GENERIC, K_FAST_16, K_FAST_64):
            tile_kernel("synth%d_150" % D, k, k != K_GENERIC)
            for G in SYNTH_G[:-1]:                                    # the other state counts: one and two tiles of rows, a lane pair
                tile_kernel("synth%d_%d" % (D, G), k, False, only=("a%d" % (TILE_ROWS[k] + 1),))
    # the hybrid kernel: a (no tiles: the sizes of a 128-row kernel), c (scattered holes, row 0 among them: skip_unused is ignored) -
    # and c once more with max_blocks = 1, which launch_gmm does not apply to this kernel (the grid stays one thread per cell)
    for n in (1, 127, 128, 129, 257):
        cases.append(Case("jd_hybrid_kernel-a%d" % n, "hybrid", K_HYBRID, _random_map(rng, n)))
    src = _random_map(rng, 296)
    src[[0, 3, 17, 73, 127, 258]] = -1
    src[192:256] = -1
    for skip in (0, 1):
        cases.append(Case("jd_hybrid_kernel-c_skip%d" % skip, "hybrid", K_HYBRID, src.copy(), skip, 0, -1, None, "holes"))
    cases.append(Case("jd_hybrid_kernel-c_max_blocks_ignored", "hybrid", K_HYBRID, src.copy(), 1, 1, -1, None, "holes"))
    assert len({c.id for c in cases}) == len(cases)
    return cases


CASES = _build_cases()
CASE_IDS = [c.id for c in CASES]


def f64_deviation(key):
    """largest |oracle - float64| / max(1, |float64|) over the oracle's finite cells of a random model's table, and their number"""
    from indep_viterbi_np import gmm_loglik
    m = model(key)
    assert m.kind == "synth"
    o = m.oracle_table().astype(np.float64)
    fin = np.isfinite(o)
    with np.errstate(invalid="ignore"):
        ref = gmm_loglik(m.am, m.frames)
    return float((np.abs(o[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max()), int(fin.sum())


__all__ = ["CASES", "CASE_IDS", "Case", "check_buffer", "model", "same_floats"]
