"""ctypes binding of the C ABI in include/juicer_amd.h (libjuicer_amd.so).

The library is the product; this module only marshals numpy arrays and raw
device pointers into it.  There is no CPU fallback anywhere: if the shared
library is missing or no HIP device is usable, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libjuicer_amd.so")

JD_OK, JD_EINVAL, JD_ENODEV, JD_EHIP, JD_ENOMEM, JD_EHIST, JD_ESTATE, JD_EFORMAT = 0, -1, -2, -3, -4, -5, -6, -7
# bits of the `pushing` argument of jd_net_compose / jd_net_create_lazy / jd_multi_create_lazy
JD_PUSH_WEIGHTS, JD_PUSH_LABELS, JD_LOOKAHEAD_SETS = 1, 2, 4
LOG_ZERO = float(np.float32(-3.402823466e+38))


class JuicerAmdError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("juicer_amd error %d: %s" % (code, msg))
        self.code = code


class Stats(C.Structure):
    _fields_ = [("n_frames", C.c_int32),
                ("tot_active_emit_hyps", C.c_int64), ("tot_active_end_hyps", C.c_int64),
                ("tot_active_models", C.c_int64), ("tot_proc_emit_hyps", C.c_int64),
                ("tot_proc_end_hyps", C.c_int64), ("tot_arcs_visited", C.c_int64),
                ("tot_paths", C.c_int64), ("tot_insts_in", C.c_int64), ("ties", C.c_int64),
                # what the kernels really touched (include/juicer_amd.h: jd_stats)
                ("tot_recs_read", C.c_int64), ("tot_new_attached", C.c_int64), ("tot_recs_written", C.c_int64), ("tot_entry_items", C.c_int64),
                ("tot_items_expanded", C.c_int64), ("tot_arcs_walked", C.c_int64), ("tot_closure_items", C.c_int64), ("tot_bids_placed", C.c_int64)]


class CHyp(C.Structure):
    _fields_ = [("n", C.c_int32),
                ("label", C.POINTER(C.c_int32)), ("time", C.POINTER(C.c_int32)),
                ("score", C.POINTER(C.c_float)), ("ac", C.POINTER(C.c_float)), ("lm", C.POINTER(C.c_float)),
                ("tot_score", C.c_float), ("tot_ac", C.c_float), ("tot_lm", C.c_float),
                ("stats", Stats)]


class Timing(C.Structure):
    _fields_ = [("gmm_ms", C.c_double), ("search_ms", C.c_double), ("total_ms", C.c_double),
                ("gmm_wait_ms", C.c_double),
                ("gmm_launches", C.c_int32), ("search_launches", C.c_int32),
                ("relaunches", C.c_int32), ("cluster_wgs", C.c_int32),
                ("gmm_frames", C.c_int64), ("gmm_states", C.c_int64), ("search_frames", C.c_int64),
                ("prefetched", C.c_int32), ("ahead_frames", C.c_int32), ("slot_launches", C.c_int32), ("trace_launches", C.c_int32)]


FLOW_SERIAL, FLOW_TWO_IN_FLIGHT, FLOW_RESIDENT = 0, 1, 3      # jd_dec_set_pipeline
SCORE_EXACT, SCORE_FAST = 0, 1                                # jd_dec_set_scoring
OUTPUT_WORDS, OUTPUT_MODELS = 1, 2                            # jd_dec_set_output_level


class CModelHyp(C.Structure):
    _fields_ = [("n", C.c_int32),
                ("model", C.POINTER(C.c_int32)), ("label", C.POINTER(C.c_int32)), ("time", C.POINTER(C.c_int32)),
                ("score", C.POINTER(C.c_float)), ("ac", C.POINTER(C.c_float)), ("lm", C.POINTER(C.c_float)),
                ("tot_score", C.c_float), ("tot_ac", C.c_float), ("tot_lm", C.c_float)]


class CBest(C.Structure):
    """jd_best: the head of a stream's current best hypothesis (jd_streams_best)."""
    _fields_ = [("found", C.c_int32), ("frame", C.c_int32), ("n_words", C.c_int32), ("n_records", C.c_int32),
                ("model", C.c_int32), ("state", C.c_int32),
                ("score", C.c_float), ("ac", C.c_float), ("lm", C.c_float)]


class CFinal(C.Structure):
    """jd_final: the head of a stream's end-of-utterance view (jd_streams_final)."""
    _fields_ = [("found", C.c_int32), ("frame", C.c_int32), ("n_words", C.c_int32), ("n_records", C.c_int32),
                ("score", C.c_float), ("ac", C.c_float), ("lm", C.c_float)]


class PipeStats(C.Structure):
    _fields_ = [("mode", C.c_int32), ("depth", C.c_int32), ("slots", C.c_int32), ("resident", C.c_int32),
                ("batches_announced", C.c_int32), ("pad0", C.c_int32),
                ("frames_searched", C.c_int64), ("utts_through", C.c_int64), ("rows_scored", C.c_int64),
                ("batches_back", C.c_int64), ("collections", C.c_int64),
                ("slot_busy_us", C.c_double), ("on_us", C.c_double)]


@dataclass
class Hyp:
    """1-best in DecHyp chain order (index 0 = newest word)."""
    n: int
    label: np.ndarray
    time: np.ndarray
    score: np.ndarray
    ac: np.ndarray
    lm: np.ndarray
    tot_score: float
    tot_ac: float
    tot_lm: float
    stats: dict
    models: Optional["ModelHyp"] = None      # model-level output (Decoder.set_output_level(OUTPUT_WORDS | OUTPUT_MODELS))


@dataclass
class ModelHyp:
    """Model-level result (jd_model_hyp), newest first: model = HMM index + 1 (0: a word label on an epsilon-input arc),
    label = word id + 1 of the same arc (0: none), time = the frame the token left the model; a segment starts at the
    next entry's time (frame 0 for the oldest)."""
    n: int
    model: np.ndarray
    label: np.ndarray
    time: np.ndarray
    score: np.ndarray
    ac: np.ndarray
    lm: np.ndarray
    tot_score: float
    tot_ac: float
    tot_lm: float


# every symbol include/juicer_amd.h declares
EXPORTS = [
    "jd_net_create_arcs", "jd_net_create_csr", "jd_net_load_fsm", "jd_net_num_arcs", "jd_net_num_states",
    "jd_net_init_state", "jd_net_destroy", "jd_net_get_csr", "jd_net_load_jwnt", "jd_net_save_jwnt",
    "jd_am_load_jmbi", "jd_am_save_jmbi", "jd_am_create_htk", "jd_am_create_flat", "jd_am_num_hmms", "jd_am_num_gmms",
    "jd_am_vec_size", "jd_am_max_states", "jd_am_max_mix", "jd_am_num_transmats", "jd_am_get_topology", "jd_am_load_mmf", "jd_am_get_flat", "jd_am_get_trans", "jd_am_destroy",
    "jd_dec_create", "jd_dec_destroy", "jd_dec_set_capacity", "jd_stream_init", "jd_stream_push",
    "jd_stream_finish", "jd_decode_batch", "jd_decode_batch_device", "jd_dec_last_timing",
    "jd_am_score_frames", "jd_last_error", "jd_version", "jd_dec_debug_trace", "jd_debug_expf",
    "jd_multi_create", "jd_multi_create_lazy", "jd_multi_decode_batch", "jd_multi_destroy",
    "jd_dec_set_partial_interval", "jd_stream_partial", "jd_stream_collect_info", "jd_stream_path_counts", "jd_dec_quiesce", "jd_debug_closure_path_counts", "jd_dec_set_max_alloc_models", "jd_net_compose", "jd_am_create_hybrid", "jd_net_create_lazy", "jd_net_lazy_size", "jd_net_lazy_reset",
    "jd_net_lazy_set_high_water", "jd_net_lazy_generation", "jd_release_cached_memory", "jd_net_push_labels", "jd_debug_cl_label_sets",
    "jd_debug_cl_lookahead", "jd_dec_prefetch_scores", "jd_streams_push", "jd_dec_info",
    "jd_broker_create", "jd_broker_destroy", "jd_broker_open", "jd_broker_close", "jd_broker_init", "jd_broker_push",
    "jd_broker_finish", "jd_broker_get_stats", "jd_dec_debug_cells", "jd_dec_set_pipeline", "jd_dec_pipeline_stats",
    "jd_dec_set_scoring", "jd_am_score_frames_mode", "jd_debug_log1pe", "jd_debug_log_add",
    "jd_debug_hist_bin", "jd_debug_hist_threshold",
    "jd_dec_set_output_level", "jd_dec_get_output_level", "jd_dec_model_result",
    "jd_am_hmm_name", "jd_stream_partial_models",
    "jd_streams_trace", "jd_dec_get_partial_interval", "jd_broker_partial", "jd_debug_score_rows",
    "jd_debug_paths",
    "jd_streams_best", "jd_stream_best_words", "jd_stream_best_models", "jd_dec_best_stats",
    "jd_streams_final", "jd_stream_final_words", "jd_stream_final_models", "jd_dec_final_stats", "jd_streams_trace_models",
    "jd_am_create_mlp", "jd_am_mlp_info", "jd_am_save_mlp", "jd_am_load_mlp", "jd_am_mlp_forward", "jd_am_mlp_forward_host",
    "jd_debug_mlp_activations", "jd_debug_mlp_time",
    "jd_am_create_hybrid_tied", "jd_am_create_mlp_tied", "jd_am_load_mlp_tied",
    "jd_am_mlp_to_bf16", "jd_am_mlp_precision",
    "jd_am_mlp_splice", "jd_am_mlp_context", "jd_debug_score_rows_span", "jd_stream_held_frames",
]

_lib = None


def lib():
    """Load libjuicer_amd.so; fail loudly when the HIP extension is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise JuicerAmdError(JD_ENODEV, "HIP extension %s is not built (run python -m juicer_amd.build); "
                                 "there is no CPU fallback" % LIB_PATH)
        try:                      # share torch's HIP runtime when torch is in the process
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        L.jd_last_error.restype = C.c_char_p
        L.jd_version.restype = C.c_char_p
        L.jd_net_num_arcs.restype = C.c_int64
        _lib = L
    return _lib


def _check(rc: int):
    if rc != 0:
        raise JuicerAmdError(rc, lib().jd_last_error().decode())


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _hyp_from_c(h: CHyp) -> Hyp:
    k = max(int(h.n), 0)

    def arr(ptr, dt):
        if k == 0:
            return np.zeros(0, dtype=dt)
        # (string_at + frombuffer: a tenth of what np.ctypeslib.as_array costs per array - 64 hypotheses x 5 arrays per step)
        return np.frombuffer(C.string_at(ptr, 4 * k), dtype=dt).copy()
    hs = h.stats                                                   # (one ctypes sub-object, not one per field)
    st = {f: int(getattr(hs, f)) for f, _ in Stats._fields_}
    return Hyp(n=int(h.n), label=arr(h.label, np.int32), time=arr(h.time, np.int32),
               score=arr(h.score, np.float32), ac=arr(h.ac, np.float32), lm=arr(h.lm, np.float32),
               tot_score=float(h.tot_score), tot_ac=float(h.tot_ac), tot_lm=float(h.tot_lm), stats=st)


def _model_hyp_from_c(h: CModelHyp) -> ModelHyp:
    k = max(int(h.n), 0)

    def arr(ptr, dt):
        return np.frombuffer(C.string_at(ptr, 4 * k), dtype=dt).copy() if k else np.zeros(0, dtype=dt)
    return ModelHyp(n=int(h.n), model=arr(h.model, np.int32), label=arr(h.label, np.int32), time=arr(h.time, np.int32),
                    score=arr(h.score, np.float32), ac=arr(h.ac, np.float32), lm=arr(h.lm, np.float32),
                    tot_score=float(h.tot_score), tot_ac=float(h.tot_ac), tot_lm=float(h.tot_lm))


def _pushing_mask(pushing, push_labels, lookahead_sets) -> int:
    return (JD_PUSH_WEIGHTS if pushing else 0) | (JD_PUSH_LABELS if push_labels else 0) | (JD_LOOKAHEAD_SETS if lookahead_sets else 0)


class Network:
    """WFSTNetwork counterpart: CSR arc table (16-byte arc records) for HBM."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def from_arcs(cls, src, dst, ilab, olab, w_file, fstate, fweight_file, lm_scale=1.0, ins_penalty=0.0):
        L = lib()
        h = C.c_void_p()
        src, dst, il, ol = _i32(src), _i32(dst), _i32(ilab), _i32(olab)
        wf, fs, fw = _f32(w_file), _i32(fstate), _f32(fweight_file)
        _check(L.jd_net_create_arcs(C.byref(h), C.c_int64(src.shape[0]), _p(src, C.c_int32), _p(dst, C.c_int32),
                                    _p(il, C.c_int32), _p(ol, C.c_int32), _p(wf, C.c_float),
                                    C.c_int32(fs.shape[0]), _p(fs, C.c_int32), _p(fw, C.c_float),
                                    C.c_float(lm_scale), C.c_float(ins_penalty)))
        return cls(h)

    @classmethod
    def from_synth(cls, net, lm_scale=1.0, ins_penalty=0.0):
        return cls.from_arcs(net.src, net.dst, net.ilab, net.olab, net.w_file, net.fstate, net.fweight_file,
                             lm_scale, ins_penalty)

    @classmethod
    def from_csr(cls, n_states, init_state, row_ptr, to, w, ilab, olab, fstate, fweight):
        L = lib()
        h = C.c_void_p()
        rp, to_, il, ol = _i32(row_ptr), _i32(to), _i32(ilab), _i32(olab)
        w_, fs, fw = _f32(w), _i32(fstate), _f32(fweight)
        _check(L.jd_net_create_csr(C.byref(h), C.c_int32(n_states), C.c_int32(init_state), _p(rp, C.c_int32),
                                   _p(to_, C.c_int32), _p(w_, C.c_float), _p(il, C.c_int32), _p(ol, C.c_int32),
                                   C.c_int32(fs.shape[0]), _p(fs, C.c_int32), _p(fw, C.c_float)))
        return cls(h)

    @classmethod
    def from_fsm_file(cls, fsm_path, insyms_path=None, outsyms_path=None, lm_scale=1.0, ins_penalty=0.0):
        L = lib()
        h = C.c_void_p()
        enc = lambda s: None if s is None else os.fsencode(s)
        _check(L.jd_net_load_fsm(C.byref(h), enc(fsm_path), enc(insyms_path), enc(outsyms_path),
                                 C.c_float(lm_scale), C.c_float(ins_penalty)))
        return cls(h)

    @classmethod
    def from_jwnt_file(cls, path, lm_scale=1.0, ins_penalty=0.0):
        """Juicer's binary network cache (<fsm>.bin, WFSTNetwork::readBinary)."""
        h = C.c_void_p()
        _check(lib().jd_net_load_jwnt(C.byref(h), os.fsencode(path), C.c_float(lm_scale), C.c_float(ins_penalty)))
        return cls(h)

    @classmethod
    def compose(cls, cl: "Network", g: "Network", device: int = 0, max_states: int = 0, max_arcs: int = 0, pushing: bool = False,
                push_labels: bool = False, lookahead_sets: bool = False):
        """C.L o G on the device (jd_net_compose): the dynamic-composition row's first step."""
        h = C.c_void_p()
        _check(lib().jd_net_compose(C.byref(h), cl.h, g.h, C.c_int32(device), C.c_int64(max_states), C.c_int64(max_arcs),
                                    C.c_int32(_pushing_mask(pushing, push_labels, lookahead_sets))))
        return cls(h)

    @classmethod
    def lazy(cls, cl: "Network", g: "Network", am: "Models", device: int = 0, max_states: int = 0, max_arcs: int = 0, pushing: bool = False,
             push_labels: bool = False, lookahead_sets: bool = False):
        """C.L o G expanded by the search, where it goes (jd_net_create_lazy)."""
        h = C.c_void_p()
        _check(lib().jd_net_create_lazy(C.byref(h), cl.h, g.h, am.h, C.c_int32(device), C.c_int64(max_states), C.c_int64(max_arcs),
                                        C.c_int32(_pushing_mask(pushing, push_labels, lookahead_sets))))
        return cls(h)

    def label_sets(self, cap: int = -1):
        """The label sets of JD_LOOKAHEAD_SETS for every state of this C.L transducer (jd_debug_cl_label_sets, host only):
        (row_ptr int64 [n_states + 1], labels int32 - sorted per state, -1 alone for "every label" -, mayfin bool [n_states]).
        cap: room for the labels (default: as many as there are)."""
        L = lib()
        ns = self.n_states
        rp, mf, n = np.zeros(ns + 1, np.int64), np.zeros(ns, np.uint8), C.c_int64(0)
        if cap < 0:
            dummy = np.zeros(1, np.int32)
            rc = L.jd_debug_cl_label_sets(self.h, _p(rp, C.c_int64), _p(dummy, C.c_int32), C.c_int64(0), C.byref(n), _p(mf, C.c_uint8))
            if rc != 0 and not (rc == JD_ENOMEM and n.value > 0):
                _check(rc)
            cap = n.value
        labels = np.zeros(max(cap, 1), np.int32)
        _check(L.jd_debug_cl_label_sets(self.h, _p(rp, C.c_int64), _p(labels, C.c_int32), C.c_int64(cap), C.byref(n), _p(mf, C.c_uint8)))
        return rp, labels[:n.value], mf.astype(bool)

    def lookahead(self):
        """The look-ahead intervals of every state of this C.L transducer (jd_debug_cl_lookahead, host only):
        (lo int32 [n_states], hi int32 [n_states], mayfin bool [n_states]); lo > hi: no label is reachable."""
        ns = self.n_states
        lo, hi, mf = np.zeros(ns, np.int32), np.zeros(ns, np.int32), np.zeros(ns, np.uint8)
        _check(lib().jd_debug_cl_lookahead(self.h, _p(lo, C.c_int32), _p(hi, C.c_int32), _p(mf, C.c_uint8)))
        return lo, hi, mf.astype(bool)

    def push_labels(self):
        """C.L with its output labels pushed towards the initial state (jd_net_push_labels): (network, labels moved)."""
        h, n = C.c_void_p(), C.c_int64(0)
        _check(lib().jd_net_push_labels(C.byref(h), self.h, C.byref(n)))
        return type(self)(h), n.value

    def lazy_reset(self):
        _check(lib().jd_net_lazy_reset(self.h))

    def lazy_set_high_water(self, fraction: float):
        """The fill beyond which the arena starts a new generation between utterances (jd_net_lazy_set_high_water)."""
        _check(lib().jd_net_lazy_set_high_water(self.h, C.c_double(fraction)))

    def lazy_generation(self) -> int:
        g = C.c_int64(0)
        _check(lib().jd_net_lazy_generation(self.h, C.byref(g)))
        return g.value

    def lazy_size(self):
        ns, na = C.c_int64(0), C.c_int64(0)
        _check(lib().jd_net_lazy_size(self.h, C.byref(ns), C.byref(na)))
        return ns.value, na.value

    def save_jwnt(self, path):
        """WFSTNetwork::writeBinary counterpart (-writeBinaryFiles)."""
        _check(lib().jd_net_save_jwnt(self.h, os.fsencode(path)))

    def csr(self):
        ns, na = self.n_states, self.n_arcs
        rp = np.zeros(ns + 1, np.int32); to = np.zeros(na, np.int32); w = np.zeros(na, np.float32)
        il = np.zeros(na, np.int32); ol = np.zeros(na, np.int32); fw = np.zeros(ns, np.float32)
        _check(lib().jd_net_get_csr(self.h, _p(rp, C.c_int32), _p(to, C.c_int32), _p(w, C.c_float),
                                    _p(il, C.c_int32), _p(ol, C.c_int32), _p(fw, C.c_float)))
        return dict(row_ptr=rp, to=to, w=w, ilab=il, olab=ol, fin_w=fw)

    def closure_path_counts(self, models):
        """(per-state Path counts of the reference's propagateToken closure, acyclic) - jd_debug_closure_path_counts (host only)."""
        out = np.zeros(self.n_states, np.int32)
        ok = C.c_int32(0)
        _check(lib().jd_debug_closure_path_counts(self.h, models.h, _p(out, C.c_int32), C.byref(ok)))
        return out, bool(ok.value)

    @property
    def n_arcs(self):
        return int(lib().jd_net_num_arcs(self.h))

    @property
    def n_states(self):
        return int(lib().jd_net_num_states(self.h))

    @property
    def init_state(self):
        return int(lib().jd_net_init_state(self.h))

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.jd_net_destroy(self.h)
            self.h = None


class Models:
    """HTKFlatModels counterpart (IModels, Models.h:29-67)."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def from_htk(cls, am):
        L = lib()
        h = C.c_void_p()
        nm, wt, mu, var = _i32(am.n_mix), _f32(am.weight), _f32(am.mean), _f32(am.var)
        hn, hg, ht = _i32(am.hmm_nstates), _i32(am.hmm_gmm), _i32(am.hmm_tm)
        tn, tp = _i32(am.tm_nstates), _f32(am.transp)
        _check(L.jd_am_create_htk(C.byref(h), C.c_int32(am.D), C.c_int32(am.n_gmm), C.c_int32(am.max_mix),
                                  _p(nm, C.c_int32), _p(wt, C.c_float), _p(mu, C.c_float), _p(var, C.c_float),
                                  C.c_int32(am.n_hmm), C.c_int32(am.max_n), _p(hn, C.c_int32), _p(hg, C.c_int32),
                                  _p(ht, C.c_int32), C.c_int32(am.n_tm), _p(tn, C.c_int32), _p(tp, C.c_float)))
        return cls(h)

    @classmethod
    def from_flat(cls, det, mean, ivar, n_mix):
        """Models from the prepared arrays as they are (jd_am_create_flat): det [G, M], mean / ivar [G, M, D] (inverse
        variances), n_mix [G]; one 3-state HMM on tied state 0 as the topology.  Scoring a frame equal to a component's mean
        gives its det exactly."""
        det, mean, ivar, nm = _f32(det), _f32(mean), _f32(ivar), _i32(n_mix)
        G, M, D = mean.shape
        assert det.shape == (G, M) and ivar.shape == mean.shape and nm.shape == (G,)
        hn, hg, ht, tn = _i32([3]), _i32([-1, 0, -1]), _i32([0]), _i32([3])
        tee = _f32([LOG_ZERO])
        trP = np.full((1, 3, 3), LOG_ZERO, np.float32)
        trP[0, 0, 1] = 0.0
        trP[0, 1, 1] = trP[0, 1, 2] = np.log(np.float32(0.5))
        se = np.array([[[0, 0], [0, 2], [1, 2]]], np.int16)
        h = C.c_void_p()
        _check(lib().jd_am_create_flat(C.byref(h), C.c_int32(D), C.c_int32(G), C.c_int32(M), _p(nm, C.c_int32), _p(det, C.c_float),
                                       _p(mean, C.c_float), _p(ivar, C.c_float), C.c_int32(1), C.c_int32(3), _p(hn, C.c_int32),
                                       _p(hg, C.c_int32), _p(ht, C.c_int32), _p(tee, C.c_float), C.c_int32(1), _p(tn, C.c_int32),
                                       _p(trP, C.c_float), _p(se, C.c_int16)))
        return cls(h)

    @classmethod
    def from_mmf_file(cls, path):
        L = lib()
        h = C.c_void_p()
        _check(L.jd_am_load_mmf(C.byref(h), os.fsencode(path)))
        return cls(h)

    @classmethod
    def from_jmbi_file(cls, path):
        """Juicer's binary model cache (<mmf>.bin, HTKModels::readBinary)."""
        h = C.c_void_p()
        _check(lib().jd_am_load_jmbi(C.byref(h), os.fsencode(path)))
        return cls(h)

    def save_jmbi(self, path):
        """HTKModels::output(path, true) counterpart (-writeBinaryFiles)."""
        _check(lib().jd_am_save_jmbi(self.h, os.fsencode(path)))

    @property
    def n_hmms(self):
        return int(lib().jd_am_num_hmms(self.h))

    def hmm_names(self) -> Optional[List[str]]:
        """The HMMs' names in index order (jd_am_hmm_name; HMM i = in-label i + 1), or None: models built from arrays."""
        out = []
        for i in range(self.n_hmms):
            nm = C.c_char_p()
            _check(lib().jd_am_hmm_name(self.h, C.c_int32(i), C.byref(nm)))
            if nm.value is None:
                return None
            out.append(nm.value.decode())
        return out

    @property
    def n_gmms(self):
        return int(lib().jd_am_num_gmms(self.h))

    @property
    def vec_size(self):
        return int(lib().jd_am_vec_size(self.h))

    @property
    def max_states(self):
        return int(lib().jd_am_max_states(self.h))

    @property
    def max_mix(self):
        return int(lib().jd_am_max_mix(self.h))

    @property
    def n_tm(self):
        return int(lib().jd_am_num_transmats(self.h))

    def topology(self):
        H, MN, G = self.n_hmms, self.max_states, self.n_gmms
        hn = np.zeros(H, np.int32); hg = np.zeros((H, MN), np.int32); ht = np.zeros(H, np.int32)
        nm = np.zeros(G, np.int32)
        _check(lib().jd_am_get_topology(self.h, _p(hn, C.c_int32), _p(hg, C.c_int32), _p(ht, C.c_int32),
                                        _p(nm, C.c_int32)))
        return hn, hg, ht, nm

    def flat(self):
        G, M, D = self.n_gmms, self.max_mix, self.vec_size
        det = np.zeros((G, M), np.float32)
        mean = np.zeros((G, M, D), np.float32)
        ivar = np.zeros((G, M, D), np.float32)
        _check(lib().jd_am_get_flat(self.h, _p(det, C.c_float), _p(mean, C.c_float), _p(ivar, C.c_float)))
        return det, mean, ivar

    def trans(self):
        MN = self.max_states
        trP = np.zeros((self.n_tm, MN, MN), np.float32)
        se = np.zeros((self.n_tm, MN, 2), np.int16)
        tee = np.zeros(self.n_hmms, np.float32)
        _check(lib().jd_am_get_trans(self.h, _p(trP, C.c_float), _p(se, C.c_int16), _p(tee, C.c_float)))
        return trP, se, tee

    @classmethod
    def from_hybrid(cls, priors, states_per_model: int = 5):
        """Hybrid ANN / HMM models (HTKModels::Load(phones, priors, statesPerModel)): features are log posteriors."""
        pr = _f32(priors)
        h = C.c_void_p()
        _check(lib().jd_am_create_hybrid(C.byref(h), C.c_int32(pr.shape[0]), _p(pr, C.c_float), C.c_int32(states_per_model)))
        return cls(h)

    @classmethod
    def from_mlp(cls, priors, states_per_model, layers):
        """Neural acoustic models (jd_am_create_mlp): jd_am_create_hybrid's models with the network that yields the log posteriors.
        layers: [(weight [out, in], bias [out], act)], act one of ACT_LINEAR / ACT_RELU / ACT_SIGMOID for a hidden layer (the last
        layer's outputs are the logits; its act is ignored and may be left out).  Feature vectors hold in = layers[0] weight's columns."""
        pr = _f32(priors)
        ws = [np.ascontiguousarray(_f32(l[0])) for l in layers]
        bs = [np.ascontiguousarray(_f32(l[1])) for l in layers]
        n = len(layers)
        assert n >= 1 and all(w.ndim == 2 and b.shape == (w.shape[0],) for w, b in zip(ws, bs))
        assert all(ws[i].shape[1] == ws[i - 1].shape[0] for i in range(1, n))
        width = _i32([w.shape[0] for w in ws])
        act = _i32([int(l[2]) for l in layers[:-1]] + [ACT_LINEAR])
        wp = (C.POINTER(C.c_float) * n)(*[_p(w, C.c_float) for w in ws])
        bp = (C.POINTER(C.c_float) * n)(*[_p(b, C.c_float) for b in bs])
        h = C.c_void_p()
        _check(lib().jd_am_create_mlp(C.byref(h), C.c_int32(pr.shape[0]), _p(pr, C.c_float), C.c_int32(states_per_model),
                                      C.c_int32(ws[0].shape[1]), C.c_int32(n), _p(width, C.c_int32), _p(act, C.c_int32), wp, bp))
        return cls(h)

    @classmethod
    def from_hybrid_tied(cls, topology: "Models", priors):
        """Tied hybrid models (jd_am_create_hybrid_tied): the HMMs, state tying, transitions and names of `topology` - any GMM
        models - with one log posterior per TIED STATE as the feature vector; priors: one per tied state (topology.n_gmms)."""
        pr = _f32(priors)
        assert pr.shape == (topology.n_gmms,)
        h = C.c_void_p()
        _check(lib().jd_am_create_hybrid_tied(C.byref(h), topology.h, _p(pr, C.c_float)))
        return cls(h)

    @classmethod
    def from_mlp_tied(cls, topology: "Models", priors, layers):
        """Tied neural models (jd_am_create_mlp_tied): from_hybrid_tied's models with the network that yields the tied states' log
        posteriors; layers as from_mlp's, the last of topology.n_gmms outputs (up to 16384)."""
        pr = _f32(priors)
        assert pr.shape == (topology.n_gmms,)
        ws = [np.ascontiguousarray(_f32(l[0])) for l in layers]
        bs = [np.ascontiguousarray(_f32(l[1])) for l in layers]
        n = len(layers)
        assert n >= 1 and all(w.ndim == 2 and b.shape == (w.shape[0],) for w, b in zip(ws, bs))
        assert all(ws[i].shape[1] == ws[i - 1].shape[0] for i in range(1, n))
        width = _i32([w.shape[0] for w in ws])
        act = _i32([int(l[2]) for l in layers[:-1]] + [ACT_LINEAR])
        wp = (C.POINTER(C.c_float) * n)(*[_p(w, C.c_float) for w in ws])
        bp = (C.POINTER(C.c_float) * n)(*[_p(b, C.c_float) for b in bs])
        h = C.c_void_p()
        _check(lib().jd_am_create_mlp_tied(C.byref(h), topology.h, _p(pr, C.c_float), C.c_int32(ws[0].shape[1]), C.c_int32(n),
                                           _p(width, C.c_int32), _p(act, C.c_int32), wp, bp))
        return cls(h)

    @classmethod
    def load_mlp_tied(cls, topology: "Models", path):
        """Tied neural models from a JMLP version 2 file (jd_am_load_mlp_tied) beside the HMM set it was trained for."""
        h = C.c_void_p()
        _check(lib().jd_am_load_mlp_tied(C.byref(h), topology.h, os.fsencode(path)))
        return cls(h)

    @classmethod
    def load_mlp(cls, path):
        """Neural acoustic models from a JMLP file (jd_am_load_mlp)."""
        h = C.c_void_p()
        _check(lib().jd_am_load_mlp(C.byref(h), os.fsencode(path)))
        return cls(h)

    def save_mlp(self, path):
        _check(lib().jd_am_save_mlp(self.h, os.fsencode(path)))

    def to_bf16(self) -> "Models":
        """New models of the same kind whose network weights are these models' rounded to bf16 (jd_am_mlp_to_bf16): every entry
        point serves them, on the bf16 kernels, with no mode set."""
        h = C.c_void_p()
        _check(lib().jd_am_mlp_to_bf16(self.h, C.byref(h)))
        return type(self)(h)

    def splice(self, left: int, right: int) -> "Models":
        """New models with the same network, topology, priors and precision whose feature vectors are single frames of
        in_dim / (left + right + 1) values: the window of left + 1 + right frames is gathered on the device (jd_am_mlp_splice)."""
        h = C.c_void_p()
        _check(lib().jd_am_mlp_splice(self.h, C.c_int32(left), C.c_int32(right), C.byref(h)))
        return type(self)(h)

    @property
    def mlp_context(self):
        """(left, right) of spliced models, (0, 0) of an unspliced network (jd_am_mlp_context)."""
        left, right = C.c_int32(0), C.c_int32(0)
        _check(lib().jd_am_mlp_context(self.h, C.byref(left), C.byref(right)))
        return left.value, right.value

    @property
    def mlp_precision(self) -> int:
        """MLP_F32, MLP_BF16, or -1 for models without a network (jd_am_mlp_precision)."""
        return int(lib().jd_am_mlp_precision(self.h))

    def mlp_info(self):
        """(in_dim, [width], [act]) of the network (jd_am_mlp_info)."""
        d, n = C.c_int32(0), C.c_int32(0)
        width, act = np.zeros(16, np.int32), np.zeros(16, np.int32)
        _check(lib().jd_am_mlp_info(self.h, C.byref(d), C.byref(n), _p(width, C.c_int32), _p(act, C.c_int32)))
        return d.value, [int(v) for v in width[:n.value]], [int(v) for v in act[:n.value]]

    def mlp_forward(self, frames, device: int = 0):
        """The network's log posteriors [T, n_phones] for feature vectors [T, in_dim], from the device (jd_am_mlp_forward)."""
        x = _f32(frames)
        assert x.ndim == 2 and (x.shape[0] == 0 or x.shape[1] == self.vec_size)
        out = np.zeros((x.shape[0], self.n_gmms), np.float32)
        _check(lib().jd_am_mlp_forward(self.h, C.c_int32(device), _p(x, C.c_float), C.c_int32(x.shape[0]), _p(out, C.c_float)))
        return out

    def mlp_forward_host(self, frames):
        """... and from the host twin, which defines them (jd_am_mlp_forward_host; needs no device)."""
        x = _f32(frames)
        assert x.ndim == 2 and (x.shape[0] == 0 or x.shape[1] == self.vec_size)
        out = np.zeros((x.shape[0], self.n_gmms), np.float32)
        _check(lib().jd_am_mlp_forward_host(self.h, _p(x, C.c_float), C.c_int32(x.shape[0]), _p(out, C.c_float)))
        return out

    def mlp_activations(self, frames, layer: int, on_device: bool = True, device: int = 0):
        """The activations [T, width[layer]] behind a layer, the raw logits for the last (jd_debug_mlp_activations): the kernel's or
        the host twin's."""
        x = _f32(frames)
        assert x.ndim == 2 and (x.shape[0] == 0 or x.shape[1] == self.vec_size)
        width = self.mlp_info()[1]
        if not 0 <= layer < len(width):
            raise JuicerAmdError(JD_EINVAL, "mlp_activations: layer %d outside [0, %d)" % (layer, len(width)))
        out = np.zeros((x.shape[0], width[layer]), np.float32)
        _check(lib().jd_debug_mlp_activations(self.h, C.c_int32(device), C.c_int32(1 if on_device else 0), _p(x, C.c_float),
                                              C.c_int32(x.shape[0]), C.c_int32(layer), _p(out, C.c_float)))
        return out

    def mlp_time(self, frames, warmup: int = 5, iters: int = 20, max_blocks: int = 0, device: int = 0):
        """ms of `iters` scoring launches of these models on the rows of frames, after `warmup` unmeasured ones (jd_debug_mlp_time)."""
        x = _f32(frames)
        assert x.ndim == 2 and x.shape[0] >= 1 and x.shape[1] == self.vec_size
        ms = np.zeros(iters, np.float32)
        _check(lib().jd_debug_mlp_time(self.h, C.c_int32(device), _p(x, C.c_float), C.c_int32(x.shape[0]), C.c_int32(max_blocks),
                                       C.c_int32(warmup), C.c_int32(iters), _p(ms, C.c_float)))
        return ms

    def score_frames(self, frames, device: int = 0, mode: int = 0):
        """Companion GMM kernel on its own: [T, D] -> [T, n_gmm] log-likelihoods (mode: SCORE_EXACT, the default, or SCORE_FAST)."""
        x = _f32(frames)
        out = np.zeros((x.shape[0], self.n_gmms), np.float32)
        _check(lib().jd_am_score_frames_mode(self.h, C.c_int32(device), C.c_int32(mode), _p(x, C.c_float), C.c_int32(x.shape[0]),
                                             _p(out, C.c_float)))
        return out

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.jd_am_destroy(self.h)
            self.h = None


# a hidden layer's activation (jd_am_create_mlp)
ACT_LINEAR, ACT_RELU, ACT_SIGMOID = 0, 1, 2

# jd_debug_log_add's variants: the generic kernel's logAdd, jd_gmm_kernel39's pairwise step, jd_gmm_fast39's (device only)
LOGADD_GENERIC, LOGADD_PAIR, LOGADD_FAST = 0, 1, 2
# jd_debug_log1pe's: the replica of the libm's log(1 + e), the table value
LOG1PE_LIBM, LOG1PE_TABLE = 0, 1


def debug_log_add(x, y, variant: int, device: int = -1):
    """logAdd(x[i], y[i]) as the kernels compute it (device -1: the host twin compiled from the same source)."""
    x, y = _f32(x), _f32(y)
    assert x.shape == y.shape and x.ndim == 1
    out = np.empty_like(x)
    _check(lib().jd_debug_log_add(C.c_int32(device), C.c_int32(variant), _p(x, C.c_float), _p(y, C.c_float),
                                  C.c_int64(x.shape[0]), _p(out, C.c_float)))
    return out


def debug_log1pe(d, variant: int, device: int = -1):
    """log(1.0 + (double)expf(d[i])) in double, d[i] in [-19, 0], as the kernels compute it."""
    d = _f32(d)
    assert d.ndim == 1
    out = np.empty(d.shape[0], np.float64)
    _check(lib().jd_debug_log1pe(C.c_int32(device), C.c_int32(variant), _p(d, C.c_float), C.c_int64(d.shape[0]),
                                 _p(out, C.c_double)))
    return out


# jd_debug_score_rows: the kernel launch_gmm chose (jd_score_kernel)
(KERNEL_NONE, KERNEL_GMM_GENERIC, KERNEL_GMM39_16, KERNEL_GMM39_64, KERNEL_GMM_FAST39_16, KERNEL_GMM_FAST39_64, KERNEL_GMM_FAST_16,
 KERNEL_GMM_FAST_64, KERNEL_HYBRID) = range(9)
KERNEL_MLP = 9                     # jd_mlp_kernel (Models.from_mlp); beside KERNEL_NAMES, the list of the kernels of tests/score_rows_cases.py
KERNEL_MLP_TIED = 10               # jd_mlp_tied_kernel (Models.from_mlp_tied)
KERNEL_MLP_BF16 = 11               # jd_mlp_bf16_kernel (Models.to_bf16 of from_mlp's models)
KERNEL_MLP_TIED_BF16 = 12          # jd_mlp_tied_bf16_kernel (... of from_mlp_tied's)
KERNEL_MLP_SPLICED, KERNEL_MLP_TIED_SPLICED, KERNEL_MLP_BF16_SPLICED, KERNEL_MLP_TIED_BF16_SPLICED = 13, 14, 15, 16   # Models.splice of the four
MLP_F32, MLP_BF16 = 0, 1           # Models.mlp_precision
KERNEL_NAMES = ["none", "jd_gmm_kernel<0>", "jd_gmm_kernel39<16>", "jd_gmm_kernel39<64>", "jd_gmm_fast39<16>", "jd_gmm_fast39<64>",
                "jd_gmm_fast<16>", "jd_gmm_fast<64>", "jd_hybrid_kernel"]


def debug_score_rows(models: "Models", frames, row_src, out, mode: int = SCORE_EXACT, skip_unused: int = 0, max_blocks: int = 0,
                     used_row_tiles: int = -1, rt_base=None, guard_rows: int = 0, device: int = 0, row_lo=None, row_hi=None):
    """One launch of the scoring kernels with the decoder's own launch arguments (jd_debug_score_rows): out is the caller's
    PREFILLED [(guard_rows + n_rows + guard_rows), n_gmm] buffer.  Returns (the buffer as the launch left it - a copy -, the
    kernel that ran (KERNEL_*), its grid).  row_lo / row_hi: the rows' spans, for spliced models (jd_debug_score_rows_span)."""
    x, src = _f32(frames), _i32(row_src)
    buf = np.array(out, dtype=np.float32, order="C", copy=True)
    n_rows = src.shape[0]
    assert x.ndim == 2 and src.ndim == 1 and buf.shape == (n_rows + 2 * guard_rows, models.n_gmms)
    assert x.shape[0] == 0 or x.shape[1] == models.vec_size
    lst = None if rt_base is None else _i32(rt_base)
    k, g = C.c_int32(0), C.c_int32(0)
    if row_lo is not None or row_hi is not None:
        lo, hi = _i32(row_lo), _i32(row_hi)
        assert lo.shape == src.shape and hi.shape == src.shape
        _check(lib().jd_debug_score_rows_span(models.h, C.c_int32(device), C.c_int32(mode), _p(x, C.c_float), C.c_int32(x.shape[0]),
                                              _p(src, C.c_int32), _p(lo, C.c_int32), _p(hi, C.c_int32), C.c_int32(n_rows),
                                              C.c_int32(skip_unused), C.c_int32(max_blocks), C.c_int32(used_row_tiles),
                                              None if lst is None else _p(lst, C.c_int32), C.c_int32(0 if lst is None else lst.shape[0]),
                                              C.c_int32(guard_rows), _p(buf, C.c_float), C.byref(k), C.byref(g)))
        return buf, k.value, g.value
    _check(lib().jd_debug_score_rows(models.h, C.c_int32(device), C.c_int32(mode), _p(x, C.c_float), C.c_int32(x.shape[0]),
                                     _p(src, C.c_int32), C.c_int32(n_rows), C.c_int32(skip_unused), C.c_int32(max_blocks),
                                     C.c_int32(used_row_tiles), None if lst is None else _p(lst, C.c_int32),
                                     C.c_int32(0 if lst is None else lst.shape[0]), C.c_int32(guard_rows), _p(buf, C.c_float),
                                     C.byref(k), C.byref(g)))
    return buf, k.value, g.value


# jd_debug_hist_bin's sentinel below hist_min (above hist_max it gives JD_EHIST)
HIST_BELOW = -1


def debug_hist_bin(s, hist_min: int, hist_max: int, device: int = -1):
    """The search kernels' Histogram::addScore bin of s[i]: the bin index, HIST_BELOW or JD_EHIST (device -1: the host twin)."""
    s = _f32(s)
    assert s.ndim == 1
    out = np.empty(s.shape[0], np.int32)
    _check(lib().jd_debug_hist_bin(C.c_int32(device), _p(s, C.c_float), C.c_int64(s.shape[0]), C.c_int32(hist_min),
                                   C.c_int32(hist_max), _p(out, C.c_int32)))
    return out


def debug_hist_threshold(bins, max_hyps, hist_min: int, device: int = 0):
    """The search kernels' Histogram::calcThresh (one wave per case): bins is n_cases x nb, max_hyps n_cases (device only)."""
    bins, max_hyps = _i32(bins), _i32(max_hyps)
    assert bins.ndim == 2 and max_hyps.shape == (bins.shape[0],)
    out = np.empty(bins.shape[0], np.float32)
    _check(lib().jd_debug_hist_threshold(C.c_int32(device), _p(bins, C.c_int32), C.c_int64(bins.shape[0]),
                                         C.c_int32(bins.shape[1]), _p(max_hyps, C.c_int32), C.c_int32(hist_min),
                                         _p(out, C.c_float)))
    return out


def debug_paths(desc, device: int = 0):
    """The Path collection and the partial trace (csrc/jd_gc.h) on a described state: desc is the int32 word list of
    csrc/jd_paths.h, and the words that come back are those it lists (device only; a description that fails the validation
    raises JD_EINVAL before any device call)."""
    desc = _i32(desc)
    assert desc.ndim == 1
    n = C.c_int64(0)
    rc = lib().jd_debug_paths(C.c_int32(device), _p(desc, C.c_int32), C.c_int64(desc.shape[0]), None, C.c_int64(0), C.byref(n))
    if rc != JD_ENOMEM:
        _check(rc if rc != 0 else JD_ESTATE)
    out = np.empty(max(n.value, 1), np.int32)
    _check(lib().jd_debug_paths(C.c_int32(device), _p(desc, C.c_int32), C.c_int64(desc.shape[0]), _p(out, C.c_int32),
                                C.c_int64(n.value), C.byref(n)))
    return out[:n.value]


class Decoder:
    """WFSTDecoderLite counterpart over the C ABI (one jd_dec)."""

    def __init__(self, net: Network, models: Models, start_beam=0.0, main_beam=0.0, end_beam=0.0,
                 word_beam=0.0, max_hyps=0, block_size=5, device=0, max_streams=1,
                 max_slots=0, max_paths=0, max_items=0):
        L = lib()
        self.net, self.models = net, models       # keep alive: the decoder does not own them
        self.max_streams = int(max_streams)
        self.h = C.c_void_p()
        _check(L.jd_dec_create(C.byref(self.h), net.h, models.h, C.c_float(start_beam), C.c_float(main_beam),
                               C.c_float(end_beam), C.c_float(word_beam), C.c_int32(max_hyps),
                               C.c_int32(block_size), C.c_int32(device), C.c_int32(max_streams)))
        if max_slots or max_paths or max_items:
            _check(L.jd_dec_set_capacity(self.h, C.c_int64(max_slots), C.c_int64(max_paths), C.c_int64(max_items)))

    # -- IDecoder protocol on one stream
    def stream_init(self, s: int = 0):
        _check(lib().jd_stream_init(self.h, C.c_int32(s)))

    def stream_push(self, s: int, frames):
        x = _f32(frames)
        _check(lib().jd_stream_push(self.h, C.c_int32(s), _p(x, C.c_float), C.c_int32(x.shape[0])))

    def stream_held_frames(self, s: int = 0) -> int:
        """Frames pushed to stream s and not yet searched: a stream of spliced models (Models.splice) holds the last `right`
        frames back; 0 for every other kind of model (jd_stream_held_frames)."""
        n = C.c_int32(0)
        _check(lib().jd_stream_held_frames(self.h, C.c_int32(s), C.byref(n)))
        return n.value

    def stream_finish(self, s: int = 0) -> Hyp:
        h = CHyp()
        _check(lib().jd_stream_finish(self.h, C.c_int32(s), C.byref(h)))
        return self._with_models(_hyp_from_c(h), s, self.output_level() & OUTPUT_MODELS)

    # -- model-level output (jd_dec_set_output_level)
    def set_output_level(self, level: int):
        """OUTPUT_WORDS (default) or OUTPUT_WORDS | OUTPUT_MODELS: every result then has .models (a ModelHyp) beside the
        words, which stay what word output gives.  Between decodes."""
        _check(lib().jd_dec_set_output_level(self.h, C.c_int32(level)))

    def output_level(self) -> int:
        v = C.c_int32(0)
        _check(lib().jd_dec_get_output_level(self.h, C.byref(v)))
        return v.value

    def model_result(self, i: int) -> ModelHyp:
        """Result i of the last stream_finish (i = the stream) or decode_batch / decode_batch_device (i = the utterance)."""
        h = CModelHyp()
        _check(lib().jd_dec_model_result(self.h, C.c_int32(i), C.byref(h)))
        return _model_hyp_from_c(h)

    def _with_models(self, hyp: Hyp, i: int, models: int) -> Hyp:
        if models:
            hyp.models = self.model_result(i)
        return hyp

    def streams_push(self, streams, frames):
        """jd_stream_push for several streams at once: one scoring launch + one search launch (jd_streams_push)."""
        xs = [_f32(f) for f in frames]
        n = len(xs)
        ss = _i32(list(streams))
        ptrs = (C.POINTER(C.c_float) * n)(*[_p(x, C.c_float) for x in xs])
        nfr = _i32([x.shape[0] for x in xs])
        _check(lib().jd_streams_push(self.h, C.c_int32(n), _p(ss, C.c_int32), ptrs, _p(nfr, C.c_int32)))

    def set_max_alloc_models(self, v: int):
        """WFSTDecoderLite::setMaxAllocModels (:807-820): percentage / MB / count, see juicer_amd.h."""
        _check(lib().jd_dec_set_max_alloc_models(self.h, C.c_int32(v)))

    # -- PARTIAL_DECODING (WFSTDecoderLite.cpp:822-896)
    def set_partial_interval(self, interval: int):
        _check(lib().jd_dec_set_partial_interval(self.h, C.c_int32(interval)))

    def get_partial_interval(self) -> int:
        v = C.c_int32(0)
        _check(lib().jd_dec_get_partial_interval(self.h, C.byref(v)))
        return v.value

    def streams_trace(self, streams):
        """tracePartialPath now on each of the listed streams (each once), each at the frame it has reached: one launch and one
        fetch for all of them (jd_streams_trace).  Returns found per stream; the lists are read with stream_partial(s)."""
        ss = _i32(list(streams))
        found = np.zeros(max(1, ss.shape[0]), np.int32)
        _check(lib().jd_streams_trace(self.h, C.c_int32(ss.shape[0]), _p(ss, C.c_int32), _p(found, C.c_int32)))
        return [bool(f) for f in found[:ss.shape[0]]]

    def stream_collect_info(self, s: int = 0):
        """(collectPaths runs of the stream's utterance so far, lastPathCollectFrame) - counted while PARTIAL_DECODING is on."""
        n, last = C.c_int32(0), C.c_int32(-1)
        _check(lib().jd_stream_collect_info(self.h, C.c_int32(s), C.byref(n), C.byref(last)))
        return n.value, last.value

    def quiesce(self):
        """The decoder's resident kernel (FLOW_RESIDENT) leaves the device - call before a device-wide synchronisation (jd_dec_quiesce)."""
        _check(lib().jd_dec_quiesce(self.h))

    def set_pipeline(self, mode: int, depth: int = 0, slots: int = 0):
        """How batches that follow each other share the chip (jd_dec_set_pipeline): FLOW_SERIAL, FLOW_TWO_IN_FLIGHT (default) or
        FLOW_RESIDENT (depth = batches announced and not handed back at most, slots = one-workgroup slots of the resident kernel)."""
        _check(lib().jd_dec_set_pipeline(self.h, C.c_int32(mode), C.c_int32(depth), C.c_int32(slots)))

    def set_scoring(self, mode: int):
        """How the likelihood tables are scored (jd_dec_set_scoring): SCORE_EXACT (default: the reference's roundings, bit-identical
        log-likelihoods) or SCORE_FAST (fused multiply-add distance, fp32 logAdd: scores within 1e-4, the table at 0.4 of the cost at D = 39; GMM models of
        every vector size)."""
        _check(lib().jd_dec_set_scoring(self.h, C.c_int32(mode)))

    def pipeline_stats(self) -> dict:
        """What FLOW_RESIDENT has done so far, cumulative (jd_dec_pipeline_stats)."""
        t = PipeStats()
        _check(lib().jd_dec_pipeline_stats(self.h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in PipeStats._fields_ if not f.startswith("pad")}

    def stream_path_counts(self, s: int = 0):
        """(nPath, nPathNew, exact): collectPaths' trigger counts; exact = they are the reference's (jd_stream_path_counts)."""
        a, b, e = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check(lib().jd_stream_path_counts(self.h, C.c_int32(s), C.byref(a), C.byref(b), C.byref(e)))
        return a.value, b.value, bool(e.value)

    def stream_partial(self, s: int = 0, trace_now: bool = False):
        """(found, partialPaths as [(label, frame)], oldest first); trace_now runs tracePartialPath first."""
        n, found = C.c_int32(0), C.c_int32(0)
        cap, was_found = 256, False
        while True:
            lab, tim = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
            _check(lib().jd_stream_partial(self.h, C.c_int32(s), C.c_int32(1 if trace_now else 0), C.c_int32(cap), C.byref(n),
                                           _p(lab, C.c_int32), _p(tim, C.c_int32), C.byref(found)))
            if trace_now:
                was_found = bool(found.value)
            if n.value <= cap:
                break
            cap, trace_now = n.value, False
        return was_found, [(int(lab[i]), int(tim[i])) for i in range(n.value)]

    def stream_partial_models(self, s: int = 0, trace_now: bool = False):
        """(found, ModelHyp): stream_partial's trace at model level (jd_stream_partial_models) - every record from the root up
        to the record the word list ends at, OLDEST first (unlike Hyp.models); tot_* are 0."""
        n, found = C.c_int32(0), C.c_int32(0)
        cap, was_found = 256, False
        while True:
            mod, lab, tim = (np.zeros(cap, np.int32) for _ in range(3))
            sc, ac, lm = (np.zeros(cap, np.float32) for _ in range(3))
            _check(lib().jd_stream_partial_models(self.h, C.c_int32(s), C.c_int32(1 if trace_now else 0), C.c_int32(cap), C.byref(n),
                                                  _p(mod, C.c_int32), _p(lab, C.c_int32), _p(tim, C.c_int32),
                                                  _p(sc, C.c_float), _p(ac, C.c_float), _p(lm, C.c_float), C.byref(found)))
            if trace_now:
                was_found = bool(found.value)
            if n.value <= cap:
                break
            cap, trace_now = n.value, False
        k = n.value
        return was_found, ModelHyp(n=k, model=mod[:k].copy(), label=lab[:k].copy(), time=tim[:k].copy(), score=sc[:k].copy(),
                                   ac=ac[:k].copy(), lm=lm[:k].copy(), tot_score=0.0, tot_ac=0.0, tot_lm=0.0)

    # -- the current best hypothesis of live streams (jd_streams_best)
    def streams_best(self, streams):
        """The best emitting-state token of each listed stream (each once) at the frame it has reached: one launch and one fetch
        for all of them (jd_streams_best).  Returns a dict per stream with jd_best's fields; the lists are read with
        stream_best_words(s) / stream_best_models(s).  A stream whose chain exceeds the result capacity raises (JD_ENOMEM) after
        the others were served: the error carries what was delivered as .entries."""
        ss = _i32(list(streams))
        n = int(ss.shape[0])
        out = (CBest * max(1, n))()
        rc = lib().jd_streams_best(self.h, C.c_int32(n), _p(ss, C.c_int32), out)
        entries = [{f: getattr(out[i], f) for f, _ in CBest._fields_} for i in range(n)]
        if rc != 0:
            err = JuicerAmdError(rc, lib().jd_last_error().decode())
            err.entries = entries if rc == JD_ENOMEM else None
            raise err
        return entries

    def stream_best_words(self, s: int = 0):
        """The word list of stream s's best hypothesis as of the last streams_best, oldest first: (label, time, score, ac, lm)
        arrays (jd_stream_best_words; at model level the labelled entries of stream_best_models)."""
        n = C.c_int32(0)
        cap = 256
        while True:
            lab, tim = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
            sc, ac, lm = (np.zeros(cap, np.float32) for _ in range(3))
            _check(lib().jd_stream_best_words(self.h, C.c_int32(s), C.c_int32(cap), C.byref(n), _p(lab, C.c_int32), _p(tim, C.c_int32),
                                              _p(sc, C.c_float), _p(ac, C.c_float), _p(lm, C.c_float)))
            if n.value <= cap:
                break
            cap = n.value
        k = n.value
        return lab[:k].copy(), tim[:k].copy(), sc[:k].copy(), ac[:k].copy(), lm[:k].copy()

    def stream_best_models(self, s: int = 0) -> "ModelHyp":
        """Every record of the chain of stream s's best hypothesis as of the last streams_best, OLDEST first, as a ModelHyp
        (jd_stream_best_models, JD_OUTPUT_MODELS only); tot_* are 0."""
        n = C.c_int32(0)
        cap = 256
        while True:
            mod, lab, tim = (np.zeros(cap, np.int32) for _ in range(3))
            sc, ac, lm = (np.zeros(cap, np.float32) for _ in range(3))
            _check(lib().jd_stream_best_models(self.h, C.c_int32(s), C.c_int32(cap), C.byref(n), _p(mod, C.c_int32), _p(lab, C.c_int32),
                                               _p(tim, C.c_int32), _p(sc, C.c_float), _p(ac, C.c_float), _p(lm, C.c_float)))
            if n.value <= cap:
                break
            cap = n.value
        k = n.value
        return ModelHyp(n=k, model=mod[:k].copy(), label=lab[:k].copy(), time=tim[:k].copy(), score=sc[:k].copy(),
                        ac=ac[:k].copy(), lm=lm[:k].copy(), tot_score=0.0, tot_ac=0.0, tot_lm=0.0)

    def best_stats(self):
        """(kernel launches, device-to-host copies) the streams_best calls of this decoder have made (jd_dec_best_stats)."""
        a, b = C.c_int64(0), C.c_int64(0)
        _check(lib().jd_dec_best_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- the end-of-utterance view of live streams (jd_streams_final)
    def streams_final(self, streams):
        """What stream_finish would return now for each listed stream (each once), without finishing: one launch and one fetch
        for all of them (jd_streams_final).  Returns a dict per stream with jd_final's fields; the lists are read with
        stream_final_words(s) / stream_final_models(s).  A stream whose chain exceeds the result capacity raises (JD_ENOMEM)
        after the others were served: the error carries what was delivered as .entries."""
        ss = _i32(list(streams))
        n = int(ss.shape[0])
        out = (CFinal * max(1, n))()
        rc = lib().jd_streams_final(self.h, C.c_int32(n), _p(ss, C.c_int32), out)
        entries = [{f: getattr(out[i], f) for f, _ in CFinal._fields_} for i in range(n)]
        if rc != 0:
            err = JuicerAmdError(rc, lib().jd_last_error().decode())
            err.entries = entries if rc == JD_ENOMEM else None
            raise err
        return entries

    def stream_final_words(self, s: int = 0):
        """The word list of stream s's final hypothesis as of the last streams_final, OLDEST first: (label, time, score, ac, lm)
        arrays (jd_stream_final_words); reversed it is the Hyp of a stream_finish behind the same frames."""
        n = C.c_int32(0)
        cap = 256
        while True:
            lab, tim = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
            sc, ac, lm = (np.zeros(cap, np.float32) for _ in range(3))
            _check(lib().jd_stream_final_words(self.h, C.c_int32(s), C.c_int32(cap), C.byref(n), _p(lab, C.c_int32), _p(tim, C.c_int32),
                                               _p(sc, C.c_float), _p(ac, C.c_float), _p(lm, C.c_float)))
            if n.value <= cap:
                break
            cap = n.value
        k = n.value
        return lab[:k].copy(), tim[:k].copy(), sc[:k].copy(), ac[:k].copy(), lm[:k].copy()

    def stream_final_models(self, s: int = 0) -> "ModelHyp":
        """Every record of the chain of stream s's final hypothesis as of the last streams_final, OLDEST first, as a ModelHyp
        (jd_stream_final_models, JD_OUTPUT_MODELS only); tot_* are 0 (the totals: the entry of streams_final)."""
        n = C.c_int32(0)
        cap = 256
        while True:
            mod, lab, tim = (np.zeros(cap, np.int32) for _ in range(3))
            sc, ac, lm = (np.zeros(cap, np.float32) for _ in range(3))
            _check(lib().jd_stream_final_models(self.h, C.c_int32(s), C.c_int32(cap), C.byref(n), _p(mod, C.c_int32), _p(lab, C.c_int32),
                                                _p(tim, C.c_int32), _p(sc, C.c_float), _p(ac, C.c_float), _p(lm, C.c_float)))
            if n.value <= cap:
                break
            cap = n.value
        k = n.value
        return ModelHyp(n=k, model=mod[:k].copy(), label=lab[:k].copy(), time=tim[:k].copy(), score=sc[:k].copy(),
                        ac=ac[:k].copy(), lm=lm[:k].copy(), tot_score=0.0, tot_ac=0.0, tot_lm=0.0)

    def final_stats(self):
        """(kernel launches, device-to-host copies) the streams_final calls of this decoder have made (jd_dec_final_stats)."""
        a, b = C.c_int64(0), C.c_int64(0)
        _check(lib().jd_dec_final_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def streams_trace_models(self, streams):
        """stream_partial_models(s, trace_now=True) for each of the listed streams (each once) of a model-level decoder: one launch
        and one fetch for all of them (jd_streams_trace_models).  Returns found per stream; the lists are read with
        stream_partial_models(s) and stream_partial(s)."""
        ss = _i32(list(streams))
        found = np.zeros(max(1, ss.shape[0]), np.int32)
        _check(lib().jd_streams_trace_models(self.h, C.c_int32(ss.shape[0]), _p(ss, C.c_int32), _p(found, C.c_int32)))
        return [bool(f) for f in found[:ss.shape[0]]]

    # -- DecoderBatchTest inner loop
    def decode_batch(self, feats: Sequence[np.ndarray]) -> List[Hyp]:
        n = len(feats)
        xs = [_f32(f) for f in feats]
        ptrs = (C.POINTER(C.c_float) * n)(*[_p(x, C.c_float) for x in xs])
        nfr = _i32([x.shape[0] for x in xs])
        hyps = (CHyp * n)()
        rc = lib().jd_decode_batch(self.h, C.c_int32(n), ptrs, _p(nfr, C.c_int32), hyps)
        _check(rc)
        m = self.output_level() & OUTPUT_MODELS
        return [self._with_models(_hyp_from_c(hyps[i]), i, m) for i in range(n)]

    def decode_batch_device(self, d_feats_ptr: int, offs, hip_stream: int = 0, raw: bool = False):
        """Features already in HBM: d_feats_ptr = device address of [total_frames, D] floats."""
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        n = offs.shape[0] - 1
        hyps = (CHyp * n)()
        rc = lib().jd_decode_batch_device(self.h, C.c_int32(n), C.c_void_p(d_feats_ptr), _p(offs, C.c_int64),
                                          C.c_void_p(hip_stream), hyps)
        _check(rc)
        if raw:
            return hyps
        m = self.output_level() & OUTPUT_MODELS
        return [self._with_models(_hyp_from_c(hyps[i]), i, m) for i in range(n)]

    def prefetch_scores(self, d_feats_ptr: int, offs, hip_stream: int = 0):
        """Announce the batch the NEXT decode_batch_device call will decode (same arguments): its likelihood table is
        scored on the CUs the current batch's search leaves idle (jd_dec_prefetch_scores).  The device buffer and the
        offsets must stay as they are until that call."""
        offs = np.ascontiguousarray(offs if offs is not None else [0], dtype=np.int64)
        n = offs.shape[0] - 1                                          # (one entry = no utterance: drops what was scored ahead)
        _check(lib().jd_dec_prefetch_scores(self.h, C.c_int32(n), C.c_void_p(d_feats_ptr), _p(offs, C.c_int64),
                                            C.c_void_p(hip_stream)))

    def last_timing(self) -> dict:
        t = Timing()
        _check(lib().jd_dec_last_timing(self.h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in Timing._fields_}

    def debug_cells(self, enable: bool):
        """Mark (enable) / count (not enable -> (cells read, cells of the last decode's table)) the likelihood cells the search reads."""
        a, b = C.c_int64(0), C.c_int64(0)
        _check(lib().jd_dec_debug_cells(self.h, C.c_int32(1 if enable else 0), C.byref(a), C.byref(b)))
        return a.value, b.value

    def debug_trace(self, enable: int = 0, fetch: bool = False):
        """In-kernel cycle accounting of k_search: enable, or fetch [1024, 16] int64 sums per workgroup
        {lists A, phase A, wg wait, barrier 1, lists X, phase X, wg wait, barriers X, frames} in 100 MHz ticks."""
        buf = np.zeros((1024, 16), np.int64) if fetch else None
        _check(lib().jd_dec_debug_trace(self.h, C.c_int32(enable), None if buf is None else _p(buf, C.c_int64)))
        return buf

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.jd_dec_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class BrokerStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("ticks", "frames", "stream_ticks", "us_idle", "us_coalesce", "us_init", "us_push", "us_finish",
                                         "us_search", "resident")]


class Broker:
    """Many serial IDecoder callers (threads) on the streams of one Decoder (jd_broker_*): each caller opens a client
    and drives it with init / push / finish; a worker thread of the library coalesces what the clients have pushed into
    one scoring launch and one search launch per tick.  ctypes releases the GIL during the calls, so Python threads
    do run side by side.  The Decoder must not be used directly while the broker lives."""

    def __init__(self, dec: Decoder, n_clients: int = 0):
        self.dec = dec
        self.h = C.c_void_p()
        _check(lib().jd_broker_create(C.byref(self.h), dec.h, C.c_int32(n_clients or dec.max_streams)))

    def open(self) -> int:
        c = C.c_int32(-1)
        _check(lib().jd_broker_open(self.h, C.byref(c)))
        return c.value

    def close_client(self, client: int):
        _check(lib().jd_broker_close(self.h, C.c_int32(client)))

    def init(self, client: int):
        _check(lib().jd_broker_init(self.h, C.c_int32(client)))

    def push(self, client: int, frames):
        x = _f32(frames)
        _check(lib().jd_broker_push(self.h, C.c_int32(client), _p(x, C.c_float), C.c_int32(x.shape[0])))

    def finish(self, client: int) -> Hyp:
        h = CHyp()
        _check(lib().jd_broker_finish(self.h, C.c_int32(client), C.byref(h)))
        return _hyp_from_c(h)

    def partial(self, client: int):
        """The client's partialPaths as [(label, frame)], oldest first, as of the worker's last tick; after finish the complete
        list (jd_broker_partial).  The interval is set on the Decoder before the Broker is made."""
        n, cap = C.c_int32(0), 256
        while True:
            lab, tim = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
            _check(lib().jd_broker_partial(self.h, C.c_int32(client), C.c_int32(cap), C.byref(n), _p(lab, C.c_int32), _p(tim, C.c_int32)))
            if n.value <= cap:
                break
            cap = n.value
        return [(int(lab[i]), int(tim[i])) for i in range(n.value)]

    def stats(self) -> dict:
        st = BrokerStats()
        _check(lib().jd_broker_get_stats(self.h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in BrokerStats._fields_}

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.jd_broker_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

