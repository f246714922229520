"""The graph and model preparation of jd_dec_create (juicer_amd/csrc/jd_prep.h) on the CPU: tests/prep_driver.cpp, compiled with plain g++,
runs it over the cases of tests/prep_cases.py and is held to tests/golden/prep_golden.json - what the lines of jd_dec_create that jd_prep.h
replaced made of the same inputs, recorded from the commit named in the file - scalar by scalar and array by array (SHA-256 of the raw bytes);
and, independent of the recording, every array is checked in Python for what the kernels rely on - the SOLE_FLAG invariant among it.
"""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import prep_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "juicer_amd", "csrc")
TEE_FLAG, SOLE_FLAG = 0x40000000, 0x20000000
ARRAYS = ["state_new", "row_ptr", "arcs", "xst", "fin_w", "tmax0", "se32", "aux", "lrt", "pcount"]
LZ_BITS = pc.fbits(pc.LZ)


@pytest.fixture(scope="module")
def prep(built, tmp_path_factory):
    """(constants the driver was built with, nets, ams, [(case, scalars and digests, arrays)], the recording)"""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    driver = str(tmp_path_factory.mktemp("prep") / "prep_driver")
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           "-o", driver, os.path.join(HERE, "prep_driver.cpp")])
    nets, ams, cases = pc.build()
    lines = subprocess.run([driver, "arrays"], input=pc.driver_input(nets, ams, cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[0].startswith("consts ") and len(lines) == 1 + len(cases) * (1 + len(ARRAYS))
    consts = {k: int(v) for k, v in (kv.split("=") for kv in lines[0].split()[1:])}
    runs = []
    for i, c in enumerate(cases):
        blk = lines[1 + i * (1 + len(ARRAYS)):][:1 + len(ARRAYS)]
        out = {k: (v if k.startswith("sha256_") else int(v)) for k, v in (kv.split("=") for kv in blk[0].split())}
        arrays = {}
        for name, l in zip(ARRAYS, blk[1:]):
            head, n, rest = (l + " ").split(" ", 2)
            assert head == name
            arrays[name] = np.array(rest.split(), dtype=np.uint32)
            assert arrays[name].shape[0] == int(n)
        runs.append((c, out, arrays))
    with open(os.path.join(HERE, "golden", "prep_golden.json")) as f:
        doc = json.load(f)
    return consts, nets, ams, runs, doc


def test_prep_matches_recorded(prep):
    _, nets, ams, runs, doc = prep
    assert re.fullmatch(r"[0-9a-f]{7,40}", doc["commit"])
    assert len(runs) >= 40
    # the recording is of THESE inputs: a change of the generators is not a change of the preparation
    assert doc["inputs"]["nets"] == {k: pc.digest_inputs(n, pc.NET_FIELDS) for k, n in nets.items()}, "inputs changed: the networks are not the recorded ones"
    assert doc["inputs"]["ams"] == {k: pc.digest_inputs(a, pc.AM_FIELDS) for k, a in ams.items()}, "inputs changed: the model sets are not the recorded ones"
    assert [c["in"] for c in doc["cases"]] == [c for c, _, _ in runs], "the cases are not the recorded ones"
    bad = []
    for (c, out, _), rec in zip(runs, doc["cases"]):
        if out != rec["out"]:
            bad.append(c["name"])
            print(c["name"], {k: (rec["out"].get(k), out.get(k)) for k in set(out) | set(rec["out"]) if out.get(k) != rec["out"].get(k)})
    assert not bad


def f32(words):
    return np.asarray(words, np.uint32).view(np.float32)


def check_case(consts, net, am, c, out, arr):
    """what the kernels rely on, from the driver's full arrays"""
    name, knobs = c["name"], c["knobs"]
    ns, n_arcs = net["n_states"], len(net["to"])
    xsort, sole_on = knobs["xsort"] != 0, knobs["sole"] != 0
    # ---- the numbering: a permutation (or none); the initial state, the final weights and the Path counts move with it
    sn = arr["state_new"].astype(np.int64)
    assert out["renumbered"] == (sn.size > 0), name
    if sn.size:
        assert sorted(sn.tolist()) == list(range(ns)), name
        assert not np.array_equal(sn, np.arange(ns)), name
    else:
        sn = np.arange(ns)
    assert out["init_state"] == sn[net["init"]], name
    fw = np.zeros(ns, np.uint32)
    fw[sn] = pc.bits(net["fin_w"])
    assert np.array_equal(fw, arr["fin_w"]), name
    old_of = np.argsort(sn)
    rp_in = net["row_ptr"].astype(np.int64)
    rp = arr["row_ptr"].astype(np.int64)
    assert rp.size == ns + 1 and rp[0] == 0 and rp[-1] == n_arcs, name
    assert np.array_equal(np.diff(rp), np.diff(rp_in)[old_of]), name
    # ---- the device arcs: every state keeps its arcs, `to` mapped; flags; order
    A = arr["arcs"].reshape(-1, 4).astype(np.int64)
    assert A.shape[0] == n_arcs, name
    d_to, d_w, d_in, d_out = A[:, 0], A[:, 1], A[:, 2], A[:, 3]
    inl = d_in & ~(TEE_FLAG | SOLE_FLAG)
    tee_of = f32(pc.bits(am["hmm_tee"])) > pc.LZ
    is_tee = np.where(inl > 0, tee_of[np.maximum(inl, 1) - 1], False)
    assert np.array_equal((d_in & TEE_FLAG) != 0, is_tee), name
    # tmax0: the largest log probability out of the entry state
    trP = am["trP"].reshape(am["n_tm"], am["max_n"], am["max_n"])
    tmax0 = np.asarray([max([pc.LZ] + [trP[am["hmm_tm"][h], 0, j] for j in range(am["hmm_n"][h])]) for h in range(am["n_hmm"])], np.float32)
    assert np.array_equal(pc.bits(tmax0), arr["tmax0"]), name
    in_w = np.asarray(net["w"], np.float32)
    in_key = in_w + np.where(net["ilab"] > 0, tmax0[np.maximum(net["ilab"], 1) - 1], np.float32(0.0)).astype(np.float32)   # (float32 + float32, as the header adds them)
    in_tee = np.where(net["ilab"] > 0, tee_of[np.maximum(net["ilab"], 1) - 1], False)
    X = arr["xst"].reshape(-1, 16)
    assert X.shape[0] == ns, name
    x_rows, x_wmax = X.tolist(), f32(X[:, 2].copy()).tolist()
    in_rows = list(zip(sn[net["to"]].tolist(), pc.bits(in_w).tolist(), net["ilab"].tolist(), net["olab"].tolist()))
    dev_rows = list(zip(d_to.tolist(), d_w.tolist(), inl.tolist(), d_out.tolist()))
    keys, tees = pc.bits(in_key).tolist(), in_tee.tolist()
    keyf, wf = in_key.tolist(), in_w.tolist()
    n_sorted = n_model_all = 0
    for n in range(ns):
        q = int(old_of[n])
        a0, a1 = int(rp_in[q]), int(rp_in[q + 1])
        src = list(range(a0, a1))
        sort_row = xsort and a1 - a0 <= consts["XSORT_MAX_ROW"]
        entry = [b for b in src if sort_row and in_rows[b][2] != 0 and not tees[b]]
        in_entry = set(entry)
        always = [b for b in src if b not in in_entry]
        # (a stable sort by descending key: Python's sort is stable, and -key orders the floats as the header's comparison does)
        want = always + sorted(entry, key=lambda b: -keyf[b])
        got = dev_rows[int(rp[n]):int(rp[n + 1])]
        assert sorted(got) == sorted(in_rows[a0:a1]), (name, n, "the state's arcs are not its arcs")
        assert got == [in_rows[b] for b in want], (name, n, "arc order")
        ek = [keyf[b] for b in want[len(always):]]
        assert all(x >= y for x, y in zip(ek, ek[1:])), (name, n)
        if not sort_row:
            assert got == in_rows[a0:a1], (name, n, "a row that is not sorted keeps the file's order")
        model = [b for b in src if in_rows[b][2] != 0]
        xr = x_rows[n]
        assert xr[0] == len(always) and xr[1] == len(entry) and xr[3] == len(model), (name, n)
        assert x_wmax[n] == max([float(pc.LZ)] + [wf[b] for b in model]), (name, n, "wmax")
        for i in range(consts["XNCAND"]):
            p = pc.XCAND[i]
            assert xr[4 + i] == (keys[want[len(always) + p]] if p < len(entry) else LZ_BITS), (name, n, i, "k[]")
        n_sorted += len(entry)
        n_model_all += len(model)
    assert (out["n_sorted"], out["n_model_all"], out["n_model"]) == (n_sorted, n_model_all, n_model_all), name
    # ---- THE SOLE INVARIANT (jd_prep.h: prep_arcs): flagged if and only if the arc enters a model, the model is no tee model and the
    # destination has in-degree 1 over all arcs of the decoder's table
    indeg = np.bincount(d_to, minlength=ns)
    want_sole = (inl != 0) & ~is_tee & (indeg[d_to] == 1) & sole_on
    assert np.array_equal((d_in & SOLE_FLAG) != 0, want_sole), name
    assert out["n_sole"] == int(want_sole.sum()), name
    # ---- the cut, and the layout of the per-state words (jd_search.h: DecConst::srec_stride ..)
    want_xcut = int(xsort and n_model_all > 0 and 20 * n_sorted >= 19 * n_model_all) if knobs["xcut"] < 0 else int(knobs["xcut"] != 0 and xsort)
    assert out["xcut"] == want_xcut, name
    n_next = sum(1 for n in range(ns) for b in range(int(rp[n]), int(rp[n + 1])) if d_to[b] == n + 1)
    assert out["n_next"] == n_next, name
    split = (2 if n_arcs > 0 and 4 * n_next >= n_arcs else 0) if knobs["srec_split"] < 0 else knobs["srec_split"]
    assert out["split"] == split, name
    table = {0: (32, 16, 32, 8), 1: (16, 16 * ns, 16, 8), 2: (16, 16 * ns, 8, 8 * ns)}
    assert (out["srec_stride"], out["srec_arr"], out["srec_estride"], out["srec_par"]) == table[split], name
    # ---- models
    assert out["AI"] == (4 if am["max_n"] <= 5 else 8), name
    assert arr["aux"].size == am["n_hmm"] * out["AI"] and arr["se32"].size == am["n_tm"] * am["max_n"], name
    assert np.array_equal(arr["aux"].reshape(-1, out["AI"])[:, 0], (am["hmm_n"] | (am["hmm_tm"] << 8)).astype(np.uint32)), name
    assert out["all_lr"] == (arr["lrt"].size > 0), name
    if out["all_lr"]:
        assert knobs["no_lr"] != 1 and arr["lrt"].size == am["n_tm"] * (8 if am["max_n"] <= 5 else 16) <= consts["TRP_LDS_MAX"], name


def test_prep_invariants(prep):
    consts, nets, ams, runs, _ = prep
    for c, out, arr in runs:
        check_case(consts, nets[c["net"]], ams[c["am"]], c, out, arr)
    # the renumbered breadth-first lexicon IS the chain-numbered one: the numbering the decoder makes is the layout of a lexicon written chain after chain
    by = {c["name"]: (out, arr) for c, out, arr in runs}
    for k in ("row_ptr", "arcs", "xst", "fin_w"):
        assert np.array_equal(by["lex_bfs"][1][k], by["lex_chain"][1][k]), k


def test_prep_constants_are_the_builds(prep):
    """the constants the golden was recorded with are those the kernels are compiled with"""
    consts, _, _, _, doc = prep

    def define(header, name):
        with open(os.path.join(CSRC, header)) as f:
            m = re.search(r"^#define %s (\d+)\b" % name, f.read(), re.M)
        assert m, (header, name)
        return int(m.group(1))

    assert doc["consts"] == consts == {"XSORT_MAX_ROW": define("jd_prep.h", "XSORT_MAX_ROW"), "XNCAND": define("jd_prep.h", "XNCAND"),
                                       "TRP_LDS_MAX": define("jd_prep.h", "TRP_LDS_MAX"), "JD_MAXN": define("jd_internal.h", "JD_MAXN")}
    assert consts["XSORT_MAX_ROW"] == 57
    with open(os.path.join(CSRC, "jd_prep.h")) as f:
        m = re.search(r"constexpr int xcand\(int i\)\s*\{\s*return ([^;]*);", f.read())
    assert [int(x) for x in re.findall(r"\? (\d+) :", m.group(1))] + [int(m.group(1).rsplit(":", 1)[1])] == list(pc.XCAND)


def test_prep_cases_cover_what_they_must(prep):
    consts, nets, ams, runs, _ = prep
    seen = set()
    lrw = {5: 8, 6: 16}
    for c, out, arr in runs:
        net, am, knobs = nets[c["net"]], ams[c["am"]], c["knobs"]
        n_arcs = len(net["to"])
        if c["net"] in ("toy", "small", "small_tree", "mixed"):
            seen.add("%s %s" % (c["net"], " ".join("%s=%d" % (k, knobs[k]) for k in pc.KNOBS if knobs[k] >= 0) or "default"))
        # numbering
        seen.add("numbering kept: the rule says no" if not out["renumber_tried"] and knobs["renumber"] < 0 else "")
        seen.add("numbering kept: the knob says no" if not out["renumber_tried"] and knobs["renumber"] == 0 else "")
        seen.add("numbering kept: equals the network's" if out["renumber_tried"] and out["renumber_same"] else "")
        seen.add("renumbered by the rule" if out["renumbered"] and knobs["renumber"] < 0 else "")
        if c["net"] == "unreachable" and out["renumbered"]:
            sn = arr["state_new"]
            assert sn[net["init"]] == 0 and set(sn[[0, 1, 5]].tolist()) == {4, 5, 6}      # (what the initial state does not reach comes last)
            seen.add("states unreachable from init")
        seen.add("self-loops" if c["net"] == "selfloops" and out["renumber_tried"] else "")
        seen.add("label-less cycle" if not out["acyclic"] else "")
        if knobs["renumber"] < 0:
            seen.add("renumber threshold met" if 4 * out["n_next_net"] == n_arcs - 1 else "renumber threshold missed by one arc" if 4 * out["n_next_net"] == n_arcs else "")
        if knobs["srec_split"] < 0:
            seen.add("split threshold met" if 4 * out["n_next"] == n_arcs else "split threshold missed by one arc" if 4 * out["n_next"] == n_arcs - 1 else "")
            seen.add("split %d by the rule" % out["split"])
        if knobs["xcut"] < 0 and knobs["xsort"] != 0:
            d = 20 * out["n_sorted"] - 19 * out["n_model_all"]
            seen.add("xcut threshold met" if d == 0 else "xcut threshold missed by one arc" if -19 <= d < 0 and 20 * out["n_sorted"] >= 19 * (out["n_model_all"] - 1) else "")
            assert d != 0 or out["xcut"] == 1
        # arc order
        rows = np.diff(net["row_ptr"])
        seen.update("row of %d arcs" % r for r in (57, 58) if (rows == r).any() and knobs["xsort"] != 0)
        X = arr["xst"].reshape(-1, 16).astype(np.int64)
        for p in pc.XCAND:
            if p < consts["XSORT_MAX_ROW"]:
                seen.add("n_entry %d" % p if (X[:, 1] == p).any() else "")
                seen.add("n_entry %d" % (p + 1) if (X[:, 1] == p + 1).any() else "")
        seen.add("epsilon and tee arcs inside a sorted row" if ((X[:, 0] >= 2) & (X[:, 1] >= 2)).any() and c["net"] == "xcand_rows" else "")
        if c["net"] == "xcand_rows" and knobs["xsort"] != 0:
            ties = [n for n in range(net["n_states"]) if X[n, 1] >= 2 and len(set(X[n, 4:4 + 5].tolist())) == 1]
            if ties:
                A = arr["arcs"].reshape(-1, 4)
                r0 = int(arr["row_ptr"][ties[0]])
                assert A[r0:r0 + 9, 3].tolist() == list(range(1, 10))     # equal keys: the file's order
                seen.add("equal keys keep the file's order")
        # SOLE
        if c["net"] == "sole" and knobs["sole"] != 0:
            A = arr["arcs"].reshape(-1, 4).astype(np.int64)
            sn = arr["state_new"].astype(np.int64) if arr["state_new"].size else np.arange(net["n_states"])
            flagged = {(int(np.argsort(sn)[a[0]]), int(a[2] & ~(TEE_FLAG | SOLE_FLAG))) for a in A if a[2] & SOLE_FLAG}
            assert (1, 1) in flagged and not any(to in (2, 3, 4, 5, 6) for to, _ in flagged)
            seen.add("sole: in-degree 1 by a model arc, a tee arc, an epsilon arc; in-degree 2 from one state")
        seen.add("sole off" if knobs["sole"] == 0 and out["n_sole"] == 0 and out["n_model"] > 0 else "")
        # models
        seen.add("AI %d" % out["AI"])
        seen.add("a transition matrix with n < 3" if (am["tm_n"] < 3).any() and not out["all_lr"] else "")
        seen.add("a skip transition" if c["am"] == "skip5" and not out["all_lr"] else "")
        seen.add("hmm_n differs from tm_n" if (am["hmm_n"] != am["tm_n"][am["hmm_tm"]]).any() and not out["all_lr"] else "")
        seen.add("left-to-right" if out["all_lr"] else "left-to-right, forced off" if knobs["no_lr"] == 1 else "")
        w = lrw.get(am["max_n"])
        if w and knobs["no_lr"] != 1:
            if am["n_tm"] * w == consts["TRP_LDS_MAX"]:
                assert out["all_lr"]
                seen.add("n_tm at TRP_LDS_MAX / %d" % w)
            if (am["n_tm"] - 1) * w == consts["TRP_LDS_MAX"]:
                assert not out["all_lr"]
                seen.add("n_tm one above TRP_LDS_MAX / %d" % w)
        # histogram
        seen.add("hist off" if c["max_hyps"] == 0 and out["hist_nbins"] == 0 else "")
        if c["max_hyps"] > 0:
            seen.add("main_beam 0" if c["main_beam"] == 0 else "main_beam below 0" if c["main_beam"] < 0 else "")
            assert c["main_beam"] > 0 or (out["hist_min"], out["hist_max"], out["hist_nbins"]) == (-1001, 201, 1203)
            seen.add("hist_nbins %d" % out["hist_nbins"] if 2047 <= out["hist_nbins"] <= 2049 else "")
    synth_knobs = ["default", "sole=0", "renumber=1 sole=0", "xsort=0", "xcut=0", "xcut=1", "xsort=0 xcut=1", "no_lr=1"] + \
                  ["renumber=%d srec_split=%d" % (r, s) for r in (0, 1) for s in (0, 1, 2)]
    want = ["%s %s" % (n, k) for n in ("toy", "small", "small_tree", "mixed") for k in synth_knobs] + [
        "numbering kept: the rule says no", "numbering kept: the knob says no", "numbering kept: equals the network's", "renumbered by the rule",
        "states unreachable from init", "self-loops", "label-less cycle",
        "renumber threshold met", "renumber threshold missed by one arc", "split threshold met", "split threshold missed by one arc",
        "split 0 by the rule", "split 2 by the rule", "xcut threshold met", "xcut threshold missed by one arc",
        "row of 57 arcs", "row of 58 arcs", "epsilon and tee arcs inside a sorted row", "equal keys keep the file's order",
        "sole: in-degree 1 by a model arc, a tee arc, an epsilon arc; in-degree 2 from one state", "sole off",
        "AI 4", "AI 8", "a transition matrix with n < 3", "a skip transition", "hmm_n differs from tm_n", "left-to-right", "left-to-right, forced off",
        "n_tm at TRP_LDS_MAX / 8", "n_tm one above TRP_LDS_MAX / 8", "n_tm at TRP_LDS_MAX / 16", "n_tm one above TRP_LDS_MAX / 16",
        "hist off", "main_beam 0", "main_beam below 0", "hist_nbins 2047", "hist_nbins 2048", "hist_nbins 2049"] + \
        ["n_entry %d" % n for p in pc.XCAND if p < 57 for n in (p, p + 1)]
    assert [w for w in want if w not in seen] == []
    ins = [json.dumps(dict(c, name=""), sort_keys=True) for c, _, _ in runs]
    assert len(ins) == len(set(ins)) and len({c["name"] for c, _, _ in runs}) == len(runs)      # no case twice
