"""Label-set look-ahead (JD_LOOKAHEAD_SETS) on the CPU: the host-side set computation (juicer_amd/csrc/jd_labelsets.h) through
jd_debug_cl_label_sets - from the built library, and compiled on its own with g++ and sanitizers (tests/labelsets_driver.cpp) - against
Python sets grown by a naive fix-point (tests/compose_sets_ref.py).  No device is needed: the call is host code."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from compose_sets_ref import add_variants, label_sets, permute_words, random_perm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED = 5
FIXTURES = ["plain", "sp", "terminal", "permuted", "variants"]


def _pair(kind):
    from juicer_amd import synth
    am = synth.make_models(SEED, n_gmm=100, n_hmm=45, n_mix=2, n_tm=8, sep=0.6, with_tee=True)
    cl, g = synth.make_cl_g(SEED, am, n_words=40, n_succ=4, n_tri=30, with_sp=kind != "plain", terminal=kind == "terminal")
    if kind == "variants":
        cl = add_variants(cl, am, list(range(3, 40, 5)), seed=11)
    if kind == "permuted":
        cl, g = permute_words(cl, g, random_perm(cl, g, 21))
    return am, cl, g


@pytest.fixture(scope="module")
def lib_built():
    from juicer_amd import build as jbuild
    jbuild.build()
    return True


def _got_sets(ncl, **kw):
    rp, labels, mf = ncl.label_sets(**kw)
    return [labels[rp[c]:rp[c + 1]].tolist() for c in range(ncl.n_states)], mf.tolist()


def _want_sets(csr):
    sets, mf = label_sets(csr)
    return [[-1] if s is None else sorted(s) for s in sets], mf


@pytest.mark.parametrize("kind", FIXTURES)
def test_label_sets_match_python_sets(lib_built, kind):
    from juicer_amd import capi
    am, cl, g = _pair(kind)
    ncl = capi.Network.from_synth(cl, 1.0, 0.0)
    got, got_mf = _got_sets(ncl)
    want, want_mf = _want_sets(ncl.csr())
    assert got == want
    assert got_mf == want_mf
    assert any(len(s) > 1 for s in want)
    if kind == "terminal":
        assert any(want_mf) and not all(want_mf)
    if kind in ("plain", "sp", "terminal"):
        # the generator numbers the words in the tree's depth-first order: every set is exactly its interval
        assert all(s == list(range(s[0], s[-1] + 1)) for s in want if s)
    else:
        # ... and a renumbering, or a second pronunciation elsewhere in the tree, breaks that
        assert any(s != list(range(s[0], s[-1] + 1)) for s in want if s)


def _cycle_net():
    """0 -eps-> 1 -eps-> 2 -eps-> 1 (a label-less cycle), 2 -:7-> 3, 0 -:4-> 4 -eps-> 5 -:9-> 3, 5 -:2-> 3; 3 final, 6 -eps-> 3"""
    src = [0, 0, 1, 2, 2, 4, 5, 5, 6]
    dst = [1, 4, 2, 1, 3, 5, 3, 3, 3]
    ol = [0, 4, 0, 0, 7, 0, 9, 2, 0]
    il = [1] * len(src)
    return dict(src=src, dst=dst, il=il, ol=ol, n_states=7, final=[3])


def test_label_less_cycle_means_every_label(lib_built):
    from juicer_amd import capi
    n = _cycle_net()
    ncl = capi.Network.from_arcs(n["src"], n["dst"], n["il"], n["ol"], np.zeros(len(n["src"]), np.float32), n["final"], [0.0])
    got, mf = _got_sets(ncl)
    assert got == [[-1], [-1], [-1], [], [2, 9], [2, 9], []]            # the cycle (1, 2) and its ancestor 0: every label
    assert mf == [False, False, False, True, False, False, True]
    want, want_mf = _want_sets(ncl.csr())
    assert got == want and mf == want_mf


def test_list_bound_and_cap_are_errors(lib_built, monkeypatch):
    from juicer_amd import capi
    am, cl, g = _pair("variants")
    ncl = capi.Network.from_synth(cl, 1.0, 0.0)
    want, _ = _want_sets(ncl.csr())
    total = sum(len(s) for s in want)
    with pytest.raises(capi.JuicerAmdError) as ei:                      # room for fewer labels than there are
        ncl.label_sets(cap=total - 1)
    assert ei.value.code == capi.JD_ENOMEM and str(total) in str(ei.value)
    assert _got_sets(ncl, cap=total)[0] == want
    # the bound on the lists (the sets that are no interval under the internal numbering), lowered through the development knob:
    # the documented error, naming the bound - never a silent fall-back to intervals
    monkeypatch.setenv("JD_LA_SET_MAX", "3")
    with pytest.raises(capi.JuicerAmdError) as ei:
        ncl.label_sets()
    assert ei.value.code == capi.JD_ENOMEM and "JD_LA_SET_MAX" in str(ei.value) and "more than 3 labels" in str(ei.value)
    # the generator's own numbering needs no list at all: the same bound is no obstacle
    am, cl, g = _pair("sp")
    assert _got_sets(capi.Network.from_synth(cl, 1.0, 0.0))[0] == _want_sets(capi.Network.from_synth(cl, 1.0, 0.0).csr())[0]


def _driver_input(n_states, init, src, dst, il, ol, final, cap):
    order = np.argsort(np.asarray(src), kind="stable")
    fin = [1 if c in set(final) else 0 for c in range(n_states)]
    lines = ["%d %d %d %d" % (n_states, init, len(src), cap), " ".join(str(x) for x in fin)]
    lines += ["%d %d %d %d" % (src[a], dst[a], il[a], ol[a]) for a in order]
    return "\n".join(lines) + "\n"


def test_stand_alone_driver_matches_python_sets(tmp_path):
    """The same computation without the library: jd_labelsets.h in a stand-alone host program, built with AddressSanitizer and
    UndefinedBehaviorSanitizer (any report ends the program with an error, which check=True turns into a failure)."""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    driver = str(tmp_path / "labelsets_driver")
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "juicer_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", driver, os.path.join(HERE, "labelsets_driver.cpp")])
    cases = []
    for kind in FIXTURES:
        am, cl, g = _pair(kind)
        S = cl.n_states
        csr_like = _csr_of(S, cl.src, cl.dst, cl.olab, cl.fstate)
        cases.append((S, 0, cl.src.tolist(), cl.dst.tolist(), cl.ilab.tolist(), cl.olab.tolist(), cl.fstate.tolist(), csr_like))
    n = _cycle_net()
    cases.append((n["n_states"], 0, n["src"], n["dst"], n["il"], n["ol"], n["final"], _csr_of(n["n_states"], n["src"], n["dst"], n["ol"], n["final"])))
    for S, init, src, dst, il, ol, final, csr in cases:
        want, want_mf = _want_sets(csr)
        out = subprocess.run([driver], input=_driver_input(S, init, src, dst, il, ol, final, 1 << 20), capture_output=True, text=True, check=True)
        lines = out.stdout.splitlines()
        assert lines[0] == "0 %d" % sum(len(s) for s in want)
        assert len(lines) == S + 1
        for c in range(S):
            v = [int(x) for x in lines[1 + c].split()]
            assert bool(v[0]) == want_mf[c] and v[1:] == want[c], c


def _csr_of(S, src, dst, ol, final):
    order = np.argsort(np.asarray(src), kind="stable")
    src, dst, ol = np.asarray(src)[order], np.asarray(dst)[order], np.asarray(ol)[order]
    row_ptr = np.zeros(S + 1, np.int64)
    np.add.at(row_ptr, src + 1, 1)
    fin_w = np.full(S, np.inf, np.float32)
    fin_w[np.asarray(final)] = 0.0
    return dict(row_ptr=np.cumsum(row_ptr), to=dst, olab=ol, fin_w=fin_w)
