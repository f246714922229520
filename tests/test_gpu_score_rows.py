"""The scoring kernels under the decoder's own launch arguments: jd_debug_score_rows (one launch_gmm call on a prefilled, guarded
buffer) over the cases of tests/score_rows_cases.py - row maps with repeats and unused rows, skip_unused, bounded grids, tile lists,
both tile widths - for jd_gmm_kernel<0>, jd_gmm_kernel39<16|64>, jd_gmm_fast39<16|64>, jd_gmm_fast<16|64> and jd_hybrid_kernel.  A test
asserts the kernel that ran and its grid, then every cell of the buffer: untouched (the prefill, bit for bit), value (the CPU oracle's:
bit for bit under JD_SCORE_EXACT, within RTOL under JD_SCORE_FAST; rows of one frame identical) or unspecified."""
import numpy as np
import pytest

import score_rows_cases as sc
from score_rows_cases import CASES, CASE_IDS
from test_gpu_fastscore import RTOL
from test_gpu_logadd import RTOL as RTOL_LOGADD

pytestmark = pytest.mark.gpu

_GPU_MODELS = {}


def _models(key):
    if key not in _GPU_MODELS:
        _GPU_MODELS[key] = sc.model(key).gpu_models()
    return _GPU_MODELS[key]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_score_rows(built, case):
    from juicer_amd import capi
    assert RTOL == RTOL_LOGADD == 1e-4
    assert capi.KERNEL_NAMES == sc.KERNEL_NAMES
    m = sc.model(case.model_key)
    got, kernel, grid = capi.debug_score_rows(_models(case.model_key), m.frames, case.row_src, case.prefill(), mode=case.mode,
                                              skip_unused=case.skip_unused, max_blocks=case.max_blocks, used_row_tiles=case.used_row_tiles,
                                              rt_base=case.rt_base, guard_rows=case.guard_rows)
    assert kernel == case.kernel, "ran %s, the case is %s's" % (capi.KERNEL_NAMES[kernel], sc.KERNEL_NAMES[case.kernel])
    assert grid == case.grid()
    sc.check_buffer(case, got, RTOL)


def test_tile_list_is_refused_where_no_kernel_takes_one(built):
    """launch_gmm's own refusal, passed on: exact scoring of D != 39 (64-row tiles) has no tile list (hybrid models: refused on the host,
    tests/test_score_rows_cpu.py)"""
    from juicer_amd import capi
    for key in ("synth13_17",):
        m = sc.model(key)
        src = np.arange(130, dtype=np.int32) % sc.N_FRAMES
        pre = np.full((130, m.G), -1.0, np.float32)
        with pytest.raises(capi.JuicerAmdError) as e:
            capi.debug_score_rows(_models(key), m.frames, src, pre, rt_base=[0], used_row_tiles=1)
        assert e.value.code == capi.JD_EINVAL and "tile lists" in str(e.value)


def test_score_frames_is_the_identity_case(built):
    """jd_am_score_frames and the entry share their device side: an identity map, no guards, is the same table bit for bit"""
    from juicer_amd import capi
    m = sc.model("crafted39")
    gam = _models("crafted39")
    for mode in (capi.SCORE_EXACT, capi.SCORE_FAST):
        a = gam.score_frames(m.frames, mode=mode)
        b, kernel, _ = capi.debug_score_rows(gam, m.frames, np.arange(sc.N_FRAMES), np.zeros_like(a), mode=mode)
        assert kernel == (capi.KERNEL_GMM39_16 if mode == capi.SCORE_EXACT else capi.KERNEL_GMM_FAST39_16)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
