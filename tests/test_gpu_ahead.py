"""k_path's reserve of camera rays and its gated bounds test on the GPU (-m gpu): renders whose units are shorter than the reserve, end
inside a block, span several blocks, change pixel and pass, every one bit for bit against the CPU oracle - the image and the three
counts. Scene 0 (Cornell box), Philox, depth 50 unless a case says otherwise; the untouched instantiations (TEA + LCG, the fog scene's
cold one) once each. Small renders run single-block units only (rtw_plan.h plan_path), so the cases with several blocks per unit set
the planner's knobs; the oracle's frames are rendered once per (scene, size, samples, shard, generator) and shared."""
import os

import numpy as np
import pytest

import oracle
from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu
DEPTH = 50
KNOBS = ("RTW_PATH_UNIT_BLOCKS", "RTW_PATH_FINE_BLOCKS", "RTW_BLOCKSUM_BYTES", "RTW_CULL")
_refs = {}
_blobs = {}


@pytest.fixture(scope="module")
def gpu():
    r = abi.Renderer(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def blob_of(scene, w, h):
    if (scene, w, h) not in _blobs:
        _blobs[(scene, w, h)] = abi.build_scene(scene, w, h)
    return _blobs[(scene, w, h)]


def reference(scene, w, h, spp, **kw):
    """the oracle's frame and counts, rendered once"""
    key = (scene, w, h, spp, tuple(sorted(kw.items())))
    if key not in _refs:
        img, st = oracle.render(blob_of(scene, w, h), abi.make_params(w, h, spp, DEPTH, **kw), threads=16)
        img.setflags(write=False)
        _refs[key] = (img, (st.samples, st.segments, st.shadow_rays))
    return _refs[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(gpu, scene, w, h, spp, **kw):
    gpu.upload_scene(blob_of(scene, w, h))
    img, st = gpu.render(abi.make_params(w, h, spp, DEPTH, **kw))
    ref, counts = reference(scene, w, h, spp, **kw)
    assert (st.samples, st.segments, st.shadow_rays) == counts
    assert np.array_equal(_bits(img), _bits(ref)), f"{np.count_nonzero(_bits(img) != _bits(ref))} words differ"


@pytest.mark.parametrize("spp", [1, 2, 3, 16, 17, 20, 48])
def test_sample_counts_around_the_reserve_and_the_block(gpu, spp):
    """fewer samples than K + 1, whole blocks, a cap inside a block"""
    check(gpu, 0, 96, 64, spp)


def test_fewer_pixels_than_a_wave(gpu):
    check(gpu, 0, 5, 3, 37)


@pytest.mark.parametrize("row0,stride", [(1, 3), (3, 8)])
def test_interleaved_shards(gpu, row0, stride):
    check(gpu, 0, 250, 130, 144, row0=row0, row_stride=stride)


@pytest.mark.parametrize("cull", ["0", "1"])
def test_with_and_without_the_cull(gpu, monkeypatch, cull):
    monkeypatch.setenv("RTW_CULL", cull)
    check(gpu, 0, 250, 130, 144, row0=3, row_stride=8)


@pytest.mark.parametrize("env", [
    {"RTW_BLOCKSUM_BYTES": str(8 * 96 * 64 * 16)},                        # three k_path passes of 8, 8 and 2 blocks: block0 > 0
    {"RTW_PATH_UNIT_BLOCKS": "4", "RTW_PATH_FINE_BLOCKS": "2"},           # 4-block units, then single blocks
    {"RTW_PATH_UNIT_BLOCKS": "8", "RTW_PATH_FINE_BLOCKS": "2"},           # 8-block units that store unit sums
    {"RTW_PATH_UNIT_BLOCKS": "8", "RTW_PATH_FINE_BLOCKS": "0"},           # the last unit is cut by the pass and the cap
], ids=["passes", "units_of_4", "units_of_8", "no_end_game"])
def test_several_passes_and_blocks_per_unit(gpu, monkeypatch, env):
    """276 samples = 17 blocks and 4 samples: the reserve runs across block boundaries inside a unit and stops at the unit's end"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    check(gpu, 0, 96, 64, 276)


def test_sample_offset_calls(gpu):
    """48 samples as three calls of 16 at sample_offset 0, 16, 32: each call is the oracle's call"""
    for off in (0, 16, 32):
        check(gpu, 0, 96, 64, 16, sample_offset=off, samples_per_pass=16)


def test_adaptive_render_list_passes(gpu):
    """the LIST instantiation: every pixel of the adaptive image is the oracle's pixel at its own sample count"""
    w, h = 96, 64
    gpu.upload_scene(blob_of(0, w, h))
    p = abi.make_params(w, h, 96, DEPTH)
    _, _, err, _ = gpu.render_adaptive(p, np.inf, min_spp=32)
    e = err[np.isfinite(err) & (err > 0)]
    img, spp, _, st = gpu.render_adaptive(p, float(np.quantile(e, 0.5)), min_spp=32, dilate=0)
    assert len(np.unique(spp)) >= 2, np.unique(spp)
    assert st.samples == int(spp.astype(np.int64).sum())
    for n in np.unique(spp):
        ref, _ = reference(0, w, h, int(n))
        m = spp == n
        assert np.array_equal(_bits(img[m]), _bits(ref[m])), f"spp {n}: {np.count_nonzero(_bits(img[m]) != _bits(ref[m]))} words differ"


def test_accumulation_session_of_three_adds(gpu):
    w, h = 96, 64
    gpu.upload_scene(blob_of(0, w, h))
    gpu.accum_begin(abi.make_params(w, h, 48, DEPTH))
    try:
        tot = [0, 0, 0]
        for done in (16, 32, 48):
            st = gpu.accum_add(16)
            for k, v in enumerate((st.samples, st.segments, st.shadow_rays)):
                tot[k] += v
            ref, counts = reference(0, w, h, done)
            assert np.array_equal(_bits(gpu.accum_read()), _bits(ref)), done
            assert tuple(tot) == counts, done
    finally:
        gpu.accum_end()


def test_untouched_generator_tea_lcg(gpu):
    check(gpu, 0, 96, 64, 20, rng_kind=abi.RTW_RNG_TEA_LCG)


def test_untouched_cold_instantiation_fog(gpu):
    check(gpu, 3, 96, 64, 17)
