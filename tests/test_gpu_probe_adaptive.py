"""GPU suite of the adaptive probes (include/rtw.h rtw_probe_adaptive / rtw_probe_adaptive_device). The referee is built from the
library's own older entry points: sample s of probe i is the rtw_radiance sample (irradiance) or the RTW_CAST_ANY query (occlusion)
of ray (p_i, d_is, tmin, tmax), d_is restated by probe_ref.directions; the samples' block sums go through
probe_adaptive_ref.reference, which gives n_i, err and the value. spp_out must be equal and rgba_out and error_out equal in bits,
and every row must be rtw_probe's row at spp = n_i. Then unit and pass boundaries, the threshold's extremes, the stats, independence
of the batch, chunks, slab ranges and knobs, the torch path, every refusal, groups, sessions, the older entry points afterwards and
the baker."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # (before the HIP library is loaded, as in a run of the whole suite)

import geometry_ref as G
import probe_adaptive_ref as PA
import probe_ref as P
import radiance_ref as R
from gpu_common import (BOTH, GOLDEN_PAIR, KNOBS, UPLOADS, check_golden_render, check_stream_order,  # noqa: F401
                        golden, gpu, left_alone, same3, same_words as same, sentinel_stats, upload)
from raytracing_weekend_amd import abi, bake
from raytracing_weekend_amd.torch_probe import probe_adaptive_torch

pytestmark = pytest.mark.gpu

MODES = ("irradiance", "occlusion")
TMAX = {"scene0": 150.0, "scene1": 3.0, "scene3": 150.0, "random_volumes_motion": 70.0}  # test_gpu_probe.py's occlusion distances
N, CAP, MIN_SPP, DEPTH, KEY, THRESHOLD = 96, 256, 32, 8, 5, 0.02  # the rehearsed inputs (test_probe_adaptive_cpu.py)


def describe(got, want):
    bad = np.nonzero((got[1] != want[1]) | (got[0].view(np.uint32) != want[0].view(np.uint32)).any(1) | (got[2].view(np.uint32) != want[2].view(np.uint32)))[0]
    if not len(bad):
        return ""
    i = bad[0]
    return f"{len(bad)} probes differ, first {i}: n {got[1][i]} != {want[1][i]}, err {got[2][i]!r} != {want[2][i]!r}, {got[0][i]} != {want[0][i]}"


@functools.lru_cache(maxsize=None)
def floor_of_scene0():
    blob = R.scene("scene0")
    prims = abi.parse_scene(blob)["prims"]
    return blob, next(i for i, p in enumerate(prims) if p.type == abi.PRIM_RECT_Y and p.p[4] == 0.0 and p.xform == 0)


@functools.lru_cache(maxsize=None)
def floor_probes(nu=12, nv=8):
    blob, floor = floor_of_scene0()
    return bake.rect_probes(blob, floor, nu, nv)


_probes = {}


def probes_of(gpu, name, mode):
    """The batch of a scene (the scene must be uploaded): scene 0 takes the rehearsed floor probes, the others N probes from
    gpu.cast hits; occlusion at the scene's TMAX."""
    if name not in _probes:
        _probes[name] = floor_probes() if name == "scene0" else P.scene_probes(gpu.cast, R.scene(name), N)
    p = _probes[name].copy()
    if mode == "occlusion":
        p[:, 7] = TMAX[name]
    return p


_blocks = {}


def blocks_of(gpu, tag, probes, mode, cap, depth=DEPTH, rng_kind=abi.RTW_RNG_PHILOX, estimator=0, sample_offset=0, key_offset=KEY):
    """The referee's input, computed once per case and shared: (cap / 16, n, 3) block sums from gpu.radiance(spp = 1) per sample index,
    or (cap / 16, n) counts from gpu.cast(mode="any"). The scene of `tag` must be uploaded."""
    key = (tag, mode, cap, depth, rng_kind, estimator, sample_offset, key_offset)
    if key not in _blocks:
        d = P.directions(probes, cap, rng_kind=rng_kind, sample_offset=sample_offset, key_offset=key_offset)
        if mode == "irradiance":
            smp = np.empty((cap, len(probes), 3), np.float32)
            for s in range(cap):
                smp[s] = gpu.radiance(P.rays_of(probes, d, s), 1, depth, rng_kind=rng_kind, estimator=estimator, sample_offset=sample_offset + s,
                                      key_offset=key_offset)[:, :3]
            _blocks[key] = PA.block_sums(smp)
        else:
            open_ = np.empty((cap, len(probes)), bool)
            for s in range(cap):
                open_[s] = gpu.cast(P.rays_of(probes, d, s), mode="any", want=("prim",))["prim"] < 0
            _blocks[key] = PA.block_counts(open_)
    return _blocks[key]


def check_against_referee(gpu, tag, probes, mode, rng_kind=abi.RTW_RNG_PHILOX, estimator=0, cap=CAP, min_spp=MIN_SPP, step_spp=0,
                          threshold=THRESHOLD, sample_offset=0, key_offset=KEY, assert_spread=False):
    blocks = blocks_of(gpu, tag, probes, mode, cap, DEPTH, rng_kind, estimator, sample_offset, key_offset)
    want = PA.reference(blocks, threshold, min_spp, step_spp, cap, mode)
    kw = dict(rng_kind=rng_kind, estimator=estimator, sample_offset=sample_offset, key_offset=key_offset, mode=mode)
    st = abi.Stats()
    got = gpu.probe_adaptive(probes, cap, DEPTH, threshold, min_spp=min_spp, step_spp=step_spp, stats=st, **kw)
    print(f"{tag} {mode} rng {rng_kind} estimator {estimator} offset {sample_offset}: n_i {PA.histogram(got[1])}, referee {PA.histogram(want[1])}")
    assert got[0].shape == (len(probes), 4) and got[1].shape == (len(probes),) and got[2].shape == (len(probes),)
    assert same3(got, want), describe(got, want)
    assert st.samples == int(got[1].astype(np.int64).sum()) and st.seconds > 0.0
    for n_i in np.unique(got[1]):  # every row is rtw_probe's row at its own sample count
        rows = got[1] == n_i
        uniform = gpu.probe(probes, int(n_i), DEPTH, **kw)
        assert same(got[0][rows], uniform[rows]), (int(n_i), got[0][rows][0], uniform[rows][0])
    if assert_spread:
        assert PA.not_vacuous(got[1], min_spp, cap), PA.histogram(got[1])
    return got, st


# ---------------------------------------------------------------- 1. bit equality with the referee
@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("mode", MODES)
def test_the_rehearsed_floor_probes_equal_the_referee_in_bits(gpu, monkeypatch, mode, rng_kind):
    upload(gpu, monkeypatch, R.scene("scene0"))
    check_against_referee(gpu, "scene0", probes_of(gpu, "scene0", mode), mode, rng_kind, assert_spread=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("how", list(UPLOADS))
@pytest.mark.parametrize("name", ["scene1", "scene3", "random_volumes_motion"])
def test_other_scenes_as_uploaded_and_with_the_tree_forced(gpu, monkeypatch, name, how, mode):
    upload(gpu, monkeypatch, R.scene(name), how)
    check_against_referee(gpu, name, probes_of(gpu, name, mode), mode)


@pytest.mark.parametrize("estimator", [1, 2, 3])
def test_the_corrected_estimators_on_scene_0(gpu, monkeypatch, estimator):
    upload(gpu, monkeypatch, R.scene("scene0"))
    check_against_referee(gpu, "scene0", probes_of(gpu, "scene0", "irradiance"), "irradiance", estimator=estimator)


# ---------------------------------------------------------------- 2. unit and pass boundaries
@pytest.mark.parametrize("sample_offset", [0, 16])
def test_passes_that_end_on_and_cross_a_unit_boundary(gpu, monkeypatch, sample_offset):
    """(32, 48, 272): 32 80 128 176 224 272 - the pass to 128 ends a summation unit, the pass from 224 to 272 crosses one."""
    upload(gpu, monkeypatch, R.scene("scene0"))
    for mode in MODES:
        got, _ = check_against_referee(gpu, "scene0", probes_of(gpu, "scene0", mode), mode, cap=272, step_spp=48, sample_offset=sample_offset)
        assert set(PA.histogram(got[1])) <= {32, 80, 128, 176, 224, 272}


# ---------------------------------------------------------------- 3. the threshold's extremes
def test_threshold_zero_infinity_and_depth_zero(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene0"))
    for mode in MODES:
        probes = probes_of(gpu, "scene0", mode)
        kw = dict(key_offset=KEY, mode=mode)
        for threshold, n_all in ((0.0, CAP), (float("inf"), MIN_SPP)):
            s0, s1 = abi.Stats(), abi.Stats()
            out, spp, err = gpu.probe_adaptive(probes, CAP, DEPTH, threshold, min_spp=MIN_SPP, stats=s0, **kw)
            assert (spp == n_all).all()
            assert same(out, gpu.probe(probes, n_all, DEPTH, stats=s1, **kw))
            assert (s0.samples, s0.segments, s0.shadow_rays, s0.algorithmic_bytes) == (s1.samples, s1.segments, s1.shadow_rays, s1.algorithmic_bytes)
            assert np.isfinite(err).all() and (err >= 0).all() and (err > 0).any()
    # no segment is traced: zeros, err 0, so min_spp under any positive threshold and the cap under 0
    probes = probes_of(gpu, "scene0", "irradiance")
    zero = np.tile(np.array([0, 0, 0, 1], np.float32), (N, 1))
    for threshold, n_all in ((THRESHOLD, MIN_SPP), (0.0, CAP)):
        st = abi.Stats(segments=5)
        out, spp, err = gpu.probe_adaptive(probes, CAP, 0, threshold, min_spp=MIN_SPP, key_offset=KEY, stats=st)
        assert same(out, zero) and (spp == n_all).all() and not err.any()
        assert (st.samples, st.segments, st.shadow_rays) == (N * n_all, 0, 0)


# ---------------------------------------------------------------- 4. stats
def test_stats_are_those_of_the_samples_taken(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene0"))
    probes = probes_of(gpu, "scene0", "irradiance")
    st = abi.Stats()
    out, spp, _ = gpu.probe_adaptive(probes, CAP, DEPTH, THRESHOLD, min_spp=MIN_SPP, key_offset=KEY, stats=st)
    seg = shadow = 0
    for i in range(N):
        s1 = abi.Stats()
        one = gpu.probe(probes[i:i + 1], int(spp[i]), DEPTH, key_offset=KEY + i, stats=s1)
        assert same(one, out[i:i + 1])
        seg, shadow = seg + s1.segments, shadow + s1.shadow_rays
    assert (st.samples, st.segments, st.shadow_rays) == (int(spp.astype(np.int64).sum()), seg, shadow) and seg > st.samples
    assert st.algorithmic_bytes == 128 * st.segments + 32 * st.samples and st.seconds > 0.0
    assert not any(st.kernel_seconds) and not any(st.kernel_launches) and not any(st.kernel_segments)
    so = abi.Stats(segments=9)
    _, spp_o, _ = gpu.probe_adaptive(probes_of(gpu, "scene0", "occlusion"), CAP, DEPTH, THRESHOLD, min_spp=MIN_SPP, key_offset=KEY, mode="occlusion", stats=so)
    assert (so.samples, so.shadow_rays, so.segments, so.algorithmic_bytes) == (int(spp_o.astype(np.int64).sum()),) * 2 + (0, 0) and so.seconds > 0.0


# ---------------------------------------------------------------- 5. independence
def test_a_probe_does_not_depend_on_its_batch(gpu, monkeypatch):
    """2^17 + 3 floor probes, cap 64 (32 48 64): 257 scattered probes equal one-probe calls with their own keys."""
    upload(gpu, monkeypatch, R.scene("scene0"))
    n = (1 << 17) + 3
    probes = floor_probes(512, 257)[:n].copy()
    probes[:, 7] = TMAX["scene0"]
    ends = np.array([0, 1, 63, 64, n - 2, n - 1])
    pick = np.concatenate([ends, np.setdiff1d(np.random.default_rng(3).choice(n, 300, replace=False), ends)[:251]])
    assert len(np.unique(pick)) == 257
    for mode in MODES:
        kw = dict(min_spp=32, mode=mode)
        st = abi.Stats()
        big = gpu.probe_adaptive(probes, 64, 4, THRESHOLD, key_offset=0, stats=st, **kw)
        hist = PA.histogram(big[1])
        print(f"{mode}: n_i of {n} probes {hist}")
        assert st.samples == int(big[1].astype(np.int64).sum()) and set(hist) <= {32, 48, 64} and len(hist) >= 2 and (big[0][:, 3] == 1.0).all()
        for j in pick:
            one = gpu.probe_adaptive(probes[j:j + 1], 64, 4, THRESHOLD, key_offset=int(j), **kw)
            assert same3(one, tuple(a[j:j + 1] for a in big)), (mode, j, one, big[0][j], big[1][j], big[2][j])


def test_chunks_slab_ranges_lds_and_wrapping_keys_change_no_bit(gpu, monkeypatch):
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    probes = floor_probes(80, 63)[:5003].copy()
    probes[:, 7] = TMAX["scene0"]
    d_probes = torch.from_numpy(probes).cuda()
    k0 = 2 ** 32 - 2501  # the keys wrap in the middle of the batch
    for mode in MODES:
        kw = dict(min_spp=32, key_offset=k0, mode=mode)
        s0 = abi.Stats()
        whole = gpu.probe_adaptive(probes, 80, 6, THRESHOLD, stats=s0, **kw)
        assert len(PA.histogram(whole[1])) >= 2
        # past the wrap probe i has key i - 2501: the tail equals a call that starts at key 0
        assert same3(gpu.probe_adaptive(probes[2501:], 80, 6, THRESHOLD, min_spp=32, key_offset=0, mode=mode), tuple(a[2501:] for a in whole))
        variants = ({"RTW_RADIANCE_CHUNK": "1000"},
                    {"RTW_RADIANCE_SLAB_BYTES": str(700 * 2 * 16)},  # 700 positions of the first pass's two blocks: eight ranges, fewer later
                    {"RTW_RADIANCE_CHUNK": "1000", "RTW_RADIANCE_SLAB_BYTES": "16"})  # one position per range
        for env in variants:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            s1 = abi.Stats()
            assert same3(gpu.probe_adaptive(probes, 80, 6, THRESHOLD, stats=s1, **kw), whole), env
            assert (s1.samples, s1.segments, s1.shadow_rays) == (s0.samples, s0.segments, s0.shadow_rays)
            if "RTW_RADIANCE_CHUNK" not in env:
                got = probe_adaptive_torch(gpu, d_probes, 80, 6, THRESHOLD, **kw)
                assert same3(tuple(t.cpu().numpy() for t in got), whole), env
            for k in env:
                monkeypatch.delenv(k)
        for lds in ("0", "48"):  # read at upload
            monkeypatch.setenv("RTW_LDS_KB", lds)
            monkeypatch.setenv("RTW_BRUTE_MAX", "0")
            gpu.upload_scene(blob)
            assert same3(gpu.probe_adaptive(probes, 80, 6, THRESHOLD, **kw), whole), lds
        upload(gpu, monkeypatch, blob)


# ---------------------------------------------------------------- 6. the device path
def test_probe_adaptive_torch_equals_the_host_path_and_is_ordered_on_the_current_stream(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene0"))
    for mode in MODES:
        probes = probes_of(gpu, "scene0", mode)
        d_probes = torch.from_numpy(probes).cuda()
        kw = dict(min_spp=MIN_SPP, key_offset=KEY, mode=mode)
        s0, st = abi.Stats(), abi.Stats()
        want = gpu.probe_adaptive(probes, CAP, DEPTH, THRESHOLD, stats=s0, **kw)
        got = probe_adaptive_torch(gpu, d_probes, CAP, DEPTH, THRESHOLD, stats=st, **kw)
        assert all(t.is_cuda for t in got) and got[1].dtype == torch.int32 and tuple(got[0].shape) == (N, 4) and tuple(got[1].shape) == (N,)
        assert same3(tuple(t.cpu().numpy() for t in got), want)
        assert (st.segments, st.shadow_rays, st.samples) == (s0.segments, s0.shadow_rays, s0.samples) and st.seconds > 0.0
        check_stream_order(lambda t: probe_adaptive_torch(gpu, t, CAP, DEPTH, THRESHOLD, **kw), d_probes,
                           lambda got: same3(tuple(t.cpu().numpy() for t in got), want))
        empty = probe_adaptive_torch(gpu, torch.zeros((0, 8), device="cuda:0"), 64, 4, THRESHOLD, mode=mode)
        assert [tuple(t.shape) for t in empty] == [(0, 4), (0,), (0,)]
    for cap, mode in ((0, "irradiance"), (64, "ao")):
        with pytest.raises(ValueError):
            probe_adaptive_torch(gpu, d_probes, cap, DEPTH, THRESHOLD, mode=mode)


# ---------------------------------------------------------------- 7. refusals
def test_every_refusal_leaves_the_context_usable_and_writes_nothing(gpu, monkeypatch):
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    probes = probes_of(gpu, "scene0", "irradiance")
    want = gpu.probe_adaptive(probes, 64, DEPTH, THRESHOLD, min_spp=MIN_SPP, key_offset=KEY)
    lib, n = gpu.lib, N
    out, spp, err = np.full((n, 4), -7, np.float32), np.full(n, -7, np.int32), np.full(n, -7, np.float32)
    d_probes = torch.from_numpy(np.concatenate([probes.ravel(), np.zeros(8, np.float32)])).cuda()
    d_out = torch.full((n * 4 + 8,), -7.0, device="cuda:0")
    d_spp = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda:0")
    d_err = torch.full((n + 8,), -7.0, device="cuda:0")
    R_, O_, S_, E_ = probes.ctypes.data, out.ctypes.data, spp.ctypes.data, err.ctypes.data
    D_, DO_, DS_, DE_ = d_probes.data_ptr(), d_out.data_ptr(), d_spp.data_ptr(), d_err.data_ptr()

    def pp(**kw):
        p = abi.make_probe_params(64, DEPTH, key_offset=KEY)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def ad(min_spp=MIN_SPP, step_spp=0, threshold=THRESHOLD, dilate=0):
        return C.byref(abi.Adaptive(min_spp, step_spp, threshold, dilate))
    fresh = abi.Renderer(0)
    try:
        assert lib.rtw_probe_adaptive(fresh.ctx, R_, n, pp(), ad(), O_, S_, E_, None) == -3        # RTW_ERR_NO_SCENE
        assert lib.rtw_probe_adaptive_device(fresh.ctx, D_, n, pp(), ad(), DO_, DS_, DE_, None, None) == -3
        assert b"rtw_upload_scene" in lib.rtw_last_error(fresh.ctx)
    finally:
        fresh.close()

    def still_fine():
        assert same3(gpu.probe_adaptive(probes, 64, DEPTH, THRESHOLD, min_spp=MIN_SPP, key_offset=KEY), want)
    # rtw_probe's refusals, then the adaptive ones: the cap (params->spp), min_spp, step_spp, the threshold, dilate, a NULL ad
    bad = [(None, ad()), (pp(spp=0), ad()), (pp(spp=-16), ad()), (pp(max_depth=-1), ad()), (pp(rng_kind=2), ad()), (pp(rng_kind=-1), ad()),
           (pp(estimator=4), ad()), (pp(estimator=-1), ad()), (pp(sample_offset=-1), ad()), (pp(sample_offset=2 ** 31 - 64), ad()),
           (pp(mode=-1), ad()), (pp(mode=2), ad()), (pp(mode=1, spp=0), ad()), (pp(mode=1, estimator=4), ad()),
           (pp(), None), (pp(spp=72), ad()), (pp(spp=16), ad(16)), (pp(), ad(16)), (pp(), ad(40)), (pp(), ad(80)), (pp(), ad(0)),
           (pp(), ad(step_spp=-16)), (pp(), ad(step_spp=8)), (pp(), ad(threshold=-0.5)), (pp(), ad(threshold=float("nan"))),
           (pp(), ad(dilate=1)), (pp(), ad(dilate=2)), (pp(), ad(dilate=-1)), (pp(mode=1), ad(dilate=1)), (pp(mode=1), None)]
    host = [(R_, n, p, a, O_) for p, a in bad] + [(R_, 1 << 31, pp(), ad(), O_), (None, n, pp(), ad(), O_), (R_, n, pp(), ad(), None),
                                                  (R_, n, pp(mode=1), ad(), None)]
    for r_, m, p, a, o_ in host:
        st = sentinel_stats()
        assert lib.rtw_probe_adaptive(gpu.ctx, r_, m, p, a, o_, S_, E_, C.byref(st)) == -1
        assert lib.rtw_last_error(gpu.ctx) and left_alone(st)  # a refused call leaves *stats alone
    still_fine()
    dev = [(D_, n, p, a, DO_, DS_, DE_) for p, a in bad] + [
        (D_, 1 << 31, pp(), ad(), DO_, DS_, DE_), (None, n, pp(), ad(), DO_, DS_, DE_), (D_, n, pp(), ad(), None, DS_, DE_),
        (D_ + 4, n, pp(), ad(), DO_, DS_, DE_), (D_ + 8, n, pp(mode=1), ad(), DO_, DS_, DE_), (D_, n, pp(), ad(), DO_ + 4, DS_, DE_),
        (D_, n, pp(mode=1), ad(), DO_ + 8, DS_, DE_), (D_, n, pp(), ad(), DO_, DS_ + 2, DE_), (D_, n, pp(), ad(), DO_, DS_, DE_ + 1),
        (D_, n, pp(mode=1), ad(), DO_, DS_ + 1, None)]
    for r_, m, p, a, o_, s_, e_ in dev:
        st = sentinel_stats()
        assert lib.rtw_probe_adaptive_device(gpu.ctx, r_, m, p, a, o_, s_, e_, None, C.byref(st)) == -1
        assert left_alone(st)
    still_fine()  # after a misaligned pointer as after any other refusal: the next call works
    torch.cuda.synchronize()
    assert (out == -7).all() and (spp == -7).all() and (err == -7).all()  # no refused call wrote anything
    assert bool((d_out == -7).all().item()) and bool((d_spp == -7).all().item()) and bool((d_err == -7).all().item())
    # n = 0 is fine and launches nothing, whatever the pointers
    for mode in (0, 1):
        st = abi.Stats(segments=77)
        assert lib.rtw_probe_adaptive(gpu.ctx, None, 0, pp(mode=mode), ad(), None, None, None, C.byref(st)) == 0
        assert (st.segments, st.samples, st.seconds) == (0, 0, 0.0)
        assert lib.rtw_probe_adaptive_device(gpu.ctx, None, 0, pp(mode=mode), ad(), None, None, None, None, None) == 0
        assert lib.rtw_probe_adaptive_device(gpu.ctx, D_ + 4, 0, pp(mode=mode), ad(), DO_ + 4, DS_ + 1, DE_ + 1, None, None) == 0
        empty = gpu.probe_adaptive(np.zeros((0, 8), np.float32), 64, 4, THRESHOLD, mode=MODES[mode])
        assert [a.shape for a in empty] == [(0, 4), (0,), (0,)]
    # spp_out and error_out may be NULL; from probe 1 on the pointers are aligned enough
    assert lib.rtw_probe_adaptive(gpu.ctx, R_, n, pp(), ad(), O_, None, None, None) == 0 and same(out, want[0]) and (spp == -7).all() and (err == -7).all()
    assert lib.rtw_probe_adaptive_device(gpu.ctx, D_ + 32, n - 1, pp(key_offset=KEY + 1), ad(), DO_ + 16, DS_ + 4, None, None, None) == 0
    assert same(d_out[4:4 + 4 * (n - 1)].cpu().numpy().reshape(-1, 4), want[0][1:]) and np.array_equal(d_spp[1:n].cpu().numpy(), want[1][1:])
    assert bool((d_err == -7).all().item())


# ---------------------------------------------------------------- 8. neighbours
def test_a_group_answers_on_its_first_device_with_single_device_bits(gpu, monkeypatch):
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    group = abi.Renderer([0, 0])
    try:
        probes = probes_of(gpu, "scene0", "irradiance")
        out, spp, err = np.zeros((N, 4), np.float32), np.zeros(N, np.int32), np.zeros(N, np.float32)
        p0, a0 = abi.make_probe_params(64, DEPTH), abi.Adaptive(32, 0, THRESHOLD, 0)
        assert group.lib.rtw_probe_adaptive(group.ctx, probes.ctypes.data, N, C.byref(p0), C.byref(a0), out.ctypes.data, spp.ctypes.data,
                                            err.ctypes.data, None) == -3
        group.upload_scene(blob)
        for mode in MODES:
            probes = probes_of(gpu, "scene0", mode)
            kw = dict(min_spp=MIN_SPP, key_offset=KEY, mode=mode)
            s0, s1 = abi.Stats(), abi.Stats()
            want = gpu.probe_adaptive(probes, CAP, DEPTH, THRESHOLD, stats=s0, **kw)
            assert same3(group.probe_adaptive(probes, CAP, DEPTH, THRESHOLD, stats=s1, **kw), want)
            assert (s1.samples, s1.segments, s1.shadow_rays) == (s0.samples, s0.segments, s0.shadow_rays)
            got = probe_adaptive_torch(group, torch.from_numpy(probes).cuda(), CAP, DEPTH, THRESHOLD, **kw)
            assert same3(tuple(t.cpu().numpy() for t in got), want)
    finally:
        group.close()


def test_an_open_accumulation_session_goes_on_bit_exactly(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene0"))
    want = {m: gpu.probe_adaptive(probes_of(gpu, "scene0", m), CAP, DEPTH, THRESHOLD, min_spp=MIN_SPP, key_offset=KEY, mode=m) for m in MODES}
    p = abi.make_params(32, 32, 32, 6)
    one_shot, _ = gpu.render(p)
    gpu.accum_begin(p)
    try:
        gpu.accum_add(16)
        for m in MODES:
            assert same3(gpu.probe_adaptive(probes_of(gpu, "scene0", m), CAP, DEPTH, THRESHOLD, min_spp=MIN_SPP, key_offset=KEY, mode=m), want[m])
        gpu.accum_add(16)
        assert same(gpu.accum_read(), one_shot)
        assert gpu.accum_status().done == 32
    finally:
        gpu.accum_end()
    for m in MODES:
        assert same3(gpu.probe_adaptive(probes_of(gpu, "scene0", m), CAP, DEPTH, THRESHOLD, min_spp=MIN_SPP, key_offset=KEY, mode=m), want[m])


def test_probe_radiance_and_render_are_what_they_were_before_adaptive_calls(gpu, monkeypatch):
    """The slab is shared: calls beyond 128 spp of the older entry points before and after adaptive calls of both modes."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for g in map(golden, GOLDEN_PAIR):
        blob, rng, seed = g.blob, g.rng, g.seed
        gpu.upload_scene(blob)
        rays, _, _ = G.scene_rays(blob, 5, 300)
        rays[:, 6], rays[:, 7] = 1e-6, 1e27
        probes = P.scene_probes(gpu.cast, blob, 300, tmax=100.0)
        rad = gpu.radiance(rays, 160, 4, rng_kind=rng)
        a = gpu.probe(probes, 160, 3, rng_kind=rng, estimator=1)
        b = gpu.probe(probes, 160, 3, rng_kind=rng, mode="occlusion")
        for mode in MODES:
            out, n_i, err = gpu.probe_adaptive(probes, 192, 4, THRESHOLD, min_spp=32, rng_kind=rng, mode=mode)
            assert np.isfinite(out).all() and set(np.unique(n_i)) <= {32, 48, 80, 128, 192} and (err >= 0).all()
        check_golden_render(gpu, g)
        assert same(gpu.radiance(rays, 160, 4, rng_kind=rng), rad)
        assert same(gpu.probe(probes, 160, 3, rng_kind=rng, estimator=1), a) and same(gpu.probe(probes, 160, 3, rng_kind=rng, mode="occlusion"), b)


# ---------------------------------------------------------------- 9. the baker
def test_bake_rect_adaptive_on_the_cornell_floor(gpu, monkeypatch):
    blob, floor = floor_of_scene0()
    upload(gpu, monkeypatch, blob)
    nu, nv = 16, 12
    probes = bake.rect_probes(blob, floor, nu, nv)
    for mode in MODES:
        kw = dict(min_spp=32, key_offset=3, mode=mode)
        m, spp, err = bake.bake_rect_adaptive(gpu, blob, floor, nu, nv, 128, 6, THRESHOLD, **kw)
        want = gpu.probe_adaptive(probes, 128, 6, THRESHOLD, **kw)
        assert m.shape == (nv, nu, 4) and spp.shape == (nv, nu) and err.shape == (nv, nu) and spp.dtype == np.int32
        assert same3((m.reshape(-1, 4), spp.reshape(-1), err.reshape(-1)), want) and len(np.unique(spp)) >= 2
