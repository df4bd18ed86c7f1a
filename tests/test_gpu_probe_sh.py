"""GPU suite of the spherical-harmonic probes (include/rtw.h rtw_probe_sh / rtw_probe_sh_device). The referee is the contract itself:
sample s of point i is the rtw_radiance sample of ray (p_i, d_is, tmin, tmax), with d_is and the basis restated by sh_ref - and
rtw_radiance is refereed by the oracle in its own suite. Then the summation units and offsets, independence of the batch, chunks and
slab ranges, keys that wrap, the unused floats, the analytic sky, the torch path, every refusal, groups, sessions and the older
entry points afterwards."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # (before the HIP library is loaded, as in a run of the whole suite)

import geometry_ref as G
import gpu_common
import probe_ref as P
import radiance_ref as R
import sh_ref as S
from gpu_common import (BOTH, GOLDEN_PAIR, KNOBS, UPLOADS, check_golden_render, check_stream_order,  # noqa: F401
                        golden, gpu, left_alone, same, sentinel_stats, upload)
from raytracing_weekend_amd import abi, bake
from raytracing_weekend_amd.torch_probe_sh import probe_sh_torch

pytestmark = pytest.mark.gpu
first_difference = functools.partial(gpu_common.first_difference, what="points")

SCENES = ("scene0", "scene1", "scene3", "random_volumes_motion")
N, SPP, DEPTH, KEY = R.N, R.SPP, R.DEPTH, R.KEY  # 96 points (one and a half waves), 48 spp (three blocks), depth 8, key offset 5


_points = {}


def points_of(gpu, name):
    """The batch of a scene: the positions of N probe_ref.scene_probes (the scene must be uploaded); made once. Floats 3..5 keep the
    probes' normals: a probe tensor is a valid point tensor."""
    if name not in _points:
        _points[name] = P.scene_probes(gpu.cast, R.scene(name), N)
    return _points[name]


@functools.lru_cache(maxsize=None)
def directions(n, spp, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, key_offset=0):
    return S.directions(n, spp, rng_kind=rng_kind, sample_offset=sample_offset, key_offset=key_offset)


def referee(gpu, points, spp, depth, rng_kind=abi.RTW_RNG_PHILOX, estimator=0, sample_offset=0, key_offset=0):
    """(expected (n, 9, 4), segments, shadow rays): one rtw_radiance call with spp = 1 per sample index on the rays (p_i, d_is), every
    Y_j * L_c in float32, each of the 27 sums in the library's order, / spp, times the float nearest 4 pi."""
    n = len(points)
    d = directions(n, spp, rng_kind, sample_offset, key_offset)
    smp = np.empty((spp, n, 4), np.float32)
    seg = shadow = 0
    for s in range(spp):
        st = abi.Stats()
        smp[s] = gpu.radiance(S.rays_of(points, d, s), 1, depth, rng_kind=rng_kind, estimator=estimator, sample_offset=sample_offset + s,
                              key_offset=key_offset, stats=st)
        seg, shadow = seg + st.segments, shadow + st.shadow_rays
    return S.project(smp, d, spp), seg, shadow


# ---------------------------------------------------------------- 1. every sample is the rtw_radiance sample, weighted by the basis
def check_main(gpu, name, rng_kind, estimator=0):
    points = points_of(gpu, name)
    want, seg, shadow = referee(gpu, points, SPP, DEPTH, rng_kind, estimator, key_offset=KEY)
    st = abi.Stats()
    got = gpu.probe_sh(points, SPP, DEPTH, rng_kind=rng_kind, estimator=estimator, key_offset=KEY, stats=st)
    lit = int((got[:, 0, :3] != 0).any(1).sum())
    print(f"{name} rng {rng_kind} estimator {estimator}: segments {st.segments} (referee {seg}), shadow rays {st.shadow_rays} ({shadow}), {lit} of {N} points have c0 != 0")
    assert got.shape == (N, 9, 4) and same(got, want), first_difference(got, want)
    assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, N * SPP)
    assert st.algorithmic_bytes == 128 * st.segments + 32 * st.samples and st.seconds > 0.0
    assert not any(st.kernel_seconds) and not any(st.kernel_launches) and not any(st.kernel_segments)
    # not vacuous: enough points see light, and the light has a direction
    assert lit >= N // 4 and (got[:, 1:4, :3] != 0).any() and (got[:, 4:, :3] != 0).any()
    assert not got[:, :, 3].any()  # w = 0


@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("how", list(UPLOADS))
@pytest.mark.parametrize("name", SCENES)
def test_every_sample_is_the_rtw_radiance_sample_times_the_basis(gpu, monkeypatch, name, how, rng_kind):
    upload(gpu, monkeypatch, R.scene(name), how)
    check_main(gpu, name, rng_kind)


@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("estimator", [1, 2, 3])
def test_under_the_corrected_estimators_on_scene_0(gpu, monkeypatch, estimator, rng_kind):
    upload(gpu, monkeypatch, R.scene("scene0"))
    check_main(gpu, "scene0", rng_kind, estimator)


# ---------------------------------------------------------------- 2. units, tails, offsets
@pytest.mark.parametrize("spp", [1, 16, 17, 129, 272])
def test_summation_blocks_units_and_sample_offsets(gpu, monkeypatch, spp):
    """One sample; one full block; a block and a one-sample tail; a unit and a one-sample unit (the slab and the resolve); two units
    and a 16-sample tail. Offset 40 starts inside what would be a block of an offset-0 call: blocks count from sample_offset."""
    upload(gpu, monkeypatch, R.scene("scene0"))
    points = points_of(gpu, "scene0")[:5]
    for off in (0, 40):
        want, seg, shadow = referee(gpu, points, spp, 6, sample_offset=off, key_offset=9)
        st = abi.Stats()
        got = gpu.probe_sh(points, spp, 6, sample_offset=off, key_offset=9, stats=st)
        assert same(got, want), first_difference(got, want)
        assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, 5 * spp)
        assert spp < 16 or (got[:, 0, :3] != 0).any()


# ---------------------------------------------------------------- 3. independence at scale
def test_a_point_does_not_depend_on_its_batch(gpu, monkeypatch):
    """n = 2^16 + 3 points: more units than a launch's first wave of jobs. Scattered points equal one-point calls with their own keys;
    at spp 144 the same through the unit slab and the resolve."""
    upload(gpu, monkeypatch, R.scene("scene0"))
    n = (1 << 16) + 3
    base = P.scene_probes(gpu.cast, R.scene("scene0"), 4096, seed=7)
    points = np.tile(base, ((n + 4095) // 4096, 1))[:n].copy()
    ends = np.array([0, 1, 63, 64, n - 2, n - 1])
    pick = np.concatenate([ends, np.setdiff1d(np.random.default_rng(3).choice(n, 30, replace=False), ends)[:18]])
    d_points = torch.from_numpy(points).cuda()
    for spp in (16, 144):
        st = abi.Stats()
        big = gpu.probe_sh(points, spp, 4, stats=st)
        assert st.samples == n * spp and not big[..., 3].any()
        assert (big[:, 0, 0] > 0).mean() > 0.2 and len(np.unique(big[:, 1, 0])) > 1000
        for j in pick:
            one = gpu.probe_sh(points[j:j + 1], spp, 4, key_offset=int(j))
            assert same(one, big[j:j + 1]), (spp, j, one, big[j])
        assert same(probe_sh_torch(gpu, d_points, spp, 4).cpu().numpy(), big)


# ---------------------------------------------------------------- 4. chunks and slab ranges
def test_chunks_and_slab_ranges_do_not_change_the_bits(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene1"))
    points = points_of(gpu, "scene1")
    d_points = torch.from_numpy(points).cuda()
    for spp in (8, 272):
        for k in ("RTW_RADIANCE_CHUNK", "RTW_RADIANCE_SLAB_BYTES"):
            monkeypatch.delenv(k, raising=False)
        s0, s1, s2 = abi.Stats(), abi.Stats(), abi.Stats()
        whole = gpu.probe_sh(points, spp, 6, key_offset=123, stats=s0)
        monkeypatch.setenv("RTW_RADIANCE_CHUNK", "2")
        assert same(gpu.probe_sh(points, spp, 6, key_offset=123, stats=s1), whole)
        monkeypatch.delenv("RTW_RADIANCE_CHUNK")
        monkeypatch.setenv("RTW_RADIANCE_SLAB_BYTES", str(40 * 3 * 144))  # 40 points of three units: ranges of 40, 40 and 16 at spp 272
        assert same(gpu.probe_sh(points, spp, 6, key_offset=123, stats=s2), whole)
        assert same(probe_sh_torch(gpu, d_points, spp, 6, key_offset=123).cpu().numpy(), whole)
        for s in (s1, s2):
            assert (s.segments, s.shadow_rays, s.samples) == (s0.segments, s0.shadow_rays, s0.samples)
        assert (whole[:, 0, 0] > 0).mean() > 0.5 and len(np.unique(whole[:, 1, 0])) > 3


# ---------------------------------------------------------------- 5. keys wrap
@pytest.mark.parametrize("rng_kind", BOTH)
def test_keys_wrap_modulo_2_to_the_32(gpu, monkeypatch, rng_kind):
    upload(gpu, monkeypatch, R.scene("scene0"))
    points = points_of(gpu, "scene0")[:8]
    k0 = 2 ** 32 - 3
    want, seg, shadow = referee(gpu, points, 16, 6, rng_kind, key_offset=k0)
    st = abi.Stats()
    got = gpu.probe_sh(points, 16, 6, rng_kind=rng_kind, key_offset=k0, stats=st)
    assert same(got, want), first_difference(got, want)
    assert (st.segments, st.shadow_rays) == (seg, shadow)
    assert same(gpu.probe_sh(points[3:], 16, 6, rng_kind=rng_kind, key_offset=0), got[3:]) and (got[:, 0, :3] != 0).any()
    monkeypatch.setenv("RTW_RADIANCE_CHUNK", "3")  # a chunk that ends on the wrap and one that starts on it
    assert same(gpu.probe_sh(points, 16, 6, rng_kind=rng_kind, key_offset=k0), want)
    monkeypatch.setenv("RTW_RADIANCE_CHUNK", "2")
    assert same(gpu.probe_sh(points, 16, 6, rng_kind=rng_kind, key_offset=k0), want)


# ---------------------------------------------------------------- 6. floats 3..5 are not used
def test_floats_3_to_5_change_nothing(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene0"))
    points = points_of(gpu, "scene0")
    want = gpu.probe_sh(points, SPP, DEPTH, key_offset=KEY)
    for fill in (np.nan, 0.0, np.inf, -3.0):
        other = points.copy()
        other[:, 3:6] = fill
        assert same(gpu.probe_sh(other, SPP, DEPTH, key_offset=KEY), want), fill
        assert same(probe_sh_torch(gpu, torch.from_numpy(other).cuda(), SPP, DEPTH, key_offset=KEY).cpu().numpy(), want), fill
    assert same(gpu.probe_sh(bake.probe_grid(points[0, :3], points[0, :3], 1, 1, 1), SPP, DEPTH, key_offset=KEY), want[:1])


# ---------------------------------------------------------------- 7. the analytic sky
def test_the_sky_above_scene_1(gpu, monkeypatch):
    """Every first segment ends in the sky: L = (1 - t) + t (0.5, 0.7, 1) with t = (y + 1) / 2, that is a + b y with a = (0.75, 0.85, 1)
    and b = (-0.25, -0.15, 0). Its coefficients are c_0 = 2 sqrt(pi) a, c_y = 0.4886025 (4 pi / 3) b and 0 elsewhere; its irradiance
    at the normal +y is pi (7/12, 3/4, 1), the value test_gpu_probe.py pins for the same sky."""
    blob = R.scene("scene1")
    assert abi.parse_scene(blob)["header"].sky_light == 1
    upload(gpu, monkeypatch, blob)
    n, spp = 64, 256
    up = np.zeros((n, 8), np.float32)
    up[:, 0], up[:, 2] = np.arange(n) - 32.0, np.arange(n) % 7
    up[:, 1], up[:, 6], up[:, 7] = 50.0, 1e-6, 1e-3
    st = abi.Stats()
    c = gpu.probe_sh(up, spp, 1, stats=st)
    assert (st.segments, st.shadow_rays, st.samples) == (n * spp, 0, n * spp)
    mean = c[:, :, :3].astype(np.float64).mean(0)  # (9, 3)
    a, b = np.array([0.75, 0.85, 1.0]), np.array([-0.25, -0.15, 0.0])
    expected = np.zeros((9, 3))
    expected[0], expected[1] = 2.0 * np.sqrt(np.pi) * a, 0.4886025 * (4.0 * np.pi / 3.0) * b
    # the standard errors, in float64, from the very directions the kernel draws: the sky along the normalised direction
    d = S.directions(n, spp).astype(np.float64).reshape(-1, 3)
    unit = d / np.linalg.norm(d, axis=1, keepdims=True)
    lum = a + b * unit[:, 1:2]  # (n * spp, 3)
    val = 4.0 * np.pi * S.basis(d.astype(np.float32)).astype(np.float64)[:, :, None] * lum[:, None, :]  # (n * spp, 9, 3)
    se = np.maximum(val.std(0, ddof=1) / np.sqrt(n * spp), 1e-5)
    print("coefficients:\n", mean, "\nexpected:\n", expected, "\ndistance in standard errors:\n", np.abs(mean - expected) / se)
    assert (np.abs(mean - expected) <= 6.0 * se).all()
    # the irradiance the mean coefficients give at +y, over pi
    up_n = np.array([0, 1, 0], np.float32)
    e = bake.sh_irradiance(mean, up_n) / np.pi
    weights = bake.sh_basis(up_n).astype(np.float64) * np.array([np.pi] + [2 * np.pi / 3] * 3 + [np.pi / 4] * 5) / np.pi
    e_se = np.maximum((val * weights[None, :, None]).sum(1).std(0, ddof=1) / np.sqrt(n * spp), 1e-5)
    print("sh irradiance / pi at +y:", e, "expected", (7 / 12, 3 / 4, 1.0), "standard errors", e_se)
    assert (np.abs(e - np.array([7 / 12, 3 / 4, 1.0])) <= 6.0 * e_se).all()


# ---------------------------------------------------------------- 8. the device path
def test_probe_sh_torch_equals_probe_sh_and_is_ordered_on_the_current_stream(gpu, monkeypatch):
    name = "random_volumes_motion"
    upload(gpu, monkeypatch, R.scene(name))
    points = points_of(gpu, name)
    d_points = torch.from_numpy(points).cuda()
    s0, st = abi.Stats(), abi.Stats()
    want = gpu.probe_sh(points, SPP, DEPTH, key_offset=KEY, stats=s0)
    got = probe_sh_torch(gpu, d_points, SPP, DEPTH, key_offset=KEY, stats=st)
    assert got.is_cuda and tuple(got.shape) == (N, 9, 4) and same(got.cpu().numpy(), want) and want[:, 0, :3].sum() > 0
    assert (st.segments, st.shadow_rays, st.samples) == (s0.segments, s0.shadow_rays, N * SPP) and st.seconds > 0.0
    check_stream_order(lambda t: probe_sh_torch(gpu, t, SPP, DEPTH, key_offset=KEY), d_points, lambda got: same(got.cpu().numpy(), want))
    assert tuple(probe_sh_torch(gpu, torch.zeros((0, 8), device="cuda:0"), 4, 4).shape) == (0, 9, 4)
    with pytest.raises(ValueError):
        probe_sh_torch(gpu, d_points, 0, DEPTH)


# ---------------------------------------------------------------- 9. refusals
def test_every_refusal_leaves_the_context_usable_and_writes_nothing(gpu, monkeypatch):
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    points = points_of(gpu, "scene0").copy()
    want = gpu.probe_sh(points, SPP, DEPTH, key_offset=KEY)
    lib, n = gpu.lib, N
    out = np.full((n, 9, 4), -7, np.float32)
    d_points = torch.from_numpy(np.concatenate([points.ravel(), np.zeros(8, np.float32)])).cuda()
    d_out = torch.full((n * 36 + 8,), -7.0, device="cuda:0")
    R_, O_, D_, DO_ = points.ctypes.data, out.ctypes.data, d_points.data_ptr(), d_out.data_ptr()

    def rp(**kw):
        p = abi.make_radiance_params(SPP, DEPTH, key_offset=KEY)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)
    fresh = abi.Renderer(0)
    try:
        assert lib.rtw_probe_sh(fresh.ctx, R_, n, rp(), O_, None) == -3        # RTW_ERR_NO_SCENE
        assert lib.rtw_probe_sh_device(fresh.ctx, D_, n, rp(), DO_, None, None) == -3
        assert b"rtw_upload_scene" in lib.rtw_last_error(fresh.ctx)
    finally:
        fresh.close()

    def still_fine():
        assert same(gpu.probe_sh(points, SPP, DEPTH, key_offset=KEY), want)
    bad_params = [None, rp(spp=0), rp(spp=-1), rp(max_depth=-1), rp(rng_kind=2), rp(rng_kind=-1), rp(estimator=4), rp(estimator=-1),
                  rp(sample_offset=-1), rp(sample_offset=2 ** 31 - SPP), rp(spp=2 ** 31 - 1, sample_offset=1), rp(reserved=1), rp(reserved=2 ** 31)]
    refusals = [(R_, n, p, O_) for p in bad_params] + [(R_, 1 << 31, rp(), O_), (None, n, rp(), O_), (R_, n, rp(), None)]
    for r_, m, p, o_ in refusals:
        st = sentinel_stats()
        assert lib.rtw_probe_sh(gpu.ctx, r_, m, p, o_, C.byref(st)) == -1
        assert lib.rtw_last_error(gpu.ctx) and left_alone(st)  # a refused call leaves *stats alone
    still_fine()
    dev_refusals = [(D_, n, p, DO_) for p in bad_params] + [(D_, 1 << 31, rp(), DO_), (None, n, rp(), DO_), (D_, n, rp(), None),
                                                            (D_ + 4, n, rp(), DO_), (D_ + 8, n, rp(), DO_), (D_, n, rp(), DO_ + 4), (D_, n, rp(), DO_ + 8)]
    for r_, m, p, o_ in dev_refusals:
        st = sentinel_stats()
        assert lib.rtw_probe_sh_device(gpu.ctx, r_, m, p, o_, None, C.byref(st)) == -1
        assert left_alone(st)
    still_fine()  # after a misaligned pointer as after any other refusal: the next call works
    torch.cuda.synchronize()
    assert (out == -7).all() and bool((d_out == -7).all().item())  # no refused call wrote anything
    # n = 0 is fine and launches nothing, whatever the pointers
    st = abi.Stats(segments=77)
    assert lib.rtw_probe_sh(gpu.ctx, None, 0, rp(), None, C.byref(st)) == 0 and (st.segments, st.samples, st.seconds) == (0, 0, 0.0)
    assert lib.rtw_probe_sh_device(gpu.ctx, None, 0, rp(), None, None, None) == 0
    assert lib.rtw_probe_sh_device(gpu.ctx, D_ + 4, 0, rp(), DO_ + 4, None, None) == 0
    assert gpu.probe_sh(np.zeros((0, 8), np.float32), 4, 4).shape == (0, 9, 4)
    torch.cuda.synchronize()
    assert bool((d_out == -7).all().item())
    assert lib.rtw_probe_sh_device(gpu.ctx, D_ + 32, n - 1, rp(key_offset=KEY + 1), DO_ + 16, None, None) == 0  # from point 1 on: aligned enough
    assert same(d_out[4:4 + 36 * (n - 1)].cpu().numpy().reshape(-1, 9, 4), want[1:])
    assert bool((d_out[:4] == -7).all().item()) and bool((d_out[4 + 36 * (n - 1):] == -7).all().item())  # and nothing beside them
    zero = gpu.probe_sh(points, SPP, 0)  # max_depth = 0: zeros, w included
    assert same(zero, np.zeros((n, 9, 4), np.float32)) and same(gpu.probe_sh(points, 200, 0), zero)


# ---------------------------------------------------------------- 10. neighbours
def test_a_group_answers_on_its_first_device_with_single_device_bits(gpu, monkeypatch):
    blob = R.scene("scene1")
    upload(gpu, monkeypatch, blob)
    points = points_of(gpu, "scene1")
    group = abi.Renderer([0, 0])
    try:
        out = np.zeros((N, 9, 4), np.float32)
        p0 = abi.make_radiance_params(SPP, DEPTH)
        assert group.lib.rtw_probe_sh(group.ctx, points.ctypes.data, N, C.byref(p0), out.ctypes.data, None) == -3
        group.upload_scene(blob)
        for spp in (SPP, 144):
            s0, s1 = abi.Stats(), abi.Stats()
            want = gpu.probe_sh(points, spp, DEPTH, key_offset=KEY, stats=s0)
            assert same(group.probe_sh(points, spp, DEPTH, key_offset=KEY, stats=s1), want)
            assert (s1.segments, s1.shadow_rays) == (s0.segments, s0.shadow_rays)
            assert same(probe_sh_torch(group, torch.from_numpy(points).cuda(), spp, DEPTH, key_offset=KEY).cpu().numpy(), want)
    finally:
        group.close()


def test_an_open_accumulation_session_goes_on_bit_exactly(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene0"))
    points = points_of(gpu, "scene0")
    want = gpu.probe_sh(points, SPP, DEPTH, key_offset=KEY)
    p = abi.make_params(32, 32, 32, 6)
    one_shot, _ = gpu.render(p)
    gpu.accum_begin(p)
    try:
        gpu.accum_add(16)
        assert same(gpu.probe_sh(points, SPP, DEPTH, key_offset=KEY), want)
        assert same(probe_sh_torch(gpu, torch.from_numpy(points).cuda(), SPP, DEPTH, key_offset=KEY).cpu().numpy(), want)
        gpu.probe_sh(points, 144, 4)  # the unit slab and the resolve
        gpu.accum_add(16)
        assert same(gpu.accum_read(), one_shot)
        assert gpu.accum_status().done == 32
    finally:
        gpu.accum_end()
    assert same(gpu.probe_sh(points, SPP, DEPTH, key_offset=KEY), want)


def test_render_probe_radiance_and_cast_are_what_they_were_before_probe_sh_calls(gpu, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for g in map(golden, GOLDEN_PAIR):
        blob, rng, seed = g.blob, g.rng, g.seed
        gpu.upload_scene(blob)
        rays, _, _ = G.scene_rays(blob, 5, 300)
        rays[:, 6], rays[:, 7] = 1e-6, 1e27
        rad = gpu.radiance(rays, 24, 6, rng_kind=rng)
        hits = gpu.cast(rays)
        probes = P.scene_probes(gpu.cast, blob, 300, tmax=100.0)
        irr = gpu.probe(probes, 160, 3, rng_kind=rng)
        occ = gpu.probe(probes, 160, 3, rng_kind=rng, mode="occlusion")
        a = gpu.probe_sh(probes, 24, 6, rng_kind=rng)
        b = gpu.probe_sh(probes, 160, 3, rng_kind=rng, estimator=1)  # the slab rtw_probe's resolves read as well
        assert np.isfinite(a).all() and np.isfinite(b).all() and a[:, 0, :3].sum() > 0 and b[:, 0, :3].sum() > 0
        check_golden_render(gpu, g)
        assert same(gpu.radiance(rays, 24, 6, rng_kind=rng), rad) and same(gpu.probe_sh(probes, 24, 6, rng_kind=rng), a)
        assert same(gpu.probe(probes, 160, 3, rng_kind=rng), irr) and same(gpu.probe(probes, 160, 3, rng_kind=rng, mode="occlusion"), occ)
        again = gpu.cast(rays)
        assert all(np.array_equal(hits[k].view(np.uint32), again[k].view(np.uint32)) for k in hits)
