"""GPU suite of the probes (include/rtw.h rtw_probe / rtw_probe_device). The referee is the contract itself: sample s of probe i is
the rtw_radiance sample (irradiance) or the RTW_CAST_ANY query (occlusion) of ray (p_i, d_is, tmin, tmax), with d_is restated by
probe_ref.directions - and rtw_radiance and rtw_cast are refereed by the oracle in their own suites. Then the summation units and
offsets, independence of the batch, chunks and slab ranges, keys that wrap, analytic values, the torch path, every refusal, groups,
sessions, rtw_render afterwards, and the lightmap baker."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # (before the HIP library is loaded, as in a run of the whole suite)

import geometry_ref as G
import gpu_common
import probe_ref as P
import radiance_ref as R
from gpu_common import (BOTH, GOLDEN_PAIR, KNOBS, UPLOADS, check_golden_render, check_stream_order,  # noqa: F401
                        golden, gpu, left_alone, same, sentinel_stats, upload)
from raytracing_weekend_amd import abi, bake
from raytracing_weekend_amd.torch_probe import probe_torch

pytestmark = pytest.mark.gpu
first_difference = functools.partial(gpu_common.first_difference, what="probes")

SCENES = ("scene0", "scene1", "scene3", "random_volumes_motion")
# occlusion distances of the scenes' sizes: a good part of the probes is then neither open nor closed
TMAX = {"scene0": 150.0, "scene1": 3.0, "scene3": 150.0, "random_volumes_motion": 70.0}
N, SPP, DEPTH, KEY = R.N, R.SPP, R.DEPTH, R.KEY  # 96 probes (one and a half waves), 48 spp (three blocks), depth 8, key offset 5
PI = np.float32(np.pi)
assert PI == np.float32(3.14159265)


_probes = {}


def probes_of(gpu, name):
    """The batch of a scene: N probes from gpu.cast hits (the scene must be uploaded); made once (rtw_cast's bits do not depend on
    how the scene was uploaded)."""
    if name not in _probes:
        _probes[name] = P.scene_probes(gpu.cast, R.scene(name), N)
    return _probes[name]


@functools.lru_cache(maxsize=None)
def _directions(key, spp, rng_kind, sample_offset, key_offset):
    return P.directions(_dir_src[key], spp, rng_kind=rng_kind, sample_offset=sample_offset, key_offset=key_offset)


_dir_src = {}


def directions(probes, spp, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, key_offset=0):
    key = probes[:, 3:6].tobytes()
    _dir_src[key] = probes
    return _directions(key, spp, rng_kind, sample_offset, key_offset)


def irradiance_referee(gpu, probes, spp, depth, rng_kind=abi.RTW_RNG_PHILOX, estimator=0, sample_offset=0, key_offset=0):
    """(expected (n, 4), segments, shadow rays): one rtw_radiance call per sample index on the rays (p_i, d_is), the samples summed in
    the library's order, the mean times pi."""
    d = directions(probes, spp, rng_kind, sample_offset, key_offset)
    smp = np.empty((spp, len(probes), 4), np.float32)
    seg = shadow = 0
    for s in range(spp):
        st = abi.Stats()
        smp[s] = gpu.radiance(P.rays_of(probes, d, s), 1, depth, rng_kind=rng_kind, estimator=estimator, sample_offset=sample_offset + s,
                              key_offset=key_offset, stats=st)
        seg, shadow = seg + st.segments, shadow + st.shadow_rays
    want = np.ones((len(probes), 4), np.float32)
    for i in range(len(probes)):
        want[i, :3] = R.sum_in_order(smp[:, i, :3], spp) * PI
    return want, seg, shadow


def occlusion_referee(gpu, probes, spp, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, key_offset=0):
    """(expected (n, 4), the unoccluded counts): one RTW_CAST_ANY call per sample index."""
    d = directions(probes, spp, rng_kind, sample_offset, key_offset)
    open_ = np.zeros(len(probes), np.int64)
    for s in range(spp):
        open_ += gpu.cast(P.rays_of(probes, d, s), mode="any", want=("prim",))["prim"] < 0
    want = np.ones((len(probes), 4), np.float32)
    want[:, :3] = (open_.astype(np.float32) / np.float32(spp))[:, None]
    return want, open_


# ---------------------------------------------------------------- 1. irradiance equals rtw_radiance, sample for sample
def check_irradiance(gpu, name, rng_kind, estimator=0):
    probes = probes_of(gpu, name)
    want, seg, shadow = irradiance_referee(gpu, probes, SPP, DEPTH, rng_kind, estimator, key_offset=KEY)
    st = abi.Stats()
    got = gpu.probe(probes, SPP, DEPTH, rng_kind=rng_kind, estimator=estimator, key_offset=KEY, stats=st)
    lit = int((want[:, :3].sum(1) > 0).sum())
    print(f"{name} rng {rng_kind} estimator {estimator}: segments {st.segments} (referee {seg}), shadow rays {st.shadow_rays} ({shadow}), {lit} of {N} probes lit")
    assert got.shape == (N, 4) and same(got, want), first_difference(got, want)
    assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, N * SPP)
    assert st.algorithmic_bytes == 128 * st.segments + 32 * st.samples and st.seconds > 0.0
    assert not any(st.kernel_seconds) and not any(st.kernel_launches) and not any(st.kernel_segments)
    # not vacuous: enough probes see light, and the directions matter (the radiance along the normals is something else)
    assert lit >= N // 4
    along = gpu.radiance(probes, SPP, DEPTH, rng_kind=rng_kind, estimator=estimator, key_offset=KEY)
    assert not same(along[:, :3] * PI, got[:, :3])


@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("how", list(UPLOADS))
@pytest.mark.parametrize("name", SCENES)
def test_irradiance_is_rtw_radiance_sample_for_sample(gpu, monkeypatch, name, how, rng_kind):
    upload(gpu, monkeypatch, R.scene(name), how)
    check_irradiance(gpu, name, rng_kind)


@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("estimator", [1, 2, 3])
@pytest.mark.parametrize("how", list(UPLOADS))
def test_irradiance_under_the_corrected_estimators_on_scene_0(gpu, monkeypatch, how, estimator, rng_kind):
    upload(gpu, monkeypatch, R.scene("scene0"), how)
    check_irradiance(gpu, "scene0", rng_kind, estimator)


# ---------------------------------------------------------------- 2. occlusion equals rtw_cast
@pytest.mark.parametrize("rng_kind", BOTH)
@pytest.mark.parametrize("how", list(UPLOADS))
@pytest.mark.parametrize("name", SCENES)
def test_occlusion_is_rtw_cast_any_sample_for_sample(gpu, monkeypatch, name, how, rng_kind):
    upload(gpu, monkeypatch, R.scene(name), how)
    probes = probes_of(gpu, name).copy()
    probes[:, 7] = TMAX[name]
    want, open_ = occlusion_referee(gpu, probes, SPP, rng_kind, key_offset=KEY)
    st = abi.Stats(segments=9)
    got = gpu.probe(probes, SPP, DEPTH, rng_kind=rng_kind, key_offset=KEY, mode="occlusion", stats=st)
    partial = int(((open_ > 0) & (open_ < SPP)).sum())
    print(f"{name} rng {rng_kind}: {partial} of {N} probes partly occluded, {int((open_ == SPP).sum())} open, {int((open_ == 0).sum())} closed")
    assert same(got, want), first_difference(got, want)
    assert (st.segments, st.shadow_rays, st.samples) == (0, N * SPP, N * SPP) and st.seconds > 0.0
    assert partial >= N // 8
    # max_depth and estimator are unused
    assert same(gpu.probe(probes, SPP, 0, rng_kind=rng_kind, key_offset=KEY, estimator=2, mode="occlusion"), want)


# ---------------------------------------------------------------- 3. units, tails, offsets
def lit_probe(gpu):
    probes = probes_of(gpu, "scene0")
    e = gpu.probe(probes, SPP, DEPTH, key_offset=KEY)
    return probes[int(np.argmax(e[:, :3].sum(1)))][None].copy()


def test_units_tails_and_sample_offsets(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene0"))
    one = lit_probe(gpu)
    probes = np.repeat(one, 80, 0)
    for spp, off in ((272, 0), (16, 16)):  # two units and a 16-sample tail; one block that starts at sample 16
        want, seg, shadow = irradiance_referee(gpu, probes, spp, 6, sample_offset=off, key_offset=9)
        st = abi.Stats()
        got = gpu.probe(probes, spp, 6, sample_offset=off, key_offset=9, stats=st)
        assert same(got, want), first_difference(got, want)
        assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, 80 * spp)
        assert len(np.unique(got.view(np.uint32), axis=0)) > 40 and got[:, :3].sum() > 0  # one probe, eighty streams
    # the same samples reached two ways: samples 16 ... 31 are the second block of a 32-spp call (sums recovered exactly: x16, /32)
    first = gpu.probe(one, 16, 6, key_offset=9)
    second = gpu.probe(one, 16, 6, key_offset=9, sample_offset=16)
    both = gpu.probe(one, 32, 6, key_offset=9)
    d32 = directions(one, 32, key_offset=9)
    halves = []
    for off in (0, 16):
        smp = np.stack([gpu.radiance(P.rays_of(one, d32, off + s), 1, 6, key_offset=9, sample_offset=off + s)[0, :3] for s in range(16)])
        halves.append(R.sum_in_order(smp, 16) * np.float32(16))
    assert same(first[0, :3], (halves[0] / np.float32(16)) * PI) and same(second[0, :3], (halves[1] / np.float32(16)) * PI)
    assert same(both[0, :3], ((halves[0] + halves[1]) / np.float32(32)) * PI)
    three = probes_of(gpu, "scene0")[:3]
    for spp in (1, 129):
        want, seg, shadow = irradiance_referee(gpu, three, spp, 8, rng_kind=abi.RTW_RNG_TEA_LCG, key_offset=1000)
        st = abi.Stats()
        got = gpu.probe(three, spp, 8, rng_kind=abi.RTW_RNG_TEA_LCG, key_offset=1000, stats=st)
        assert same(got, want), first_difference(got, want)
        assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, 3 * spp)
    occ = probes_of(gpu, "scene0")[:40].copy()
    occ[:, 7] = TMAX["scene0"]
    for spp, rng_kind in ((272, abi.RTW_RNG_PHILOX), (129, abi.RTW_RNG_TEA_LCG)):
        want, open_ = occlusion_referee(gpu, occ, spp, rng_kind, key_offset=77)
        st = abi.Stats()
        got = gpu.probe(occ, spp, 4, rng_kind=rng_kind, key_offset=77, mode="occlusion", stats=st)
        assert same(got, want), first_difference(got, want)
        assert (st.segments, st.shadow_rays, st.samples) == (0, 40 * spp, 40 * spp) and ((open_ > 0) & (open_ < spp)).any()


# ---------------------------------------------------------------- 4. independence at scale
def big_batch(gpu, n):
    base = P.scene_probes(gpu.cast, R.scene("scene0"), 4096, tmax=TMAX["scene0"], seed=7)
    return np.tile(base, ((n + 4095) // 4096, 1))[:n].copy()


def test_a_probe_does_not_depend_on_its_batch(gpu, monkeypatch):
    """n = 2^19 + 3 probes: more units than the device holds lanes, so the queue hands out jobs to the end (and the occlusion lanes
    stride). 65 scattered probes equal one-probe calls with their own keys; at spp 144 the same through the unit slab and the resolves."""
    upload(gpu, monkeypatch, R.scene("scene0"))
    n = (1 << 19) + 3
    probes = big_batch(gpu, n)
    ends = np.array([0, 1, 63, 64, n - 2, n - 1])
    pick = np.concatenate([ends, np.setdiff1d(np.random.default_rng(3).choice(n, 80, replace=False), ends)[:59]])
    assert len(np.unique(pick)) == 65
    d_probes = torch.from_numpy(probes).cuda()
    for mode in ("irradiance", "occlusion"):
        for spp in (16, 144):
            st = abi.Stats()
            big = gpu.probe(probes, spp, 4, key_offset=0, mode=mode, stats=st)
            assert st.samples == n * spp and (big[:, 3] == 1.0).all()
            assert (big[:, 0] > 0).mean() > 0.2 and len(np.unique(big[:, 0])) > 3
            for j in pick:
                one = gpu.probe(probes[j:j + 1], spp, 4, key_offset=int(j), mode=mode)
                assert same(one, big[j:j + 1]), (mode, spp, j, one, big[j])
        assert same(probe_torch(gpu, d_probes, 144, 4, mode=mode).cpu().numpy(), big)


# ---------------------------------------------------------------- 5. chunks and slab ranges
def test_chunks_and_slab_ranges_do_not_change_the_bits(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene1"))
    base = P.scene_probes(gpu.cast, R.scene("scene1"), 512, tmax=TMAX["scene1"], seed=11)
    probes = np.tile(base, (10, 1))[:5003].copy()
    d_probes = torch.from_numpy(probes).cuda()
    for mode in ("irradiance", "occlusion"):
        for spp in (8, 144):
            for k in ("RTW_RADIANCE_CHUNK", "RTW_RADIANCE_SLAB_BYTES"):
                monkeypatch.delenv(k, raising=False)
            s0, s1, s2 = abi.Stats(), abi.Stats(), abi.Stats()
            kw = dict(key_offset=123, mode=mode)
            whole = gpu.probe(probes, spp, 6, stats=s0, **kw)
            monkeypatch.setenv("RTW_RADIANCE_CHUNK", "1000")
            assert same(gpu.probe(probes, spp, 6, stats=s1, **kw), whole)
            monkeypatch.delenv("RTW_RADIANCE_CHUNK")
            monkeypatch.setenv("RTW_RADIANCE_SLAB_BYTES", str(700 * 2 * 16))  # 700 probes of two units: eight ranges at spp 144
            assert same(gpu.probe(probes, spp, 6, stats=s2, **kw), whole)
            assert same(probe_torch(gpu, d_probes, spp, 6, **kw).cpu().numpy(), whole)
            for s in (s1, s2):
                assert (s.segments, s.shadow_rays, s.samples) == (s0.segments, s0.shadow_rays, s0.samples)
            assert (whole[:, 0] > 0).mean() > 0.5 and len(np.unique(whole[:, 0])) > 3


# ---------------------------------------------------------------- 6. keys wrap
@pytest.mark.parametrize("rng_kind", BOTH)
def test_keys_wrap_modulo_2_to_the_32(gpu, monkeypatch, rng_kind):
    upload(gpu, monkeypatch, R.scene("scene0"))
    all_ = probes_of(gpu, "scene0")
    e = gpu.probe(all_, SPP, DEPTH, key_offset=KEY)
    probes = all_[np.argsort(-e[:, :3].sum(1))[:8]].copy()
    k0 = 2 ** 32 - 3
    want, _, _ = irradiance_referee(gpu, probes, 16, 6, rng_kind, key_offset=k0)
    got = gpu.probe(probes, 16, 6, rng_kind=rng_kind, key_offset=k0)
    assert same(got, want), first_difference(got, want)
    assert same(gpu.probe(probes[3:], 16, 6, rng_kind=rng_kind, key_offset=0), got[3:]) and got[:, :3].sum() > 0
    occ = probes.copy()
    occ[:, 7] = TMAX["scene0"]
    want_o, _ = occlusion_referee(gpu, occ, 16, rng_kind, key_offset=k0)
    monkeypatch.setenv("RTW_RADIANCE_CHUNK", "3")  # a chunk that ends on the wrap and one that starts on it
    assert same(gpu.probe(probes, 16, 6, rng_kind=rng_kind, key_offset=k0), want)
    assert same(gpu.probe(occ, 16, 6, rng_kind=rng_kind, key_offset=k0, mode="occlusion"), want_o)
    monkeypatch.setenv("RTW_RADIANCE_CHUNK", "2")
    assert same(gpu.probe(probes, 16, 6, rng_kind=rng_kind, key_offset=k0), want)


# ---------------------------------------------------------------- 7. analytic pins
def test_the_sky_above_scene_1_and_the_floor_of_scene_0(gpu, monkeypatch):
    blob = R.scene("scene1")
    assert abi.parse_scene(blob)["header"].sky_light == 1
    upload(gpu, monkeypatch, blob)
    up = np.zeros((64, 8), np.float32)
    up[:, 0], up[:, 2] = np.arange(64) - 32.0, np.arange(64) % 7
    up[:, 1], up[:, 4], up[:, 6], up[:, 7] = 50.0, 1.0, 1e-6, 1e27
    st = abi.Stats()
    e = gpu.probe(up, 256, 1, stats=st)
    # every first segment misses: radiance = (1 - t) + t * (0.5, 0.7, 1) with t = (y + 1) / 2; E[y] = 2/3 under cos / pi, Var[y] = 1/18,
    # so the mean over 64 * 256 samples is (7/12, 3/4, 1) with standard errors (4.6e-4, 2.8e-4, 0): the bounds are six of them
    mean = e[:, :3].astype(np.float64).mean(0) / np.pi
    print("sky irradiance / pi:", mean, "expected", (7 / 12, 3 / 4, 1.0))
    assert (st.segments, st.shadow_rays) == (64 * 256, 0)
    assert np.all(np.abs(mean - np.array([7 / 12, 3 / 4, 1.0])) <= np.array([2.8e-3, 1.7e-3, 1e-5]))
    assert same(gpu.probe(up, 256, 1, mode="occlusion"), np.ones((64, 4), np.float32))
    # scene 0: a floor point with nothing within 20 units but the floor
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    prims = abi.parse_scene(blob)["prims"]
    floor = next(i for i, p in enumerate(prims) if p.type == abi.PRIM_RECT_Y and p.p[4] == 0.0 and p.xform == 0)
    point = np.array([100.0, 0.0, 60.0])
    dirs = np.random.default_rng(1).normal(size=(4096, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dirs[:, 1] = np.abs(dirs[:, 1]) + 1e-3  # the upper half space, from just above the floor
    rays = np.concatenate([np.tile(point + [0, 1e-3, 0], (4096, 1)), dirs, np.full((4096, 1), 1e-6), np.full((4096, 1), 25.0)], axis=1).astype(np.float32)
    assert (gpu.cast(rays, want=("prim",))["prim"] < 0).all()
    down = np.array([[100.0, 1.0, 60.0, 0, -1, 0, 1e-6, 1e27]], np.float32)
    assert gpu.cast(down, want=("prim",))["prim"][0] == floor
    for rng_kind in BOTH:
        above = np.array([[100.0, 1e-3, 60.0, 0, 1, 0, 1e-6, 20.0]], np.float32)
        assert same(gpu.probe(above, 256, 1, rng_kind=rng_kind, mode="occlusion"), np.ones((1, 4), np.float32))
        below = np.array([[100.0, 1e-3, 60.0, 0, -1, 0, 1e-6, 20.0]], np.float32)
        assert same(gpu.probe(below, 256, 1, rng_kind=rng_kind, mode="occlusion"), np.array([[0, 0, 0, 1]], np.float32))


# ---------------------------------------------------------------- 8. the device path
def test_probe_torch_equals_probe_and_is_ordered_on_the_current_stream(gpu, monkeypatch):
    name = "random_volumes_motion"
    upload(gpu, monkeypatch, R.scene(name))
    probes = probes_of(gpu, name).copy()
    probes[:, 7] = TMAX[name]
    d_probes = torch.from_numpy(probes).cuda()
    for mode in ("irradiance", "occlusion"):
        kw = dict(key_offset=KEY, mode=mode)
        s0, st = abi.Stats(), abi.Stats()
        want = gpu.probe(probes, SPP, DEPTH, stats=s0, **kw)
        got = probe_torch(gpu, d_probes, SPP, DEPTH, stats=st, **kw)
        assert got.is_cuda and tuple(got.shape) == (N, 4) and same(got.cpu().numpy(), want) and want[:, :3].sum() > 0
        assert (st.segments, st.shadow_rays, st.samples) == (s0.segments, s0.shadow_rays, N * SPP) and st.seconds > 0.0
        check_stream_order(lambda t: probe_torch(gpu, t, SPP, DEPTH, **kw), d_probes, lambda got: same(got.cpu().numpy(), want))
        assert tuple(probe_torch(gpu, torch.zeros((0, 8), device="cuda:0"), 4, 4, mode=mode).shape) == (0, 4)
    for spp, mode in ((0, "irradiance"), (4, "ao")):
        with pytest.raises(ValueError):
            probe_torch(gpu, d_probes, spp, DEPTH, mode=mode)


# ---------------------------------------------------------------- 9. refusals
def test_every_refusal_leaves_the_context_usable_and_writes_nothing(gpu, monkeypatch):
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    probes = probes_of(gpu, "scene0").copy()
    want = gpu.probe(probes, SPP, DEPTH, key_offset=KEY)
    lib, n = gpu.lib, N
    out = np.full((n, 4), -7, np.float32)
    d_probes = torch.from_numpy(np.concatenate([probes.ravel(), np.zeros(8, np.float32)])).cuda()
    d_out = torch.full((n * 4 + 8,), -7.0, device="cuda:0")
    R_, O_, D_, DO_ = probes.ctypes.data, out.ctypes.data, d_probes.data_ptr(), d_out.data_ptr()

    def pp(**kw):
        p = abi.make_probe_params(SPP, DEPTH, key_offset=KEY)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)
    fresh = abi.Renderer(0)
    try:
        assert lib.rtw_probe(fresh.ctx, R_, n, pp(), O_, None) == -3        # RTW_ERR_NO_SCENE
        assert lib.rtw_probe_device(fresh.ctx, D_, n, pp(), DO_, None, None) == -3
        assert b"rtw_upload_scene" in lib.rtw_last_error(fresh.ctx)
    finally:
        fresh.close()

    def still_fine():
        assert same(gpu.probe(probes, SPP, DEPTH, key_offset=KEY), want)
    bad_params = [None, pp(spp=0), pp(spp=-1), pp(max_depth=-1), pp(rng_kind=2), pp(rng_kind=-1), pp(estimator=4), pp(estimator=-1),
                  pp(sample_offset=-1), pp(sample_offset=2 ** 31 - SPP), pp(spp=2 ** 31 - 1, sample_offset=1), pp(mode=-1), pp(mode=2),
                  pp(mode=1, spp=0), pp(mode=1, estimator=4), pp(mode=1, max_depth=-1)]
    refusals = [(R_, n, p, O_) for p in bad_params] + [(R_, 1 << 31, pp(), O_), (None, n, pp(), O_), (R_, n, pp(), None), (R_, n, pp(mode=1), None)]
    for r_, m, p, o_ in refusals:
        st = sentinel_stats()
        assert lib.rtw_probe(gpu.ctx, r_, m, p, o_, C.byref(st)) == -1
        assert lib.rtw_last_error(gpu.ctx) and left_alone(st)  # a refused call leaves *stats alone
    still_fine()
    dev_refusals = [(D_, n, p, DO_) for p in bad_params] + [(D_, 1 << 31, pp(), DO_), (None, n, pp(), DO_), (D_, n, pp(), None),
                                                            (D_ + 4, n, pp(), DO_), (D_ + 8, n, pp(mode=1), DO_), (D_, n, pp(), DO_ + 4), (D_, n, pp(mode=1), DO_ + 8)]
    for r_, m, p, o_ in dev_refusals:
        st = sentinel_stats()
        assert lib.rtw_probe_device(gpu.ctx, r_, m, p, o_, None, C.byref(st)) == -1
        assert left_alone(st)
    still_fine()  # after a misaligned pointer as after any other refusal: the next call works
    torch.cuda.synchronize()
    assert (out == -7).all() and bool((d_out == -7).all().item())  # no refused call wrote anything
    # n = 0 is fine and launches nothing, whatever the pointers
    for mode in (0, 1):
        st = abi.Stats(segments=77)
        assert lib.rtw_probe(gpu.ctx, None, 0, pp(mode=mode), None, C.byref(st)) == 0 and (st.segments, st.samples, st.seconds) == (0, 0, 0.0)
        assert lib.rtw_probe_device(gpu.ctx, None, 0, pp(mode=mode), None, None, None) == 0
        assert lib.rtw_probe_device(gpu.ctx, D_ + 4, 0, pp(mode=mode), DO_ + 4, None, None) == 0
        assert gpu.probe(np.zeros((0, 8), np.float32), 4, 4, mode=("irradiance", "occlusion")[mode]).shape == (0, 4)
    assert lib.rtw_probe_device(gpu.ctx, D_ + 32, n - 1, pp(key_offset=KEY + 1), DO_ + 16, None, None) == 0  # from probe 1 on: aligned enough
    assert same(d_out[4:4 + 4 * (n - 1)].cpu().numpy().reshape(-1, 4), want[1:])
    zero = gpu.probe(probes, SPP, 0)
    assert same(zero, np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1))) and same(gpu.probe(probes, 200, 0), zero)


# ---------------------------------------------------------------- 10. neighbours
def test_a_group_answers_on_its_first_device_with_single_device_bits(gpu, monkeypatch):
    blob = R.scene("scene1")
    upload(gpu, monkeypatch, blob)
    probes = probes_of(gpu, "scene1").copy()
    probes[:, 7] = TMAX["scene1"]
    group = abi.Renderer([0, 0])
    try:
        out = np.zeros((N, 4), np.float32)
        p0 = abi.make_probe_params(SPP, DEPTH)
        assert group.lib.rtw_probe(group.ctx, probes.ctypes.data, N, C.byref(p0), out.ctypes.data, None) == -3
        group.upload_scene(blob)
        for mode in ("irradiance", "occlusion"):
            for spp in (SPP, 144):
                s0, s1 = abi.Stats(), abi.Stats()
                want = gpu.probe(probes, spp, DEPTH, key_offset=KEY, mode=mode, stats=s0)
                assert same(group.probe(probes, spp, DEPTH, key_offset=KEY, mode=mode, stats=s1), want)
                assert (s1.segments, s1.shadow_rays) == (s0.segments, s0.shadow_rays)
                assert same(probe_torch(group, torch.from_numpy(probes).cuda(), spp, DEPTH, key_offset=KEY, mode=mode).cpu().numpy(), want)
    finally:
        group.close()


def test_an_open_accumulation_session_goes_on_bit_exactly(gpu, monkeypatch):
    upload(gpu, monkeypatch, R.scene("scene0"))
    probes = probes_of(gpu, "scene0").copy()
    probes[:, 7] = TMAX["scene0"]
    want = {m: gpu.probe(probes, SPP, DEPTH, key_offset=KEY, mode=m) for m in ("irradiance", "occlusion")}
    p = abi.make_params(32, 32, 32, 6)
    one_shot, _ = gpu.render(p)
    gpu.accum_begin(p)
    try:
        gpu.accum_add(16)
        for m in want:
            assert same(gpu.probe(probes, SPP, DEPTH, key_offset=KEY, mode=m), want[m])
            assert same(probe_torch(gpu, torch.from_numpy(probes).cuda(), SPP, DEPTH, key_offset=KEY, mode=m).cpu().numpy(), want[m])
            gpu.probe(probes, 144, 4, mode=m)  # the unit slab and the resolves
        gpu.accum_add(16)
        assert same(gpu.accum_read(), one_shot)
        assert gpu.accum_status().done == 32
    finally:
        gpu.accum_end()
    for m in want:
        assert same(gpu.probe(probes, SPP, DEPTH, key_offset=KEY, mode=m), want[m])


def test_render_radiance_and_cast_are_what_they_were_before_probe_calls(gpu, monkeypatch):
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
        a = gpu.probe(probes, 24, 6, rng_kind=rng)
        b = gpu.probe(probes, 160, 3, rng_kind=rng, estimator=1)
        c = gpu.probe(probes, 160, 3, rng_kind=rng, mode="occlusion")
        assert np.isfinite(a).all() and np.isfinite(b).all() and a[:, :3].sum() > 0 and 0 < c[:, 0].mean() < 1
        check_golden_render(gpu, g)
        assert same(gpu.radiance(rays, 24, 6, rng_kind=rng), rad) and same(gpu.probe(probes, 24, 6, rng_kind=rng), a)
        again = gpu.cast(rays)
        assert all(np.array_equal(hits[k].view(np.uint32), again[k].view(np.uint32)) for k in hits)


# ---------------------------------------------------------------- 11. bake_rect
def test_bake_rect_on_the_cornell_floor(gpu, monkeypatch):
    blob = R.scene("scene0")
    upload(gpu, monkeypatch, blob)
    prims = abi.parse_scene(blob)["prims"]
    floor = next(i for i, p in enumerate(prims) if p.type == abi.PRIM_RECT_Y and p.p[4] == 0.0 and p.xform == 0)
    nu = nv = 16
    probes = bake.rect_probes(blob, floor, nu, nv)
    m = bake.bake_rect(gpu, blob, floor, nu, nv, 32, 6, key_offset=3)
    assert m.shape == (nv, nu, 4) and same(m, gpu.probe(probes, 32, 6, key_offset=3).reshape(nv, nu, 4)) and (m[..., :3].sum(-1) > 0).mean() > 0.5
    ao = bake.bake_rect(gpu, blob, floor, nu, nv, 32, 6, mode="occlusion")  # (the box is open towards the camera: neither 0 nor 1)
    assert same(ao, gpu.probe(probes, 32, 6, mode="occlusion").reshape(nv, nu, 4)) and 0.0 < ao[..., 0].mean() < 1.0
    # every probe's foot is its texel's centre in rtw_cast's uv
    back = probes.copy()
    back[:, 3:6] = -probes[:, 3:6]
    back[:, 6], back[:, 7] = 0.0, 1.0
    h = gpu.cast(back, want=("prim", "uv"))
    centre = np.stack(np.meshgrid((np.arange(nu) + 0.5) / nu, (np.arange(nv) + 0.5) / nv), axis=-1).reshape(-1, 2)
    err = np.abs(h["uv"].astype(np.float64) - centre).max()
    print(f"bake_rect: largest |uv - texel centre| = {err:.3e}")
    assert (h["prim"] == floor).all() and err <= 1e-4
