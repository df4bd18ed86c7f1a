"""What the GPU test files of the query family and of the float64 checks share: the renderer fixture, the upload under chosen knobs,
the bit-equality helpers, the golden fixtures, the stream-order check of a *_torch call, the sentinel Stats of the refusal tests and
the GPU half of law_common.py: a case observed through rtw_radiance and rtw_render, held to its float64 law and to the oracle.
A plain module (not a conftest): a test file imports what it uses by name, the `gpu` fixture included."""
import functools
import os
import types

import numpy as np
import pytest

import law_common
from raytracing_weekend_amd import abi

GOLD = os.path.join(abi.REPO_DIR, "tests", "golden")
UPLOADS = {"as_uploaded": {}, "forced_tree": {"RTW_BRUTE_MAX": "0"}}  # the knob is read at upload
UPLOADS_LDS = dict(UPLOADS, no_lds={"RTW_LDS_KB": "0"})  # both knobs are read at upload
UPLOAD_KNOBS = ("RTW_BRUTE_MAX", "RTW_LDS_KB")
KNOBS = UPLOAD_KNOBS + ("RTW_RADIANCE_CHUNK", "RTW_RADIANCE_SLAB_BYTES")
BOTH = (abi.RTW_RNG_PHILOX, abi.RTW_RNG_TEA_LCG)
GOLDEN_PAIR = ("cornell_200x200_16spp_d4_philox", "fog_96x96_8spp_d12_lcg")


@pytest.fixture(scope="module")
def gpu():
    r = abi.Renderer(0)
    yield r
    r.close()


def upload(gpu, monkeypatch, blob, how="as_uploaded", knobs=KNOBS, env=None):
    """Upload `blob` with exactly `knobs` cleared, then the upload variant's and `env`'s set. A file whose tests set other knobs
    passes its own tuple: clearing more than it did would change what its tests exercise."""
    for k in knobs:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(UPLOADS_LDS[how], **(env or {})).items():
        monkeypatch.setenv(k, v)
    gpu.upload_scene(blob)


upload_lds = functools.partial(upload, knobs=UPLOAD_KNOBS)  # for the files that set no knob but the two read at upload


# ---------------------------------------------------------------- the same bits
def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_words(a, b):
    """Two arrays of one 4-byte dtype and one shape carry the same bits."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same(a, b):
    """same_words, and both float32."""
    return np.asarray(a).dtype == np.float32 and same_words(a, b)


def same_dict(a, b):
    """Two result dicts (or arrays) carry the same names in the same order and the same bits."""
    if isinstance(a, dict):
        return list(a) == list(b) and all(same_words(a[k], b[k]) for k in a)
    return same_words(a, b)


def same_bits(a, b):
    """The float32 values of a and b carry the same bits (either may be given in another type)."""
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def same3(got, want):
    """(values, spp, err) triples: the counts equal, the floats equal in bits."""
    return same_words(got[0], want[0]) and got[1].dtype == np.int32 and np.array_equal(got[1], want[1]) and same_words(got[2], want[2])


def first_difference(got, want, what, axes=1):
    """The assertion message of a failed same(): how many of the items indexed by the first `axes` axes differ, and the first."""
    bad = np.argwhere((words(got) != words(want)).reshape(got.shape[:axes] + (-1,)).any(-1))
    if not len(bad):
        return ""
    i = tuple(bad[0])
    return f"{len(bad)} {what} differ, first {i if axes > 1 else i[0]}: {got[i]} != {want[i]}"


def to_numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


# ---------------------------------------------------------------- the golden renders
def golden(name):
    """A golden fixture: the file (z), its scene blob and the parameters of its render."""
    z = np.load(os.path.join(GOLD, name + ".npz"))
    scene, w, h, spp, depth, rng, seed = (int(v) for v in z["meta"])
    return types.SimpleNamespace(z=z, blob=z["blob"].tobytes(), scene=scene, w=w, h=h, spp=spp, depth=depth, rng=rng, seed=seed)


def check_golden_render(gpu, g):
    """rtw_render of the uploaded golden scene still gives the fixture's pixels and counts."""
    img, st = gpu.render(abi.make_params(g.w, g.h, g.spp, g.depth, seed=g.seed, rng_kind=g.rng))
    assert np.array_equal(img[..., :3], g.z["rgb"][..., :3]) and np.all(img[..., 3] == 1.0)
    assert (st.samples, st.segments, st.shadow_rays) == tuple(int(v) for v in g.z["stats"])


# ---------------------------------------------------------------- a *_torch call on torch's current stream
def check_stream_order(call, d_in, right, default=None):
    """call(tensor) runs a *_torch wrapper on a tensor like d_in; right(outputs) says whether they are d_in's. The input is written
    on a side stream immediately before the call, behind work that keeps the stream busy - results that are right can only have been
    computed after that write - then the same under torch's default stream, whose null handle the library reads as "the context's
    own stream" (default: another (call, right) pair for that leg). Then the four tensors every wrapper refuses: on the host, not
    float32, a column short, not contiguous."""
    import torch

    side = torch.cuda.Stream(device="cuda:0")
    busy = torch.empty(1 << 26, device="cuda:0")
    stale = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            busy.normal_()
        stale.copy_(d_in, non_blocking=True)
        got = call(stale)
    assert right(got)
    torch.cuda.synchronize()
    stale.zero_()
    torch.cuda.synchronize()
    for _ in range(8):
        busy.normal_()
    stale.copy_(d_in, non_blocking=True)
    call_default, right_default = default or (call, right)
    assert right_default(call_default(stale))
    for bad in (d_in.cpu(), d_in.double(), d_in[:, :-1], d_in.t().contiguous().t()):
        with pytest.raises(ValueError):
            call(bad)


# ---------------------------------------------------------------- a refused call leaves *stats alone
def sentinel_stats():
    return abi.Stats(segments=77, shadow_rays=77, seconds=7.0)


def left_alone(st):
    return (st.segments, st.shadow_rays, st.seconds) == (77, 77, 7.0)


# ---------------------------------------------------------------- a law_common.Case on the GPU: observed, then checked
def radiance_observed(gpu, monkeypatch, case, how, rng, est, seed, base):
    """The case through rtw_radiance under upload `how`: one sample per ray, ray j's keys by key_offset; alpha is 1."""
    upload_lds(gpu, monkeypatch, case.blob, how)
    st = abi.Stats()
    out = gpu.radiance(case.rays(est), 1, case.depth, seed=seed, rng_kind=rng, estimator=est, key_offset=base, stats=st)
    assert np.array_equal(out[:, 3], np.ones(len(out), np.float32))
    return law_common.Observed(out[:, :3].reshape(case.m, case.keys_per_ray, 3), int(st.segments), int(st.shadow_rays))


def render_observed(gpu, monkeypatch, case, path, rng, est, seed, base):
    """The case through rtw_render of each ray's own blob, uploaded as is, by k_path (RTW_PATH=1) or the wavefront kernels (0)."""
    for k in UPLOAD_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RTW_PATH", path)

    def render(blob, params):
        gpu.upload_scene(blob)
        return gpu.render(params)
    return law_common.observe(render, case, rng, est, seed, base)


def check_both(module, name, observed, run, counts):
    """The float64 law of case `name` of `module` first (it takes the counts named in `counts` beside the samples), then the oracle's
    bits on the keys of run = (rng, est, seed, base), then the oracle's counts: a failure says which side moved."""
    rng, est, seed, base = run
    print(module.check(name, observed.samples, est, **{k: getattr(observed, k) for k in counts}))
    want = law_common.oracle_samples(module.case(name), rng, est, seed, base)
    differ = int((words(np.asarray(observed.samples, np.float32)) != words(want.samples)).any(-1).sum())
    assert same_bits(observed.samples, want.samples), f"{name}: {differ} samples differ from the oracle's"
    for k in counts:
        assert getattr(observed, k) == getattr(want, k), f"{name}: {k} {getattr(observed, k)}, the oracle's {getattr(want, k)}"


def probe_is_pi_times_radiance(gpu, probes, out, rng, est, n=1024):
    """Each of the first n irradiance probes `out` of one sample and one segment is, bit for bit, pi times rtw_radiance along
    probe_ref.directions on the same key (the keys count from 0, so the first probes are the first rays)."""
    import probe_ref
    rays = probe_ref.rays_of(probes[:n], probe_ref.directions(probes[:n], 1, rng_kind=rng), 0)
    rad = gpu.radiance(rays, 1, 1, rng_kind=rng, estimator=est, key_offset=0)
    assert same_bits(out[:n, :3], rad[:, :3] * law_common.PI32)
