"""The empty-pixel cull of k_path renders on the GPU (-m gpu): RTW_CULL=0 (every group gets jobs) against the default in one
process - identical image, identical (samples, segments, shadow_rays) -, k_path's own segment count with the cull on equal to the
call's segments minus one per sample of the pixels the host function culls (tests/native/cull_check.cpp prints that count, so the
test fails when nothing is culled), a frame aimed past the scene, and a scene with a sky light, where nothing may be culled."""
import os
import subprocess

import numpy as np
import pytest

from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu
ROOT = abi.REPO_DIR
K_PATH = abi.Stats.KERNELS.index("k_path")


@pytest.fixture(scope="module")
def gpu():
    r = abi.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cull") / "cull_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", path,
                           os.path.join(ROOT, "tests", "native", "cull_check.cpp")])
    return path


def culled_pixels(exe, tmp_path, blob, p):
    """pixels of the shard that lie in culled groups, by the host function"""
    f = tmp_path / "scene.blob"
    f.write_bytes(blob)
    out = subprocess.run([exe, str(f), str(p.width), str(p.height), str(p.row0), str(p.row1), str(max(1, p.row_stride))], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    tok = [ln for ln in out.stdout.splitlines() if ln.startswith("groups")][0].split()
    return int(tok[tok.index("culled_pixels") + 1])


def render_with(gpu, p, cull):
    """the knobs are read per render call"""
    old = os.environ.get("RTW_CULL")
    if cull is None:
        os.environ.pop("RTW_CULL", None)
    else:
        os.environ["RTW_CULL"] = cull
    try:
        return gpu.render(p)
    finally:
        if old is None:
            os.environ.pop("RTW_CULL", None)
        else:
            os.environ["RTW_CULL"] = old


def counts(st):
    return (st.samples, st.segments, st.shadow_rays)


def compare(gpu, exe, tmp_path, blob, p, expect_culled=True):
    gpu.upload_scene(blob)
    off, st_off = render_with(gpu, p, "0")
    on, st_on = render_with(gpu, p, None)
    n_culled = culled_pixels(exe, tmp_path, blob, p)
    print(f"{p.width}x{p.height} rows {p.row0}:{p.row1}:{p.row_stride} spp {p.spp} depth {p.max_depth} rng {p.rng_kind}: culled pixels {n_culled}, "
          f"segments {st_on.segments}, k_path on {st_on.kernel_segments[K_PATH]} off {st_off.kernel_segments[K_PATH]}")
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
    assert counts(st_on) == counts(st_off)
    assert st_off.kernel_segments[K_PATH] == st_off.segments
    assert st_on.kernel_segments[K_PATH] == st_on.segments - n_culled * p.spp
    assert (n_culled > 0) == expect_culled
    return on, st_on


@pytest.mark.parametrize("rng", [abi.RTW_RNG_PHILOX, abi.RTW_RNG_TEA_LCG])
def test_headline_frame(gpu, exe, tmp_path, rng):
    compare(gpu, exe, tmp_path, abi.build_scene(0, 1920, 1080), abi.make_params(1920, 1080, 16, 50, rng_kind=rng))


@pytest.mark.parametrize("w,h,spp,kw", [
    (800, 800, 16, {}),                                    # groups wrap rows, 7.7 % of them empty at most
    (250, 130, 48, {}),                                    # groups wrap rows, a partial last group
    (1920, 1080, 16, {"row0": 3, "row_stride": 8}),        # an interleaved shard
    (640, 360, 32, {"max_depth": 1}),
    (640, 360, 128, {"rng_kind": abi.RTW_RNG_TEA_LCG}),    # several blocks per pixel: unit hand-out over culled lists
])
def test_shapes_and_knobs(gpu, exe, tmp_path, w, h, spp, kw):
    kw = dict(kw)
    depth = kw.pop("max_depth", 12)
    compare(gpu, exe, tmp_path, abi.build_scene(0, w, h), abi.make_params(w, h, spp, depth, **kw))


def test_sample_passes_add_up(gpu, exe, tmp_path):
    """48 spp as three calls of 16 (sample_offset 0, 16, 32), each with and without the cull: the same calls, the same counts"""
    w, h = 640, 360
    blob = abi.build_scene(0, w, h)
    total = 0
    for off in (0, 16, 32):
        _, st = compare(gpu, exe, tmp_path, blob, abi.make_params(w, h, 16, 12, sample_offset=off, samples_per_pass=16))
        total += st.segments
    assert total > 3 * 16 * w * h


def test_small_block_sum_buffer(gpu, exe, tmp_path, monkeypatch):
    """RTW_BLOCKSUM_BYTES small enough for several k_path passes per call: every pass resolves around the culled pixels"""
    w, h = 640, 360
    monkeypatch.setenv("RTW_BLOCKSUM_BYTES", str(8 * w * h * 16))
    compare(gpu, exe, tmp_path, abi.build_scene(0, w, h), abi.make_params(w, h, 512, 6))


def aimed_aside(blob):
    parts = dict(abi.parse_scene(blob))
    hdr = abi.SceneHeader.from_buffer_copy(bytes(parts["header"]))
    for a in range(3):
        hdr.camera.lower_left[a] += 3.0 * hdr.camera.horizontal[a]
    parts["header"] = hdr
    return abi.assemble_scene(parts)


def test_frame_aimed_past_the_scene(gpu, exe, tmp_path):
    w, h = 320, 180
    blob = aimed_aside(abi.build_scene(0, w, h))
    p = abi.make_params(w, h, 32, 12)
    img, st = compare(gpu, exe, tmp_path, blob, p)
    assert (img[..., :3].view(np.uint32) == 0).all() and (img[..., 3] == 1.0).all()
    assert st.segments == st.samples == w * h * 32 and st.shadow_rays == 0 and st.kernel_segments[K_PATH] == 0


def test_sky_light_culls_nothing(gpu, exe, tmp_path):
    w, h = 640, 360
    parts = dict(abi.parse_scene(abi.build_scene(0, w, h)))
    hdr = abi.SceneHeader.from_buffer_copy(bytes(parts["header"]))
    hdr.sky_light = 1
    parts["header"] = hdr
    img, st = compare(gpu, exe, tmp_path, abi.assemble_scene(parts), abi.make_params(w, h, 16, 12), expect_culled=False)
    assert st.kernel_segments[K_PATH] == st.segments
    assert img[0, 0, :3].max() > 0.0  # the corner pixel sees the sky
