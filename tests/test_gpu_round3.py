"""GPU parity tests added in round 3 (-m gpu), all through the C ABI and against the CPU oracle bit for bit:
the sample ranges and pixels the earlier suites never compared with the oracle - the tree scenes at their BASELINE sample
counts under the default two-lane schedule, the rows of the metric frame where whole waves skip the walk, BASELINE config 5's
shard at its full 4096 spp -, the bare `bench.py --gpus N` launch, frames beyond 65535 pixels on a side, and the C ABI's
exception barrier with faults injected in the middle of an upload and inside a group's worker thread."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu
ROOT = abi.REPO_DIR


@pytest.fixture(scope="module")
def gpu():
    r = abi.Renderer(0)
    yield r
    r.close()


def check(img, ref, st=None, st_ref=None):
    assert np.isfinite(img).all()
    d = img[..., :3].astype(np.float64) - ref[..., :3]
    assert float(np.sqrt(np.mean(d * d))) < 1e-4  # the north star's tolerance
    assert np.array_equal(img[..., :3], ref[..., :3])  # and the arithmetic spec's: exact
    assert np.all(img[..., 3] == 1.0)
    if st is not None and st_ref is not None:
        assert (st.samples, st.segments, st.shadow_rays) == (st_ref.samples, st_ref.segments, st_ref.shadow_rays)


@pytest.mark.parametrize("scene,spp,rows", [(1, 512, (400, 402)), (3, 2048, (538, 540))])
def test_baseline_configs_3_and_4_at_their_sample_counts(gpu, scene, spp, rows):
    """BASELINE config 3 (random spheres, 512 spp: the wavefront tree schedule - several batches, two lanes, k_trace_bvh's
    refill) and config 4 (Cornell + fog, 2048 spp, k_path's cold instantiation) rendered as bench.py renders them, default
    knobs; two rows of the full frame against the oracle, which covers every sample index of the configuration."""
    W, H = 1920, 1080
    blob = abi.build_scene(scene, W, H)
    gpu.upload_scene(blob)
    full, st = gpu.render(abi.make_params(W, H, spp, 50))
    assert st.samples == W * H * spp
    p = abi.make_params(W, H, spp, 50, row0=rows[0], row1=rows[1])
    ref, st_ref = oracle.render(blob, p, threads=64)
    check(full[rows[0]:rows[1]], ref)
    band, st_b = gpu.render(p)  # the same rows as a shard of their own: counts comparable with the oracle's
    check(band, ref, st_b, st_ref)


@pytest.mark.parametrize("scene,spp", [(0, 64), (3, 32), (1, 2), (2, 1), (4, 1)])
def test_whole_frames_at_metric_resolution(gpu, scene, spp):
    """EVERY pixel of a 1920x1080 frame against the oracle, all five reference scenes (the bands of the other tests cover all
    sample indices on a few rows; this covers all rows, columns, job orders and the frame's edges at a few samples): scene 0 at
    64 spp (4 summation blocks through k_path's unit hand-out), scene 3 through the cold instantiation, the tree scenes through
    the wavefront kernels with the sample count the oracle's single-threaded-per-row walk affords."""
    W, H = 1920, 1080
    blob = abi.build_scene(scene, W, H)
    gpu.upload_scene(blob)
    p = abi.make_params(W, H, spp, 50)
    img, st = gpu.render(p)
    ref, st_ref = oracle.render(blob, p, threads=64)
    check(img, ref, st, st_ref)


METRIC_FRAMES = os.path.join(ROOT, "tests", "golden", "metric_frames.json")


@pytest.mark.parametrize("name", sorted(json.load(open(METRIC_FRAMES))) if os.path.exists(METRIC_FRAMES) else ["missing"])
def test_whole_baseline_frames_match_the_oracle_hashes(gpu, name):
    """The metric workload ITSELF - all 1920 x 1080 pixels at 4096 spp, 8.49 G samples - and BASELINE configs 1, 2 and 4 whole, at
    their sample counts: SHA-256 of the image bytes and the sample / segment / probe counts against what the CPU oracle
    produced for the same frame (tests/golden/metric_frames.json, written by tests/golden/make_metric_frame_hashes.py: ten
    minutes of a 64-thread host, once; the bands were compared pixel by pixel with the GPU image when it was made). The tree
    scenes' entries are whole frames at 64 / 32 / 16 spp (the oracle walks no tree)."""
    import hashlib
    g = json.load(open(METRIC_FRAMES))[name]
    blob = abi.build_scene(g["scene"], g["width"], g["height"])
    gpu.upload_scene(blob)
    img, st = gpu.render(abi.make_params(g["width"], g["height"], g["spp"], g["max_depth"], seed=g["seed"]))
    assert (st.samples, st.segments, st.shadow_rays) == (g["samples"], g["segments"], g["shadow_rays"])
    assert hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == g["sha256"]


@pytest.mark.parametrize("path", ["1", "0"])
def test_headline_silhouette_rows_at_4096_spp(gpu, monkeypatch, path):
    """The metric workload at 4096 spp on the rows where whole waves skip the walk (may_hit_scene's wave vote, k_classify's
    class 0 / 1 boundary, the box silhouette): rows 24-25 and 1054-1055 of the full frame, both pipelines."""
    monkeypatch.setenv("RTW_PATH", path)
    W, H, spp = 1920, 1080, 4096
    blob = abi.build_scene(0, W, H)
    gpu.upload_scene(blob)
    full, st = gpu.render(abi.make_params(W, H, spp, 50))
    for r0 in (24, 1054):
        p = abi.make_params(W, H, spp, 50, row0=r0, row1=r0 + 2)
        ref, _ = oracle.render(blob, p, threads=64)
        check(full[r0:r0 + 2], ref)


def test_config5_shard_at_4096_spp(gpu):
    """BASELINE config 5 as one rank of eight renders it: rows 7, 15, ... of 7680x4320 at the full 4096 spp (17 G samples in one
    call: the block-sum buffer's largest case); one row of the shard against the oracle."""
    W, H, spp = 7680, 4320, 4096
    blob = abi.build_scene(0, W, H)
    gpu.upload_scene(blob)
    p = abi.make_params(W, H, spp, 50, row0=7, row1=H, row_stride=8)
    img, st = gpu.render(p)
    assert img.shape[0] == 540 and st.samples == 540 * W * spp
    k = 271  # shard row 271 = image row 7 + 8 * 271 = 2175, through the boxes
    pr = abi.make_params(W, H, spp, 50, row0=7 + 8 * k, row1=7 + 8 * k + 1)
    ref, _ = oracle.render(blob, pr, threads=64)
    check(img[k:k + 1], ref)


def test_frames_beyond_65535_pixels_on_a_side(gpu):
    """k_path packs a unit's pixel as x | y << 16; a 70000 x 2 strip must not take that kernel silently."""
    W, H = 70000, 2
    blob = abi.build_scene(0, W, H)
    gpu.upload_scene(blob)
    p = abi.make_params(W, H, 2, 8)
    img, st = gpu.render(p)
    ref, st_ref = oracle.render(blob, p, threads=32)
    check(img, ref, st, st_ref)


def run_bench(extra, env_extra=None, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **(env_extra or {}))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2 ...` from a plain shell (no launcher, no WORLD_SIZE): bench.py starts its two ranks as a fresh
    child and relays the JSON line (VERDICT r02 #1a). gloo: both ranks share this box's one GPU; --check compares the gathered
    frame with a single-tile render."""
    d = run_bench(["--gpus", "2", "--steps", "1", "--warmup", "1", "--spp", "8", "--backend", "gloo", "--check", "--no-cpu-baseline"],
                  {"RTW_POOL_PATHS": str(1 << 22)})
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    assert d["config"]["segments_per_sample"] > 1.0
    assert d["roofline"]["bound"] == "valu" and 0 < d["roofline"]["frac"] < 1


def test_bench_refuses_more_rccl_ranks_than_gpus():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--spp", "4", "--no-cpu-baseline"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    import torch
    if torch.cuda.device_count() >= 2:
        assert out.returncode == 0
    else:
        assert out.returncode != 0 and "needs 2 GPUs" in out.stderr


@pytest.mark.parametrize("config,kernel", [("c3", "k_trace_bvh"), ("c4", "k_path"), ("c2", "k_path")])
def test_bench_other_baseline_configs(config, kernel):
    """--config c2 / c3 / c4: each line names its own dominant kernel and carries a roofline block (at reduced spp here: the
    structure is under test, the numbers are the profile runs')."""
    d = run_bench(["--config", config, "--steps", "1", "--warmup", "1", "--spp", "32", "--no-cpu-baseline"])
    assert d["config"]["name"] == config and d["roofline"]["kernel"] == kernel
    assert d["roofline"]["bound"] == ("valu" if kernel == "k_path" else "hbm")
    assert 0 < d["roofline"]["frac"] < 1 and d["roofline"]["launches"] >= 1
    assert d["roofline"]["per_kernel"] and d["config"]["Msegments_per_s"] > 0


def test_bench_dump_outputs_are_the_last_steps_frame(gpu, tmp_path):
    """--dump-outputs DIR: the frame and counts the timed path computed in its last step are the C ABI's render of the same
    workload; a plain run carries no CPU baseline and no copy probe (those are --full's)."""
    d = run_bench(["--config", "c2", "--steps", "3", "--warmup", "0", "--spp", "8", "--dump-outputs", str(tmp_path)])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert "cpu_baseline" not in d and "device_copy_GBps" not in d["roofline"]
    img, counts = np.load(tmp_path / "image.npy"), np.load(tmp_path / "counts.npy")
    assert img.dtype == np.float32 and counts.dtype == np.float64 and not (tmp_path / "image_rows.npy").exists()
    gpu.upload_scene(abi.build_scene(0, 800, 800))
    want, st = gpu.render(abi.make_params(800, 800, 8, 50, seed=0x6314759))
    assert np.array_equal(img, want) and tuple(counts) == (st.samples, st.segments, st.shadow_rays)


def test_faults_inside_the_library_become_error_codes(monkeypatch):
    """The C ABI's exception barrier (include/rtw.h) with the fault where it would really happen: a std::bad_alloc in the
    middle of rtw_upload_scene (host vectors built, device not yet touched) and one inside a group's worker thread. Either
    comes back as RTW_ERR_OOM with a message, the context stays usable, and the next call succeeds."""
    lib = abi.load_hip()
    w, h = 64, 48
    blob = abi.build_scene(0, w, h)
    one = abi.Renderer(0)
    grp = abi.Renderer([0, 0])
    try:
        monkeypatch.setenv("RTW_TEST_FAULT", "upload:bad_alloc")
        assert lib.rtw_upload_scene(one.ctx, blob, len(blob)) == -5
        assert b"bad_alloc" in lib.rtw_last_error(one.ctx)
        monkeypatch.delenv("RTW_TEST_FAULT")
        one.upload_scene(blob)
        grp.upload_scene(blob)
        p = abi.make_params(w, h, 4, 8)
        want, st1 = one.render(p)
        out = np.empty((h, w, 4), np.float32)
        for kind, code in (("bad_alloc", -5), ("runtime", -4)):
            monkeypatch.setenv("RTW_TEST_FAULT", "worker:" + kind)
            assert lib.rtw_render(grp.ctx, C.byref(p), out.ctypes.data, None) == code
            assert lib.rtw_last_error(grp.ctx)
        monkeypatch.delenv("RTW_TEST_FAULT")
        got, stn = grp.render(p)
        assert np.array_equal(got, want) and stn.segments == st1.segments
    finally:
        one.close()
        grp.close()


def test_group_render_creates_no_threads_per_call(gpu):
    """One persistent worker thread per device of a group: the process's thread count does not move between the
    second and the sixth render call, and every call returns the single-device image."""
    def n_threads():
        return len(os.listdir("/proc/self/task"))
    w, h = 96, 64
    blob = abi.build_scene(0, w, h)
    gpu.upload_scene(blob)
    p = abi.make_params(w, h, 16, 10)
    want, _ = gpu.render(p)
    grp = abi.Renderer([0, 0, 0])
    try:
        grp.upload_scene(blob)
        grp.render(p)
        grp.render(p)
        before = n_threads()
        for _ in range(4):
            got, _ = grp.render(p)
            assert np.array_equal(got, want)
        assert n_threads() == before
    finally:
        grp.close()


def test_pool_that_does_not_fit_is_halved_not_refused(monkeypatch):
    """The wavefront pipeline keeps up to 2^29 paths in flight (120 GiB of state on an MI355X it has to itself). When the
    allocation fails - here: a pool of 2^33 paths asked for through the knob, 2 TB - the render halves the pool until it fits
    instead of returning RTW_ERR_OOM, and the image is the one the default pool gives."""
    W, H, spp = 1920, 1080, 1024
    blob = abi.build_scene(1, W, H)
    want = None
    for pool in (None, str(1 << 33)):
        if pool is None:
            monkeypatch.delenv("RTW_POOL_PATHS", raising=False)
        else:
            monkeypatch.setenv("RTW_POOL_PATHS", pool)
        r = abi.Renderer(0)
        try:
            r.upload_scene(blob)
            img, st = r.render(abi.make_params(W, H, spp, 50))  # 2 lanes x 512 spp x 2 M pixels x 240 B = 509 GB asked for first
        finally:
            r.close()
        if want is None:
            want = (img, st.segments)
        else:
            assert np.array_equal(img, want[0]) and st.segments == want[1]
