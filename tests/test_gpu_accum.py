"""Accumulation sessions (include/rtw.h rtw_accum_*) on the GPU. The contract makes them exact: the frame after n samples is, bit for
bit, rtw_render's frame with spp = n whatever the schedule of adds, and the error map is rtw_render_adaptive's - so the existing
renderer is the oracle. Frames are 64x64 (64 groups of 64 pixels: job ranges, the cull rectangle and the end-game launch all occur),
depth 8, caps of at most 512."""
import os
import subprocess

import numpy as np
import pytest
import torch  # (before the HIP library is loaded, as in a run of the whole suite: first imported after it, torch found no device)

from raytracing_weekend_amd import abi
from test_gpu_adaptive import CASES
from test_gpu_cull import K_PATH, aimed_aside

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 64
DEPTH = 8
SCHEDULES = ([256], [16] * 16, [48, 80, 128], [128, 128], [112, 32, 112])
KNOBS = ("RTW_PATH_UNIT_BLOCKS", "RTW_PATH_FINE_BLOCKS", "RTW_BLOCKSUM_BYTES")


@pytest.fixture(scope="module")
def gpu():
    r = abi.Renderer(0)
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _with_spp(p, n):
    return abi.make_params(p.width, p.height, int(n), p.max_depth, seed=p.seed, row0=p.row0, row1=p.row1, rng_kind=p.rng_kind,
                           sample_offset=p.sample_offset, samples_per_pass=p.samples_per_pass, row_stride=p.row_stride, estimator=p.estimator)


class Refs:
    """render(spp = n) of one scene and one set of params, rendered once per n"""

    def __init__(self, gpu, p):
        self.gpu, self.p, self.cache = gpu, p, {}

    def __call__(self, n):
        if n not in self.cache:
            self.cache[n] = self.gpu.render(_with_spp(self.p, n))
        return self.cache[n]


def _run(gpu, p, schedule, refs, error=False):
    """One session over `schedule`; after every add the frame must be refs(done). Returns the summed (samples, segments, shadow rays)."""
    gpu.accum_begin(p, error=error)
    done, tot = 0, [0, 0, 0]
    try:
        for n in schedule:
            st = gpu.accum_add(n)
            done += n
            assert st.samples == abi.local_rows(p) * p.width * n
            for k, v in enumerate((st.samples, st.segments, st.shadow_rays)):
                tot[k] += v
            img = gpu.accum_read()
            ref = refs(done)[0]
            assert _same(img, ref), f"schedule {schedule} at {done}: {np.count_nonzero(_bits(img) != _bits(ref))} words differ"
        info = gpu.accum_status()
        assert (info.active, info.done, info.cap) == (1, done, p.spp)
        assert [info.samples, info.segments, info.shadow_rays] == tot
    finally:
        gpu.accum_end()
    return tot


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_schedule_gives_the_one_shot_render(gpu, case):
    make, kw = CASES[case]
    gpu.upload_scene(make(W, H))
    p = abi.make_params(W, H, 256, DEPTH, **kw)
    refs = Refs(gpu, p)
    st_ref = refs(256)[1]
    for schedule in SCHEDULES:
        tot = _run(gpu, p, schedule, refs)
        assert tot == [st_ref.samples, st_ref.segments, st_ref.shadow_rays], (schedule, tot)


@pytest.mark.parametrize("regime", ["unit_sums", "passes", "unit_sums_in_passes"])
def test_unit_sum_and_multi_pass_regimes(gpu, monkeypatch, regime):
    """The planner picks 8-block lane units (one stored sum per 128 samples) and passes over the samples for long renders only; the
    tuning knobs force them at this size: RTW_PATH_UNIT_BLOCKS=8 RTW_PATH_FINE_BLOCKS=2, and RTW_BLOCKSUM_BYTES=65536 (one slot per
    pixel at 64x64: passes of 8 blocks, all single-block launches); the third regime has passes that keep a unit-sum region. Same bits
    as render under the same knobs and under none."""
    env = {}
    if regime != "passes":
        env.update(RTW_PATH_UNIT_BLOCKS="8", RTW_PATH_FINE_BLOCKS="2")
    if regime == "passes":
        env.update(RTW_BLOCKSUM_BYTES="65536")
    if regime == "unit_sums_in_passes":
        # 9 slots per pixel: with 8-block units and 2 fine blocks a 16-block pass takes 1 unit slot + 8 block slots, a 24-block pass
        # 2 + 8, so the 32 blocks of [512] run as two passes of 16 with a coarse (unit-sum) region of 8 blocks each
        env.update(RTW_BLOCKSUM_BYTES=str(9 * 65536))
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    gpu.upload_scene(abi.build_scene(0, W, H))
    p = abi.make_params(W, H, 512, DEPTH)
    schedules = ([512], [48, 464], [128, 384], [272, 240])
    dones = sorted({sum(s[:k + 1]) for s in schedules for k in range(len(s))})
    plain = Refs(gpu, p)
    for n in dones:
        plain(n)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    knobbed = Refs(gpu, p)
    for n in dones:
        assert _same(knobbed(n)[0], plain(n)[0]), n
    st_ref = plain(512)[1]
    for schedule in schedules:
        tot = _run(gpu, p, schedule, knobbed)
        assert tot == [st_ref.samples, st_ref.segments, st_ref.shadow_rays], (schedule, tot)


def test_adds_to_a_frame_aimed_past_the_scene(gpu):
    """Every group of pixels is culled: an add launches no k_path, the state stays black, and each sample counts as one segment on the host"""
    gpu.upload_scene(aimed_aside(abi.build_scene(0, W, H)))
    p = abi.make_params(W, H, 64, DEPTH)
    refs = Refs(gpu, p)
    gpu.accum_begin(p)
    done, tot = 0, [0, 0, 0]
    try:
        for n in (16, 48):
            st = gpu.accum_add(n)
            done += n
            assert st.samples == st.segments == W * H * n and st.shadow_rays == 0 and st.kernel_segments[K_PATH] == 0
            for k, v in enumerate((st.samples, st.segments, st.shadow_rays)):
                tot[k] += v
            img, ref = gpu.accum_read(), refs(done)[0]
            assert _same(img, ref), f"at {done}: {np.count_nonzero(_bits(img) != _bits(ref))} words differ"
        info = gpu.accum_status()
        assert (info.active, info.done, info.cap) == (1, done, p.spp)
        st_ref = refs(64)[1]
        assert [info.samples, info.segments, info.shadow_rays] == tot == [st_ref.samples, st_ref.segments, st_ref.shadow_rays]
    finally:
        gpu.accum_end()


@pytest.mark.parametrize("case", ["scene0_path_hot", "tree_wavefront"])
def test_error_map_is_the_adaptive_renderers(gpu, case):
    make, kw = CASES[case]
    gpu.upload_scene(make(W, H))
    p = abi.make_params(W, H, 256, DEPTH, **kw)
    refs = Refs(gpu, p)
    gpu.accum_begin(p, error=True)
    try:
        done = 0
        for n in (32, 64, 96):
            gpu.accum_add(n)
            done += n
            img, err = gpu.accum_read(error=True)
            _, spp, ref_err, _ = gpu.render_adaptive(_with_spp(p, done), 0.0, min_spp=done)
            assert (spp == done).all()
            assert _same(err, ref_err), f"at {done}: {np.count_nonzero(_bits(err) != _bits(ref_err))} of {err.size} differ"
            assert _same(img, refs(done)[0]), done
            assert _same(gpu.accum_read(), img)
        assert gpu.accum_status().flags == abi.RTW_ACCUM_ERROR
    finally:
        gpu.accum_end()
    # the error map needs the flag, and two blocks
    gpu.accum_begin(p)
    try:
        gpu.accum_add(32)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            gpu.accum_read(error=True)
        assert _same(gpu.accum_read(), refs(32)[0])
    finally:
        gpu.accum_end()
    gpu.accum_begin(p, error=True)
    try:
        gpu.accum_add(16)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            gpu.accum_read(error=True)
        assert _same(gpu.accum_read(), refs(16)[0])
    finally:
        gpu.accum_end()


def test_other_calls_between_adds_do_not_disturb_the_session(gpu):
    gpu.upload_scene(abi.build_scene(0, W, H))
    p = abi.make_params(W, H, 128, DEPTH)
    small = abi.make_params(48, 40, 48, DEPTH)
    guide_p = abi.make_params(W, H, 16, DEPTH)
    adapt_p = abi.make_params(W, H, 96, DEPTH)

    def others():
        img, st = gpu.render(small)
        g = gpu.render_guides(guide_p)
        a = gpu.render_adaptive(adapt_p, 0.02, min_spp=32)
        d = gpu.denoise(np.sqrt(np.clip(img, 0, 1)), iterations=2)
        return [img, g["albedo"], g["normal"], g["depth"], g["prim"], a[0], a[1], a[2], d], (st.samples, st.segments, st.shadow_rays)

    alone, alone_counts = others()
    ref, _ = gpu.render(p)
    gpu.accum_begin(p, error=True)
    try:
        gpu.accum_add(64)
        between, between_counts = others()
        gpu.accum_add(64)
        img, err = gpu.accum_read(error=True)
    finally:
        gpu.accum_end()
    assert _same(img, ref)
    assert _same(err, gpu.render_adaptive(p, 0.0, min_spp=128)[2])
    assert between_counts == alone_counts
    for a, b in zip(alone, between):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("error", [False, True])
@pytest.mark.parametrize("case", ["scene0_path_hot", "philox_offset_shard_tree"])
def test_save_and_restore_continue_exactly(gpu, case, error):
    make, kw = CASES[case]
    blob = make(W, H)
    gpu.upload_scene(blob)
    p = abi.make_params(W, H, 256, DEPTH, **kw)
    ref, st_ref = gpu.render(p)
    ref_err = gpu.render_adaptive(p, 0.0, min_spp=256)[2] if error else None
    gpu.accum_begin(p, error=error)
    gpu.accum_add(48)
    saved = gpu.accum_save()
    info = gpu.accum_status()
    assert len(saved) == info.state_bytes == 128 + abi.local_rows(p) * W * 16 * (3 if error else 2)
    gpu.accum_end()
    assert gpu.accum_status().active == 0

    other = abi.Renderer(0)  # a new context
    try:
        other.upload_scene(blob)
        for r in (gpu, other):
            r.accum_restore(saved)
            info = r.accum_status()
            assert (info.active, info.done, info.cap, info.flags) == (1, 48, 256, int(error))
            assert bytes(info.params) == bytes(p)
            assert r.accum_save() == saved
            r.accum_add(208)
            got = r.accum_read(error=error)
            info = r.accum_status()
            r.accum_end()
            assert _same(got[0] if error else got, ref)
            if error:
                assert _same(got[1], ref_err)
            assert (info.samples, info.segments, info.shadow_rays) == (st_ref.samples, st_ref.segments, st_ref.shadow_rays)
    finally:
        other.close()


def test_refusals_leave_the_context_usable(gpu):
    blob = abi.build_scene(0, W, H)
    gpu.upload_scene(blob)
    p = abi.make_params(W, H, 64, DEPTH)
    ref, _ = gpu.render(p)

    def refused(f, *a, code=-1):
        with pytest.raises(RuntimeError, match=r"\(%d\)" % code):
            f(*a)

    def usable(active):
        assert gpu.accum_status().active == active
        assert _same(gpu.render(p)[0], ref)

    # nothing to read, add to, save or end without a session
    for f, a in ((gpu.accum_add, (16,)), (gpu.accum_read, ()), (gpu.accum_save, ()), (gpu.accum_end, ())):
        refused(f, *a)
    refused(gpu.accum_begin, abi.make_params(W, H, 40, DEPTH))       # a cap that is not whole blocks
    refused(gpu.accum_begin, abi.make_params(W, H, 0x7ffffff0, DEPTH, sample_offset=16))  # sample_offset + cap overflows
    usable(0)
    gpu.accum_begin(p)
    refused(gpu.accum_begin, p)   # twice
    refused(gpu.accum_read)       # done = 0
    refused(gpu.accum_add, 24)    # not whole blocks
    refused(gpu.accum_add, 0)
    refused(gpu.accum_add, 80)    # past the cap
    usable(1)
    gpu.accum_add(48)
    refused(gpu.accum_add, 32)    # 48 + 32 > 64
    saved = gpu.accum_save()
    refused(gpu.accum_restore, saved)  # a session is active
    assert gpu.accum_status().done == 48
    gpu.accum_add(16)
    assert _same(gpu.accum_read(), ref)
    # a new scene ends the session
    gpu.upload_scene(abi.build_scene(3, W, H))
    assert gpu.accum_status().active == 0
    refused(gpu.accum_add, 16)
    refused(gpu.accum_restore, saved)  # another scene
    assert gpu.accum_status().active == 0
    gpu.render(p)
    gpu.upload_scene(blob)
    flipped = bytearray(saved)
    flipped[0] ^= 0x40
    refused(gpu.accum_restore, bytes(flipped))
    usable(0)
    refused(gpu.accum_restore, saved[:-16])
    usable(0)
    refused(gpu.accum_restore, saved + bytes(16))
    usable(0)
    gpu.accum_restore(saved)  # and the real thing still works
    gpu.accum_add(16)
    assert _same(gpu.accum_read(), ref)
    gpu.accum_end()
    # no scene at all: a fresh context
    r = abi.Renderer(0)
    try:
        with pytest.raises(RuntimeError, match=r"\(-3\)"):
            r.accum_begin(p)
        with pytest.raises(RuntimeError, match=r"\(-3\)"):
            r.accum_restore(saved)
        assert r.accum_status().active == 0
    finally:
        r.close()


def test_read_device_on_a_torch_stream(gpu):
    gpu.upload_scene(abi.build_scene(0, W, H))
    p = abi.make_params(W, H, 64, DEPTH, row0=8, row1=40)
    gpu.accum_begin(p)
    try:
        gpu.accum_add(32)
        host = gpu.accum_read()
        stream = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(stream):
            t = torch.full((32, W, 4), -1.0, dtype=torch.float32, device="cuda:0")
            gpu.accum_read_device(t.data_ptr(), stream.cuda_stream)
            doubled = t * 2  # ordered behind the read on the same stream
        stream.synchronize()
        assert np.array_equal(t.cpu().numpy().view(np.uint32), _bits(host))
        assert np.array_equal(doubled.cpu().numpy(), host * 2)
        t0 = torch.zeros((32, W, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        gpu.accum_read_device(t0.data_ptr())  # the context's own stream
        assert np.array_equal(t0.cpu().numpy().view(np.uint32), _bits(host))
    finally:
        gpu.accum_end()


def test_group_session_equals_the_single_device_frame(gpu):
    blob = abi.build_scene(0, W, H)
    gpu.upload_scene(blob)
    p = abi.make_params(W, H, 128, DEPTH)
    ref, st_ref = gpu.render(p)
    g = abi.Renderer([0, 0])
    try:
        g.upload_scene(blob)
        g.accum_begin(p)
        g.accum_add(48)
        assert _same(g.render(p)[0], ref)  # the group's own render between the adds
        g.accum_add(80)
        img = g.accum_read()
        info = g.accum_status()
        g.accum_end()
        assert _same(img, ref)
        assert (info.samples, info.segments, info.shadow_rays) == (st_ref.samples, st_ref.segments, st_ref.shadow_rays)
    finally:
        g.close()


def test_cli_progressive_checkpoint_resume(tmp_path):
    cli = os.path.join(ROOT, "raytracing_weekend_amd", "host", "rtw_render")
    base = [cli, "-s", "0", "-dx", "64", "-dy", "64", "-d", "8"]
    a, b, c, d, st = (str(tmp_path / n) for n in ("a.pfm", "b.pfm", "c.pfm", "d.pfm", "st.bin"))

    def run(args):
        return subprocess.run(base + args, capture_output=True, text=True, timeout=120)

    assert run(["-ns", "128", "-o", a]).returncode == 0
    r = run(["-ns", "128", "-progressive", "32", "-v", "-o", b])
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == open(b, "rb").read()
    assert [l for l in r.stderr.split("\n") if "progressive:" in l] == [f"INFO: progressive: {n} of 128 spp" for n in (32, 64, 96, 128)]
    r = run(["-ns", "64", "-checkpoint", st, "-o", c])
    assert r.returncode == 0 and os.path.getsize(st) == 128 + 64 * 64 * 32, r.stderr
    r = run(["-resume", st, "-ns", "128", "-o", d])
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == open(d, "rb").read()
    assert open(c, "rb").read() != open(a, "rb").read()
    bad = subprocess.run([cli, "-s", "3", "-dx", "64", "-dy", "64", "-d", "8", "-resume", st, "-ns", "128", "-o", str(tmp_path / "f.pfm")],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "rtw_accum_restore" in bad.stderr and "another scene" in bad.stderr, bad.stderr
    assert not os.path.exists(str(tmp_path / "f.pfm"))
    bad = run(["-resume", st, "-ns", "32", "-o", str(tmp_path / "g.pfm")])
    assert bad.returncode != 0 and "more than -ns" in bad.stderr, bad.stderr
