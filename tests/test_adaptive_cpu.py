"""Adaptive sampling without a GPU: the checkpoint schedule and argument validation of csrc/rtw_plan.h (tests/native/
adaptive_check.cpp, compiled with g++), the numpy reference tests/adaptive_ref.py pinned to the CPU oracle's summation order, the
error estimate and the stop rule, and the C entry point's error paths."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
import oracle
from raytracing_weekend_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GOOD = [(64, 0, 4096), (32, 0, 512), (64, 0, 64), (32, 32, 128), (48, 64, 1024), (64, 0, 1024), (128, 16, 256), (32, 0, 4000)]
BAD = [(16, 0, 64, 0.1, 1),    # min_spp < 32
       (40, 0, 64, 0.1, 1),    # min_spp not a multiple of 16
       (64, 0, 48, 0.1, 1),    # min_spp above the cap
       (64, 0, 250, 0.1, 1),   # cap not a multiple of 16
       (64, 8, 256, 0.1, 1),   # step not a multiple of 16
       (64, -16, 256, 0.1, 1),  # negative step
       (64, 0, 256, -1.0, 1),  # negative threshold
       (64, 0, 256, "nan", 1),  # NaN threshold
       (64, 0, 256, 0.1, 2),   # dilate not 0 / 1
       (64, 0, 256, 0.1, -1)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adaptive") / "adaptive_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "adaptive_check.cpp")])

    def run(groups):
        args = [str(v) for g in groups for v in g]
        out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.split("\n")
        return [l for l in out if l]
    return run


def test_schedule_example_from_the_header():
    assert ar.checkpoints(64, 0, 4096) == [64, 96, 144, 224, 336, 512, 768, 1152, 1728, 2592, 3888, 4096]


def test_native_schedules_match_the_reference(checker):
    lines = checker([(m, s, c, 0.01, 1) for m, s, c in GOOD])
    assert len(lines) == len(GOOD)
    for (m, s, c), line in zip(GOOD, lines):
        head, _, tail = line.partition(":")
        assert head.split() == ["ok", str(m), str(s), str(c)], line
        cps = [int(v) for v in tail.split()]
        assert cps == ar.checkpoints(m, s, c)
        assert cps[0] == m and cps[-1] == c
        assert all(b > a for a, b in zip(cps, cps[1:])) and all(v % 16 == 0 for v in cps)
        if s:
            assert all(b - a == s for a, b in zip(cps[:-2], cps[1:-1]))


def test_native_validation_rejects_every_bad_field(checker):
    lines = checker(BAD)
    assert len(lines) == len(BAD)
    assert all(l.startswith("bad ") for l in lines), lines
    assert checker([(64, 0, 256, "inf", 0), (64, 0, 256, 0, 1)])[0].startswith("ok ")


def _oracle_blocks(blob, w, h, nblk, offset, depth):
    """Block sums from 16-spp oracle renders: 16 x the mean of samples [offset + 16 b, offset + 16 b + 16)."""
    S = np.empty((nblk, h, w, 3), np.float32)
    for b in range(nblk):
        img, _ = oracle.render(blob, abi.make_params(w, h, 16, depth, sample_offset=offset + 16 * b), threads=4)
        S[b] = img[..., :3] * np.float32(16)  # exact: undoes a division by a power of two
    return S


def test_reference_mean_is_the_oracle_render_at_every_checkpoint():
    w = h = 16
    blob = abi.build_scene(0, w, h)
    off, cap = 32, 176  # 11 blocks: two summation units, the second open
    S = _oracle_blocks(blob, w, h, cap // 16, off, 6)
    for n in ar.checkpoints(32, 0, cap):
        ref, _ = oracle.render(blob, abi.make_params(w, h, n, 6, sample_offset=off), threads=4)
        got = ar.mean_image(S, n)
        assert np.array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32)), n


def test_error_estimate_is_the_textbook_standard_error():
    rng = np.random.default_rng(5)
    B = 40
    v = rng.gamma(2.0, 0.3, size=(B, 3, 5)).astype(np.float32)
    S = np.repeat(v[..., None], 3, axis=-1) * np.float32(16)
    m1, m2 = ar.moments(S, B)
    err = ar.error(m1, m2, B)
    y = ar.block_y(S).astype(np.float64)
    for i in range(3):
        for j in range(5):
            mean = y[:, i, j].mean()
            want = ar.textbook_se(y[:, i, j], B) / (2.0 * np.sqrt(max(mean, 1e-3)))
            assert err[i, j] == pytest.approx(want, rel=1e-6)
    # a constant pixel has no error; a dark pixel is measured against 1e-3
    S0 = np.full((8, 1, 1, 3), 0.0, np.float32)
    assert ar.error(*ar.moments(S0, 8), 8)[0, 0] == 0.0
    # NaN stays NaN and never compares below a threshold
    Sn = np.full((4, 1, 1, 3), np.nan, np.float32)
    e = ar.error(*ar.moments(Sn, 4), 4)
    assert np.isnan(e[0, 0]) and not (e[0, 0] < np.float32(1.0))


def test_dilation_on_a_hand_worked_grid():
    # err of a 4 x 4 frame, threshold 0.5: two noisy pixels
    err = np.array([[0.1, 0.1, 0.1, 0.1],
                    [0.1, 0.9, 0.1, 0.1],
                    [0.1, 0.1, 0.1, 0.1],
                    [0.1, 0.1, 0.1, 0.7]], np.float32)
    active = np.ones((4, 4), bool)
    keep0 = ar.decide(err, active, 0.5, 0, False)
    assert keep0.sum() == 2 and keep0[1, 1] and keep0[3, 3]
    keep1 = ar.decide(err, active, 0.5, 1, False)
    want = np.array([[1, 1, 1, 0],
                     [1, 1, 1, 0],
                     [1, 1, 1, 1],
                     [0, 0, 1, 1]], bool)
    assert np.array_equal(keep1, want)
    # a pixel that stopped earlier never blocks a neighbour
    active2 = active.copy()
    active2[1, 1] = False
    keep2 = ar.decide(err, active2, 0.5, 1, False)
    assert not keep2[0, 0] and not keep2[1, 1] and keep2[3, 3] and keep2[2, 2]
    # at the cap everything stops
    assert not ar.decide(err, active, 0.5, 1, True).any()


def test_reference_adaptive_extremes():
    rng = np.random.default_rng(1)
    S = rng.gamma(2.0, 0.5, size=(16, 6, 7, 3)).astype(np.float32)
    img, n, err = ar.adaptive(S, 0.0, 32, 0, 256, 1)
    assert (n == 256).all() and np.array_equal(img, ar.mean_image(S, 256))
    img, n, err = ar.adaptive(S, np.inf, 32, 0, 256, 1)
    assert (n == 32).all() and np.array_equal(img, ar.mean_image(S, 32))


def test_adaptive_struct_and_entry_point_without_a_gpu(monkeypatch):
    assert C.sizeof(abi.Adaptive) == 16
    lib = abi.load_hip()
    p = abi.make_params(8, 8, 64, 2)
    ad = abi.Adaptive(32, 0, 0.01, 1)
    out = (C.c_float * 256)()
    assert lib.rtw_render_adaptive(None, C.byref(p), C.byref(ad), out, None, None, None) < 0
    monkeypatch.setenv("RTW_TEST_FAULT", "entry:bad_alloc")
    assert lib.rtw_render_adaptive(None, C.byref(p), C.byref(ad), out, None, None, None) == -5
    monkeypatch.setenv("RTW_TEST_FAULT", "entry:runtime")
    assert lib.rtw_render_adaptive(None, C.byref(p), C.byref(ad), out, None, None, None) == -4
