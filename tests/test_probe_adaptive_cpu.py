"""CPU suite of the adaptive probes (include/rtw.h rtw_probe_adaptive / rtw_probe_adaptive_device): the additive ABI, the planning
header under the sanitizers, the referee probe_adaptive_ref.reference on synthetic block sums, and a rehearsal of the GPU test's
inputs on the oracle alone, which shows that those inputs spread the probes over the checkpoints."""
import ast
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_ref as A
import oracle
import probe_adaptive_ref as PA
import probe_ref as P
import radiance_ref as R
from raytracing_weekend_amd import abi, bake


# ---------------------------------------------------------------- ABI
def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(abi.REPO_DIR, "include", "rtw.h")).read(), flags=re.S)


def test_header_declares_both_entry_points_and_stays_at_version_5():
    text = " ".join(header().split())
    assert ("int rtw_probe_adaptive(rtw_ctx* ctx, const float* probes, size_t n, const rtw_probe_params* params, const rtw_adaptive* ad, "
            "float* rgba_out, int32_t* spp_out, float* error_out, rtw_stats* stats);") in text
    assert ("int rtw_probe_adaptive_device(rtw_ctx* ctx, const float* d_probes, size_t n, const rtw_probe_params* params, "
            "const rtw_adaptive* ad, void* d_rgba, void* d_spp, void* d_error, void* hip_stream, rtw_stats* stats);") in text
    assert "#define RTW_ABI_VERSION 5" in text
    assert abi.RTW_ABI_VERSION == 5 and C.sizeof(abi.Adaptive) == 16 and C.sizeof(abi.ProbeParams) == 32
    assert C.sizeof(abi.Stats) == 184 and C.sizeof(abi.Params) == 48 and C.sizeof(abi.RadianceParams) == 32


def test_symbols_are_listed_and_exported():
    assert "rtw_probe_adaptive" in abi.HIP_SYMBOLS and "rtw_probe_adaptive_device" in abi.HIP_SYMBOLS
    lib = abi.load_hip()
    assert hasattr(lib, "rtw_probe_adaptive") and hasattr(lib, "rtw_probe_adaptive_device") and lib.rtw_abi_version() == 5


def test_both_definitions_run_inside_guarded_and_the_unit_is_built():
    hip = open(os.path.join(abi.PKG_DIR, "csrc", "rtw_hip.hip")).read()
    for name in ("rtw_probe_adaptive", "rtw_probe_adaptive_device"):
        body = re.search(r"\nint " + name + r"\(rtw_ctx\* c,[^{]*\{(.*?)\n\}", hip, flags=re.S).group(1)
        assert body.strip().startswith("return guarded(c, [&] {"), name
    assert '#include "rtw_probe_adaptive.hip"' not in hip  # (a translation unit of its own, in no other)
    entry = open(os.path.join(abi.REPO_DIR, "__graft_entry__.py")).read()
    assert '("rtw_probe_adaptive.hip", "rtw_probe_adaptive.o", [])' in entry
    assert '"rtw_probe_adaptive.hip"' not in entry.split("UNIT_FLAGS = ")[1].split("\n")[0]  # the common flags
    # the shared body and the older probe kernels are not part of this feature's source: the new kernels live in their own unit
    unit = open(os.path.join(abi.PKG_DIR, "csrc", "rtw_probe_adaptive.hip")).read()
    assert "radiance_raygen<KIND, true>" in unit and "probe_direction(" in unit and "traverse<NoRng, true, true>" in unit


def test_null_context_is_an_error_not_a_crash():
    lib = abi.load_hip()
    probes, out = np.zeros((4, 8), np.float32), np.zeros((4, 4), np.float32)
    spp, err = np.zeros(4, np.int32), np.zeros(4, np.float32)
    ad = abi.Adaptive(32, 0, 0.02, 0)
    for mode in abi.PROBE_MODES:
        pp = abi.make_probe_params(64, 4, mode=mode)
        for n in (0, 4):
            assert lib.rtw_probe_adaptive(None, probes.ctypes.data, n, C.byref(pp), C.byref(ad), out.ctypes.data, spp.ctypes.data, err.ctypes.data, None) < 0
            assert lib.rtw_probe_adaptive_device(None, probes.ctypes.data, n, C.byref(pp), C.byref(ad), out.ctypes.data, spp.ctypes.data,
                                                 err.ctypes.data, None, None) < 0
    assert lib.rtw_probe_adaptive(None, None, 0, None, None, None, None, None, None) < 0
    assert not out.any() and not spp.any() and not err.any()


def test_torch_is_imported_inside_the_function_only():
    for name in ("torch_probe.py", "bake.py"):
        tree = ast.parse(open(os.path.join(abi.PKG_DIR, name)).read())
        top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
        names = {a.name.split(".")[0] for n in top if isinstance(n, ast.Import) for a in n.names} | {(n.module or "").split(".")[0] for n in top if isinstance(n, ast.ImportFrom)}
        assert "torch" not in names, name
    from raytracing_weekend_amd import torch_probe
    assert callable(torch_probe.probe_adaptive_torch) and callable(bake.bake_rect_adaptive)


class NoLibrary:
    """A Renderer that must refuse before it reaches the library."""
    ctx = None

    class lib:
        @staticmethod
        def rtw_probe_adaptive(*a):
            raise AssertionError("the library was called")


def test_python_side_argument_validation():
    call = abi.Renderer.probe_adaptive
    good = np.zeros((5, 8), np.float32)
    for probes in (np.zeros((5, 7), np.float32), np.zeros(8, np.float32), np.zeros((5, 8), np.float64), [[0.0] * 8]):
        with pytest.raises(ValueError):
            call(NoLibrary, probes, 64, 4, 0.02)
    for cap in (0, -16, 1.5, None, True):
        with pytest.raises(ValueError):
            call(NoLibrary, good, cap, 4, 0.02)
    with pytest.raises(ValueError):
        call(NoLibrary, good, 64, 4, 0.02, mode="ao")


# ---------------------------------------------------------------- the planning header, under the sanitizers
def test_plan_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "probe_adaptive_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-o", exe, os.path.join(abi.REPO_DIR, "tests", "native", "probe_adaptive_plan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "probe_adaptive_plan_check ok" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------- the referee on synthetic block sums
def hand_err(y):
    """err of block statistics y (float64 values of float32 numbers), written out once more."""
    b = float(len(y))
    m1 = m2 = 0.0
    for v in y:
        m1, m2 = m1 + v, m2 + v * v
    mean = m1 / b
    var = max(0.0, (m2 - m1 * mean) / (b - 1.0))
    return np.float32(np.sqrt(var / b) / (2.0 * np.sqrt(max(mean, 1e-3))))


def test_referee_on_hand_computed_irradiance_blocks():
    """Checkpoints of (32, 0, 128): 32, 48, 80, 128. Five probes: constant blocks (err 0), all zero, a NaN block, two blocks that
    differ widely and then settle, and one that stays noisy."""
    assert A.checkpoints(32, 0, 128) == [32, 48, 80, 128]
    S = np.zeros((8, 5, 3), np.float32)
    S[:, 0] = 16.0                     # y_b = 1 (up to the luminance weights' rounding): err 0 at 32
    S[0, 2] = np.nan                   # a NaN in the first block: err is NaN at every checkpoint
    S[1:, 2] = (4.0, 20.0, 9.0)
    S[:, 3, :] = np.array([1, 31, 16, 16, 16, 16, 16, 16], np.float32)[:, None]
    S[:, 4, :] = np.array([1, 31, 1, 31, 1, 31, 1, 31], np.float32)[:, None]
    out, n, err = PA.reference(S, 0.16, 32, 0, 128)
    y3 = A.block_y(S[:, 3]).astype(np.float64)
    y4 = A.block_y(S[:, 4]).astype(np.float64)
    e3 = [hand_err(y3[:k]) for k in (2, 3, 5, 8)]
    e4 = [hand_err(y4[:k]) for k in (2, 3, 5, 8)]
    print("probe 3 err at the checkpoints:", e3, "probe 4:", e4)
    # with y = S / 16 exactly: probe 3 has 0.469, 0.271, 0.148, 0.089 and probe 4 0.469, 0.377, 0.255, 0.177 (the luminance weights
    # move the last digits): under 0.16 probe 3 stops at 80 and probe 4 reaches the cap; under 0.3 they stop at 48 and 80
    assert e3[1] > 0.16 > e3[2] and e4[2] > 0.16 and e3[0] > 0.3 > e3[1] and e4[1] > 0.3 > e4[2]
    assert list(n) == [32, 32, 128, 80, 128]
    assert err[0] == 0.0 and err[1] == 0.0 and np.isnan(err[2]) and err[3] == e3[2] and err[4] == e4[3]
    assert np.isnan(out[2, :3]).all() and (out[:, 3] == 1.0).all()
    assert np.array_equal(out[0, :3], np.full(3, (np.float32(32.0) / np.float32(32.0)) * PA.PI, np.float32)) and not out[1, :3].any()
    _, n2, err2 = PA.reference(S, 0.3, 32, 0, 128)
    assert list(n2) == [32, 32, 128, 48, 80] and err2[3] == e3[1] and err2[4] == e4[2]
    # the NaN probe does not stop before the cap even at an infinite threshold: NaN < inf is false
    _, n3, _ = PA.reference(S, np.inf, 48, 0, 128)
    assert list(n3) == [48, 48, 128, 48, 48]
    # the all-zero probe: err 0, so min_spp for any threshold > 0 and the cap for threshold 0
    for thr, want in ((1e-30, 32), (0.0, 128)):
        o, nn, ee = PA.reference(S[:, 1:2], thr, 32, 0, 128)
        assert list(nn) == [want] and ee[0] == 0.0 and np.array_equal(o[0], np.array([0, 0, 0, 1], np.float32))
    # the value is the sum in the contract's order: units of 8 blocks, the open unit last (272 = two units and three blocks)
    rng = np.random.default_rng(5)
    T = rng.random((17, 3, 3)).astype(np.float32) * 40
    o, nn, _ = PA.reference(T, 0.0, 32, 48, 272)
    for i in range(3):
        units = [functools.reduce(lambda a, b: a + b, T[u:min(u + 8, 17), i], np.zeros(3, np.float32)) for u in (0, 8, 16)]
        want = ((((np.zeros(3, np.float32) + units[0]) + units[1]) + units[2]) / np.float32(272)) * PA.PI
        assert nn[i] == 272 and np.array_equal(o[i, :3].view(np.uint32), want.astype(np.float32).view(np.uint32))


def test_referee_on_hand_computed_occlusion_counts():
    c = np.zeros((8, 4), np.int64)
    c[:, 0] = 16                                   # open: y = 1, err 0
    c[:, 2] = [0, 16, 8, 8, 8, 8, 8, 8]            # settles
    c[:, 3] = [0, 16, 0, 16, 0, 16, 0, 16]         # never
    out, n, err = PA.reference(c, 0.15, 32, 0, 128, mode="occlusion")
    e2 = [hand_err([float(np.float32(v) * np.float32(0.0625)) for v in c[:k, 2]]) for k in (2, 3, 5, 8)]
    e3 = [hand_err([float(np.float32(v) * np.float32(0.0625)) for v in c[:k, 3]]) for k in (2, 3, 5, 8)]
    print("occlusion probe 2 err:", e2, "probe 3:", e3)
    # probe 2: 0.354, 0.204, 0.112, 0.067; probe 3: 0.354, 0.289, 0.194, 0.134
    first = next(k for k, e in enumerate(e2) if e < 0.15)
    assert first == 2 and all(e >= 0.15 for e in e3[:3])
    assert list(n) == [32, 32, [32, 48, 80, 128][first], 128]
    assert err[0] == 0.0 and err[1] == 0.0 and err[2] == e2[first] and err[3] == e3[3]
    want2 = np.float32(c[: n[2] // 16, 2].sum()) / np.float32(n[2])
    assert np.array_equal(out[:, 0], np.array([1.0, 0.0, want2, 0.5], np.float32)) and (out[:, 3] == 1.0).all()
    assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 0], out[:, 2])
    _, n0, _ = PA.reference(c, 0.0, 32, 0, 128, mode="occlusion")
    assert list(n0) == [128] * 4
    _, ninf, _ = PA.reference(c, np.inf, 32, 0, 128, mode="occlusion")
    assert list(ninf) == [32] * 4


def test_block_helpers():
    s = np.arange(32 * 2 * 3, dtype=np.float32).reshape(32, 2, 3)
    b = PA.block_sums(s)
    assert b.shape == (2, 2, 3) and np.array_equal(b[1, 0], s[16:32, 0].sum(0))
    o = np.zeros((32, 3), bool)
    o[3:20, 1] = True
    assert np.array_equal(PA.block_counts(o), [[0, 13, 0], [0, 4, 0]])
    assert PA.histogram([32, 32, 256]) == {32: 2, 256: 1}


# ---------------------------------------------------------------- rehearsal of the GPU test's inputs, on the oracle alone
CAP, MIN_SPP, DEPTH, KEY, THRESHOLD = 256, 32, 8, 5, 0.02


def floor_probes():
    blob = abi.build_scene(0, 32, 32)
    prims = abi.parse_scene(blob)["prims"]
    floor = next(i for i, p in enumerate(prims) if p.type == abi.PRIM_RECT_Y and p.p[4] == 0.0 and p.xform == 0)
    return blob, bake.rect_probes(blob, floor, 12, 8)


def test_rehearsal_the_gpu_tests_inputs_spread_over_the_checkpoints():
    """Statistical, not a bit check: the direction goes to the oracle as the point ll = o + d, one rounding away from d."""
    blob, probes = floor_probes()
    n = len(probes)
    assert n == 96 and A.checkpoints(MIN_SPP, 0, CAP) == [32, 48, 80, 128, 192, 256]
    d = P.directions(probes, CAP, key_offset=KEY)
    smp = np.empty((CAP, n, 3), np.float32)
    for i in range(n):
        o = probes[i, :3]
        for s in range(CAP):
            smp[s, i] = R.trace_samples(blob, o, (o + d[i, s]).astype(np.float32), KEY + i, 1, DEPTH, 0x6314759, abi.RTW_RNG_PHILOX, s, 0)[0]
    smp = np.where(np.isnan(smp), np.float32(0), smp)
    _, n_i, err = PA.reference(PA.block_sums(smp), THRESHOLD, MIN_SPP, 0, CAP)
    print("irradiance n_i:", PA.histogram(n_i))
    assert PA.not_vacuous(n_i, MIN_SPP, CAP), PA.histogram(n_i)
    # occlusion at tmax 150
    occ = probes.copy()
    occ[:, 7] = 150.0
    open_ = np.empty((CAP, n), bool)
    for s in range(CAP):
        _, prim = oracle.intersect(blob, P.rays_of(occ, d, s))
        open_[s] = prim < 0
    _, n_o, _ = PA.reference(PA.block_counts(open_), THRESHOLD, MIN_SPP, 0, CAP, mode="occlusion")
    print("occlusion n_i:", PA.histogram(n_o))
    assert PA.not_vacuous(n_o, MIN_SPP, CAP), PA.histogram(n_o)
