"""CPU suite of the path records (include/rtw.h rtw_paths / rtw_paths_views and their _device variants): the ABI as the C compiler
lays it out, the chunk plan under the sanitizers, the float32 fold of a sample's contributions, what the Python layer hands to the
library and what it refuses first, and bake.path_segments."""
import ast
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import paths_ref as P
from raytracing_weekend_amd import abi, bake

NEW = ("rtw_paths", "rtw_paths_device", "rtw_paths_views", "rtw_paths_views_device")
HEADER = os.path.join(abi.REPO_DIR, "include", "rtw.h")
CSRC = os.path.join(abi.PKG_DIR, "csrc")
STRUCTS = {"rtw_path_vertex": (abi.PathVertex, abi.PATH_VERTEX, 64), "rtw_path_head": (abi.PathHead, abi.PATH_HEAD, 32),
           "rtw_paths_params": (abi.PathsParams, None, 40)}


# ---------------------------------------------------------------- ABI
def test_structs_are_laid_out_as_the_c_compiler_lays_them_out(tmp_path):
    """sizeof and every offsetof, printed by a C program that includes the header, against ctypes and the numpy dtypes"""
    lines = []
    for name, (ct, _, _) in STRUCTS.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in ct._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rtw.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-o", exe, str(src)])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, (ct, dt, size) in STRUCTS.items():
        assert int(got[name]) == C.sizeof(ct) == size
        for f, _ in ct._fields_:
            assert int(got[f"{name}.{f}"]) == getattr(ct, f).offset, (name, f)
        if dt is not None:
            assert dt.itemsize == size and list(dt.names) == [f for f, _ in ct._fields_]
            assert all(dt.fields[f][1] == getattr(ct, f).offset for f in dt.names)
    assert [f for f, _ in abi.PathsParams._fields_] == ["spp", "max_depth", "seed", "rng_kind", "sample_offset", "estimator", "key_offset", "max_records",
                                                        "reserved"]
    # the first seven words are rtw_radiance_params' own
    assert [(f, getattr(abi.PathsParams, f).offset) for f, _ in abi.RadianceParams._fields_[:7]] == \
           [(f, getattr(abi.RadianceParams, f).offset) for f, _ in abi.RadianceParams._fields_[:7]]


def test_the_change_is_additive_and_the_header_lists_what_abi_lists():
    text = open(HEADER).read()
    assert re.search(r"#define RTW_ABI_VERSION 5\b", text) and abi.RTW_ABI_VERSION == 5
    assert C.sizeof(abi.Stats) == 184 and C.sizeof(abi.Params) == 48 and C.sizeof(abi.RadianceParams) == 32 and C.sizeof(abi.ViewParams) == 32
    assert C.sizeof(abi.View) == 112
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(rtw_[a-z_]+)\s*\(", code))) == sorted(abi.HIP_SYMBOLS)
    assert all(name in abi.HIP_SYMBOLS for name in NEW)
    assert "enum { RTW_PATH_MISS = 0, RTW_PATH_SCATTER = 1, RTW_PATH_END = 2, RTW_PATH_CANCEL = 3 };" in code
    assert "enum { RTW_PATH_EVENT_MASK = 3, RTW_PATH_LIGHT_SAMPLED = 4, RTW_PATH_LIGHT_ADDED = 8 };" in code
    assert (abi.RTW_PATH_MISS, abi.RTW_PATH_SCATTER, abi.RTW_PATH_END, abi.RTW_PATH_CANCEL) == (0, 1, 2, 3)
    assert (abi.RTW_PATH_EVENT_MASK, abi.RTW_PATH_LIGHT_SAMPLED, abi.RTW_PATH_LIGHT_ADDED) == (3, 4, 8)
    for phrase in ("Same path as rtw_radiance", "a -0 comes back as +0", "Entries\n *     beyond that are not written", "leaves *stats alone",
                   "RTW_PATHS_CHUNK_BYTES", "An accumulation session on the context is not disturbed"):
        assert phrase in text, phrase


def test_the_event_constants_are_the_kernels_own_by_a_static_assert():
    unit = re.sub(r"\s+", " ", open(os.path.join(CSRC, "rtw_paths.h")).read())
    assert ("static_assert((int)RTW_PATH_MISS == (int)EV_MISS && (int)RTW_PATH_SCATTER == (int)EV_HIT && (int)RTW_PATH_END == (int)EV_FINISH && "
            "(int)RTW_PATH_CANCEL == (int)EV_CANCEL,") in unit
    assert "static_assert(sizeof(rtw_path_vertex) == 64 && sizeof(rtw_path_head) == 32 && sizeof(rtw_paths_params) == 40" in unit
    assert "enum { EV_MISS = 0, EV_HIT = 1, EV_FINISH = 2, EV_CANCEL = 3 };" in open(os.path.join(CSRC, "rtw_device.h")).read()


def test_the_definitions_run_inside_guarded_and_the_unit_is_built():
    hip = open(os.path.join(CSRC, "rtw_hip.hip")).read()
    for name in NEW:
        body = re.search(r"\nint " + name + r"\(rtw_ctx\* c,[^{]*\{(.*?)\n\}", hip, flags=re.S).group(1)
        assert body.strip().startswith("return guarded(c, [&] {"), name
    assert '#include "rtw_paths.hip"' not in hip  # (a translation unit of its own, in no other)
    entry = open(os.path.join(abi.REPO_DIR, "__graft_entry__.py")).read()
    assert '("rtw_paths.hip", "rtw_paths.o", [])' in entry
    assert '"rtw_paths.hip"' not in entry.split("UNIT_FLAGS = ")[1].split("\n")[0]  # the common flags
    # the kernel takes its regeneration step and its segment from the shared headers, which it includes as they are
    unit = open(os.path.join(CSRC, "rtw_paths.hip")).read()
    for piece in ('#include "rtw_radiance_body.h"', "radiance_raygen<KIND, false>(", "view_raygen<KIND>(", "traverse<Rng<KIND>, false, false>(",
                  "traverse<Rng<KIND>, true, false>(", "shade_a<KIND, TEX>(", "shade_b<KIND>(", "g.ray_time(depth)"):
        assert piece in unit, piece
    assert "RTW_PATHS_CHUNK_BYTES" in open(os.path.join(CSRC, "rtw_plan.h")).read()


def test_symbols_are_exported_and_a_null_context_is_an_error():
    lib = abi.load_hip()
    for name in NEW:
        assert getattr(lib, name).restype is C.c_int
    assert [len(getattr(lib, name).argtypes) for name in NEW] == [7, 8, 10, 11]
    rays = np.zeros((2, 8), np.float32)
    heads, vertices = np.zeros((2, 1), abi.PATH_HEAD), np.zeros((2, 1, 1), abi.PATH_VERTEX)
    pp = abi.make_paths_params(1, 1)
    vp = abi.make_view_params(4, 4, 1, 1)
    v = abi.View()
    for n in (0, 2):
        assert lib.rtw_paths(None, rays.ctypes.data, n, C.byref(pp), heads.ctypes.data, vertices.ctypes.data, None) < 0
        assert lib.rtw_paths_device(None, rays.ctypes.data, n, C.byref(pp), heads.ctypes.data, vertices.ctypes.data, None, None) < 0
        assert lib.rtw_paths_views(None, C.byref(v), 1, C.byref(vp), 0, n, 1, heads.ctypes.data, vertices.ctypes.data, None) < 0
        assert lib.rtw_paths_views_device(None, C.byref(v), 1, C.byref(vp), 0, n, 1, heads.ctypes.data, vertices.ctypes.data, None, None) < 0
    assert lib.rtw_paths(None, None, 0, None, None, None, None) < 0
    assert not heads.view(np.uint8).any() and not vertices.view(np.uint8).any()


# ---------------------------------------------------------------- paths_plan
def test_paths_plan_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "paths_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-o", exe, os.path.join(abi.REPO_DIR, "tests", "native", "paths_plan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "paths_plan_check ok" in out.stdout, out.stdout + out.stderr[-2000:]


# ---------------------------------------------------------------- paths_ref.fold
def records(*contributions):
    v = np.zeros(len(contributions), abi.PATH_VERTEX)
    v["contribution"] = np.array(contributions, np.float32).reshape(-1, 3)
    return v


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def test_fold_is_the_float32_sum_in_order_from_plus_zero_then_the_scrub():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    assert bits(P.fold(records())) == bits([0, 0, 0])
    assert bits(P.fold(records((-0.0, -0.0, 1.5)))) == bits([0.0, 0.0, 1.5])  # +0 + -0 = +0: a -0 never comes back
    # float32, in order: 2^24 + 1 + 1 stays 2^24, 1 + 1 + 2^24 does not
    big = np.float32(2 ** 24)
    assert bits(P.fold(records((big, 1, 0), (1, 1, 0), (1, big, 0)))) == bits([big, big + np.float32(2), 0])
    assert bits(P.fold(records((0.1, 0.2, 0.3), (0.7, 0.1, 0.6)))) == bits([np.float32(0.1) + np.float32(0.7), np.float32(0.2) + np.float32(0.1),
                                                                           np.float32(0.3) + np.float32(0.6)])
    # an inf stays, inf - inf and a NaN channel become 0 - that channel alone, and only at the end (a NaN swallows what follows)
    assert bits(P.fold(records((inf, inf, 1), (1, -inf, nan), (2, 5, 3)))) == bits([inf, 0, 0])
    assert bits(P.fold(records((nan, 0, 0), (4, 4, -4)))) == bits([0, 4, -4])
    assert bits(P.fold(records((3.0e38, -3.0e38, 0), (3.0e38, -3.0e38, 0)))) == bits([inf, -inf, 0])  # overflow is an inf like any other
    # fold_all is fold for every sample, and stops at the sample's segments
    heads = np.zeros((1, 3), abi.PATH_HEAD)
    vertices = np.zeros((1, 3, 3), abi.PATH_VERTEX)
    heads["segments"][0] = (0, 2, 5)
    vertices["contribution"][0, :] = np.array([(inf, 1, -0.0), (-inf, 2, -0.0), (7, nan, 7)], np.float32)
    want = [P.fold(vertices[0, s, :min(int(heads["segments"][0, s]), 3)]) for s in range(3)]
    assert bits(P.fold_all(heads, vertices)[0]) == bits(want) == bits([[0, 0, 0], [0, 3, 0], [0, 0, 7]])
    assert P.complete(heads, vertices).tolist() == [[True, True, False]]
    assert P.written(heads, vertices).tolist() == [[[False] * 3, [True, True, False], [True] * 3]]
    vertices["flags"][0, :, :] = abi.RTW_PATH_LIGHT_SAMPLED | abi.RTW_PATH_SCATTER
    assert P.light_sampled(heads, vertices).tolist() == [[0, 2, 3]] and (P.event(vertices) == abi.RTW_PATH_SCATTER).all()


# ---------------------------------------------------------------- what the Python layer hands to the library
class Recorder:
    """every attribute is a function that appends (name, args) and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


@pytest.fixture
def r():
    r = object.__new__(abi.Renderer)
    r.lib, r.ctx, r.devices = Recorder(), C.c_void_p(0xC0FFEE), [0]
    yield r
    r.ctx = C.c_void_p()  # so that close() calls nothing


def plain(a):
    if hasattr(a, "_obj"):
        return a._obj
    return a.value if isinstance(a, C.c_void_p) else a


def only_call(r, name):
    assert [c[0] for c in r.lib.calls] == [name]
    args = r.lib.calls.pop()[1]
    assert args[0] is r.ctx
    return [plain(a) for a in args[1:]]


def raises(r, text, call, *args, **kw):
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        call(*args, **kw)
    assert r.lib.calls == []


BATCH = np.arange(24, dtype=np.float32).reshape(3, 8)


def paths_bytes(spp, depth, k, seed=0x6314759, rng_kind=0, sample_offset=0, estimator=0, key_offset=0):
    return bytes(abi.PathsParams(spp, depth, seed, rng_kind, sample_offset, estimator, key_offset, k, (C.c_uint32 * 2)(0, 0)))


def test_paths_and_paths_device(r):
    for st in (None, abi.Stats()):
        heads, vertices = r.paths(BATCH, 4, 5, stats=st)
        src, n, p, h, v, stats = only_call(r, "rtw_paths")
        assert (src, n, h, v) == (BATCH.ctypes.data, 3, heads.ctypes.data, vertices.ctypes.data) and (stats is st)
        assert heads.shape == (3, 4) and heads.dtype == abi.PATH_HEAD and vertices.shape == (3, 4, 5) and vertices.dtype == abi.PATH_VERTEX
        assert heads.flags.c_contiguous and vertices.flags.c_contiguous and not vertices.view(np.uint8).any()
        assert type(p) is abi.PathsParams and bytes(p) == paths_bytes(4, 5, 5)
    heads, vertices = r.paths(BATCH, np.int64(7), 6, 2, 2 ** 32 + 9, abi.RTW_RNG_TEA_LCG, 16, 2, 2 ** 32 + 3)
    src, n, p, h, v, stats = only_call(r, "rtw_paths")
    assert vertices.shape == (3, 7, 2) and bytes(p) == paths_bytes(7, 6, 2, 9, 1, 16, 2, 3) and stats is None
    heads, vertices = r.paths(BATCH, 2, 6, 0)  # heads alone: no vertex pointer
    src, n, p, h, v, stats = only_call(r, "rtw_paths")
    assert v is None and h == heads.ctypes.data and vertices.shape == (3, 2, 0) and bytes(p) == paths_bytes(2, 6, 0)
    heads, vertices = r.paths(BATCH, 2, 0)  # no depth: no records either
    assert only_call(r, "rtw_paths")[4] is None and vertices.shape == (3, 2, 0)
    assert [a.shape for a in r.paths(np.zeros((0, 8), np.float32), 2, 3)] == [(0, 2), (0, 2, 3)] and only_call(r, "rtw_paths")[1] == 0
    for bad in (BATCH.tolist(), BATCH.astype(np.float64), None):
        raises(r, "paths: rays must be a float32 numpy array", r.paths, bad, 4, 5)
    raises(r, "paths: rays of shape (3, 7), expected (n, 8)", r.paths, BATCH[:, :7], 0, 5)  # the batch comes first
    for bad in (0, -1, True, 4.0, None):
        raises(r, f"paths: spp = {bad!r}, expected a positive integer", r.paths, BATCH, bad, 5)
    for bad in (-1, 6, True, 2.0, "2"):
        raises(r, f"paths: max_records = {bad!r}, expected an integer in 0 .. max_depth", r.paths, BATCH, 4, 5, bad)
    raises(r, "paths: more than 2^31 - 1 samples in one call", r.paths, BATCH, 2 ** 30, 5, 0)

    for st in (None, abi.Stats()):
        assert r.paths_device(3, 0x10000, 0x20000, 0x30000, 4, 5, stream_ptr=0x70000, stats=st) is None
        src, n, p, h, v, stream, stats = only_call(r, "rtw_paths_device")
        assert (src, n, h, v, stream) == (0x10000, 3, 0x20000, 0x30000, 0x70000) and stats is st and bytes(p) == paths_bytes(4, 5, 5)
    r.paths_device(3, 0x10000, 0x20000, 0, 7, 6, 0, 2 ** 32 + 9, 1, 16, 2, 2 ** 32 + 3)
    src, n, p, h, v, stream, stats = only_call(r, "rtw_paths_device")
    assert (v, stream, stats) == (None, None, None) and bytes(p) == paths_bytes(7, 6, 0, 9, 1, 16, 2, 3)
    raises(r, "paths: spp = 0, expected a positive integer", r.paths_device, 3, 1, 2, 3, 0, 5)
    raises(r, "paths: max_records = 9, expected an integer in 0 .. max_depth", r.paths_device, 3, 1, 2, 3, 4, 5, 9)


def test_paths_views_and_paths_views_device(r):
    views = abi.view_array([abi.make_view(np.arange(24, dtype=np.float32), abi.RTW_CAM_PERSPECTIVE, 5),
                            abi.make_view(np.arange(24, dtype=np.float32) + 1, abi.RTW_CAM_ORTHOGRAPHIC, 6)])
    for st in (None, abi.Stats()):
        heads, vertices = r.paths_views(views, 3, 2, 4, 5, 7, 6, stats=st)
        src, n, p, first, count, k, h, v, stats = only_call(r, "rtw_paths_views")
        assert (src, n, first, count, k, h, v) == (C.addressof(views), 2, 4, 5, 6, heads.ctypes.data, vertices.ctypes.data) and stats is st
        assert heads.shape == (5, 7) and vertices.shape == (5, 7, 6) and not vertices.view(np.uint8).any()
        assert type(p) is abi.ViewParams and bytes(p) == bytes(abi.ViewParams(3, 2, 7, 6, 0, 0, 0, 0))
    heads, vertices = r.paths_views([views[1]], np.int32(3), 2, np.int64(5), 1, 1, 6, 0, 1, 16, 2)
    src, n, p, first, count, k, h, v, stats = only_call(r, "rtw_paths_views")
    assert (n, first, count, k, v, stats) == (1, 5, 1, 0, None, None) and bytes(p) == bytes(abi.ViewParams(3, 2, 1, 6, 1, 16, 2, 0))
    assert heads.shape == (1, 1) and vertices.shape == (1, 1, 0)
    assert [a.shape for a in r.paths_views(views, 3, 2, 12, 0, 2, 3)] == [(0, 2), (0, 2, 3)] and only_call(r, "rtw_paths_views")[4] == 0
    raises(r, "views: expected abi.View records (abi.make_view, abi.scene_view, bake.cube_views, bake.orbit_views)", r.paths_views, [5], 3, 2, 0, 1, 1, 1)
    raises(r, "views: width = 0, expected a positive integer", r.paths_views, views, 0, 2, 0, 1, 1, 1)
    raises(r, "paths_views: more than 2^31 - 1 pixels in one call", r.paths_views, views, 32768, 32768, 0, 1, 1, 1)
    raises(r, "paths_views: pixels [8, 13) of 12", r.paths_views, views, 3, 2, 8, 5, 1, 1)
    raises(r, "paths_views: first = -1, expected a non-negative integer", r.paths_views, views, 3, 2, -1, 5, 1, 1)
    raises(r, "paths_views: count = 1.0, expected a non-negative integer", r.paths_views, views, 3, 2, 0, 1.0, 1, 1)
    raises(r, "paths_views: max_records = 2, expected an integer in 0 .. max_depth", r.paths_views, views, 3, 2, 0, 1, 1, 1, 2)

    assert r.paths_views_device(2, 0x10000, 0x20000, 0x30000, 3, 2, 4, 5, 7, 6, stream_ptr=0x70000) is None
    src, n, p, first, count, k, h, v, stream, stats = only_call(r, "rtw_paths_views_device")
    assert (src, n, first, count, k, h, v, stream, stats) == (0x10000, 2, 4, 5, 6, 0x20000, 0x30000, 0x70000, None)
    assert bytes(p) == bytes(abi.ViewParams(3, 2, 7, 6, 0, 0, 0, 0))
    raises(r, "views: spp = 0, expected a positive integer", r.paths_views_device, 2, 1, 2, 3, 3, 2, 0, 1, 0, 6)


def test_the_torch_wrappers_refuse_before_any_call(r):
    torch = pytest.importorskip("torch")
    from raytracing_weekend_amd.torch_paths import HEAD_COLUMNS, HEAD_FLOATS, VERTEX_COLUMNS, VERTEX_FLOATS, paths_torch, paths_views_torch
    from raytracing_weekend_amd.torch_views import views_tensor

    assert (HEAD_FLOATS, VERTEX_FLOATS) == (8, 16)
    # the columns are the fields' words
    for cols, dt in ((HEAD_COLUMNS, abi.PATH_HEAD), (VERTEX_COLUMNS, abi.PATH_VERTEX)):
        assert list(cols) == list(dt.names)
        assert all((c.start if isinstance(c, slice) else c) * 4 == dt.fields[f][1] for f, c in cols.items())
    batch = torch.from_numpy(BATCH)
    raises(r, "paths_torch: rays of shape (3, 7), expected (n, 8)", paths_torch, r, batch[:, :7], 4, 5)
    raises(r, "paths_torch: rays on cpu, the renderer answers on cuda:0", paths_torch, r, batch, 4, 5)
    views = views_tensor([abi.make_view(np.arange(24, dtype=np.float32))], "cpu")
    raises(r, "paths_views_torch: views of shape (1, 27), expected (n, 28)", paths_views_torch, r, views[:, :27], 3, 2, 0, 1, 1, 1)
    raises(r, "paths_views_torch: views on cpu, the renderer answers on cuda:0", paths_views_torch, r, views, 3, 2, 0, 1, 1, 1)


def test_torch_is_imported_inside_the_functions_only():
    tree = ast.parse(open(os.path.join(abi.PKG_DIR, "torch_paths.py")).read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name.split(".")[0] for n in top if isinstance(n, ast.Import) for a in n.names} | {(n.module or "").split(".")[0] for n in top if isinstance(n, ast.ImportFrom)}
    assert "torch" not in names


# ---------------------------------------------------------------- bake.path_segments
def test_path_segments_are_the_origins_and_the_last_end_point():
    heads = np.zeros((2, 2), abi.PATH_HEAD)
    vertices = np.zeros((2, 2, 3), abi.PATH_VERTEX)
    heads["segments"] = [[2, 0], [5, 1]]  # two records; none; five segments of which three are kept; a miss at once
    vertices["o"][0, 0, :2] = [(0, 0, 0), (1, 2, 3)]
    vertices["d"][0, 0, :2] = [(1, 2, 3), (0, 0, -2)]
    vertices["t"][0, 0, :2] = [1.0, 0.25]
    vertices["o"][1, 0] = [(0, 0, 0), (1, 0, 0), (1, 1, 0)]
    vertices["d"][1, 0, 2] = (0, 0, 4)
    vertices["t"][1, 0, 2] = 0.5
    vertices["o"][1, 1, 0], vertices["d"][1, 1, 0], vertices["t"][1, 1, 0], vertices["prim"][1, 1, 0] = (1, 1, 1), (0, 1, 0), 1e27, -1
    got = bake.path_segments(heads, vertices, miss_length=2.0)
    assert len(got) == 4 and all(g.dtype == np.float32 and g.ndim == 2 and g.shape[1] == 3 for g in got)
    assert got[0].tolist() == [[0, 0, 0], [1, 2, 3], [1, 2, 2.5]] and got[1].shape == (0, 3)
    assert got[2].tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 2]]
    assert got[3].tolist() == [[1, 1, 1], [1, 3, 1]]
    raw = bake.path_segments(heads, vertices)[3]
    assert raw[0].tolist() == [1, 1, 1] and raw[1, 1] == np.float32(1) + np.float32(1e27)  # o + t * d as it is
    with pytest.raises(ValueError):
        bake.path_segments(heads, vertices[:1])
    with pytest.raises(ValueError):
        bake.path_segments(heads.view(np.uint8), vertices)
