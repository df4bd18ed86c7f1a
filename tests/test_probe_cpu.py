"""CPU suite of the probes (include/rtw.h rtw_probe / rtw_probe_device): the additive ABI, the Python surface's argument handling,
probe_ref.directions (the restated direction formula the GPU tests referee with) and bake.rect_probes against the oracle."""
import ast
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import probe_ref as P
from raytracing_weekend_amd import abi, bake

BOTH = (abi.RTW_RNG_PHILOX, abi.RTW_RNG_TEA_LCG)


# ---------------------------------------------------------------- ABI
def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(abi.REPO_DIR, "include", "rtw.h")).read(), flags=re.S)


def test_header_declares_both_entry_points_the_modes_and_the_struct():
    text = " ".join(header().split())
    assert ("int rtw_probe(rtw_ctx* ctx, const float* probes, size_t n, const rtw_probe_params* params, float* rgba_out, "
            "rtw_stats* stats);") in text
    assert ("int rtw_probe_device(rtw_ctx* ctx, const float* probes, size_t n, const rtw_probe_params* params, void* d_rgba, "
            "void* hip_stream, rtw_stats* stats);") in text
    assert "enum { RTW_PROBE_IRRADIANCE = 0, RTW_PROBE_OCCLUSION = 1 };" in text
    fields = re.search(r"typedef struct rtw_probe_params \{(.*?)\} rtw_probe_params;", text).group(1)
    decl = [f.split() for f in fields.split(";") if f.strip()]
    assert [d[-1] for d in decl] == ["spp", "max_depth", "seed", "rng_kind", "sample_offset", "estimator", "key_offset", "mode"]
    assert [d[0] for d in decl] == ["int32_t", "int32_t", "uint32_t", "int32_t", "int32_t", "int32_t", "uint32_t", "int32_t"]
    assert "#define RTW_ABI_VERSION 5" in text  # additive: the version and the older structs stay


def test_params_mirror_the_struct_and_the_older_structs_keep_their_sizes():
    assert C.sizeof(abi.ProbeParams) == 32
    assert [f for f, _ in abi.ProbeParams._fields_] == ["spp", "max_depth", "seed", "rng_kind", "sample_offset", "estimator", "key_offset", "mode"]
    assert abi.PROBE_MODES == {"irradiance": 0, "occlusion": 1}
    assert abi.RTW_ABI_VERSION == 5 and C.sizeof(abi.Stats) == 184 and C.sizeof(abi.Params) == 48 and C.sizeof(abi.RadianceParams) == 32


def test_symbols_are_listed_and_exported():
    assert "rtw_probe" in abi.HIP_SYMBOLS and "rtw_probe_device" in abi.HIP_SYMBOLS
    lib = abi.load_hip()
    assert hasattr(lib, "rtw_probe") and hasattr(lib, "rtw_probe_device") and lib.rtw_abi_version() == 5


def test_null_context_is_an_error_not_a_crash():
    lib = abi.load_hip()
    probes, out = np.zeros((4, 8), np.float32), np.zeros((4, 4), np.float32)
    for mode in abi.PROBE_MODES:
        pp = abi.make_probe_params(4, 4, mode=mode)
        for n in (0, 4):
            assert lib.rtw_probe(None, probes.ctypes.data, n, C.byref(pp), out.ctypes.data, None) < 0
            assert lib.rtw_probe_device(None, probes.ctypes.data, n, C.byref(pp), out.ctypes.data, None, None) < 0
    assert lib.rtw_probe(None, None, 0, None, None, None) < 0
    assert not out.any()


def test_the_kernels_are_a_unit_of_the_build_with_the_common_flags():
    entry = open(os.path.join(abi.REPO_DIR, "__graft_entry__.py")).read()
    assert '("rtw_probe.hip", "rtw_probe.o", [])' in entry and '"rtw_probe.hip"' not in entry.split("UNIT_FLAGS = ")[1].split("\n")[0]
    assert entry.index('("rtw_radiance.hip", "rtw_radiance.o", [])') < entry.index('("rtw_probe.hip", "rtw_probe.o", [])')
    hip = open(os.path.join(abi.PKG_DIR, "csrc", "rtw_hip.hip")).read()
    assert '#include "rtw_probe.hip"' not in hip  # (a translation unit of its own, in no other)
    assert hip.count("return guarded(c, [&] { return impl_probe") == 2
    # the two kernels share their body: one piece of source, not a copy
    csrc = os.path.join(abi.PKG_DIR, "csrc")
    body, rad, probe = (open(os.path.join(csrc, f)).read() for f in ("rtw_radiance_body.h", "rtw_radiance.hip", "rtw_probe.hip"))
    assert "RTW_RADIANCE_BODY(false)" in rad and "RTW_RADIANCE_BODY(true)" in probe
    assert body.count("shade_a<KIND, TEX>") == 1 and "shade_a<" not in rad and "shade_a<" not in probe


# ---------------------------------------------------------------- the Python surface
class NoLibrary:
    """A Renderer that must refuse before it reaches the library."""
    ctx = None

    class lib:
        @staticmethod
        def rtw_probe(*a):
            raise AssertionError("the library was called")


def test_python_side_argument_validation():
    call = abi.Renderer.probe
    good = np.zeros((5, 8), np.float32)
    for probes in (np.zeros((5, 7), np.float32), np.zeros(8, np.float32), np.zeros((5, 8, 1), np.float32),  # shape
                   np.zeros((5, 8), np.float64), np.zeros((5, 8), np.int32), [[0.0] * 8]):                   # dtype
        with pytest.raises(ValueError):
            call(NoLibrary, probes, 4, 4)
    for spp in (0, -3, 1.5, None, True):
        with pytest.raises(ValueError):
            call(NoLibrary, good, spp, 4)
    for mode in ("ao", 0, None, "IRRADIANCE"):
        with pytest.raises(ValueError):
            call(NoLibrary, good, 4, 4, mode=mode)
    pp = abi.make_probe_params(7, 3, seed=9, rng_kind=1, sample_offset=16, estimator=2, key_offset=2 ** 32 - 3, mode="occlusion")
    assert (pp.spp, pp.max_depth, pp.seed, pp.rng_kind, pp.sample_offset, pp.estimator, pp.key_offset, pp.mode) == (7, 3, 9, 1, 16, 2, 2 ** 32 - 3, 1)
    assert abi.make_probe_params(1, 0).mode == 0


def test_torch_is_imported_inside_the_function_only():
    for name in ("torch_probe.py", "bake.py"):
        tree = ast.parse(open(os.path.join(abi.PKG_DIR, name)).read())
        top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
        names = {a.name.split(".")[0] for n in top if isinstance(n, ast.Import) for a in n.names} | {(n.module or "").split(".")[0] for n in top if isinstance(n, ast.ImportFrom)}
        assert "torch" not in names, name
    from raytracing_weekend_amd import torch_probe
    assert callable(torch_probe.probe_torch)


# ---------------------------------------------------------------- probe_ref.directions
def normals64():
    """64 normals: the axes, both sides of the |w.x| > 0.9 switch of the basis, non-unit lengths, the rest random."""
    fixed = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
             (0.95, 0.2, 0.24), (-0.95, 0.2, 0.24), (0.89, 0.3, 0.34), (-0.89, 0.3, 0.34), (0.91, -0.4, 0.1), (-0.899, 0.0, 0.44),
             (3e-3, 4e-3, 0.0), (0.0, 700.0, 100.0), (9e4, 1e4, -2e4), (-2.0, 0.5, 0.5)]
    rnd = np.random.default_rng(5).normal(size=(64 - len(fixed), 3)) * np.random.default_rng(6).uniform(0.1, 10.0, size=(64 - len(fixed), 1))
    n = np.concatenate([np.array(fixed, np.float64), rnd]).astype(np.float32)
    unit_x = n[:, 0].astype(np.float64) / np.linalg.norm(n.astype(np.float64), axis=1)
    assert (np.abs(unit_x) > 0.9).sum() >= 6 and (unit_x > 0.9).any() and (unit_x < -0.9).any() and (np.abs(unit_x) < 0.9).sum() >= 40
    return n


def probes_of(normals):
    p = np.zeros((len(normals), 8), np.float32)
    p[:, 3:6] = normals
    p[:, 6], p[:, 7] = 1e-6, 1e27
    return p


@pytest.mark.parametrize("rng_kind", BOTH)
def test_directions_are_unit_cosine_weighted_and_on_the_normals_side(rng_kind):
    n = normals64()
    d = P.directions(probes_of(n), 1024, rng_kind=rng_kind, key_offset=11).astype(np.float64)
    assert d.shape == (64, 1024, 3)
    length = np.sqrt((d * d).sum(-1))
    assert np.abs(length - 1.0).max() <= 2 * 2.0 ** -23, np.abs(length - 1.0).max()  # within 2 float32 ulps of 1
    nh = n.astype(np.float64) / np.linalg.norm(n.astype(np.float64), axis=1, keepdims=True)
    cos = (d * nh[:, None, :]).sum(-1)
    assert (cos > 0.0).all(), cos.min()
    # E[cos] = 2/3 under the density cos / pi, variance 1/18: the standard error over 65 536 samples is 9.2e-4, the bound five of them
    print(f"rng {rng_kind}: mean cosine {cos.mean():.6f} (2/3 = {2 / 3:.6f}), min {cos.min():.3e}, max |length - 1| {np.abs(length - 1.0).max():.3e}")
    assert abs(cos.mean() - 2.0 / 3.0) <= 4.6e-3


@pytest.mark.parametrize("rng_kind", BOTH)
def test_directions_depend_on_key_and_sample_index_alone(rng_kind):
    p = probes_of(normals64()[:20])
    whole = P.directions(p, 32, rng_kind=rng_kind, key_offset=3)
    assert np.array_equal(P.directions(p, 16, rng_kind=rng_kind, key_offset=3, sample_offset=16).view(np.uint32), whole[:, 16:].view(np.uint32))
    assert len(np.unique(whole.reshape(-1, 3).view(np.uint32), axis=0)) == whole.shape[0] * whole.shape[1]
    # probe i at key offset K is probe 0 at K + i, across the 2^32 wrap as well
    same_normal = probes_of(np.repeat(normals64()[7:8], 6, 0))
    for k0 in (40, 2 ** 32 - 3):
        batch = P.directions(same_normal, 8, rng_kind=rng_kind, key_offset=k0)
        for i in range(6):
            one = P.directions(same_normal[:1], 8, rng_kind=rng_kind, key_offset=(k0 + i) & 0xffffffff)
            assert np.array_equal(one[0].view(np.uint32), batch[i].view(np.uint32)), (k0, i)
        assert not np.array_equal(batch[0], batch[1])
    if rng_kind == abi.RTW_RNG_PHILOX:  # (tea<64>(key, sample) takes no seed)
        assert not np.array_equal(P.directions(p[:2], 4, seed=1, rng_kind=rng_kind), P.directions(p[:2], 4, seed=2, rng_kind=rng_kind))


# ---------------------------------------------------------------- bake.rect_probes
RECTS = (abi.PRIM_RECT_X, abi.PRIM_RECT_Y, abi.PRIM_RECT_Z)


def coincident(parts, prim, points):
    """The other rectangles that contain every one of the world-space `points` (within 1e-4 of their plane, inside their bounds)."""
    out = []
    for q, p in enumerate(parts["prims"]):
        if q == prim or p.type not in RECTS:
            continue
        inv = np.array(list(parts["xforms"][p.xform].inv), np.float64).reshape(3, 4)
        obj = points @ inv[:, :3].T + inv[:, 3]
        k, a, b = {abi.PRIM_RECT_X: (0, 1, 2), abi.PRIM_RECT_Y: (1, 0, 2), abi.PRIM_RECT_Z: (2, 0, 1)}[p.type]
        if (np.abs(obj[:, k] - p.p[4]) < 1e-4).all() and (obj[:, a] >= p.p[0]).all() and (obj[:, a] <= p.p[1]).all() \
                and (obj[:, b] >= p.p[2]).all() and (obj[:, b] <= p.p[3]).all():
            out.append(q)
    return out


def test_rect_probes_sit_on_their_rectangle_and_on_no_other():
    blob = abi.build_scene(0, 32, 32)
    parts = abi.parse_scene(blob)
    prims, ties = parts["prims"], {}
    rects = [i for i, p in enumerate(prims) if p.type in RECTS]
    assert len(rects) >= 6 and any(prims[i].xform != 0 for i in rects)  # the walls and the rotated boxes' sides
    nu, nv, offset = 5, 3, 1e-3
    for prim in rects:
        for side in (1, -1):
            pr = bake.rect_probes(blob, prim, nu, nv, side=side, offset=offset)
            assert pr.shape == (nv * nu, 8) and pr.dtype == np.float32
            assert np.all(pr[:, 6] == np.float32(1e-6)) and np.all(pr[:, 7] == np.float32(1e27))
            length = np.sqrt((pr[:, 3:6].astype(np.float64) ** 2).sum(1))
            assert np.abs(length - 1.0).max() <= 2 * 2.0 ** -23
            back = pr.copy()
            back[:, 3:6] = -pr[:, 3:6]
            back[:, 6], back[:, 7] = 0.0, 2 * offset
            t, hit = oracle.intersect(blob, back)
            foot = pr[:, 0:3].astype(np.float64) - offset * pr[:, 3:6].astype(np.float64)
            twins = coincident(parts, prim, foot)
            # that primitive and no other - except where another rectangle occupies the very same points (the rotated box stands
            # on the floor: its bottom face lies in the floor's plane, and a closest hit at equal t goes to the lower index)
            assert np.array_equal(hit, np.full(nv * nu, min([prim] + twins), np.int32)), (prim, side, hit, twins)
            ties[prim] = twins
            assert np.abs(t - offset).max() < 2e-4  # the foot lies `offset` below, up to the rounding of coordinates of a few hundred
        both = bake.rect_probes(blob, prim, nu, nv), bake.rect_probes(blob, prim, nu, nv, side=-1)
        assert np.array_equal(both[0][:, 3:6], -both[1][:, 3:6])
    assert sum(1 for v in ties.values() if v) <= 1  # the one box face on the floor: every other rectangle is hit alone
    spheres = [i for i, p in enumerate(prims) if p.type == abi.PRIM_SPHERE]
    assert spheres
    for bad in (spheres[0], -1, len(prims)):
        with pytest.raises(ValueError):
            bake.rect_probes(blob, bad, 4, 4)
    with pytest.raises(ValueError):
        bake.rect_probes(blob, rects[0], 0, 4)
