"""What abi.Renderer's query-family methods and the *_torch wrappers hand to the library, without a GPU: a Renderer made with
object.__new__ whose `lib` records every call. For each method the C function, the scalars, the bytes of every struct passed by
reference, the pointers (those of the arrays returned or given), the NULL-ness of stats, and every ValueError of the Python layer
with its full text - none of which may reach the library."""
import ctypes as C
import re

import numpy as np
import pytest

from raytracing_weekend_amd import abi

SEED = 0x6314759
CTX = 0xC0FFEE


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
    r.lib, r.ctx, r.devices = Recorder(), C.c_void_p(CTX), [0]
    yield r
    r.ctx = C.c_void_p()  # so that close() calls nothing


def plain(a):
    """an argument as the library would see it: a by-reference struct as the struct, a pointer as its integer, NULL as None"""
    if hasattr(a, "_obj"):
        return a._obj
    if isinstance(a, C.c_void_p):
        return a.value
    return a


def only_call(r, name):
    """the arguments after the context of the one call recorded, which went to `name`"""
    assert [c[0] for c in r.lib.calls] == [name]
    args = r.lib.calls.pop()[1]
    assert args[0] is r.ctx
    return [plain(a) for a in args[1:]]


def raises(r, text, call, *args, **kw):
    """`call` raises ValueError with exactly this text, and the library hears nothing"""
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        call(*args, **kw)
    assert r.lib.calls == []


def is_array(a, shape, dtype):
    return isinstance(a, np.ndarray) and a.shape == shape and a.dtype == dtype and a.flags.c_contiguous


def fields(s):
    return {k: getattr(s, k) for k, _ in s._fields_}


def stats_cases():
    return (None, abi.Stats())


def stats_ok(arg, st):
    return arg is None if st is None else arg is st


BATCH = np.arange(24, dtype=np.float32).reshape(3, 8)
TIMES = np.arange(3, dtype=np.float32)
PTR = {"in": 0x10000, "out": 0x20000, "spp": 0x30000, "err": 0x40000, "a": 0x50000, "b": 0x60000, "stream": 0x70000}


def views2():
    return abi.view_array([abi.make_view(np.arange(24, dtype=np.float32), abi.RTW_CAM_PERSPECTIVE, 5),
                           abi.make_view(np.arange(24, dtype=np.float32) + 1, abi.RTW_CAM_ORTHOGRAPHIC, 2 ** 32 + 6)])


# ---------------------------------------------------------------- cast, debug_intersect
def test_cast(r):
    for st in stats_cases():
        out = r.cast(BATCH, TIMES, None, stats=st)
        rays, rt, gt, n, mode, hits, stats = only_call(r, "rtw_cast")
        assert (rays, rt, gt, n, mode) == (BATCH.ctypes.data, TIMES.ctypes.data, None, 3, 0) and stats_ok(stats, st)
        assert list(out) == ["t", "prim", "material", "normal", "uv"]
        assert is_array(out["t"], (3,), np.float32) and is_array(out["prim"], (3,), np.int32) and is_array(out["material"], (3,), np.int32)
        assert is_array(out["normal"], (3, 4), np.float32) and is_array(out["uv"], (3, 2), np.float32)
        assert isinstance(hits, abi.Hits) and fields(hits) == {k: v.ctypes.data for k, v in out.items()}
    out = r.cast(BATCH.astype(np.float64).tolist(), None, [0.0, 1.0, 2.0], mode="any", want=("uv", "prim", "t"))  # converted, not refused
    rays, rt, gt, n, mode, hits, stats = only_call(r, "rtw_cast")
    assert rays and rt is None and gt and (n, mode, stats) == (3, 1, None)
    assert list(out) == ["t", "prim"] and fields(hits) == {"t": out["t"].ctypes.data, "prim": out["prim"].ctypes.data, "material": None,
                                                           "normal": None, "uv": None}
    assert r.cast(np.zeros((0, 8), np.float32), want=("uv",))["uv"].shape == (0, 2)
    assert only_call(r, "rtw_cast")[3] == 0
    raises(r, "cast: mode 'nearest' is neither 'closest' nor 'any'", r.cast, BATCH, mode="nearest")
    raises(r, "cast: unknown or no output names ['z']", r.cast, BATCH, want=("t", "z"))
    raises(r, "cast: unknown or no output names ()", r.cast, BATCH, want=())
    raises(r, "cast: mode 'any' has t and prim only, not ('normal', 'uv')", r.cast, BATCH, mode="any", want=("normal", "uv"))
    raises(r, "cast: rays of shape (3, 7), expected (n, 8)", r.cast, BATCH[:, :7])
    raises(r, "cast: rays of shape (24,), expected (n, 8)", r.cast, BATCH.ravel())
    raises(r, "cast: times of shape (2,) for 3 rays", r.cast, BATCH, TIMES[:2])
    raises(r, "cast: times of shape (3, 1) for 3 rays", r.cast, BATCH, None, TIMES[:, None])
    raises(r, "cast: mode 'x' is neither 'closest' nor 'any'", r.cast, BATCH[:, :7], mode="x")  # the names come first


def test_cast_device(r):
    for st in stats_cases():
        assert r.cast_device(3, PTR["in"], {"prim": PTR["out"], "uv": PTR["a"]}, PTR["b"], mode="any", stream_ptr=PTR["stream"], stats=st) is None
        rays, rt, gt, n, mode, hits, stream, stats = only_call(r, "rtw_cast_device")
        assert (rays, rt, gt, n, mode, stream) == (PTR["in"], PTR["b"], None, 3, 1, PTR["stream"]) and stats_ok(stats, st)
        assert fields(hits) == {"t": None, "prim": PTR["out"], "material": None, "normal": None, "uv": PTR["a"]}
    r.cast_device(0, 0, {})
    assert only_call(r, "rtw_cast_device")[:5] == [None, None, None, 0, 0]


def test_debug_intersect(r):
    t, prim = r.debug_intersect(BATCH, None, TIMES)
    rays, rt, gt, n, tp, pp = only_call(r, "rtw_debug_intersect")
    assert (rays, rt, gt, n, tp, pp) == (BATCH.ctypes.data, None, TIMES.ctypes.data, 3, t.ctypes.data, prim.ctypes.data)
    assert is_array(t, (3,), np.float32) and is_array(prim, (3,), np.int32)
    t, prim = r.debug_intersect(BATCH.astype(np.float64), [0, 0, 0])  # converted, not refused
    rays, rt, gt, n, tp, pp = only_call(r, "rtw_debug_intersect")
    assert rays and rays != BATCH.ctypes.data and rt and gt is None and n == 3 and is_array(t, (3,), np.float32)


# ---------------------------------------------------------------- radiance, probe, probe_sh: (n, 8) in, one array out
def params_bytes(kind, spp, depth, seed=SEED, rng_kind=0, sample_offset=0, estimator=0, key_offset=0, last=0):
    return bytes(kind(spp, depth, seed, rng_kind, sample_offset, estimator, key_offset, last))


ONE_OUT = (("radiance", "rays", abi.RadianceParams, (4,), "radiance", {}, 0),
           ("probe", "probes", abi.ProbeParams, (4,), "probe", {"mode": "occlusion"}, 1),
           ("probe_sh", "points", abi.RadianceParams, (9, 4), "radiance", {}, 0))


@pytest.mark.parametrize("method,what,kind,tail,params_prefix,extra,last", ONE_OUT, ids=[c[0] for c in ONE_OUT])
def test_one_output_families(r, method, what, kind, tail, params_prefix, extra, last):
    call, c_name = getattr(r, method), "rtw_" + method
    for st in stats_cases():
        out = call(BATCH, 4, 5, stats=st)
        src, n, p, dst, stats = only_call(r, c_name)
        assert (src, n, dst) == (BATCH.ctypes.data, 3, out.ctypes.data) and is_array(out, (3,) + tail, np.float32) and stats_ok(stats, st)
        assert type(p) is kind and bytes(p) == params_bytes(kind, 4, 5)
    out = call(np.zeros((6, 8), np.float32)[::2], np.int64(7), 0, 2 ** 32 + 9, abi.RTW_RNG_TEA_LCG, 16, 2, 2 ** 32 + 3, **extra)
    src, n, p, dst, stats = only_call(r, c_name)
    assert src and (n, dst, stats) == (3, out.ctypes.data, None) and bytes(p) == params_bytes(kind, 7, 0, 9, 1, 16, 2, 3, last)
    assert call(np.zeros((0, 8), np.float32), 1, 1).shape == (0,) + tail
    assert only_call(r, c_name)[1] == 0
    for bad in (BATCH.tolist(), BATCH.astype(np.float64), BATCH.astype(np.int32), None):
        raises(r, f"{method}: {what} must be a float32 numpy array", call, bad, 4, 5)
    raises(r, f"{method}: {what} of shape (3, 7), expected (n, 8)", call, BATCH[:, :7], 4, 5)
    raises(r, f"{method}: {what} of shape (24,), expected (n, 8)", call, BATCH.ravel(), 4, 5)
    raises(r, f"{method}: {what} of shape (3, 7), expected (n, 8)", call, BATCH[:, :7], 0, 5)  # the batch comes first
    for bad in (0, -1, True, 4.0, "4", None):
        raises(r, f"{params_prefix}: spp = {bad!r}, expected a positive integer", call, BATCH, bad, 5)
    if method == "probe":
        raises(r, "probe: mode 'ao' is neither 'irradiance' nor 'occlusion'", call, BATCH, 4, 5, mode="ao")

    dev = getattr(r, method + "_device")
    for st in stats_cases():
        assert dev(3, PTR["in"], PTR["out"], 4, 5, stream_ptr=PTR["stream"], stats=st) is None
        src, n, p, dst, stream, stats = only_call(r, c_name + "_device")
        assert (src, n, dst, stream) == (PTR["in"], 3, PTR["out"], PTR["stream"]) and stats_ok(stats, st)
        assert type(p) is kind and bytes(p) == params_bytes(kind, 4, 5)
    dev(3, PTR["in"], PTR["out"], 7, 0, 2 ** 32 + 9, abi.RTW_RNG_TEA_LCG, 16, 2, 2 ** 32 + 3, **extra)
    src, n, p, dst, stream, stats = only_call(r, c_name + "_device")
    assert (stream, stats) == (None, None) and bytes(p) == params_bytes(kind, 7, 0, 9, 1, 16, 2, 3, last)
    raises(r, f"{params_prefix}: spp = 0, expected a positive integer", dev, 3, PTR["in"], PTR["out"], 0, 5)
    if method == "probe":
        raises(r, "probe: mode 'ao' is neither 'irradiance' nor 'occlusion'", dev, 3, PTR["in"], PTR["out"], 4, 5, mode="ao")


# ---------------------------------------------------------------- probe_adaptive
def test_probe_adaptive(r):
    for st in stats_cases():
        got = r.probe_adaptive(BATCH, 256, 5, 0.05, stats=st)
        src, n, p, ad, out, spp, err, stats = only_call(r, "rtw_probe_adaptive")
        assert (src, n) == (BATCH.ctypes.data, 3) and (out, spp, err) == tuple(a.ctypes.data for a in got) and stats_ok(stats, st)
        assert isinstance(got, tuple) and is_array(got[0], (3, 4), np.float32) and is_array(got[1], (3,), np.int32) and is_array(got[2], (3,), np.float32)
        assert type(p) is abi.ProbeParams and bytes(p) == params_bytes(abi.ProbeParams, 256, 5)
        assert type(ad) is abi.Adaptive and bytes(ad) == bytes(abi.Adaptive(64, 0, 0.05, 0))
    r.probe_adaptive(BATCH, 128, 3, 0.25, 32, 16, 2 ** 32 + 9, 1, 16, 2, 2 ** 32 + 3, "occlusion")
    src, n, p, ad, out, spp, err, stats = only_call(r, "rtw_probe_adaptive")
    assert bytes(p) == params_bytes(abi.ProbeParams, 128, 3, 9, 1, 16, 2, 3, 1) and bytes(ad) == bytes(abi.Adaptive(32, 16, 0.25, 0)) and stats is None
    assert [a.shape for a in r.probe_adaptive(np.zeros((0, 8), np.float32), 16, 1, 0.1)] == [(0, 4), (0,), (0,)]
    assert only_call(r, "rtw_probe_adaptive")[1] == 0
    for bad in (BATCH.tolist(), BATCH.astype(np.float64)):
        raises(r, "probe_adaptive: probes must be a float32 numpy array", r.probe_adaptive, bad, 256, 5, 0.05)
    raises(r, "probe_adaptive: probes of shape (3, 7), expected (n, 8)", r.probe_adaptive, BATCH[:, :7], 0, 5, 0.05)
    for bad in (0, True, 16.0):
        raises(r, f"probe: spp = {bad!r}, expected a positive integer", r.probe_adaptive, BATCH, bad, 5, 0.05)
    raises(r, "probe: mode 'ao' is neither 'irradiance' nor 'occlusion'", r.probe_adaptive, BATCH, 256, 5, 0.05, mode="ao")

    for st in stats_cases():
        assert r.probe_adaptive_device(3, PTR["in"], PTR["out"], PTR["spp"], 0, 256, 5, 0.05, stream_ptr=PTR["stream"], stats=st) is None
        src, n, p, ad, out, spp, err, stream, stats = only_call(r, "rtw_probe_adaptive_device")
        assert (src, n, out, spp, err, stream) == (PTR["in"], 3, PTR["out"], PTR["spp"], None, PTR["stream"]) and stats_ok(stats, st)
        assert bytes(p) == params_bytes(abi.ProbeParams, 256, 5) and bytes(ad) == bytes(abi.Adaptive(64, 0, 0.05, 0))
    r.probe_adaptive_device(3, PTR["in"], PTR["out"], PTR["spp"], PTR["err"], 128, 3, 0.25, 32, 16, 2 ** 32 + 9, 1, 16, 2, 2 ** 32 + 3, "occlusion")
    src, n, p, ad, out, spp, err, stream, stats = only_call(r, "rtw_probe_adaptive_device")
    assert bytes(p) == params_bytes(abi.ProbeParams, 128, 3, 9, 1, 16, 2, 3, 1) and bytes(ad) == bytes(abi.Adaptive(32, 16, 0.25, 0))
    assert (err, stream, stats) == (PTR["err"], None, None)
    raises(r, "probe: spp = 0, expected a positive integer", r.probe_adaptive_device, 3, PTR["in"], PTR["out"], 0, 0, 0, 5, 0.05)


# ---------------------------------------------------------------- views, views_adaptive, views_guides, denoise_views
def view_params_bytes(w, h, spp, depth, rng_kind=0, sample_offset=0, estimator=0):
    return bytes(abi.ViewParams(w, h, spp, depth, rng_kind, sample_offset, estimator, 0))


NOT_VIEWS = "views: expected abi.View records (abi.make_view, abi.scene_view, bake.cube_views, bake.orbit_views)"


def size_refusals(r, prefix, call, views):
    """what every host call on views refuses before the library: bad records, bad sizes, too many pixels - in this order"""
    raises(r, NOT_VIEWS, *call(views=[views[0], 5]))
    raises(r, NOT_VIEWS, *call(views=[views[0], 5], width=0))
    for name in ("width", "height", "spp"):
        for bad in (0, -2, True, 3.0):
            raises(r, f"views: {name} = {bad!r}, expected a positive integer", *call(**{name: bad}))
    raises(r, "views: width = 0, expected a positive integer", *call(width=0, height=0, spp=0))
    raises(r, f"{prefix}: more than 2^31 - 1 pixels in one call", *call(width=32768, height=32768))
    raises(r, "views: spp = 0, expected a positive integer", *call(width=32768, height=32768, spp=0))


def test_views(r):
    views = views2()
    for st in stats_cases():
        out = r.views(views, 3, 2, 4, 5, stats=st)
        src, n, p, dst, stats = only_call(r, "rtw_views")
        assert (src, n, dst) == (C.addressof(views), 2, out.ctypes.data) and is_array(out, (2, 2, 3, 4), np.float32) and stats_ok(stats, st)
        assert type(p) is abi.ViewParams and bytes(p) == view_params_bytes(3, 2, 4, 5)
    out = r.views([views[1]], np.int32(3), np.int64(2), 4, 0, 1, 16, 2)
    src, n, p, dst, stats = only_call(r, "rtw_views")
    assert src and (n, dst, stats) == (1, out.ctypes.data, None) and out.shape == (1, 2, 3, 4) and bytes(p) == view_params_bytes(3, 2, 4, 0, 1, 16, 2)
    assert r.views(views[0], 3, 2, 4, 5).shape == (1, 2, 3, 4) and only_call(r, "rtw_views")[1] == 1  # one View is a batch of one
    assert r.views([], 3, 2, 4, 5).shape == (0, 2, 3, 4) and only_call(r, "rtw_views")[1] == 0
    size_refusals(r, "views", lambda views=views, width=3, height=2, spp=4: (r.views, views, width, height, spp, 5), views)

    for st in stats_cases():
        assert r.views_device(2, PTR["in"], PTR["out"], 3, 2, 4, 5, stream_ptr=PTR["stream"], stats=st) is None
        src, n, p, dst, stream, stats = only_call(r, "rtw_views_device")
        assert (src, n, dst, stream) == (PTR["in"], 2, PTR["out"], PTR["stream"]) and stats_ok(stats, st) and bytes(p) == view_params_bytes(3, 2, 4, 5)
    r.views_device(2, PTR["in"], PTR["out"], 3, 2, 4, 0, 1, 16, 2)
    src, n, p, dst, stream, stats = only_call(r, "rtw_views_device")
    assert (stream, stats) == (None, None) and bytes(p) == view_params_bytes(3, 2, 4, 0, 1, 16, 2)
    raises(r, "views: height = 0, expected a positive integer", r.views_device, 2, PTR["in"], PTR["out"], 3, 0, 4, 5)


def test_views_adaptive(r):
    views = views2()
    for st in stats_cases():
        got = r.views_adaptive(views, 3, 2, 256, 5, 0.05, stats=st)
        src, n, p, ad, out, spp, err, stats = only_call(r, "rtw_views_adaptive")
        assert (src, n) == (C.addressof(views), 2) and (out, spp, err) == tuple(a.ctypes.data for a in got) and stats_ok(stats, st)
        assert isinstance(got, tuple) and is_array(got[0], (2, 2, 3, 4), np.float32) and is_array(got[1], (2, 2, 3), np.int32)
        assert is_array(got[2], (2, 2, 3), np.float32)
        assert type(p) is abi.ViewParams and bytes(p) == view_params_bytes(3, 2, 256, 5)
        assert type(ad) is abi.Adaptive and bytes(ad) == bytes(abi.Adaptive(64, 0, 0.05, 1))
    r.views_adaptive(list(views), 3, 2, 128, 3, 0.25, 32, 16, 0, 1, 16, 2)
    src, n, p, ad, out, spp, err, stats = only_call(r, "rtw_views_adaptive")
    assert n == 2 and bytes(p) == view_params_bytes(3, 2, 128, 3, 1, 16, 2) and bytes(ad) == bytes(abi.Adaptive(32, 16, 0.25, 0)) and stats is None
    assert [a.shape for a in r.views_adaptive([], 3, 2, 16, 1, 0.1)] == [(0, 2, 3, 4), (0, 2, 3), (0, 2, 3)]
    assert only_call(r, "rtw_views_adaptive")[1] == 0
    size_refusals(r, "views_adaptive", lambda views=views, width=3, height=2, spp=256: (r.views_adaptive, views, width, height, spp, 5, 0.05), views)

    for st in stats_cases():
        assert r.views_adaptive_device(2, PTR["in"], PTR["out"], PTR["spp"], 0, 3, 2, 256, 5, 0.05, stream_ptr=PTR["stream"], stats=st) is None
        src, n, p, ad, out, spp, err, stream, stats = only_call(r, "rtw_views_adaptive_device")
        assert (src, n, out, spp, err, stream) == (PTR["in"], 2, PTR["out"], PTR["spp"], None, PTR["stream"]) and stats_ok(stats, st)
        assert bytes(p) == view_params_bytes(3, 2, 256, 5) and bytes(ad) == bytes(abi.Adaptive(64, 0, 0.05, 1))
    r.views_adaptive_device(2, PTR["in"], PTR["out"], PTR["spp"], PTR["err"], 3, 2, 128, 3, 0.25, 32, 16, 0, 1, 16, 2)
    src, n, p, ad, out, spp, err, stream, stats = only_call(r, "rtw_views_adaptive_device")
    assert bytes(p) == view_params_bytes(3, 2, 128, 3, 1, 16, 2) and bytes(ad) == bytes(abi.Adaptive(32, 16, 0.25, 0))
    assert (err, stream, stats) == (PTR["err"], None, None)
    raises(r, "views: spp = 0, expected a positive integer", r.views_adaptive_device, 2, PTR["in"], PTR["out"], 0, 0, 3, 2, 0, 5, 0.05)


GUIDE_SHAPES = {"albedo": ((4,), np.float32), "normal": ((4,), np.float32), "depth": ((), np.float32), "prim": ((), np.int32)}


def guides_ok(out, g, which, lead):
    assert list(out) == list(which) and isinstance(g, abi.Guides)
    assert all(is_array(out[k], lead + GUIDE_SHAPES[k][0], GUIDE_SHAPES[k][1]) for k in which)
    assert fields(g) == {k: (out[k].ctypes.data if k in which else None) for k in abi.GUIDES}
    return True


def test_views_guides(r):
    views = views2()
    for st in stats_cases():
        out = r.views_guides(views, 3, 2, stats=st)
        src, n, p, g, stats = only_call(r, "rtw_views_guides")
        assert (src, n) == (C.addressof(views), 2) and stats_ok(stats, st) and guides_ok(out, g, abi.GUIDES, (2, 2, 3))
        assert type(p) is abi.ViewParams and bytes(p) == view_params_bytes(3, 2, 16, 0)  # max_depth 0, estimator 0
    out = r.views_guides(list(views), 3, 2, 4, ["prim"], 1, 16)
    src, n, p, g, stats = only_call(r, "rtw_views_guides")
    assert n == 2 and stats is None and guides_ok(out, g, ("prim",), (2, 2, 3)) and bytes(p) == view_params_bytes(3, 2, 4, 0, 1, 16, 0)
    out = r.views_guides([], 3, 2, which=("depth", "albedo"))
    assert guides_ok(out, only_call(r, "rtw_views_guides")[3], ("depth", "albedo"), (0, 2, 3))
    raises(r, "views_guides: unknown or no guide names ['colour']", r.views_guides, views, 3, 2, which=("depth", "colour"))
    raises(r, "views_guides: unknown or no guide names ()", r.views_guides, views, 3, 2, which=())
    raises(r, "views_guides: unknown or no guide names ['x']", r.views_guides, [5], 0, 2, which=("x",))  # the names come first
    size_refusals(r, "views_guides", lambda views=views, width=3, height=2, spp=16: (r.views_guides, views, width, height, spp), views)

    for st in stats_cases():
        assert r.views_guides_device(2, PTR["in"], {"depth": PTR["a"], "albedo": PTR["b"]}, 3, 2, stream_ptr=PTR["stream"], stats=st) is None
        src, n, p, g, stream, stats = only_call(r, "rtw_views_guides_device")
        assert (src, n, stream) == (PTR["in"], 2, PTR["stream"]) and stats_ok(stats, st) and bytes(p) == view_params_bytes(3, 2, 16, 0)
        assert isinstance(g, abi.Guides) and fields(g) == {"albedo": PTR["b"], "normal": None, "depth": PTR["a"], "prim": None}
    r.views_guides_device(2, PTR["in"], {"prim": np.int64(PTR["a"])}, 3, 2, 4, 1, 16)
    src, n, p, g, stream, stats = only_call(r, "rtw_views_guides_device")
    assert (stream, stats) == (None, None) and bytes(p) == view_params_bytes(3, 2, 4, 0, 1, 16, 0) and g.prim == PTR["a"]
    raises(r, "views_guides_device: unknown guide names ['colour']", r.views_guides_device, 2, PTR["in"], {"depth": 1, "colour": 2}, 3, 2)
    raises(r, "views_guides_device: unknown guide names ['x']", r.views_guides_device, 2, PTR["in"], {"x": 2}, 0, 2)  # the names come first
    raises(r, "views: width = 0, expected a positive integer", r.views_guides_device, 2, PTR["in"], {"depth": 1}, 0, 2)


def test_denoise_views(r):
    frames = np.arange(2 * 2 * 3 * 4, dtype=np.float32).reshape(2, 2, 3, 4)
    albedo, normal = frames + 1, frames + 2
    out = r.denoise_views(frames, albedo, normal)
    src, a, nm, dst, n, w, h, it, s, sa, sn = only_call(r, "rtw_denoise_views")
    assert (src, a, nm, dst) == (frames.ctypes.data, albedo.ctypes.data, normal.ctypes.data, out.ctypes.data) and is_array(out, (2, 2, 3, 4), np.float32)
    assert (n, w, h, it, s, sa, sn) == (2, 3, 2, 5, 0.5, 0.4, 0.5)
    out = r.denoise_views(frames.astype(np.float64), albedo.tolist(), normal, 3, 0.25, 0.125, 0.75)  # converted, not refused
    src, a, nm, dst, n, w, h, it, s, sa, sn = only_call(r, "rtw_denoise_views")
    assert src and a and nm == normal.ctypes.data and dst == out.ctypes.data and is_array(out, (2, 2, 3, 4), np.float32)
    assert (n, w, h, it, s, sa, sn) == (2, 3, 2, 3, 0.25, 0.125, 0.75)
    raises(r, "denoise_views: frames of shape (2, 2, 3, 3), expected (n, h, w, 4)", r.denoise_views, frames[..., :3], albedo, normal)
    raises(r, "denoise_views: frames of shape (2, 3, 4), expected (n, h, w, 4)", r.denoise_views, frames[0], albedo, normal)
    raises(r, "denoise_views: guide of shape (1, 2, 3, 4) for frames of shape (2, 2, 3, 4)", r.denoise_views, frames, albedo[:1], normal)
    raises(r, "denoise_views: guide of shape (2, 2, 3, 3) for frames of shape (2, 2, 3, 4)", r.denoise_views, frames, albedo, normal[..., :3])

    assert r.denoise_views_device(2, PTR["in"], PTR["a"], PTR["b"], PTR["out"], 3, 2, stream_ptr=PTR["stream"]) is None
    assert only_call(r, "rtw_denoise_views_device") == [PTR["in"], PTR["a"], PTR["b"], PTR["out"], 2, 3, 2, 5, 0.5, 0.4, 0.5, PTR["stream"]]
    r.denoise_views_device(2, PTR["in"], PTR["a"], PTR["b"], PTR["out"], 3, 2, 3, 0.25, 0.125, 0.75)
    assert only_call(r, "rtw_denoise_views_device") == [PTR["in"], PTR["a"], PTR["b"], PTR["out"], 2, 3, 2, 3, 0.25, 0.125, 0.75, None]


# ---------------------------------------------------------------- render_guides, render_adaptive, denoise_guided
def test_render_guides(r):
    p = abi.make_params(3, 8, 4, 5, row0=1, row1=7, row_stride=2)  # rows 1, 3, 5
    for st in stats_cases():
        out = r.render_guides(p, stats=st)
        params, g, stats = only_call(r, "rtw_render_guides")
        assert params is p and stats_ok(stats, st) and guides_ok(out, g, abi.GUIDES, (3, 3))
    out = r.render_guides(p, ["prim", "normal"])
    params, g, stats = only_call(r, "rtw_render_guides")
    assert params is p and stats is None and guides_ok(out, g, ("prim", "normal"), (3, 3))
    raises(r, "render_guides: unknown or no guide names ['colour']", r.render_guides, p, ("depth", "colour"))
    raises(r, "render_guides: unknown or no guide names ()", r.render_guides, p, ())


def test_render_adaptive(r):
    p = abi.make_params(3, 8, 256, 5, row0=1, row1=7, row_stride=2)
    img, spp, err, st = r.render_adaptive(p, 0.05)
    params, ad, a, b, c, stats = only_call(r, "rtw_render_adaptive")
    assert params is p and (a, b, c) == (img.ctypes.data, spp.ctypes.data, err.ctypes.data) and stats is st and type(st) is abi.Stats
    assert is_array(img, (3, 3, 4), np.float32) and is_array(spp, (3, 3), np.int32) and is_array(err, (3, 3), np.float32)
    assert type(ad) is abi.Adaptive and bytes(ad) == bytes(abi.Adaptive(64, 0, 0.05, 1))
    r.render_adaptive(p, 0.25, 32, 16, 0)
    assert bytes(only_call(r, "rtw_render_adaptive")[1]) == bytes(abi.Adaptive(32, 16, 0.25, 0))


def test_denoise_guided(r):
    img = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    albedo, normal = img + 1, (img + 2)[..., :3]
    out = r.denoise_guided(img, albedo, normal)
    src, a, nm, dst, w, h, it, s, sa, sn = only_call(r, "rtw_denoise_guided")
    assert (src, a, dst) == (img.ctypes.data, albedo.ctypes.data, out.ctypes.data) and nm and nm != normal.ctypes.data  # (padded to four channels)
    assert is_array(out, (2, 3, 4), np.float32) and (w, h, it, s, sa, sn) == (3, 2, 5, 0.5, 0.4, 0.5)
    r.denoise_guided(img.tolist(), albedo, albedo, 3, 0.25, 0.125, 0.75)
    assert only_call(r, "rtw_denoise_guided")[4:] == [3, 2, 3, 0.25, 0.125, 0.75]
    raises(r, "denoise_guided: guide of shape (2, 3, 2) for a 2x3 image", r.denoise_guided, img, albedo[..., :2], normal)
    raises(r, "denoise_guided: guide of shape (3, 2, 4) for a 2x3 image", r.denoise_guided, img, albedo, albedo.reshape(3, 2, 4))
    raises(r, "denoise_guided: guide of shape (2, 3) for a 2x3 image", r.denoise_guided, img, albedo[..., 0], normal)


# ---------------------------------------------------------------- the parameter builders' own refusals
def test_parameter_builders():
    def refuses(text, call, *args, **kw):
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            call(*args, **kw)
    assert bytes(abi.make_radiance_params(np.int32(4), 5.0, -1, 1, 2, 3, -1)) == params_bytes(abi.RadianceParams, 4, 5, 2 ** 32 - 1, 1, 2, 3, 2 ** 32 - 1)
    assert bytes(abi.make_probe_params(4, 5, mode="occlusion")) == params_bytes(abi.ProbeParams, 4, 5, last=1)
    assert bytes(abi.make_view_params(np.int64(3), 2, 4, 5.0, 1, 2, 3)) == view_params_bytes(3, 2, 4, 5, 1, 2, 3)
    for bad in (0, -3, False, 1.0, None):
        refuses(f"radiance: spp = {bad!r}, expected a positive integer", abi.make_radiance_params, bad, 5)
        refuses(f"probe: spp = {bad!r}, expected a positive integer", abi.make_probe_params, bad, 5)
        refuses(f"probe: spp = {bad!r}, expected a positive integer", abi.make_probe_params, bad, 5, mode="ao")  # spp comes first
        refuses(f"views: height = {bad!r}, expected a positive integer", abi.make_view_params, 3, bad, 4, 5)
    refuses("probe: mode None is neither 'irradiance' nor 'occlusion'", abi.make_probe_params, 4, 5, mode=None)
    refuses("make_view: camera of shape (23,), expected a Camera or 24 floats", abi.make_view, np.zeros(23))
    for bad in (3, -1, True, 1.0):
        refuses(f"make_view: camera_type = {bad!r}, expected 0, 1 or 2", abi.make_view, np.zeros(24), bad)


# ---------------------------------------------------------------- the torch wrappers, as far as a CPU tensor goes
def test_torch_wrappers_refuse_before_any_call(r):
    torch = pytest.importorskip("torch")
    from raytracing_weekend_amd.torch_cast import cast_torch
    from raytracing_weekend_amd.torch_probe import probe_adaptive_torch, probe_torch
    from raytracing_weekend_amd.torch_probe_sh import probe_sh_torch
    from raytracing_weekend_amd.torch_radiance import radiance_torch
    from raytracing_weekend_amd.torch_views import denoise_views_torch, views_adaptive_torch, views_guides_torch, views_tensor, views_torch

    batch = torch.from_numpy(BATCH)
    for name, call, what, rest in (("cast_torch", cast_torch, "rays", ()), ("radiance_torch", radiance_torch, "rays", (4, 5)),
                                   ("probe_torch", probe_torch, "probes", (4, 5)), ("probe_adaptive_torch", probe_adaptive_torch, "probes", (256, 5, 0.05)),
                                   ("probe_sh_torch", probe_sh_torch, "points", (4, 5))):
        raises(r, f"{name}: {what} of shape (3, 7), expected (n, 8)", call, r, batch[:, :7], *rest)
        raises(r, f"{name}: {what} of shape (24,), expected (n, 8)", call, r, batch.reshape(24), *rest)
        raises(r, f"{name}: {what} on cpu, the renderer answers on cuda:0", call, r, batch, *rest)
        raises(r, f"{name}: {what} on cpu, the renderer answers on cuda:0", call, r, batch.double(), *rest)  # the device comes before the dtype
    raises(r, "cast: mode 'x' is neither 'closest' nor 'any'", cast_torch, r, batch[:, :7], mode="x")  # the names come first
    raises(r, "cast: unknown or no output names ['z']", cast_torch, r, batch, want=("z",))
    r.devices = [3]
    raises(r, "radiance_torch: rays on cpu, the renderer answers on cuda:3", radiance_torch, r, batch, 4, 5)
    r.devices = [0]

    views = views_tensor(views2(), "cpu")
    assert views.dtype == torch.float32 and tuple(views.shape) == (2, 28) and views.numpy().tobytes() == bytes(views2())
    for name, call, rest in (("views_torch", views_torch, (3, 2, 4, 5)), ("views_guides_torch", views_guides_torch, (3, 2)),
                             ("views_adaptive_torch", views_adaptive_torch, (3, 2, 256, 5, 0.05))):
        raises(r, f"{name}: views of shape (2, 27), expected (n, 28)", call, r, views[:, :27], *rest)
        raises(r, f"{name}: views of shape (56,), expected (n, 28)", call, r, views.reshape(56), *rest)
        raises(r, f"{name}: views on cpu, the renderer answers on cuda:0", call, r, views, *rest)
        raises(r, f"{name}: views on cpu, the renderer answers on cuda:0", call, r, views, 0, *rest[1:])  # the device comes before the sizes
    raises(r, "views_guides_torch: unknown or no guide names ['colour']", views_guides_torch, r, views[:, :27], 3, 2, which=("colour",))
    raises(r, "views_guides_torch: unknown or no guide names ()", views_guides_torch, r, views, 3, 2, which=())

    frames = torch.zeros((2, 2, 3, 4))
    raises(r, "denoise_views_torch: frames of shape (2, 2, 3, 3), expected (n, height, width, 4)", denoise_views_torch, r, frames[..., :3], frames, frames)
    raises(r, "denoise_views_torch: frames of shape (2, 3, 4), expected (n, height, width, 4)", denoise_views_torch, r, frames[0], frames, frames)
    raises(r, "denoise_views_torch: frames on cpu, the renderer answers on cuda:0", denoise_views_torch, r, frames, frames[:1], frames)
    raises(r, "denoise_views_torch: frames on cpu, the renderer answers on cuda:0", denoise_views_torch, r, frames, frames, frames)
