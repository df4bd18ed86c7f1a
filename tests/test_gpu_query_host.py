"""GPU suite of what the host variants of the query family share (rtw_cast, rtw_radiance, rtw_probe_sh, rtw_views_guides,
rtw_probe_adaptive, rtw_views_adaptive: one staging slab, one call scope, one chunk loop). The referee is the library itself on a
fresh context: a call made after calls of other families, of other sizes and with other outputs wanted, or after a refused call,
returns the bits and the counts of the same call made first on a context of its own - a slab whose sections were left where an
earlier, larger call had put them would show here."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import geometry_ref as G
import probe_ref as P
import radiance_ref as R
import view_ref as V
from gpu_common import same_dict as same  # noqa: F401
from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu

KNOBS = ("RTW_BRUTE_MAX", "RTW_LDS_KB", "RTW_CAST_CHUNK", "RTW_CAST_GRID_MULT", "RTW_RADIANCE_CHUNK", "RTW_RADIANCE_SLAB_BYTES")
UPLOADS = {"scene0": {}, "scene1": {"RTW_BRUTE_MAX": "0"}}  # scene 1 through the tree walk (the knob is read at upload)
W, H, DEPTH, THRESHOLD = 7, 5, 8, 0.05
INVALID = -1  # RTW_ERR_INVALID_ARG


@contextlib.contextmanager
def knobs(env):
    """the tuning knobs as `env` says and nothing else of them, put back afterwards"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def context(name):
    r = abi.Renderer(0)
    with knobs(UPLOADS[name]):
        r.upload_scene(R.scene(name))
    return r


class Inputs:
    def __init__(self, name):
        blob = R.scene(name)
        self.rays, self.ray_time, self.gather_time = G.scene_rays(blob, G.RAY_SEED, 1000)
        self.paths = R.make_rays(*R.pairs(blob, 37))
        r = context(name)
        self.probes = P.scene_probes(r.cast, blob, 64)
        r.close()
        self.views = list(V.cameras(name))


# the sequence: (name, knobs of the call, the call -> a dict of its output arrays); each fills the Stats it is given
def _cast300(r, d, st):
    return r.cast(d.rays[:300], d.ray_time[:300], d.gather_time[:300], stats=st)


def _radiance37(r, d, st):
    return {"rgba": r.radiance(d.paths, 144, DEPTH, stats=st)}


def _guides(r, d, st):
    return r.views_guides(d.views[:2], W, H, which=("depth", "prim"), stats=st)


def _probe_adaptive(r, d, st):
    return dict(zip(("rgba", "spp", "err"), r.probe_adaptive(d.probes, 256, DEPTH, THRESHOLD, stats=st)))


def _cast1000_uv(r, d, st):
    return r.cast(d.rays, None, d.gather_time, want=("uv",), stats=st)


def _views_adaptive(r, d, st):
    return dict(zip(("rgba", "spp", "err"), r.views_adaptive(d.views, W, H, 128, DEPTH, THRESHOLD, min_spp=32, stats=st)))


def _probe_sh(r, d, st):
    return {"sh": r.probe_sh(d.probes[:5], 200, 4, stats=st)}


def _cast10(r, d, st):
    return r.cast(d.rays[:10], stats=st)


SEQUENCE = (("cast of 300 in chunks of 100", {"RTW_CAST_CHUNK": "100"}, _cast300),
            ("radiance of 37 at 144 spp", {}, _radiance37),
            ("views_guides of 2 views, depth and prim", {}, _guides),
            ("probe_adaptive of 64, cap 256", {}, _probe_adaptive),
            ("cast of 1000, uv only", {}, _cast1000_uv),
            ("views_adaptive of 3 views in chunks of 50", {"RTW_RADIANCE_CHUNK": "50"}, _views_adaptive),
            ("probe_sh of 5", {}, _probe_sh),
            ("cast of 10", {}, _cast10))


def run(r, d, env, call):
    st = abi.Stats()
    with knobs(env):
        out = call(r, d, st)
    return out, st


def counts(st):
    return (st.samples, st.segments, st.shadow_rays)


@pytest.fixture(scope="module", params=list(UPLOADS))
def case(request):
    """(scene, inputs, every call of the sequence on a fresh context of its own, the sequence on one context)"""
    name = request.param
    d = Inputs(name)
    fresh = []
    for _, env, call in SEQUENCE:
        r = context(name)
        fresh.append(run(r, d, env, call))
        r.close()
    r = context(name)
    mixed = [run(r, d, env, call) for _, env, call in SEQUENCE]
    r.close()
    return name, d, fresh, mixed


def test_the_slab_is_reused_across_families_and_sizes(case):
    name, _, fresh, mixed = case
    for (what, _, _), (want, _), (got, _) in zip(SEQUENCE, fresh, mixed):
        assert same(got, want), (name, what)
    # (not vacuous: something was hit, light arrived, the adaptive calls stopped at more than one count)
    assert (fresh[0][0]["prim"] >= 0).any() and (fresh[7][0]["prim"] >= 0).any() and fresh[1][0]["rgba"][:, :3].any()
    assert (fresh[2][0]["prim"] >= 0).any() and fresh[6][0]["sh"].any() and fresh[4][0]["uv"].any()
    assert len(np.unique(fresh[3][0]["spp"])) >= 2 and len(np.unique(fresh[5][0]["spp"])) >= 2


def test_the_stats_after_a_mixed_sequence(case):
    name, d, fresh, mixed = case
    for (what, _, _), (_, want), (_, got) in zip(SEQUENCE, fresh, mixed):
        print(name, what, counts(got), f"{got.seconds:.6f} s (fresh context {want.seconds:.6f} s)")
        assert counts(got) == counts(want), (name, what)
        assert got.seconds > 0.0 and want.seconds > 0.0, (name, what)
    assert counts(mixed[0][1]) == (0, 300, 0) and counts(mixed[4][1]) == (0, 1000, 0) and counts(mixed[7][1]) == (0, 10, 0)
    assert counts(mixed[2][1]) == (2 * W * H * 16, 2 * W * H * 16, 0) and mixed[1][1].samples == 37 * 144 and mixed[6][1].samples == 5 * 200
    assert mixed[3][1].samples == int(mixed[3][0]["spp"].astype(np.int64).sum()) and mixed[5][1].samples == int(mixed[5][0]["spp"].astype(np.int64).sum())


def refused(r, rc, text, st):
    """a refusal: the code, the message, and *stats left alone"""
    assert rc == INVALID and r.lib.rtw_last_error(r.ctx).decode() == text, (rc, r.lib.rtw_last_error(r.ctx), text)
    assert st.samples == 77 and st.segments == 78 and st.seconds == 79.0, text


def test_a_refused_call_of_each_family_leaves_the_next_good_call_alone(case):
    name, d, fresh, _ = case
    r = context(name)
    lib, ctx = r.lib, r.ctx
    st = abi.Stats(samples=77, segments=78, seconds=79.0)
    sp = C.byref(st)
    n = len(d.rays)
    buf = np.zeros(16 * n, np.float32)  # room for any one output of the calls below
    hits = abi.Hits(t=buf.ctypes.data)
    rp = abi.make_radiance_params(144, DEPTH)
    pp = abi.make_probe_params(256, DEPTH)
    bad_pp = abi.make_probe_params(256, DEPTH)
    bad_pp.mode = 7
    ad = abi.Adaptive(64, 0, THRESHOLD, 0)
    vp = abi.make_view_params(W, H, 16, DEPTH)
    vp_ad, ad_v = abi.make_view_params(W, H, 128, DEPTH), abi.Adaptive(32, 0, THRESHOLD, 1)
    views = abi.view_array(d.views)
    bad_views = abi.view_array(d.views)
    bad_views[1].camera_type = 9
    vptr, bad_vptr = C.cast(views, C.c_void_p), C.cast(bad_views, C.c_void_p)
    guides = abi.Guides(depth=buf.ctypes.data)

    def good(i):
        _, env, call = SEQUENCE[i]
        got, got_st = run(r, d, env, call)
        assert same(got, fresh[i][0]) and counts(got_st) == counts(fresh[i][1]), (name, SEQUENCE[i][0])

    # rtw_cast
    refused(r, lib.rtw_cast(ctx, d.rays.ctypes.data, None, None, n, 5, C.byref(hits), sp), "rtw_cast: bad mode", st)
    refused(r, lib.rtw_cast(ctx, d.rays.ctypes.data, None, None, n, 0, None, sp), "rtw_cast: null rays or outputs", st)
    good(0)
    # rtw_radiance, rtw_probe_sh
    refused(r, lib.rtw_radiance(ctx, d.paths.ctypes.data, len(d.paths), C.byref(rp), None, sp), "rtw_radiance: null rays or output", st)
    good(1)
    refused(r, lib.rtw_probe_sh(ctx, d.probes.ctypes.data, 5, C.byref(rp), None, sp), "rtw_probe_sh: null rays or output", st)
    good(6)
    # rtw_probe, rtw_probe_adaptive
    refused(r, lib.rtw_probe(ctx, d.probes.ctypes.data, 64, C.byref(bad_pp), buf.ctypes.data, sp), "rtw_probe: bad mode", st)
    refused(r, lib.rtw_probe(ctx, d.probes.ctypes.data, 64, C.byref(pp), None, sp), "rtw_probe: null rays or output", st)
    refused(r, lib.rtw_probe_adaptive(ctx, d.probes.ctypes.data, 64, C.byref(bad_pp), C.byref(ad), buf.ctypes.data, None, None, sp),
            "rtw_probe_adaptive: bad mode", st)
    refused(r, lib.rtw_probe_adaptive(ctx, d.probes.ctypes.data, 64, C.byref(pp), C.byref(ad), None, None, None, sp),
            "rtw_probe_adaptive: null rays or output", st)
    good(3)
    # rtw_views, rtw_views_guides, rtw_views_adaptive
    refused(r, lib.rtw_views(ctx, vptr, 3, C.byref(vp), None, sp), "rtw_views: null views or output", st)
    refused(r, lib.rtw_views(ctx, bad_vptr, 3, C.byref(vp), buf.ctypes.data, sp), "rtw_views: view 1: bad camera_type", st)
    refused(r, lib.rtw_views_guides(ctx, vptr, 3, C.byref(vp), None, sp), "rtw_views_guides: no output buffer", st)
    refused(r, lib.rtw_views_guides(ctx, bad_vptr, 3, C.byref(vp), C.byref(guides), sp), "rtw_views_guides: view 1: bad camera_type", st)
    good(2)
    refused(r, lib.rtw_views_adaptive(ctx, vptr, 3, C.byref(vp_ad), C.byref(ad_v), None, None, None, sp), "rtw_views_adaptive: null views or output", st)
    refused(r, lib.rtw_views_adaptive(ctx, bad_vptr, 3, C.byref(vp_ad), C.byref(ad_v), buf.ctypes.data, None, None, sp),
            "rtw_views_adaptive: view 1: bad camera_type", st)
    good(5)
    good(4)
    good(7)
    assert not buf.any()  # no refused call wrote anything
    r.close()
