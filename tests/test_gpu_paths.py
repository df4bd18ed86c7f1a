"""GPU suite of the path records (include/rtw.h rtw_paths / rtw_paths_views and their _device variants). The referees are the older
members of the family, bit for bit: the oracle's pixels and counts behind rtw_radiance (radiance_ref.py) for the heads' sums,
rtw_radiance and rtw_views sample by sample for every head, the header's fold for the records against their heads, rtw_cast for every
recorded segment's hit. Then truncation, independence of the batch and the chunks, the views form, the plumbing and the command line.
The shapes are radiance_ref's, so the oracle results the radiance suite computed are reused.

The cases are plain functions (case_*), each a few hundredths of a second on the device; the two tests at the end of the file run
them over their scenes, generators, uploads and estimators, go on after a case that fails and name every failed case with its
parameters."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # (before the HIP library is loaded, as in a run of the whole suite)

import geometry_ref as G
import paths_ref as P
import radiance_ref as R
import view_ref as V
from gpu_common import (BOTH, GOLDEN_PAIR, KNOBS, UPLOADS, check_golden_render, check_stream_order, golden, gpu, left_alone, same,  # noqa: F401
                        same_words, sentinel_stats, upload)
from raytracing_weekend_amd import abi
from raytracing_weekend_amd.torch_paths import paths_torch, paths_views_torch
from raytracing_weekend_amd.torch_views import views_tensor

pytestmark = pytest.mark.gpu
N, SPP, DEPTH, KEY = R.N, R.SPP, R.DEPTH, R.KEY
PATHS_KNOBS = KNOBS + ("RTW_PATHS_CHUNK_BYTES",)
FIELDS_H, FIELDS_V = abi.PATH_HEAD.names, abi.PATH_VERTEX.names


def up(gpu, monkeypatch, blob, how="as_uploaded"):
    upload(gpu, monkeypatch, blob, how, knobs=PATHS_KNOBS)


def same_records(a, b):
    """two structured arrays of one dtype and shape carry the same bytes"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_written(ha, va, hb, vb):
    """the same heads and, of each sample, the same written records"""
    if not same_records(ha, hb) or va.shape != vb.shape:
        return False
    w = P.written(ha, va)
    return same_records(va[w], vb[w])


def as_records(t, dtype):
    """a float32 tensor whose last axis is one record, as the structured array Renderer.paths returns"""
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view(dtype).reshape(a.shape[:-1])


def paths_case(gpu, name, rng_kind, estimator=0, k=None, stats=None):
    blob, o, ll, rays, want, seg, shadow = R.case(name, rng_kind, estimator)
    return gpu.paths(rays, SPP, DEPTH, k, rng_kind=rng_kind, estimator=estimator, key_offset=KEY, stats=stats)


# ---------------------------------------------------------------- 1. the oracle's bits
def check_case(gpu, name, rng_kind, estimator=0):
    blob, o, ll, rays, want, seg, shadow = R.case(name, rng_kind, estimator)
    st = abi.Stats()
    heads, vertices = paths_case(gpu, name, rng_kind, estimator, 0, st)
    assert heads.shape == (N, SPP) and vertices.shape == (N, SPP, 0)
    got = np.stack([R.sum_in_order(heads["radiance"][i], SPP) for i in range(N)])
    bad = np.flatnonzero((got.view(np.uint32) != np.ascontiguousarray(want[:, :3]).view(np.uint32)).any(1))
    print(f"{name} rng {rng_kind} estimator {estimator}: segments {st.segments} (oracle {seg}), shadow rays {st.shadow_rays} ({shadow})")
    assert len(bad) == 0, f"{len(bad)} rays differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0], :3]}"
    assert (int(heads["segments"].sum()), int(heads["shadow_rays"].sum())) == (seg, shadow)
    assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, N * SPP)
    assert st.algorithmic_bytes == 128 * st.segments + 32 * st.samples and st.seconds > 0.0
    assert not any(st.kernel_seconds) and not any(st.kernel_launches) and not any(st.kernel_segments)
    assert np.array_equal(heads["key"], np.broadcast_to((KEY + np.arange(N, dtype=np.uint32))[:, None], (N, SPP)))
    assert np.array_equal(heads["sample"], np.broadcast_to(np.arange(SPP, dtype=np.uint32), (N, SPP)))
    assert heads["segments"].min() >= 1 and heads["segments"].max() <= DEPTH


def case_the_heads_sum_to_the_oracles_pixels_and_counts(gpu, monkeypatch, name, how, rng_kind):
    up(gpu, monkeypatch, R.scene(name), how)
    check_case(gpu, name, rng_kind)


def case_the_corrected_estimators_on_scene_0(gpu, monkeypatch, how, estimator, rng_kind):
    up(gpu, monkeypatch, R.scene("scene0"), how)
    check_case(gpu, "scene0", rng_kind, estimator)


# ---------------------------------------------------------------- 2. rtw_radiance, sample by sample
def case_every_head_is_rtw_radiance_at_one_sample(gpu, monkeypatch, name, rng_kind):
    blob, o, ll, rays, want, seg, shadow = R.case(name, rng_kind)
    up(gpu, monkeypatch, blob)
    heads, _ = paths_case(gpu, name, rng_kind, k=0)
    seg = shadow = 0
    for s in range(SPP):
        st = abi.Stats()
        one = gpu.radiance(rays, 1, DEPTH, rng_kind=rng_kind, sample_offset=s, key_offset=KEY, stats=st)
        assert same(one[:, :3], heads["radiance"][:, s]), s
        assert (st.segments, st.shadow_rays) == (int(heads["segments"][:, s].sum()), int(heads["shadow_rays"][:, s].sum())), s
    assert not (np.signbit(heads["radiance"]) & (heads["radiance"] == 0)).any()  # a -0 comes back as +0
    # a sample offset moves the window: samples 5 ... 12 of a longer call
    part, _ = gpu.paths(rays, 8, DEPTH, 0, rng_kind=rng_kind, sample_offset=5, key_offset=KEY)
    assert same(part["radiance"], heads["radiance"][:, 5:13]) and np.array_equal(part["sample"], heads["sample"][:, 5:13])
    assert same_words(part["gather_time"], heads["gather_time"][:, 5:13])


# ---------------------------------------------------------------- 3. the records fold to their heads
def case_the_records_fold_to_their_heads(gpu, monkeypatch, name, rng_kind):
    up(gpu, monkeypatch, R.scene(name))
    st = abi.Stats()
    heads, vertices = paths_case(gpu, name, rng_kind, k=None, stats=st)
    assert vertices.shape == (N, SPP, DEPTH) and P.complete(heads, vertices).all()
    folded = P.fold_all(heads, vertices)
    assert same(folded, heads["radiance"]), np.argwhere((folded.view(np.uint32) != heads["radiance"].view(np.uint32)).any(-1))[:4]
    assert np.array_equal(P.light_sampled(heads, vertices), heads["shadow_rays"])
    assert (int(heads["segments"].sum()), int(heads["shadow_rays"].sum())) == (st.segments, st.shadow_rays)
    w = P.written(heads, vertices)
    assert same(vertices["throughput"][:, :, 0], np.ones((N, SPP, 3), np.float32))
    ev, flags = P.event(vertices), vertices["flags"]
    added, sampled = (flags & abi.RTW_PATH_LIGHT_ADDED) != 0, (flags & abi.RTW_PATH_LIGHT_SAMPLED) != 0
    assert not (added & ~sampled)[w].any() and (flags[w] < 16).all()
    quiet = w & (ev == abi.RTW_PATH_SCATTER) & ~added
    assert quiet.any() and (vertices["contribution"][quiet] == 0).all()
    # a path goes on after a scatter alone, so every written record but a sample's last is one; a miss has no primitive
    last = np.arange(DEPTH) == (heads["segments"] - 1)[..., None]
    assert (ev[w & ~last] == abi.RTW_PATH_SCATTER).all()
    assert ((vertices["prim"] < 0) == (ev == abi.RTW_PATH_MISS))[w].all()
    # and the next record starts where this one's scatter left: its origin is not the caller's any more
    assert np.isfinite(vertices["o"][w]).all() and (heads["segments"] > 1).mean() > 0.25
    assert heads["radiance"].sum() > 0 and sampled[w].any() == (heads["shadow_rays"].sum() > 0)


# ---------------------------------------------------------------- 4. every recorded segment against rtw_cast
def case_every_record_is_the_hit_rtw_cast_finds(gpu, monkeypatch, name, how):
    """Scenes without volume primitives, where rtw_cast (which skips them) walks what the path walked."""
    rng_kind = abi.RTW_RNG_PHILOX
    blob, o, ll, rays, want, seg, shadow = R.case(name, rng_kind)
    assert not any(p.type in (abi.PRIM_VOLUME_BOX, abi.PRIM_VOLUME_SPHERE) for p in abi.parse_scene(blob)["prims"])
    up(gpu, monkeypatch, blob, how)
    heads, vertices = paths_case(gpu, name, rng_kind)
    w = P.written(heads, vertices)
    # record 0 carries the caller's ray; on a miss its t is the caller's tmax
    assert same(vertices["o"][:, :, 0], np.broadcast_to(rays[:, None, 0:3], (N, SPP, 3)))
    assert same(vertices["d"][:, :, 0], np.broadcast_to(rays[:, None, 3:6], (N, SPP, 3)))
    miss0 = vertices["prim"][:, :, 0] < 0
    assert same(vertices["t"][:, :, 0][miss0], np.broadcast_to(rays[:, None, 7], (N, SPP))[miss0])
    tmin = np.full((N, SPP, DEPTH), np.float32(1e-6), np.float32)  # the reference estimator's start distance
    tmax = np.full((N, SPP, DEPTH), np.float32(1e27), np.float32)
    tmin[:, :, 0], tmax[:, :, 0] = rays[:, None, 6], rays[:, None, 7]
    v = vertices[w]
    again = np.concatenate([v["o"], v["d"], tmin[w][:, None], tmax[w][:, None]], axis=1).astype(np.float32)
    gather = np.broadcast_to(heads["gather_time"][..., None], w.shape)[w]
    hits = gpu.cast(again, np.ascontiguousarray(v["ray_time"]), np.ascontiguousarray(gather), want=("t", "prim"))
    assert np.array_equal(hits["prim"], v["prim"]), f"{int((hits['prim'] != v['prim']).sum())} of {len(v)} records"
    assert same(hits["t"], np.ascontiguousarray(v["t"]))
    assert (v["prim"] >= 0).mean() > 0.5 and len(v) == int(heads["segments"].sum())


# ---------------------------------------------------------------- 5. truncation
def raw_paths(gpu, rays, spp, depth, k, fill, **kw):
    """rtw_paths into arrays filled with `fill` bytes first: (heads, vertices, rc)"""
    n = len(rays)
    heads = np.frombuffer(bytes([fill]) * (n * spp * 32), abi.PATH_HEAD).reshape(n, spp).copy()
    vertices = np.frombuffer(bytes([fill]) * (n * spp * k * 64), abi.PATH_VERTEX).reshape(n, spp, k).copy()
    pp = abi.make_paths_params(spp, depth, k, **kw)
    rc = gpu.lib.rtw_paths(gpu.ctx, rays.ctypes.data, n, C.byref(pp), heads.ctypes.data, vertices.ctypes.data if k else None, None)
    return heads, vertices, rc


def case_fewer_records_than_segments_change_nothing_else(gpu, monkeypatch):
    name, rng_kind = "scene3", abi.RTW_RNG_PHILOX
    blob, o, ll, rays, want, seg, shadow = R.case(name, rng_kind)
    up(gpu, monkeypatch, blob)
    heads, vertices = paths_case(gpu, name, rng_kind)
    assert (heads["segments"] > 2).mean() > 0.25 and (heads["segments"] == 1).any()
    st = abi.Stats()
    h2, v2 = paths_case(gpu, name, rng_kind, k=2, stats=st)
    h0, v0 = paths_case(gpu, name, rng_kind, k=0)
    assert same_records(h2, heads) and same_records(h0, heads) and v2.shape == (N, SPP, 2) and v0.shape == (N, SPP, 0)
    w2 = P.written(h2, v2)
    assert same_records(v2[w2], vertices[:, :, :2][w2]) and w2[:, :, 0].all() and not w2[:, :, 1].all()
    assert (st.segments, st.shadow_rays) == (int(heads["segments"].sum()), int(heads["shadow_rays"].sum()))  # all of them, kept or not
    # what is not written keeps what was there
    for k in (2, DEPTH):
        hs, vs, rc = raw_paths(gpu, rays, SPP, DEPTH, k, 0xA5, key_offset=KEY)
        assert rc == 0 and same_records(hs, heads)
        w = P.written(hs, vs)
        assert same_records(vs[w], vertices[:, :, :k][w]) and (~w).any()
        assert (np.ascontiguousarray(vs[~w]).view(np.uint8) == 0xA5).all()
    # no depth: no segment, no record, radiance 0; the gather time, the key and the sample index are the sample's all the same
    hz, vz, rc = raw_paths(gpu, rays, SPP, 0, 0, 0xA5, key_offset=KEY)
    st0 = abi.Stats(segments=5)
    h_, v_ = gpu.paths(rays, SPP, 0, key_offset=KEY, stats=st0)
    assert rc == 0 and same_records(hz, h_) and v_.shape == (N, SPP, 0)
    assert not hz["segments"].any() and not hz["shadow_rays"].any() and not hz["radiance"].view(np.uint32).any()
    assert np.array_equal(hz["key"], heads["key"]) and np.array_equal(hz["sample"], heads["sample"]) and same_words(hz["gather_time"], heads["gather_time"])
    assert (st0.segments, st0.shadow_rays, st0.samples) == (0, 0, N * SPP)
    # depth 1: the first segment alone, which is the first record of the long paths
    h1, v1 = gpu.paths(rays, SPP, 1, key_offset=KEY)
    assert (h1["segments"] == 1).all() and same_records(v1[:, :, 0]["o"], vertices[:, :, 0]["o"]) and same_words(v1["t"][:, :, 0], vertices["t"][:, :, 0])
    assert np.array_equal(v1["prim"][:, :, 0], vertices["prim"][:, :, 0])


# ---------------------------------------------------------------- 6. independence
def case_a_sample_does_not_depend_on_its_batch(gpu, monkeypatch):
    """n = 2^16 + 3 rays of three samples: more pairs than the device holds lanes, so lanes stride. 65 scattered rays equal one-ray
    calls with their own keys; the device path gives the same bytes."""
    blob = R.scene("scene0")
    up(gpu, monkeypatch, blob)
    n, spp, k = (1 << 16) + 3, 3, 2
    rays, _, _ = G.scene_rays(blob, 7, n)
    rays[:, 6], rays[:, 7] = 1e-6, 1e27
    ends = np.array([0, 1, 63, 64, n - 2, n - 1])
    pick = np.concatenate([ends, np.setdiff1d(np.random.default_rng(3).choice(n, 80, replace=False), ends)[:59]])
    assert len(np.unique(pick)) == 65
    st = abi.Stats()
    heads, vertices = gpu.paths(rays, spp, 6, k, key_offset=11, stats=st)
    assert st.samples == n * spp and st.segments == int(heads["segments"].sum()) >= n * spp and (heads["radiance"].sum(-1) > 0).mean() > 0.1
    for j in pick:
        h1, v1 = gpu.paths(rays[j:j + 1], spp, 6, k, key_offset=11 + int(j))
        assert same_written(h1, v1, heads[j:j + 1], vertices[j:j + 1]), j
    dh, dv = paths_torch(gpu, torch.from_numpy(rays).cuda(), spp, 6, k, key_offset=11)
    assert same_written(as_records(dh, abi.PATH_HEAD), as_records(dv, abi.PATH_VERTEX), heads, vertices)


def case_chunks_do_not_change_the_bytes_and_keys_wrap(gpu, monkeypatch, rng_kind):
    blob = R.scene("scene1")
    up(gpu, monkeypatch, blob)
    n, spp, k = 1003, 3, 4
    rays, _, _ = G.scene_rays(blob, 11, n)
    rays[:, 6], rays[:, 7] = 1e-6, 1e27
    ray_bytes = spp * (32 + 64 * k)
    k0 = 2 ** 32 - 501  # the keys wrap inside the batch, and inside a chunk of three rays
    s0 = abi.Stats()
    heads, vertices = gpu.paths(rays, spp, 6, k, rng_kind=rng_kind, key_offset=k0, stats=s0)
    assert np.array_equal(heads["key"][:, 0], (k0 + np.arange(n)).astype(np.uint64).astype(np.uint32))
    for budget in (ray_bytes, ray_bytes * 7 // 2, 1):
        monkeypatch.setenv("RTW_PATHS_CHUNK_BYTES", str(budget))
        s1 = abi.Stats()
        h1, v1 = gpu.paths(rays, spp, 6, k, rng_kind=rng_kind, key_offset=k0, stats=s1)
        assert same_written(h1, v1, heads, vertices), budget
        assert (s1.segments, s1.shadow_rays, s1.samples) == (s0.segments, s0.shadow_rays, s0.samples)
    monkeypatch.delenv("RTW_PATHS_CHUNK_BYTES")
    # the rays past the wrap are a call of their own from key 0
    h2, v2 = gpu.paths(rays[501:], spp, 6, k, rng_kind=rng_kind, key_offset=0)
    assert same_written(h2, v2, heads[501:], vertices[501:]) and (heads["radiance"].sum(-1) > 0).mean() > 0.5


# ---------------------------------------------------------------- 7. the views form
VW = VH = 8
VSPP = 5


def view_heads_are_the_views_samples(gpu, view, rng_kind, heads):
    for s in range(VSPP):
        frame = gpu.views([view], VW, VH, 1, DEPTH, rng_kind=rng_kind, sample_offset=s)
        assert same(frame.reshape(VW * VH, 4)[:, :3], heads["radiance"][:, s]), s


def case_the_views_form_replays_rtw_views(gpu, monkeypatch, rng_kind):
    blob = R.scene("scene1")  # moving spheres: the gather and ray times matter
    up(gpu, monkeypatch, blob)
    own = abi.scene_view(blob, 4242)
    _, env, ortho = V.cameras("scene1")
    views = [own, env, ortho]
    npix = VW * VH
    st = abi.Stats()
    heads, vertices = gpu.paths_views(views, VW, VH, 0, 3 * npix, VSPP, DEPTH, rng_kind=rng_kind, stats=st)
    assert heads.shape == (3 * npix, VSPP) and vertices.shape == (3 * npix, VSPP, DEPTH)
    assert (st.samples, st.segments, st.shadow_rays) == (3 * npix * VSPP, int(heads["segments"].sum()), int(heads["shadow_rays"].sum()))
    assert np.array_equal(heads["key"][:, 0], np.tile(np.arange(npix, dtype=np.uint32), 3))
    for v, view in enumerate(views):
        view_heads_are_the_views_samples(gpu, view, rng_kind, heads[v * npix:(v + 1) * npix])
        assert (heads["radiance"][v * npix:(v + 1) * npix].sum(-1) > 0).mean() > 0.5
    assert same(P.fold_all(heads, vertices), heads["radiance"]) and np.array_equal(P.light_sampled(heads, vertices), heads["shadow_rays"])
    # a window is the same slice of the whole call, wherever it begins and ends; one sample of one pixel is the firefly hunt's call
    for first, count in ((0, 1), (npix - 3, 7), (2 * npix + 5, npix - 5), (3 * npix, 0)):
        h, v = gpu.paths_views(views, VW, VH, first, count, VSPP, DEPTH, rng_kind=rng_kind)
        assert same_written(h, v, heads[first:first + count], vertices[first:first + count]), (first, count)
    x, y, s = 5, 6, 3
    p = (1 * VH + y) * VW + x
    h, v = gpu.paths_views(views, VW, VH, p, 1, 1, DEPTH, rng_kind=rng_kind, sample_offset=s)
    assert same_written(h, v, heads[p:p + 1, s:s + 1], vertices[p:p + 1, s:s + 1]) and int(h["key"][0, 0]) == VW * y + x and int(h["sample"][0, 0]) == s
    monkeypatch.setenv("RTW_PATHS_CHUNK_BYTES", str(VSPP * (32 + 64 * DEPTH) * 5 // 2))  # chunks of two pixels
    h, v = gpu.paths_views(views, VW, VH, npix - 3, 7, VSPP, DEPTH, rng_kind=rng_kind)
    assert same_written(h, v, heads[npix - 3:npix + 4], vertices[npix - 3:npix + 4])
    monkeypatch.delenv("RTW_PATHS_CHUNK_BYTES")
    dh, dv = paths_views_torch(gpu, views_tensor(views, "cuda:0"), VW, VH, npix - 3, 7, VSPP, DEPTH, rng_kind=rng_kind)
    assert same_written(as_records(dh, abi.PATH_HEAD), as_records(dv, abi.PATH_VERTEX), heads[npix - 3:npix + 4], vertices[npix - 3:npix + 4])
    # the blob's own perspective view: its camera rays, fed back as the caller's rays under the pixels' keys and the view's seed,
    # are the same paths
    assert own.camera_type == abi.RTW_CAM_PERSPECTIVE
    for s in range(VSPP):
        r0 = vertices[:npix, s, 0]
        rays = np.concatenate([r0["o"], r0["d"], np.full((npix, 1), 1e-6, np.float32), np.full((npix, 1), 1e27, np.float32)], axis=1).astype(np.float32)
        h, v = gpu.paths(rays, 1, DEPTH, rng_kind=rng_kind, seed=own.seed, sample_offset=s, key_offset=0)
        assert same_written(h, v, heads[:npix, s:s + 1], vertices[:npix, s:s + 1]), s


# ---------------------------------------------------------------- 8. plumbing
def case_paths_torch_equals_paths_and_is_ordered_on_the_current_stream(gpu, monkeypatch):
    name, rng_kind = "random_volumes_motion", abi.RTW_RNG_PHILOX
    blob, o, ll, rays, want, seg, shadow = R.case(name, rng_kind)
    up(gpu, monkeypatch, blob)
    heads, vertices = paths_case(gpu, name, rng_kind)
    d_rays = torch.from_numpy(rays).cuda()
    st = abi.Stats()
    dh, dv = paths_torch(gpu, d_rays, SPP, DEPTH, key_offset=KEY, stats=st)
    assert dh.is_cuda and dv.is_cuda and tuple(dh.shape) == (N, SPP, 8) and tuple(dv.shape) == (N, SPP, DEPTH, 16)
    assert (st.segments, st.shadow_rays, st.samples) == (seg, shadow, N * SPP) and st.seconds > 0.0

    def right(got):
        return same_written(as_records(got[0], abi.PATH_HEAD), as_records(got[1], abi.PATH_VERTEX), heads, vertices)
    assert right((dh, dv))
    # the int fields through a view of the same words
    assert np.array_equal(dh[..., 3].contiguous().view(torch.int32).cpu().numpy(), heads["segments"])
    assert np.array_equal(dv[..., 7].contiguous().view(torch.int32).cpu().numpy(), vertices["prim"])
    check_stream_order(lambda t: paths_torch(gpu, t, SPP, DEPTH, key_offset=KEY), d_rays, right)
    h0, v0 = paths_torch(gpu, d_rays, SPP, DEPTH, 0, key_offset=KEY)
    assert tuple(v0.shape) == (N, SPP, 0, 16) and same_records(as_records(h0, abi.PATH_HEAD), heads)
    e = paths_torch(gpu, torch.zeros((0, 8), device="cuda:0"), 4, 4)
    assert tuple(e[0].shape) == (0, 4, 8) and tuple(e[1].shape) == (0, 4, 4, 16)
    for bad in ((0, DEPTH), (SPP, DEPTH, DEPTH + 1)):
        with pytest.raises(ValueError):
            paths_torch(gpu, d_rays, *bad)


def case_every_refusal_writes_nothing_and_leaves_the_context_usable(gpu, monkeypatch):
    name, rng_kind = "scene0", abi.RTW_RNG_PHILOX
    blob, o, ll, rays, want, _, _ = R.case(name, rng_kind)
    lib, n, k = gpu.lib, N, 2
    heads = np.frombuffer(b"\xa5" * (n * SPP * 32), abi.PATH_HEAD).copy()
    vertices = np.frombuffer(b"\xa5" * (n * SPP * k * 64), abi.PATH_VERTEX).copy()
    d_rays = torch.from_numpy(np.concatenate([rays.ravel(), np.zeros(8, np.float32)])).cuda()
    d_heads = torch.full((n * SPP * 8 + 8,), -7.0, device="cuda:0")
    d_vertices = torch.full((n * SPP * k * 16 + 8,), -7.0, device="cuda:0")
    R_, H_, V_, DR, DH, DV = rays.ctypes.data, heads.ctypes.data, vertices.ctypes.data, d_rays.data_ptr(), d_heads.data_ptr(), d_vertices.data_ptr()
    views = abi.view_array([abi.scene_view(blob)] * 2)
    d_views = views_tensor(views, "cuda:0")
    VS, DVS = C.cast(views, C.c_void_p), d_views.data_ptr()

    def pp(**kw):
        p = abi.make_paths_params(SPP, DEPTH, k, key_offset=KEY)
        for f, v in kw.items():
            setattr(p, f, v)
        return C.byref(p)

    def vp(**kw):
        p = abi.make_view_params(8, 8, 4, DEPTH)  # 128 pixels in the two views
        for f, v in kw.items():
            setattr(p, f, v)
        return C.byref(p)
    fresh = abi.Renderer(0)
    try:
        assert lib.rtw_paths(fresh.ctx, R_, n, pp(), H_, V_, None) == -3  # RTW_ERR_NO_SCENE
        assert lib.rtw_paths_device(fresh.ctx, DR, n, pp(), DH, DV, None, None) == -3
        assert lib.rtw_paths_views(fresh.ctx, VS, 2, vp(), 0, 4, k, H_, V_, None) == -3
        assert lib.rtw_paths_views_device(fresh.ctx, DVS, 2, vp(), 0, 4, k, DH, DV, None, None) == -3
        assert b"rtw_upload_scene" in lib.rtw_last_error(fresh.ctx)
    finally:
        fresh.close()
    up(gpu, monkeypatch, blob)
    good_heads, good_vertices = paths_case(gpu, name, rng_kind, k=k)

    def still_fine():
        h, v = paths_case(gpu, name, rng_kind, k=k)
        assert same_written(h, v, good_heads, good_vertices)
    two = (C.c_uint32 * 2)
    bad_params = [(None, b"null params"), (pp(spp=0), b"spp"), (pp(spp=-1), b"spp"), (pp(max_depth=-1), b"max_depth"), (pp(rng_kind=2), b"rng_kind"),
                  (pp(estimator=4), b"estimator"), (pp(estimator=-1), b"estimator"), (pp(sample_offset=-1), b"sample_offset"),
                  (pp(sample_offset=2 ** 31 - SPP), b"sample_offset"), (pp(max_records=-1), b"max_records"), (pp(max_records=DEPTH + 1), b"max_records"),
                  (pp(max_depth=1), b"max_records"), (pp(reserved=two(1, 0)), b"reserved"), (pp(reserved=two(0, 1)), b"reserved"),
                  (pp(spp=2 ** 26), b"2^31 - 1 samples")]  # 96 * 2^26 pairs
    host = [(R_, n, p, H_, V_, msg) for p, msg in bad_params] + [
        (R_, 1 << 31, pp(), H_, V_, b"2^31 - 1 rays"), (None, n, pp(), H_, V_, b"null rays"), (R_, n, pp(), None, V_, b"null heads"),
        (R_, n, pp(), H_, None, b"vertices must be NULL exactly"), (R_, n, pp(max_records=0), H_, V_, b"vertices must be NULL exactly")]
    for r_, m, p, h_, v_, msg in host:
        st = sentinel_stats()
        assert lib.rtw_paths(gpu.ctx, r_, m, p, h_, v_, C.byref(st)) == -1, msg
        assert msg in lib.rtw_last_error(gpu.ctx) and left_alone(st), (msg, lib.rtw_last_error(gpu.ctx))
    still_fine()
    dev = [(DR, n, p, DH, DV, msg) for p, msg in bad_params] + [
        (DR, 1 << 31, pp(), DH, DV, b"2^31 - 1 rays"), (None, n, pp(), DH, DV, b"null rays"), (DR, n, pp(), None, DV, b"null heads"),
        (DR, n, pp(), DH, None, b"vertices must be NULL exactly"), (DR, n, pp(max_records=0), DH, DV, b"vertices must be NULL exactly"),
        (DR + 4, n, pp(), DH, DV, b"16-byte aligned"), (DR, n, pp(), DH + 8, DV, b"16-byte aligned"), (DR, n, pp(), DH, DV + 4, b"16-byte aligned")]
    for r_, m, p, h_, v_, msg in dev:
        st = sentinel_stats()
        assert lib.rtw_paths_device(gpu.ctx, r_, m, p, h_, v_, None, C.byref(st)) == -1, msg
        assert msg in lib.rtw_last_error(gpu.ctx) and left_alone(st), (msg, lib.rtw_last_error(gpu.ctx))
    still_fine()
    # the views form: rtw_views' list, then the window and the records
    bad_view = abi.view_array([abi.scene_view(blob), abi.make_view(np.zeros(24, np.float32))])
    bad_view[1].camera_type = 3
    def view_refusals(vs, h_, v_):
        return [(vs, 2, None, 0, 4, k, h_, v_, b"null params"), (vs, 2, vp(width=0), 0, 4, k, h_, v_, b"width"), (vs, 2, vp(spp=0), 0, 4, k, h_, v_, b"spp"),
                (vs, 2, vp(reserved=1), 0, 4, k, h_, v_, b"reserved"), (vs, 2, vp(width=32768, height=32768), 0, 4, k, h_, v_, b"pixels"),
                (None, 2, vp(), 0, 4, k, h_, v_, b"null views"), (vs, 2, vp(), 0, 4, -1, h_, v_, b"max_records"),
                (vs, 2, vp(), 0, 4, DEPTH + 1, h_, v_, b"max_records"), (vs, 2, vp(), 125, 4, k, h_, v_, b"beyond the call's pixels"),
                (vs, 2, vp(), 129, 0, k, h_, v_, b"beyond the call's pixels"), (vs, 2, vp(), 2 ** 64 - 1, 2, k, h_, v_, b"beyond the call's pixels"),
                (vs, 2, vp(), 0, 4, k, None, v_, b"null heads"), (vs, 2, vp(), 0, 4, k, h_, None, b"vertices must be NULL exactly"),
                (vs, 2, vp(), 0, 4, 0, h_, v_, b"vertices must be NULL exactly"),
                (vs, 2, vp(width=16384, height=16384, spp=1024), 0, 2 ** 22, 0, h_, None, b"2^31 - 1 samples")]
    vhost = view_refusals(VS, H_, V_)
    for a in vhost:
        st = sentinel_stats()
        assert lib.rtw_paths_views(gpu.ctx, *a[:-1], C.byref(st)) == -1, a[-1]
        assert a[-1] in lib.rtw_last_error(gpu.ctx) and left_alone(st), (a[-1], lib.rtw_last_error(gpu.ctx))
    st = sentinel_stats()
    assert lib.rtw_paths_views(gpu.ctx, C.cast(bad_view, C.c_void_p), 2, vp(), 0, 4, k, H_, V_, C.byref(st)) == -1 and left_alone(st)
    assert b"camera_type" in lib.rtw_last_error(gpu.ctx)
    vdev = view_refusals(DVS, DH, DV) + [(DVS + 4, 2, vp(), 0, 4, k, DH, DV, b"16-byte aligned"), (DVS, 2, vp(), 0, 4, k, DH + 4, DV, b"16-byte aligned"),
                                         (DVS, 2, vp(), 0, 4, k, DH, DV + 8, b"16-byte aligned")]
    for a in vdev:
        st = sentinel_stats()
        assert lib.rtw_paths_views_device(gpu.ctx, *a[:-1], None, C.byref(st)) == -1, a[-1]
        assert a[-1] in lib.rtw_last_error(gpu.ctx) and left_alone(st), (a[-1], lib.rtw_last_error(gpu.ctx))
    still_fine()
    torch.cuda.synchronize()
    assert (heads.view(np.uint8) == 0xA5).all() and (vertices.view(np.uint8) == 0xA5).all()  # no refused call wrote anything
    assert bool((d_heads == -7).all().item()) and bool((d_vertices == -7).all().item())
    # nothing to do is fine and launches nothing, whatever the pointers
    st = abi.Stats(segments=77)
    assert lib.rtw_paths(gpu.ctx, None, 0, pp(), None, None, C.byref(st)) == 0 and (st.segments, st.samples, st.seconds) == (0, 0, 0.0)
    assert lib.rtw_paths_device(gpu.ctx, DR + 4, 0, pp(), DH + 4, None, None, None) == 0
    assert lib.rtw_paths_views(gpu.ctx, VS, 2, vp(), 128, 0, k, None, None, None) == 0
    assert lib.rtw_paths_views_device(gpu.ctx, None, 0, vp(), 0, 0, k, None, None, None, None) == 0
    # from ray 1 on: aligned enough
    assert lib.rtw_paths_device(gpu.ctx, DR + 32, n - 1, pp(key_offset=KEY + 1), DH + 32, DV + 64, None, None) == 0
    got_h = d_heads[8:8 + (n - 1) * SPP * 8].reshape(n - 1, SPP, 8)
    got_v = d_vertices[16:16 + (n - 1) * SPP * k * 16].reshape(n - 1, SPP, k, 16)
    assert same_written(as_records(got_h, abi.PATH_HEAD), as_records(got_v, abi.PATH_VERTEX), good_heads[1:], good_vertices[1:])


def case_groups_sessions_and_rtw_render_afterwards(gpu, monkeypatch):
    name, rng_kind = "scene1", abi.RTW_RNG_PHILOX
    blob, o, ll, rays, want, seg, shadow = R.case(name, rng_kind)
    up(gpu, monkeypatch, blob)
    heads, vertices = paths_case(gpu, name, rng_kind)
    views = [abi.scene_view(blob, 7)]
    vh, vv = gpu.paths_views(views, VW, VH, 3, 20, VSPP, DEPTH)
    group = abi.Renderer([0, 0])
    try:
        pp = abi.make_paths_params(SPP, DEPTH, 0)
        out = np.zeros((N, SPP), abi.PATH_HEAD)
        assert group.lib.rtw_paths(group.ctx, rays.ctypes.data, N, C.byref(pp), out.ctypes.data, None, None) == -3
        group.upload_scene(blob)
        st = abi.Stats()
        h, v = paths_case(group, name, rng_kind, stats=st)
        assert same_written(h, v, heads, vertices) and (st.segments, st.shadow_rays) == (seg, shadow)
        dh, dv = paths_torch(group, torch.from_numpy(rays).cuda(), SPP, DEPTH, key_offset=KEY)
        assert same_written(as_records(dh, abi.PATH_HEAD), as_records(dv, abi.PATH_VERTEX), heads, vertices)
        h, v = group.paths_views(views, VW, VH, 3, 20, VSPP, DEPTH)
        assert same_written(h, v, vh, vv)
    finally:
        group.close()
    # a session that is open across the calls continues exactly
    p = abi.make_params(32, 32, 32, 6)
    one_shot, _ = gpu.render(p)
    gpu.accum_begin(p)
    try:
        gpu.accum_add(16)
        h, v = paths_case(gpu, name, rng_kind)
        assert same_written(h, v, heads, vertices)
        h, v = gpu.paths_views(views, VW, VH, 3, 20, VSPP, DEPTH)
        assert same_written(h, v, vh, vv)
        gpu.accum_add(16)
        assert same(gpu.accum_read(), one_shot) and gpu.accum_status().done == 32
    finally:
        gpu.accum_end()
    # rtw_render afterwards
    for k in PATHS_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for g in map(golden, GOLDEN_PAIR):
        gpu.upload_scene(g.blob)
        o2, ll2 = R.pairs(g.blob, 300)
        a, _ = gpu.paths(R.make_rays(o2, ll2), 6, 6, 3, rng_kind=g.rng)
        b, _ = gpu.paths_views([abi.scene_view(g.blob, g.seed)], g.w, g.h, 100, 300, 2, g.depth, 0, rng_kind=g.rng)
        assert np.isfinite(a["radiance"]).all() and a["radiance"].sum() > 0 and np.isfinite(b["radiance"]).all()
        check_golden_render(gpu, g)
        assert same_records(gpu.paths(R.make_rays(o2, ll2), 6, 6, 3, rng_kind=g.rng)[0], a)


# ---------------------------------------------------------------- 9. the command line
def floats_after(tokens, name, n):
    """the n floats after `name` in a line's tokens, from their hex bit patterns; the decimal beside each says the same"""
    i = tokens.index(name) + 1
    got = np.array([int(tokens[i + 2 * j], 16) for j in range(n)], np.uint32).view(np.float32)
    for j in range(n):
        assert re.fullmatch(r"[0-9a-f]{8}", tokens[i + 2 * j])
        dec = np.float32(float(tokens[i + 2 * j + 1]))
        assert dec.view(np.uint32) == got[j].view(np.uint32) or (np.isnan(dec) and np.isnan(got[j]))  # %.9g round-trips a float32
    return got


def cli_pixel(gpu, cli, tmp_path, w, h, x, y):
    """rtw_render ... -paths x y: the file against the frame of the same run and against paths_views; the frame's pixel"""
    txt, pfm = tmp_path / f"p_{x}_{y}.txt", tmp_path / f"f_{x}_{y}.pfm"
    run = subprocess.run([cli, "-s", "0", "-dx", str(w), "-dy", str(h), "-ns", str(SPP), "-d", str(DEPTH), "-v", "-paths", str(x), str(y), str(txt),
                          "-o", str(pfm)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    raw = open(pfm, "rb").read()
    frame = np.frombuffer(raw[len(raw) - w * h * 12:], "<f4").reshape(h, w, 3)
    lines = [ln.split() for ln in open(txt).read().splitlines()]
    samples = [t for t in lines if t[0] == "sample"]
    assert [int(t[1]) for t in samples] == list(range(SPP)) and all(int(t[t.index("key") + 1]) == w * y + x for t in samples)
    rad = np.stack([floats_after(t, "radiance", 3) for t in samples])
    assert same(R.sum_in_order(rad, SPP), np.ascontiguousarray(frame[y, x]))
    # the same samples through the library
    blob = abi.build_scene(0, w, h)
    gpu.upload_scene(blob)
    heads, vertices = gpu.paths_views([abi.scene_view(blob)], w, h, y * w + x, 1, SPP, DEPTH)
    assert same(rad, heads["radiance"][0])
    assert [int(t[t.index("segments") + 1]) for t in samples] == heads["segments"][0].tolist()
    assert [int(t[t.index("shadow_rays") + 1]) for t in samples] == heads["shadow_rays"][0].tolist()
    assert same(np.array([floats_after(t, "gather_time", 1)[0] for t in samples], np.float32), heads["gather_time"][0])
    vlines = [t for t in lines if t[0] == "vertex"]
    assert len(vlines) == int(heads["segments"][0].sum()) == len(lines) - SPP
    at = 0
    for s in range(SPP):
        for j in range(int(heads["segments"][0, s])):
            t, v = vlines[at], vertices[0, s, j]
            at += 1
            assert (int(t[1]), int(t[2]), int(t[t.index("prim") + 1]), int(t[t.index("flags") + 1])) == (s, j, int(v["prim"]), int(v["flags"]))
            for name, n in (("o", 3), ("d", 3), ("contribution", 3), ("throughput", 3)):
                assert same(floats_after(t, name, n), v[name]), (s, j, name)
            for name in ("t", "ray_time"):
                assert floats_after(t, name, 1)[0].view(np.uint32) == v[name].view(np.uint32), (s, j, name)
    # -v names the brightest sample (the first of them)
    assert f"is sample {int(np.argmax(P.luminance(heads['radiance'][0])))} " in run.stderr
    return frame[y, x]


def case_cli_paths_replays_a_pixel_of_the_frame_it_renders(gpu, monkeypatch, tmp_path):
    for k in PATHS_KNOBS:
        monkeypatch.delenv(k, raising=False)
    cli = os.path.join(abi.REPO_DIR, "raytracing_weekend_amd", "host", "rtw_render")
    assert os.path.exists(cli), "build() has not produced the CLI"
    w = h = 32
    cli_pixel(gpu, cli, tmp_path, w, h, 11, 7)  # (beside the box at this size: every sample misses)
    assert cli_pixel(gpu, cli, tmp_path, w, h, 16, 16).sum() > 0  # the middle of the box
    # refused before anything is rendered
    base = [cli, "-s", "0", "-dx", str(w), "-dy", str(h), "-ns", "4", "-d", "4", "-o", str(tmp_path / "x.pfm")]
    for bad in (["-paths", "1", "2"], ["-paths", str(w), "0", str(tmp_path / "q.txt")], ["-paths", "1", "1", str(tmp_path / "q.txt"), "-orbit", "2"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "ERROR" in r.stderr
    assert not os.path.exists(tmp_path / "q.txt")


# ---------------------------------------------------------------- the two tests: every case above, over its parameters
def run_cases(cases):
    """Every (function, arguments) in turn; a failed assertion does not stop the others. Fails with the list of what failed."""
    failed = []
    for fn, args in cases:
        label = f"{fn.__name__}({', '.join(repr(a) for a in args if isinstance(a, (str, int)))})"
        try:
            fn(*args)
        except AssertionError as e:
            failed.append(f"{label}: {str(e)[:2000]}")
        print("ran", label, flush=True)
    assert not failed, f"{len(failed)} of {len(cases)} cases failed:\n" + "\n".join(failed)


def test_paths_are_the_samples_of_the_older_entry_points_bit_for_bit(gpu, monkeypatch):
    g, m = gpu, monkeypatch
    cases = [(case_the_heads_sum_to_the_oracles_pixels_and_counts, (g, m, name, how, rng)) for name in R.SCENES for how in UPLOADS for rng in BOTH]
    cases += [(case_the_corrected_estimators_on_scene_0, (g, m, how, est, rng)) for how in UPLOADS for est in (1, 2, 3) for rng in BOTH]
    cases += [(case_every_head_is_rtw_radiance_at_one_sample, (g, m, name, rng)) for name in ("scene0", "random_volumes_motion") for rng in BOTH]
    cases += [(case_the_records_fold_to_their_heads, (g, m, name, rng)) for name in R.SCENES for rng in BOTH]
    cases += [(case_every_record_is_the_hit_rtw_cast_finds, (g, m, name, how)) for name in ("scene0", "scene1") for how in UPLOADS]
    cases += [(case_fewer_records_than_segments_change_nothing_else, (g, m)), (case_a_sample_does_not_depend_on_its_batch, (g, m))]
    cases += [(case_chunks_do_not_change_the_bytes_and_keys_wrap, (g, m, rng)) for rng in BOTH]
    cases += [(case_the_views_form_replays_rtw_views, (g, m, rng)) for rng in BOTH]
    assert len(cases) == 56
    run_cases(cases)


def test_plumbing_refusals_neighbours_and_the_command_line(gpu, monkeypatch, tmp_path):
    g, m = gpu, monkeypatch
    run_cases([(case_paths_torch_equals_paths_and_is_ordered_on_the_current_stream, (g, m)),
               (case_every_refusal_writes_nothing_and_leaves_the_context_usable, (g, m)),
               (case_groups_sessions_and_rtw_render_afterwards, (g, m)),
               (case_cli_paths_replays_a_pixel_of_the_frame_it_renders, (g, m, tmp_path))])
