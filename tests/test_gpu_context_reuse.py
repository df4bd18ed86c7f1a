"""GPU suite of what the render half keeps in a context from call to call (rtw_render, rtw_render_adaptive, rtw_render_guides, the
accumulation session, the two denoisers, rtw_upload_scene): the buffers a context grows on demand and the scratch of single calls.
The render half's counterpart of test_gpu_query_host.py, with the same referee, the library itself on a fresh context: every call of
a sequence on one long-lived context - frames that grow the buffers, smaller frames laid out inside the larger allocations, more
samples, other entry points, another scene in between - returns the bits and the counts (samples, segments, shadow rays) of the same
call made first on a context of its own. Scene 0 goes through k_path (its unit sums, job order and queue), scene 1 under
RTW_BRUTE_MAX=0 through the wavefront lanes (their slabs, radiance buffers and counters, and the three per-pixel sums). A group of
two shards on one device is held to the single-device frames: the gather buffer and the kids' shard buffers."""
import numpy as np
import pytest

from gpu_common import gpu, same_words, upload  # noqa: F401
from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu

UPLOADS = {"scene0": (0, "as_uploaded"), "scene1": (1, "forced_tree")}  # (scene, gpu_common.UPLOADS: the knob is read at upload)
OTHER = {"scene0": "scene1", "scene1": "scene0"}
DEPTH, THRESHOLD = 8, 0.05


def blob_of(name):
    return abi.build_scene(UPLOADS[name][0], 24, 16)


def put(r, name):
    """scene `name` into context r, under its knobs and no others"""
    with pytest.MonkeyPatch.context() as mp:
        upload(r, mp, blob_of(name), UPLOADS[name][1])


def counts(*stats):
    return tuple((st.samples, st.segments, st.shadow_rays) for st in stats)


# ---- the calls: each takes the context and what it depends on (name: the uploaded scene; fresh: the earlier calls' results on fresh
# contexts) and returns (a dict of its output arrays, its counts)
def render(w, h, spp):
    def call(r, name, fresh):
        img, st = r.render(abi.make_params(w, h, spp, DEPTH))
        return {"img": img}, counts(st)
    return call


def adaptive(w, h):
    def call(r, name, fresh):
        img, spp, err, st = r.render_adaptive(abi.make_params(w, h, 128, DEPTH), THRESHOLD, min_spp=32)
        return {"img": img, "spp": spp, "err": err}, counts(st)
    return call


def guides(r, name, fresh):
    st = abi.Stats()
    out = r.render_guides(abi.make_params(24, 16, 16, DEPTH), stats=st)
    return out, counts(st)


def session(r, name, fresh):
    r.accum_begin(abi.make_params(24, 16, 32, DEPTH), error=True)
    st = [r.accum_add(16), r.accum_add(16)]
    img, err = r.accum_read(error=True)
    r.accum_end()
    assert not r.accum_status().active
    return {"img": img, "err": err}, counts(*st)


def denoisers(r, name, fresh):
    img, g = fresh["render 24x16"][0]["img"], fresh["guides 24x16"][0]
    return {"plain": r.denoise(np.clip(img, 0.0, 1.0)), "guided": r.denoise_guided(np.clip(img, 0.0, 1.0), g["albedo"], g["normal"])}, ()


def other_scene(r, name, fresh):
    r.accum_begin(abi.make_params(8, 8, 16, DEPTH))  # left open: it belongs to the scene that the upload replaces
    put(r, OTHER[name])
    assert not r.accum_status().active
    return render(24, 16, 16)(r, OTHER[name], fresh)


def first_scene_again(r, name, fresh):
    put(r, name)
    return render(24, 16, 16)(r, name, fresh)


SEQUENCE = (("render 24x16", render(24, 16, 16)),
            ("render 40x24, larger", render(40, 24, 16)),
            ("render 8x8, inside the larger allocation", render(8, 8, 16)),
            ("render 24x16 at 256 spp", render(24, 16, 256)),
            ("render 24x16 again", render(24, 16, 16)),
            ("adaptive 24x16", adaptive(24, 16)),
            ("adaptive 40x24", adaptive(40, 24)),
            ("guides 24x16", guides),
            ("session of 2 x 16 samples, read with its error map", session),
            ("denoise and denoise_guided", denoisers),
            ("the other scene uploaded and rendered", other_scene),
            ("the first scene uploaded again and rendered", first_scene_again))
GROUP_STEPS = (0, 1, 2, 4)


@pytest.fixture(scope="module", params=list(UPLOADS))
def case(request, gpu):  # noqa: F811
    """(scene, every call of the sequence on a fresh context of its own, the sequence on the module's one context)"""
    name = request.param
    fresh = {}
    for what, call in SEQUENCE:
        r = abi.Renderer(0)
        put(r, name)
        fresh[what] = call(r, name, fresh)
        r.close()
    put(gpu, name)
    mixed = {what: call(gpu, name, fresh) for what, call in SEQUENCE}
    return name, fresh, mixed


def test_a_long_lived_context_returns_what_a_fresh_one_does(case):
    name, fresh, mixed = case
    for what, _ in SEQUENCE:
        (want, want_counts), (got, got_counts) = fresh[what], mixed[what]
        print(name, what, got_counts)
        assert list(got) == list(want) and all(same_words(got[k], want[k]) for k in want), (name, what)
        assert got_counts == want_counts, (name, what)
    # (not vacuous: light arrived, shadow rays were traced, something was hit, the adaptive calls stopped at more than one count,
    # the error map and the denoisers did something, the two scenes differ, and the repeats are repeats)
    first = fresh["render 24x16"]
    assert first[0]["img"][..., :3].any() and first[1][0][0] == 24 * 16 * 16 and first[1][0][1] > first[1][0][0]
    assert first[1][0][2] > 0 or name == "scene1"  # (scene 1 is lit by its sky alone: no light to sample)
    assert fresh["render 24x16 at 256 spp"][1][0][0] == 24 * 16 * 256
    assert (fresh["guides 24x16"][0]["prim"] >= 0).any() and fresh["guides 24x16"][0]["albedo"].any()
    for what in ("adaptive 24x16", "adaptive 40x24"):
        spp = fresh[what][0]["spp"]
        assert spp.min() >= 32 and spp.max() <= 128 and len(np.unique(spp)) >= 2 and fresh[what][1][0][0] == int(spp.astype(np.int64).sum()), what
    ses = fresh["session of 2 x 16 samples, read with its error map"]
    assert ses[0]["err"].any() and [c[0] for c in ses[1]] == [24 * 16 * 16] * 2
    dn = fresh["denoise and denoise_guided"][0]
    assert not same_words(dn["plain"], dn["guided"]) and not same_words(dn["plain"], np.clip(first[0]["img"], 0.0, 1.0))
    assert not same_words(fresh["the other scene uploaded and rendered"][0]["img"], first[0]["img"])
    for what in ("render 24x16 again", "the first scene uploaded again and rendered"):
        assert same_words(fresh[what][0]["img"], first[0]["img"]) and fresh[what][1] == first[1], what


def test_a_group_returns_the_single_device_frames(case):
    name, fresh, _ = case
    g = abi.Renderer([0, 0])
    try:
        put(g, name)
        for what, call in (SEQUENCE[k] for k in GROUP_STEPS):
            got, got_counts = call(g, name, fresh)
            assert same_words(got["img"], fresh[what][0]["img"]), (name, what)
            assert got_counts == fresh[what][1], (name, what)
    finally:
        g.close()
