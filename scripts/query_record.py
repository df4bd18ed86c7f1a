"""What the 18 entry points of the query family return, over the small matrix of tests/test_gpu_query_host.py: scene 0 (the candidate
lists) and scene 1 under RTW_BRUTE_MAX=0 (the tree walk), on one context per scene - rtw_cast, rtw_radiance, rtw_probe, rtw_probe_sh,
rtw_views, rtw_views_guides, rtw_denoise_views, rtw_probe_adaptive, rtw_views_adaptive, then their device variants on torch tensors.
One line per call: a CRC-32 of every output array and samples, segments, shadow_rays; no times. Two checkouts whose host code stages,
issues and counts alike print the same bytes:

    python scripts/query_record.py > new.txt
    python scripts/query_record.py --root PARENT_CHECKOUT > parent.txt     (the package, built library and test inputs of that checkout)

profiles/query_host_record.txt keeps one output."""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:  # (before the imports: the package of that checkout)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the HIP library is loaded)

import geometry_ref as G  # noqa: E402
import probe_ref as P  # noqa: E402
import radiance_ref as R  # noqa: E402
import view_ref as V  # noqa: E402
from raytracing_weekend_amd import abi  # noqa: E402

W, H, DEPTH, THRESHOLD = 7, 5, 8, 0.05
KNOBS = ("RTW_BRUTE_MAX", "RTW_LDS_KB", "RTW_CAST_CHUNK", "RTW_CAST_GRID_MULT", "RTW_RADIANCE_CHUNK", "RTW_RADIANCE_SLAB_BYTES")
UPLOADS = {"scene0": {}, "scene1": {"RTW_BRUTE_MAX": "0"}}


def knobs(env):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)


def line(tag, out, st=None):
    crcs = " ".join(f"{k} {zlib.crc32(np.ascontiguousarray(v).tobytes()):08x}" for k, v in out.items())
    tail = "" if st is None else f"  samples {st.samples} segments {st.segments} shadow_rays {st.shadow_rays}"
    print(f"{tag:44s} {crcs}{tail}", flush=True)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32 if np.asarray(a).dtype.kind == 'f' else None)).cuda()  # (a writable copy)


def empty(shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def record(name):
    blob = R.scene(name)
    r = abi.Renderer(0)
    knobs(UPLOADS[name])
    r.upload_scene(blob)
    knobs({})
    rays, ray_time, gather_time = G.scene_rays(blob, G.RAY_SEED, 1000)
    paths = R.make_rays(*R.pairs(blob, 37))
    probes = P.scene_probes(r.cast, blob, 64)
    views = list(V.cameras(name))
    n_pix = 3 * H * W

    # ---- the host variants, in the order and under the knobs of the test's sequence, then the ones it leaves out
    def st():
        return abi.Stats()
    s = st()
    knobs({"RTW_CAST_CHUNK": "100"})
    line(f"{name} cast 300 chunk 100", r.cast(rays[:300], ray_time[:300], gather_time[:300], stats=s), s)
    knobs({})
    s = st()
    line(f"{name} radiance 37 x 144", {"rgba": r.radiance(paths, 144, DEPTH, stats=s)}, s)
    s = st()
    line(f"{name} views_guides 2 depth prim", r.views_guides(views[:2], W, H, which=("depth", "prim"), stats=s), s)
    s = st()
    line(f"{name} probe_adaptive 64 cap 256", dict(zip(("rgba", "spp", "err"), r.probe_adaptive(probes, 256, DEPTH, THRESHOLD, stats=s))), s)
    s = st()
    line(f"{name} cast 1000 uv", r.cast(rays, None, gather_time, want=("uv",), stats=s), s)
    s = st()
    knobs({"RTW_RADIANCE_CHUNK": "50"})
    line(f"{name} views_adaptive 3 chunk 50", dict(zip(("rgba", "spp", "err"), r.views_adaptive(views, W, H, 128, DEPTH, THRESHOLD, min_spp=32, stats=s))), s)
    knobs({})
    s = st()
    line(f"{name} probe_sh 5 x 200", {"sh": r.probe_sh(probes[:5], 200, 4, stats=s)}, s)
    s = st()
    line(f"{name} cast 10", r.cast(rays[:10], stats=s), s)
    for mode in ("irradiance", "occlusion"):
        s = st()
        knobs({"RTW_RADIANCE_CHUNK": "30"})
        line(f"{name} probe 64 x 144 {mode} chunk 30", {"rgba": r.probe(probes, 144, DEPTH, mode=mode, stats=s)}, s)
        knobs({})
    s = st()
    line(f"{name} probe_adaptive 64 occlusion", dict(zip(("rgba", "spp", "err"), r.probe_adaptive(probes, 256, DEPTH, THRESHOLD, mode="occlusion", stats=s))), s)
    s = st()
    knobs({"RTW_RADIANCE_CHUNK": "50"})
    frames = r.views(views, W, H, 144, DEPTH, stats=s)
    line(f"{name} views 3 x 144 chunk 50", {"rgba": frames}, s)
    s = st()
    guides = r.views_guides(views, W, H, stats=s)
    line(f"{name} views_guides 3 all chunk 50", guides, s)
    knobs({})
    line(f"{name} denoise_views 3", {"rgba": r.denoise_views(frames, guides["albedo"], guides["normal"], iterations=3)})

    # ---- the device variants: torch tensors, the context's own stream
    d_rays, d_rt, d_gt, d_paths, d_probes = dev(rays), dev(ray_time), dev(gather_time), dev(paths), dev(probes)
    d_views = dev(np.frombuffer(bytes(abi.view_array(views)), np.uint8))
    torch.cuda.synchronize()
    s = st()
    out = {"t": empty(1000), "prim": empty(1000, torch.int32), "material": empty(1000, torch.int32), "normal": empty((1000, 4)), "uv": empty((1000, 2))}
    r.cast_device(1000, d_rays.data_ptr(), {k: v.data_ptr() for k, v in out.items()}, d_rt.data_ptr(), d_gt.data_ptr(), stats=s)
    line(f"{name} cast_device 1000", host(out), s)
    s = st()
    out = {"t": empty(1000), "prim": empty(1000, torch.int32)}
    r.cast_device(1000, d_rays.data_ptr(), {k: v.data_ptr() for k, v in out.items()}, mode="any", stats=s)
    line(f"{name} cast_device 1000 any", host(out), s)
    s = st()
    out = {"rgba": empty((37, 4))}
    r.radiance_device(37, d_paths.data_ptr(), out["rgba"].data_ptr(), 144, DEPTH, stats=s)
    line(f"{name} radiance_device 37 x 144", host(out), s)
    for mode in ("irradiance", "occlusion"):
        s = st()
        out = {"rgba": empty((64, 4))}
        r.probe_device(64, d_probes.data_ptr(), out["rgba"].data_ptr(), 144, DEPTH, mode=mode, stats=s)
        line(f"{name} probe_device 64 x 144 {mode}", host(out), s)
    s = st()
    out = {"sh": empty((5, 9, 4))}
    r.probe_sh_device(5, d_probes.data_ptr(), out["sh"].data_ptr(), 200, 4, stats=s)
    line(f"{name} probe_sh_device 5 x 200", host(out), s)
    for mode in ("irradiance", "occlusion"):
        s = st()
        out = {"rgba": empty((64, 4)), "spp": empty(64, torch.int32), "err": empty(64)}
        r.probe_adaptive_device(64, d_probes.data_ptr(), out["rgba"].data_ptr(), out["spp"].data_ptr(), out["err"].data_ptr(), 256, DEPTH, THRESHOLD,
                                mode=mode, stats=s)
        line(f"{name} probe_adaptive_device 64 {mode}", host(out), s)
    s = st()
    d_frames = empty((n_pix, 4))
    r.views_device(3, d_views.data_ptr(), d_frames.data_ptr(), W, H, 144, DEPTH, stats=s)
    line(f"{name} views_device 3 x 144", host({"rgba": d_frames}), s)
    s = st()
    d_guides = {"albedo": empty((n_pix, 4)), "normal": empty((n_pix, 4)), "depth": empty(n_pix), "prim": empty(n_pix, torch.int32)}
    r.views_guides_device(3, d_views.data_ptr(), {k: v.data_ptr() for k, v in d_guides.items()}, W, H, stats=s)
    line(f"{name} views_guides_device 3 all", host(d_guides), s)
    out = {"rgba": empty((n_pix, 4))}
    r.denoise_views_device(3, d_frames.data_ptr(), d_guides["albedo"].data_ptr(), d_guides["normal"].data_ptr(), out["rgba"].data_ptr(), W, H, iterations=3)
    line(f"{name} denoise_views_device 3", host(out))
    s = st()
    out = {"rgba": empty((n_pix, 4)), "spp": empty(n_pix, torch.int32), "err": empty(n_pix)}
    r.views_adaptive_device(3, d_views.data_ptr(), out["rgba"].data_ptr(), out["spp"].data_ptr(), out["err"].data_ptr(), W, H, 128, DEPTH, THRESHOLD,
                            min_spp=32, stats=s)
    line(f"{name} views_adaptive_device 3", host(out), s)
    r.close()


if __name__ == "__main__":
    for scene in UPLOADS:
        record(scene)
