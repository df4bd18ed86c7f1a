"""Rates of rtw_views_guides and rtw_denoise_views beside the routes a caller had before (profiles/view_guides_rates.txt).

  python scripts/view_guides_rates.py [--calls 10] [--positions 256] [--out profiles/view_guides_rates.txt]
      (i)   6 x positions views of 32 x 32 at 16 spp from bake.cube_views (positions on a grid in the Cornell box): one
            rtw_views_guides call (host pointers, all four buffers copied out: the host clock around the call, and its stats.seconds)
            against per view rtw_upload_scene of a camera-patched blob + rtw_render_guides, the host clock around the whole loop. Every
            97th view of the loop is compared with the call's for equality.
      (ii)  The same frames (rtw_views at 16 spp, display-encoded) and their guides through 5 passes: one rtw_denoise_views_device call
            on device tensors, timed by events on its stream, against one rtw_denoise_guided call per frame (host pointers, the
            only route there was), the host clock around the loop; and one rtw_denoise_views call (host pointers), host clock.
      (iii) One 1920 x 1080 view - the scene's own camera - of scenes 0 and 1 at 16 spp: rtw_views_guides_device against
            rtw_render_guides, each by its own stats.seconds, which spans the kernel alone in both.
      Medians of --calls calls after two warm-up calls; the loops run --loops times after one warm-up loop.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def med(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--positions", type=int, default=256)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_guides_rates.txt"))
    a = ap.parse_args()
    import torch
    from raytracing_weekend_amd import abi, bake
    from raytracing_weekend_amd.torch_views import denoise_views_torch, views_guides_torch, views_tensor
    gpu = abi.Renderer(0)
    side, spp, nv = 32, 16, 6 * a.positions
    blob = abi.build_scene(0, side, side)
    grid = bake.probe_grid((60.0, 60.0, 60.0), (495.0, 495.0, 495.0), 8, 8, max(1, a.positions // 64))[:a.positions, :3]
    views = [v for k, p in enumerate(grid) for v in bake.cube_views(p, seed=1000 + k)]
    arr = abi.view_array(views)
    gpu.upload_scene(blob)

    # (i) the guides of many small views: one call against an upload and a guide pass per view
    one, host = [], []
    for i in range(a.calls + 2):
        st = abi.Stats()
        t0 = time.perf_counter()
        guides = gpu.views_guides(arr, side, side, spp, stats=st)
        t1 = time.perf_counter()
        if i >= 2:
            one.append(st.seconds)
            host.append(t1 - t0)
    hdr, rest = blob[:C.sizeof(abi.SceneHeader)], blob[C.sizeof(abi.SceneHeader):]
    blobs = []
    for v in views:  # (patching the header is not part of the timed loop)
        hd = abi.SceneHeader.from_buffer_copy(hdr)
        hd.camera, hd.camera_type = abi.Camera.from_buffer_copy(bytes(v.camera)), v.camera_type
        blobs.append(bytes(hd) + rest)
    loop, same, kernel = [], True, []
    for i in range(a.loops + 1):
        ksum = 0.0
        t0 = time.perf_counter()
        for k, v in enumerate(views):
            gpu.upload_scene(blobs[k])
            st = abi.Stats()
            g = gpu.render_guides(abi.make_params(side, side, spp, 0, seed=v.seed), stats=st)
            ksum += st.seconds
            if i == 0 and k % 97 == 0:
                same = same and all(np.array_equal(g[n].view(np.uint32), guides[n][k].view(np.uint32)) for n in abi.GUIDES)
        t1 = time.perf_counter()
        if i >= 1:
            loop.append(t1 - t0)
            kernel.append(ksum)
    hit = float((guides["prim"] >= 0).mean())
    lines = [f"# (i) {nv} views of {side} x {side} at {spp} spp, Philox: {a.positions} positions in the Cornell box x bake.cube_views; {hit:.3f} of the pixels hit",
             f"#   one rtw_views_guides call (host pointers, four buffers copied out), median of {a.calls} after 2 warm-ups:",
             f"#     host clock around the call {med(host):.4f} s (min {min(host):.4f}, max {max(host):.4f}); its stats.seconds {med(one):.5f} s",
             f"#   {nv} x (rtw_upload_scene of a camera-patched blob + rtw_render_guides), host clock around the whole loop, {a.loops} loops after 1 warm-up:",
             f"#     median {med(loop):.4f} s (min {min(loop):.4f}, max {max(loop):.4f}) = {1e3 * med(loop) / nv:.3f} ms per view; the sum of the calls'",
             f"#     stats.seconds (the k_guides launches alone) {med(kernel):.4f} s",
             f"#   ratio of the medians (loop / call) {med(loop) / med(host):.1f}; every 97th view of the loop equals the call's, bit for bit: {same}"]
    print("\n".join(lines), flush=True)

    # (ii) the denoiser over the same frames
    gpu.upload_scene(blob)
    frames = gpu.views(arr, side, side, spp, 8)
    frames[..., :3] = np.sqrt(np.clip(np.nan_to_num(frames[..., :3], nan=0.0), 0.0, 1.0))  # the display encoding
    alb, nrm = guides["albedo"], guides["normal"]
    d = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (frames, alb, nrm)]
    stream = torch.cuda.Stream(device="cuda:0")
    dev = []
    with torch.cuda.stream(stream):
        for i in range(a.calls + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            out = denoise_views_torch(gpu, *d, iterations=5)
            e1.record(stream)
            e1.synchronize()
            if i >= 2:
                dev.append(e0.elapsed_time(e1) * 1e-3)
    hostcall = []
    for i in range(a.calls + 2):
        t0 = time.perf_counter()
        out_h = gpu.denoise_views(frames, alb, nrm, iterations=5)
        t1 = time.perf_counter()
        if i >= 2:
            hostcall.append(t1 - t0)
    dloop, dsame = [], np.array_equal(out.cpu().numpy().view(np.uint32), out_h.view(np.uint32))
    for i in range(a.loops + 1):
        t0 = time.perf_counter()
        for k in range(nv):
            f = gpu.denoise_guided(frames[k], alb[k], nrm[k], iterations=5)
            if i == 0 and k % 97 == 0:
                dsame = dsame and np.array_equal(f.view(np.uint32), out_h[k].view(np.uint32))
        t1 = time.perf_counter()
        if i >= 1:
            dloop.append(t1 - t0)
    tail = ["#", f"# (ii) the same {nv} frames (rtw_views at {spp} spp, display-encoded) with their guides, 5 passes:",
            f"#   one rtw_denoise_views_device call on device tensors, events on its stream, median of {a.calls} after 2 warm-ups:",
            f"#     {med(dev):.6f} s (min {min(dev):.6f}, max {max(dev):.6f})",
            f"#   one rtw_denoise_views call (host pointers, three buffers in, one out), host clock: {med(hostcall):.4f} s (min {min(hostcall):.4f}, max {max(hostcall):.4f})",
            f"#   {nv} x rtw_denoise_guided (host pointers), host clock around the whole loop, {a.loops} loops after 1 warm-up:",
            f"#     median {med(dloop):.4f} s (min {min(dloop):.4f}, max {max(dloop):.4f}) = {1e3 * med(dloop) / nv:.3f} ms per frame",
            f"#   ratio of the medians: loop / device call {med(dloop) / med(dev):.0f}, loop / host call {med(dloop) / med(hostcall):.1f}; the three routes agree bit for bit",
            f"#   (device and host call everywhere, every 97th frame of the loop): {dsame}"]
    print("\n".join(tail), flush=True)
    del d, out

    # (iii) one large view: the view kernel beside k_guides
    w, h = a.size
    tail += ["#", f"# (iii) one {w} x {h} view (the scene's own camera) at {spp} spp, Philox; each call by its own stats.seconds (the kernel alone); median of {a.calls}",
             "# after 2 warm-ups; Msamples/s = stats.samples / seconds; vs = seconds over rtw_render_guides'",
             "# scene route                       median_s   min_s      max_s      Msamples/s   vs k_guides"]
    print("\n".join(tail[-4:]), flush=True)
    for scene in (0, 1):
        blob = abi.build_scene(scene, w, h)
        gpu.upload_scene(blob)
        d_views = views_tensor([abi.scene_view(blob)], "cuda:0")
        torch.cuda.synchronize()

        def guides_call():
            st = abi.Stats()
            gpu.render_guides(abi.make_params(w, h, spp, 0), stats=st)
            return st

        def views_call():
            st = abi.Stats()
            views_guides_torch(gpu, d_views, w, h, spp, stats=st)
            return st
        secs = {}
        for r in range(2):  # the two routes alternate, twice
            for name, fn in (("rtw_render_guides", guides_call), ("rtw_views_guides_device", views_call)):
                for i in range(a.calls // 2 + 2):
                    st = fn()
                    if i >= 2:
                        secs.setdefault(name, []).append(st.seconds)
        base = med(secs["rtw_render_guides"])
        for name in ("rtw_render_guides", "rtw_views_guides_device"):
            s = secs[name]
            line = f"  {scene}     {name:27s} {med(s):.6f}   {min(s):.6f}   {max(s):.6f}   {w * h * spp / med(s) / 1e6:10.1f}   {med(s) / base:.3f}"
            tail.append(line)
            print(line, flush=True)
    gpu.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines + tail) + "\n")


if __name__ == "__main__":
    main()
