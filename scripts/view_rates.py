"""Rates of rtw_views_device beside its yardsticks and beside the route a caller had before (profiles/view_rates.txt).

  python scripts/view_rates.py [--calls 10] [--depth 50] [--out profiles/view_rates.txt]
      (i) One 1920 x 1080 view - the scene's own camera - of scenes 0 and 1 at 64 and 1024 spp, Philox. Per scene and spp, in one
          process:
            rtw_radiance_device, pixel-centre rays     the per-segment yardstick: k_radiance, the same queue and body on one fixed
                                                       ray per pixel
            rtw_views_device, the scene's camera       k_view: the camera ray of every sample made on the device
            rtw_render_device                          the specialised pipelines, which a single large frame from the uploaded
                                                       camera belongs to
          Each call is timed by its own stats.seconds; the median of --calls calls after two warm-up calls. Gseg/s =
          stats.segments / seconds.
      (ii) The case the call exists for: --positions positions x bake.cube_views = 6 x positions views of 32 x 32 at 64 spp in one
          rtw_views call (host pointers, the frames copied out: the host clock around the call, and its stats.seconds), against the
          only route there was before: per view rtw_upload_scene of a camera-patched blob + rtw_render, the host clock around the
          whole loop. The loop runs --loops times.
      scripts/probe_isa.py gives the ISA counts, and bench.py the headline, that the file keeps below the rates.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def centre_rays(blob, w, h):
    """(w * h, 8) float32: the ray through every pixel's centre from the blob's perspective camera without its lens."""
    from raytracing_weekend_amd import abi
    c = np.frombuffer(bytes(abi.scene_view(blob).camera), np.float32)
    o, ll, hor, ver = c[0:3], c[12:15], c[15:18], c[18:21]
    s = ((np.arange(w, dtype=np.float32) + np.float32(0.5)) / np.float32(w))[None, :, None]
    t = ((np.arange(h, dtype=np.float32) + np.float32(0.5)) / np.float32(h))[:, None, None]
    d = (ll + s * hor + t * ver - o).astype(np.float32).reshape(-1, 3)
    rays = np.empty((w * h, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, d, np.float32(1e-6), np.float32(1e27)
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--spp", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080])
    ap.add_argument("--positions", type=int, default=256)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_rates.txt"))
    a = ap.parse_args()
    import torch
    from raytracing_weekend_amd import abi, bake
    from raytracing_weekend_amd.torch_radiance import radiance_torch
    from raytracing_weekend_amd.torch_views import views_tensor, views_torch
    gpu = abi.Renderer(0)
    w, h = a.size
    lines = [f"# (i) rtw_views_device beside its yardsticks: one {w} x {h} view (the scene's own camera), depth {a.depth}, Philox; median of {a.calls} calls",
             "# after 2 warm-up calls, every call by its own stats.seconds; Gseg/s = stats.segments / seconds; vs = Gseg/s over the yardstick's",
             "# scene spp   route                                   median_s   min_s      max_s      segments        Gseg/s   vs k_radiance"]
    print("\n".join(lines), flush=True)
    for scene in (0, 1):
        blob = abi.build_scene(scene, w, h)
        gpu.upload_scene(blob)
        d_rays = torch.from_numpy(centre_rays(blob, w, h)).cuda()
        d_views = views_tensor([abi.scene_view(blob)], "cuda:0")
        d_img = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()

        def radiance_call(spp):
            st = abi.Stats()
            radiance_torch(gpu, d_rays, spp, a.depth, stats=st)
            return st.seconds, st.segments

        def views_call(spp):
            st = abi.Stats()
            views_torch(gpu, d_views, w, h, spp, a.depth, stats=st)
            return st.seconds, st.segments

        def render_call(spp):
            st = gpu.render_device(abi.make_params(w, h, spp, a.depth), d_img.data_ptr())
            return st.seconds, st.segments

        yard = "rtw_radiance_device, pixel-centre rays"
        routes = [(yard, radiance_call), ("rtw_views_device, the scene's camera", views_call), ("rtw_render_device", render_call)]
        for spp in a.spp:
            rate = {}
            for name, fn in routes:
                secs, count = [], 0
                for i in range(a.calls + 2):
                    s, count = fn(spp)
                    if i >= 2:
                        secs.append(s)
                med = float(np.median(secs))
                rate[name] = count / med / 1e9
                ratio = "" if name == yard else f"{rate[name] / rate[yard]:.3f}"
                line = f"  {scene}     {spp:5d} {name:39s} {med:.6f}   {min(secs):.6f}   {max(secs):.6f}   {count:13d}  {rate[name]:7.3f}   {ratio}"
                lines.append(line)
                print(line, flush=True)
        del d_rays, d_views, d_img

    # (ii) many small views: one call against an upload and a render per view
    side, spp, nv = 32, 64, 6 * a.positions
    blob = abi.build_scene(0, side, side)
    grid = bake.probe_grid((60.0, 60.0, 60.0), (495.0, 495.0, 495.0), 8, 8, max(1, a.positions // 64))[:a.positions, :3]
    views = [v for k, p in enumerate(grid) for v in bake.cube_views(p, seed=1000 + k)]
    arr = abi.view_array(views)
    gpu.upload_scene(blob)
    one, host = [], []
    for i in range(a.calls + 2):
        st = abi.Stats()
        t0 = time.perf_counter()
        frames = gpu.views(arr, side, side, spp, a.depth, stats=st)
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
    loop, same = [], True
    for i in range(a.loops + 1):
        t0 = time.perf_counter()
        for k, v in enumerate(views):
            gpu.upload_scene(blobs[k])
            img, _ = gpu.render(abi.make_params(side, side, spp, a.depth, seed=v.seed))
            if i == 0 and k % 97 == 0:
                same = same and np.array_equal(img.view(np.uint32), frames[k].view(np.uint32))
        t1 = time.perf_counter()
        if i >= 1:
            loop.append(t1 - t0)
    tail = ["#", f"# (ii) {nv} views of {side} x {side} at {spp} spp, depth {a.depth}, Philox: {a.positions} positions in the Cornell box x bake.cube_views",
            f"#   one rtw_views call (host pointers, frames copied out), median of {a.calls} after 2 warm-ups:",
            f"#     host clock around the call {np.median(host):.4f} s (min {min(host):.4f}, max {max(host):.4f}); its stats.seconds {np.median(one):.4f} s",
            f"#   {nv} x (rtw_upload_scene of a camera-patched blob + rtw_render), host clock around the whole loop, {a.loops} loops after 1 warm-up:",
            f"#     median {np.median(loop):.4f} s (min {min(loop):.4f}, max {max(loop):.4f}) = {1e3 * np.median(loop) / nv:.3f} ms per view",
            f"#   ratio of the medians (loop / call) {np.median(loop) / np.median(host):.1f}; every {97}th frame of the loop equals the call's, bit for bit: {same}"]
    print("\n".join(tail), flush=True)
    gpu.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines + tail) + "\n")


if __name__ == "__main__":
    main()
