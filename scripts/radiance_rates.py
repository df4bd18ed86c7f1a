"""Segments per second of rtw_radiance_device beside rtw_render_device on the same frame (profiles/radiance_rates.txt).

  python scripts/radiance_rates.py [--calls 10] [--depth 50] [--out profiles/radiance_rates.txt]
      scenes 0 (candidate lists: rtw_render takes k_path) and 1 (the tree: rtw_render takes the wavefront pipeline). The rays are the
      scene camera's rays through the pixel centres of a 1920x1080 frame, in scan order, ray i on the stream of pixel i; spp 64 and
      1024. Each call is timed by its own stats.seconds; the median of --calls calls after two warm-up calls. rtw_render_device runs
      in the same process on the same scene, frame size, spp and depth. The two trace different paths (the render jitters its camera
      rays inside the pixel), so the comparison is segments per second, not seconds per call.
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

W, H = 1920, 1080


def camera_rays(blob):
    import geometry_ref as G
    from raytracing_weekend_amd import abi
    hdr = abi.SceneHeader.from_buffer_copy(blob[:C.sizeof(abi.SceneHeader)])
    ys, xs = np.mgrid[0:H, 0:W]
    o, d = G.camera_rays(hdr, (xs.ravel() + 0.5) / W, (ys.ravel() + 0.5) / H)
    rays = np.empty((W * H, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, d, 1e-6, 1e27
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--spp", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance_rates.txt"))
    a = ap.parse_args()
    import torch
    from raytracing_weekend_amd import abi
    from raytracing_weekend_amd.torch_radiance import radiance_torch
    gpu = abi.Renderer(0)
    lines = [f"# rtw_radiance_device beside rtw_render_device, {W}x{H} (rays: the camera's through the pixel centres), depth {a.depth}, Philox;",
             f"# median of {a.calls} calls after 2 warm-up calls, each call's own stats.seconds; Gseg/s = stats.segments / seconds",
             "# scene spp   call                 median_s   min_s      max_s      segments      Gseg/s   Gsamples/s  radiance/render (Gseg/s)"]
    print("\n".join(lines), flush=True)
    frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    for scene in (0, 1):
        blob = abi.build_scene(scene, W, H)
        gpu.upload_scene(blob)
        d_rays = torch.from_numpy(camera_rays(blob)).cuda()
        torch.cuda.synchronize()
        for spp in a.spp:
            res = {}
            for what in ("rtw_render_device", "rtw_radiance_device"):
                secs, st = [], None
                for i in range(a.calls + 2):
                    if what == "rtw_render_device":
                        st = gpu.render_device(abi.make_params(W, H, spp, a.depth), frame.data_ptr())
                    else:
                        st = abi.Stats()
                        out = radiance_torch(gpu, d_rays, spp, a.depth, stats=st)
                        del out
                    if i >= 2:
                        secs.append(st.seconds)
                med = float(np.median(secs))
                res[what] = st.segments / med / 1e9
                ratio = f"{res['rtw_radiance_device'] / res['rtw_render_device']:.3f}" if what == "rtw_radiance_device" else ""
                line = (f"  {scene}     {spp:5d} {what:20s} {med:.6f}   {min(secs):.6f}   {max(secs):.6f}   {st.segments:12d}  {res[what]:7.3f}  "
                        f"{st.samples / med / 1e9:7.3f}     {ratio}")
                lines.append(line)
                print(line, flush=True)
        del d_rays
    gpu.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
