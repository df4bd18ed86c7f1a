"""Rates of rtw_views_adaptive_device beside rtw_views_device (profiles/view_adaptive_rates.txt), in 4.13's method.

  python scripts/view_adaptive_rates.py [--calls 10] [--depth 50] [--positions 256] [--out profiles/view_adaptive_rates.txt]
      Two batches of scene 0, Philox: --positions positions x bake.cube_views = 6 x positions views of 32 x 32 (the cube-map batch),
      and one 512 x 512 view (the scene's own camera). Every call is timed by its own stats.seconds; the median, minimum and maximum
      of --calls calls after two warm-up calls.
      (a) overhead: rtw_views_adaptive_device at threshold 0 (every pixel runs to the cap) against rtw_views_device at spp = cap, in
          the same process, caps 256 and 1024, min_spp 64 (the default schedule), dilate 1.
      (b) thresholds 0.01, 0.02, 0.04 at cap 1024: time, sum n_p / (pixels * cap), the time against the uniform call's, the histogram
          of n_p.
      (c) the cube-map batch at threshold 0.02, cap 1024 through the host entry (host clock around the call) against the only route
          there was before: per view rtw_upload_scene of a camera-patched blob + rtw_render_adaptive, host clock around the whole
          loop, --loops loops after one warm-up; every 97th view of the loop compared with the call's in bits.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def checkpoints(min_spp, cap):
    out, n = [], min_spp
    while True:
        out.append(n)
        if n >= cap:
            return out
        n = min(cap, n + (n // 2 + 15) // 16 * 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--positions", type=int, default=256)
    ap.add_argument("--min-spp", type=int, default=64)
    ap.add_argument("--loops", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_adaptive_rates.txt"))
    a = ap.parse_args()
    import torch
    from raytracing_weekend_amd import abi, bake
    from raytracing_weekend_amd.torch_views import views_adaptive_torch, views_tensor, views_torch
    gpu = abi.Renderer(0)
    lines = [f"# rtw_views_adaptive_device beside rtw_views_device, scene 0, depth {a.depth}, Philox, min_spp {a.min_spp}, step_spp 0, dilate 1;",
             f"# every call by its own stats.seconds: median (min .. max) of {a.calls} calls after 2 warm-up calls"]
    print("\n".join(lines), flush=True)

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    def timed(fn):
        secs, last, st = [], None, None
        for i in range(a.calls + 2):
            st = abi.Stats()
            last = fn(st)
            if i >= 2:
                secs.append(st.seconds)
        return float(np.median(secs)), min(secs), max(secs), st, last

    side = 32
    blob = abi.build_scene(0, side, side)
    grid = bake.probe_grid((60.0, 60.0, 60.0), (495.0, 495.0, 495.0), 8, 8, max(1, a.positions // 64))[:a.positions, :3]
    cube = [v for k, p in enumerate(grid) for v in bake.cube_views(p, seed=1000 + k)]
    batches = [(f"{len(cube)} cube-map faces of {side} x {side}", cube, side, side),
               ("one 512 x 512 view, the scene's camera", [abi.scene_view(abi.build_scene(0, 512, 512))], 512, 512)]
    gpu.upload_scene(blob)  # (the views carry their cameras: the blob's own camera is not used)
    for what, views, w, h in batches:
        d_views = views_tensor(views, "cuda:0")
        npix = len(views) * w * h
        torch.cuda.synchronize()
        emit(f"# {what}: (a) overhead at threshold 0")
        emit("#  cap  checkpoints  uniform_s (min .. max)              adaptive_s (min .. max)             ratio   extra_s    per checkpoint")
        uniform = {}
        for cap in (256, 1024):
            k = len(checkpoints(a.min_spp, cap))
            um, ulo, uhi, ust, _ = timed(lambda st: views_torch(gpu, d_views, w, h, cap, a.depth, stats=st))
            am, alo, ahi, ast_, out = timed(lambda st: views_adaptive_torch(gpu, d_views, w, h, cap, a.depth, 0.0, min_spp=a.min_spp, stats=st))
            assert bool((out[1] == cap).all().item()) and (ast_.samples, ast_.segments) == (ust.samples, ust.segments)
            uniform[cap] = (um, ust.samples)
            emit(f"  {cap:4d}  {k:5d}        {um:.6f} ({ulo:.6f} .. {uhi:.6f})   {am:.6f} ({alo:.6f} .. {ahi:.6f})   {am / um:.3f}   {am - um:.6f}   {(am - um) / k:.6f}")
        emit(f"# {what}: (b) thresholds at cap 1024 (uniform at 1024 spp: {uniform[1024][0]:.6f} s, {uniform[1024][1] / uniform[1024][0] / 1e9:.3f} Gsamples/s)")
        emit("# threshold  adaptive_s (min .. max)             samples / (pixels * cap)   Gsamples/s   time vs uniform   n_p histogram")
        for thr in (0.01, 0.02, 0.04):
            am, alo, ahi, ast_, out = timed(lambda st: views_adaptive_torch(gpu, d_views, w, h, 1024, a.depth, thr, min_spp=a.min_spp, stats=st))
            v, c = np.unique(out[1].cpu().numpy(), return_counts=True)
            hist = " ".join(f"{int(x)}:{int(y)}" for x, y in zip(v, c))
            emit(f"  {thr:.2f}       {am:.6f} ({alo:.6f} .. {ahi:.6f})   {ast_.samples / (npix * 1024):.4f}                     {ast_.samples / am / 1e9:.3f}        {am / uniform[1024][0]:.3f}             {hist}")
        del d_views

    # (c) the cube-map batch through the host entry against an upload and an adaptive render per view
    cap, thr, nv = 1024, 0.02, len(cube)
    arr = abi.view_array(cube)
    one, host, got = [], [], None
    for i in range(a.calls + 2):
        st = abi.Stats()
        t0 = time.perf_counter()
        got = gpu.views_adaptive(arr, side, side, cap, a.depth, thr, min_spp=a.min_spp, dilate=1, stats=st)
        t1 = time.perf_counter()
        if i >= 2:
            one.append(st.seconds)
            host.append(t1 - t0)
    hdr, rest = blob[:C.sizeof(abi.SceneHeader)], blob[C.sizeof(abi.SceneHeader):]
    blobs = []
    for v in cube:  # (patching the header is not part of the timed loop)
        hd = abi.SceneHeader.from_buffer_copy(hdr)
        hd.camera, hd.camera_type = abi.Camera.from_buffer_copy(bytes(v.camera)), v.camera_type
        blobs.append(bytes(hd) + rest)
    loop, same, compared = [], True, 0
    for i in range(a.loops + 1):
        t0 = time.perf_counter()
        for k, v in enumerate(cube):
            gpu.upload_scene(blobs[k])
            img, n_p, err, _ = gpu.render_adaptive(abi.make_params(side, side, cap, a.depth, seed=v.seed), thr, min_spp=a.min_spp, dilate=1)
            if i == 0 and k % 97 == 0:
                compared += 1
                same = (same and np.array_equal(img.view(np.uint32), got[0][k].view(np.uint32)) and np.array_equal(n_p, got[1][k])
                        and np.array_equal(err.view(np.uint32), got[2][k].view(np.uint32)))
        t1 = time.perf_counter()
        if i >= 1:
            loop.append(t1 - t0)
    tail = ["#", f"# (c) {nv} views of {side} x {side}, cap {cap}, threshold {thr}, min_spp {a.min_spp}, dilate 1, depth {a.depth}, Philox",
            f"#   one rtw_views_adaptive call (host pointers, the three results copied out), median of {a.calls} after 2 warm-ups:",
            f"#     host clock around the call {np.median(host):.4f} s (min {min(host):.4f}, max {max(host):.4f}); its stats.seconds {np.median(one):.4f} s",
            f"#   {nv} x (rtw_upload_scene of a camera-patched blob + rtw_render_adaptive), host clock around the whole loop, {a.loops} loops after 1 warm-up:",
            f"#     median {np.median(loop):.4f} s (min {min(loop):.4f}, max {max(loop):.4f}) = {1e3 * np.median(loop) / nv:.3f} ms per view",
            f"#   ratio of the medians (loop / call) {np.median(loop) / np.median(host):.1f}; every 97th view of the loop ({compared} views) equals the call's "
            f"frame, counts and errors, bit for bit: {same}"]
    print("\n".join(tail), flush=True)
    gpu.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines + tail) + "\n")


if __name__ == "__main__":
    main()
