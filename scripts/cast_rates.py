"""Rays per second of rtw_cast_device (profiles/cast_rates.txt) and its yardstick, k_debug_intersect's kernel time.

  python scripts/cast_rates.py [--log2n 24] [--calls 10]
      scenes 0 (candidate lists) and 1 (528 spheres, the tree), each with camera-coherent rays (the scene's camera through the
      pixel centres of a 2^(log2n / 2)-pixel-square image, in scan order) and with geometry_ref.scene_rays' incoherent mix;
      closest (t and prim only), closest (all five outputs) and any: the median of the call's own stats.seconds over --calls calls
      after two warm-up calls.
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/cast_rates.py --yardstick
      the same four ray sets through rtw_debug_intersect (one thread per ray, one workgroup per 256 rays) and through rtw_cast
      (closest, t and prim only, the whole batch in one chunk: one launch, as rtw_cast_device makes it), one warm-up call and
      --calls timed ones each; then
  python scripts/cast_rates.py --summarize DIR
      prints the median kernel times of k_debug_intersect and k_cast per ray set from the trace.
"""
import argparse
import csv
import ctypes as C
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SETS = [(0, "coherent"), (0, "incoherent"), (1, "coherent"), (1, "incoherent")]


def ray_set(scene, kind, log2n):
    import geometry_ref as G
    from raytracing_weekend_amd import abi
    side = 1 << (log2n // 2)
    n = side * side
    blob = abi.build_scene(scene, side, side)
    if kind == "incoherent":
        return blob, G.scene_rays(blob, G.RAY_SEED, n)[0]
    hdr = abi.SceneHeader.from_buffer_copy(blob[:C.sizeof(abi.SceneHeader)])
    ys, xs = np.mgrid[0:side, 0:side]
    o, d = G.camera_rays(hdr, (xs.ravel() + 0.5) / side, (ys.ravel() + 0.5) / side)
    rays = np.empty((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, d, 1e-6, 1e27
    return blob, rays


def rates(args):
    import torch
    from raytracing_weekend_amd import abi
    from raytracing_weekend_amd.torch_cast import cast_torch
    gpu = abi.Renderer(0)
    print(f"# rtw_cast_device, {1 << (args.log2n // 2 * 2)} rays per call, median of {args.calls} calls after 2 warm-up calls, stats.seconds of the call")
    print("# scene rays        mode            median_s   min_s      max_s      Grays/s  hit_share")
    for scene, kind in SETS:
        blob, rays = ray_set(scene, kind, args.log2n)
        gpu.upload_scene(blob)
        d_rays = torch.from_numpy(rays).cuda()
        modes = (("closest t,prim", "closest", ("t", "prim")), ("closest all", "closest", abi.CAST_OUTPUTS), ("any", "any", ("t", "prim")))
        for label, mode, want in modes[:1] if args.quick else modes:
            secs = []
            for i in range(args.calls + 2):
                st = abi.Stats()
                out = cast_torch(gpu, d_rays, mode=mode, want=want, stats=st)
                if i >= 2:
                    secs.append(st.seconds)
            hit = float((out["prim"] >= 0).float().mean())
            print(f"  {scene}     {kind:11s} {label:15s} {np.median(secs):.6f}   {min(secs):.6f}   {max(secs):.6f}   {len(rays) / np.median(secs) / 1e9:7.3f}  {hit:.3f}", flush=True)
            del out
        del d_rays
    gpu.close()


def yardstick(args):
    from raytracing_weekend_amd import abi
    os.environ["RTW_CAST_CHUNK"] = str(1 << 30)  # one k_cast launch per call, as rtw_cast_device makes it
    gpu = abi.Renderer(0)
    for scene, kind in SETS:
        blob, rays = ray_set(scene, kind, args.log2n)
        gpu.upload_scene(blob)
        for _ in range(args.calls + 1):
            gpu.debug_intersect(rays)
        for _ in range(args.calls + 1):
            gpu.cast(rays, want=("t", "prim"))
        print("done", scene, kind, flush=True)
    gpu.close()


def summarize(args):
    files = glob.glob(os.path.join(args.summarize, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = args.calls + 1
    n = 1 << (args.log2n // 2 * 2)
    launches = 1  # (--yardstick sets RTW_CAST_CHUNK above the batch: one launch per call)
    print(f"# kernel time from rocprofv3 --kernel-trace, {n} rays per call, median of {args.calls} calls after 1 warm-up call")
    print("# scene rays        kernel              median_s   Grays/s")
    for name, group in (("k_debug_intersect", per), ("k_cast", per * launches)):
        mine = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in rows if name in r["Kernel_Name"]]
        assert len(mine) == group * len(SETS), (name, len(mine))
        for k, (scene, kind) in enumerate(SETS):
            calls = np.array(mine[k * group:(k + 1) * group]).reshape(per, -1).sum(1)[1:]
            print(f"  {scene}     {kind:11s} {name:19s} {np.median(calls):.6f}   {n / np.median(calls) / 1e9:7.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--quick", action="store_true", help="closest (t, prim) only: for sweeps of RTW_CAST_GRID_MULT")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    summarize(a) if a.summarize else yardstick(a) if a.yardstick else rates(a)
