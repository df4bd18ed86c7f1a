"""Samples and records per second of rtw_paths_device (profiles/paths_rates.txt) and its yardstick, rtw_radiance_device
on the same rays and params.

  python scripts/paths_rates.py [--log2n 20] [--spp 16] [--depth 8] [--calls 10]
      scene 0 with camera-coherent rays (the scene's camera through the pixel centres of a 2^(log2n / 2)-pixel-square image, in scan
      order) and with geometry_ref.scene_rays' incoherent mix; rtw_radiance_device, then rtw_paths_device with max_records 0, 2 and
      the depth, into buffers allocated once: the median of the call's own stats.seconds over --calls calls after two warm-up calls.
      A record is a vertex the call wrote: sum of min(segments, max_records) over the samples.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from cast_rates import ray_set


def main(args):
    import torch
    from raytracing_weekend_amd import abi
    from raytracing_weekend_amd.torch_radiance import radiance_torch
    gpu = abi.Renderer(0)
    n = 1 << (args.log2n // 2 * 2)
    print(f"# rtw_paths_device against rtw_radiance_device, scene 0, {n} rays per call, {args.spp} spp, depth {args.depth}, "
          f"median of {args.calls} calls after 2 warm-up calls, stats.seconds of the call")
    print("# rays        call                 median_s   min_s      max_s      Msamples/s  Mrecords/s  segments/sample  x radiance")
    for kind in ("coherent", "incoherent"):
        blob, rays = ray_set(0, kind, args.log2n)
        gpu.upload_scene(blob)
        d_rays = torch.from_numpy(rays).cuda()
        pairs = n * args.spp

        def timed(call):
            secs, st = [], None
            for i in range(args.calls + 2):
                st = abi.Stats()
                call(st)
                if i >= 2:
                    secs.append(st.seconds)
            return secs, st

        def row(label, secs, st, records):
            med = float(np.median(secs))
            print(f"  {kind:11s} {label:20s} {med:.6f}   {min(secs):.6f}   {max(secs):.6f}   {pairs / med / 1e6:10.1f}  {records / med / 1e6:10.1f}  "
                  f"{st.segments / pairs:15.3f}  {med / base:10.3f}", flush=True)
        secs, st = timed(lambda st: radiance_torch(gpu, d_rays, args.spp, args.depth, stats=st))
        base = float(np.median(secs))
        row("radiance", secs, st, 0)
        d_heads = torch.zeros((pairs, 8), dtype=torch.float32, device="cuda:0")
        for k in sorted({0, min(2, args.depth), args.depth}):
            d_vertices = torch.zeros((pairs * k, 16), dtype=torch.float32, device="cuda:0") if k else None
            torch.cuda.synchronize()
            secs, st = timed(lambda st: gpu.paths_device(n, d_rays.data_ptr(), d_heads.data_ptr(), d_vertices.data_ptr() if k else 0, args.spp,
                                                         args.depth, k, stats=st))
            segments = d_heads[:, 3].contiguous().view(torch.int32)
            assert int(segments.sum().item()) == st.segments
            row(f"paths max_records {k}", secs, st, int(torch.clamp(segments, max=k).sum().item()))
            del d_vertices
        del d_heads, d_rays
    gpu.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--calls", type=int, default=10)
    main(ap.parse_args())
