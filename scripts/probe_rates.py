"""Rates of rtw_probe_device beside its yardsticks (profiles/probe_rates.txt).

  python scripts/probe_rates.py [--calls 10] [--depth 50] [--side 512] [--out profiles/probe_rates.txt]
      Probes: a side x side bake of the Cornell floor (scene 0: bake.rect_probes), and as many probes on scene 1's surfaces (the hits
      of the camera's rays through a side x side frame, lifted 1e-3 along the normal turned against the ray; misses are filled by
      repeating hits). spp 64 and 1024, Philox. Per scene and spp:
        rtw_probe_device irradiance / occlusion   the library's integrated probes
        rtw_radiance_device along the normals     the kernel-speed yardstick: the same queue and body without the direction generator
        torch rays + rtw_radiance_device spp 1    the route a caller had before: n * spp cosine-weighted rays generated in torch,
                                                  one path each, the mean taken in torch (the whole route timed by torch events)
        torch rays + rtw_cast_device any          the same for occlusion
      Each library call is timed by its own stats.seconds; the median of --calls calls after two warm-up calls. scripts/probe_isa.py
      gives the ISA counts that the file keeps below the rates.
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def scene1_probes(gpu, blob, side):
    import geometry_ref as G
    from raytracing_weekend_amd import abi
    hdr = abi.SceneHeader.from_buffer_copy(blob[:C.sizeof(abi.SceneHeader)])
    ys, xs = np.mgrid[0:side, 0:side]
    o, d = G.camera_rays(hdr, (xs.ravel() + 0.5) / side, (ys.ravel() + 0.5) / side)
    rays = np.empty((side * side, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, d, 1e-6, 1e27
    h = gpu.cast(rays, want=("t", "prim", "normal"))
    hit = np.nonzero(h["prim"] >= 0)[0]
    hit = np.resize(hit, side * side)
    n = h["normal"][hit, :3].astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    dd = rays[hit, 3:6].astype(np.float64)
    n[(n * dd).sum(1) > 0] *= -1.0
    probes = np.empty((side * side, 8), np.float32)
    probes[:, 0:3] = rays[hit, 0:3].astype(np.float64) + dd * h["t"][hit, None].astype(np.float64) + 1e-3 * n
    probes[:, 3:6], probes[:, 6], probes[:, 7] = n, 1e-6, 1e27
    return probes


def torch_rays(torch, d_probes, spp, gen):
    """n * spp cosine-weighted rays about the probes' normals, generated in torch (sample-major per probe)."""
    n = d_probes.shape[0]
    w = torch.nn.functional.normalize(d_probes[:, 3:6], dim=1)
    a = torch.where((w[:, :1].abs() > 0.9), torch.tensor([0.0, 1.0, 0.0], device=w.device), torch.tensor([1.0, 0.0, 0.0], device=w.device))
    v = torch.nn.functional.normalize(torch.linalg.cross(w, a), dim=1)
    u = torch.linalg.cross(w, v)
    r = torch.rand((n, spp, 2), device=w.device, generator=gen)
    phi, sq = 2 * np.pi * r[..., 0], r[..., 1].sqrt()
    lx, ly, lz = phi.cos() * sq, phi.sin() * sq, (1 - r[..., 1]).sqrt()
    d = lz[..., None] * w[:, None] + ly[..., None] * v[:, None] + lx[..., None] * u[:, None]
    rays = torch.empty((n, spp, 8), dtype=torch.float32, device=w.device)
    rays[..., 0:3] = d_probes[:, None, 0:3]
    rays[..., 3:6] = d
    rays[..., 6:8] = d_probes[:, None, 6:8]
    return rays.view(n * spp, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--spp", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_rates.txt"))
    a = ap.parse_args()
    import torch
    from raytracing_weekend_amd import abi, bake
    from raytracing_weekend_amd.torch_cast import cast_torch
    from raytracing_weekend_amd.torch_probe import probe_torch
    from raytracing_weekend_amd.torch_radiance import radiance_torch
    gpu = abi.Renderer(0)
    n = a.side * a.side
    lines = [f"# rtw_probe_device beside its yardsticks, {n} probes ({a.side}x{a.side}), depth {a.depth}, Philox; median of {a.calls} calls after 2 warm-up",
             "# calls; library calls by their own stats.seconds, the torch routes (ray generation + call + mean) by torch events;",
             "# Gseg/s = stats.segments / seconds (irradiance, radiance), Grays/s = stats.shadow_rays / seconds (occlusion, cast)",
             "# scene spp   route                                   median_s   min_s      max_s      segments|rays   G/s      vs yardstick"]
    print("\n".join(lines), flush=True)
    gen = torch.Generator(device="cuda:0")
    for scene in (0, 1):
        blob = abi.build_scene(scene, a.side, a.side)
        gpu.upload_scene(blob)
        if scene == 0:
            prims = abi.parse_scene(blob)["prims"]
            floor = next(i for i, p in enumerate(prims) if p.type == abi.PRIM_RECT_Y and p.p[4] == 0.0 and p.xform == 0)
            probes = bake.rect_probes(blob, floor, a.side, a.side)
        else:
            probes = scene1_probes(gpu, blob, a.side)
        occ = probes.copy()
        occ[:, 7] = 150.0 if scene == 0 else 3.0  # occlusion distances of the scenes' sizes
        d_probes, d_occ = torch.from_numpy(probes).cuda(), torch.from_numpy(occ).cuda()
        torch.cuda.synchronize()

        def lib_call(what, spp):
            st = abi.Stats()
            if what == "irradiance":
                probe_torch(gpu, d_probes, spp, a.depth, stats=st)
            elif what == "occlusion":
                probe_torch(gpu, d_occ, spp, a.depth, mode="occlusion", stats=st)
            else:
                radiance_torch(gpu, d_probes, spp, a.depth, stats=st)
            return st.seconds, st.shadow_rays if what == "occlusion" else st.segments

        def torch_route(what, spp):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = abi.Stats()
            e0.record()
            rays = torch_rays(torch, d_probes if what == "radiance" else d_occ, spp, gen)
            if what == "radiance":
                out = radiance_torch(gpu, rays, 1, a.depth, stats=st).view(n, spp, 4).mean(1) * np.pi
            else:
                out = (cast_torch(gpu, rays, mode="any", want=("prim",), stats=st)["prim"].view(n, spp) < 0).float().mean(1)
            e1.record()
            torch.cuda.synchronize()
            del rays, out
            return e0.elapsed_time(e1) * 1e-3, st.segments if what == "radiance" else st.shadow_rays

        routes = [("rtw_radiance_device along the normals", lambda spp: lib_call("radiance", spp), None),
                  ("rtw_probe_device irradiance", lambda spp: lib_call("irradiance", spp), "rtw_radiance_device along the normals"),
                  ("torch rays + rtw_radiance_device spp 1", lambda spp: torch_route("radiance", spp), "rtw_radiance_device along the normals"),
                  ("rtw_probe_device occlusion", lambda spp: lib_call("occlusion", spp), None),
                  ("torch rays + rtw_cast_device any", lambda spp: torch_route("cast", spp), "rtw_probe_device occlusion")]
        for spp in a.spp:
            rate = {}
            for name, fn, yard in routes:
                secs, count = [], 0
                for i in range(a.calls + 2):
                    s, count = fn(spp)
                    if i >= 2:
                        secs.append(s)
                med = float(np.median(secs))
                rate[name] = count / med / 1e9
                ratio = f"{rate[name] / rate[yard]:.3f}" if yard else ""
                line = f"  {scene}     {spp:5d} {name:39s} {med:.6f}   {min(secs):.6f}   {max(secs):.6f}   {count:13d}  {rate[name]:7.3f}   {ratio}"
                lines.append(line)
                print(line, flush=True)
        del d_probes, d_occ
    gpu.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
