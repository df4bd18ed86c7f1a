"""Rates of rtw_probe_sh_device beside the route a caller had before and the per-segment yardstick (profiles/probe_sh_rates.txt,
DESIGN.md 4.11).

  python scripts/probe_sh_rates.py [--calls 10] [--depth 50] [--side 64] [--out profiles/probe_sh_rates.txt]
      Points: a side^3 bake.probe_grid inside the Cornell box (scene 0) and as many points over scene 1's ground. spp 64 and 1024,
      Philox. Per scene and spp:
        rtw_probe_sh_device                        the library's integrated light probes
        torch rays + rtw_radiance_device spp 1     the route a caller had before: n * spp uniform directions generated in torch, one
                                                   path each, the projection onto the nine basis functions in torch (the whole route
                                                   timed by torch events)
        rtw_probe_device irradiance, normal +y     the per-segment yardstick: the same queue and body on the same positions, three
                                                   running sums instead of 27
      Each library call is timed by its own stats.seconds; the median of --calls calls after two warm-up calls.
      Then, on 64 points of the Cornell box at --check-spp samples: bake.sh_irradiance of rtw_probe_sh's coefficients at +y against
      rtw_probe's irradiance at the same point and normal - the error of truncating the radiance at band 2.
      scripts/probe_isa.py gives the ISA counts that the file keeps below the rates.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def torch_route(torch, gpu, radiance_torch, d_points, spp, depth, gen):
    """n * spp uniform directions in torch, rtw_radiance_device at spp 1, the projection in torch: (n, 9, 3) coefficients."""
    n = d_points.shape[0]
    r = torch.rand((n, spp, 2), device=d_points.device, generator=gen)
    z = 1 - 2 * r[..., 1]
    sq, phi = (1 - z * z).clamp_min(0).sqrt(), 2 * np.pi * r[..., 0]
    x, y = phi.cos() * sq, phi.sin() * sq
    rays = torch.empty((n, spp, 8), dtype=torch.float32, device=d_points.device)
    rays[..., 0:3] = d_points[:, None, 0:3]
    rays[..., 3], rays[..., 4], rays[..., 5] = x, y, z
    rays[..., 6:8] = d_points[:, None, 6:8]
    st_rad = radiance_torch(gpu, rays.view(n * spp, 8), 1, depth).view(n, spp, 4)[..., :3]
    basis = torch.stack([torch.full_like(x, 0.282094792), 0.488602512 * y, 0.488602512 * z, 0.488602512 * x, 1.092548431 * x * y,
                         1.092548431 * y * z, 0.315391565 * (3 * z * z - 1), 1.092548431 * x * z, 0.546274215 * (x * x - y * y)], dim=-1)
    return torch.einsum("nsj,nsc->njc", basis, st_rad) * (4 * np.pi / spp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--spp", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--check-spp", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_sh_rates.txt"))
    a = ap.parse_args()
    import torch
    from raytracing_weekend_amd import abi, bake
    from raytracing_weekend_amd.torch_probe import probe_torch
    from raytracing_weekend_amd.torch_probe_sh import probe_sh_torch
    from raytracing_weekend_amd.torch_radiance import radiance_torch
    gpu = abi.Renderer(0)
    n = a.side ** 3
    lines = [f"# rtw_probe_sh_device beside its yardsticks, {n} points ({a.side}^3 bake.probe_grid), depth {a.depth}, Philox; median of {a.calls} calls after",
             "# 2 warm-up calls; library calls by their own stats.seconds, the torch route (directions + call + projection) by torch events;",
             "# Gseg/s = stats.segments / seconds",
             "# scene spp   route                                   median_s   min_s      max_s      segments        Gseg/s   vs yardstick"]
    print("\n".join(lines), flush=True)
    gen = torch.Generator(device="cuda:0")
    grids = {0: ((20.0, 20.0, 20.0), (535.0, 535.0, 535.0)), 1: ((-11.0, 0.25, -11.0), (11.0, 6.0, 11.0))}
    for scene in (0, 1):
        gpu.upload_scene(abi.build_scene(scene, 64, 64))
        points = bake.probe_grid(*grids[scene], a.side, a.side, a.side)
        points[:, 4] = 1.0  # the yardstick's normal; rtw_probe_sh does not read it
        d_points = torch.from_numpy(points).cuda()
        torch.cuda.synchronize()

        def lib_call(what, spp):
            st = abi.Stats()
            (probe_sh_torch if what == "sh" else probe_torch)(gpu, d_points, spp, a.depth, stats=st)
            return st.seconds, st.segments

        def torch_call(spp):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = abi.Stats()
            e0.record()
            out = torch_route(torch, gpu, lambda g, r, s, d: radiance_torch(g, r, s, d, stats=st), d_points, spp, a.depth, gen)
            e1.record()
            torch.cuda.synchronize()
            del out
            return e0.elapsed_time(e1) * 1e-3, st.segments

        yard = "rtw_probe_device irradiance, normal +y"
        routes = [(yard, lambda spp: lib_call("irradiance", spp)),
                  ("rtw_probe_sh_device", lambda spp: lib_call("sh", spp)),
                  ("torch rays + rtw_radiance_device spp 1", torch_call)]
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
        if scene == 0:  # the order-2 truncation: 4 x 4 x 4 points well inside the box, normal +y
            chk = bake.probe_grid((100.0, 100.0, 100.0), (455.0, 455.0, 455.0), 4, 4, 4)
            chk[:, 4] = 1.0
            sh = bake.sh_irradiance(gpu.probe_sh(chk, a.check_spp, a.depth)[:, :, :3], np.array([0, 1, 0], np.float32))
            irr = gpu.probe(chk, a.check_spp, a.depth, key_offset=1 << 20)[:, :3].astype(np.float64)
            lit = irr.sum(1) > 1e-3 * irr.sum(1).max()  # (a point inside one of the boxes sees nothing)
            rel = np.abs(sh[lit] - irr[lit]).sum(1) / irr[lit].sum(1)
            tail = ["#", f"# Band-2 truncation, scene 0: bake.sh_irradiance(rtw_probe_sh) at +y against rtw_probe irradiance at the same point and normal,",
                    f"# {int(lit.sum())} lit points of a 4 x 4 x 4 grid in [100, 455]^3, {a.check_spp} spp each (independent keys), depth {a.depth}, relative difference summed over rgb:",
                    f"#   median {np.median(rel):.4f}   mean {rel.mean():.4f}   max {rel.max():.4f}   min {rel.min():.4f}"]
            print("\n".join(tail), flush=True)
        del d_points
    gpu.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines + tail) + "\n")


if __name__ == "__main__":
    main()
