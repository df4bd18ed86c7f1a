"""Rates of rtw_probe_adaptive_device beside rtw_probe_device (profiles/probe_adaptive_rates.txt).

  python scripts/probe_adaptive_rates.py [--calls 10] [--depth 50] [--side 512] [--scenes 0 3] [--out profiles/probe_adaptive_rates.txt]
      Probes: a side x side bake of the floor of scenes 0 and 3 (bake.rect_probes), Philox, irradiance. Every call is timed by its own
      stats.seconds; the median, minimum and maximum of --calls calls after two warm-up calls.
      (a) overhead: rtw_probe_adaptive_device at threshold 0 (every probe runs to the cap) against rtw_probe_device at spp = cap, in
          the same process, caps 256 and 1024, min_spp 64 (the default schedule); and the fixed cost of a checkpoint from a 64-probe
          call: (adaptive - uniform) / checkpoints.
      (b) thresholds 0.01, 0.02, 0.04 at cap 1024: time, sum n_i / (n * cap), samples/s beside the uniform call's, the histogram of n_i.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
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
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--scenes", type=int, nargs="+", default=[0, 3])
    ap.add_argument("--min-spp", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_adaptive_rates.txt"))
    a = ap.parse_args()
    import torch
    from raytracing_weekend_amd import abi, bake
    from raytracing_weekend_amd.torch_probe import probe_adaptive_torch, probe_torch
    gpu = abi.Renderer(0)
    n = a.side * a.side
    lines = [f"# rtw_probe_adaptive_device beside rtw_probe_device, {n} floor probes ({a.side}x{a.side}), irradiance, depth {a.depth}, Philox, min_spp {a.min_spp},",
             f"# step_spp 0; every call by its own stats.seconds: median (min .. max) of {a.calls} calls after 2 warm-up calls"]
    print("\n".join(lines), flush=True)

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    def timed(fn):
        secs, last = [], None
        for i in range(a.calls + 2):
            st = abi.Stats()
            last = fn(st)
            if i >= 2:
                secs.append(st.seconds)
        return float(np.median(secs)), min(secs), max(secs), st, last

    for scene in a.scenes:
        blob = abi.build_scene(scene, a.side, a.side)
        gpu.upload_scene(blob)
        prims = abi.parse_scene(blob)["prims"]
        floor = next(i for i, p in enumerate(prims) if p.type == abi.PRIM_RECT_Y and p.xform == 0 and p.p[4] == min(
            q.p[4] for q in prims if q.type == abi.PRIM_RECT_Y and q.xform == 0))
        probes = bake.rect_probes(blob, floor, a.side, a.side)
        d_probes = torch.from_numpy(probes).cuda()
        d_few = d_probes[:: max(1, n // 64)][:64].contiguous()
        torch.cuda.synchronize()
        emit(f"# scene {scene}: (a) overhead at threshold 0")
        emit("# probes   cap  checkpoints  uniform_s (min .. max)              adaptive_s (min .. max)             ratio   extra_s    per checkpoint")
        uniform = {}
        for cap in (256, 1024):
            k = len(checkpoints(a.min_spp, cap))
            for d_p in (d_probes, d_few):
                um, ulo, uhi, ust, _ = timed(lambda st: probe_torch(gpu, d_p, cap, a.depth, stats=st))
                am, alo, ahi, ast_, out = timed(lambda st: probe_adaptive_torch(gpu, d_p, cap, a.depth, 0.0, min_spp=a.min_spp, stats=st))
                assert bool((out[1] == cap).all().item()) and (ast_.samples, ast_.segments) == (ust.samples, ust.segments)
                if d_p is d_probes:
                    uniform[cap] = (um, ust.samples)
                emit(f"  {d_p.shape[0]:6d}  {cap:4d}  {k:5d}        {um:.6f} ({ulo:.6f} .. {uhi:.6f})   {am:.6f} ({alo:.6f} .. {ahi:.6f})   {am / um:.3f}   {am - um:.6f}   {(am - um) / k:.6f}")
        emit(f"# scene {scene}: (b) thresholds at cap 1024 (uniform at 1024 spp: {uniform[1024][0]:.6f} s, {uniform[1024][1] / uniform[1024][0] / 1e9:.3f} Gsamples/s)")
        emit("# threshold  adaptive_s (min .. max)             samples / (n * cap)   Gsamples/s   time vs uniform   n_i histogram")
        for thr in (0.01, 0.02, 0.04):
            am, alo, ahi, ast_, out = timed(lambda st: probe_adaptive_torch(gpu, d_probes, 1024, a.depth, thr, min_spp=a.min_spp, stats=st))
            v, c = np.unique(out[1].cpu().numpy(), return_counts=True)
            hist = " ".join(f"{int(x)}:{int(y)}" for x, y in zip(v, c))
            emit(f"  {thr:.2f}       {am:.6f} ({alo:.6f} .. {ahi:.6f})   {ast_.samples / (n * 1024):.4f}                {ast_.samples / am / 1e9:.3f}        {am / uniform[1024][0]:.3f}             {hist}")
        del d_probes, d_few
    gpu.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
