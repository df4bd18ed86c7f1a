"""Measurements of the accumulation sessions on the metric frame (scene 0, 1920 x 1080, depth 50, 4096 spp), medians of
--reps runs after a warm-up render in the same process, every variant alternated with rtw_render_device in the same loop:

    one    begin + add(4096) + read_device                      against rtw_render_device(4096)
    c128   begin + 32 adds of 128 (+ read_device after each)    the preview cadence: overhead per add
    c512   begin + 8 adds of 512 (+ read_device after each)
    err    the same single add with RTW_ACCUM_ERROR             against `one` and against rtw_render_adaptive at threshold 0

    render rtw_render_device(4096) alone: with --root DIR the package (and its built library) of another checkout is used, which
           is how the parent commit's own time is taken: the same script, run on the parent's tree, alternated with this one's

    python scripts/accum_sweep.py --out DIR [--parts one,c128,c512,err] [--reps 5] [--spp 4096]
    python scripts/accum_sweep.py --out DIR --parts render --root PARENT_CHECKOUT

Times are device seconds from rtw_stats.seconds (summed over a session's adds) and host wall seconds around the whole sequence."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:  # (before the import: the package of that checkout)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
from raytracing_weekend_amd import abi  # noqa: E402


def session(r, p, adds, d_ptr, error=False, read_each=True):
    """One session: device seconds summed over the adds, k_path seconds, wall seconds of everything from begin to end."""
    t0 = time.perf_counter()
    r.accum_begin(p, error=error)
    dev = kp = 0.0
    for i, n in enumerate(adds):
        st = r.accum_add(n)
        dev += st.seconds
        kp += st.kernel_seconds[4]
        if read_each or i + 1 == len(adds):
            r.accum_read_device(d_ptr)
    if error:
        r.accum_read(error=True)
    r.accum_end()
    return dev, kp, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parts", default="one,c128,c512,err")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=4096)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--root", default=None, help="checkout whose package and library to use (default: this one)")
    a = ap.parse_args()
    import torch
    os.makedirs(a.out, exist_ok=True)
    w, h, spp = a.width, a.height, a.spp
    r = abi.Renderer(0)
    r.upload_scene(abi.build_scene(0, w, h))
    p = abi.make_params(w, h, spp, 50)
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r.render(abi.make_params(w, h, 256, 50))  # warm-up
    variants = {"one": ([spp], False), "c128": ([128] * (spp // 128), False), "c512": ([512] * (spp // 512), False), "err": ([spp], True)}
    out = {}
    if "render" in a.parts.split(","):
        rows = {"render_dev": [], "render_kpath": [], "render_wall": []}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            st = r.render_device(p, frame.data_ptr())
            rows["render_wall"].append(time.perf_counter() - t0)
            rows["render_dev"].append(st.seconds)
            rows["render_kpath"].append(st.kernel_seconds[4])
        out["render"] = {"root": ROOT, "median": {k: float(np.median(v)) for k, v in rows.items()}, "runs": rows}
        print("render", json.dumps({"root": ROOT, "median": out["render"]["median"], "render_dev": rows["render_dev"]}), flush=True)
    for part in [q for q in a.parts.split(",") if q != "render"]:
        adds, error = variants[part]
        rows = {"render_dev": [], "render_kpath": [], "render_wall": [], "sess_dev": [], "sess_kpath": [], "sess_wall": [], "adaptive_dev": []}
        for _ in range(a.reps):  # alternated
            t0 = time.perf_counter()
            st = r.render_device(p, frame.data_ptr())
            rows["render_wall"].append(time.perf_counter() - t0)
            rows["render_dev"].append(st.seconds)
            rows["render_kpath"].append(st.kernel_seconds[4])
            dev, kp, wall = session(r, p, adds, frame.data_ptr(), error=error)
            rows["sess_dev"].append(dev); rows["sess_kpath"].append(kp); rows["sess_wall"].append(wall)
            if error:
                _, _, _, sa = r.render_adaptive(p, 0.0, min_spp=64)
                rows["adaptive_dev"].append(sa.seconds)
        med = {k: float(np.median(v)) for k, v in rows.items() if v}
        res = {"adds": len(adds), "median": med, "runs": rows,
               "sess_over_render_dev": med["sess_dev"] / med["render_dev"], "sess_over_render_wall": med["sess_wall"] / med["render_wall"],
               "dev_overhead_per_add_ms": 1e3 * (med["sess_dev"] - med["render_dev"]) / len(adds),
               "wall_overhead_per_add_ms": 1e3 * (med["sess_wall"] - med["render_wall"]) / len(adds),
               "render_dev_spread": (max(rows["render_dev"]) - min(rows["render_dev"])) / med["render_dev"]}
        if error:
            res["adaptive_over_render_dev"] = med["adaptive_dev"] / med["render_dev"]
        out[part] = res
        print(part, json.dumps({k: v for k, v in res.items() if k != "runs"}), flush=True)
    r.close()
    with open(os.path.join(a.out, "accum_sweep.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
