"""Measurements of rtw_render_adaptive: overhead against uniform sampling at threshold 0, image quality per sample
and per second against uniform renders, the pass table of one render, and the quality test's setting (tests/test_gpu_adaptive.py).

    python scripts/adaptive_sweep.py --out DIR [--parts overhead,quality,passes,testcfg,units] [--reps 5]
    python scripts/adaptive_sweep.py --out DIR --parts one     (one threshold-0 render of the metric frame, for a profiler)

Display error = |sqrt(clamp(img, 0, 1)) - sqrt(clamp(ref, 0, 1))| over the three channels; RMSE and the 99th percentile."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raytracing_weekend_amd import abi  # noqa: E402


def disp(img):
    return np.sqrt(np.clip(img[..., :3].astype(np.float64), 0.0, 1.0))


def errors(img, ref):
    d = np.abs(disp(img) - disp(ref))
    return float(np.sqrt(np.mean(d * d))), float(np.quantile(d, 0.99))


def overhead(r, reps, out):
    w, h, cap = 1920, 1080, 4096
    r.upload_scene(abi.build_scene(0, w, h))
    p = abi.make_params(w, h, cap, 50)
    r.render(abi.make_params(w, h, 256, 50))
    p64 = abi.make_params(w, h, 64, 50)
    t_u, t_a, t_64 = [], [], []
    for _ in range(reps):  # alternated
        _, st = r.render(p)
        t_u.append(st.seconds)
        _, spp, _, sa = r.render_adaptive(p, 0.0, min_spp=64)
        assert (spp == cap).all()
        t_a.append(sa.seconds)
        _, s64 = r.render(p64)  # what the first checkpoint's samples cost as a uniform render of their own
        t_64.append(s64.seconds)
    res = {"uniform_s": t_u, "adaptive_s": t_a, "uniform64_s": t_64, "median_uniform": float(np.median(t_u)),
           "median_adaptive": float(np.median(t_a)), "median_uniform64": float(np.median(t_64)), "ratio": float(np.median(t_a) / np.median(t_u))}
    out["overhead"] = res
    print("overhead", json.dumps(res), flush=True)


def quality(r, scenes, out, size=512, ref_spp=16384, thresholds=(0.01, 0.015, 0.02, 0.03, 0.04, 0.06)):
    res = {}
    for sc in scenes:
        r.upload_scene(abi.build_scene(sc, size, size))
        ref, _ = r.render(abi.make_params(size, size, ref_spp, 50, seed=0x5eed))
        rows = []
        for n in (64, 128, 256, 512, 1024, 2048):
            img, st = r.render(abi.make_params(size, size, n, 50))
            rmse, p99 = errors(img, ref)
            rows.append({"kind": "uniform", "spp": n, "mean_spp": n, "seconds": st.seconds, "rmse": rmse, "p99": p99})
        for t in thresholds:
            img, spp, _, st = r.render_adaptive(abi.make_params(size, size, 2048, 50), t, min_spp=64)
            rmse, p99 = errors(img, ref)
            rows.append({"kind": "adaptive", "threshold": t, "mean_spp": float(spp.mean()), "max_spp": int(spp.max()), "seconds": st.seconds,
                         "rmse": rmse, "p99": p99})
        res[str(sc)] = rows
        for row in rows:
            print("quality scene", sc, json.dumps(row), flush=True)
    out["quality"] = res


def passes(out):
    """Pass tables (RTW_VERBOSE=1 prints them) of the metric frame at thresholds 0 and 0.01, each in a child process; a child that
    fails ends the script before anything else opens the GPU."""
    out["passes"] = {}
    for t in (0.0, 0.01):
        code = ("import sys; sys.path.insert(0, %r); from raytracing_weekend_amd import abi; r = abi.Renderer(0); "
                "r.upload_scene(abi.build_scene(0, 1920, 1080)); r.render(abi.make_params(1920, 1080, 256, 50)); "
                "r.render_adaptive(abi.make_params(1920, 1080, 4096, 50), %r, min_spp=64)" % (ROOT, t))
        env = dict(os.environ, RTW_VERBOSE="1")
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            raise SystemExit(f"pass-table child (threshold {t}) exited with {p.returncode}: stopping before any further GPU work")
        lines = [l for l in p.stderr.split("\n") if "adaptive pass" in l]
        out["passes"][str(t)] = lines
        print(f"passes threshold {t}:", flush=True)
        print("\n".join(lines), flush=True)


def one(r):
    """A warm-up render and one threshold-0 adaptive render of the metric frame (for rocprofv3 --kernel-trace --stats)."""
    r.upload_scene(abi.build_scene(0, 1920, 1080))
    r.render(abi.make_params(1920, 1080, 256, 50))
    _, spp, _, st = r.render_adaptive(abi.make_params(1920, 1080, 4096, 50), 0.0, min_spp=64)
    print("one", st.seconds, int(spp.min()), flush=True)


def units(r, out, reps=3):
    """Threshold-0 time of the metric frame under k_path's unit-size knobs (the adaptive passes plan with their own copy of them)."""
    r.upload_scene(abi.build_scene(0, 1920, 1080))
    p = abi.make_params(1920, 1080, 4096, 50)
    r.render(abi.make_params(1920, 1080, 256, 50))
    settings = [{}, {"RTW_PATH_FINE_BLOCKS": "8"}, {"RTW_PATH_FINE_BLOCKS": "4"}, {"RTW_PATH_FINE_BLOCKS": "2"},
                {"RTW_PATH_FINE_BLOCKS": "4", "RTW_PATH_UNIT_BLOCKS": "2"}, {"RTW_PATH_FINE_BLOCKS": "8", "RTW_PATH_UNIT_BLOCKS": "6"}]
    saved = {k: os.environ.get(k) for k in ("RTW_PATH_FINE_BLOCKS", "RTW_PATH_UNIT_BLOCKS")}
    res = {}
    for _ in range(reps):
        for st_ in settings:
            for k in saved:
                os.environ.pop(k, None)
            os.environ.update(st_)
            _, _, _, st = r.render_adaptive(p, 0.0, min_spp=64)
            res.setdefault(json.dumps(st_), []).append(st.seconds)
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    out["units"] = {k: {"seconds": v, "median": float(np.median(v))} for k, v in res.items()}
    for k, v in out["units"].items():
        print("units", k, json.dumps(v), flush=True)


def testcfg(r, out):
    """tests/test_gpu_adaptive.py::test_quality: scene 0 at 256 x 256, min 64, cap 1024, against uniform 256 and an 8192-spp reference."""
    w = h = 256
    r.upload_scene(abi.build_scene(0, w, h))
    ref, _ = r.render(abi.make_params(w, h, 8192, 50, seed=0x5eed))
    u, _ = r.render(abi.make_params(w, h, 256, 50))
    base = errors(u, ref)
    rows = [{"kind": "uniform256", "rmse": base[0], "p99": base[1], "samples": w * h * 256}]
    for dilate in (1, 0):
        for t in (0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.1, 0.12):
            img, spp, _, st = r.render_adaptive(abi.make_params(w, h, 1024, 50), t, min_spp=64, dilate=dilate)
            e = errors(img, ref)
            rows.append({"kind": "adaptive", "dilate": dilate, "threshold": t, "samples": int(spp.astype(np.int64).sum()), "rmse": e[0],
                         "p99": e[1], "p99_gain": 1.0 - e[1] / base[1]})
    out["testcfg"] = rows
    for row in rows:
        print("testcfg", json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parts", default="overhead,quality,passes,testcfg")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", default="0,2,4")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    parts = a.parts.split(",")
    out = {}
    if "passes" in parts:
        passes(out)
    r = abi.Renderer(0)
    if "one" in parts:
        one(r)
    if "units" in parts:
        units(r, out)
    if "testcfg" in parts:
        testcfg(r, out)
    if "overhead" in parts:
        overhead(r, a.reps, out)
    if "quality" in parts:
        quality(r, [int(s) for s in a.scenes.split(",")], out)
    r.close()
    with open(os.path.join(a.out, "adaptive_sweep.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
