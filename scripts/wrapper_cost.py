"""Per-call cost of abi.Renderer's query-family methods on the CPU, against a library that records nothing and returns 0, so that no
GPU time is mixed in: for every method the minimum and the spread (maximum - minimum) of five timeit batches, in microseconds per
call, on the smallest inputs (3 rays or probes, 2 views of 3 x 2, one guide name).

    python scripts/wrapper_cost.py                             this tree alone
    python scripts/wrapper_cost.py --against PARENT_CHECKOUT   that checkout's abi.py beside this tree's, their batches taken in turn
                                                               (so that a drift of the machine meets both alike)

A method of this tree is no slower than the parent's when its minimum is at most the parent's minimum plus the parent's spread."""
import ctypes as C
import importlib.util
import os
import sys
import timeit

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NUMBER, REPEAT = 2000, 5


class Null:
    def __getattr__(self, name):
        def f(*args):
            return 0
        setattr(self, name, f)
        return f


def load_abi(root, name):
    """abi.py of the checkout at `root` as a module of its own (it imports nothing else of its package)"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "raytracing_weekend_amd", "abi.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def calls(abi):
    r = object.__new__(abi.Renderer)
    r.lib, r.ctx, r.devices = Null(), C.c_void_p(1), [0]
    batch, times = np.zeros((3, 8), np.float32), np.zeros(3, np.float32)
    views = abi.view_array([abi.make_view(np.zeros(24, np.float32)), abi.make_view(np.ones(24, np.float32))])
    frames = np.zeros((2, 2, 3, 4), np.float32)
    p, st = abi.make_params(3, 2, 4, 5), abi.Stats()
    return r, (
        ("cast", lambda: r.cast(batch, times, times, stats=st)),
        ("cast_device", lambda: r.cast_device(3, 16, {"t": 32, "prim": 48}, stats=st)),
        ("radiance", lambda: r.radiance(batch, 4, 5, stats=st)),
        ("radiance_device", lambda: r.radiance_device(3, 16, 32, 4, 5, stats=st)),
        ("probe", lambda: r.probe(batch, 4, 5, stats=st)),
        ("probe_device", lambda: r.probe_device(3, 16, 32, 4, 5, stats=st)),
        ("probe_adaptive", lambda: r.probe_adaptive(batch, 64, 5, 0.05, stats=st)),
        ("probe_adaptive_device", lambda: r.probe_adaptive_device(3, 16, 32, 48, 64, 64, 5, 0.05, stats=st)),
        ("probe_sh", lambda: r.probe_sh(batch, 4, 5, stats=st)),
        ("probe_sh_device", lambda: r.probe_sh_device(3, 16, 32, 4, 5, stats=st)),
        ("views", lambda: r.views(views, 3, 2, 4, 5, stats=st)),
        ("views_device", lambda: r.views_device(2, 16, 32, 3, 2, 4, 5, stats=st)),
        ("views_adaptive", lambda: r.views_adaptive(views, 3, 2, 64, 5, 0.05, stats=st)),
        ("views_adaptive_device", lambda: r.views_adaptive_device(2, 16, 32, 48, 64, 3, 2, 64, 5, 0.05, stats=st)),
        ("views_guides", lambda: r.views_guides(views, 3, 2, which=("depth",), stats=st)),
        ("views_guides_device", lambda: r.views_guides_device(2, 16, {"depth": 32}, 3, 2, stats=st)),
        ("denoise_views", lambda: r.denoise_views(frames, frames, frames)),
        ("denoise_views_device", lambda: r.denoise_views_device(2, 16, 32, 48, 64, 3, 2)),
        ("render_guides", lambda: r.render_guides(p, ("depth",), stats=st)),
        ("render_adaptive", lambda: r.render_adaptive(p, 0.05)),
        ("denoise_guided", lambda: r.denoise_guided(frames[0], frames[0], frames[0])),
        ("debug_intersect", lambda: r.debug_intersect(batch, times, times)),
    )


def batch(call):
    return 1e6 * timeit.timeit(call, number=NUMBER) / NUMBER


if __name__ == "__main__":
    trees = [calls(load_abi(ROOT, "abi_here"))]
    if "--against" in sys.argv:
        trees.insert(0, calls(load_abi(os.path.abspath(sys.argv[sys.argv.index("--against") + 1]), "abi_parent")))
    for rows in zip(*(table for _, table in trees)):
        for _, call in rows:
            call()
        t = [[] for _ in rows]
        for _ in range(REPEAT):
            for k, (_, call) in enumerate(rows):
                t[k].append(batch(call))
        line = "  ".join(f"min {min(v):6.2f} us spread {max(v) - min(v):5.2f} us" for v in t)
        verdict = "" if len(t) == 1 else ("  ok" if min(t[1]) <= min(t[0]) + max(t[0]) - min(t[0]) else "  over")
        print(f"{rows[0][0]:24s} {line}{verdict}", flush=True)
    for r, _ in trees:
        r.ctx = C.c_void_p()  # so that close() calls nothing
