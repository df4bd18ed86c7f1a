"""Guide buffers and the guided denoiser, measured (not part of bench.py):
  - RMSE against 1024-spp references of the colour-only and the guided filter on 8-spp renders of scenes 0 and 2 at 256 x 256
    (display-encoded), over a grid of guide sigmas: what abi.DENOISE_SIGMA_ALBEDO / _NORMAL were chosen from
  - rtw_render_guides at 16 spp on 1920 x 1080 scenes 0 and 4 (rtw_stats.seconds: device time of the k_guides launch)
  - rtw_denoise_guided, 5 passes on 1920 x 1080 (wall time of the call, host transfers included)
usage: python scripts/guide_sweep.py [--no-sweep] [--no-timing]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from raytracing_weekend_amd import abi  # noqa: E402
import guides_ref  # noqa: E402


def sweep(r):
    sas, sns = (0.05, 0.1, 0.2, 0.4, 1.0), (0.1, 0.25, 0.5, 1.0)
    tot = {}
    for scene in (0, 2):
        n = 256
        r.upload_scene(abi.build_scene(scene, n, n))
        p = abi.make_params(n, n, 8, 50)
        noisy, _ = r.render(p)
        ref, _ = r.render(abi.make_params(n, n, 1024, 50, seed=0x1234567))
        g = r.render_guides(p, which=("albedo", "normal"))
        enc, ref_enc = guides_ref.encode(noisy), guides_ref.encode(ref)
        rm = lambda a: float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref_enc[..., :3]) ** 2)))  # noqa: E731
        plain = rm(r.denoise(enc, 5, 0.5))
        print(f"scene {scene}: noisy {rm(enc):.5f} colour-only {plain:.5f}")
        for sa in sas:
            row = []
            for sn in sns:
                v = rm(r.denoise_guided(enc, g["albedo"], g["normal"], 5, 0.5, sa, sn))
                tot.setdefault((sa, sn), []).append(v / plain)
                row.append(f"{v:.5f} ({1 - v / plain:+.1%})")
            print(f"  sigma_albedo {sa:<5} " + "  ".join(f"sn {sn}: {x}" for sn, x in zip(sns, row)))
    best = min(tot, key=lambda k: max(tot[k]))
    print(f"best (worst-scene ratio): sigma_albedo {best[0]} sigma_normal {best[1]}: " + ", ".join(f"{1 - x:+.1%}" for x in tot[best]))


def timing(r):
    for scene in (0, 4):
        r.upload_scene(abi.build_scene(scene, 1920, 1080))
        p = abi.make_params(1920, 1080, 16, 50)
        secs = []
        for _ in range(4):
            st = abi.Stats()
            r.render_guides(p, which=("albedo", "normal", "depth"), stats=st)
            secs.append(st.seconds)
        print(f"guides scene {scene} 1920x1080 16 spp: {', '.join(f'{s * 1e3:.2f}' for s in secs)} ms (k_guides device time)")
    rs = np.random.RandomState(0)
    img = rs.uniform(0, 1, (1080, 1920, 4)).astype(np.float32)
    a = rs.uniform(0, 1, img.shape).astype(np.float32)
    nn = rs.uniform(-1, 1, img.shape).astype(np.float32)
    for name, f in (("rtw_denoise", lambda: r.denoise(img, 5, 0.5)), ("rtw_denoise_guided", lambda: r.denoise_guided(img, a, nn, 5, 0.5))):
        ts = []
        for _ in range(4):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        print(f"{name} 5 passes 1920x1080: {', '.join(f'{t * 1e3:.1f}' for t in ts)} ms wall (transfers included)")


if __name__ == "__main__":
    r = abi.Renderer(0)
    if "--no-sweep" not in sys.argv:
        sweep(r)
    if "--no-timing" not in sys.argv:
        timing(r)
    r.close()
