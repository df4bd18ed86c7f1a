"""What every renderer launches, as rtw_stats counts it, over a fixed small matrix: scene 0 (k_path) and scene 1 (a tree: the wavefront
kernels) at 64 x 64, depth 8; rtw_render at 16 / 144 / 512 spp, rtw_render_adaptive with the default checkpoints to 256, accumulation
sessions adding [256] and [48, 80, 128]; each call plain, under RTW_PATH_UNIT_BLOCKS=8 RTW_PATH_FINE_BLOCKS=2 and under
RTW_BLOCKSUM_BYTES=65536. One line per call: bounce_launches, kernel_launches[*], kernel_segments[*], samples, segments, shadow_rays.
Two checkouts that issue the same launches print the same bytes:

    python scripts/launch_record.py > new.txt
    python scripts/launch_record.py --root PARENT_CHECKOUT > parent.txt     (the package and built library of that checkout)

profiles/share_schedules_launches.txt keeps one output."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:  # (before the import: the package of that checkout)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
from raytracing_weekend_amd import abi  # noqa: E402

W = H = 64
DEPTH = 8
KNOBS = {"plain": {}, "units": {"RTW_PATH_UNIT_BLOCKS": "8", "RTW_PATH_FINE_BLOCKS": "2"}, "blocksum": {"RTW_BLOCKSUM_BYTES": "65536"}}


def line(tag, st):
    print(f"{tag:44s} launches {st.bounce_launches:4d}  kernel_launches {list(st.kernel_launches)}  kernel_segments {list(st.kernel_segments)}  "
          f"samples {st.samples} segments {st.segments} shadow_rays {st.shadow_rays}", flush=True)


def main():
    r = abi.Renderer(0)
    for scene in (0, 1):
        r.upload_scene(abi.build_scene(scene, W, H))
        for knob, env in KNOBS.items():
            for k in ("RTW_PATH_UNIT_BLOCKS", "RTW_PATH_FINE_BLOCKS", "RTW_BLOCKSUM_BYTES"):
                os.environ.pop(k, None)
            os.environ.update(env)
            for spp in (16, 144, 512):
                line(f"scene{scene} {knob} render {spp}", r.render(abi.make_params(W, H, spp, DEPTH))[1])
            line(f"scene{scene} {knob} adaptive 256", r.render_adaptive(abi.make_params(W, H, 256, DEPTH), 0.05)[3])
            for adds in ([256], [48, 80, 128]):
                r.accum_begin(abi.make_params(W, H, 256, DEPTH))
                for i, n in enumerate(adds):
                    line(f"scene{scene} {knob} accum {adds} add {i}", r.accum_add(n))
                r.accum_end()
    r.close()


if __name__ == "__main__":
    main()
