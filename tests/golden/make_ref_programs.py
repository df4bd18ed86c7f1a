"""Generates tests/golden/ref_programs/*.npz from the REFERENCE's own device programs, compiled where they lie by oracle/Makefile
(target `ref`) into oracle/_ref/libref_programs.so and libref_programs_fma.so (oracle/ref_programs_wrap.cpp). Run where the
reference tree is (it does not travel); the files it writes are the committed fixtures: inputs and recorded outputs only.
Prints the measured constant and the per-case shares that tests/ref_programs.py records.

    make -C oracle ref && python tests/golden/make_ref_programs.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ref_programs as RP  # noqa: E402


def main():
    constant = 0.0
    os.makedirs(os.path.dirname(RP.fixture_path("a", "x")), exist_ok=True)
    for name in RP.LEVEL_A:
        out = RP.record_level_a(name)
        np.savez_compressed(RP.fixture_path("a", name), **out)
        print(f"level A {name}: {len(out['rays'])} rays, {int((out['prim_plain'] >= 0).sum())} hits, "
              f"{int((out['prim_plain'] != out['prim_fma']).sum())} rays on which the builds pick another primitive")
    np.savez_compressed(RP.fixture_path("a", "textures"), **RP.record_textures())
    print(f"level A textures: {RP.TEXTURES}, {os.path.getsize(RP.fixture_path('a', 'textures'))} bytes")
    for module, names in RP.LAW_CASES.items():
        for name in names:
            out = RP.record_law(module, name)
            np.savez_compressed(RP.fixture_path("a", f"{module}_{name}"), **out)
            m = RP.law_module(module)
            o = RP.law_common.Observed(out["samples_plain"], int(out["counts_plain"][0]), int(out["counts_plain"][1]))
            print(f"level A {module} " + m.check(name, o.samples, RP.law_common.REF, **RP.law_common.counts_of(m, o))
                  + f"; {os.path.getsize(RP.fixture_path('a', f'{module}_{name}'))} bytes")
    out = RP.record_camera_lens()
    np.savez_compressed(RP.fixture_path("a", "camera_lens"), **out)
    print("level A camera_lens: " + RP.check_camera("camera_lens", out["blob"].tobytes(), out["camera_origin_plain"], out["camera_direction_plain"]))
    for name in RP.LEVEL_B:
        out = RP.record_level_b(name)
        np.savez_compressed(RP.fixture_path("b", name), **out)
        differ, c = RP.builds_disagree(out)
        constant = max(constant, c)
        frame, st = RP.oracle_frame(out["blob"].tobytes())
        rel = RP.relative(frame, out["frame_plain"]).max(-1)
        ok = "" if differ.mean() <= RP.BUILDS_CAP else "  <-- the builds disagree on too many samples: replace the case"
        print(f'level B {name}: constant {c:.4e}; builds disagree on {100 * differ.mean():.3f} %, oracle outside the tolerance on '
              f'{100 * (rel > RP.TOLERANCE).mean():.3f} % (SHARES: "{name}": ({differ.mean():.6f}, {(rel > RP.TOLERANCE).mean():.6f})); traversals '
              f'{int(out["counts_plain"][..., 0].sum())} / segments {st.segments}, shadow {int(out["counts_plain"][..., 1].sum())} / {st.shadow_rays}; '
              f'{os.path.getsize(RP.fixture_path("b", name))} bytes{ok}')
    print(f"MEASURED_CONSTANT_SAMPLE = {constant:.4e} (recorded: {RP.MEASURED_CONSTANT_SAMPLE})")


if __name__ == "__main__":
    main()
