"""What the float64 checks of shading, lighting and the path loop observe and conclude on the CPU: for every case of
tests/shading_ref.py, tests/lighting_ref.py and tests/path_ref.py, under every (generator, estimator, draw) their CPU tests run, one
line with the CRC-32 of the oracle's samples, the counts the module's oracle_samples returns beside them, and the string its check
returns. It uses only what every such module has had from the start (CASES, case, check, oracle_samples, RNGS, DRAWS), so it runs
on any checkout; two checkouts whose scaffolds observe and check alike print the same bytes:

    python scripts/law_record.py > new.txt
    python scripts/law_record.py --root PARENT_CHECKOUT > parent.txt     (the tests, package and built oracle of that checkout)

With --digest a case's lines are folded into one: the case, the number of its runs and the CRC-32 of the lines above (600 KB become
some 12 KB; the full form says which run differs). No GPU is needed. profiles/law_record.txt keeps one output of --digest."""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:  # (before the imports: the modules of that checkout)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import lighting_ref  # noqa: E402
import path_ref  # noqa: E402
import shading_ref  # noqa: E402

# module -> whether a case's samples depend on the draws (a case without draws runs on the first draw only), as its CPU test has it
MODULES = (
    (shading_ref, lambda name: name.split("-")[0] not in ("emitter", "texture", "texture32")),
    (lighting_ref, lambda name: not isinstance(lighting_ref.case(name), lighting_ref.ExactCase) or bool(lighting_ref.case(name).media)),
    (path_ref, lambda name: True),
)
COUNTS = {0: (), 1: ("shadow_rays",), 2: ("segments", "shadow_rays")}  # by how many counts oracle_samples returns beside the samples


def record(M, drawn, digest):
    for name in M.CASES:
        lines = []
        for est in M.case(name).estimators:
            for rng in M.RNGS:
                for seed, base in M.DRAWS[rng][:2 if drawn(name) else 1]:
                    out = M.oracle_samples(name, rng, est, seed, base)
                    samples, counts = (out[0], out[1:]) if isinstance(out, tuple) else (out, ())
                    kw = dict(zip(COUNTS[len(counts)], counts))
                    crc = zlib.crc32(np.ascontiguousarray(samples, np.float32).tobytes())
                    lines.append(f"{M.__name__} rng{rng} est{est} seed{seed:x} key{base}  samples {samples.shape} crc {crc:08x}"
                                 + "".join(f" {k} {v}" for k, v in kw.items()) + "  | " + M.check(name, samples, est, **kw) + "\n")
        if digest:
            print(f"{M.__name__} {name}: {len(lines)} runs, crc {zlib.crc32(''.join(lines).encode()):08x}", flush=True)
        else:
            print("".join(lines), end="", flush=True)


if __name__ == "__main__":
    for module, drawn_ in MODULES:
        record(module, drawn_, "--digest" in sys.argv)
