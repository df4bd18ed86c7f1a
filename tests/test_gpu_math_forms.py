"""The short reciprocal / root forms of csrc/rtw_math.h against the compiler's correctly rounded forms on the device, for every
one of the 2^32 inputs (rtw_debug_math, include/rtw.h). Each operation must show 0 differing patterns, and the number of
patterns that took the short form must EQUAL what the range predicate gives in numpy over the same patterns: a sweep that
sent everything to the compiler's form would prove nothing. One launch per operation, each in a child process of its own
under a time limit. The host-model half of the proof is tests/test_math_forms_cpu.py."""
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

from raytracing_weekend_amd import abi

pytestmark = pytest.mark.gpu

LO, HI = np.float32(2.0 ** -64), np.float32(2.0 ** 64)  # rtw_math.h RTW_MATH_LO / RTW_MATH_HI


@functools.lru_cache(maxsize=None)
def window_count(signed):
    """Patterns x with LO <= x <= HI (signed: LO <= |x| <= HI), NaN outside, counted over all 2^32 patterns in numpy."""
    n = 0
    step = 1 << 26
    base = np.arange(step, dtype=np.uint32)
    with np.errstate(invalid="ignore"):
        for lo in range(0, 1 << 32, step):
            x = (base | np.uint32(lo)).view(np.float32)  # (lo is a multiple of step: or = add)
            if signed:
                x = np.abs(x)
            n += int(np.count_nonzero((x >= LO) & (x <= HI)))
    return n


def sweep(op):
    code = ("import json; from raytracing_weekend_amd import abi; r = abi.Renderer(0); "
            f"print('SWEEP ' + json.dumps(r.debug_math({op!r}))); r.close()")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=abi.REPO_DIR)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("SWEEP ")][-1]
    differ, fast, first = json.loads(line[6:])
    print(f"rtw_debug_math {op}: differ={differ} fast={fast} first={'-' if first is None else '%08x' % first}")
    return differ, fast, first


def test_the_window_predicate_in_numpy_counts_what_the_exponents_say():
    # 2^-64 .. 2^64: 128 exponents of 2^23 significands and 2^64 itself, per sign
    assert window_count(False) == 128 * (1 << 23) + 1
    assert window_count(True) == 2 * (128 * (1 << 23) + 1)


# the forms as the renderer takes them, then the header's alternatives by name (one / two reciprocal steps, the root without /
# with the coupled step): DESIGN.md 4.4 states that all of them are exact on this hardware
@pytest.mark.parametrize("op,signed", [("rcp", True), ("sqrt", False), ("rcp_sqrt", False), ("rcp_one_step", True),
                                       ("rcp_two_steps", True), ("sqrt_residual_only", False), ("sqrt_coupled", False)])
def test_short_form_equals_the_compilers_form_for_every_input(op, signed):
    differ, fast, first = sweep(op)
    assert fast == window_count(signed)
    assert differ == 0 and first is None
