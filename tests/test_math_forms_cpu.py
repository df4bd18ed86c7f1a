"""The short reciprocal / root forms of csrc/rtw_math.h on a host model (tests/native/math_forms_check.cpp, compiled with g++ and
-ffp-contract=off): the hardware approximations are modelled as the correctly rounded 1/x and 1/sqrt(x) displaced by k ulp.
For every significand at the window's lowest and highest exponents, just outside them and in the middle, and for every exponent
at sampled significands, the short form is compared with 1.0f / x, sqrtf(x), 1.0f / sqrtf(x) bit for bit wherever the range test
says "fast".

The header ships the shortest forms the hardware sweep proves: ONE Newton step on v_rcp_f32, the residual step alone on
v_rsq_f32. It also holds the longer forms (-DRTW_RCP_STEPS=2, -DRTW_SQRT_COUPLED=1), which need less of the hardware. What the
model shows, and where it ends:
* from the correctly rounded start (k = 0) every form, shipped or longer, is exact: asserted;
* the root with the coupled step is exact from every start within 2 ulp (k = -2 .. 2): asserted;
* the reciprocal with TWO steps is exact from a neighbouring start (k = -1, 1) everywhere except the all-ones significand
  0x7fffff, where 1/x lies 2^-24 ulp above a tie and the step from the wrong neighbour lands on the tie: asserted (every miss is
  such an input). No Newton form passes k = -1, 1 there, so a model with displaced starts cannot prove a reciprocal;
* the shipped forms from a displaced start miss a few hundred inputs (reciprocal) or a few dozen (root): printed, not asserted.
  Whether the short forms are enough hangs on what v_rcp_f32 and v_rsq_f32 return, input by input, and only the hardware can
  say: tests/test_gpu_math_forms.py runs all 2^32 inputs on the device and is the proof (0 differing on gfx950). This file is
  the reasoning behind it and guards the header's text (window, sequences) on machines without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = 1 << 23  # significands of one exponent
OPS = ("rcp", "sqrt", "rcp_sqrt", "rcp3")


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{(form, op, k): {"tried": n, "fast": n, "differ": n, "ones": n, "first": hex}}; form 0: the header as shipped, 2: the longer
    forms (two reciprocal steps, coupled root step)."""
    d = tmp_path_factory.mktemp("math_forms")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    if " fma " in open("/proc/cpuinfo").read():
        cmd.append("-mfma")  # fmaf as one instruction (same result as the library's, much faster)
    procs = {}
    for steps in (0, 2):
        exe = str(d / f"math_forms_check{steps}")
        subprocess.check_call(cmd + (["-DRTW_RCP_STEPS=2", "-DRTW_SQRT_COUPLED=1"] if steps else []) +
                              ["-o", exe, os.path.join(ROOT, "tests", "native", "math_forms_check.cpp")])
        for op in OPS:
            for k in (-2, -1, 0, 1, 2):
                procs[(steps, op, k)] = subprocess.Popen([exe, op, str(k)], stdout=subprocess.PIPE, text=True)
    out = {}
    for (steps, op, k), p in procs.items():
        line = p.communicate(timeout=900)[0].strip()
        assert p.returncode == 0, (steps, op, k)
        print("as shipped: " if not steps else "longer forms:", line)
        w = line.split()
        assert w[0] == op and int(w[1]) == k, line
        out[(steps, op, k)] = {w[i]: (w[i + 1] if w[i] == "first" else int(w[i + 1])) for i in range(2, len(w), 2)}
    return out


@pytest.mark.parametrize("k", [-2, -1, 0, 1, 2])
def test_root_with_the_coupled_step_is_exact_from_any_start_within_two_ulp(results, k):
    r = results[(2, "sqrt", k)]
    assert r["differ"] == 0, r
    assert r["fast"] > 7 * FULL  # seven of the nine fully swept exponents are inside the window: the fast path was exercised


@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("op", OPS)
def test_every_form_is_exact_from_the_correctly_rounded_start(results, op, form):
    r = results[(form, op, 0)]
    assert r["differ"] == 0, r
    assert r["fast"] > 7 * FULL


@pytest.mark.parametrize("op", ["rcp", "rcp3", "rcp_sqrt"])
@pytest.mark.parametrize("k", [-1, 1])
def test_two_steps_from_a_neighbouring_start_miss_only_the_all_ones_significand(results, op, k):
    r = results[(2, op, k)]
    assert r["differ"] == r["ones"], r
    assert 0 < r["ones"] < 1000 and r["fast"] > 7 * FULL


def test_window_admits_exactly_the_exponents_it_names(results):
    # rcp, both signs: exponents 63 .. 190 in full and 2^64 itself. Of the 9 fully swept exponents 62 and 191 (but for its
    # significand 0) are outside; of the 256 sampled ones 128 are inside, and 191's sample with significand 0.
    assert results[(0, "rcp", 0)]["fast"] == 2 * (7 * FULL + 1) + 2 * (128 * 4096 + 1)
    # sqrt, positive only, each input twice (with the range test and as sqrt_inside)
    assert results[(0, "sqrt", 0)]["fast"] == 2 * ((7 * FULL + 1) + (128 * 4096 + 1))
