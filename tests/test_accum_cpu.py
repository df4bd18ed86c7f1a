"""Accumulation sessions without a GPU: the host arithmetic of csrc/rtw_accum_state.h - the splitter of an add, the saved session's
header and its refusals, the scene fingerprint - checked by tests/native/accum_check.cpp, a stand-alone program built with the
address and undefined-behaviour sanitizers and run directly."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("accum") / "accum_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "accum_check.cpp")])
    return exe


def test_native_accum_state_check(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "accum_check ok", r.stdout + r.stderr


def test_fingerprint_matches_a_python_fnv1a():
    """The fingerprint the native check pins for "a" and "foobar", recomputed here step by step (FNV-1a, 64 bit)."""
    def fnv(b):
        h = 0xcbf29ce484222325
        for c in b:
            h = ((h ^ c) * 0x100000001b3) % 2 ** 64
        return h
    assert fnv(b"") == 0xcbf29ce484222325
    assert fnv(b"a") == 0xaf63dc4c8601ec8c
    assert fnv(b"foobar") == 0x85944171f73967e8


def _one_shot(S):
    """rtw_render's order over block sums S[b] (include/rtw.h): blocks in order inside aligned units of 8, units in order; what
    k_resolve_blocks computes from block slots and, for whole units, k_path itself (0 + S_0 + S_1 ...)."""
    a = np.zeros(S.shape[1:], np.float32)
    for u0 in range(0, len(S), 8):
        u = np.zeros_like(a)
        for b in range(u0, min(u0 + 8, len(S))):
            u = u + S[b]
        a = a + u
    return a


def _session(S, schedule, split):
    """The session's order (csrc/rtw_accum.h): per piece of every add, unit slots go to accum, block slots to the open unit, which is
    closed when its eighth block arrives; the read adds the open unit to a copy."""
    a = np.zeros(S.shape[1:], np.float32)
    u = np.zeros_like(a)
    done = 0
    for n in schedule:
        for n_from, n_to, unit_sums, _, _ in split(done, done + n):
            b0, b1 = n_from // 16, n_to // 16
            if unit_sums:
                assert b0 % 8 == 0 and b1 % 8 == 0 and not u.any()
                for u0 in range(b0, b1, 8):
                    slot = np.zeros_like(a)  # k_path: prev = 0, then + every block of the unit
                    for b in range(u0, u0 + 8):
                        slot = slot + S[b]
                    a = a + slot
            else:
                for b in range(b0, b1):
                    u = u + S[b]
                    if (b + 1) % 8 == 0:
                        a = a + u
                        u = np.zeros_like(a)
        done += n
    return a + u


@pytest.mark.parametrize("every_block", [0, 1])
def test_session_summation_order_equals_the_one_shot_order(checker, every_block):
    """fp32 emulation of both orders over random block sums (wide dynamic range, so that a changed order changes bits): every
    schedule gives the one-shot bits, with the native splitter deciding where unit sums are allowed."""
    rng = np.random.default_rng(5)
    S = (rng.standard_normal((32, 4096)) * np.exp(rng.uniform(-6, 6, (32, 4096)))).astype(np.float32)
    cache = {}

    def split(n_from, n_to):
        if (n_from, n_to) not in cache:
            out = subprocess.run([checker, "split", str(n_from), str(n_to), str(every_block)], capture_output=True, text=True, check=True).stdout
            cache[(n_from, n_to)] = [tuple(int(v) for v in line.split()) for line in out.split("\n") if line]
        return cache[(n_from, n_to)]

    schedules = [[512], [16] * 32, [48, 464], [128, 384], [272, 240], [48, 80, 128, 256], [112, 32, 112, 256], [16, 496], [496, 16], [144, 112, 256]]
    for sched in schedules:
        assert sum(sched) == 512
        done = 0
        for k, n in enumerate(sched):
            done += n
            got = _session(S, sched[:k + 1], split)
            ref = _one_shot(S[:done // 16])
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (sched, done)
    # the emulation can tell orders apart: plain ascending order over all blocks differs
    plain = np.zeros(4096, np.float32)
    for b in range(32):
        plain = plain + S[b]
    assert not np.array_equal(plain.view(np.uint32), _one_shot(S).view(np.uint32))
