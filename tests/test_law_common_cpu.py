"""The one copy of the scaffold the float64 checks share (tests/law_common.py and its GPU half in tests/gpu_common.py), on the
cheapest case of each family and without a GPU: check_both is given the oracle's samples as if they were the kernels'."""
import numpy as np
import pytest

import law_common as C
import lighting_ref as L
import path_ref as P
import shading_ref as S
from gpu_common import check_both

RUN = (C.RNGS[0], C.CORR, C.SEEDS[0], 0)  # Philox, the corrected estimator, the first draw
SMALL = [(S, "emitter-light"), (L, "point00-d1"), (P, "corridor-k2-d2")]
ids = [name for _, name in SMALL]


def oracle(module, name):
    return C.oracle_samples(module.case(name), *RUN)


def test_runs_reproduce_the_ids_written_out_by_hand():
    """One case of each module: a case without draws has the first draw only, the upload column is there when asked for, and the
    second draw of TEA+LCG lies on other keys."""
    def listed(*a, **kw):
        return [(p.id, p.values) for p in C.runs(*a, **kw)]
    assert listed(S, ["emitter-light"]) == [
        (f"emitter-light-rng{r}-est{e}-seed6314759-key0", ("emitter-light", r, e, 0x6314759, 0)) for e in (0, 1) for r in (0, 1)]
    assert [i for i, _ in listed(L, ["point00-d1"], ["as_uploaded", "no_lds"], slice(0, 1))] == [
        "point00-d1-as_uploaded-rng0-est0-seed6314759-key0", "point00-d1-as_uploaded-rng1-est0-seed6314759-key0",
        "point00-d1-no_lds-rng0-est0-seed6314759-key0", "point00-d1-no_lds-rng1-est0-seed6314759-key0",
        "point00-d1-as_uploaded-rng0-est1-seed6314759-key0", "point00-d1-as_uploaded-rng1-est1-seed6314759-key0",
        "point00-d1-no_lds-rng0-est1-seed6314759-key0", "point00-d1-no_lds-rng1-est1-seed6314759-key0"]
    assert listed(L, ["point00-d1"], ["as_uploaded"], slice(1, 2)) == []  # a deterministic case has no second draw
    assert [i for i, _ in listed(P, ["corridor-k2-d2"])] == [
        f"corridor-k2-d2-rng{r}-est{e}-seed{s}-key{k}" for e in (0, 1)
        for r, s, k in ((0, "6314759", 0), (0, "badc0de", 0), (1, "6314759", 0), (1, "6314759", 1048576))]
    assert listed(P, ["corridor-k2-d2"], ["forced_tree"], slice(1, 2))[-1] == (
        "corridor-k2-d2-forced_tree-rng1-est1-seed6314759-key1048576", ("corridor-k2-d2", "forced_tree", 1, 1, 0x6314759, 1 << 20))
    assert len(C.runs(S)) + len(C.runs(L)) + len(C.runs(P)) == 1232  # every run of the three CPU tests (profiles/law_record.txt)


@pytest.mark.parametrize("module,name", SMALL, ids=ids)
def test_check_both_passes_on_the_oracles_own_triple(module, name):
    check_both(module, name, oracle(module, name), RUN, module.COUNTS)


@pytest.mark.parametrize("module,name", SMALL, ids=ids)
def test_check_both_raises_on_one_flipped_mantissa_bit(module, name):
    """The lowest mantissa bit of the first sample's red. The point light's tolerance has room for it, so there the comparison of
    bits with the oracle speaks; the emitter's law is equality and the corridor's black sample becomes a value its law does not
    know, so there the float64 check speaks first."""
    got = oracle(module, name)
    bits = got.samples.copy().view(np.uint32)
    bits[0, 0, 0] ^= 1
    with pytest.raises(AssertionError) as e:
        check_both(module, name, got._replace(samples=bits.view(np.float32)), RUN, module.COUNTS)
    print(e.value)
    assert module is not L or "1 samples differ from the oracle's" in str(e.value)


@pytest.mark.parametrize("count", ["segments", "shadow_rays"])
@pytest.mark.parametrize("module,name", SMALL, ids=ids)
def test_check_both_raises_on_a_compared_count_off_by_one_only(module, name, count):
    got = oracle(module, name)
    off = got._replace(**{count: getattr(got, count) + 1})
    if count in module.COUNTS:
        with pytest.raises(AssertionError):
            check_both(module, name, off, RUN, module.COUNTS)
    else:  # shading compares no count, lighting not the segments
        check_both(module, name, off, RUN, module.COUNTS)


def test_oracle_samples_are_computed_once_and_read_only():
    got = oracle(P, "corridor-k2-d2")
    assert got is oracle(P, "corridor-k2-d2") and not got.samples.flags.writeable
    assert P.oracle_samples("corridor-k2-d2", *RUN) == tuple(got) and P.oracle_samples("corridor-k2-d2", *RUN)[0] is got.samples
    assert L.oracle_samples("point00-d1", *RUN) == (oracle(L, "point00-d1").samples, oracle(L, "point00-d1").shadow_rays)
    assert S.oracle_samples("emitter-light", *RUN) is oracle(S, "emitter-light").samples


def test_measured_band_is_0_9_to_1_0005_of_the_recorded_value():
    for recorded in (0.2579, 3.58e-7):
        C.measured_band(0.9 * recorded, recorded, "lower end")
        C.measured_band(1.0005 * recorded, recorded, "upper end")
        for factor in (0.89, 1.001):
            with pytest.raises(AssertionError, match="MEASURED_X: measured"):
                C.measured_band(factor * recorded, recorded, "MEASURED_X")
