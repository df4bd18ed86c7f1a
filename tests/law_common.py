"""What the float64 checks built on one Case share (shading_ref.py, lighting_ref.py, path_ref.py, their CPU tests and, through
gpu_common.py, their GPU tests): the limits and draws, the Case itself and how it is observed through the oracle, the registry that
turns a dict of case factories into case(name) and check(name, ...), the parameter lists of the tests, the band of a measured
constant and the negative-control helper. A plain module (not a conftest), imported by name. Like the reference modules it shares
nothing with the oracle at import time: the oracle library is loaded inside oracle_samples."""
import collections
import functools

import numpy as np
import pytest

import radiance_ref as R
from raytracing_weekend_amd import abi

U = 2.0 ** -24
K_FACTOR = 4.0        # geometry_ref.py's: the oracle and the kernels fuse multiply-adds and order operations otherwise than numpy
KS_LIMIT = 2.23       # Kolmogorov: P(D sqrt(n) > 2.23) = 2 exp(-2 * 2.23^2) = 0.96e-4
Z_LIMIT = 3.89        # normal, two-sided: P(|z| > 3.89) = 1.0e-4
SEEDS = (0x6314759, 0x0BADC0DE)  # the project's default seed and one more; both fixed
KEY_SHIFT = 1 << 20              # TEA+LCG takes no seed (include/rtw.h rtw_rng_kind): its second sample comes from other stream keys
SIDE = 128
N_STAT = SIDE * SIDE  # samples of a statistical case: 128 x 128 keys, one sample each
REF, CORR, NO_NEE, MIX = abi.RTW_EST_REFERENCE, abi.RTW_EST_CORRECTED, abi.RTW_EST_CORRECTED_NO_NEE, abi.RTW_EST_MIXTURE
RNGS = (abi.RTW_RNG_PHILOX, abi.RTW_RNG_TEA_LCG)
# generator -> the (seed, key base) of its two independent samples
DRAWS = {abi.RTW_RNG_PHILOX: ((SEEDS[0], 0), (SEEDS[1], 0)), abi.RTW_RNG_TEA_LCG: ((SEEDS[0], 0), (SEEDS[0], KEY_SHIFT))}
PI32 = np.float32(3.14159265)  # the library's pi (rtw_probe: irradiance = pi * radiance)


# ---------------------------------------------------------------- small algebra, at the precision of its arguments
def _dot(a, b):
    return (a * b).sum(-1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


# ---------------------------------------------------------------- a case and how it is observed
class Case:
    """m rays (o, d), each traced on keys_per_ray consecutive stream keys with one sample per key: ray j owns the keys
    j * keys_per_ray ...; a sample array has the shape (m, keys_per_ray, 3). drawn: whether the samples depend on the draws."""
    depth = 2
    estimators = (REF, CORR)
    drawn = True

    def __init__(self, blob, o, d, keys_per_ray):
        self.blob, self.keys_per_ray = blob, keys_per_ray
        self.o = np.atleast_2d(np.asarray(o, np.float32))
        self.ll = (self.o + np.atleast_2d(np.asarray(d, np.float32))).astype(np.float32)
        self.d = ((np.float32(0) + self.ll) - self.o).astype(np.float64)  # the bits the camera ray carries
        assert np.array_equal(self.d, np.atleast_2d(np.asarray(d, np.float64))), "the direction is not exact in float32"
        self.m = len(self.o)

    def rays(self, estimator):
        """(m * keys_per_ray, 8) float32 for rtw_radiance: ray j repeated keys_per_ray times, tmin = the estimator's start distance."""
        return np.repeat(R.make_rays(self.o, self.ll, estimator), self.keys_per_ray, axis=0)

    def tmin(self, estimator):
        return float(np.float32(1e-6 if estimator == REF else 1e-3))


def render_params(c, j, rng_kind, estimator, seed, key_base=0):
    """The rtw_params under which a render of radiance_ref.ray_blob(c.blob, c.o[j], c.ll[j]) gives ray j's samples on ray j's keys,
    key_base + j * keys_per_ray ...: min(keys_per_ray, 128) pixels wide, the rows from key_base / width + j * rows - a render's
    stream key is width * y + x."""
    w = min(c.keys_per_ray, SIDE)
    rows = c.keys_per_ray // w
    assert key_base % w == 0
    r0 = key_base // w + j * rows
    return abi.make_params(w, r0 + rows, 1, c.depth, seed=seed, row0=r0, row1=r0 + rows, rng_kind=rng_kind, estimator=estimator)


# what one run of a case gives, whoever traced it: the samples (m, keys_per_ray, 3) float32 and the two counts over all its rays
Observed = collections.namedtuple("Observed", "samples segments shadow_rays")


def observe(render, c, rng_kind, estimator, seed, key_base):
    """The case as `render(blob, params) -> (image, stats)` sees it: every ray through its own blob (radiance_ref.ray_blob: each
    pixel the same ray on its own key), the counts summed."""
    samples, segments, shadow_rays = np.empty((c.m, c.keys_per_ray, 3), np.float32), 0, 0
    for j in range(c.m):
        img, st = render(R.ray_blob(c.blob, c.o[j], c.ll[j]), render_params(c, j, rng_kind, estimator, seed, key_base))
        samples[j] = img[..., :3].reshape(c.keys_per_ray, 3)
        segments, shadow_rays = segments + int(st.segments), shadow_rays + int(st.shadow_rays)
    return Observed(samples, segments, shadow_rays)


@functools.lru_cache(maxsize=None)
def oracle_samples(c, rng_kind, estimator, seed, key_base):
    """The oracle's Observed of case c, computed once and left unchanged (the oracle's results do not depend on its threads)."""
    import oracle
    out = observe(functools.partial(oracle.render, threads=4), c, rng_kind, estimator, seed, key_base)
    out.samples.setflags(write=False)
    return out


def counts_of(module, observed):
    """The counts module.check takes beside the samples, as keywords: module.COUNTS names them."""
    return {k: getattr(observed, k) for k in module.COUNTS}


# ---------------------------------------------------------------- a module's cases
def registry(cases, prefix):
    """(case, check) of a dict {name: case factory}: case(name) builds a case once; check(name, samples, estimator, **kw) runs the
    case's assertions on a sample array (m, keys_per_ray, 3) and returns the figures, behind `prefix` (a format of name and est),
    for the caller to print."""
    @functools.lru_cache(maxsize=None)
    def case(name):
        return cases[name]()

    def check(name, samples, estimator, **kw):
        return prefix.format(name=name, est=estimator) + case(name).check(np.asarray(samples), estimator, **kw)
    return case, check


def runs(module, names=None, hows=None, draws=slice(0, 2)):
    """The parameter list (case[, upload], generator, estimator, seed, key base) of the named cases of `module` (all of them by
    default) under the estimators each is defined for, every upload of `hows` (none: the list has no such column), both generators
    and the generator's independent samples DRAWS[rng][draws]: a second seed for Philox, other keys for TEA+LCG. A case whose
    samples do not depend on the draws has the first draw only."""
    out = []
    for name in module.CASES if names is None else names:
        c = module.case(name)
        for est in c.estimators:
            out += [pytest.param(*head, rng, est, seed, base, id="-".join(head + (f"rng{rng}", f"est{est}", f"seed{seed:x}", f"key{base}")))
                    for head in ([(name, how) for how in hows] if hows else [(name,)]) for rng in RNGS
                    for seed, base in DRAWS[rng][draws] if c.drawn or (seed, base) == DRAWS[rng][0]]
    return out


# ---------------------------------------------------------------- what the CPU tests of every float64 check assert alike
def measured_band(measured, recorded, what):
    """A MEASURED_* value re-measured: no more than a rounding above the recorded one, and no more than a tenth below it."""
    assert 0.9 * recorded <= measured <= 1.0005 * recorded, f"{what}: measured {measured:.6g}, recorded {recorded}"


def rejected(module, name, est, rng=abi.RTW_RNG_PHILOX, observed=None, **wrong):
    """A negative control: on the oracle's first draw (or on `observed`) the right model passes and the model with `wrong` raises."""
    observed = observed or oracle_samples(module.case(name), rng, est, SEEDS[0], 0)
    counts = counts_of(module, observed)
    module.check(name, observed.samples, est, **counts)  # the right model passes on these very samples
    with pytest.raises(AssertionError) as e:
        module.check(name, observed.samples, est, **counts, **wrong)
    print(f"{name}, estimator {est}, with {sorted(wrong)}: rejected, {str(e.value).split(' || ')[0][:300]}")
