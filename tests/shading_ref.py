"""A float64 numpy reference for what happens after the closest hit: a second reading of include/rtw.h, DESIGN.md / SURVEY.md and of
the reference's material, medium, texture and miss programs (material/*.cu, lib/sampling.cuh, lib/onb.cuh, geometry/volumeBox.cu,
volumeSphere.cu, texture/*.cu, miss/miss.cu, raygen/raygen.cu), written without looking at oracle/rtw_oracle.c or the kernels. Shared
by test_shading_cpu.py (the oracle against this file) and test_gpu_shading.py (the kernels against this file, then against the oracle).
Its neighbours: geometry_ref.py (the closest hit itself, shading normals, texture coordinates) and lighting_ref.py (direct lighting:
the light sample, its probe and the emitter hits under all four estimators), which reuses this file's cases, draws and limits.

How a single event is observed
  Sky decoder   max_depth = 2, sky_light = 1, no lights, white constant albedo. The second segment misses everything and the sample's
                red is (1 - t) + 0.5 t, t = 0.5 (u.y + 1), u the normalised scattered direction (miss.cu:8-16): u.y = 3 - 4 red, a
                float32-accurate read-out. Red is never 0 on a miss, so a sample that is exactly 0 is a LOST path (a cancel, a re-hit,
                the depth cap). The first hit is exact: plane k = 0, origin = -d, so t = 1 and the hit point is 0; the reference
                estimator's restart at 1e-6 then never re-hits. Under XFORM_Y (rotate about y, translate) the hit is inexact and the
                case runs with a corrected estimator (restart at 1e-3); lost must be 0 there too.
  Emitter       max_depth = 1, no sky. An emitter of radiance 1 behind media: the sample is 1 when the free flight passes, 0 when a
                medium (isotropic, no emission) scatters it. An emitter carrying a texture, met by rays along -y from one above an
                exactly representable point: the sample is the texture's value there.
  Keys          ray j of a case is traced on keys_per_ray consecutive stream keys, one sample each, counted from a key base. Seeds
                and keys are fixed, so every case is deterministic. Every statistical case is drawn twice (DRAWS): Philox with the
                project's default seed and with a second one; TEA+LCG, which takes no seed, on the keys from 0 and on the keys
                from KEY_SHIFT = 2^20. Cases without draws (emitters, textures) run once per generator.

What is modelled, case by case (closed form or quadrature; conditioning rule; share left out; the constant that bounds it)
  direction-mirror_*   metal at fuzz 0 (metalMaterial.cu:42-46): u = unit(d - 2 (d . n) n). The reference estimator reflects the ray
                direction as it comes, the corrected ones the unit direction: the same u after normalisation. 24
                incidences (INCIDENCES), tangents 0 to 16.5, |d| up to 66 in mirror_above_long. Nothing left out.
                MEASURED_CONSTANT_MIRROR.
  direction-glass_*    dielectricMaterial.cu:37-113 at eta 1.5: the face by dot(d, n) (front: 1 -> eta, back: eta -> 1, local normal
                turned), Snell's direction ratio (ud + cos_i n) - cos_t n, total internal reflection when ratio sin_i > 1, reflection
                with Schlick's probability r0 + (1 - r0) (1 - cos_i)^5, r0 = ((eta_i - eta_t) / (eta_i + eta_t))^2. A sample that
                returns to the side the ray came from is REFLECTED, else REFRACTED; each is held to its direction's y, the pooled
                reflected count to sum p_j by the binomial rule, and no sample may refract where only reflection is possible. Left
                out: incidences with |ratio sin_i - 1| < CRITICAL_EPS = 1e-3 - one of 24 from below (tangent 0.8949 against the
                critical 0.8944; 4.2 %), none elsewhere; at least 90 % of the rays and at least 50 samples of either kind are asked for.
                glass_share and glass_share_below put 16384 keys on one incidence of either face for the share alone.
                MEASURED_CONSTANT_MIRROR (reflected), MEASURED_CONSTANT_REFRACT (refracted).
  emitter-light*       diffuseLight.cu:54-62: the texture's colour exactly where dot(n, d) < 0, black elsewhere; both flips, both
                sides, normal and oblique. Exact equality (no arithmetic is involved). Nothing left out.
  emitter-normal_material  normalMaterial.cu:29-30 ends the path (Ray_Finish) with 0.5 n + 0.5 in the attenuation, which raygen.cu:60
                never adds to the radiance (kept): the sample is exactly 0. The colour itself is the albedo guide's
                business (include/rtw.h rtw_render_guides, tests of the guides).
  lambert-normal_*     the lobe's normal component c = |u . n| (lambert_normal_cdf): F = c^2 for the corrected estimators; the reference
                lobe (2 cos, 2 sin) sqrt(r2), sqrt(1 - r2), normalised (sampling.cuh:49-60, SURVEY Q1, kept by RTW_EST_REFERENCE)
                has F = 1 - (1 - c^2) / (1 + 3 c^2). The Lambertian scatters about the shading normal on whichever side the ray
                arrives (lambertianMaterial.cu:44-48 never looks at the ray), so flip = 1 mirrors the law: u.y = -c, below the plane.
  lambert-tangent_*    normal along +-x or +-z, so u.y is a tangent component rho cos(phi) (lambert_tangent_cdf): the semicircle law for
                the corrected lobe (rho = sqrt(r2)); for the reference lobe the marginal through rho = 2 sqrt(r2) / sqrt(1 + 3 r2) by
                Gauss-Legendre after the substitution that removes the square-root edge. The +-x cases take the other branch of the
                basis (onb.cuh:25: |w.x| > 0.9).
  fuzz-*               metal at fuzz 0.5: u = unit(r + f b), b uniform in the unit ball (FuzzLaw: the chord-length density of a ball
                seen from outside, azimuth in closed form, midpoint rule in psi, linear table). Effective fuzz f / |d| under the
                reference estimator (Q5), f under the others. At grazing incidence the cancelled samples (u . n <= 0: exactly 0,
                metalMaterial.cu:56-59) are held to the ball cap's closed form by the binomial rule and the others to the conditional
                law; elsewhere the law predicts no cancel and lost must be 0.
  slab-slab            isotropicMaterial.cu:30-51 in a wide thin slab (SlabCase, slab_law), corrected estimator: passed, escaped and
                lost shares by the binomial rule, the escaped directions' y by Kolmogorov. Neglected: escapes through the slab's
                sides (they need |mu| < 1e-4 and then survive with probability e^-10000) and the second segment's start distance
                (1e-3 of a direction no longer than 1 against a mean free path of 16: 6e-5 relative).
  media-*              transmittance(): Beer-Lambert over the chord for the corrected estimators, over everything up to the closest
                surface for the reference estimator (kept: the media never end). Both volume primitives; unnormalised
                and oblique directions, off-centre chords, origins inside (h1 < 0), the estimator's own start distance inside the
                medium (directions 2^20 and 1024 long make 1e-6 and 1e-3 one unit long), a box under XFORM_Y, two disjoint media
                whose transmittances multiply (corrected estimators). Every expected share lies in (0.05, 0.95).
  texture-noise_*      noiseTexture.cu:19-80 from the blob's own tables: gradient noise with Hermite weights, 7-octave turbulence,
                0.5 (1 + sin(scale z + 5 turb)). Noise is continuous across lattice planes: nothing left out.
                MEASURED_CONSTANT_NOISE, one per case (the error is made of other parts at scale |p| = 16 than at 2200).
  texture-checker_*    checkeredTexture.cu:9-20 with its sin(10 - p.y) kept (Textures) and the children evaluated
                (include/rtw.h): two constants; a noise and an image. Left out: points with any |sin| < SIN_EPS = 1e-3 (1 of 2000
                in either case; at least 95 % are asked for). A constant child's value must be equal, the others are bounded by
                the child's constant.
  texture-image        bilinear fetch with clamp, texel centres at (i + 0.5) / w, row 0 at v = 0 (include/rtw.h), on the 64 x 32
                test image over a 64 x 32 rectangle (u, v exact): 1200 interior points, 400 texel centres, 400 points with u or v
                equal to 0 or 1, corners included. Nothing left out. MEASURED_CONSTANT_IMAGE.

Error units of the deterministic values (first-order, in units of 2^-24; the tolerance is K_FACTOR * MEASURED_CONSTANT_* * unit)
  decoded y     4 for the decode (four times the rounding of a red in [0.5, 1]) + 8 for the direction's own operations on components
                no larger than 1; the refracted ray adds 2 ratio^2 / cos_t for the root cos_t = sqrt(1 - (ratio sin_i)^2).
  noise         0.5 ((|scale z| + 10) + 5 (7 NOISE_GRADIENT dq + 32)) + 8: dq = sum_i |fl32(scale p_i) - scale p_i| / 2^-24 is what
                fp32 does to the lattice coordinates (of the size 2^-24 scale |p|; nothing when the product is exact), carried through
                seven octaves of gradient <= NOISE_GRADIENT = 3 (octave k sees 2^k times the error at weight 2^-k) and the factor
                5; the sine's argument is rounded at its own size |scale z| + 10; 32 for the roundings inside the sums, 8 for the
                sine and what follows. The error follows scale |p|.
  image         8 + 3 (w |u| + h |v|): u and v carry two roundings each, the texel coordinate a third, texel values differ by <= 1.
  constant      none: the value is copied and must be equal.
  texture32-*   texture-* cut down to 32 points each (TextureCase.subset) for rtw_render, which takes one ray per call.
MEASURED_CONSTANT_* is the largest |fp32 - fp64| / (2^-24 unit) of THIS FILE evaluated at two precisions over the inputs of the
tests, on the CPU (`python tests/shading_ref.py` prints them; test_shading_cpu.py re-measures them and holds them to the recorded
values): MIRROR 0.2579, REFRACT 0.2055, IMAGE 0.1511, NOISE 0.0650 / 0.1136 / 0.8327 / 0.0741 (scale 4 near, scale 0.05 far, scale 4
far, the checker's noise child). The factor K_FACTOR = 4 is geometry_ref.py's: the oracle and
the kernels use fused multiply-adds where numpy rounds twice, and another, equally valid, operation order. No number here comes
from the oracle or the kernels.

Statistical cases: n = 16384 (128 x 128 keys, one sample each) per case, generator, estimator and seed; the textbook limits at a
per-case alpha of 1e-4: Kolmogorov D sqrt(n) <= 2.23, binomial |z| <= 3.89. The laws are closed forms or quadratures accurate to
1e-6 (quadrature_errors(): each against a closed form or against itself at twice the nodes), never samples.
"""
import functools
import os
import sys

import numpy as np

if __name__ == "__main__":  # `python tests/shading_ref.py` from anywhere: the package lies one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import geometry_ref as G
import law_common as C
# the limits, the draws, Case and render_params lived here first: they keep their names in this module (S.N_STAT, S.Case, ...)
from law_common import CORR, DRAWS, K_FACTOR, KEY_SHIFT, KS_LIMIT, N_STAT, REF, RNGS, SEEDS, SIDE, U, Z_LIMIT  # noqa: F401
from law_common import Case, _dot, _unit, render_params  # noqa: F401
from raytracing_weekend_amd import abi

CRITICAL_EPS = 1e-3   # incidences with |ratio * sin_i - 1| below this are left out
SIN_EPS = 1e-3        # checker points with a |sin| below this are left out
NOISE_GRADIENT = 3.0  # bound of |grad noise|: the smoothstep's slope 1.5 times the corner dots' range, plus the unit gradient

# `python tests/shading_ref.py`: this file at float32 against itself at float64, in the units of the module text
MEASURED_CONSTANT_MIRROR = 0.2579   # direction-mirror_above, reference estimator
MEASURED_CONSTANT_REFRACT = 0.2055  # direction-glass_above
MEASURED_CONSTANT_NOISE = {"noise_scale4_near": 0.0650, "noise_scale005_far": 0.1136, "noise_scale4_far": 0.8327,
                           "checker_noise_image": 0.0741}  # per texture case: the error's make-up differs with scale |p|
MEASURED_CONSTANT_IMAGE = 0.1511    # texture-checker_noise_image (the image child under inexact u, v)


# ---------------------------------------------------------------- small algebra, at the precision of its arguments
def sky_red(u, ft=np.float64):
    """Red of the sky along direction u (miss.cu:8-16): (1 - t) * 1 + t * 0.5 with t = 0.5 (unit(u).y + 1)."""
    un = _unit(np.asarray(u, ft))
    t = ft(0.5) * (un[..., 1] + ft(1.0))
    return (ft(1.0) - t) * ft(1.0) + t * ft(0.5)


def decode_uy(red):
    """The world-space y of the normalised direction that missed into the sky, from the sample's red channel."""
    return 3.0 - 4.0 * np.asarray(red, np.float64)


def mirror(d, n, ft=np.float64, unit_in=True):
    """Unit mirror direction of d about n (metalMaterial.cu:42-46 at fuzz 0). unit_in = False reflects the ray direction as it
    comes (the reference estimator) and normalises afterwards: the same direction up to rounding."""
    d, n = np.asarray(d, ft), np.asarray(n, ft)
    if unit_in:
        d = _unit(d)
    return _unit(d - ft(2.0) * _dot(d, n)[..., None] * n)


def dielectric(d, n, eta, ft=np.float64, schlick_exponent=5, invert_back_eta=False):
    """dielectricMaterial.cu:37-113 for rays d (m, 3) at a surface of shading normal n: the face by dot(d, n), Snell's direction,
    total internal reflection when ratio * sin_i > 1, Schlick's reflection probability. Returns a dict of per-ray arrays: refl, refr
    (unit directions), p (reflection probability; 1 under total internal reflection), only_reflect, margin = ratio * sin_i - 1,
    cos_t, ratio."""
    d, n = np.asarray(d, ft), np.broadcast_to(np.asarray(n, ft), np.shape(d))
    ud = _unit(d)
    front = _dot(d, n) < 0
    ln = np.where(front[:, None], n, -n)
    one = np.ones(len(d), ft)
    ei, et = np.where(front, one, ft(eta)), np.where(front, ft(eta), one)
    if invert_back_eta:
        ei, et = np.where(front, ei, one), np.where(front, et, ft(eta))
    ratio = ei / et
    cos_i = np.minimum(_dot(-ud, ln), ft(1.0))
    sin_i = np.sqrt(ft(1.0) - cos_i * cos_i)
    only_reflect = ratio * sin_i > ft(1.0)
    r0 = (ei - et) / (ei + et)
    r0 = r0 * r0
    p = np.where(only_reflect, ft(1.0), r0 + (ft(1.0) - r0) * (ft(1.0) - cos_i) ** schlick_exponent)
    refl = ud - ft(2.0) * _dot(ud, ln)[:, None] * ln
    sin_t = np.minimum(ratio * sin_i, ft(1.0))
    cos_t = np.sqrt(ft(1.0) - sin_t * sin_t)
    refr = ratio[:, None] * (ud + cos_i[:, None] * ln) - cos_t[:, None] * ln
    return {"refl": _unit(refl), "refr": _unit(refr), "p": p, "only_reflect": only_reflect,
            "margin": (ratio * sin_i - ft(1.0)).astype(np.float64), "cos_t": cos_t.astype(np.float64), "ratio": ratio.astype(np.float64)}


# ---------------------------------------------------------------- statistics
def ks_sqrt_n(x, cdf):
    """Kolmogorov's D * sqrt(n) of the sample x against the callable cdf."""
    x = np.sort(np.asarray(x, np.float64))
    n = len(x)
    f = cdf(x)
    i = np.arange(1, n + 1)
    return float(max(np.max(i / n - f), np.max(f - (i - 1) / n)) * np.sqrt(n))


def binomial_z(k, n, p):
    return float((k - n * p) / np.sqrt(n * p * (1.0 - p)))


@functools.lru_cache(maxsize=None)
def _gauss(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w  # nodes and weights on [0, 1]


def lambert_normal_cdf(c, reference):
    """CDF of c = |u . n| of the Lambertian lobe: the corrected lobe has z = sqrt(1 - r2), so c^2 = 1 - r2 and F = c^2; the reference
    lobe (2 cos sqrt(r2), 2 sin sqrt(r2), sqrt(1 - r2)) normalised (sampling.cuh:49-60) has c^2 = (1 - r2) / (1 + 3 r2),
    F = 1 - (1 - c^2) / (1 + 3 c^2)."""
    c = np.clip(np.asarray(c, np.float64), 0.0, 1.0)
    return 1.0 - (1.0 - c * c) / (1.0 + 3.0 * c * c) if reference else c * c


def semicircle_cdf(y):
    y = np.clip(np.asarray(y, np.float64), -1.0, 1.0)
    return 0.5 + (y * np.sqrt(1.0 - y * y) + np.arcsin(y)) / np.pi


def lambert_tangent_cdf(y, reference, nodes=96):
    """CDF of a tangent component y = rho cos(phi) of the Lambertian lobe, phi uniform, rho the lobe's radius in the tangent
    plane: sqrt(r2) for the corrected lobe (the closed form is semicircle_cdf, which checks this quadrature), 2 sqrt(r2) /
    sqrt(1 + 3 r2) for the reference lobe. F(|y|) = r0 + int_{r0}^{1} (1 - acos(|y| / rho(r)) / pi) dr with rho(r0) = |y|; the
    substitution r = r0 + (1 - r0) s^2 takes the square-root edge out, Gauss-Legendre in s."""
    y = np.asarray(y, np.float64)
    a = np.minimum(np.abs(y), 1.0)
    r0 = a * a / (4.0 - 3.0 * a * a) if reference else a * a
    s, w = _gauss(nodes)
    r = r0[:, None] + (1.0 - r0)[:, None] * s * s
    rho = np.sqrt(4.0 * r / (1.0 + 3.0 * r)) if reference else np.sqrt(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.clip(np.where(rho > 0, a[:, None] / rho, 1.0), 0.0, 1.0)
    inner = 1.0 - np.arccos(c) / np.pi
    fa = r0 + ((1.0 - r0)[:, None] * 2.0 * s * w * inner).sum(1)
    return np.where(y >= 0, fa, 1.0 - fa)


class FuzzLaw:
    """The law of y = u . n for u = normalize(r + f b), r the unit mirror direction with r . n = cos_a, b uniform in the unit ball,
    f < 1. r + f b is uniform in a ball that does not hold the origin, so the direction at angle theta from r has the density
    (s2^3 - s1^3) / (4 pi f^3) per steradian, s1, s2 = cos(theta) -+ sqrt(f^2 - sin(theta)^2) the ends of its chord; with
    sin(theta) = f sin(psi) that is q(psi) = sin(psi) cos(psi)^2 (3 cos(theta)^2 + f^2 cos(psi)^2) / cos(theta) on [0, pi / 2]. At
    angle theta the azimuth is uniform: P(y <= x | theta) = 1 - acos(c) / pi, c = (x - cos(theta) cos_a) / (sin(theta) sin_a) clipped
    to [-1, 1]. F is tabulated on `grid` points of y's support by the midpoint rule in psi and interpolated linearly; at normal
    incidence (sin_a = 0) y = cos(theta) and F comes from the cumulative sum of q. The cancelled share P(y <= 0) has the closed form
    of a ball's cap, k^2 (3 f - k) / (4 f^3) with k = f - cos_a, which checks the table (quadrature_error)."""

    def __init__(self, cos_a, f, grid=4097, nodes=8192):
        assert 0.0 < f < 1.0 and 0.0 < cos_a <= 1.0
        self.cos_a, self.f = float(cos_a), float(f)
        sin_a = np.sqrt(max(0.0, 1.0 - cos_a * cos_a))
        h = 0.5 * np.pi / nodes
        psi = (np.arange(nodes) + 0.5) * h
        sth = f * np.sin(psi)
        cth = np.sqrt(1.0 - sth * sth)
        q = np.sin(psi) * np.cos(psi) ** 2 * (3.0 * cth * cth + (f * np.cos(psi)) ** 2) / cth * h
        self.mass_error = abs(q.sum() - 1.0)
        if sin_a < 1e-12:
            # y = cos(theta), decreasing in psi: F(x) = 1 - Q(psi(x)), Q the cumulative of q at the cell edges
            edges_y = np.sqrt(1.0 - (f * np.sin(np.arange(nodes + 1) * h)) ** 2)
            self.x, self.F = edges_y[::-1], (1.0 - np.r_[0.0, np.cumsum(q)])[::-1]
        else:
            a, tm = np.arccos(cos_a), np.arcsin(f)
            self.x = np.linspace(np.cos(min(a + tm, np.pi)), np.cos(max(a - tm, 0.0)), grid)
            self.F = np.empty(grid)
            den = sth * sin_a
            for lo in range(0, grid, 128):
                c = (self.x[lo:lo + 128, None] - cth[None, :] * cos_a) / den[None, :]
                self.F[lo:lo + 128] = ((1.0 - np.arccos(np.clip(c, -1.0, 1.0)) / np.pi) * q[None, :]).sum(1)
        k = f - cos_a
        self.cancel_share = k * k * (3.0 * f - k) / (4.0 * f ** 3) if k > 0 else 0.0
        self.quadrature_error = max(self.mass_error, abs(float(self.cdf(0.0)) - self.cancel_share))

    def cdf(self, x):
        return np.interp(np.asarray(x, np.float64), self.x, self.F, left=0.0, right=1.0)

    def cdf_alive(self, x):
        """CDF of y given that the sample was not cancelled (y > 0)."""
        return np.clip((self.cdf(x) - self.cancel_share) / (1.0 - self.cancel_share), 0.0, 1.0)


def slab_law(tau):
    """Single scattering in a slab of optical thickness tau hit at normal incidence from above, isotropic phase function: the
    scatter depth has density e^{-z} in optical units, the direction's cosine mu to the upward normal is uniform in [-1, 1], the
    path escapes without a second collision with probability e^{-z / mu} (upwards) or e^{-(tau - z) / |mu|} (downwards). Integrated
    over the depth: A(mu) = (1 - e^{-tau (1 + 1 / mu)}) / (1 + 1 / mu) for mu > 0 and e^{-tau} (1 - e^{-tau k}) / k with
    k = 1 / |mu| - 1 for mu < 0 (tau e^{-tau} at k = 0). Returns (passed share e^{-tau}, escaped share, cdf): cdf(x) = P(mu <= x |
    scattered once and escaped), Gauss-Legendre over [-1, x] and [0, x]."""
    s, w = _gauss(96)

    def a_up(mu):
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            g = 1.0 + 1.0 / mu
            return np.where(mu > 0, -np.expm1(-tau * g) / g, 0.0)

    def a_down(m):
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            k = 1.0 / m - 1.0
            return np.where(m > 0, np.exp(-tau) * np.where(k > 1e-12, -np.expm1(-tau * k) / np.where(k > 1e-12, k, 1.0), tau), 0.0)
    down_all = float((0.5 * a_down(s) * w).sum())
    up_all = float((0.5 * a_up(s) * w).sum())
    escaped = down_all + up_all

    def cdf(x):
        x = np.clip(np.asarray(x, np.float64), -1.0, 1.0)
        m_lo = np.maximum(-x, 0.0)  # |mu| from m_lo to 1 on the downward side
        down = (0.5 * a_down(m_lo[:, None] + (1.0 - m_lo)[:, None] * s) * w * (1.0 - m_lo)[:, None]).sum(1)
        hi = np.maximum(x, 0.0)
        up = (0.5 * a_up(hi[:, None] * s) * w * hi[:, None]).sum(1)
        return (down + up) / escaped
    return float(np.exp(-tau)), escaped, cdf


# ---------------------------------------------------------------- media
def transmittance(blob, o, d, tmin, bounded, density_factor=1.0):
    """The probability that the free flight of ray (o, d) passes every medium of the blob before its closest surface hit at t_s
    (geometry_ref.closest_hit). Per volume primitive, in its object space (t is the same parameter there): [h1, h2] the ray's
    interval inside the boundary, entry = max(h1, tmin, 0), exit = min(h2, t_s); nothing happens when entry >= exit
    (volumeBox.cu:62-71, volumeSphere.cu:74-86). bounded: exp(-density (exit - entry) |d|), the corrected estimators; not bounded:
    exp(-density (t_s - entry) |d|), the reference estimator, whose media never end (the flight is accepted while it is
    shorter than the closest hit). The media's draws are independent, so the probabilities multiply."""
    prims, xforms = G.scene_tables(blob)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    ray = np.concatenate([o, d, [tmin, 1e27]]).astype(np.float32)[None, :]
    t_s = float(G.closest_hit(blob, ray)["t"][0])
    out = 1.0
    for pr in prims:
        if pr["type"] not in (abi.PRIM_VOLUME_BOX, abi.PRIM_VOLUME_SPHERE):
            continue
        inv = xforms["inv"][pr["xform"]].reshape(3, 4).astype(np.float64)
        oo, dd = inv[:, :3] @ o + inv[:, 3], inv[:, :3] @ d
        p = pr["p"].astype(np.float64)
        if pr["type"] == abi.PRIM_VOLUME_BOX:
            with np.errstate(divide="ignore"):
                t0, t1 = (p[0:3] - oo) / dd, (p[3:6] - oo) / dd
            h1, h2, density = np.max(np.minimum(t0, t1)), np.min(np.maximum(t0, t1)), p[6]
            if h1 > h2:
                continue
        else:
            oc = oo - p[0:3]
            a, b, c = dd @ dd, oc @ dd, oc @ oc - p[3] * p[3]
            disc = b * b - a * c
            if disc <= 0:
                continue
            h1, h2, density = (-b - np.sqrt(disc)) / a, (-b + np.sqrt(disc)) / a, p[4]
        entry, leave = max(h1, tmin, 0.0), min(h2, t_s)
        if entry >= leave:
            continue
        out *= np.exp(-density * density_factor * ((leave if bounded else t_s) - entry) * np.sqrt(dd @ dd))
    return float(out)


# ---------------------------------------------------------------- textures
def _perlin(ranvec, perm, q, ft):
    """noiseTexture.cu:19-54: gradient noise with Hermite weights over the lattice cell of q (n, 3)."""
    fl = np.floor(q)
    f = q - fl
    ijk = fl.astype(np.int64)
    s = f * f * (ft(3.0) - ft(2.0) * f)
    acc = np.zeros(q.shape[0], ft)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                idx = perm[0][(ijk[:, 0] + di) & 255] ^ perm[1][(ijk[:, 1] + dj) & 255] ^ perm[2][(ijk[:, 2] + dk) & 255]
                c = ranvec[idx].astype(ft)
                wv = f - np.array([di, dj, dk], ft)
                wx = s[:, 0] if di else ft(1.0) - s[:, 0]
                wy = s[:, 1] if dj else ft(1.0) - s[:, 1]
                wz = s[:, 2] if dk else ft(1.0) - s[:, 2]
                acc = acc + wx * wy * wz * _dot(c, wv)
    return acc


def _turbulence(ranvec, perm, q, ft):
    """noiseTexture.cu:56-69: seven octaves, weights halving, frequencies doubling, absolute value of the sum."""
    acc, weight = np.zeros(q.shape[0], ft), ft(1.0)
    for _ in range(7):
        acc = acc + weight * _perlin(ranvec, perm, q, ft)
        weight = weight * ft(0.5)
        q = q * ft(2.0)
    return np.abs(acc)


def texture_value(blob, tex, u, v, p, ft=np.float64, checker_py="10-y", row0_at_v1=False):
    """(value (n, 3), well-conditioned (n,), error unit (n,), kind (n,)) of texture `tex` of the blob at coordinates u, v and points
    p (n, 3), evaluated at precision ft. The unit is the first-order fp32 error of the value in units of 2^-24 (module text); kind is
    the type of the texture that gave the value (a checker hands on its child's), which selects the measured constant."""
    parts = abi.parse_scene(blob)
    words = np.frombuffer(parts["texdata"], "<u4") if parts["texdata"] else np.zeros(0, "<u4")
    return _texture(parts["textures"], words, tex, np.asarray(u, ft), np.asarray(v, ft), np.asarray(p, ft), ft, checker_py, row0_at_v1)


def _texture(texs, words, tex, u, v, p, ft, checker_py, row0_at_v1):
    t = texs[tex]
    n = p.shape[0]
    if t.type == abi.TEX_CONSTANT:
        return np.broadcast_to(np.array(list(t.color), ft), (n, 3)).copy(), np.ones(n, bool), np.ones(n), np.full(n, abi.TEX_CONSTANT)
    if t.type == abi.TEX_NOISE:  # noiseTexture.cu:72-80
        base = int(t.data)
        ranvec = words[base:base + 768].view("<f4").reshape(256, 3)
        perm = [words[base + 768 + 256 * a:base + 1024 + 256 * a].view("<i4").astype(np.int64) for a in range(3)]
        scale = ft(np.float32(t.scale))
        q = scale * p
        val = ft(0.5) * (ft(1.0) + np.sin(scale * p[:, 2] + ft(5.0) * _turbulence(ranvec, perm, q, ft)))
        # the unit: what fp32 does to q = scale * p (nothing when the product is exact) goes through seven octaves of gradient
        # <= NOISE_GRADIENT each (octave k sees 2^k times the error with weight 2^-k) and through the factor 5; the argument
        # scale * z + 5 turb is rounded at its own size; 32 for the roundings inside the octaves' sums, 8 for sin and what follows
        q64 = np.float64(np.float32(t.scale)) * p.astype(np.float64)
        dq = np.abs((np.float32(t.scale) * p.astype(np.float32)).astype(np.float64) - q64).sum(1) / U
        unit = 0.5 * ((np.abs(q64[:, 2]) + 10.0) + 5.0 * (7.0 * NOISE_GRADIENT * dq + 32.0)) + 8.0
        return np.repeat(val[:, None], 3, 1), np.ones(n, bool), unit, np.full(n, abi.TEX_NOISE)
    if t.type == abi.TEX_IMAGE:  # imageTexture.cu:10-16 with include/rtw.h's conventions: bilinear, clamped, centres at (i + 0.5) / w
        base = int(t.data)
        w, h = int(words[base]), int(words[base + 1])
        texel = words[base + 2:base + 2 + w * h].reshape(h, w)
        rgb = np.stack([(texel >> s) & 255 for s in (0, 8, 16)], -1).astype(ft) / ft(255.0)
        if row0_at_v1:
            rgb = rgb[::-1]
        x, y = u * ft(w) - ft(0.5), v * ft(h) - ft(0.5)
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0)[:, None], (y - y0)[:, None]
        i0, i1 = np.clip(x0.astype(np.int64), 0, w - 1), np.clip(x0.astype(np.int64) + 1, 0, w - 1)
        j0, j1 = np.clip(y0.astype(np.int64), 0, h - 1), np.clip(y0.astype(np.int64) + 1, 0, h - 1)
        top = (ft(1.0) - fx) * rgb[j0, i0] + fx * rgb[j0, i1]
        bot = (ft(1.0) - fx) * rgb[j1, i0] + fx * rgb[j1, i1]
        unit = 8.0 + 3.0 * (w * np.abs(u.astype(np.float64)) + h * np.abs(v.astype(np.float64)))
        return (ft(1.0) - fy) * top + fy * bot, np.ones(n, bool), unit, np.full(n, abi.TEX_IMAGE)
    if t.type == abi.TEX_CHECKER:  # checkeredTexture.cu:9-20; the children are evaluated (include/rtw.h)
        py = ft(10.0) - p[:, 1] if checker_py == "10-y" else ft(10.0) * p[:, 1]
        sx, sy, sz = np.sin(ft(10.0) * p[:, 0]), np.sin(py), np.sin(ft(10.0) * p[:, 2])
        odd = (sx * sy * sz) < 0
        well = (np.abs(sx) >= SIN_EPS) & (np.abs(sy) >= SIN_EPS) & (np.abs(sz) >= SIN_EPS)
        vo, oo, uo, ko = _texture(texs, words, t.odd, u, v, p, ft, checker_py, row0_at_v1)
        ve, oe, ue, ke = _texture(texs, words, t.even, u, v, p, ft, checker_py, row0_at_v1)
        return np.where(odd[:, None], vo, ve), well & np.where(odd, oo, oe), np.where(odd, uo, ue), np.where(odd, ko, ke)
    raise ValueError(f"texture type {t.type}")


# ---------------------------------------------------------------- scene builders
def _header(sky):
    hdr = abi.SceneHeader()
    hdr.magic, hdr.version, hdr.sky_light = abi.RTW_SCENE_MAGIC, abi.RTW_SCENE_VERSION, sky
    return hdr


def _constant(rgb):
    t = abi.Texture(type=abi.TEX_CONSTANT)
    t.color[0], t.color[1], t.color[2] = (float(c) for c in rgb)
    return t


def _prim(ptype, params, material=0, xf=0, flip=0):
    pr = abi.Prim(type=ptype, material=material, xform=xf, flip=flip)
    for i, v in enumerate(params):
        pr.p[i] = float(v)
    return pr


def _scene(sky, prims, materials, textures, xforms=(), texdata=b""):
    return abi.assemble_scene({"header": _header(sky), "prims": prims, "xforms": [G.identity_xform()] + list(xforms), "lights": [],
                               "materials": materials, "textures": textures, "texdata": texdata})


BSDF_EVAL = {abi.MAT_LAMBERTIAN: 0, abi.MAT_DIELECTRIC: 1, abi.MAT_METAL: 2}
RECT_OF_AXIS = (abi.PRIM_RECT_X, abi.PRIM_RECT_Y, abi.PRIM_RECT_Z)
XFORM_Y = (1, 30.0, (3.0, 0.5, -2.0))  # rotate about y, then translate: the plane y = 0 becomes y = 0.5, its normal stays +-y


def surface_scene(mat, fuzz_or_eta=0.0, axis=1, flip=0, xformed=False, sky=1, color=(1.0, 1.0, 1.0)):
    """One rectangle |a|, |b| <= 1000 in the plane k = 0 of the given axis, carrying one material with a constant texture."""
    xf = [G.rigid_xform(*XFORM_Y)] if xformed else []
    return _scene(sky, [_prim(RECT_OF_AXIS[axis], (-1000.0, 1000.0, -1000.0, 1000.0, 0.0), xf=len(xf), flip=flip)],
                  [abi.Material(type=mat, texture=0, fuzz_or_eta=fuzz_or_eta, bsdf_eval=BSDF_EVAL.get(mat, -1))], [_constant(color)], xf)


def media_scene(media, xformed=False):
    """An emitter of radiance 1 in the plane y = 0 (facing up) below the given media: ("box", (x0, y0, z0, x1, y1, z1), density) or
    ("sphere", (cx, cy, cz, r), density); isotropic white. xformed puts the first medium under XFORM_Y."""
    prims = [_prim(abi.PRIM_RECT_Y, (-1000.0, 1000.0, -1000.0, 1000.0, 0.0), material=0)]
    for i, (kind, geo, density) in enumerate(media):
        prims.append(_prim(abi.PRIM_VOLUME_BOX if kind == "box" else abi.PRIM_VOLUME_SPHERE, tuple(geo) + (density,), material=1,
                           xf=1 if xformed and i == 0 else 0))
    mats = [abi.Material(type=abi.MAT_DIFFUSE_LIGHT, texture=0, fuzz_or_eta=0.0, bsdf_eval=-1),
            abi.Material(type=abi.MAT_ISOTROPIC, texture=0, fuzz_or_eta=0.0, bsdf_eval=-1)]
    return _scene(0, prims, mats, [_constant((1.0, 1.0, 1.0))], [G.rigid_xform(*XFORM_Y)] if xformed else [])


def probe_scene():
    """Sky and, a million units below, a white Lambertian rectangle of two by two that no sample reaches: every direction misses."""
    return _scene(1, [_prim(abi.PRIM_RECT_Y, (-1.0, 1.0, -1.0, 1.0, -1.0e6))],
                  [abi.Material(type=abi.MAT_LAMBERTIAN, texture=0, fuzz_or_eta=0.0, bsdf_eval=0)], [_constant((1.0, 1.0, 1.0))])


STRIP_K = (-3.5, -2.25, -1.125, -0.375, 0.5, 1.75, 2.625, 3.875)  # the strips' planes for X = 4; they scale with X


def strip_scene(textures, texdata, tex, X):
    """Eight emitters showing texture `tex`: y-rectangles facing up over disjoint strips of x in [-X, X] (strip j: one sixteenth of
    its width free on both sides), z in [-X, X], at the heights STRIP_K * X / 4, so that rays along -y reach points of many y."""
    wd = 2.0 * X / len(STRIP_K)
    prims = [_prim(abi.PRIM_RECT_Y, (-X + j * wd + wd / 16, -X + (j + 1) * wd - wd / 16, -X, X, k * X / 4)) for j, k in enumerate(STRIP_K)]
    return _scene(0, prims, [abi.Material(type=abi.MAT_DIFFUSE_LIGHT, texture=tex, fuzz_or_eta=0.0, bsdf_eval=-1)], textures, texdata=texdata)


def strip_points(blob, n, grid, seed):
    """n points (float64, every coordinate a multiple of `grid`) strictly inside strip_scene's rectangles, and their strips."""
    prims, _ = G.scene_tables(blob)
    rng = np.random.default_rng(seed)
    j = rng.integers(0, len(prims), n)
    P = prims["p"][j].astype(np.float64)

    def inside(lo, hi):
        a, b = np.ceil(lo / grid) + 1, np.floor(hi / grid) - 1
        return grid * np.floor(a + rng.uniform(0, 1, n) * (b - a + 1)).clip(a, b)
    return np.stack([inside(P[:, 0], P[:, 1]), P[:, 4], inside(P[:, 2], P[:, 3])], -1), j


# ---------------------------------------------------------------- cases
def lost_count(red):
    return int((np.asarray(red) == 0).sum())


class DirectionCase(Case):
    """Mirror (eta None) or glass at a surface of unit shading normal n (+-y): the y of every sample's scattered direction against
    the mirror and the Snell direction, every sample classified (it returns to the side the ray came from: reflected), the
    reflected share against Schlick."""

    def __init__(self, blob, o, d, n, eta, keys_per_ray, estimators=(REF, CORR)):
        super().__init__(blob, o, d, keys_per_ray)
        self.n, self.eta, self.estimators = np.asarray(n, np.float64), eta, estimators

    def expect(self, estimator, ft=np.float64, **model):
        m = self.m
        if self.eta is None:
            r = mirror(self.d, self.n, ft, unit_in=estimator != REF)
            e = {"refl": r, "refr": r, "p": np.ones(m), "only_reflect": np.ones(m, bool), "margin": np.full(m, -1.0), "cos_t": np.ones(m),
                 "ratio": np.ones(m)}
        else:
            e = dielectric(self.d, self.n, self.eta, ft, **model)
        e["ok"] = np.abs(e["margin"]) >= CRITICAL_EPS
        # units of 2^-24: 4 for the decode (four times the rounding of a red in [0.5, 1]), 8 for the direction's own operations, and
        # for the refracted ray the root cos_t = sqrt(1 - (ratio sin_i)^2), whose error grows as ratio^2 / cos_t
        e["unit_refl"] = np.full(m, 12.0)
        e["unit_refr"] = 12.0 + 2.0 * e["ratio"] ** 2 / np.maximum(e["cos_t"], 1e-12)
        return e

    def fp32_constants(self, estimator):
        """(mirror, refraction): max |y32 - y64| / (2^-24 unit) of the decoded y, this file at float32 against itself at float64."""
        e64, e32 = self.expect(estimator), self.expect(estimator, np.float32)
        ok = e64["ok"]
        out = []
        for key, unit in (("refl", "unit_refl"), ("refr", "unit_refr")):
            y32 = decode_uy(sky_red(e32[key], np.float32))
            out.append(float(np.max(np.abs(y32 - e64[key][:, 1])[ok] / (U * e64[unit][ok]))))
        return out[0], out[1] if self.eta is not None else 0.0

    def check(self, samples, estimator, **model):
        e = self.expect(estimator, **model)
        red = samples[..., 0].astype(np.float64)
        lost = lost_count(red)
        uy = decode_uy(red)
        back = uy * self.d[:, 1:2] < 0
        ok, both = e["ok"], e["ok"] & ~e["only_reflect"]
        err_r = np.abs(uy - e["refl"][:, 1:2]) / (U * e["unit_refl"][:, None])
        err_t = np.abs(uy - e["refr"][:, 1:2]) / (U * e["unit_refr"][:, None])
        worst_r = float(err_r[ok][back[ok]].max()) if back[ok].any() else 0.0
        worst_t = float(err_t[ok][~back[ok]].max()) if (~back[ok]).any() else 0.0
        k_r, k_t = K_FACTOR * MEASURED_CONSTANT_MIRROR, K_FACTOR * MEASURED_CONSTANT_REFRACT
        n_refl, n_refr = int(back[both].sum()), int((~back[both]).sum())
        z = 0.0
        if both.any():
            p = e["p"][both].astype(np.float64)
            z = float((n_refl - self.keys_per_ray * p.sum()) / np.sqrt(self.keys_per_ray * (p * (1.0 - p)).sum()))
        fig = (f"lost {lost}, rays checked {ok.sum()} of {self.m}, reflected y off by {worst_r:.2f} units (K = {k_r:.2f}), refracted y off by "
               f"{worst_t:.2f} units (K = {k_t:.2f}), {n_refl} reflected / {n_refr} refracted where both are possible, Schlick z = {z:+.2f}")
        assert lost == 0, fig
        assert ok.mean() >= 0.9, fig
        assert not (~back[ok & e["only_reflect"]]).any(), fig + "; a refracted sample where only reflection is possible"
        assert worst_r <= k_r and worst_t <= k_t, fig
        if both.any():
            assert n_refl >= 50 and n_refr >= 50, fig
            assert abs(z) <= Z_LIMIT, fig
        return fig


class LambertCase(Case):
    """One ray at a Lambertian rectangle; kind "normal": the surface's normal is sign * y and y = sign * c is tested against the
    lobe's normal-component law; kind "tangent": the normal is along x or z and y is a tangent component."""

    def __init__(self, blob, o, d, kind, sign=1.0, estimators=(REF, CORR)):
        super().__init__(blob, o, d, N_STAT)
        self.kind, self.sign, self.estimators = kind, sign, estimators

    def check(self, samples, estimator, lobe=None):
        reference = (estimator == REF) if lobe is None else lobe == "reference"
        red = samples[0, :, 0].astype(np.float64)
        lost, uy = lost_count(red), decode_uy(red)
        if self.kind == "normal":
            ks = ks_sqrt_n(self.sign * uy, lambda c: lambert_normal_cdf(c, reference))
        else:
            ks = ks_sqrt_n(uy, lambda y: lambert_tangent_cdf(y, reference))
        fig = f"lost {lost}, KS sqrt(n) = {ks:.2f} against the {'reference' if reference else 'cosine'} lobe (limit {KS_LIMIT})"
        assert lost == 0, fig
        assert ks <= KS_LIMIT, fig
        return fig


class FuzzCase(Case):
    """One ray at a metal of fuzz f, normal +y: the cancelled share (samples that are exactly 0) against the ball's cap, the y of
    the others against FuzzLaw. The effective fuzz is f / |d| under the reference estimator, f under the others."""

    def __init__(self, blob, o, d, fuzz):
        super().__init__(blob, o, d, N_STAT)
        self.fuzz = fuzz

    def law(self, estimator):
        length = float(np.sqrt(_dot(self.d[0], self.d[0])))
        return _fuzz_law(round(float(-self.d[0, 1] / length), 15), self.fuzz / length if estimator == REF else self.fuzz)

    def check(self, samples, estimator):
        law = self.law(estimator)
        red = samples[0, :, 0].astype(np.float64)
        lost, n = lost_count(red), len(red)
        ks = ks_sqrt_n(decode_uy(red[red != 0]), law.cdf_alive)
        z = binomial_z(lost, n, law.cancel_share) if law.cancel_share > 0 else 0.0
        fig = (f"effective fuzz {law.f:.4f}, cancelled {lost} of {n} (expected share {law.cancel_share:.5f}, z = {z:+.2f}), "
               f"KS sqrt(n) = {ks:.2f} (limit {KS_LIMIT}), quadrature error {law.quadrature_error:.1e}")
        assert law.quadrature_error < 1e-6, fig
        assert (lost == 0) if law.cancel_share == 0 else abs(z) <= Z_LIMIT, fig
        assert ks <= KS_LIMIT, fig
        return fig


@functools.lru_cache(maxsize=None)
def _fuzz_law(cos_a, f):
    return FuzzLaw(cos_a, f)


SLAB_H, SLAB_SIGMA, SLAB_HALF = 16.0, 1.0 / 16.0, 262144.0


class SlabCase(Case):
    """A wide thin slab of isotropic medium (thickness 16, half-width 2^18 >= 1e4 thicknesses, optical thickness 1) under the sky,
    hit at normal incidence from above with max_depth = 2: the passed share (red exactly 1: the sky straight down), the lost share
    (a second collision ends at the depth cap) and the law of the escaped directions' y against slab_law."""
    estimators = (CORR,)

    def __init__(self):
        blob = _scene(1, [_prim(abi.PRIM_VOLUME_BOX, (-SLAB_HALF, 16.0, -SLAB_HALF, SLAB_HALF, 16.0 + SLAB_H, SLAB_HALF, SLAB_SIGMA))],
                      [abi.Material(type=abi.MAT_ISOTROPIC, texture=0, fuzz_or_eta=0.0, bsdf_eval=-1)], [_constant((1.0, 1.0, 1.0))])
        super().__init__(blob, (0.0, 48.0, 0.0), (0.0, -1.0, 0.0), N_STAT)

    def check(self, samples, estimator):
        passed_p, escaped_p, cdf = slab_law(SLAB_SIGMA * SLAB_H)
        red = samples[0, :, 0].astype(np.float64)
        n = len(red)
        passed, lost = int((red == 1.0).sum()), lost_count(red)
        esc = decode_uy(red[(red != 0) & (red != 1.0)])
        ks = ks_sqrt_n(esc, cdf)
        z_pass, z_lost, z_esc = binomial_z(passed, n, passed_p), binomial_z(lost, n, 1.0 - passed_p - escaped_p), binomial_z(len(esc), n, escaped_p)
        fig = (f"passed {passed} (expected {passed_p:.4f}, z = {z_pass:+.2f}), escaped {len(esc)} ({escaped_p:.4f}, z = {z_esc:+.2f}), lost {lost} "
               f"({1 - passed_p - escaped_p:.4f}, z = {z_lost:+.2f}), KS sqrt(n) of the escaped y = {ks:.2f}")
        assert max(abs(z_pass), abs(z_lost), abs(z_esc)) <= Z_LIMIT and ks <= KS_LIMIT, fig
        return fig


class MediaCase(Case):
    """One ray through media towards an emitter of radiance 1, max_depth = 1: a sample is 1 when the free flight passes and 0 when
    a medium scatters it; the share of ones against transmittance()."""
    depth = 1
    estimators = (REF, CORR, abi.RTW_EST_CORRECTED_NO_NEE, abi.RTW_EST_MIXTURE)

    def __init__(self, blob, o, d, n=N_STAT, estimators=None):
        super().__init__(blob, o, d, n)
        if estimators is not None:
            self.estimators = estimators

    def expect(self, estimator, bounded=None, density_factor=1.0):
        bounded = (estimator != REF) if bounded is None else bounded
        return transmittance(self.blob, self.o[0], self.d[0], self.tmin(estimator), bounded, density_factor)

    def check(self, samples, estimator, **model):
        p = self.expect(estimator, **model)
        s = samples[0]
        assert np.isin(s, (0.0, 1.0)).all() and (s == s[:, :1]).all(), "a sample that is neither the emitter nor black"
        k, n = int((s[:, 0] == 1.0).sum()), len(s)
        z = binomial_z(k, n, p)
        fig = f"passed {k} of {n}, expected share {p:.5f}, z = {z:+.2f} (limit {Z_LIMIT})"
        assert 0.05 < p < 0.95, fig  # the case has power in both directions
        assert abs(z) <= Z_LIMIT, fig
        return fig


class EmitterCase(Case):
    """Rays at a rectangle (normal +-y by its flip flag) from both sides, max_depth = 1: a diffuse light of colour `color` shows its
    colour exactly where dot(n, d) < 0 and black elsewhere (diffuseLight.cu:54-62); RTW_MAT_NORMAL (color None) ends the path with
    its colour 0.5 n + 0.5 in the attenuation, which never reaches the radiance (normalMaterial.cu:29-30): black."""
    depth = 1
    drawn = False

    def __init__(self, mat, flip, color):
        d = np.array([(0.0, -1.0, 0.0), (0.5, -1.0, 0.25), (-3.0, -1.0, 2.0), (0.0, 1.0, 0.0), (0.5, 1.0, 0.25), (-3.0, 1.0, 2.0)])
        super().__init__(surface_scene(mat, flip=flip, sky=0, color=color or (1.0, 1.0, 1.0)), -d, d, 4)
        self.color, self.n_y = color, -1.0 if flip else 1.0

    def check(self, samples, estimator):
        want = np.zeros((self.m, 1, 3), np.float32)
        if self.color is not None:
            want[self.n_y * self.d[:, 1] < 0, 0] = np.array(self.color, np.float32)
        assert np.array_equal(samples, np.broadcast_to(want, samples.shape)), f"got {samples[:, 0]}, expected {want[:, 0]}"
        return f"{self.m} rays exact"


class TextureCase(Case):
    """Rays along -y from one above to exactly representable points of emitters that carry a texture, max_depth = 1: the sample is
    the texture's value at the point."""
    depth = 1
    drawn = False

    def __init__(self, blob, points, strips, noise_constant=0.0, classes=None):
        super().__init__(blob, points + np.array([0.0, 1.0, 0.0]), np.broadcast_to(np.array([0.0, -1.0, 0.0]), points.shape), 1)
        assert np.array_equal(self.o.astype(np.float64), points + np.array([0.0, 1.0, 0.0])), "a point is not exact in float32"
        self.points, self.strips, self.noise_constant = points, strips, noise_constant
        self.classes = np.zeros(len(points), np.int64) if classes is None else classes

    def subset(self, n=32):
        """The case cut down to n well-conditioned points for entries that take one ray per call: the points are dealt out in turn to
        the groups (strip, class of point, texture that gives the value, which constant it is), so that every strip, every class of
        the image's points (interior, texel centre, the two edges, corner) and both parities of a checker are among them."""
        val, ok, _, kind = self.expect()
        key = np.stack([self.strips, self.classes, kind, np.where(kind == abi.TEX_CONSTANT, np.rint(10 * val[:, 0]), 0).astype(np.int64)], -1)
        groups = [np.nonzero(ok & (key == g).all(1))[0] for g in np.unique(key[ok], axis=0)]
        pick, turn = [], 0
        while len(pick) < n:
            pick += [g[turn] for g in groups if turn < len(g)][:n - len(pick)]
            turn += 1
        pick = np.array(sorted(pick))
        return TextureCase(self.blob, self.points[pick], self.strips[pick], self.noise_constant, self.classes[pick])

    def expect(self, ft=np.float64, **model):
        parts = abi.parse_scene(self.blob)
        val, ok, unit, kind = np.zeros((self.m, 3), ft), np.zeros(self.m, bool), np.ones(self.m), np.zeros(self.m, np.int64)
        for j in np.unique(self.strips):
            mine = self.strips == j
            pr = parts["prims"][int(j)]
            a0, a1, b0, b1 = (ft(np.float32(pr.p[i])) for i in range(4))
            p = self.points[mine].astype(ft)
            u, v = (p[:, 0] - a0) / (a1 - a0), (p[:, 2] - b0) / (b1 - b0)
            val[mine], ok[mine], unit[mine], kind[mine] = texture_value(self.blob, parts["materials"][pr.material].texture, u, v, p, ft, **model)
        return val, ok, unit, kind

    def fp32_constants(self):
        """{texture type: max |value32 - value64| / (2^-24 unit)} over the well-conditioned points."""
        v64, ok, unit, kind = self.expect()
        v32 = self.expect(np.float32)[0]
        err = np.abs(v32.astype(np.float64) - v64).max(1) / (U * unit)
        return {int(k): float(err[ok & (kind == k)].max()) for k in np.unique(kind[ok])}

    def check(self, samples, estimator, **model):
        val, ok, unit, kind = self.expect(**model)
        # a constant's value is copied: equality; the others: 4 x the case's own noise constant, 4 x the image's
        k = K_FACTOR * np.select([kind == abi.TEX_NOISE, kind == abi.TEX_IMAGE], [self.noise_constant, MEASURED_CONSTANT_IMAGE], 0.0)
        err = np.abs(samples[:, 0, :].astype(np.float64) - val).max(1) / (U * unit)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(ok, np.where(k > 0, err / k, np.where(err > 0, np.inf, 0.0)), 0.0)
        worst = int(np.argmax(rel))
        fig = (f"{ok.sum()} of {self.m} points checked, largest error / K = {rel[worst]:.3f} ({err[worst]:.2f} units at point "
               f"{self.points[worst]}, K = {k[worst]:.3f}), largest |value - value64| = {np.abs(samples[:, 0, :] - val)[ok].max():.2e}")
        assert ok.mean() >= 0.95, fig
        assert (err[ok] <= k[ok]).all(), fig
        return fig


# the incidences of the deterministic direction cases: (dx, dz) beside dy = -+1, tangents from 0 to 16.5; the back face's critical
# tangent is 0.8944 (eta 1.5): (7/8, 3/16) lies within CRITICAL_EPS of it and is left out there
INCIDENCES = ((0, 0), (1 / 16, 0), (0, 1 / 8), (3 / 16, 1 / 8), (1 / 4, 1 / 4), (1 / 2, 0), (1 / 2, 1 / 4), (5 / 8, 1 / 4), (3 / 4, 1 / 8), (3 / 4, 3 / 8),
              (7 / 8, 1 / 8), (7 / 8, 3 / 16), (1, 0), (1, 1 / 2), (1, 1), (3 / 2, 1 / 2), (2, 0), (2, 1), (3, 1), (4, 0), (5, 2), (8, 1), (0, 12), (16, 4))
ETA = 1.5


def _direction_case(mat, eta, side, flip=0, xformed=False, scale=1.0):
    """side -1: rays from above (d.y = -scale), +1: from below. Identity: the origin is -d and the hit point 0 exactly (t = 1)."""
    d = np.array([(dx, side, dz) for dx, dz in INCIDENCES], np.float64) * scale
    hit = np.array([1.0, 0.5, -3.0]) if xformed else np.zeros(3)
    blob = surface_scene(mat, fuzz_or_eta=eta or 0.0, flip=flip, xformed=xformed)
    return DirectionCase(blob, hit - d, d, (0.0, -1.0 if flip else 1.0, 0.0), eta, 256, estimators=(CORR,) if xformed else (REF, CORR))


def _lambert_case(axis, flip, o, d, kind, xformed=False):
    blob = surface_scene(abi.MAT_LAMBERTIAN, axis=axis, flip=flip, xformed=xformed)
    return LambertCase(blob, o, d, kind, sign=-1.0 if flip else 1.0, estimators=(CORR,) if xformed else (REF, CORR))


def _fuzz_case(d, fuzz=0.5):
    d = np.asarray(d, np.float64)
    return FuzzCase(surface_scene(abi.MAT_METAL, fuzz_or_eta=fuzz), -d, d, fuzz)


BOX = ("box", (-50.0, 1.0, -50.0, 50.0, 3.0, 50.0), 0.4)
BALL = ("sphere", (0.0, 3.0, 0.0, 1.5), 0.5)


def _texture_cases():
    import oracle  # the builders of Perlin tables and of the test image only (pure Python): the oracle library is not loaded here
    tables, image = oracle.perlin_tables(1), oracle.test_image()
    texdata = tables + image

    def noise(scale):
        return [abi.Texture(type=abi.TEX_NOISE, scale=scale, data=0)]
    chk_const = [abi.Texture(type=abi.TEX_CHECKER, odd=1, even=2), _constant((0.9, 0.2, 0.1)), _constant((0.1, 0.2, 0.9))]
    chk_nested = [abi.Texture(type=abi.TEX_CHECKER, odd=1, even=2), abi.Texture(type=abi.TEX_NOISE, scale=4.0, data=0),
                  abi.Texture(type=abi.TEX_IMAGE, data=len(tables) // 4)]

    def strips(name, textures, X, grid, seed):
        blob = strip_scene(textures, texdata, 0, X)
        return TextureCase(blob, *strip_points(blob, 2000, grid, seed), noise_constant=MEASURED_CONSTANT_NOISE.get(name, 0.0))

    def image_case():
        # one 64 x 32 rectangle showing the 64 x 32 test image: u = x / 64 and v = z / 32 are exact, x and z are texel coordinates
        blob = _scene(0, [_prim(abi.PRIM_RECT_Y, (0.0, 64.0, 0.0, 32.0, 0.0))],
                      [abi.Material(type=abi.MAT_DIFFUSE_LIGHT, texture=0, fuzz_or_eta=0.0, bsdf_eval=-1)],
                      [abi.Texture(type=abi.TEX_IMAGE, data=0)], texdata=image)
        rng = np.random.default_rng(11)
        interior = np.stack([rng.integers(1, 64 * 16, 1200) / 16.0, rng.integers(1, 32 * 16, 1200) / 16.0], -1)
        centres = np.stack([rng.integers(0, 64, 400) + 0.5, rng.integers(0, 32, 400) + 0.5], -1)
        edge_x = np.stack([rng.choice([0.0, 64.0], 200), rng.integers(0, 32 * 16 + 1, 200) / 16.0], -1)
        edge_z = np.stack([rng.integers(0, 64 * 16 + 1, 196) / 16.0, rng.choice([0.0, 32.0], 196)], -1)
        corners = np.array([(0.0, 0.0), (64.0, 0.0), (0.0, 32.0), (64.0, 32.0)])
        xz = np.concatenate([interior, centres, edge_x, edge_z, corners])
        classes = np.repeat(np.arange(5), [1200, 400, 200, 196, 4])  # interior, texel centre, edge in u, edge in v, corner
        return TextureCase(blob, np.stack([xz[:, 0], np.zeros(len(xz)), xz[:, 1]], -1), np.zeros(len(xz), np.int64), classes=classes)
    setups = {"noise_scale4_near": (noise(4.0), 4.0, 2.0 ** -8, 21), "noise_scale005_far": (noise(0.05), 552.0, 2.0 ** -4, 22),
              "noise_scale4_far": (noise(4.0), 552.0, 2.0 ** -4, 23), "checker_constants": (chk_const, 4.0, 2.0 ** -8, 24),
              "checker_noise_image": (chk_nested, 4.0, 2.0 ** -8, 25)}
    out = {name: (lambda name=name, a=a: strips(name, *a)) for name, a in setups.items()}
    out["image"] = image_case
    return out


DIRECTION_CASES = {
    "mirror_above": lambda: _direction_case(abi.MAT_METAL, None, -1.0),
    "mirror_above_long": lambda: _direction_case(abi.MAT_METAL, None, -1.0, scale=4.0),  # |d| up to 66: Q5 changes nothing at fuzz 0
    "mirror_xformed": lambda: _direction_case(abi.MAT_METAL, None, -1.0, xformed=True),
    "glass_above": lambda: _direction_case(abi.MAT_DIELECTRIC, ETA, -1.0),
    "glass_below": lambda: _direction_case(abi.MAT_DIELECTRIC, ETA, 1.0),
    "glass_below_flipped": lambda: _direction_case(abi.MAT_DIELECTRIC, ETA, 1.0, flip=1),  # from below a flipped face is the front
    "glass_xformed": lambda: _direction_case(abi.MAT_DIELECTRIC, ETA, -1.0, xformed=True),
    "glass_share_below": lambda: DirectionCase(surface_scene(abi.MAT_DIELECTRIC, fuzz_or_eta=ETA), (-0.75, -1.0, -0.25), (0.75, 1.0, 0.25), (0.0, 1.0, 0.0), ETA, N_STAT),
    "glass_share": lambda: DirectionCase(surface_scene(abi.MAT_DIELECTRIC, fuzz_or_eta=ETA), (-0.5, 1.0, -0.25), (0.5, -1.0, 0.25), (0.0, 1.0, 0.0), ETA, N_STAT),
}
LAMBERT_CASES = {
    "normal_up": lambda: _lambert_case(1, 0, (-0.5, 1.0, -0.25), (0.5, -1.0, 0.25), "normal"),
    "normal_flipped": lambda: _lambert_case(1, 1, (-0.5, 1.0, -0.25), (0.5, -1.0, 0.25), "normal"),  # scatters about n = -y: below the plane
    "normal_xformed": lambda: _lambert_case(1, 0, (0.5, 1.5, -3.25), (0.5, -1.0, 0.25), "normal", xformed=True),
    "tangent_x": lambda: _lambert_case(0, 0, (1.0, 0.5, 0.25), (-1.0, -0.5, -0.25), "tangent"),   # |w.x| > 0.9: the basis' other branch
    "tangent_minus_x": lambda: _lambert_case(0, 1, (1.0, 0.5, 0.25), (-1.0, -0.5, -0.25), "tangent"),
    "tangent_z": lambda: _lambert_case(2, 0, (0.5, 0.25, 1.0), (-0.5, -0.25, -1.0), "tangent"),
    "tangent_minus_z": lambda: _lambert_case(2, 1, (0.5, 0.25, 1.0), (-0.5, -0.25, -1.0), "tangent"),
}
FUZZ_CASES = {
    "normal_incidence": lambda: _fuzz_case((0.0, -2.0, 0.0)),       # effective fuzz 0.25 / 0.5
    "oblique": lambda: _fuzz_case((1.0, -1.0, 0.5)),                # |d| = 1.5: 1/3 / 0.5, no cancels (cos_a = 2/3)
    "grazing": lambda: _fuzz_case((1.0, -0.25, 0.0)),               # cos_a = 0.2425: both estimators cancel
}
SLAB_CASES = {"slab": SlabCase}
MEDIA_CASES = {
    "box_normal": lambda: MediaCase(media_scene([BOX]), (0.0, 5.0, 0.0), (0.0, -1.0, 0.0)),
    "box_unnormalised": lambda: MediaCase(media_scene([BOX]), (0.0, 5.0, 0.0), (0.0, -2.0, 0.0)),
    "box_oblique": lambda: MediaCase(media_scene([BOX]), (-3.0, 5.0, 0.0), (0.75, -1.0, 0.0)),
    "sphere_centre": lambda: MediaCase(media_scene([BALL]), (0.0, 6.0, 0.0), (0.0, -2.0, 0.0)),
    "sphere_off_centre": lambda: MediaCase(media_scene([BALL]), (0.875, 6.0, 0.25), (0.0, -1.0, 0.0)),
    "sphere_oblique": lambda: MediaCase(media_scene([BALL]), (-2.0, 6.0, 0.5), (0.75, -1.0, 0.0)),
    "box_origin_inside": lambda: MediaCase(media_scene([BOX]), (0.0, 2.5, 0.0), (0.0, -1.0, 0.0)),
    "sphere_origin_inside": lambda: MediaCase(media_scene([BALL]), (0.25, 3.5, 0.0), (0.75, -1.0, 0.0)),
    # |d| = 2^20 / 1024: the estimator's start distance (1e-6 / 1e-3) lies about one unit into the box
    "box_tmin_inside_reference": lambda: MediaCase(media_scene([BOX]), (0.0, 3.5, 0.0), (0.0, -2.0 ** 20, 0.0), estimators=(REF,)),
    "box_tmin_inside_corrected": lambda: MediaCase(media_scene([BOX]), (0.0, 3.5, 0.0), (0.0, -1024.0, 0.0), estimators=MediaCase.estimators[1:]),
    "box_xformed": lambda: MediaCase(media_scene([("box", (-4.0, 1.0, -3.0, 4.0, 3.0, 3.0), 0.4)], xformed=True), (2.0, 6.0, -1.5), (0.5, -1.0, -0.25)),
    "two_media": lambda: MediaCase(media_scene([BOX, ("sphere", (0.0, 6.0, 0.0, 1.5), 0.25)]), (0.5, 9.0, 0.0), (0.0, -1.0, 0.0),
                                   estimators=MediaCase.estimators[1:]),
}
EMITTER_CASES = {
    "light": lambda: EmitterCase(abi.MAT_DIFFUSE_LIGHT, 0, (0.25, 0.5, 0.75)),
    "light_flipped": lambda: EmitterCase(abi.MAT_DIFFUSE_LIGHT, 1, (0.25, 0.5, 0.75)),
    "normal_material": lambda: EmitterCase(abi.MAT_NORMAL, 0, None),
}
TEXTURE_CASES = _texture_cases()
# the same textures on 32 points each, for the entries that take one ray per call (rtw_render of the ray's own blob)
TEXTURE_SUBSETS = {name: (lambda name=name: case("texture-" + name).subset()) for name in TEXTURE_CASES}
CASES = {}
for _family, _cases in (("direction", DIRECTION_CASES), ("lambert", LAMBERT_CASES), ("fuzz", FUZZ_CASES), ("slab", SLAB_CASES),
                        ("media", MEDIA_CASES), ("emitter", EMITTER_CASES), ("texture", TEXTURE_CASES), ("texture32", TEXTURE_SUBSETS)):
    CASES.update({f"{_family}-{k}": v for k, v in _cases.items()})
COUNTS = ()  # check takes the samples alone
case, check = C.registry(CASES, "{name}: ")


def oracle_samples(name, rng_kind, estimator, seed, key_base=0):
    """(m, keys_per_ray, 3) float32: the oracle's samples of case `name`, computed once and left unchanged."""
    return C.oracle_samples(case(name), rng_kind, estimator, seed, key_base).samples


# ---------------------------------------------------------------- the measurement behind the MEASURED_CONSTANT_* values
def measure_constants(verbose=False):
    """{name: constant}: this file at float32 against itself at float64 over the inputs of the tests, in the stated units."""
    mir = refr = 0.0
    for name in DIRECTION_CASES:
        c = case("direction-" + name)
        for est in c.estimators:
            a, b = c.fp32_constants(est)
            if verbose:
                print(f"direction-{name:22s} estimator {est}: mirror {a:.4f}  refraction {b:.4f}")
            mir, refr = max(mir, a), max(refr, b)
    image, noise = 0.0, {}
    for name in TEXTURE_CASES:
        ks = case("texture-" + name).fp32_constants()
        if verbose:
            print(f"texture-{name:24s} " + "  ".join(f"{ {abi.TEX_CONSTANT: 'constant', abi.TEX_NOISE: 'noise', abi.TEX_IMAGE: 'image'}[k]} {v:.4f}" for k, v in ks.items()))
        assert ks.get(abi.TEX_CONSTANT, 0.0) == 0.0  # a constant's value is copied at either precision
        image = max(image, ks.get(abi.TEX_IMAGE, 0.0))
        if abi.TEX_NOISE in ks:
            noise[name] = ks[abi.TEX_NOISE]
    return {"MIRROR": mir, "REFRACT": refr, "NOISE": noise, "IMAGE": image}


def quadrature_errors():
    """What the quadratures of the statistical laws are worth: each against a closed form or against itself at twice the nodes."""
    y = np.linspace(-1.0, 1.0, 4001)
    out = {"tangent, cosine lobe: quadrature - semicircle law": float(np.abs(lambert_tangent_cdf(y, False) - semicircle_cdf(y)).max()),
           "tangent, reference lobe: 96 nodes - 192 nodes": float(np.abs(lambert_tangent_cdf(y, True) - lambert_tangent_cdf(y, True, 192)).max())}
    for name in FUZZ_CASES:
        c = case("fuzz-" + name)
        for est in c.estimators:
            law = c.law(est)
            fine = FuzzLaw(law.cos_a, law.f, grid=8193, nodes=16384)
            x = np.linspace(law.x[0], law.x[-1], 20001)
            out[f"fuzz-{name}, estimator {est}: table - table at twice the grid and nodes"] = float(np.abs(law.cdf(x) - fine.cdf(x)).max())
            out[f"fuzz-{name}, estimator {est}: mass and cap"] = law.quadrature_error
    return out


if __name__ == "__main__":
    for k_, v_ in measure_constants(verbose=True).items():
        print(f"MEASURED_CONSTANT_{k_} = " + (f"{v_:.4f}" if isinstance(v_, float) else str({n_: round(c_, 4) for n_, c_ in v_.items()})))
    for k_, v_ in quadrature_errors().items():
        print(f"{k_}: {v_:.2e}")
