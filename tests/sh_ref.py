"""Helper of the spherical-harmonic probe tests (include/rtw.h rtw_probe_sh), not a test: the direction and the basis of every
sample, restated.

directions() and basis() write the header's formulas in numpy float32 arithmetic: probe_ref.uniforms (the two raygen uniforms from
the oracle's exported generators), the oracle's rtwo_sincos2pi and probe_ref.fma (libm's fmaf) for the one fused step. Sample s of
point i is then, by the contract, the rtw_radiance sample of ray (p_i, directions[i, s], tmin, tmax) with the same key and sample
index, weighted by basis(directions[i, s]): the GPU tests referee rtw_probe_sh with rtw_radiance, which the oracle referees bit for
bit. The sums are radiance_ref.sum_in_order's, each of the 27 on its own."""
import ctypes as C

import numpy as np

import oracle
import probe_ref as P
import radiance_ref as R
from raytracing_weekend_amd import abi

FOUR_PI = np.float32(12.5663706)  # the float nearest 4 pi
K0, K1, K2, K3, K4 = (np.float32(v) for v in (0.282094792, 0.488602512, 1.092548431, 0.315391565, 0.546274215))


def parts(n, spp, seed=0x6314759, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, key_offset=0):
    """(r2, z, s2, d): the second uniform, z = 1 - 2 r2, s2 = fma(-z, z, 1) and the (n, spp, 3) float32 directions of sample s of
    point i (rtw.h rtw_probe_sh, "Direction"); the points themselves do not enter."""
    lib = oracle.load()
    r1, r2 = np.empty((n, spp), np.float32), np.empty((n, spp), np.float32)
    sn, cs = np.empty((n, spp), np.float32), np.empty((n, spp), np.float32)
    s_, c_ = C.c_float(), C.c_float()
    for i in range(n):
        key = (key_offset + i) & 0xffffffff
        for s in range(spp):
            r1[i, s], r2[i, s] = P.uniforms(key, sample_offset + s, seed, rng_kind)
            lib.rtwo_sincos2pi(C.c_float(r1[i, s]), C.byref(s_), C.byref(c_))
            sn[i, s], cs[i, s] = s_.value, c_.value
    z = np.float32(1.0) - np.float32(2.0) * r2
    s2 = P.fma(-z, z, np.float32(1.0))
    sq = np.sqrt(s2)
    return r2, z, s2, np.stack([cs * sq, sn * sq, z], axis=-1).astype(np.float32)


def directions(n, spp, seed=0x6314759, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, key_offset=0):
    return parts(n, spp, seed, rng_kind, sample_offset, key_offset)[3]


def basis(d):
    """(..., 9) float32: the nine basis values at (..., 3) float32 directions, one rounding per operation, parenthesised as the header
    writes them."""
    d = np.asarray(d, np.float32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full(x.shape, K0, np.float32), K1 * y, K1 * z, K1 * x, K2 * (x * y), K2 * (y * z),
                     K3 * (np.float32(3.0) * (z * z) - np.float32(1.0)), K2 * (x * z), K4 * ((x * x) - (y * y))], axis=-1).astype(np.float32)


def rays_of(points, dirs, s):
    """The (n, 8) rays of sample s: the points with floats 3..5 replaced by directions[:, s]."""
    return P.rays_of(points, dirs, s)


def project(samples, dirs, spp):
    """(n, 9, 4) float32 expected coefficients from (spp, n, 3) float32 sample radiances and (n, spp, 3) directions: Y_j * L_c in
    float32, radiance_ref.sum_in_order (which divides by spp), times the float nearest 4 pi; w = 0."""
    n = dirs.shape[0]
    y = basis(dirs)  # (n, spp, 9)
    out = np.zeros((n, 9, 4), np.float32)
    for i in range(n):
        for j in range(9):
            out[i, j, :3] = R.sum_in_order((y[i, :, j, None] * samples[:, i, :3]).astype(np.float32), spp) * FOUR_PI
    return out
