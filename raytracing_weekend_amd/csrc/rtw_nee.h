// rtw_nee.h - the light sample of k_path's one-light instantiation as straight-line code (DESIGN.md 4.1 "The one-light sample is
// straight-line code"; rtw_kernels.h shade_a, NEE1).
//
// shade_a's generic text nests four divergent tests (ldist > 1e-6, costa > 1e-6, lpdf > 0 && bsdf_eval == 0, 0 < bpdf && f != 0) and
// gives every result a default. On gfx950 each level costs a saveexec / branch pair and, in front of it, moves that re-materialise the
// defaults of everything the level may leave untouched. Nothing reads those defaults: k_path looks at dir, tmin, tmax and rad only
// under `has`. Here the same operations run in the same order for every lane that reaches the sample, with no control flow between
// them, and the four tests are combined into `has` at the end. A lane that fails a test computes values nobody reads (a division
// by zero, a NaN: no traps in fp32 arithmetic here).
//
// Like rtw_math.h: no HIP in here, the primitives come from the policy P (P::fma, P::rcp, P::rsq, P::all), vectors are any type V3
// with float members x, y, z, so that tests/native/nee_flat_check.cpp compiles the same text with g++ (-ffp-contract=off) beside a
// transcription of the nested form.
#pragma once
#include "../../include/rtw.h"
#include "rtw_math.h"

// 1: k_path<..., NEE1 = 1> takes its light sample through rect_sample_flat and sets the Lambertian vertex's event with a select;
// 0: those instantiations keep shade_a's nested text (the instruction stream they had without this header), for A/B runs
#ifndef RTW_PATH_FLAT_NEE
#define RTW_PATH_FLAT_NEE 1
#endif

namespace rtwnee {

template <class P, class V3>
RTW_MATH_FN float dot(V3 a, V3 b) { return P::fma(a.z, b.z, P::fma(a.y, b.y, a.x * b.x)); }

// One point on the listed rectangle (pdf/rectPdf.cu:124-193), the Lambertian's value and density towards it
// (lambertianMaterial.cu:74-81), the power-heuristic weight (raydata.cuh:167-171) and the probe's interval (closehit.cu:95-113),
// under the reference estimator with one listed light.
//   ra, rb        the two draws            rc0 .. rc4   the rectangle: [rc0, rc1] x [rc2, rc3] at rc4 on the axis
//   gen           RTW_PDF_RECT_X / _Y, anything else is Z (wave-uniform on the device)
//   lnrm, lemi, larea   the light's normal, emission (used unscaled: one light) and area
//   so, hn, att   the vertex, its normal and albedo         bsdf_eval   the hit record's flag (0: the material has a value)
//   eps           the probe's offset
// Returns `has`. dir, tmin, tmax and rad are what shade_a's nested text gives when has holds, bit for bit; when it does not hold
// they are UNSPECIFIED (the nested text leaves its defaults there), and the caller must not read them.
template <class P, class V3>
RTW_MATH_FN bool rect_sample_flat(const float ra, const float rb, const float rc0, const float rc1, const float rc2, const float rc3,
                                  const float rc4, const int gen, const V3 lnrm, const V3 lemi, const float larea, const V3 so, const V3 hn,
                                  const V3 att, const int bsdf_eval, const float eps, V3& dir, float& tmin, float& tmax, V3& rad) {
    const bool on_x = gen == RTW_PDF_RECT_X, on_y = gen == RTW_PDF_RECT_Y;
    const float pa = P::fma(ra, rc1 - rc0, rc0);
    const float pb = P::fma(rb, rc3 - rc2, rc2);
    // X: (k, pa, pb)   Y: (pa, k, pb)   Z: (pa, pb, k). Branches on the wave-uniform axis, on purpose: as selects on the two scalar
    // conditions they save 3 VALU instructions and 6 branches, and the hot instantiation's scratch grows from 28 to 32 B
    V3 ldir;
    if (on_x) { ldir.x = rc4 - so.x; ldir.y = pa - so.y; ldir.z = pb - so.z; }
    else if (on_y) { ldir.x = pa - so.x; ldir.y = rc4 - so.y; ldir.z = pb - so.z; }
    else { ldir.x = pa - so.x; ldir.y = pb - so.y; ldir.z = rc4 - so.z; }
    float ldist, inv;
    rtwmath::sqrt_rcp<P>(dot<P>(ldir, ldir), ldist, inv);  // length3 and rcp_ behind one range test
    ldir.x *= inv; ldir.y *= inv; ldir.z *= inv;
    V3 nl;
    nl.x = -ldir.x; nl.y = -ldir.y; nl.z = -ldir.z;
    const float costa = dot<P>(nl, lnrm);
    const float lpdf = (ldist * ldist) / (larea * costa);
    V3 f;
    f.x = att.x * 0.318309886183790671538f; f.y = att.y * 0.318309886183790671538f; f.z = att.z * 0.318309886183790671538f;
    const float ndl = dot<P>(ldir, hn);
    const float bpdf = __builtin_fmaxf(0.0f, ndl * 0.318309886183790671538f);
    const float a2 = lpdf * lpdf;
    const float weight = a2 / P::fma(bpdf, bpdf, a2);
    const float k = (weight * ndl) / lpdf;
    dir = ldir;
    tmin = eps;
    tmax = ldist - eps;
    rad.x = (f.x * lemi.x) * k; rad.y = (f.y * lemi.y) * k; rad.z = (f.z * lemi.z) * k;
    return (ldist > 1.0e-6f) & (costa > 1.0e-6f) & (lpdf > 0.0f) & (bsdf_eval == 0) & (0.0f < bpdf) &
           ((f.x != 0.0f) | (f.y != 0.0f) | (f.z != 0.0f));
}

}  // namespace rtwnee
