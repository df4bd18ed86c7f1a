// rtw_math.h - short, bit-identical forms of the correctly rounded fp32 reciprocal and square root.
//
// The arithmetic spec wants IEEE results for 1.0f / x and sqrtf(x). The compiler's correctly rounded expansions on gfx950 are 11
// and 16 VALU instructions, most of them for inputs a renderer almost never sees (denormals, huge and tiny exponents, zero,
// infinity). Each function here is: a range test; where EVERY active lane of the wave passes it, a hardware approximation
// refined with explicit fused multiply-adds; otherwise the compiler's own form for the whole wave. Outside the window the
// old code runs, so those inputs keep their bits by construction; inside it, equality with the compiler's form is proved by
// trying every input (tests/test_gpu_math_forms.py on the hardware, tests/test_math_forms_cpu.py on a host model of it).
//
// No includes: the primitives come from the policy P, so that the same text compiles with g++ against a host model.
//   P::rcp(x)  ~ 1/x        within 1 ulp (v_rcp_f32)      P::fma(a, b, c)  one rounding
//   P::rsq(x)  ~ 1/sqrt(x)  within 1 ulp (v_rsq_f32)      P::all(ok)       true when ok holds on every active lane of the wave
#pragma once

#ifndef RTW_MATH_FN
#define RTW_MATH_FN inline
#endif
// Refinement steps of the reciprocal (1 or 2) and form of the root (0 = the residual step alone, 1 = a coupled step before it).
// Shipped: the shortest ones, 3 and 5 instructions. They are exact because of what v_rcp_f32 and v_rsq_f32 return on gfx950, input
// by input - the exhaustive sweep shows 0 differing results for them and for the longer forms alike. A host model that only
// knows "within 1 ulp" needs the longer forms (and for the reciprocal still fails at the all-ones significand, from any start
// but the correctly rounded one): should another device ever fail the sweep, these two switches are the first thing to try.
#ifndef RTW_RCP_STEPS
#define RTW_RCP_STEPS 1
#endif
#ifndef RTW_SQRT_COUPLED
#define RTW_SQRT_COUPLED 0
#endif

namespace rtwmath {

// The window: 2^-64 <= |x| <= 2^64. A reciprocal, a root and the reciprocal of a root of such an x are inside it again, and
// no intermediate of the short forms (the residuals are about 2^-24 and 2^-48 of their operands) leaves the normal range.
#define RTW_MATH_LO 5.42101086242752217e-20f  // 2^-64
#define RTW_MATH_HI 1.8446744073709551616e19f  // 2^64

// (false for NaN)
RTW_MATH_FN bool rcp_window(float x) { const float a = __builtin_fabsf(x); return a >= RTW_MATH_LO && a <= RTW_MATH_HI; }
RTW_MATH_FN bool sqrt_window(float x) { return x >= RTW_MATH_LO && x <= RTW_MATH_HI; }
// one test for three: the largest and the smallest magnitude (v_max3_f32 / v_min3_f32). A NaN component is not seen by
// max / min; it gives NaN in the short form and in the compiler's alike.
RTW_MATH_FN bool rcp_window3(float x, float y, float z) {
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y), az = __builtin_fabsf(z);
    const float hi = __builtin_fmaxf(__builtin_fmaxf(ax, ay), az), lo = __builtin_fminf(__builtin_fminf(ax, ay), az);
    return lo >= RTW_MATH_LO && hi <= RTW_MATH_HI;
}

// Newton steps on r ~ 1/x from a start r0 within 2 ulp: r += r * (1 - x * r), the residual exact in the fma.
template <class P, int STEPS>
RTW_MATH_FN float rcp_refine(float x, float r) {
    float e = P::fma(-x, r, 1.0f);
    r = P::fma(e, r, r);
    if (STEPS == 2) {
        e = P::fma(-x, r, 1.0f);
        r = P::fma(e, r, r);
    }
    return r;
}
template <class P, int STEPS = RTW_RCP_STEPS>
RTW_MATH_FN float rcp_short(float x) { return rcp_refine<P, STEPS>(x, P::rcp(x)); }

// g ~ sqrt(x), h ~ 1 / (2 sqrt(x)) from the reciprocal root; optionally one coupled Goldschmidt step on both; then the residual
// x - g * g (exact in the fma) corrects g. (Without the coupled step a start displaced by an ulp misses 14 to 24 of the host
// model's inputs; the hardware's own starts miss none.)
template <class P, int COUPLED = RTW_SQRT_COUPLED>
RTW_MATH_FN float sqrt_short(float x) {
    const float r = P::rsq(x);
    float g = x * r;
    float h = 0.5f * r;
    if (COUPLED) {
        const float e = P::fma(-h, g, 0.5f);
        g = P::fma(g, e, g);
        h = P::fma(h, e, h);
    }
    const float d = P::fma(-g, g, x);
    return P::fma(d, h, g);
}

// 1.0f / x
template <class P>
RTW_MATH_FN float rcp(float x) {
    if (__builtin_expect(P::all(rcp_window(x)), 1)) return rcp_short<P>(x);
    return 1.0f / x;
}
// sqrtf(x)
template <class P>
RTW_MATH_FN float sqrt(float x) {
    if (__builtin_expect(P::all(sqrt_window(x)), 1)) return sqrt_short<P>(x);
    return __builtin_sqrtf(x);
}
// sqrtf(x) where the code around it bounds x inside the window: no test
template <class P>
RTW_MATH_FN float sqrt_inside(float x) { return sqrt_short<P>(x); }
// 1.0f / sqrtf(x), two roundings like the expression; the root of an x inside the window is inside it too: one test.
// (Refining 1 / g from 2 h instead of a second hardware approximation misses where g has the all-ones significand: the
// Newton step from 0.5 lands on the tie below the true quotient. v_rcp_f32 returns the start above it there.)
template <class P>
RTW_MATH_FN float rcp_sqrt_short(float x) { return rcp_short<P>(sqrt_short<P>(x)); }
template <class P>
RTW_MATH_FN float rcp_sqrt(float x) {
    if (__builtin_expect(P::all(sqrt_window(x)), 1)) return rcp_sqrt_short<P>(x);
    return 1.0f / __builtin_sqrtf(x);
}
// root = sqrtf(x) and inv = 1.0f / root, the length of a vector and the factor that normalises it: one test for both, by the
// argument of rcp_sqrt (the root of an x inside the window is inside it). The sequences are sqrt's and rcp's own.
template <class P>
RTW_MATH_FN void sqrt_rcp(float x, float& root, float& inv) {
    if (__builtin_expect(P::all(sqrt_window(x)), 1)) {
        root = sqrt_short<P>(x);
        inv = rcp_short<P>(root);
    } else {
        root = __builtin_sqrtf(x);
        inv = 1.0f / root;
    }
}
// (1/x, 1/y, 1/z) in place, one test
template <class P>
RTW_MATH_FN void rcp3(float& x, float& y, float& z) {
    if (__builtin_expect(P::all(rcp_window3(x, y, z)), 1)) {
        x = rcp_short<P>(x); y = rcp_short<P>(y); z = rcp_short<P>(z);
    } else {
        x = 1.0f / x; y = 1.0f / y; z = 1.0f / z;
    }
}

}  // namespace rtwmath
