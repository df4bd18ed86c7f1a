// CPU check of raytracing_weekend_amd/csrc/rtw_nee.h: the straight-line light sample of k_path's one-light instantiation beside a
// literal transcription of shade_a's nested form with its defaults (rtw_kernels.h, the lines for rectPdf.cu:124-193,
// lambertianMaterial.cu:74-81 and closehit.cu:95-113). Run by tests/test_nee_flat_cpu.py. Compile with -ffp-contract=off: every
// fusion is written out. The hardware approximations are modelled by their correctly rounded values, from which rtw_math.h's
// short forms are exact (tests/test_math_forms_cpu.py), so both sides compute 1.0f / x and sqrtf(x).
//
// Inputs: about 10^6 seeded random vertices around the Cornell box's light, on each of the three axes; and every edge below,
// singly and in pairs, on each axis: a distance of 0, of 1e-6 and its neighbours; costa of +0, -0, 1e-6 and its neighbour, negative;
// an area of 0, inf, NaN, negative (lpdf inf, 0, NaN, negative); ndl negative and zero; albedos with every pattern of 0 and -0
// channels; bsdf_eval 1 and -1; NaN and inf in the vertex; oblique directions.
// Asserts: `has` is equal everywhere, and where it holds dir, tmin, tmax and rad are equal bit for bit. The program also checks that
// the edges it names were met (a distance of exactly 1e-6, a costa of exactly +0, ...), and that a control - the straight-line form
// with one & of the predicate replaced by | - is rejected by the same inputs.
// Prints "nee_flat_check ok ..." and returns 0, or the first mismatch and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <vector>

#include "../../raytracing_weekend_amd/csrc/rtw_nee.h"

struct v3 { float x, y, z; };
static v3 V(float x, float y, float z) { v3 r; r.x = x; r.y = y; r.z = z; return r; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float up(float f) { return std::nextafterf(f, std::numeric_limits<float>::infinity()); }
static float down(float f) { return std::nextafterf(f, -std::numeric_limits<float>::infinity()); }

struct Host {
    static float rcp(float x) { return 1.0f / x; }
    static float rsq(float x) { return (float)(1.0L / sqrtl((long double)x)); }
    static float fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
    static bool all(bool ok) { return ok; }
};

// rtw_device.h's vector functions, as the nested form calls them
static float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
static v3 vsub(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static v3 vmul(v3 a, v3 b) { return V(a.x * b.x, a.y * b.y, a.z * b.z); }
static v3 vscale(v3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
static v3 vneg(v3 a) { return V(-a.x, -a.y, -a.z); }
static float dot3(v3 a, v3 b) { return fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)); }
static float rcp_(float x) { return rtwmath::rcp<Host>(x); }
static float sqrt_(float x) { return rtwmath::sqrt<Host>(x); }
static float length3(v3 a) { return sqrt_(dot3(a, a)); }
#define RTW_1_PI_F 0.318309886183790671538f

struct In {
    float ra, rb, rc[5];
    int gen;
    v3 lnrm, lemi;
    float larea;
    v3 so, hn, att;
    int bsdf_eval;
    float eps;
};
struct Nee {
    bool has;
    v3 dir, rad;
    float tmin, tmax;
};

// shade_a's text for one listed light under the reference estimator (NEE1: nl = 1, lem = lemi)
static Nee nested(const In& in, float* seen = nullptr) {
    Nee nee;
    nee.has = false;
    nee.dir = V(0.f, 0.f, 0.f); nee.rad = V(0.f, 0.f, 0.f); nee.tmin = 0.f; nee.tmax = -1.f;
    const v3 so = in.so, hn = in.hn, att = in.att, lnrm = in.lnrm, lemi = in.lemi;
    const float larea = in.larea, rc0 = in.rc[0], rc1 = in.rc[1], rc2 = in.rc[2], rc3 = in.rc[3], rc4 = in.rc[4];
    const int gen = in.gen;
    float lpdf = 0.0f, ldist = 0.0f, costa_seen = std::numeric_limits<float>::quiet_NaN();
    v3 ldir = V(0.f, 0.f, 0.f), lem = V(0.f, 0.f, 0.f);
    {
        float ra = in.ra, rb = in.rb;
        float pa = fma_(ra, rc1 - rc0, rc0);
        float pb = fma_(rb, rc3 - rc2, rc2);
        float k = rc4;
        v3 rp = (gen == RTW_PDF_RECT_X) ? V(k, pa, pb) : (gen == RTW_PDF_RECT_Y) ? V(pa, k, pb) : V(pa, pb, k);
        ldir = vsub(rp, so);
        ldist = length3(ldir);
        if (ldist > 1.0e-6f) {
            ldir = vscale(ldir, rcp_(ldist));
            float costa = dot3(vneg(ldir), lnrm);
            costa_seen = costa;
            if (costa > 1.0e-6f) {
                lem = lemi;
                lpdf = (ldist * ldist) / (larea * costa);
            }
        }
    }
    if (seen) { seen[0] = ldist; seen[1] = costa_seen; seen[2] = lpdf; }
    if (lpdf > 0.0f && in.bsdf_eval == 0) {
        v3 f = vscale(att, RTW_1_PI_F);
        float ndl = dot3(ldir, hn);
        float bpdf = __builtin_fmaxf(0.0f, ndl * RTW_1_PI_F);
        if (seen) seen[3] = ndl;
        if (0.0f < bpdf && (f.x != 0.0f || f.y != 0.0f || f.z != 0.0f)) {
            const float eps = in.eps;
            float a2 = lpdf * lpdf;
            float weight = a2 / fma_(bpdf, bpdf, a2);
            float k = (weight * ndl) / lpdf;
            nee.has = true;
            nee.dir = ldir;
            nee.tmin = eps;
            nee.tmax = ldist - eps;
            nee.rad = vscale(vmul(f, lem), k);
        }
    }
    return nee;
}

static Nee flat(const In& in) {
    Nee nee;
    nee.has = rtwnee::rect_sample_flat<Host>(in.ra, in.rb, in.rc[0], in.rc[1], in.rc[2], in.rc[3], in.rc[4], in.gen, in.lnrm, in.lemi, in.larea,
                                             in.so, in.hn, in.att, in.bsdf_eval, in.eps, nee.dir, nee.tmin, nee.tmax, nee.rad);
    return nee;
}

// the negative control: the header's outputs under a predicate whose first & is an | (a vertex whose costa fails and whose
// distance passes then has a sample)
static Nee control(const In& in) {
    Nee nee = flat(in);
    const float pa = fma_(in.ra, in.rc[1] - in.rc[0], in.rc[0]), pb = fma_(in.rb, in.rc[3] - in.rc[2], in.rc[2]), k = in.rc[4];
    const v3 rp = (in.gen == RTW_PDF_RECT_X) ? V(k, pa, pb) : (in.gen == RTW_PDF_RECT_Y) ? V(pa, k, pb) : V(pa, pb, k);
    v3 ldir = vsub(rp, in.so);
    const float ldist = length3(ldir);
    ldir = vscale(ldir, 1.0f / ldist);
    const float costa = dot3(vneg(ldir), in.lnrm);
    const float lpdf = (ldist * ldist) / (in.larea * costa);
    const v3 f = vscale(in.att, RTW_1_PI_F);
    const float bpdf = __builtin_fmaxf(0.0f, dot3(ldir, in.hn) * RTW_1_PI_F);
    nee.has = ((ldist > 1.0e-6f) | (costa > 1.0e-6f)) & (lpdf > 0.0f) & (in.bsdf_eval == 0) & (0.0f < bpdf) &
              ((f.x != 0.0f) | (f.y != 0.0f) | (f.z != 0.0f));
    return nee;
}

static bool same(const Nee& a, const Nee& b) {
    if (a.has != b.has) return false;
    if (!a.has) return true;
    const float fa[8] = {a.dir.x, a.dir.y, a.dir.z, a.rad.x, a.rad.y, a.rad.z, a.tmin, a.tmax};
    const float fb[8] = {b.dir.x, b.dir.y, b.dir.z, b.rad.x, b.rad.y, b.rad.z, b.tmin, b.tmax};
    for (int i = 0; i < 8; i++)
        if (bits(fa[i]) != bits(fb[i])) return false;
    return true;
}

static void print_case(const char* what, const In& in, const Nee& a, const Nee& b) {
    printf("%s: gen %d ra %a rb %a rect %a %a %a %a %a so %a %a %a hn %a %a %a att %a %a %a lnrm %a %a %a larea %a bsdf_eval %d\n", what, in.gen,
           in.ra, in.rb, in.rc[0], in.rc[1], in.rc[2], in.rc[3], in.rc[4], in.so.x, in.so.y, in.so.z, in.hn.x, in.hn.y, in.hn.z, in.att.x, in.att.y,
           in.att.z, in.lnrm.x, in.lnrm.y, in.lnrm.z, in.larea, in.bsdf_eval);
    printf("  nested: has %d dir %a %a %a rad %a %a %a t %a %a\n  flat:   has %d dir %a %a %a rad %a %a %a t %a %a\n", a.has, a.dir.x, a.dir.y,
           a.dir.z, a.rad.x, a.rad.y, a.rad.z, a.tmin, a.tmax, b.has, b.dir.x, b.dir.y, b.dir.z, b.rad.x, b.rad.y, b.rad.z, b.tmin, b.tmax);
}

// An input in the rectangle's own frame - (u, v) along its edges, w along its axis - placed on the axis of `gen`:
// X: (w, u, v)   Y: (u, w, v)   Z: (u, v, w), the orders of rectPdf.cu's three generators.
struct Local {
    float ra, rb, rc[5];
    v3 so, hn, lnrm, att;  // so, hn, lnrm as (u, v, w)
    float larea;
    int bsdf_eval;
};
static v3 placed(int gen, v3 l) { return gen == RTW_PDF_RECT_X ? V(l.z, l.x, l.y) : gen == RTW_PDF_RECT_Y ? V(l.x, l.z, l.y) : l; }
static In placed(int gen, const Local& l) {
    In in;
    in.ra = l.ra; in.rb = l.rb;
    for (int i = 0; i < 5; i++) in.rc[i] = l.rc[i];
    in.gen = gen;
    in.lnrm = placed(gen, l.lnrm); in.so = placed(gen, l.so); in.hn = placed(gen, l.hn);
    in.lemi = V(4.f, 2.f, 1.f);
    in.larea = l.larea;
    in.att = l.att;
    in.bsdf_eval = l.bsdf_eval;
    in.eps = 5.0e-5f;
    return in;
}
// the point (0, 0) of the rectangle [0, 2] x [0, 1.5] at w = 2, seen from one unit below it by a surface that faces it
static Local base() {
    Local l;
    l.ra = 0.f; l.rb = 0.f;
    l.rc[0] = 0.f; l.rc[1] = 2.f; l.rc[2] = 0.f; l.rc[3] = 1.5f; l.rc[4] = 2.f;
    l.so = V(0.f, 0.f, 1.f); l.hn = V(0.f, 0.f, 1.f); l.lnrm = V(0.f, 0.f, -1.f); l.att = V(0.5f, 0.25f, 1.0f);
    l.larea = 3.f;
    l.bsdf_eval = 0;
    return l;
}

struct Seen {
    uint64_t n = 0, has = 0, dist0 = 0, dist_at = 0, dist_up = 0, costa_p0 = 0, costa_m0 = 0, costa_at = 0, costa_neg = 0, lpdf_inf = 0, lpdf_nan = 0,
             lpdf_0 = 0, ndl_le0 = 0;
};

int main() {
    typedef std::function<void(Local&)> Edit;
    std::vector<Edit> edits;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the distance: the vertex on the sampled point; the plane at 0 and the vertex d below it, so that the difference is d exactly
    edits.push_back([](Local& l) { l.so = V(0.f, 0.f, l.rc[4]); });
    for (float d : {1.0e-6f, up(1.0e-6f), down(1.0e-6f), up(up(1.0e-6f))})
        edits.push_back([d](Local& l) { l.rc[4] = 0.f; l.so = V(0.f, 0.f, -d); });
    // costa = -lnrm.w for a direction along the axis
    for (float w : {-0.0f, 0.0f, -1.0e-6f, -up(1.0e-6f), -down(1.0e-6f), 1.0f, 1.0e-6f})
        edits.push_back([w](Local& l) { l.lnrm.z = w; });
    for (float a : {0.0f, -0.0f, inf, -inf, nan, -3.0f, 1.0e-30f, 1.0e30f})
        edits.push_back([a](Local& l) { l.larea = a; });
    // ndl: a surface that faces away, one that sees the light edge-on
    edits.push_back([](Local& l) { l.hn = V(0.f, 0.f, -1.f); });
    edits.push_back([](Local& l) { l.hn = V(1.f, 0.f, 0.f); });
    edits.push_back([](Local& l) { l.hn = V(0.f, 1.f, -0.0f); });
    // albedos: every pattern of 0.5, 0 and -0 but the plain one
    const float ch[3] = {0.5f, 0.0f, -0.0f};
    for (int i = 1; i < 27; i++)
        edits.push_back([=](Local& l) { l.att = V(ch[i % 3], ch[(i / 3) % 3], ch[i / 9]); });
    for (int b : {1, -1})
        edits.push_back([b](Local& l) { l.bsdf_eval = b; });
    for (int c = 0; c < 3; c++)
        for (float bad : {nan, inf})
            edits.push_back([=](Local& l) { (c == 0 ? l.so.x : c == 1 ? l.so.y : l.so.z) = bad; });
    // other points of the rectangle: oblique directions, seen from where the vertex then is
    edits.push_back([](Local& l) { l.ra = 0.37f; l.rb = 0.81f; });
    edits.push_back([](Local& l) { l.ra = 0.999999940395355224609375f; l.so.x = -3.f; l.so.y = 7.f; });

    Seen seen;
    uint64_t mismatches = 0, control_mismatches = 0;
    auto one = [&](const In& in) {
        float s[4] = {0.f, 0.f, 0.f, 1.f};
        const Nee a = nested(in, s), b = flat(in);
        seen.n++;
        seen.has += a.has;
        seen.dist0 += s[0] == 0.0f;
        seen.dist_at += s[0] == 1.0e-6f;
        seen.dist_up += s[0] == up(1.0e-6f);
        seen.costa_p0 += s[1] == 0.0f && !std::signbit(s[1]);
        seen.costa_m0 += s[1] == 0.0f && std::signbit(s[1]);
        seen.costa_at += s[1] == 1.0e-6f;
        seen.costa_neg += s[1] < 0.0f;
        seen.lpdf_inf += s[2] == inf;
        seen.lpdf_nan += s[2] != s[2];
        seen.lpdf_0 += s[1] > 1.0e-6f && s[2] == 0.0f;
        seen.ndl_le0 += s[2] > 0.0f && s[3] <= 0.0f;
        if (!same(a, b) && mismatches++ == 0) print_case("MISMATCH", in, a, b);
        if (!same(a, control(in))) control_mismatches++;
    };
    const int gens[3] = {RTW_PDF_RECT_X, RTW_PDF_RECT_Y, RTW_PDF_RECT_Z};
    for (int gen : gens) {
        one(placed(gen, base()));
        for (size_t i = 0; i < edits.size(); i++) {
            Local l = base();
            edits[i](l);
            one(placed(gen, l));
            for (size_t j = 0; j < edits.size(); j++) {  // (ordered pairs: the later edit wins where two touch one field)
                if (j == i) continue;
                Local p = l;
                edits[j](p);
                one(placed(gen, p));
            }
        }
    }
    const uint64_t n_edges = seen.n;

    // random vertices of a box of the Cornell box's size around its light (213 .. 343 x 227 .. 332 at 554, 15 15 15, facing down)
    uint64_t state = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() {  // splitmix64 -> [0, 1) on the 2^-24 grid, like the renderer's draws
        state += 0x9e3779b97f4a7c15ull;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        return (float)(z >> 40) * (1.0f / 16777216.0f);
    };
    const v3 albedos[5] = {V(0.65f, 0.05f, 0.05f), V(0.73f, 0.73f, 0.73f), V(0.12f, 0.45f, 0.15f), V(0.f, 0.f, 0.f), V(0.f, 0.3f, -0.0f)};
    const v3 normals[6] = {V(1.f, 0.f, 0.f), V(-1.f, 0.f, 0.f), V(0.f, 1.f, 0.f), V(0.f, -1.f, 0.f), V(0.f, 0.f, 1.f), V(0.f, 0.f, -1.f)};
    for (int i = 0; i < 1000000; i++) {
        Local l = base();
        l.ra = rnd(); l.rb = rnd();
        l.rc[0] = 213.f; l.rc[1] = 343.f; l.rc[2] = 227.f; l.rc[3] = 332.f; l.rc[4] = 554.f;
        l.so = V(555.f * rnd(), 555.f * rnd(), 560.f * rnd());  // (a few vertices lie above the light's plane)
        const float pick = rnd();
        if (pick < 0.75f) {
            l.hn = normals[(int)(rnd() * 6.f)];
        } else {  // a sphere's normal
            const v3 r = V(rnd() - 0.5f, rnd() - 0.5f, rnd() - 0.5f);
            l.hn = vscale(r, 1.0f / sqrtf(dot3(r, r)));
        }
        l.att = albedos[(int)(rnd() * 5.f)];
        l.larea = 130.f * 105.f;
        l.bsdf_eval = rnd() < 0.9f ? 0 : 1;
        In in = placed(gens[i % 3], l);
        in.lemi = V(15.f, 15.f, 15.f);
        one(in);
    }

    int bad = 0;
    if (mismatches) { printf("%llu of %llu inputs differ\n", (unsigned long long)mismatches, (unsigned long long)seen.n); bad = 1; }
    if (!control_mismatches) { printf("the control (one & as |) was not rejected\n"); bad = 1; }
    const struct { const char* name; uint64_t n; } must[] = {
        {"has", seen.has}, {"no sample", seen.n - seen.has}, {"distance 0", seen.dist0}, {"distance 1e-6", seen.dist_at}, {"distance next up", seen.dist_up},
        {"costa +0", seen.costa_p0}, {"costa -0", seen.costa_m0}, {"costa 1e-6", seen.costa_at}, {"costa negative", seen.costa_neg},
        {"lpdf inf", seen.lpdf_inf}, {"lpdf NaN", seen.lpdf_nan}, {"lpdf 0", seen.lpdf_0}, {"ndl <= 0", seen.ndl_le0}};
    for (const auto& m : must)
        if (!m.n) { printf("no input with %s\n", m.name); bad = 1; }
    if (bad) return 1;
    printf("nee_flat_check ok: %llu inputs (%llu edges and pairs), %llu with a sample, control rejected on %llu\n", (unsigned long long)seen.n,
           (unsigned long long)n_edges, (unsigned long long)seen.has, (unsigned long long)control_mismatches);
    return 0;
}
