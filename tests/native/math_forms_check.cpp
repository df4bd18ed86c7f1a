// CPU check of the short reciprocal / root forms of raytracing_weekend_amd/csrc/rtw_math.h against a host model of the
// hardware approximations: P::rcp / P::rsq return the correctly rounded 1/x / 1/sqrt(x) displaced by K ulp (the hardware is
// documented at 1 ulp; K = -2 .. 2). Run by tests/test_math_forms_cpu.py, which says what must hold for which K.
// Compile with -ffp-contract=off: every fusion in the header is written out.
//
// usage: math_forms_check <op> <k>     op: rcp | sqrt | rcp_sqrt | rcp3
// For every significand at the lowest and the highest exponent the window admits, the ones next to them outside it and a few
// in between, and for every exponent at sampled significands (both signs for rcp): wherever the range test says "fast", the
// short form equals 1.0f / x / sqrtf(x) / 1.0f / sqrtf(x) bit for bit.
// Prints one line: "<op> <k> tried <n> fast <n> differ <n> ones <n> first <hex bits of the first differing input, or ->".
// ones: the differing inputs whose reciprocal operand (x, or its root for rcp_sqrt) has the all-ones significand 0x7fffff. There
// 1/x lies 2^-24 ulp above a tie, and two Newton steps reach it only from the correctly rounded start: whether the hardware
// gives that start is what the exhaustive sweep on the device decides (tests/test_gpu_math_forms.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../raytracing_weekend_amd/csrc/rtw_math.h"

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
// sign-magnitude: k ulp away from zero
static float displace(float f, int k) { return from_bits(to_bits(f) + (uint32_t)k); }

template <int K>
struct Host {
    static float rcp(float x) { return displace(1.0f / x, K); }
    static float rsq(float x) { return displace((float)(1.0L / sqrtl((long double)x)), K); }
    static float fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
    static bool all(bool ok) { return ok; }
};

struct Tally {
    uint64_t tried = 0, fast = 0, differ = 0, ones = 0;
    uint32_t first = 0;
    void add(uint32_t bits, bool is_fast, float got, float want, float rcp_operand = 0.0f) {
        tried++;
        if (!is_fast) return;
        fast++;
        const bool same = to_bits(got) == to_bits(want) || (got != got && want != want);
        if (same) return;
        if (differ++ == 0) first = bits;
        if ((to_bits(rcp_operand) & 0x7fffffu) == 0x7fffffu) ones++;
    }
};

template <int K>
static void one(int op, uint32_t bits, Tally& t) {
    using P = Host<K>;
    const float x = from_bits(bits);
    if (op == 0) {
        t.add(bits, rtwmath::rcp_window(x), rtwmath::rcp<P>(x), 1.0f / x, x);
    } else if (op == 1) {
        t.add(bits, rtwmath::sqrt_window(x), rtwmath::sqrt<P>(x), sqrtf(x));
        if (rtwmath::sqrt_window(x)) t.add(bits, true, rtwmath::sqrt_inside<P>(x), sqrtf(x));
    } else if (op == 2) {
        t.add(bits, rtwmath::sqrt_window(x), rtwmath::rcp_sqrt<P>(x), 1.0f / sqrtf(x), sqrtf(x));
    } else {
        // the vector form: x beside two fixed in-window components, and beside itself
        float a = x, b = 3.0f, c = -0.75f;
        const bool w = rtwmath::rcp_window3(a, b, c);
        rtwmath::rcp3<P>(a, b, c);
        t.add(bits, w, a, 1.0f / x, x);
        t.add(bits, w, b, 1.0f / 3.0f);
        t.add(bits, w, c, 1.0f / -0.75f);
        // the one test stands for the three (a NaN component passes max / min unseen and gives NaN either way: rtw_math.h)
        if (x == x && w != rtwmath::rcp_window(x) && t.differ++ == 0) t.first = bits;
    }
}

template <int K>
static Tally run(int op) {
    Tally t;
    // biased exponents: 63 = 2^-64 (lowest inside), 62 below it; 190 = 2^63 (highest with every significand inside), 191 = 2^64
    // (inside for significand 0 only)
    const int full[] = {62, 63, 64, 126, 127, 128, 189, 190, 191};
    for (int e : full)
        for (uint32_t m = 0; m < (1u << 23); m++) {
            one<K>(op, ((uint32_t)e << 23) | m, t);
            if (op == 0) one<K>(op, 0x80000000u | ((uint32_t)e << 23) | m, t);
        }
    uint32_t lcg = 12345u;
    for (int e = 0; e < 256; e++)
        for (int i = 0; i < 4096; i++) {
            uint32_t m;
            if (i == 0) m = 0;
            else if (i == 1) m = 0x7fffffu;
            else if (i == 2) m = 1;
            else if (i == 3) m = 0x7ffffeu;
            else { lcg = lcg * 1664525u + 1013904223u; m = lcg >> 9; }
            one<K>(op, ((uint32_t)e << 23) | m, t);
            one<K>(op, 0x80000000u | ((uint32_t)e << 23) | m, t);
        }
    return t;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: math_forms_check <rcp|sqrt|rcp_sqrt|rcp3> <k>\n"); return 2; }
    const char* names[] = {"rcp", "sqrt", "rcp_sqrt", "rcp3"};
    int op = -1;
    for (int i = 0; i < 4; i++) if (!strcmp(argv[1], names[i])) op = i;
    const int k = atoi(argv[2]);
    if (op < 0 || k < -2 || k > 2) return 2;
    Tally t;
    switch (k) {
        case -2: t = run<-2>(op); break;
        case -1: t = run<-1>(op); break;
        case 0: t = run<0>(op); break;
        case 1: t = run<1>(op); break;
        default: t = run<2>(op); break;
    }
    char first[16] = "-";
    if (t.differ) snprintf(first, sizeof first, "%08x", t.first);
    printf("%s %d tried %llu fast %llu differ %llu ones %llu first %s\n", names[op], k, (unsigned long long)t.tried,
           (unsigned long long)t.fast, (unsigned long long)t.differ, (unsigned long long)t.ones, first);
    return 0;
}
