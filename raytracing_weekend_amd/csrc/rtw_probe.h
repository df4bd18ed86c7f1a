// rtw_probe.h — declarations of the probe kernels (rtw_probe.hip): irradiance and ambient occlusion at surface points, the direction
// of every sample drawn on the device from the sample's own raygen uniforms (rtw.h rtw_probe / rtw_probe_device). Included by
// rtw_hip.hip, which launches them.
#pragma once
#include "rtw_kernels.h"
#include "rtw_radiance.h"

namespace rtwk {

constexpr float kProbePi = 3.14159265f;  // the irradiance estimate: the mean radiance over the density cos / pi, times pi

// RTW_PROBE_IRRADIANCE: k_radiance's launch (RadianceArgs, `rays` holding the probes: the normal in the direction's place) and its
// persistent scheme; only the regeneration step differs (rtw_radiance_body.h). units_per_ray == 1: (mean) * pi of probe i at [i].
template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe(const DScene sc, const RadianceArgs a);

// irradiance of probe i: its n_units unit sums slab[unit][i] added in ascending order, divided by spp, times pi, alpha 1
__global__ void __launch_bounds__(kBlock) k_probe_resolve(const float4* __restrict__ slab, float4* __restrict__ out, uint32_t n, uint32_t n_units, float spp);

// RTW_PROBE_OCCLUSION: one lane per (probe, summation unit of up to 128 samples), numbered unit-major as k_radiance's units
// (u -> probe = u % n, unit = u / n; n_units = n * units_per_probe < 2^31), lanes stride over the units.
struct OcclusionArgs {
    const float4* probes;
    float4* out;       // units_per_probe == 1: (unoccluded / spp) x 3, 1 of probe i at [i]
    uint32_t* counts;  // else the units' unoccluded counts, [unit][probe]
    uint32_t n, units_per_probe, n_units;
    uint32_t divn_m, divn_s1, divn_s2;  // exact division by n (magic_div)
    uint32_t spp, sample0, seed, key0;
};

// every sample: the direction generator, then traverse<NoRng, true, true> (k_cast<true, false>'s walk: volumes skipped, times 0)
template <int KIND>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe_occlusion(const DScene sc, const OcclusionArgs a);

// probe i: its n_units counts added as integers, the sum divided by spp
__global__ void __launch_bounds__(kBlock) k_probe_occlusion_resolve(const uint32_t* __restrict__ counts, float4* __restrict__ out, uint32_t n, uint32_t n_units, float spp);

}  // namespace rtwk
