// rtw_probe_sh.h — declarations of the spherical-harmonic probe kernels (rtw_probe_sh.hip): the radiance arriving at free points,
// projected onto the nine real spherical harmonics of bands 0 to 2 (rtw.h rtw_probe_sh / rtw_probe_sh_device). Included by
// rtw_hip.hip, which launches them.
#pragma once
#include "rtw_kernels.h"
#include "rtw_radiance.h"

namespace rtwk {

constexpr float kProbeSh4Pi = 12.5663706f;  // the float nearest 4 pi: the mean over the density 1 / (4 pi), times 4 pi

// k_radiance's launch (RadianceArgs, `rays` holding the points) and its persistent scheme; the regeneration step draws a direction
// uniform over the sphere and a finished path adds Y_j * L to nine coefficients (rtw_radiance_body.h). `out` is nine float4 per
// point (units_per_ray == 1: the coefficients of point i at [9 i + j]) or per unit and point (else: the unit sums at
// [(unit * n + point) * 9 + j]); 9 * n_units < 2^31 (rtw_radiance_plan.h). Static LDS: kShRows rows of kBlock floats.
template <int KIND, int TEX>
__global__ void __launch_bounds__(kBlock, RTW_MIN_WAVES) k_probe_sh(const DScene sc, const RadianceArgs a);

// coefficient j of point i: its n_units unit sums slab[(unit * n + i) * 9 + j] added in ascending order, divided by spp, times
// 4 pi, w = 0 (n_units = 0: zeros)
__global__ void __launch_bounds__(kBlock) k_probe_sh_resolve(const float4* __restrict__ slab, float4* __restrict__ out, uint32_t n, uint32_t n_units, float spp);

}  // namespace rtwk
