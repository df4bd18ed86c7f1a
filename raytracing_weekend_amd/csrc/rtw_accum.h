// rtw_accum.h — the per-pixel kernels of the accumulation sessions (include/rtw.h rtw_accum_*): the resolves that add the sums of an
// add into the session's state and keep the current summation unit open, the read that closes it into a copy, the error map. The
// adds themselves are the uniform launches (k_path with k_classify's job order, or the wavefront kernels): nothing of theirs changes.
// Included by rtw_hip.hip after rtw_adaptive.h (adapt_moments, adapt_err).
//
// Per shard pixel the state is: accum (sum of the closed summation units), upart (running sum of the open unit's finished blocks),
// with RTW_ACCUM_ERROR mom = (M1, M2) in fp64 over the block sums, and - inside a wavefront add only, zero between adds because adds
// are whole blocks - part (running sum of the current block). k_resolve_blocks / k_resolve + k_finish close the render's last unit
// when the render ends; here a unit is closed when its last block arrives, whichever add brings it, and k_accum_read adds the open
// one to a copy: the same additions in the same order, so the same bits (a closed unit leaves upart = +0, and x + 0 = x for every
// sum that started at +0).
#pragma once

namespace rtwk {

// the session counterpart of k_resolve_blocks: n_unit_slots whole unit sums [unit][pixel] (the session's unit is then empty: the host
// issues unit-sum launches on unit boundaries only, rtw_accum_state.h accum_split), then n_block_slots block sums [block][pixel], the
// first of which is block first_block of the session (counted from sample_offset; it need not be unit-aligned). mom: nullptr, or the
// moments to fold every block sum into (the host then stores no unit sums). Pixels outside the cull rectangle are left alone, as
// k_resolve_blocks leaves them.
__global__ void __launch_bounds__(kBlock) k_accum_resolve_blocks(const float4* __restrict__ slots, uint32_t npix, uint32_t n_unit_slots,
                                                                 uint32_t n_block_slots, uint32_t first_block, float4* __restrict__ accum,
                                                                 float4* __restrict__ upart, double2* __restrict__ mom, const ResolveCull R) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const uint32_t yl = fastdiv(i, R.divw_m, R.divw_s1, R.divw_s2);
        const int32_t x = (int32_t)(i - yl * R.width), y = (int32_t)(R.row0 + yl * R.row_stride);
        if (x < R.x0 || x >= R.x1 || y < R.y0 || y >= R.y1) continue;
        float4 a = accum[i], u = upart[i];
        for (uint32_t k = 0; k < n_unit_slots; k++) {
            const float4 l = slots[(size_t)k * npix + i];
            a.x += l.x; a.y += l.y; a.z += l.z;
        }
        double2 m = make_double2(0.0, 0.0);
        if (mom != nullptr) m = mom[i];
        for (uint32_t b = 0; b < n_block_slots; b++) {
            const float4 S = slots[(size_t)(n_unit_slots + b) * npix + i];
            if (mom != nullptr) adapt_moments(m, S);
            u.x += S.x; u.y += S.y; u.z += S.z;
            if (((first_block + b + 1u) % kSumUnitBlocks) == 0u) {
                a.x += u.x; a.y += u.y; a.z += u.z;
                u = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        accum[i] = a; upart[i] = u;
        if (mom != nullptr) mom[i] = m;
    }
}

// the session counterpart of k_resolve: nslots sample slots of one wavefront batch (radiance of path slot * npix + pixel), whose
// first sample is sample first_sample of the session. A block is closed (moments, unit sum) as soon as its last sample is in.
__global__ void __launch_bounds__(kBlock) k_accum_resolve_samples(const float4* __restrict__ lbuf, uint32_t npix, uint32_t nslots, uint32_t first_sample,
                                                                  float4* __restrict__ accum, float4* __restrict__ upart, float4* __restrict__ part,
                                                                  double2* __restrict__ mom) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        float4 a = accum[i], u = upart[i], b = part[i];
        double2 m = make_double2(0.0, 0.0);
        if (mom != nullptr) m = mom[i];
        for (uint32_t s = 0; s < nslots; s++) {
            const float4 l = lbuf[(size_t)s * npix + i];
            b.x += l.x; b.y += l.y; b.z += l.z;
            const uint32_t done = first_sample + s + 1u;
            if ((done % kSumBlock) == 0u) {
                if (mom != nullptr) adapt_moments(m, b);
                u.x += b.x; u.y += b.y; u.z += b.z;
                b = make_float4(0.f, 0.f, 0.f, 0.f);
                if ((done % (kSumBlock * kSumUnitBlocks)) == 0u) {
                    a.x += u.x; a.y += u.y; a.z += u.z;
                    u = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        }
        accum[i] = a; upart[i] = u; part[i] = b;
        if (mom != nullptr) mom[i] = m;
    }
}

// the frame after n samples: the open unit joins a copy of the total (as k_resolve_blocks / k_finish close the last unit), then the
// division by (float)n. The state is only read.
__global__ void __launch_bounds__(kBlock) k_accum_read(const float4* __restrict__ accum, const float4* __restrict__ upart, float4* __restrict__ out,
                                                       uint32_t npix, float n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        float4 a = accum[i];
        const float4 u = upart[i];
        a.x += u.x; a.y += u.y; a.z += u.z;
        out[i] = make_float4(a.x / n, a.y / n, a.z / n, 1.0f);
    }
}

// the error map after B blocks: rtw_render_adaptive's estimate (adapt_err) of every pixel's moments
__global__ void __launch_bounds__(kBlock) k_accum_error(const double2* __restrict__ mom, float* __restrict__ err, uint32_t npix, uint32_t B) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) err[i] = adapt_err(mom[i], B);
}

}  // namespace rtwk
