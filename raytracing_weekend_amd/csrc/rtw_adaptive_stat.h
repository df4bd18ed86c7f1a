// rtw_adaptive_stat.h — the batch-means statistic of the adaptive entry points (rtw.h rtw_render_adaptive): a block sum's luminance, the
// two fp64 moments and the error they give. Device functions only, so that a translation unit with kernels of its own
// (rtw_view_adaptive.hip) shares them with rtw_adaptive.h's kernels, which belong to rtw_hip.hip.
#pragma once

namespace rtwk {

// the batch-means statistic of one block sum: luminance of the block's mean (rtw.h, in this order, no contraction)
RTW_DEV float adapt_y(const float4 S) { return ((0.2126f * S.x + 0.7152f * S.y) + 0.0722f * S.z) * 0.0625f; }
RTW_DEV void adapt_moments(double2& m, const float4 S) {
    const double y = (double)adapt_y(S);
    m.x = m.x + y;
    m.y = m.y + y * y;
}
// standard error of sqrt(Y) from the moments of B blocks (rtw.h); NaN stays NaN (and so never compares below a threshold)
RTW_DEV float adapt_err(const double2 m, const uint32_t B) {
    const double b = (double)B;
    const double mean = m.x / b;
    double v = (m.y - m.x * mean) / (b - 1.0);
    v = v < 0.0 ? 0.0 : v;
    const double se = __builtin_sqrt(v / b);
    const double mm = mean < 1e-3 ? 1e-3 : mean;
    return (float)(se / (2.0 * __builtin_sqrt(mm)));
}

}  // namespace rtwk
