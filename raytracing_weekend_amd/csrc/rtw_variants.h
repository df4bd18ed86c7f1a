// rtw_variants.h - the shipped instantiations of the template kernels, as one table, and the host's choice among them. No HIP in
// here: rtw_hip.hip declares the rows (extern template) and expands each list into an array of kernel addresses, the rtw_inst_*.hip
// units instantiate them, and tests/native/variants_check.cpp proves the choice with g++. A new instantiation is one row here, one
// rule in its selector below and that rule's line in the check (DESIGN.md "Kernel variants: one table").
// A row is X(kernel, row name, template arguments in the kernel's order). The generator is written as its enumerator, and
// RTW_IF_<enumerator>(text) is text in a translation unit that instantiates that generator's rows (-DRTW_INST_KIND=0 / 1: one
// generator; without it: both); k_path's and k_first's frame (LIST = 0) and list (LIST = 1) rows are lists the units expand whole.
#pragma once
#include <stdint.h>

#include "../../include/rtw.h"
#include "rtw_plan.h"
#include "rtw_scene.h"

#if !defined(RTW_INST_KIND) || RTW_INST_KIND == 0
#define RTW_IF_RTW_RNG_PHILOX(...) __VA_ARGS__
#else
#define RTW_IF_RTW_RNG_PHILOX(...)
#endif
#if !defined(RTW_INST_KIND) || RTW_INST_KIND == 1
#define RTW_IF_RTW_RNG_TEA_LCG(...) __VA_ARGS__
#else
#define RTW_IF_RTW_RNG_TEA_LCG(...)
#endif
static_assert(RTW_RNG_PHILOX == 0 && RTW_RNG_TEA_LCG == 1, "RTW_INST_KIND is the generator's value");
// the parameter lists of the kernels that are instantiated explicitly
#define RTW_SIG_k_path (const KArgs)
#define RTW_SIG_k_first (const KArgs)
#define RTW_SIG_k_shade (const KArgs)
#define RTW_SIG_k_bounce (const KArgs)
#define RTW_SIG_k_classify (const KArgs, uint32_t*, uint32_t*, uint32_t)

// k_path<KIND, TEX, MEDIA5, LIST, NEE1, SHAPE>: per generator hot, cold features, cold features + the mixture estimator, cold features
// allocated for 5 waves (media); Philox's hot one has the one-light twin and its fixed-shape twin (rtw_kernels.h k_path)
#define RTW_K_PATH_ROWS_OF(X, P_, L_)                                                                                                     \
    X(k_path, P_##PHILOX_HOT, RTW_RNG_PHILOX, 0, 0, L_, 0, 0)   X(k_path, P_##TEA_HOT, RTW_RNG_TEA_LCG, 0, 0, L_, 0, 0)                   \
    X(k_path, P_##PHILOX_COLD, RTW_RNG_PHILOX, 1, 0, L_, 0, 0)  X(k_path, P_##TEA_COLD, RTW_RNG_TEA_LCG, 1, 0, L_, 0, 0)                  \
    X(k_path, P_##PHILOX_MIX, RTW_RNG_PHILOX, 2, 0, L_, 0, 0)   X(k_path, P_##TEA_MIX, RTW_RNG_TEA_LCG, 2, 0, L_, 0, 0)                   \
    X(k_path, P_##PHILOX_MEDIA, RTW_RNG_PHILOX, 1, 1, L_, 0, 0) X(k_path, P_##TEA_MEDIA, RTW_RNG_TEA_LCG, 1, 1, L_, 0, 0)                 \
    X(k_path, P_##PHILOX_ONE, RTW_RNG_PHILOX, 0, 0, L_, 1, 0)   X(k_path, P_##PHILOX_BOX, RTW_RNG_PHILOX, 0, 0, L_, 1, WALK_SHAPE_CORNELL)
#define RTW_K_PATH_FRAME_ROWS(X) RTW_K_PATH_ROWS_OF(X, PATH_, 0)
#define RTW_K_PATH_LIST_ROWS(X) RTW_K_PATH_ROWS_OF(X, PATH_LIST_, 1)
#define RTW_K_PATH_ROWS(X) RTW_K_PATH_FRAME_ROWS(X) RTW_K_PATH_LIST_ROWS(X)
// the kernels that shade exist per generator and feature level (0 hot, 1 cold features, 2 cold features + the mixture estimator):
// k_first<KIND, TEX, LIST>, k_shade<KIND, TEX>, k_bounce<KIND, TEX>
#define RTW_SHADING_ROWS_OF(X, K_, P_, ...)                                                                                               \
    X(K_, P_##PHILOX_HOT, RTW_RNG_PHILOX, 0 __VA_ARGS__) X(K_, P_##PHILOX_COLD, RTW_RNG_PHILOX, 1 __VA_ARGS__) X(K_, P_##PHILOX_MIX, RTW_RNG_PHILOX, 2 __VA_ARGS__) \
    X(K_, P_##TEA_HOT, RTW_RNG_TEA_LCG, 0 __VA_ARGS__)   X(K_, P_##TEA_COLD, RTW_RNG_TEA_LCG, 1 __VA_ARGS__)   X(K_, P_##TEA_MIX, RTW_RNG_TEA_LCG, 2 __VA_ARGS__)
#define RTW_K_FIRST_FRAME_ROWS(X) RTW_SHADING_ROWS_OF(X, k_first, FIRST_, , 0)
#define RTW_K_FIRST_LIST_ROWS(X) RTW_SHADING_ROWS_OF(X, k_first, FIRST_LIST_, , 1)
#define RTW_K_FIRST_ROWS(X) RTW_K_FIRST_FRAME_ROWS(X) RTW_K_FIRST_LIST_ROWS(X)
#define RTW_K_SHADE_ROWS(X) RTW_SHADING_ROWS_OF(X, k_shade, SHADE_)
#define RTW_K_BOUNCE_ROWS(X) RTW_SHADING_ROWS_OF(X, k_bounce, BOUNCE_)
// k_classify<WALK>, k_trace<DUAL>, k_trace_bvh<BLOCK, MODE>
#define RTW_K_CLASSIFY_ROWS(X) X(k_classify, CLASSIFY_WALK, true) X(k_classify, CLASSIFY_BOUNDS, false)
#define RTW_K_TRACE_ROWS(X) X(k_trace, TRACE_DUAL, true) X(k_trace, TRACE_GENERIC, false)
#define RTW_K_TRACE_BVH_ROWS(X)                                                                                       \
    X(k_trace_bvh, TRACE_BVH_256_0, 256, 0)   X(k_trace_bvh, TRACE_BVH_256_1, 256, 1)   X(k_trace_bvh, TRACE_BVH_256_2, 256, 2)    \
    X(k_trace_bvh, TRACE_BVH_512_0, 512, 0)   X(k_trace_bvh, TRACE_BVH_512_1, 512, 1)   X(k_trace_bvh, TRACE_BVH_512_2, 512, 2)    \
    X(k_trace_bvh, TRACE_BVH_1024_0, 1024, 0) X(k_trace_bvh, TRACE_BVH_1024_1, 1024, 1) X(k_trace_bvh, TRACE_BVH_1024_2, 1024, 2)

namespace rtwk {
using rtwdev::WALK_SHAPE_CORNELL;
// per list: the rows' indices (<LIST>_ROWS: how many; also what a selector returns when no row has the arguments it wants - the
// arrays of rtw_hip.hip hold a null address there, so such a launch fails), their template arguments and their names
struct VariantArgs { int v[6]; };
#define RTW_ROW_ENUM(K_, name, ...) name,
#define RTW_ROW_ARGS(K_, name, ...) {{__VA_ARGS__}},
#define RTW_ROW_NAME(K_, name, ...) #name,
#define RTW_VARIANT_LIST(LIST_, Enum_, args_, names_)              \
    enum Enum_ { LIST_(RTW_ROW_ENUM) Enum_##s };                   \
    constexpr VariantArgs args_[] = {LIST_(RTW_ROW_ARGS)};         \
    constexpr const char* names_[] = {LIST_(RTW_ROW_NAME) "none"};
RTW_VARIANT_LIST(RTW_K_PATH_ROWS, PathRow, kPathArgs, kPathNames)
RTW_VARIANT_LIST(RTW_K_FIRST_ROWS, FirstRow, kFirstArgs, kFirstNames)
RTW_VARIANT_LIST(RTW_K_SHADE_ROWS, ShadeRow, kShadeArgs, kShadeNames)
RTW_VARIANT_LIST(RTW_K_BOUNCE_ROWS, BounceRow, kBounceArgs, kBounceNames)
RTW_VARIANT_LIST(RTW_K_CLASSIFY_ROWS, ClassifyRow, kClassifyArgs, kClassifyNames)
RTW_VARIANT_LIST(RTW_K_TRACE_ROWS, TraceRow, kTraceArgs, kTraceNames)
RTW_VARIANT_LIST(RTW_K_TRACE_BVH_ROWS, TraceBvhRow, kTraceBvhArgs, kTraceBvhNames)
#undef RTW_VARIANT_LIST
// the row of a list with these template arguments (arguments a kernel does not have: 0); N when there is none
template <size_t N>
constexpr int variant_row(const VariantArgs (&rows)[N], const VariantArgs& want) {
    for (size_t r = 0; r < N; r++) {
        bool same = true;
        for (int k = 0; k < 6; k++) same = same && rows[r].v[k] == want.v[k];
        if (same) return (int)r;
    }
    return (int)N;
}
// k_path's and k_first's frame rows have LIST = 0 and their list rows LIST = 1 (what the units that expand those lists rely on),
// and no k_path row breaks the kernel's own static_assert
constexpr bool variant_lists_hold() {
    bool ok = true;
    for (int r = 0; r < PathRows; r++) ok = ok && kPathArgs[r].v[3] == (r >= PathRows / 2) && (kPathArgs[r].v[5] == 0 || (kPathArgs[r].v[4] && !kPathArgs[r].v[1]));
    for (int r = 0; r < FirstRows; r++) ok = ok && kFirstArgs[r].v[2] == (r >= FirstRows / 2);
    return ok;
}
static_assert(variant_lists_hold(), "a row in the wrong list");

// ---- the choice. S: DScene (rtw_device.h), or a record with the same header fields (the CPU check's)
// the corrected estimators live in the cold-feature instantiations
template <class S>
constexpr void apply_estimator(S& sc, int estimator) {
    if (estimator == RTW_EST_REFERENCE) return;
    sc.estimator = estimator; sc.has_tex = estimator == RTW_EST_MIXTURE ? 2 : 1;
    sc.ray_tmin = 1.0e-3f; sc.probe_eps = 1.0e-3f;
}
// The hot instantiation with Philox has a one-light twin (rtw_kernels.h k_path NEE1), for scenes whose light sample is always the same
// case of shade_a: exactly one listed light, the reference estimator (feature level 0 has no other), a rectangle generator.
template <class S>
constexpr bool path_nee1(int rng_kind, const S& sc) {
    int gen = sc.pdf.gen;
    if (gen == RTW_PDF_MIXTURE || gen == RTW_PDF_MIXTURE_BIAS) gen = sc.pdf.p1_gen;
    return rng_kind == RTW_RNG_PHILOX && sc.has_tex == 0 && sc.estimator == RTW_EST_REFERENCE && sc.n_lights == 1 &&
           (gen == RTW_PDF_RECT_X || gen == RTW_PDF_RECT_Y || gen == RTW_PDF_RECT_Z);
}
// k_path's row: generator x feature level; media scenes take the cold instantiation allocated for 5 waves (MEDIA5); list: the LIST = 1
// twin (rtw_render_adaptive). The one-light twin in turn has a fixed-shape twin (SHAPE) for the scenes whose candidate lists have a
// compiled shape: walk_shape is what prepare_scene found for the uploaded scene (SceneInfo::walk_shape; 0: none).
template <class S>
constexpr PathRow path_row(int rng_kind, const S& sc, int walk_shape, bool list) {
    const int kind = rng_kind == RTW_RNG_TEA_LCG ? RTW_RNG_TEA_LCG : RTW_RNG_PHILOX, feat = sc.has_tex;
    const bool nee1 = path_nee1(rng_kind, sc);
    const VariantArgs want = {{kind, feat == 1 || feat == 2 ? feat : 0, feat == 1 && sc.n_vol > 0, list, nee1,
                               nee1 && walk_shape == WALK_SHAPE_CORNELL ? WALK_SHAPE_CORNELL : 0}};
    return (PathRow)variant_row(kPathArgs, want);
}
// the kernels that shade: generator x feature level (feat: DScene::has_tex); k_first has a list twin (rtw_render_adaptive's wavefront passes)
constexpr VariantArgs shading_args(int rng_kind, int feat, bool list) {
    return {{rng_kind == RTW_RNG_TEA_LCG ? RTW_RNG_TEA_LCG : RTW_RNG_PHILOX, feat == 1 || feat == 2 ? feat : 0, list}};
}
constexpr FirstRow first_row(int rng_kind, int feat, bool list) { return (FirstRow)variant_row(kFirstArgs, shading_args(rng_kind, feat, list)); }
constexpr ShadeRow shade_row(int rng_kind, int feat) { return (ShadeRow)variant_row(kShadeArgs, shading_args(rng_kind, feat, false)); }
constexpr BounceRow bounce_row(int rng_kind, int feat) { return (BounceRow)variant_row(kBounceArgs, shading_args(rng_kind, feat, false)); }
// k_classify stages the walk image when the scene has one; k_trace<true> knows that the scene has no moving spheres
template <class S>
constexpr ClassifyRow classify_row(const S& sc) { return (ClassifyRow)variant_row(kClassifyArgs, {{sc.n_walk_words > 0}}); }
template <class S>
constexpr TraceRow trace_row(const S& sc) { return (TraceRow)variant_row(kTraceArgs, {{sc.n_generic == 0}}); }
// k_trace_bvh's row for a workgroup size and a tree (mode: see the kernel)
template <class S>
constexpr int trace_bvh_mode(const S& sc) { return sc.stack_wide ? 0 : sc.n_lds_nodes >= sc.n_nodes ? 2 : 1; }
constexpr TraceBvhRow trace_bvh_row(int block, int mode) {
    return (TraceBvhRow)variant_row(kTraceBvhArgs, {{block == 1024 || block == 512 ? block : 256, mode == 0 || mode == 1 ? mode : 2}});
}
// k_path: scenes walked with the brute lists; it packs a unit's pixel as x | y << 16, so frames wider or taller than 65535
// take the wavefront kernels
template <class S>
constexpr bool path_pipeline(const S& sc, int width, int height, int max_depth, const Tuning& tune) {
    const bool path_small = !sc.use_bvh && sc.n_prims <= kPathMaxPrims && (sc.n_walk_words > 0 || sc.has_tex);
    const bool fits16 = width <= 65535 && height <= 65535;
    return max_depth > 0 && tune.path != 0 && fits16 && path_small;
}
}  // namespace rtwk
