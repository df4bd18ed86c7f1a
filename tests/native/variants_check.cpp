// CPU check of the kernel choice (raytracing_weekend_amd/csrc/rtw_variants.h): which instantiation of k_path, k_first, k_shade, k_bounce,
// k_classify, k_trace and k_trace_bvh the host launches for a scene, a generator and a pass, and which pipeline renders a frame. A scene
// sent to the wrong row is not a link error but a wrong image (the fixed-shape walk reads records as the wrong kind), so the rules are
// written out here a second time, from the comments on the kernels in rtw_kernels.h, and compared over every input.
// Compiled and run by tests/test_variants_cpu.py; may be built with -fsanitize=address,undefined.
// usage: variants_check rules      every combination of the selectors' inputs against the rules below; every row of every list chosen by
//                                  some input; no input chooses a row that k_path's static_assert forbids; path_pipeline's edges
//        variants_check row <blob> <rng_kind> <estimator> <list> <width> <height> <max_depth>
//                                  prepare_scene on the blob, the estimator applied as a render applies it, then one line:
//                                  pipeline=<path|wavefront> k_path=<row> k_first=<row>. RTW_* are read as the library reads them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracing_weekend_amd/csrc/rtw_variants.h"
using namespace rtwk;
using namespace rtwdev;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// DScene's header fields that the choice reads, under DScene's names
struct Scene {
    int32_t n_prims, n_vol, n_lights, use_bvh, n_generic, n_walk_words, n_lds_nodes, has_tex, stack_wide, n_nodes, estimator;
    float ray_tmin, probe_eps;
    rtw_pdf pdf;
};

// k_path's row by the kernel's own description: the one-light instantiation for Philox without cold features, under the reference
// estimator, one listed light and a rectangle generator (also as the second child of a mixture), with the fixed-shape walks when
// the lists have the Cornell shape; otherwise by feature level, media scenes in the instantiation allocated for 5 waves
static PathRow expected_path(int kind, const Scene& sc, int walk_shape, bool list) {
    const bool tea = kind == RTW_RNG_TEA_LCG;
    const bool mixture = sc.pdf.gen == RTW_PDF_MIXTURE || sc.pdf.gen == RTW_PDF_MIXTURE_BIAS;
    const int gen = mixture ? sc.pdf.p1_gen : sc.pdf.gen;
    const bool rect = gen == RTW_PDF_RECT_X || gen == RTW_PDF_RECT_Y || gen == RTW_PDF_RECT_Z;
    if (!tea && sc.has_tex == 0 && sc.estimator == RTW_EST_REFERENCE && sc.n_lights == 1 && rect) {
        if (walk_shape == WALK_SHAPE_CORNELL) return list ? PATH_LIST_PHILOX_BOX : PATH_PHILOX_BOX;
        return list ? PATH_LIST_PHILOX_ONE : PATH_PHILOX_ONE;
    }
    if (sc.has_tex == 2) return list ? (tea ? PATH_LIST_TEA_MIX : PATH_LIST_PHILOX_MIX) : (tea ? PATH_TEA_MIX : PATH_PHILOX_MIX);
    if (sc.has_tex == 1 && sc.n_vol > 0) return list ? (tea ? PATH_LIST_TEA_MEDIA : PATH_LIST_PHILOX_MEDIA) : (tea ? PATH_TEA_MEDIA : PATH_PHILOX_MEDIA);
    if (sc.has_tex == 1) return list ? (tea ? PATH_LIST_TEA_COLD : PATH_LIST_PHILOX_COLD) : (tea ? PATH_TEA_COLD : PATH_PHILOX_COLD);
    return list ? (tea ? PATH_LIST_TEA_HOT : PATH_LIST_PHILOX_HOT) : (tea ? PATH_TEA_HOT : PATH_PHILOX_HOT);
}

static void check_rules() {
    bool seen_path[PathRows + 1] = {}, seen_first[FirstRows + 1] = {}, seen_shade[ShadeRows + 1] = {}, seen_bounce[BounceRows + 1] = {};
    bool seen_classify[ClassifyRows + 1] = {}, seen_trace[TraceRows + 1] = {}, seen_bvh[TraceBvhRows + 1] = {};
    long n = 0;
    const int estimators[] = {RTW_EST_REFERENCE, RTW_EST_CORRECTED, RTW_EST_CORRECTED_NO_NEE, RTW_EST_MIXTURE};
    for (int kind = 0; kind < 2; kind++)
    for (int tex = 0; tex < 3; tex++)
    for (int n_vol = 0; n_vol <= 3; n_vol += 3)
    for (int est : estimators)
    for (int n_lights = 0; n_lights < 3; n_lights++)
    for (int gen = RTW_PDF_COSINE; gen <= RTW_PDF_RECT_Z; gen++)
    for (int p1 = -1; p1 <= RTW_PDF_RECT_Z; p1++)
    for (int shape = 0; shape < 2; shape++)
    for (int list = 0; list < 2; list++) {
        Scene sc{};
        sc.has_tex = tex; sc.n_vol = n_vol; sc.estimator = est; sc.n_lights = n_lights; sc.pdf.gen = gen; sc.pdf.p1_gen = p1;
        const PathRow got = path_row(kind, sc, shape, list != 0), want = expected_path(kind, sc, shape, list != 0);
        n++;
        CHECK(got == want, "kind %d has_tex %d n_vol %d estimator %d n_lights %d gen %d p1_gen %d shape %d list %d: row %s, expected %s", kind, tex, n_vol,
              est, n_lights, gen, p1, shape, list, kPathNames[got], kPathNames[want]);
        if (got >= PathRows) continue;
        seen_path[got] = true;
        // the row's template arguments are the facts themselves, and none that the kernel refuses to compile
        const int* v = kPathArgs[got].v;  // KIND, TEX, MEDIA5, LIST, NEE1, SHAPE
        CHECK(v[0] == kind && v[3] == list, "%s: KIND %d LIST %d for kind %d list %d", kPathNames[got], v[0], v[3], kind, list);
        CHECK(v[1] == tex && v[2] == (tex == 1 && n_vol > 0), "%s: TEX %d MEDIA5 %d for has_tex %d n_vol %d", kPathNames[got], v[1], v[2], tex, n_vol);
        CHECK(!v[4] || (v[1] == 0 && v[0] == RTW_RNG_PHILOX && n_lights == 1 && est == RTW_EST_REFERENCE), "%s: NEE1 with TEX %d kind %d n_lights %d estimator %d",
              kPathNames[got], v[1], v[0], n_lights, est);
        CHECK(v[5] == 0 || (v[4] && v[5] == shape), "%s: SHAPE %d with NEE1 %d for shape %d", kPathNames[got], v[5], v[4], shape);
    }
    // the kernels that shade: generator x feature level, k_first with its list twin
    const FirstRow first_want[2][2][3] = {{{FIRST_PHILOX_HOT, FIRST_PHILOX_COLD, FIRST_PHILOX_MIX}, {FIRST_TEA_HOT, FIRST_TEA_COLD, FIRST_TEA_MIX}},
                                          {{FIRST_LIST_PHILOX_HOT, FIRST_LIST_PHILOX_COLD, FIRST_LIST_PHILOX_MIX}, {FIRST_LIST_TEA_HOT, FIRST_LIST_TEA_COLD, FIRST_LIST_TEA_MIX}}};
    const ShadeRow shade_want[2][3] = {{SHADE_PHILOX_HOT, SHADE_PHILOX_COLD, SHADE_PHILOX_MIX}, {SHADE_TEA_HOT, SHADE_TEA_COLD, SHADE_TEA_MIX}};
    const BounceRow bounce_want[2][3] = {{BOUNCE_PHILOX_HOT, BOUNCE_PHILOX_COLD, BOUNCE_PHILOX_MIX}, {BOUNCE_TEA_HOT, BOUNCE_TEA_COLD, BOUNCE_TEA_MIX}};
    for (int kind = 0; kind < 2; kind++)
        for (int feat = 0; feat < 3; feat++) {
            for (int list = 0; list < 2; list++) {
                const FirstRow f = first_row(kind, feat, list != 0);
                CHECK(f == first_want[list][kind][feat], "k_first kind %d feat %d list %d: %s", kind, feat, list, kFirstNames[f]);
                CHECK(f < FirstRows && kFirstArgs[f].v[0] == kind && kFirstArgs[f].v[1] == feat && kFirstArgs[f].v[2] == list, "%s: arguments", kFirstNames[f]);
                seen_first[f] = true;
            }
            const ShadeRow s = shade_row(kind, feat);
            const BounceRow b = bounce_row(kind, feat);
            CHECK(s == shade_want[kind][feat] && s < ShadeRows && kShadeArgs[s].v[0] == kind && kShadeArgs[s].v[1] == feat, "k_shade kind %d feat %d: %s", kind, feat, kShadeNames[s]);
            CHECK(b == bounce_want[kind][feat] && b < BounceRows && kBounceArgs[b].v[0] == kind && kBounceArgs[b].v[1] == feat, "k_bounce kind %d feat %d: %s", kind, feat, kBounceNames[b]);
            seen_shade[s] = true; seen_bounce[b] = true;
        }
    // k_classify stages the walk image iff the scene has one; k_trace<true> iff the scene has no moving spheres
    for (int words = 0; words <= 57; words += 57) {
        Scene sc{};
        sc.n_walk_words = words;
        const ClassifyRow c = classify_row(sc);
        CHECK(c == (words > 0 ? CLASSIFY_WALK : CLASSIFY_BOUNDS) && kClassifyArgs[c].v[0] == (words > 0), "k_classify for %d walk words: %s", words, kClassifyNames[c]);
        seen_classify[c] = true;
    }
    for (int generic = 0; generic <= 2; generic += 2) {
        Scene sc{};
        sc.n_generic = generic;
        const TraceRow t = trace_row(sc);
        CHECK(t == (generic == 0 ? TRACE_DUAL : TRACE_GENERIC) && kTraceArgs[t].v[0] == (generic == 0), "k_trace for %d generic primitives: %s", generic, kTraceNames[t]);
        seen_trace[t] = true;
    }
    // k_trace_bvh: workgroup size x mode (0: 32-bit stack entries; 2: the LDS image holds every node; 1: neither)
    const TraceBvhRow bvh_want[3][3] = {{TRACE_BVH_256_0, TRACE_BVH_256_1, TRACE_BVH_256_2}, {TRACE_BVH_512_0, TRACE_BVH_512_1, TRACE_BVH_512_2},
                                        {TRACE_BVH_1024_0, TRACE_BVH_1024_1, TRACE_BVH_1024_2}};
    for (int bi = 0; bi < 3; bi++)
        for (int wide = 0; wide < 2; wide++)
            for (int staged = 9; staged <= 11; staged++) {  // of 10 nodes
                Scene sc{};
                sc.stack_wide = wide; sc.n_lds_nodes = staged; sc.n_nodes = 10;
                const int mode = trace_bvh_mode(sc), block = 256 << bi;
                CHECK(mode == (wide ? 0 : staged >= 10 ? 2 : 1), "mode %d for stack_wide %d, %d of 10 nodes staged", mode, wide, staged);
                const TraceBvhRow t = trace_bvh_row(block, mode);
                CHECK(t == bvh_want[bi][mode] && kTraceBvhArgs[t].v[0] == block && kTraceBvhArgs[t].v[1] == mode, "k_trace_bvh block %d mode %d: %s", block, mode, kTraceBvhNames[t]);
                seen_bvh[t] = true;
            }
    // no dead rows: a row that no input chooses is a kernel that ships and never runs
    auto all_seen = [](const bool* seen, int rows, const char* const* names, const char* kernel) {
        for (int r = 0; r < rows; r++) CHECK(seen[r], "%s row %s is chosen by no input", kernel, names[r]);
        CHECK(!seen[rows], "%s: an input found no row", kernel);
    };
    all_seen(seen_path, PathRows, kPathNames, "k_path");
    all_seen(seen_first, FirstRows, kFirstNames, "k_first");
    all_seen(seen_shade, ShadeRows, kShadeNames, "k_shade");
    all_seen(seen_bounce, BounceRows, kBounceNames, "k_bounce");
    all_seen(seen_classify, ClassifyRows, kClassifyNames, "k_classify");
    all_seen(seen_trace, TraceRows, kTraceNames, "k_trace");
    all_seen(seen_bvh, TraceBvhRows, kTraceBvhNames, "k_trace_bvh");
    printf("rules: %ld k_path inputs; rows k_path %d k_first %d k_shade %d k_bounce %d k_classify %d k_trace %d k_trace_bvh %d, each chosen\n", n, (int)PathRows,
           (int)FirstRows, (int)ShadeRows, (int)BounceRows, (int)ClassifyRows, (int)TraceRows, (int)TraceBvhRows);

    // the estimator of a render: the corrected ones run the cold features, the mixture estimator feature level 2
    for (int est : estimators)
        for (int tex = 0; tex < 2; tex++) {
            Scene sc{};
            sc.has_tex = tex; sc.estimator = RTW_EST_REFERENCE; sc.ray_tmin = 1e-6f; sc.probe_eps = 5e-5f;
            apply_estimator(sc, est);
            const bool ref = est == RTW_EST_REFERENCE;
            CHECK(sc.estimator == est && sc.has_tex == (ref ? tex : est == RTW_EST_MIXTURE ? 2 : 1), "estimator %d: has_tex %d -> %d", est, tex, sc.has_tex);
            CHECK(sc.ray_tmin == (ref ? 1e-6f : 1e-3f) && sc.probe_eps == (ref ? 5e-5f : 1e-3f), "estimator %d: tmin %g eps %g", est, sc.ray_tmin, sc.probe_eps);
        }

    // path_pipeline: k_path renders list scenes of at most kPathMaxPrims primitives that have a walk image or cold features, in frames
    // whose pixel packs into 16 + 16 bits, at a depth above 0, unless RTW_PATH=0
    Scene ok{};
    ok.n_prims = 13; ok.n_walk_words = 57;
    Tuning tune;
    CHECK(tune.path != 0 && path_pipeline(ok, 800, 800, 50, tune), "the plain case");
    CHECK(path_pipeline(ok, 65535, 1, 1, tune) && !path_pipeline(ok, 65536, 1, 1, tune), "width 65535 / 65536");
    CHECK(path_pipeline(ok, 1, 65535, 1, tune) && !path_pipeline(ok, 1, 65536, 1, tune), "height 65535 / 65536");
    CHECK(!path_pipeline(ok, 800, 800, 0, tune), "max_depth 0");
    {   Tuning off; off.path = 0; CHECK(!path_pipeline(ok, 800, 800, 50, off), "RTW_PATH=0"); }
    {   Scene s = ok; s.n_prims = kPathMaxPrims; CHECK(path_pipeline(s, 800, 800, 50, tune), "kPathMaxPrims primitives");
        s.n_prims = kPathMaxPrims + 1; CHECK(!path_pipeline(s, 800, 800, 50, tune), "one more"); }
    {   Scene s = ok; s.use_bvh = 1; CHECK(!path_pipeline(s, 800, 800, 50, tune), "a scene with a tree");
        s.has_tex = 1; CHECK(!path_pipeline(s, 800, 800, 50, tune), "a textured scene with a tree"); }
    {   Scene s = ok; s.n_walk_words = 0; CHECK(!path_pipeline(s, 800, 800, 50, tune), "no walk image, no cold features");
        s.has_tex = 1; CHECK(path_pipeline(s, 800, 800, 50, tune), "no walk image, cold features"); }
}

static int print_row(int argc, char** argv) {
    std::vector<char> blob;
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    char buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + n);
    fclose(f);
    (void)argc;
    const int kind = atoi(argv[3]), estimator = atoi(argv[4]), list = atoi(argv[5]), width = atoi(argv[6]), height = atoi(argv[7]), depth = atoi(argv[8]);
    const Tuning tune = read_tuning();
    PreparedScene ps;
    std::string err;
    const int rc = prepare_scene(blob.data(), blob.size(), tune, ps, err);
    if (rc != RTW_OK) { fprintf(stderr, "FAIL: prepare_scene %d: %s\n", rc, err.c_str()); return 1; }
    // (as rtw_hip.hip upload_prepared fills the DScene of a context)
    const SceneScalars& v = ps.sc;
    const SceneFacts& sf = ps.info.facts;
    Scene sc{};
    sc.n_prims = v.n_prims; sc.n_lights = v.n_lights; sc.n_generic = v.n_generic; sc.n_walk_words = v.n_walk_words; sc.n_lds_nodes = v.n_lds_nodes;
    sc.has_tex = v.has_tex; sc.use_bvh = sf.use_bvh ? 1 : 0; sc.n_vol = sf.n_vol; sc.stack_wide = sf.stack_wide ? 1 : 0; sc.n_nodes = (int32_t)sf.n_tree_nodes;
    sc.estimator = RTW_EST_REFERENCE; sc.pdf = v.pdf;
    const bool path = path_pipeline(sc, width, height, depth, tune);  // (render_single decides before the estimator is applied)
    apply_estimator(sc, estimator);
    printf("pipeline=%s k_path=%s k_first=%s\n", path ? "path" : "wavefront", kPathNames[path_row(kind, sc, ps.info.walk_shape, list != 0)],
           kFirstNames[first_row(kind, sc.has_tex, list != 0)]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "rules")) check_rules();
    else if (argc == 9 && !strcmp(argv[1], "row")) return print_row(argc, argv);
    else {
        fprintf(stderr, "usage: variants_check rules | variants_check row <blob> <rng_kind> <estimator> <list> <width> <height> <max_depth>\n");
        return 2;
    }
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    return 0;
}
