// CPU check of the list-shape predicate (raytracing_weekend_amd/csrc/rtw_scene.h: WalkShape, walk_shape, SceneInfo::walk_shape), which
// decides whether k_path may run the walk compiled for the Cornell box's lists. Compiled and run by tests/test_shape_cpu.py; may be
// built with -fsanitize=address,undefined.
// usage: shape_check scene <blob> <id>...   prepare_scene on each blob: its SceneInfo::walk_shape must be the id that follows it and the
//                                           predicate's value for the staged group table (0 for a scene with cold features); when
//                                           it is not 0, the staged table must be kShapeCornell's, field by field
//        shape_check edits                  the Cornell group table matches; each edit of it (each of the seven counts +1 and -1, the
//                                           groups swapped, the identity group given a transform, the box group given none, a third
//                                           group appended, the second group dropped, no group) does not
// RTW_BRUTE_MAX / RTW_LDS_KB are read as the library reads them (read_tuning).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracing_weekend_amd/csrc/rtw_scene.h"
using namespace rtwk;
using namespace rtwdev;
using rtwk::scene_detail::walk_shape;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static std::vector<char> read_file(const char* path) {
    std::vector<char> blob;
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    char buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + n);
    fclose(f);
    return blob;
}

// the group table a scene of the Cornell shape stages: transform 0 first, then the box's transform
static std::vector<BruteGroup> cornell_groups() {
    std::vector<BruteGroup> g(2);
    g[0].xform = 0; g[0].first = 0; g[0].n_rx = 2; g[0].n_ry = 3; g[0].n_rz = 1; g[0].n_sph = 1;
    g[1].xform = 1; g[1].first = 7; g[1].n_rx = 2; g[1].n_ry = 2; g[1].n_rz = 2; g[1].n_sph = 0;
    return g;
}

static int check_scene(const char* path, int want) {
    const std::vector<char> blob = read_file(path);
    PreparedScene ps;
    std::string err;
    const int rc = prepare_scene(blob.data(), blob.size(), read_tuning(), ps, err);
    if (rc != RTW_OK) { fprintf(stderr, "FAIL: prepare_scene %d: %s\n", rc, err.c_str()); return 1; }
    const int got = ps.info.walk_shape;
    printf("%s: walk_shape %d, %d groups, %d walk words\n", path, got, ps.sc.n_groups, ps.sc.n_walk_words);
    CHECK(got == want, "%s: walk_shape %d, expected %d", path, got, want);
    std::vector<BruteGroup> groups((size_t)ps.sc.n_groups);
    if (!groups.empty()) memcpy(groups.data(), ps.image.data() + ps.off[ST_GROUPS], groups.size() * sizeof(BruteGroup));
    // (a scene with cold features - textures, media, another camera - never runs the fixed-shape walks: its id is 0 whatever its lists)
    CHECK(got == (ps.sc.n_walk_words > 0 && ps.sc.has_tex == 0 ? walk_shape(groups) : WALK_SHAPE_NONE), "%s: the stored id is not the staged table's", path);
    if (got != WALK_SHAPE_NONE) {
        const std::vector<BruteGroup> c = cornell_groups();
        CHECK(got == WALK_SHAPE_CORNELL && groups.size() == c.size() && ps.sc.n_walk_words > 0, "%zu groups", groups.size());
        for (size_t g = 0; g < groups.size() && g < c.size(); g++) {
            CHECK((groups[g].xform != 0) == (c[g].xform != 0) && groups[g].first == c[g].first && groups[g].n_rx == c[g].n_rx && groups[g].n_ry == c[g].n_ry &&
                  groups[g].n_rz == c[g].n_rz && groups[g].n_sph == c[g].n_sph, "group %zu: xform %d first %d counts %d %d %d %d", g, groups[g].xform, groups[g].first,
                  groups[g].n_rx, groups[g].n_ry, groups[g].n_rz, groups[g].n_sph);
        }
        // the walk image the fixed-shape walk indexes by the shape alone: 5 words per group, 2 per record, 4 of padding
        CHECK(ps.sc.n_walk_words == 5 * kShapeCornell.n_groups + 2 * walk_shape_recs(kShapeCornell, kShapeCornell.n_groups) + 4, "%d walk words", ps.sc.n_walk_words);
    }
    return 0;
}

static void check_edits() {
    const std::vector<BruteGroup> c = cornell_groups();
    CHECK(walk_shape(c) == WALK_SHAPE_CORNELL, "the Cornell table itself");
    int n_edits = 0;
    auto rejected = [&](const std::vector<BruteGroup>& g, const char* what, int a = 0, int b = 0) {
        n_edits++;
        CHECK(walk_shape(g) == WALK_SHAPE_NONE, "%s (%d, %d) is taken for the Cornell shape", what, a, b);
    };
    int32_t BruteGroup::* const counts[4] = {&BruteGroup::n_rx, &BruteGroup::n_ry, &BruteGroup::n_rz, &BruteGroup::n_sph};
    for (int g = 0; g < 2; g++)
        for (int k = 0; k < 4; k++) {
            if (g == 1 && k == 3) {  // (the box has no sphere: its eighth count can only grow)
                std::vector<BruteGroup> e = c;
                e[g].*counts[k] += 1;
                rejected(e, "box sphere count + 1");
                continue;
            }
            for (int delta = -1; delta <= 1; delta += 2) {
                std::vector<BruteGroup> e = c;
                e[g].*counts[k] += delta;
                for (size_t j = g + 1; j < e.size(); j++) e[j].first += delta;  // (as build_lists would number the records)
                rejected(e, "count edited", g * 4 + k, delta);
            }
        }
    {   std::vector<BruteGroup> e = {c[1], c[0]}; rejected(e, "groups swapped"); }
    {   std::vector<BruteGroup> e = c; e[0].xform = 2; rejected(e, "identity group given a transform"); }
    {   std::vector<BruteGroup> e = c; e[1].xform = 0; rejected(e, "box group given none"); }
    {   std::vector<BruteGroup> e = c; BruteGroup g{}; g.xform = 2; g.first = 13; e.push_back(g); rejected(e, "an empty third group appended"); }
    {   std::vector<BruteGroup> e = c; BruteGroup g = c[1]; g.xform = 2; g.first = 13; e.push_back(g); rejected(e, "a third group appended"); }
    {   std::vector<BruteGroup> e = {c[0]}; rejected(e, "the box group dropped"); }
    rejected(std::vector<BruteGroup>(), "no group");
    printf("edits: %d group tables, none taken for the Cornell shape\n", n_edits);
    CHECK(n_edits == 14 + 1 + 7, "%d edits", n_edits);
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "edits")) {
        check_edits();
    } else if (argc >= 4 && !strcmp(argv[1], "scene") && (argc - 2) % 2 == 0) {
        for (int i = 2; i + 1 < argc; i += 2)
            if (check_scene(argv[i], atoi(argv[i + 1]))) return 1;
    } else {
        fprintf(stderr, "usage: shape_check scene <blob> <id>... | shape_check edits\n");
        return 2;
    }
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    return 0;
}
