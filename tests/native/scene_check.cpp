// CPU check of the host-only scene preparation (raytracing_weekend_amd/csrc/rtw_scene.h: prepare_scene and its stages), compiled and
// run by tests/test_scene_cpu.py. Build with -ffp-contract=off.
// usage: scene_check reject <blob>...           every blob must come back RTW_ERR_BAD_SCENE with a message
//        scene_check dump <blob>...             total size, table offsets and a 64-bit FNV-1a hash of the staged image, one line per blob
//        scene_check check <blob> [listed N]    the invariants below; N: how many hit records must carry the listed-light bit
// RTW_BRUTE_MAX / RTW_LDS_KB are read as the library reads them (read_tuning).
// Tolerance of the unit-length and orthogonality checks: the hit record's vectors are fp32 results of a normalisation (dot, sqrt,
// reciprocal, product: a relative error of about 3 * 2^-24 per component) and of a cross product of two such vectors, so squared lengths
// and dot products, evaluated here in double, stay within 8 * 2^-23 of 1 and 0 (the triple product u . (w x v), of three such vectors: twice that).
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracing_weekend_amd/csrc/rtw_scene.h"
using namespace rtwk;
using namespace rtwdev;

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

template <class T>
static std::vector<T> table(const std::vector<char>& bytes, size_t off, size_t n) {
    std::vector<T> v(n);
    if (off + n * sizeof(T) > bytes.size()) { fprintf(stderr, "FAIL: table at %zu (%zu x %zu B) beyond %zu bytes\n", off, n, sizeof(T), bytes.size()); exit(1); }
    if (n) memcpy((void*)v.data(), bytes.data() + off, n * sizeof(T));
    return v;
}

static double dotd(const float* a, const float* b) { return (double)a[0] * b[0] + (double)a[1] * b[1] + (double)a[2] * b[2]; }

static int check(const std::vector<char>& blob, int want_listed) {
    const Tuning tune = read_tuning();
    PreparedScene ps, again;
    std::string err;
    int rc = prepare_scene(blob.data(), blob.size(), tune, ps, err);
    if (rc != RTW_OK) { fprintf(stderr, "FAIL: prepare_scene %d: %s\n", rc, err.c_str()); return 1; }
    CHECK(prepare_scene(blob.data(), blob.size(), tune, again, err) == RTW_OK, "second call");
    CHECK(ps.image == again.image && memcmp(ps.off, again.off, sizeof ps.off) == 0, "preparing twice gives different bytes");

    rtw_scene_header h;
    memcpy(&h, blob.data(), sizeof h);
    const std::vector<rtw_prim> prims = table<rtw_prim>(blob, h.off_prims, h.n_prims);
    const std::vector<rtw_xform> xforms = table<rtw_xform>(blob, h.off_xforms, h.n_xforms);
    const std::vector<rtw_material> mats = table<rtw_material>(blob, h.off_materials, h.n_materials);
    const std::vector<rtw_texture> texs = table<rtw_texture>(blob, h.off_textures, h.n_textures);
    const SceneScalars& sc = ps.sc;
    const SceneFacts& facts = ps.info.facts;
    const size_t total = ps.image.size();

    // offsets
    CHECK(ps.off[0] == 0 && total % 256 == 0 && total > 0, "total %zu", total);
    for (int t = 0; t < ST_COUNT; t++) {
        CHECK(ps.off[t] % 256 == 0 && ps.off[t] < total, "table %d at %zu of %zu", t, ps.off[t], total);
        if (t > 0) CHECK(ps.off[t] > ps.off[t - 1] || (h.n_prims == 0 && ps.off[t] == ps.off[t - 1]), "table %d at %zu, table %d at %zu", t, ps.off[t], t - 1, ps.off[t - 1]);
    }
    // pipeline choice and counts
    const bool use_bvh = (int)h.n_prims > tune.brute_max;
    CHECK(facts.use_bvh == use_bvh, "use_bvh %d, %u primitives, brute_max %d", (int)facts.use_bvh, h.n_prims, tune.brute_max);
    CHECK(sc.n_prims == (int)h.n_prims && sc.n_lights == (int)h.n_lights && sc.sky_light == h.sky_light && sc.cam_type == h.camera_type, "header scalars");
    CHECK(memcmp(&sc.cam, &h.camera, sizeof h.camera) == 0 && memcmp(&sc.pdf, &h.pdf, sizeof h.pdf) == 0, "camera / pdf");
    CHECK(table<rtw_prim>(ps.image, ps.off[ST_PRIMS], h.n_prims).empty() || memcmp(ps.image.data() + ps.off[ST_PRIMS], prims.data(), prims.size() * sizeof(rtw_prim)) == 0, "prims table");
    CHECK(memcmp(ps.image.data() + ps.off[ST_XFORMS], xforms.data(), xforms.size() * sizeof(rtw_xform)) == 0, "xforms table");

    // order[]: the volumes in index order, then (list scenes) the moving spheres
    std::vector<int32_t> want_order;
    for (uint32_t i = 0; i < h.n_prims; i++) if (rtwbvh::is_volume(prims[i].type)) want_order.push_back((int32_t)i);
    const int n_vol = (int)want_order.size();
    if (!use_bvh) for (uint32_t i = 0; i < h.n_prims; i++) if (prims[i].type == RTW_PRIM_MOVING_SPHERE) want_order.push_back((int32_t)i);
    CHECK(facts.n_vol == n_vol && sc.n_generic == (int)want_order.size() - n_vol, "n_vol %d n_generic %d", facts.n_vol, sc.n_generic);
    CHECK(table<int32_t>(ps.image, ps.off[ST_ORDER], want_order.size()) == want_order, "order[]");

    // candidate lists
    const std::vector<BruteGroup> groups = table<BruteGroup>(ps.image, ps.off[ST_GROUPS], (size_t)sc.n_groups);
    size_t n_recs = 0;
    for (const BruteGroup& g : groups) n_recs += (size_t)(g.n_rx + g.n_ry + g.n_rz + g.n_sph);
    const std::vector<BruteRec> recs = table<BruteRec>(ps.image, ps.off[ST_RECS], n_recs + 1);  // (+ the look-ahead record)
    if (use_bvh) CHECK(sc.n_groups == 0, "a tree scene with %d groups", sc.n_groups);
    else {
        std::vector<int> seen(h.n_prims, 0);
        size_t eligible = 0, at = 0;
        for (uint32_t i = 0; i < h.n_prims; i++) if (!rtwbvh::is_volume(prims[i].type) && prims[i].type != RTW_PRIM_MOVING_SPHERE) eligible++;
        CHECK(n_recs == eligible, "group counts add up to %zu, %zu primitives belong in the lists", n_recs, eligible);
        for (size_t gi = 0; gi < groups.size(); gi++) {
            const BruteGroup& g = groups[gi];
            CHECK(g.first == (int32_t)at, "group %zu first %d, expected %zu", gi, g.first, at);
            for (size_t gj = 0; gj < gi; gj++) CHECK(groups[gj].xform != g.xform, "groups %zu and %zu share transform %d", gj, gi, g.xform);
            const int kinds[4] = {RTW_PRIM_RECT_X, RTW_PRIM_RECT_Y, RTW_PRIM_RECT_Z, RTW_PRIM_SPHERE}, counts[4] = {g.n_rx, g.n_ry, g.n_rz, g.n_sph};
            for (int k = 0; k < 4; k++)
                for (int j = 0; j < counts[k]; j++, at++) {
                    const BruteRec& r = recs[at];
                    if (r.prim < 0 || (uint32_t)r.prim >= h.n_prims) { CHECK(false, "record %zu names primitive %d", at, r.prim); continue; }
                    const rtw_prim& p = prims[r.prim];
                    seen[r.prim]++;
                    CHECK(p.type == kinds[k] && p.xform == g.xform, "record %zu (primitive %d: type %d, transform %d) in group %zu (transform %d) among kind %d", at, r.prim, p.type, p.xform, gi, g.xform, kinds[k]);
                    CHECK(memcmp(&r.a, p.p, (k < 3 ? 5 : 4) * sizeof(float)) == 0, "record %zu parameters", at);
                    if (j > 0) CHECK(recs[at - 1].prim < r.prim, "record %zu out of index order", at);
                }
        }
        for (uint32_t i = 0; i < h.n_prims; i++) {
            const bool listable = !rtwbvh::is_volume(prims[i].type) && prims[i].type != RTW_PRIM_MOVING_SPHERE;
            CHECK(seen[i] == (listable ? 1 : 0), "primitive %u appears in %d records", i, seen[i]);
        }
    }
    // walk image
    const size_t walk_words = 5 * groups.size() + 2 * n_recs + 4;
    const bool want_walk = !use_bvh && sc.n_generic == 0 && !groups.empty() && walk_words <= (size_t)kWalkMaxWords;
    CHECK(sc.n_walk_words == (want_walk ? (int32_t)walk_words : 0), "n_walk_words %d, lists of %zu words, %d generic entries", sc.n_walk_words, walk_words, sc.n_generic);
    if (sc.n_walk_words > 0 && want_walk) {
        const std::vector<uint32_t> walk = table<uint32_t>(ps.image, ps.off[ST_WALK], walk_words * 4);
        const size_t ng = groups.size();
        CHECK(memcmp(walk.data(), groups.data(), ng * sizeof(BruteGroup)) == 0, "walk image: groups");
        for (size_t g = 0; g < ng; g++) CHECK(memcmp(&walk[(2 * ng + 3 * g) * 4], xforms[groups[g].xform].inv, 12 * sizeof(float)) == 0, "walk image: matrix of group %zu", g);
        for (size_t i = 0; i < n_recs; i++) {
            const uint32_t* w = &walk[(5 * ng + 2 * i) * 4];
            CHECK(memcmp(w, &recs[i], 5 * sizeof(float)) == 0 && w[5] == (uint32_t)recs[i].prim + 1u, "walk image: record %zu, tie key %u for primitive %d", i, w[5], recs[i].prim);
        }
        for (size_t k = (5 * ng + 2 * n_recs) * 4; k < walk.size(); k++) CHECK(walk[k] == 0u, "walk image: look-ahead word %zu not zero", k);
    }

    // hit records
    const std::vector<HitRec> hit = table<HitRec>(ps.image, ps.off[ST_HITREC], h.n_prims);
    const std::vector<rtw_light> clights = table<rtw_light>(ps.image, ps.off[ST_CLIGHTS], h.n_lights);
    const double tol = 8.0 * FLT_EPSILON;
    int n_listed = 0, has_motion = 0;
    for (uint32_t i = 0; i < h.n_prims; i++) {
        const rtw_prim& p = prims[i];
        const rtw_material& m = mats[p.material];
        const HitRec& s = hit[i];
        CHECK(s.mat_type == m.type && s.bsdf_eval == m.bsdf_eval && memcmp(&s.param, &m.fuzz_or_eta, 4) == 0 && s.xform == p.xform, "hit record %u: material fields", i);
        int tex_dyn = 0;
        if (m.texture >= 0 && texs[m.texture].type == RTW_TEX_CONSTANT) CHECK(memcmp(&s.r, texs[m.texture].color, 12) == 0, "hit record %u: constant colour", i);
        else if (m.texture >= 0 && texs[m.texture].type != RTW_TEX_NULL) tex_dyn = m.texture + 1;
        CHECK((s.kind >> 8) == tex_dyn, "hit record %u: texture index %d, expected %d", i, s.kind >> 8, tex_dyn);
        const int kind = s.kind & 0x7f;
        if (p.type == RTW_PRIM_MOVING_SPHERE) has_motion = 1;
        if (p.type == RTW_PRIM_SPHERE || p.type == RTW_PRIM_MOVING_SPHERE) {
            CHECK(kind == (p.type == RTW_PRIM_MOVING_SPHERE ? HK_MOVING_SPHERE : p.xform != 0 ? HK_SPHERE_XFORM : HK_SPHERE), "hit record %u: kind %d", i, kind);
            const float inv_r = 1.0f / p.p[3];
            CHECK(memcmp(&s.inv_r, &inv_r, 4) == 0 && memcmp(&s.nx, p.p, 12) == 0, "hit record %u: sphere centre / 1/r", i);
        } else {
            CHECK(kind == HK_CONST_NORMAL, "hit record %u: kind %d", i, kind);
            const float *n = &s.nx, *u = &s.ux, *v = &s.vx, *w = &s.wx;
            CHECK(std::fabs(dotd(n, n) - 1.0) <= tol, "hit record %u: |n|^2 = %.10f", i, dotd(n, n));
            CHECK(std::fabs(dotd(u, u) - 1.0) <= tol && std::fabs(dotd(v, v) - 1.0) <= tol && std::fabs(dotd(w, w) - 1.0) <= tol, "hit record %u: basis lengths %.10f %.10f %.10f", i, dotd(u, u), dotd(v, v), dotd(w, w));
            CHECK(std::fabs(dotd(u, v)) <= tol && std::fabs(dotd(u, w)) <= tol && std::fabs(dotd(v, w)) <= tol, "hit record %u: basis products %.3g %.3g %.3g", i, dotd(u, v), dotd(u, w), dotd(v, w));
            CHECK(std::fabs(dotd(n, w) - 1.0) <= tol, "hit record %u: w is not the normal (%.10f)", i, dotd(n, w));
            const double wxv = ((double)w[1] * v[2] - (double)w[2] * v[1]) * u[0] + ((double)w[2] * v[0] - (double)w[0] * v[2]) * u[1] + ((double)w[0] * v[1] - (double)w[1] * v[0]) * u[2];
            CHECK(std::fabs(wxv - 1.0) <= 2.0 * tol, "hit record %u: u is not cross(w, v) (u . (w x v) = %.10f)", i, wxv);
            // the normal itself: the primitive's axis (volumes: x), flipped, carried by the inverse transpose of its transform (in double)
            double ax[3] = {0, 0, 0}, wn[3], len = 0.0;
            ax[p.type == RTW_PRIM_RECT_Y ? 1 : p.type == RTW_PRIM_RECT_Z ? 2 : 0] = (p.flip && !rtwbvh::is_volume(p.type)) ? -1.0 : 1.0;
            const float* inv = xforms[p.xform].inv;
            for (int a = 0; a < 3; a++) { wn[a] = p.xform != 0 ? inv[a] * ax[0] + inv[4 + a] * ax[1] + inv[8 + a] * ax[2] : ax[a]; len += wn[a] * wn[a]; }
            for (int a = 0; a < 3; a++) CHECK(std::fabs(n[a] - wn[a] / std::sqrt(len)) <= tol, "hit record %u: normal component %d = %.9g, expected %.9g", i, a, n[a], wn[a] / std::sqrt(len));
        }
        if (s.kind & 0x80) {
            n_listed++;
            CHECK(p.type >= RTW_PRIM_RECT_X && p.type <= RTW_PRIM_RECT_Z && p.xform == 0 && m.type == RTW_MAT_DIFFUSE_LIGHT, "hit record %u: listed bit on type %d, transform %d, material type %d", i, p.type, p.xform, m.type);
            bool on_plane = false;
            for (const rtw_light& lt : clights) on_plane = on_plane || memcmp(&lt.position[p.type - RTW_PRIM_RECT_X], &p.p[4], 4) == 0;
            CHECK(on_plane, "hit record %u: no moved light definition sits on its plane", i);
            if (want_listed == 1) CHECK(!clights.empty() && memcmp(&clights[0].position[p.type - RTW_PRIM_RECT_X], &p.p[4], 4) == 0, "clights[0] is not on the plane of primitive %u", i);
        }
    }
    if (want_listed >= 0) CHECK(n_listed == want_listed, "%d listed hit records, expected %d", n_listed, want_listed);
    CHECK(n_listed <= (int)h.n_lights, "%d listed hit records for %u light definitions", n_listed, h.n_lights);
    CHECK(sc.has_motion == has_motion, "has_motion %d", sc.has_motion);

    // bounds: sc.bmin / bmax hold every primitive's world box; the cull bounds are cull_bounds's
    for (uint32_t i = 0; i < h.n_prims; i++) {
        const rtwbvh::Box wb = rtwbvh::world_bounds(prims[i], xforms[prims[i].xform]);
        for (int a = 0; a < 3; a++) CHECK(sc.bmin[a] < wb.mn[a] && sc.bmax[a] > wb.mx[a], "scene bounds do not hold primitive %u on axis %d", i, a);
    }
    float cmin[3], cmax[3];
    const bool cull_ok = cull_bounds(prims.data(), prims.size(), xforms.data(), h.camera, cmin, cmax);
    CHECK(ps.info.cull_ok == cull_ok && (!cull_ok || (memcmp(cmin, ps.info.cull_bmin, 12) == 0 && memcmp(cmax, ps.info.cull_bmax, 12) == 0)), "cull bounds");

    // the tree
    if (!use_bvh) {
        CHECK(facts.stack_depth == 0 && !facts.stack_wide && sc.n_tree == 0 && sc.n_lds_nodes == 0 && sc.n_lds_leaves == 0 && ps.info.lds_bytes == 0 && facts.n_tree_nodes == 0 && facts.n_tree_leaves == 0,
              "a list scene with tree facts: stack %d, %zu nodes, LDS %zu B", facts.stack_depth, facts.n_tree_nodes, ps.info.lds_bytes);
    } else {
        const rtwbvh::Bvh bvh = rtwbvh::build_bvh(prims.data(), h.n_prims, xforms.data());
        CHECK(facts.stack_depth == bvh.stack_need + 2, "stack depth %d, the tree needs %d", facts.stack_depth, bvh.stack_need);
        CHECK(facts.n_tree_nodes == bvh.q4.size() && facts.n_tree_leaves == bvh.n_slots && sc.n_tree == (int32_t)bvh.prim_order.size(), "tree counts");
        int32_t nn = 0, nl = 0;
        const size_t lds = tree_lds_layout(bvh.q4.size(), bvh.n_slots, facts.stack_depth, facts.stack_wide, kBlock, tune.lds_kb * 1024, nn, nl);
        CHECK(ps.info.lds_bytes == lds && sc.n_lds_nodes == nn && sc.n_lds_leaves == nl, "LDS %zu B, %d nodes, %d leaf records; tree_lds_layout says %zu, %d, %d", ps.info.lds_bytes, sc.n_lds_nodes, sc.n_lds_leaves, lds, nn, nl);
        CHECK(facts.stack_wide == ((std::max(bvh.q4.size(), (size_t)bvh.n_slots) << 2) >= 0x7ff0u), "stack_wide %d", (int)facts.stack_wide);
        CHECK(memcmp(ps.image.data() + ps.off[ST_NODES], bvh.q4.data(), bvh.q4.size() * sizeof(rtwbvh::Q4Node)) == 0, "the staged nodes are not the chosen tree's");
        CHECK(table<rtwbvh::LeafRec>(ps.image, ps.off[ST_LEAVES], bvh.leaves.size()).size() == bvh.leaves.size() &&
              memcmp(ps.image.data() + ps.off[ST_LEAVES], bvh.leaves.data(), bvh.leaves.size() * sizeof(rtwbvh::LeafRec)) == 0, "the staged leaf records are not the chosen tree's");
        const std::vector<rtwbvh::WNode> wn = table<rtwbvh::WNode>(ps.image, ps.off[ST_WNODES], bvh.wq4.size());
        size_t grown = 0;
        for (size_t i = 0; i < wn.size(); i++)
            for (int k = 0; k < 4; k++) {
                CHECK(wn[i].ref[k] == bvh.wq4[i].ref[k], "wave node %zu child %d reference", i, k);
                if (wn[i].ref[k] == rtwbvh::kQ4Empty) continue;
                for (int a = 0; a < 3; a++) {
                    CHECK(wn[i].box[k][a] <= bvh.wq4[i].box[k][a] && wn[i].box[k][3 + a] >= bvh.wq4[i].box[k][3 + a], "wave node %zu child %d axis %d does not hold its unpadded box", i, k, a);
                    if (wn[i].box[k][a] < bvh.wq4[i].box[k][a] && wn[i].box[k][3 + a] > bvh.wq4[i].box[k][3 + a]) grown++;
                }
            }
        CHECK(grown > 0, "no wave-node box was padded");
    }
    printf("ok prims %u bvh %d groups %d recs %zu walk_words %d listed %d nodes %d stack %d lds %zu\n", h.n_prims, (int)facts.use_bvh, sc.n_groups, n_recs, sc.n_walk_words, n_listed, (int)facts.n_tree_nodes,
           facts.stack_depth, ps.info.lds_bytes);
    return fails ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: scene_check reject|dump <blob>... | check <blob> [listed N]\n"); return 2; }
    const std::string mode = argv[1];
    const Tuning tune = read_tuning();
    if (mode == "check") return check(read_file(argv[2]), argc >= 5 && strcmp(argv[3], "listed") == 0 ? atoi(argv[4]) : -1);
    for (int i = 2; i < argc; i++) {
        const std::vector<char> blob = read_file(argv[i]);
        PreparedScene ps;
        std::string err;
        const int rc = prepare_scene(blob.data(), blob.size(), tune, ps, err);
        const char* name = strrchr(argv[i], '/') ? strrchr(argv[i], '/') + 1 : argv[i];
        if (mode == "reject") {
            printf("%s: %d %s\n", name, rc, err.c_str());
            if (rc != RTW_ERR_BAD_SCENE || err.empty()) { fprintf(stderr, "FAIL: %s: code %d, message \"%s\"\n", name, rc, err.c_str()); fails++; }
        } else {
            if (rc != RTW_OK) { fprintf(stderr, "FAIL: %s: %d %s\n", name, rc, err.c_str()); fails++; continue; }
            uint64_t hash = 1469598103934665603ull;
            for (char ch : ps.image) hash = (hash ^ (unsigned char)ch) * 1099511628211ull;
            printf("%s total %zu offsets", name, ps.image.size());
            for (int t = 0; t < ST_COUNT; t++) printf(" %zu", ps.off[t]);
            printf(" hash %016llx lds %zu stack %d lds_nodes %d lds_leaves %d walk_words %d\n", (unsigned long long)hash, ps.info.lds_bytes, ps.info.facts.stack_depth, ps.sc.n_lds_nodes, ps.sc.n_lds_leaves, ps.sc.n_walk_words);
        }
    }
    return fails ? 1 : 0;
}
