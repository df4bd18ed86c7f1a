// rtw_scene.h — what rtw_upload_scene does before it touches a device: the scene blob parsed and validated, the light definitions
// matched to their rectangles, one hit record baked per primitive, the small scenes' candidate lists and k_path's walk image, the tree
// and its padded wave-walk nodes, and all tables laid out in one staged image (prepare_scene). Also the plain records of that image
// which the kernels read (rtw_device.h includes this file). No HIP in here: rtw_hip.hip copies the image to each device and binds
// DScene's pointers from the offsets; tests/native/scene_check.cpp pins the stages with g++.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtw.h"
#include "rtw_bvh.h"
#include "rtw_plan.h"

namespace rtwdev {

// Per-primitive hit record baked at upload (96 B, fetched with a burst of 16-byte loads once
// the closest hit is known): material + its constant texture colour (texture/constantTexture.cu:5-10,
// nullTexture.cu:7-12) and everything the shading normal needs, so that no primitive / transform
// record has to be re-read per lane after traversal.
enum { HK_CONST_NORMAL = 0, HK_SPHERE = 1, HK_MOVING_SPHERE = 2, HK_SPHERE_XFORM = 3 };
struct HitRec {
    int32_t mat_type;   // rtw_material_type
    int32_t bsdf_eval;
    float param;        // fuzz or eta
    int32_t kind;       // HK_* | listed light << 7 | (index of a non-constant texture + 1) << 8
    float r, g, b;      // texture colour
    float inv_r;        // spheres: 1/radius (IEEE division, done once on the host)
    float nx, ny, nz;   // HK_CONST_NORMAL: world shading normal (rectangles, volumes); spheres: centre
    int32_t xform;
    // HK_CONST_NORMAL: the orthonormal basis onb::buildFromW(normal) of lib/onb.cuh:20-32, computed once on the
    // host with the same fp32 operations (u = cross(w,v), v = normalize(cross(w,a)), w = normalize(n))
    float ux, uy, uz; int32_t tex_dyn;  // (filled by load_hitrec from kind's high bits; -1 = constant colour in r, g, b)
    float vx, vy, vz; int32_t listed;    // (from kind bit 7) an emitting rectangle a light definition describes
    float wx, wy, wz, pad2;
};

// Small-scene candidate lists, built at upload (rtw_upload_scene). 32-byte records so that one
// s_load_dwordx8 brings a whole candidate into SGPRs; rectangles are sorted by axis inside a group so
// the inner loops contain no per-candidate kind dispatch at all.
struct BruteGroup {
    int32_t xform;
    int32_t first;                 // first record of the group in recs[]
    int32_t n_rx, n_ry, n_rz, n_sph;
    int32_t pad0, pad1;
};
struct BruteRec {
    float a, b, c, d, e;           // rect: a0,a1,b0,b1,k   sphere: cx,cy,cz,r,-
    int32_t prim;
    int32_t pad0, pad1;
};

constexpr int kWalkMaxWords = 400;  // k_path's walk image (rtw_device.h walk_lds): 6.4 KB of LDS; scenes whose lists are larger use the wavefront kernels

// List shapes k_path has a walk compiled for (rtw_device.h walk_lds<ANY_HIT, SHAPE>, DESIGN.md 4.1 "The metric scene's list
// shape is a compile-time fact"): the number of groups and, per group, whether it has a transform and its four counts - everything the
// walk's control flow depends on. Shape id 0 is "none": the walk that reads the image's group headers.
struct WalkShapeGroup { bool xform; int n[4]; };  // n: x-, y-, z-rectangles, spheres
struct WalkShape { int n_groups; WalkShapeGroup g[2]; };
enum { WALK_SHAPE_NONE = 0, WALK_SHAPE_CORNELL = 1 };
// the reference's Cornell box (host/ioScene.h CornellBox): walls, floor, ceiling, light and the sphere; then the rotated box
constexpr WalkShape kShapeCornell = {2, {{false, {2, 3, 1, 1}}, {true, {2, 2, 2, 0}}}};
constexpr int walk_shape_recs(const WalkShape& s, int n_groups) {  // records in the first n_groups groups
    int n = 0;
    for (int g = 0; g < n_groups; g++) for (int k = 0; k < 4; k++) n += s.g[g].n[k];
    return n;
}
constexpr int walk_shape_group(const WalkShape& s, int ri) {  // the group record ri (of the image's record stream) lies in
    int g = 0;
    while (g + 1 < s.n_groups && ri >= walk_shape_recs(s, g + 1)) g++;
    return g;
}
constexpr int walk_shape_kind(const WalkShape& s, int ri) {   // and its list there: 0, 1, 2: x-, y-, z-rectangles, 3: spheres
    const int g = walk_shape_group(s, ri);
    int k = 0, first = walk_shape_recs(s, g);
    while (k < 3 && ri >= first + s.g[g].n[k]) first += s.g[g].n[k++];
    return k;
}
static_assert(5 * kShapeCornell.n_groups + 2 * walk_shape_recs(kShapeCornell, kShapeCornell.n_groups) + 4 <= kWalkMaxWords, "a compiled shape has a walk image");
constexpr bool walk_shape_is(const WalkShape& s, const BruteGroup* groups, size_t n_groups) {
    if (n_groups != (size_t)s.n_groups) return false;
    for (int g = 0; g < s.n_groups; g++) {
        const BruteGroup& G = groups[g];
        if ((G.xform != 0) != s.g[g].xform || G.n_rx != s.g[g].n[0] || G.n_ry != s.g[g].n[1] || G.n_rz != s.g[g].n[2] || G.n_sph != s.g[g].n[3]) return false;
    }
    return true;
}
}  // namespace rtwdev

namespace rtwk {

// the tables of the staged image, in the order they lie in it
enum SceneTable { ST_PRIMS, ST_XFORMS, ST_HITREC, ST_LIGHTS, ST_CLIGHTS, ST_NODES, ST_WNODES, ST_LEAVES, ST_ORDER, ST_GROUPS, ST_RECS, ST_TEXS, ST_TEXDATA,
                  ST_WALK, ST_COUNT };

// the members of DScene (rtw_device.h) that the upload decides, under DScene's names; those that SceneFacts states are taken from there
struct SceneScalars {
    int32_t n_prims, n_tree, n_lights, sky_light, has_motion, n_groups, n_generic, n_walk_words;
    int32_t n_lds_nodes, has_tex, noise_lds_data, n_lds_leaves, cam_type;
    float bmin[3], bmax[3];
    rtw_camera cam;
    rtw_pdf pdf;
};
// what the host keeps of the uploaded scene for its renders
struct SceneInfo {
    SceneFacts facts;                   // what plan_wavefront looks at
    size_t lds_bytes;                   // dynamic LDS of k_first and the tree walks at kBlock threads: stacks + staged nodes and leaf records
    bool cull_ok;                       // cull_bmin / cull_bmax hold the bounds the empty-pixel cull projects (rtw_plan.h cull_bounds)
    float cull_bmin[3], cull_bmax[3];
    int walk_shape;                     // WALK_SHAPE_*: the compiled list shape of the walk image (walk_shape below); 0: none, no walk image, or cold features
};
struct PreparedScene {
    std::vector<char> image;            // one device allocation's worth: 256-byte aligned tables, zero padding
    size_t off[ST_COUNT];
    SceneScalars sc;
    SceneInfo info;
};

namespace scene_detail {
using namespace rtwdev;

struct Tables {
    rtw_scene_header h;
    std::vector<rtw_prim> prims;
    std::vector<rtw_xform> xforms;
    std::vector<rtw_material> mats;
    std::vector<rtw_texture> texs;
    std::vector<rtw_light> lights;
    std::vector<uint32_t> texdata;
};

inline int fail(std::string& err, const char* msg, int code = RTW_ERR_BAD_SCENE) {
    err = msg;
    return code;
}

// ---- 1, 2: header, table ranges and alignment, then every record (the test-side checker applies the same rules)
inline int parse_scene(const void* blob, size_t bytes, Tables& s, std::string& err) {
    rtw_scene_header& h = s.h;
    if (!blob || bytes < sizeof h) return fail(err, "scene blob too small");
    memcpy(&h, blob, sizeof h);
    if (h.magic != RTW_SCENE_MAGIC || h.version != RTW_SCENE_VERSION || h.total_bytes > bytes) return fail(err, "bad scene header (magic/version/size)");
    const char* b = (const char*)blob;
    bool ranges = h.n_xforms >= 1;
    auto fetch = [&](auto& v, uint32_t off, uint32_t n) {  // (copies only once every table's range has held)
        ranges = ranges && (size_t)off + (size_t)n * sizeof(v[0]) <= bytes;
        if (!ranges) return;
        v.resize(n);
        if (n) memcpy(v.data(), b + off, n * sizeof(v[0]));
    };
    fetch(s.prims, h.off_prims, h.n_prims);
    fetch(s.xforms, h.off_xforms, h.n_xforms);
    fetch(s.mats, h.off_materials, h.n_materials);
    fetch(s.texs, h.off_textures, h.n_textures);
    fetch(s.lights, h.off_lights, h.n_lights);
    if (!ranges) return fail(err, "scene table out of range");
    if (h.camera_type < RTW_CAM_PERSPECTIVE || h.camera_type > RTW_CAM_ORTHOGRAPHIC) return fail(err, "unknown camera type");
    if ((h.off_prims | h.off_xforms | h.off_materials | h.off_textures | h.off_lights | h.off_texdata) & 15u) return fail(err, "scene table not 16-byte aligned");

    for (const rtw_xform& x : s.xforms)
        for (int k = 0; k < 12; k++) if (!std::isfinite(x.m[k]) || !std::isfinite(x.inv[k])) return fail(err, "transform not finite");
    for (const rtw_material& m : s.mats)
        if (m.texture >= (int32_t)h.n_textures) return fail(err, "material texture out of range");
    if (h.off_texdata) {
        if ((size_t)h.off_texdata + (size_t)h.texdata_bytes > bytes) return fail(err, "texture data section out of range");
        s.texdata.resize(h.texdata_bytes / 4u);
        if (!s.texdata.empty()) memcpy(s.texdata.data(), b + h.off_texdata, s.texdata.size() * 4u);
    }
    const size_t n_words = s.texdata.size();
    for (const rtw_texture& t : s.texs) {
        if (t.type == RTW_TEX_CHECKER) {
            if (t.odd < 0 || t.even < 0 || (uint32_t)t.odd >= h.n_textures || (uint32_t)t.even >= h.n_textures || s.texs[t.odd].type == RTW_TEX_CHECKER ||
                s.texs[t.even].type == RTW_TEX_CHECKER)
                return fail(err, "checker texture children out of range or nested");
        } else if (t.type == RTW_TEX_NOISE) {
            if ((size_t)t.data + 1536u > n_words) return fail(err, "noise texture tables out of range");
        } else if (t.type == RTW_TEX_IMAGE) {
            if ((size_t)t.data + 2u > n_words) return fail(err, "image texture out of range");
            const uint32_t iw = s.texdata[t.data], ih = s.texdata[t.data + 1];
            if (iw == 0 || ih == 0 || iw > 32768u || ih > 32768u || (size_t)t.data + 2u + (size_t)iw * ih > n_words) return fail(err, "image texture out of range");
        } else if (t.type != RTW_TEX_CONSTANT && t.type != RTW_TEX_NULL) {
            return fail(err, "unknown texture type");
        }
    }
    for (const rtw_prim& p : s.prims) {
        if (p.type < RTW_PRIM_SPHERE || p.type > RTW_PRIM_VOLUME_SPHERE) return fail(err, "unknown primitive type");
        if (p.xform < 0 || (uint32_t)p.xform >= h.n_xforms) return fail(err, "primitive xform out of range");
        if (p.material < 0 || (uint32_t)p.material >= h.n_materials) return fail(err, "primitive material out of range");
        for (int k = 0; k < 12; k++) if (!std::isfinite(p.p[k])) return fail(err, "primitive parameter not finite");
    }
    return RTW_OK;
}

// ---- 3: RTW_EST_CORRECTED: light definitions moved onto the emitting rectangles they describe, and which primitives those
// are (same matching rule as the CPU checker: same normal axis and in-plane extent, plane within 1 % of the longer edge)
inline void match_lights(const Tables& s, std::vector<rtw_light>& clights, std::vector<uint8_t>& listed) {
    clights = s.lights;
    listed.assign(s.prims.size(), 0);
    for (rtw_light& lt : clights)
        for (size_t j = 0; j < s.prims.size(); j++) {
            const rtw_prim& pr = s.prims[j];
            if (pr.type < RTW_PRIM_RECT_X || pr.type > RTW_PRIM_RECT_Z || pr.xform != 0 || s.mats[pr.material].type != RTW_MAT_DIFFUSE_LIGHT) continue;
            const int ax = pr.type - RTW_PRIM_RECT_X, aa = ax == 0 ? 1 : 0, ab = ax == 2 ? 1 : 2;
            const float ea = pr.p[1] - pr.p[0], eb = pr.p[3] - pr.p[2];
            float u[3] = {0.f, 0.f, 0.f}, v[3] = {0.f, 0.f, 0.f};
            u[aa] = ea; v[ab] = eb;
            bool same = lt.position[aa] == pr.p[0] && lt.position[ab] == pr.p[2];
            for (int k = 0; k < 3; k++) if (lt.vec_u[k] != u[k] || lt.vec_v[k] != v[k]) same = false;
            if (!same || !(std::fabs(lt.position[ax] - pr.p[4]) <= 0.01f * std::fmax(ea, eb))) continue;
            lt.position[ax] = pr.p[4];
            listed[j] = 1;
            break;
        }
}

// ---- 4: one hit record per primitive; the fp32 operations and their order are the ones the device / the oracle would use per hit
inline void normalize3(const float* a3, float* o3) {
    const float dd = std::fmaf(a3[2], a3[2], std::fmaf(a3[1], a3[1], a3[0] * a3[0]));
    const float inv = 1.0f / std::sqrt(dd);
    for (int k = 0; k < 3; k++) o3[k] = a3[k] * inv;
}
inline void cross3(const float* a3, const float* b3, float* o3) {
    o3[0] = std::fmaf(a3[1], b3[2], -(a3[2] * b3[1]));
    o3[1] = std::fmaf(a3[2], b3[0], -(a3[0] * b3[2]));
    o3[2] = std::fmaf(a3[0], b3[1], -(a3[1] * b3[0]));
}
inline HitRec bake_hitrec(const Tables& s, size_t i, bool listed) {
    const rtw_prim& p = s.prims[i];
    const rtw_material& m = s.mats[p.material];
    HitRec r{};
    r.mat_type = m.type; r.bsdf_eval = m.bsdf_eval; r.param = m.fuzz_or_eta; r.xform = p.xform;
    if (p.type == RTW_PRIM_SPHERE || p.type == RTW_PRIM_MOVING_SPHERE) {
        r.kind = p.type == RTW_PRIM_MOVING_SPHERE ? HK_MOVING_SPHERE : (p.xform != 0 ? HK_SPHERE_XFORM : HK_SPHERE);
        r.nx = p.p[0]; r.ny = p.p[1]; r.nz = p.p[2];
        r.inv_r = 1.0f / p.p[3];
    } else {
        r.kind = HK_CONST_NORMAL;
        float n[3] = {0.f, 0.f, 0.f};
        n[p.type == RTW_PRIM_RECT_Y ? 1 : p.type == RTW_PRIM_RECT_Z ? 2 : 0] = 1.f;  // volumes report (1,0,0)
        if (p.flip && !rtwbvh::is_volume(p.type)) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        if (p.xform != 0) {  // the normal under the inverse transpose
            const float* inv = s.xforms[p.xform].inv;
            float v[3];
            for (int k = 0; k < 3; k++) v[k] = std::fmaf(inv[k], n[0], std::fmaf(inv[4 + k], n[1], inv[8 + k] * n[2]));
            normalize3(v, n);
        }
        // onb::buildFromW (lib/onb.cuh:20-32)
        float w[3], t[3], u[3], v[3];
        normalize3(n, w);
        const float a[3] = {(w[0] > 0.9f || w[0] < -0.9f) ? 0.f : 1.f, (w[0] > 0.9f || w[0] < -0.9f) ? 1.f : 0.f, 0.f};
        cross3(w, a, t);
        normalize3(t, v);
        cross3(w, v, u);
        r.nx = n[0]; r.ny = n[1]; r.nz = n[2];
        r.ux = u[0]; r.uy = u[1]; r.uz = u[2];
        r.vx = v[0]; r.vy = v[1]; r.vz = v[2];
        r.wx = w[0]; r.wy = w[1]; r.wz = w[2];
    }
    if (m.texture >= 0) {
        const rtw_texture& t = s.texs[m.texture];
        if (t.type == RTW_TEX_CONSTANT) { r.r = t.color[0]; r.g = t.color[1]; r.b = t.color[2]; }
        else if (t.type != RTW_TEX_NULL) r.kind |= (m.texture + 1) << 8;  // checker / noise / image: evaluated per hit
    }
    if (listed) r.kind |= 0x80;
    return r;
}

// ---- 5: order[]: the volumes (index order), then -- small scenes only -- the moving spheres, which keep the generic test; the other
// primitives of a small scene regrouped by instance transform, rectangles by axis
inline void build_lists(const Tables& s, bool use_bvh, std::vector<int32_t>& order, int& n_vol, std::vector<BruteGroup>& groups, std::vector<BruteRec>& recs) {
    const size_t n = s.prims.size();
    for (size_t i = 0; i < n; i++) if (rtwbvh::is_volume(s.prims[i].type)) order.push_back((int32_t)i);
    n_vol = (int)order.size();
    if (use_bvh) return;
    for (size_t i = 0; i < n; i++) if (s.prims[i].type == RTW_PRIM_MOVING_SPHERE) order.push_back((int32_t)i);
    auto listable = [](int t) { return !rtwbvh::is_volume(t) && t != RTW_PRIM_MOVING_SPHERE; };
    for (size_t first = 0; first < n; first++) {  // a group per transform, in the order the transforms first appear
        const int xf = s.prims[first].xform;
        if (!listable(s.prims[first].type) || std::any_of(groups.begin(), groups.end(), [&](const BruteGroup& g) { return g.xform == xf; })) continue;
        BruteGroup g{};
        g.xform = xf;
        g.first = (int32_t)recs.size();
        const int kinds[4] = {RTW_PRIM_RECT_X, RTW_PRIM_RECT_Y, RTW_PRIM_RECT_Z, RTW_PRIM_SPHERE};
        int32_t* counts[4] = {&g.n_rx, &g.n_ry, &g.n_rz, &g.n_sph};
        for (int k = 0; k < 4; k++)
            for (size_t i = first; i < n; i++) {
                const rtw_prim& p = s.prims[i];
                if (p.type != kinds[k] || p.xform != xf) continue;
                BruteRec r{};
                r.a = p.p[0]; r.b = p.p[1]; r.c = p.p[2]; r.d = p.p[3];
                if (k < 3) r.e = p.p[4];
                r.prim = (int32_t)i;
                recs.push_back(r);
                (*counts[k])++;
            }
        groups.push_back(g);
    }
}

// ---- 6: k_path's LDS image of the same lists (rtw_device.h walk_lds): groups, their world->object matrices, records with the walk's tie
// key (prim + 1) in place of prim, + 4 words: the reader fetches up to two records ahead. Empty when the lists are larger than the kernel's
// LDS. (A rectangle with lo > hi can never be hit under either form of the range test, so none needs removing.)
inline std::vector<uint32_t> walk_image(const Tables& s, const std::vector<BruteGroup>& groups, const std::vector<BruteRec>& recs) {
    static_assert(sizeof(BruteGroup) == 32 && sizeof(BruteRec) == 32, "walk image layout");
    const size_t ng = groups.size(), words = 5 * ng + 2 * recs.size() + 4;
    if (ng == 0 || words > (size_t)kWalkMaxWords) return {};
    std::vector<uint32_t> walk(words * 4, 0u);
    memcpy(walk.data(), groups.data(), ng * sizeof(BruteGroup));
    for (size_t g = 0; g < ng; g++) memcpy(&walk[(2 * ng + 3 * g) * 4], s.xforms[groups[g].xform].inv, 12 * sizeof(float));
    for (size_t i = 0; i < recs.size(); i++) {
        memcpy(&walk[(5 * ng + 2 * i) * 4], &recs[i], sizeof(BruteRec));
        walk[(5 * ng + 2 * i) * 4 + 5] = (uint32_t)recs[i].prim + 1u;
    }
    return walk;
}

// ---- 6b: the id of the compiled shape (WalkShape above) the group table matches exactly (groups, their order, identity or transformed, all four counts), else 0
inline int walk_shape(const std::vector<BruteGroup>& groups) {
    return walk_shape_is(kShapeCornell, groups.data(), groups.size()) ? WALK_SHAPE_CORNELL : WALK_SHAPE_NONE;
}

// ---- 7: the wave-coherent walk's nodes: fp32 child boxes, padded for its plane arithmetic. It computes a plane's distance as
// fma(plane, 1/d, -(o * 1/d)): the rounding of o * 1/d displaces a plane by about ulp(|o|) in space, so the boxes grow by
// 2^-19 of the largest coordinate around (`big`: scene bounds, camera origin; the primitives' own bounds carry 1e-4 already)
inline void pad_wave_nodes(std::vector<rtwbvh::WNode>& wq4, float big) {
    const float pad = 1.0e-4f + big * (1.0f / 524288.0f);
    for (rtwbvh::WNode& w : wq4)
        for (int k = 0; k < 4; k++)
            if (w.ref[k] != rtwbvh::kQ4Empty)
                for (int a = 0; a < 3; a++) { w.box[k][a] -= pad; w.box[k][3 + a] += pad; }
}

// ---- 8: a table is appended to the image once: at the next 256-byte boundary, room for at least min_elems elements and `extra` more than
// it holds (what the kernels may read beyond a table's end), zero filled
template <class T>
void stage(PreparedScene& out, SceneTable t, const std::vector<T>& v, size_t min_elems = 0, size_t extra = 0) {
    out.off[t] = out.image.size();
    out.image.resize((out.off[t] + (std::max(v.size(), min_elems) + extra) * sizeof(T) + 255u) & ~size_t(255), 0);
    if (!v.empty()) memcpy(out.image.data() + out.off[t], v.data(), v.size() * sizeof(T));
}

}  // namespace scene_detail

// The scene blob -> everything an upload needs, or an error code (RTW_ERR_BAD_SCENE, RTW_ERR_UNSUPPORTED) and its message. Reads
// tune.brute_max, tune.lds_kb and tune.verbose (the tree line on stderr).
inline int prepare_scene(const void* blob, size_t bytes, const Tuning& tune, PreparedScene& out, std::string& err) {
    using namespace scene_detail;
    Tables s;
    if (const int rc = parse_scene(blob, bytes, s, err)) return rc;
    const rtw_scene_header& h = s.h;
    out = PreparedScene{};
    SceneScalars& sc = out.sc;
    SceneFacts& facts = out.info.facts;

    std::vector<rtw_light> clights;
    std::vector<uint8_t> listed;
    match_lights(s, clights, listed);
    std::vector<HitRec> hitrec(h.n_prims);
    bool dyn_tex = false;
    rtwbvh::Box all;      // world bounds of everything (volumes and motion sweeps included)
    float big = 1.0f;     // the largest coordinate around
    for (uint32_t i = 0; i < h.n_prims; i++) {
        hitrec[i] = bake_hitrec(s, i, listed[i] != 0);
        dyn_tex = dyn_tex || (hitrec[i].kind >> 8) != 0;
        if (s.prims[i].type == RTW_PRIM_MOVING_SPHERE) sc.has_motion = 1;
        const rtwbvh::Box wb = rtwbvh::world_bounds(s.prims[i], s.xforms[s.prims[i].xform]);
        all.add(wb);
        for (int a = 0; a < 3; a++) big = std::max(big, std::max(std::fabs(wb.mn[a]), std::fabs(wb.mx[a])));
    }
    for (int a = 0; a < 3; a++) big = std::max(big, std::fabs(h.camera.origin[a]) + std::fabs(h.camera.lens_radius));

    facts.use_bvh = (int)h.n_prims > tune.brute_max;
    std::vector<int32_t> order;
    std::vector<BruteGroup> groups;
    std::vector<BruteRec> recs;
    build_lists(s, facts.use_bvh, order, facts.n_vol, groups, recs);
    sc.n_generic = (int)order.size() - facts.n_vol;
    const std::vector<uint32_t> walk = !facts.use_bvh && sc.n_generic == 0 ? walk_image(s, groups, recs) : std::vector<uint32_t>();
    rtwbvh::Bvh bvh;
    if (facts.use_bvh) {
        bvh = rtwbvh::build_bvh(s.prims.data(), h.n_prims, s.xforms.data());
        if (bvh.stack_need > 95) return fail(err, "tree deeper than the LDS traversal stack", RTW_ERR_UNSUPPORTED);
        if (bvh.max_exp > 60) return fail(err, "scene extent beyond 1e20", RTW_ERR_UNSUPPORTED);
        pad_wave_nodes(bvh.wq4, big);
        // LDS per block: the traversal stacks (16-bit entries when every reference fits), then as many leading (breadth-first)
        // tree nodes and, behind them, leaf records as fit the budget
        facts.stack_depth = bvh.stack_need + 2;  // + the two rows under the stack that end a walk
        facts.stack_wide = (std::max(bvh.q4.size(), (size_t)bvh.n_slots) << 2) >= 0x7ff0u;  // 16-bit entries are read sign-extended
        facts.n_tree_nodes = bvh.q4.size();
        facts.n_tree_leaves = bvh.n_slots;
        out.info.lds_bytes = tree_lds_layout(facts.n_tree_nodes, facts.n_tree_leaves, facts.stack_depth, facts.stack_wide, kBlock, tune.lds_kb * 1024, sc.n_lds_nodes, sc.n_lds_leaves);
        if (tune.verbose) fprintf(stderr, "[rtw] tree (SAH bins %d, collapse %d, sample-walk cost %.3f): %zu nodes, %zu leaf records, stack %d x %d bit; LDS %zu B: %d nodes, %d leaf records\n", bvh.bins, bvh.collapse_kind, bvh.cost,
                                  bvh.q4.size(), (size_t)bvh.n_slots, facts.stack_depth, facts.stack_wide ? 32 : 16, out.info.lds_bytes, sc.n_lds_nodes, sc.n_lds_leaves);
    }

    stage(out, ST_PRIMS, s.prims);
    stage(out, ST_XFORMS, s.xforms);
    stage(out, ST_HITREC, hitrec);
    stage(out, ST_LIGHTS, s.lights, 1);
    stage(out, ST_CLIGHTS, clights, 1);
    stage(out, ST_NODES, bvh.q4, 1);
    stage(out, ST_WNODES, bvh.wq4, 1);
    stage(out, ST_LEAVES, bvh.leaves, 1);
    stage(out, ST_ORDER, order, 1);
    stage(out, ST_GROUPS, groups, 1);
    stage(out, ST_RECS, recs, 0, 1);  // + 1: traverse_brute reads one record ahead
    stage(out, ST_TEXS, s.texs, 1);
    stage(out, ST_TEXDATA, s.texdata, 1);
    stage(out, ST_WALK, walk, 1);

    sc.n_prims = (int)h.n_prims;
    sc.n_tree = (int)bvh.prim_order.size();
    sc.n_lights = (int)h.n_lights;
    sc.sky_light = h.sky_light;
    sc.n_groups = (int)groups.size();
    sc.n_walk_words = (int32_t)(walk.size() / 4);
    // selects the kernel instantiations that contain the cold features: textures, media, (k_path) moving spheres in the brute lists,
    // camera kinds other than the reference's lens-free perspective camera
    sc.has_tex = (dyn_tex || facts.n_vol > 0 || sc.n_generic > 0 || h.camera_type != RTW_CAM_PERSPECTIVE || h.camera.lens_radius != 0.0f) ? 1 : 0;
    // (only k_path's instantiation without the cold features has fixed-shape walks)
    out.info.walk_shape = (walk.empty() || sc.has_tex != 0) ? WALK_SHAPE_NONE : walk_shape(groups);
    sc.noise_lds_data = -1;  // the first noise texture some primitive shows gets its tables staged in LDS
    for (uint32_t i = 0; i < h.n_prims && sc.noise_lds_data < 0; i++) {
        int ti = s.mats[s.prims[i].material].texture;
        if (ti < 0) continue;
        if (s.texs[ti].type == RTW_TEX_CHECKER) ti = s.texs[s.texs[ti].odd].type == RTW_TEX_NOISE ? s.texs[ti].odd : s.texs[ti].even;
        if (s.texs[ti].type == RTW_TEX_NOISE) sc.noise_lds_data = (int32_t)s.texs[ti].data;
    }
    {   // k_first's wave-uniform miss test: the bounds of everything, padded by 1 % of the diagonal
        float diag = 0.f;
        for (int a = 0; a < 3; a++) diag += (all.mx[a] - all.mn[a]) * (all.mx[a] - all.mn[a]);
        const float pad = 0.01f * std::sqrt(diag) + 1.0f;
        for (int a = 0; a < 3; a++) { sc.bmin[a] = all.mn[a] - pad; sc.bmax[a] = all.mx[a] + pad; }
    }
    sc.cam = h.camera;
    sc.pdf = h.pdf;
    sc.cam_type = h.camera_type;
    out.info.cull_ok = cull_bounds(s.prims.data(), h.n_prims, s.xforms.data(), h.camera, out.info.cull_bmin, out.info.cull_bmax);
    return RTW_OK;
}

}  // namespace rtwk
