// ref_programs_wrap.cpp — TEST INFRASTRUCTURE. Runs the reference's OWN device programs on the CPU as a referee for the
// oracle, the float64 law files and the kernels. Every reference .cu is compiled from where it lies under $(REF) (never copied),
// each inside a namespace of its own (they redefine emitted(), scatteringPdf(), get_sphere_uv() ...), against the stand-in
// headers of oracle/ref_shim/. This file adds: a host emulation of the OptiX device API those programs call (namespace refemu),
// the marshalling of this project's scene blob (include/rtw.h) into the reference's launch structures, and a C ABI.
// Built by `make -C oracle ref` into oracle/_ref/libref_programs.so (-ffp-contract=off) and libref_programs_fma.so
// (-ffp-contract=fast -mfma); what the library computes is recorded in tests/golden/ref_programs/*.npz
// (tests/golden/make_ref_programs.py). shaders/anyhit.cu is left out (never run: DISABLE_ANYHIT, and it does not compile
// against lib/raydata.cuh); texture/imageTexture.cu is left out (tex2D hardware filtering): a scene with an image is refused.
//
// Single-threaded by design: the emulation state is one record, and texture/noiseTexture.cu keeps its tables in globals.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "ref_shim/ref_shim_core.h"
#include "../include/rtw.h"

// the reference's shared headers, at global scope, once (their include guards keep them out of the namespaces below)
#include "lib/random.cuh"
#include "lib/raydata.cuh"
#include "shaders/sysparameter.h"
#include "shaders/FunctionIdx.h"
#include "lib/sampling.cuh"
#include "lib/onb.cuh"
#include "pdf/pdf.cuh"
#include "texture/texture.cuh"

// the launch parameters every program declares `extern "C" __constant__`
extern "C" { SysParamter Parameter; }

// ---- the programs, unmodified
// raygen.cu stores sqrtf(sample) (its "gamma correction (2)"); the three sqrtf calls of that file - it has no other - also leave
// their arguments here, so that a launch can hand out the sample itself and nothing has to be squared again
namespace refemu {
float gamma_arg[3];
int gamma_n = 0;
inline float gamma_hook(float x) { gamma_arg[gamma_n++ % 3] = x; return ::sqrtf(x); }
}
namespace u_raygen {
#define sqrtf refemu::gamma_hook
#include "raygen/raygen.cu"
#undef sqrtf
}
namespace u_closehit {
#include "shaders/closehit.cu"
}
namespace u_miss {
#include "miss/miss.cu"
}
namespace u_camera {
#include "shaders/camera.cu"
}
namespace u_camera6 {  // the OptiX-6 header that still holds the environment and orthographic cameras
#include "scene/camera.cuh"
}
namespace u_sphere {
#include "geometry/sphere.cu"
}
namespace u_movingsphere {
#include "geometry/movingSphere.cu"
}
namespace u_rectx {
#include "shaders/aarectx.cu"
}
namespace u_recty {
#include "shaders/aarecty.cu"
}
namespace u_rectz {
#include "shaders/aarectz.cu"
}
namespace u_volbox {
#include "geometry/volumeBox.cu"
}
namespace u_volsphere {
#include "geometry/volumeSphere.cu"
}
namespace u_lambertian {
#include "material/lambertianMaterial.cu"
}
namespace u_dielectric {
#include "material/dielectricMaterial.cu"
}
namespace u_metal {
#include "material/metalMaterial.cu"
}
namespace u_light {
#include "material/diffuseLight.cu"
}
namespace u_isotropic {
#include "material/isotropicMaterial.cu"
}
namespace u_normal {
#include "material/normalMaterial.cu"
}
namespace u_tex_constant {
#include "texture/constantTexture.cu"
}
namespace u_tex_checker {
#include "texture/checkeredTexture.cu"
}
namespace u_tex_noise {
#include "texture/noiseTexture.cu"
}
namespace u_tex_null {
#include "texture/nullTexture.cu"
}
namespace u_pdf_rect {
#include "pdf/rectPdf.cu"
}
namespace u_pdf_cosine {
#include "pdf/cosinePdf.cu"
}
namespace u_pdf_mixture {
#include "pdf/mixturePdf.cu"
}
namespace u_pdf_mixture_bias {
#include "pdf/mixtureBiasPdf.cu"
}

// ================================================================== the emulation
namespace refemu {

thread_local unsigned long long rnd_calls = 0;
void* callables[64];

[[noreturn]] void missing_callable(unsigned int idx) {
    fprintf(stderr, "ref_programs: direct callable %u is not in the table\n", idx);
    abort();
}

// One OptixInstance (geometry/ioGeometryInstance.h:20-26) with its SBT record (Director.cpp createSBT :628-885).
struct Instance {
    HitGroupData hg;
    int type;            // rtw_prim_type: which intersection program the record's header names
    unsigned int id;     // OptixInstance.instanceId = rtw_prim.material (closehit.cu:50,63)
    bool xformed;        // rtw_prim.xform != 0
    float m[12], inv[12];
    float3 c0, c1;       // moving sphere: the keys translate(C0), translate(C1) of its matrix-motion transform
};

struct Hit {  // one accepted optixReportIntersection, for level A
    float t;
    unsigned int attr[8];
};

struct State {
    // the ray of the traversal in flight
    float3 o, d;
    float tmin, tmax, time;
    unsigned int flags, p0, p1;
    // the instance whose program runs (intersection), or the committed one (closest hit)
    const Instance* cur;
    float3 oo, od, mt;
    // the hit object
    const Instance* hit;
    float3 hit_oo, hit_od, hit_mt;
    unsigned int attr[8];
    bool stop;
    uint3 idx, dim;
    unsigned long long radiance_traversals, shadow_traversals;
    std::vector<Hit>* log;
};
static State S;
static std::vector<Instance> instances;

// 3x4 row-major. The order of the sums is this file's choice (OptiX states none): products left to right, translation last.
static inline float3 xf_point(const float* m, float3 p) {
    return make_float3(m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3], m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7],
                       m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]);
}
static inline float3 xf_vector(const float* m, float3 d) {
    return make_float3(m[0] * d.x + m[1] * d.y + m[2] * d.z, m[4] * d.x + m[5] * d.y + m[6] * d.z, m[8] * d.x + m[9] * d.y + m[10] * d.z);
}
// (inverse linear part)^T n
static inline float3 xf_normal(const float* inv, float3 n) {
    return make_float3(inv[0] * n.x + inv[4] * n.y + inv[8] * n.z, inv[1] * n.x + inv[5] * n.y + inv[9] * n.z,
                       inv[2] * n.x + inv[6] * n.y + inv[10] * n.z);
}

static void run_intersection(const Instance& in) {
    switch (in.type) {
    case RTW_PRIM_SPHERE: u_sphere::__intersection__sphere(); break;
    case RTW_PRIM_MOVING_SPHERE: u_movingsphere::__intersection__movingsphere(); break;
    case RTW_PRIM_RECT_X: u_rectx::__intersection__hitRectX(); break;
    case RTW_PRIM_RECT_Y: u_recty::__intersection__hitRectY(); break;
    case RTW_PRIM_RECT_Z: u_rectz::__intersection__hitRectZ(); break;
    case RTW_PRIM_VOLUME_BOX: u_volbox::__intersection__hitVolumebox(); break;
    case RTW_PRIM_VOLUME_SPHERE: u_volsphere::__intersection__hitVolumesphere(); break;
    default: abort();
    }
}

// The ray in the object space of one instance. World -> instance by rtw_xform.inv (xform 0 is the identity and is skipped,
// as the oracle skips it). A moving sphere's child is a two-key matrix-motion transform, translate(C0) at time 0 and
// translate(C1) at time 1 (geometry/ioMovingSphere.h:161-203): OptiX interpolates the keys' matrices linearly at the ray
// time, clamped to the keys' interval (no OPTIX_MOTION_FLAG_*_VANISH), and the inverse of a translation is its negative:
// the origin moves back by C0 + s (C1 - C0) (tests/geometry_ref.py states the same reading).
static void enter(const Instance& in) {
    S.cur = &in;
    S.oo = in.xformed ? xf_point(in.inv, S.o) : S.o;
    S.od = in.xformed ? xf_vector(in.inv, S.d) : S.d;
    S.mt = make_float3(0.f);
    if (in.type == RTW_PRIM_MOVING_SPHERE) {
        const float s = fminf(fmaxf(S.time, 0.f), 1.f);
        S.mt = in.c0 + s * (in.c1 - in.c0);
        S.oo = S.oo - S.mt;
    }
}

// optixTraverse: a scan over the instances in index order (an acceleration structure visits them in an order of its own;
// the order is observable only through ties in t and through the media's draws).
void traverse(float3 o, float3 d, float tmin, float tmax, float ray_time, unsigned int flags, unsigned int p0, unsigned int p1) {
    S.o = o; S.d = d; S.tmin = tmin; S.tmax = tmax; S.time = ray_time; S.flags = flags; S.p0 = p0; S.p1 = p1;
    S.hit = nullptr;
    S.stop = false;
    if (flags & OPTIX_RAY_FLAG_TERMINATE_ON_FIRST_HIT) S.shadow_traversals++; else S.radiance_traversals++;
    for (size_t i = 0; i < instances.size() && !S.stop; i++) {
        enter(instances[i]);
        run_intersection(instances[i]);
    }
    S.cur = S.hit;
    if (S.hit) { S.oo = S.hit_oo; S.od = S.hit_od; S.mt = S.hit_mt; }
}

// optixInvoke: the closest-hit program of the hit object's record (all records name __closesthit__radiance,
// Director.cpp createSBT) or the miss program.
void invoke() {
    if (S.hit) u_closehit::__closesthit__radiance();
    else u_miss::__miss__Program();
}

}  // namespace refemu

using refemu::S;

void* optixGetSbtDataPointer() { return (void*)&S.cur->hg; }
float3 optixGetObjectRayOrigin() { return S.oo; }
float3 optixGetObjectRayDirection() { return S.od; }
float3 optixGetWorldRayOrigin() { return S.o; }
float3 optixGetWorldRayDirection() { return S.d; }
float optixGetRayTmin() { return S.tmin; }
float optixGetRayTmax() { return S.tmax; }
float optixGetRayTime() { return S.time; }
// object -> world: the motion translation first (the inverse order of refemu::enter), then the instance's matrix
float3 optixTransformPointFromObjectToWorldSpace(float3 p) {
    if (S.cur->type == RTW_PRIM_MOVING_SPHERE) p = p + S.mt;
    return S.cur->xformed ? refemu::xf_point(S.cur->m, p) : p;
}
float3 optixTransformNormalFromObjectToWorldSpace(float3 n) { return S.cur->xformed ? refemu::xf_normal(S.cur->inv, n) : n; }
// Accepted inside the open interval (tmin, tmax); an accepted hit is committed at once (no any-hit program runs:
// OPTIX_GEOMETRY_FLAG_DISABLE_ANYHIT) and shrinks tmax, so of equal t the earlier instance keeps the hit.
bool optixReportIntersection(float t, unsigned int, unsigned int a0, unsigned int a1, unsigned int a2, unsigned int a3, unsigned int a4,
                             unsigned int a5, unsigned int a6, unsigned int a7) {
    if (!(t > S.tmin && t < S.tmax)) return false;
    S.tmax = t;
    S.hit = S.cur;
    S.hit_oo = S.oo; S.hit_od = S.od; S.hit_mt = S.mt;
    const unsigned int a[8] = {a0, a1, a2, a3, a4, a5, a6, a7};
    memcpy(S.attr, a, sizeof a);
    if (S.log) { refemu::Hit h; h.t = t; memcpy(h.attr, a, sizeof a); S.log->push_back(h); }
    if (S.flags & OPTIX_RAY_FLAG_TERMINATE_ON_FIRST_HIT) S.stop = true;
    return true;
}
unsigned int optixGetPayload_0() { return S.p0; }
unsigned int optixGetPayload_1() { return S.p1; }
unsigned int optixGetAttribute_0() { return S.attr[0]; }
unsigned int optixGetAttribute_1() { return S.attr[1]; }
unsigned int optixGetAttribute_2() { return S.attr[2]; }
unsigned int optixGetAttribute_3() { return S.attr[3]; }
unsigned int optixGetAttribute_4() { return S.attr[4]; }
unsigned int optixGetAttribute_5() { return S.attr[5]; }
unsigned int optixGetAttribute_6() { return S.attr[6]; }
unsigned int optixGetAttribute_7() { return S.attr[7]; }
unsigned int optixGetInstanceId() { return S.cur->id; }
uint3 optixGetLaunchIndex() { return S.idx; }
uint3 optixGetLaunchDimensions() { return S.dim; }
bool optixHitObjectIsHit() { return S.hit != nullptr; }

// ================================================================== the scene
namespace {

enum {
    IDX_MAT = NUM_CALLABLE_CAMERA,
    IDX_TEX = NUM_CALLABLE_CAMERA + NUM_CALLABLE_MAT_IDS,   // lambertianMaterial.cu:65: texCallidx + cameras + materials
    IDX_PDF = NUM_CALLABLE_CAMERA + NUM_CALLABE_TEX_IDS + NUM_CALLABLE_MAT_IDS,  // closehit.cu:75-76
    IDX_END = IDX_PDF + NUM_CALLABLE_PDF_IDS,
    // this file's own entries, behind the reference's table
    IDX_CHECKER_ODD = IDX_END, IDX_CHECKER_EVEN, IDX_CAMERA_ENVIRONMENT, IDX_CAMERA_ORTHOGRAPHIC
};

struct Scene {
    std::vector<MaterialParams> mats;
    std::vector<textureParam> texs;       // one per rtw_texture; a material's texArr points at its texture's entry
    std::vector<int> tex_odd, tex_even;   // checker children, as indices into texs
    std::vector<LightDefinition> lights;
    pdfCallfun p0, p1;
    std::vector<uint32_t> texdata;
    textureParam null_tex;
};
Scene G;

// A checker's children. The reference stores the children's TexCallFunction ids in textureParam.odd / even
// (texture/ioTexture.h:109-110) and checkeredTexture.cu:15,18 uses them as raw SBT indices with the checker's own material
// record: it never shows a checker (include/rtw.h, rtw_texture). This project evaluates the children; here they sit behind
// two entries of this file's that hand the child its own textureParam.
float3 checker_child(MaterialParams const& matPar, float u, float v, float3 p, bool odd) {
    const size_t i = (size_t)(matPar.texArr - G.texs.data());
    const int child = odd ? G.tex_odd[i] : G.tex_even[i];
    MaterialParams mp = matPar;
    mp.texArr = &G.texs[(size_t)child];
    return optixDirectCall<float3, MaterialParams const&, float, float, float3>((unsigned)(mp.texArr->texCallidx + IDX_TEX), mp, u, v, p);
}
float3 checker_odd(MaterialParams const& m, float u, float v, float3 p) { return checker_child(m, u, v, p, true); }
float3 checker_even(MaterialParams const& m, float u, float v, float3 p) { return checker_child(m, u, v, p, false); }

// The environment and orthographic cameras exist only in scene/camera.cuh (OptiX 6, variables instead of launch parameters);
// raygen.cu:112-114 calls whatever callable Parameter.cameraType names, so they sit behind that call. Neither takes the seed.
void sync_camera6() {
    u_camera6::cameraOrigin = Parameter.cameraOrigin; u_camera6::cameraU = Parameter.cameraU; u_camera6::cameraV = Parameter.cameraV;
    u_camera6::cameraW = Parameter.cameraW; u_camera6::cameraLowerLeftCorner = Parameter.cameraLowerLeftCorner;
    u_camera6::cameraHorizontal = Parameter.cameraHorizontal; u_camera6::cameraVertical = Parameter.cameraVertical;
    u_camera6::cameraLensRadius = Parameter.cameraLensRadius; u_camera6::cameraTime0 = Parameter.cameraTime0;
    u_camera6::cameraTime1 = Parameter.cameraTime1;
}
void camera_environment(const float s, const float t, unsigned int&, float3& o, float3& d) { u_camera6::environmentCamera(s, t, o, d); }
void camera_orthographic(const float s, const float t, unsigned int&, float3& o, float3& d) { u_camera6::orthographicCamera(s, t, o, d); }

void fill_table() {
    void** c = refemu::callables;
    memset(c, 0, sizeof refemu::callables);
    c[CALLABLE_ID_PINHOLE] = (void*)&u_camera::__direct_callable__perspectiveCamera;
    c[IDX_MAT + CALLABLE_ID_LIGHT_DIFFUSE] = (void*)&u_light::__direct_callable__diffuselight;
    c[IDX_MAT + CALLABLE_ID_DIELECTRIC] = (void*)&u_dielectric::__direct_callable__dielectricMat;
    c[IDX_MAT + CALLABLE_ID_ISOTROPIC] = (void*)&u_isotropic::__direct_callable__ISOTROPIC;
    c[IDX_MAT + CALLABLE_ID_LAMBERTIAN] = (void*)&u_lambertian::__direct_callable__lambertian;
    c[IDX_MAT + CALLABLE_ID_METAL] = (void*)&u_metal::__direct_callable__metal;
    c[IDX_MAT + CALLABLE_ID_NORMAL] = (void*)&u_normal::__direct_callable__normal;
    c[IDX_TEX + CALLABLE_CHECKEDTEX] = (void*)&u_tex_checker::__direct_callable__checkerTexture;
    c[IDX_TEX + CALLABLE_CONSTANTTEX] = (void*)&u_tex_constant::__direct_callable__constantTexture;
    c[IDX_TEX + CALLABLE_NOISETEX] = (void*)&u_tex_noise::__direct_callable__noisetexture;
    c[IDX_TEX + CALLABLE_NULLTEX] = (void*)&u_tex_null::__direct_callable__nullTexture;
    c[IDX_PDF + CALLABLE_ID_cosineGenerate] = (void*)&u_pdf_cosine::__direct_callable__cosineGenerate;
    c[IDX_PDF + CALLABLE_ID_mixtureBIAS_generate] = (void*)&u_pdf_mixture_bias::__direct_callable__mixtureBIAS_generate;
    c[IDX_PDF + CALLABLE_ID_mixture_generate] = (void*)&u_pdf_mixture::__direct_callable__mixture_generate;
    c[IDX_PDF + CALLABLE_ID_rect_X_generate] = (void*)&u_pdf_rect::__direct_callable__rect_x_generate;
    c[IDX_PDF + CALLABLE_ID_rect_Y_generate] = (void*)&u_pdf_rect::__direct_callable__rect_y_generate;
    c[IDX_PDF + CALLABLE_ID_rect_Z_generate] = (void*)&u_pdf_rect::__direct_callable__rect_z_generate;
    c[IDX_PDF + CALLABLE_ID_cosineValue] = (void*)&u_pdf_cosine::__direct_callable__cosineValue;
    c[IDX_PDF + CALLABLE_ID_mixtureBIAS_value] = (void*)&u_pdf_mixture_bias::__direct_callable__mixtureBIAS_value;
    c[IDX_PDF + CALLABLE_ID_mixture_value] = (void*)&u_pdf_mixture::__direct_callable__mixture_value;
    c[IDX_PDF + CALLABLE_ID_rect_x_value] = (void*)&u_pdf_rect::__direct_callable__rect_x_value;
    c[IDX_PDF + CALLABLE_ID_rect_y_value] = (void*)&u_pdf_rect::__direct_callable__rect_y_value;
    c[IDX_PDF + CALLABLE_ID_rect_z_value] = (void*)&u_pdf_rect::__direct_callable__rect_z_value;
    c[IDX_PDF + CALLABLE_ID_LIGHT_SAMPLE_PDF] = (void*)&u_lambertian::__direct_callable__eval_bsdf_diffuse_reflection;
    c[IDX_PDF + CALLABLE_ID_LIGHT_SAMPLE_DIELECT_PDF] = (void*)&u_dielectric::__direct_callable__eval_bsdf_dielect_reflection;
    c[IDX_PDF + CALLABLE_ID_LIGHT_SAMPLE_METAL_PDF] = (void*)&u_metal::__direct_callable__eval_bsdf_metal_reflection;
    c[IDX_CHECKER_ODD] = (void*)&checker_odd;
    c[IDX_CHECKER_EVEN] = (void*)&checker_even;
    c[IDX_CAMERA_ENVIRONMENT] = (void*)&camera_environment;
    c[IDX_CAMERA_ORTHOGRAPHIC] = (void*)&camera_orthographic;
}

inline float3 f3(const float* p) { return make_float3(p[0], p[1], p[2]); }

// rtw_material_type (MaterialType, raydata.cuh:22-29) -> MatCallFunction (FunctionIdx.h:17-25), material/io*Material.h assignTo
const int MAT_CALL[6] = {CALLABLE_ID_LAMBERTIAN, CALLABLE_ID_LIGHT_DIFFUSE, CALLABLE_ID_METAL, CALLABLE_ID_DIELECTRIC, CALLABLE_ID_ISOTROPIC, CALLABLE_ID_NORMAL};

// The blob -> SysParamter, HitGroupData, MaterialParams, textureParam, LightDefinition, pdfCallfun. 0 or a negative rtw_status.
int load_scene(const void* blob, size_t bytes, int width, int height, int max_depth) {
    if (!blob || bytes < sizeof(rtw_scene_header)) return RTW_ERR_BAD_SCENE;
    const rtw_scene_header* h = (const rtw_scene_header*)blob;
    if (h->magic != RTW_SCENE_MAGIC || h->version != RTW_SCENE_VERSION || h->total_bytes > bytes) return RTW_ERR_BAD_SCENE;
    const char* b = (const char*)blob;
    if ((size_t)h->off_prims + (size_t)h->n_prims * sizeof(rtw_prim) > bytes || (size_t)h->off_xforms + (size_t)h->n_xforms * sizeof(rtw_xform) > bytes ||
        (size_t)h->off_materials + (size_t)h->n_materials * sizeof(rtw_material) > bytes || (size_t)h->off_textures + (size_t)h->n_textures * sizeof(rtw_texture) > bytes ||
        (size_t)h->off_lights + (size_t)h->n_lights * sizeof(rtw_light) > bytes || (size_t)h->off_texdata + (size_t)h->texdata_bytes > bytes || h->n_xforms < 1)
        return RTW_ERR_BAD_SCENE;
    const rtw_prim* prims = (const rtw_prim*)(b + h->off_prims);
    const rtw_xform* xforms = (const rtw_xform*)(b + h->off_xforms);
    const rtw_material* mats = (const rtw_material*)(b + h->off_materials);
    const rtw_texture* texs = (const rtw_texture*)(b + h->off_textures);
    const rtw_light* lights = (const rtw_light*)(b + h->off_lights);
    fill_table();
    G = Scene();
    G.texdata.assign((const uint32_t*)(b + h->off_texdata), (const uint32_t*)(b + h->off_texdata) + h->texdata_bytes / 4u);

    // textureParam (raydata.cuh:127-138; texture/ioTexture.h assignTo :53, :81, :109-111, :185)
    G.texs.resize(h->n_textures); G.tex_odd.assign(h->n_textures, -1); G.tex_even.assign(h->n_textures, -1);
    for (uint32_t i = 0; i < h->n_textures; i++) {
        textureParam& tp = G.texs[i];
        memset(&tp, 0, sizeof tp);
        tp.texCallidx = texs[i].type;  // rtw_texture_type has TexCallFunction's numbering
        tp.color = f3(texs[i].color);
        tp.scale = texs[i].scale;
        if (texs[i].type == RTW_TEX_IMAGE) return RTW_ERR_UNSUPPORTED;
        if (texs[i].type == RTW_TEX_CHECKER) {
            if (texs[i].odd < 0 || texs[i].even < 0 || (uint32_t)texs[i].odd >= h->n_textures || (uint32_t)texs[i].even >= h->n_textures) return RTW_ERR_BAD_SCENE;
            G.tex_odd[i] = texs[i].odd; G.tex_even[i] = texs[i].even;
            tp.odd = IDX_CHECKER_ODD; tp.even = IDX_CHECKER_EVEN;  // raw SBT indices, as checkeredTexture.cu:15,18 reads them
        }
        if (texs[i].type == RTW_TEX_NOISE) {
            if ((size_t)texs[i].data + 1536u > G.texdata.size()) return RTW_ERR_BAD_SCENE;
            const uint32_t* tab = G.texdata.data() + texs[i].data;  // float ranvec[256][3], int perm_x / y / z[256] (ioTexture.h:118-222)
            tp.randvec = (CUdeviceptr)(uintptr_t)tab;
            tp.permX = (CUdeviceptr)(uintptr_t)(tab + 768); tp.permY = (CUdeviceptr)(uintptr_t)(tab + 1024); tp.permZ = (CUdeviceptr)(uintptr_t)(tab + 1280);
        }
    }
    memset(&G.null_tex, 0, sizeof G.null_tex);
    G.null_tex.texCallidx = CALLABLE_NULLTEX;
    // MaterialParams (sysparameter.h:5-14; material/io*Material.h assignTo; Director.cpp:501-519)
    G.mats.resize(h->n_materials);
    for (uint32_t i = 0; i < h->n_materials; i++) {
        MaterialParams& mp = G.mats[i];
        memset(&mp, 0, sizeof mp);
        if (mats[i].type < 0 || mats[i].type > 5 || mats[i].texture >= (int32_t)h->n_textures) return RTW_ERR_BAD_SCENE;
        mp.matindex = MAT_CALL[mats[i].type];
        mp.lightreflectIdx = CALLABLE_ID_LIGHT_SAMPLE_PDF + (mats[i].bsdf_eval < 0 ? 0 : mats[i].bsdf_eval);  // rtw_material.bsdf_eval
        mp.texArr = mats[i].texture < 0 ? &G.null_tex : &G.texs[(size_t)mats[i].texture];
        mp.fuzz = mats[i].fuzz_or_eta;
    }
    // instances and their SBT records (Director.cpp:668-835), in the blob's primitive order
    refemu::instances.clear();
    for (uint32_t i = 0; i < h->n_prims; i++) {
        const rtw_prim& pr = prims[i];
        if (pr.type < RTW_PRIM_SPHERE || pr.type > RTW_PRIM_VOLUME_SPHERE || pr.xform < 0 || (uint32_t)pr.xform >= h->n_xforms || pr.material < 0 ||
            (uint32_t)pr.material >= h->n_materials)
            return RTW_ERR_BAD_SCENE;
        refemu::Instance in;
        memset(&in, 0, sizeof in);
        in.type = pr.type; in.id = (unsigned)pr.material; in.xformed = pr.xform != 0;
        memcpy(in.m, xforms[pr.xform].m, sizeof in.m); memcpy(in.inv, xforms[pr.xform].inv, sizeof in.inv);
        HitGroupData& hg = in.hg;
        hg.color = make_float3(0.9f, 0.1f, 0.1f);
        switch (pr.type) {
        case RTW_PRIM_SPHERE: hg.center = f3(pr.p); hg.radius = pr.p[3]; break;                      // :676-678
        case RTW_PRIM_MOVING_SPHERE:                                                                  // :718-724
            hg.center = f3(pr.p); hg.radius = pr.p[3]; hg.center1 = f3(pr.p + 4); hg.time0 = pr.p[7]; hg.time1 = pr.p[8]; hg.bMotion = 1;
            in.c0 = f3(pr.p); in.c1 = f3(pr.p + 4);
            break;
        case RTW_PRIM_RECT_X: case RTW_PRIM_RECT_Y: case RTW_PRIM_RECT_Z:                             // :774-779
            hg.rectData.a0 = pr.p[0]; hg.rectData.a1 = pr.p[1]; hg.rectData.b0 = pr.p[2]; hg.rectData.b1 = pr.p[3]; hg.rectData.k = pr.p[4];
            hg.rectData.flip = pr.flip;
            break;
        case RTW_PRIM_VOLUME_BOX: hg.VolBoxData.boxMin = f3(pr.p); hg.VolBoxData.boxMax = f3(pr.p + 3); hg.VolBoxData.density = pr.p[6]; break;  // :809-811
        default: hg.center = f3(pr.p); hg.radius = pr.p[3]; hg.density = pr.p[4]; break;              // :833-835
        }
        refemu::instances.push_back(in);
    }
    // LightDefinition (raydata.cuh:31-48; Director.cpp:523-530)
    G.lights.resize(h->n_lights);
    for (uint32_t i = 0; i < h->n_lights; i++) {
        LightDefinition& ld = G.lights[i];
        memset(&ld, 0, sizeof ld);
        ld.position = f3(lights[i].position); ld.vecU = f3(lights[i].vec_u); ld.vecV = f3(lights[i].vec_v); ld.normal = f3(lights[i].normal);
        ld.area = lights[i].area; ld.emission = f3(lights[i].emission);
    }
    // SysParamter (sysparameter.h:32-60; Director.cpp:483-553)
    memset(&Parameter, 0, sizeof Parameter);
    Parameter.handle = 1;
    Parameter.m_Nx = width; Parameter.m_Ny = height;
    Parameter.maxRayDepth = max_depth;
    Parameter.numSamples = 1;
    Parameter.lights = G.lights.empty() ? nullptr : G.lights.data();
    Parameter.numLights = (int)h->n_lights;
    Parameter.skyLight = h->sky_light;
    // pdfCallfun (sysparameter.h:16-30; scene/ioScene.h:109-140; Director.cpp:534-548): the rectangle sits in the top record
    // and, for a mixture, in child p1 (mixturePdf.cu:36-37 reads Parameter.pdf.p1->pdfrect)
    hitRectData rc;
    rc.a0 = h->pdf.rect[0]; rc.a1 = h->pdf.rect[1]; rc.b0 = h->pdf.rect[2]; rc.b1 = h->pdf.rect[3]; rc.k = h->pdf.rect[4]; rc.flip = h->pdf.flip;
    memset(&G.p0, 0, sizeof G.p0); memset(&G.p1, 0, sizeof G.p1);
    Parameter.pdf.pdfGenIdx = h->pdf.gen;
    Parameter.pdf.pdfValIdx = h->pdf.gen + CALLABLE_ID_cosineValue;
    Parameter.pdf.pdfrect = rc;
    if (h->pdf.gen == RTW_PDF_MIXTURE_BIAS) return RTW_ERR_UNSUPPORTED;  // closehit.cu:82-84 calls it with another signature than it has
    if (h->pdf.p0_gen >= 0 || h->pdf.p1_gen >= 0) {
        G.p0.pdfGenIdx = h->pdf.p0_gen < 0 ? 0 : h->pdf.p0_gen; G.p0.pdfValIdx = G.p0.pdfGenIdx + CALLABLE_ID_cosineValue;
        G.p1.pdfGenIdx = h->pdf.p1_gen < 0 ? 0 : h->pdf.p1_gen; G.p1.pdfValIdx = G.p1.pdfGenIdx + CALLABLE_ID_cosineValue;
        G.p1.pdfrect = rc;
        Parameter.pdf.p0 = &G.p0; Parameter.pdf.p1 = &G.p1;
    }
    // camera (scene/ioCamera.h getfrustum; Director.cpp:494-496, :521-522)
    const rtw_camera& cam = h->camera;
    Parameter.cameraOrigin = f3(cam.origin); Parameter.cameraU = f3(cam.u); Parameter.cameraV = f3(cam.v); Parameter.cameraW = f3(cam.w);
    Parameter.cameraTime0 = cam.time0; Parameter.cameraTime1 = cam.time1; Parameter.cameraLensRadius = cam.lens_radius;
    Parameter.cameraLowerLeftCorner = f3(cam.lower_left); Parameter.cameraHorizontal = f3(cam.horizontal); Parameter.cameraVertical = f3(cam.vertical);
    Parameter.cameraType = h->camera_type == RTW_CAM_PERSPECTIVE ? CALLABLE_ID_PINHOLE
                         : h->camera_type == RTW_CAM_ENVIRONMENT ? IDX_CAMERA_ENVIRONMENT : IDX_CAMERA_ORTHOGRAPHIC;
    Parameter.MatParams = G.mats.data();
    sync_camera6();
    S.log = nullptr;
    return RTW_OK;
}

}  // namespace

// ================================================================== C ABI
extern "C" {

// ---- level B: one launch, rows [row0, row1) of it. frame: (row1 - row0) * width float4, as raygen.cu:151-158 writes it (sqrt of
// the sample, alpha 1; image row 0 is the bottom row). linear (may be NULL): (row1 - row0) * width * 3 floats, the sample before
// that square root: the three arguments of raygen.cu's own sqrtf calls (refemu::gamma_hook). counts (may be NULL):
// (row1 - row0) * width * 3 uint32: radiance traversals, shadow traversals, rnd() calls of each pixel.
int ref_launch_rows(const void* blob, size_t bytes, int width, int height, int row0, int row1, int max_depth, float* frame, float* linear,
                    uint32_t* counts) {
    int rc = load_scene(blob, bytes, width, height, max_depth);
    if (rc) return rc;
    if (width <= 0 || height <= 0 || row0 < 0 || row1 > height || row0 > row1 || !frame) return RTW_ERR_INVALID_ARG;
    // raygen.cu:156-158 writes pixel (x, y) at frame_buffer[y * width + x]: the buffer's origin lies row0 rows before `frame`
    // (no byte before `frame` is touched: only rows row0 .. row1 - 1 are launched)
    std::vector<float4> whole((size_t)width * (size_t)height);
    Parameter.frame_buffer = whole.data();
    S.dim = make_uint3((unsigned)width, (unsigned)height, 1u);
    for (int y = row0; y < row1; y++)
        for (int x = 0; x < width; x++) {
            S.idx = make_uint3((unsigned)x, (unsigned)y, 0u);
            S.radiance_traversals = S.shadow_traversals = 0;
            refemu::rnd_calls = 0;
            refemu::gamma_n = 0;
            u_raygen::__raygen__Program();
            const size_t i = (size_t)(y - row0) * (size_t)width + (size_t)x;
            if (linear) for (int k = 0; k < 3; k++) linear[3 * i + k] = refemu::gamma_arg[k];
            if (counts) {
                uint32_t* c = counts + 3 * i;
                c[0] = (uint32_t)S.radiance_traversals; c[1] = (uint32_t)S.shadow_traversals; c[2] = (uint32_t)refemu::rnd_calls;
            }
        }
    memcpy(frame, whole.data() + (size_t)row0 * (size_t)width, (size_t)(row1 - row0) * (size_t)width * sizeof(float4));
    Parameter.frame_buffer = nullptr;
    return RTW_OK;
}
int ref_launch(const void* blob, size_t bytes, int width, int height, int max_depth, float* frame, uint32_t* counts) {
    return ref_launch_rows(blob, bytes, width, height, 0, height, max_depth, frame, nullptr, counts);
}

// ---- level A: one program at a time. (The material, pdf and miss callables are reached through launches of one-ray cameras on the
// float64 laws' own cases: tests/ref_programs.py, law_samples.)
// Intersection programs. rays: n * 8 floats (ox, oy, oz, dx, dy, dz, tmin, tmax), ray_time / gather_time: n floats or NULL.
// Every instance's program runs on every ray in index order with closest-hit commit, media left out (their hit is a draw).
// Per ray: n_reported = accepted reports; the committed hit's t, instance index (-1: none), normal, u, v, point (11 floats:
// t, nx, ny, nz, u, v, px, py, pz, and two spare).
int ref_intersect(const void* blob, size_t bytes, const float* rays, const float* ray_time, const float* gather_time, int n,
                  float* out11, int32_t* out_prim, int32_t* out_reported) {
    int rc = load_scene(blob, bytes, 1, 1, 1);
    if (rc) return rc;
    std::vector<refemu::Hit> log;
    PerRayData prd;
    for (int i = 0; i < n; i++) {
        const float* r = rays + 8 * (size_t)i;
        memset(&prd, 0, sizeof prd);
        prd.gatherTime = gather_time ? gather_time[i] : 0.f;
        const uint2 pl = splitPointer(&prd);
        log.clear();
        S.log = &log;
        S.o = make_float3(r[0], r[1], r[2]); S.d = make_float3(r[3], r[4], r[5]); S.tmin = r[6]; S.tmax = r[7];
        S.time = ray_time ? ray_time[i] : 0.f; S.flags = 0; S.p0 = pl.x; S.p1 = pl.y; S.hit = nullptr; S.stop = false;
        int prim = -1;
        for (size_t k = 0; k < refemu::instances.size(); k++) {
            const refemu::Instance& in = refemu::instances[k];
            if (in.type == RTW_PRIM_VOLUME_BOX || in.type == RTW_PRIM_VOLUME_SPHERE) continue;
            const refemu::Instance* before = S.hit;
            const float tb = S.tmax;
            refemu::enter(in);
            refemu::run_intersection(in);
            if (S.hit != before || S.tmax != tb) prim = (int)k;
        }
        S.log = nullptr;
        float* o = out11 + 11 * (size_t)i;
        memset(o, 0, 11 * sizeof(float));
        o[0] = S.tmax;
        out_prim[i] = prim;
        out_reported[i] = (int32_t)log.size();
        if (prim >= 0) {
            // the attribute order of closehit.cu:52-58: normal 0-2, u 3, v 4, point 5-7
            for (int k = 0; k < 8; k++) o[1 + k] = __uint_as_float(S.attr[k]);
        }
    }
    return RTW_OK;
}

// Camera callables: the blob's camera and camera type, on n (s, t, seed) -> origin, direction, seed after the call.
int ref_camera(const void* blob, size_t bytes, const float* s, const float* t, const uint32_t* seed, int n, float* origin, float* direction,
               uint32_t* seed_out) {
    int rc = load_scene(blob, bytes, 1, 1, 1);
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        unsigned int sd = seed[i];
        float3 o, d;
        optixDirectCall<void, const float, const float, unsigned int&, float3&, float3&>((unsigned)Parameter.cameraType, s[i], t[i], sd, o, d);
        origin[3 * i] = o.x; origin[3 * i + 1] = o.y; origin[3 * i + 2] = o.z;
        direction[3 * i] = d.x; direction[3 * i + 1] = d.y; direction[3 * i + 2] = d.z;
        seed_out[i] = sd;
    }
    return RTW_OK;
}

// Texture callables: texture `tex` of the blob at n (u, v, point) -> rgb.
int ref_texture(const void* blob, size_t bytes, int tex, const float* uv, const float* points, int n, float* rgb) {
    int rc = load_scene(blob, bytes, 1, 1, 1);
    if (rc) return rc;
    if (tex < 0 || (size_t)tex >= G.texs.size()) return RTW_ERR_INVALID_ARG;
    MaterialParams mp;
    memset(&mp, 0, sizeof mp);
    mp.texArr = &G.texs[(size_t)tex];
    for (int i = 0; i < n; i++) {
        const float3 c = optixDirectCall<float3, MaterialParams const&, float, float, float3>((unsigned)(mp.texArr->texCallidx + IDX_TEX), mp, uv[2 * i],
                                                                                                uv[2 * i + 1], f3(points + 3 * i));
        rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
    }
    return RTW_OK;
}

}  // extern "C"
