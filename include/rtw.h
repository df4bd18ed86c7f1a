/* rtw.h — C ABI of the MI355X wavefront path tracer (librtw_hip.so).
 *
 * This is the drop-in boundary for the reference's one device launch:
 *
 *   Director::renderFrame  ->  optixLaunch(pipeline, stream, d_params,
 *                                          sizeof(SysParamter), &m_sbt, Nx, Ny, 1)
 *                              (reference RestOfLife/Director.cpp:971-1008, launch at :982-984)
 *
 * and for the marshalling that feeds it:
 *
 *   Director::createSBT          (Director.cpp:628-885)  geometry records  -> rtw_prim[]
 *   Director::initLaunchParams   (Director.cpp:483-553)  camera, materials, textures,
 *                                                        lights, pdf tree  -> rtw_scene_header + arrays
 *   SysParamter                  (shaders/sysparameter.h:32-60)            -> rtw_scene_header + rtw_params
 *   HitGroupData / hitRectData / hitVolumeBoxdata (lib/raydata.cuh:79-115) -> rtw_prim
 *   OptixInstance transform[12] / instanceId / sbtOffset
 *                                (geometry/ioGeometryInstance.h:20-26)     -> rtw_xform + rtw_prim.material
 *   MaterialParams / textureParam (sysparameter.h:5-16, raydata.cuh:127-138)-> rtw_material / rtw_texture
 *   LightDefinition              (raydata.cuh:31-48)                       -> rtw_light
 *   pdfCallfun                   (sysparameter.h:18-30)                    -> rtw_pdf
 *
 * Plain pointers and sizes only. No exceptions and no exit() cross this ABI:
 * every call returns 0 on success or a negative rtw_status; the message is
 * available from rtw_last_error().  Nothing is retained from caller pointers
 * after a call returns.
 */
#ifndef RTW_H
#define RTW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_ABI_VERSION 5   /* entry points and the structs they take (rtw_params, rtw_stats, rtw_guides, rtw_adaptive, rtw_accum_info) */
#define RTW_SCENE_VERSION 1 /* layout of the scene blob (rtw_scene_header.version) */
#define RTW_SCENE_MAGIC 0x57545221u /* "!RTW" */
/* Summation order of a pixel's samples (part of the arithmetic contract). Three levels, all counted from
 * sample_offset: the samples of a render call are summed in ascending order inside aligned BLOCKS of RTW_SUM_BLOCK samples;
 * the block sums in ascending order inside aligned UNITS of RTW_SUM_UNIT_BLOCKS blocks (128 samples); the unit sums in
 * ascending order; the mean is that sum divided by spp. The reference renders one sample per launch (raygen.cu:123-159) and
 * so defines no order. Blocks let a lane own a run of a pixel's samples in registers, and a small block lets the last few
 * percent of a render be handed out in short pieces (a launch ends when its slowest piece ends); units are what a lane of a
 * long render owns at a time, so that one 16-byte sum per 128 samples reaches memory instead of one per 16 (round 3: the
 * metric frame's sums take 1.3 GB instead of 8.5 GB, BASELINE config 5's shard 2.6 GB instead of 17 GB in two passes).
 * Renders of at most 128 spp are unchanged by the unit level (0 + x = x). */
#define RTW_SUM_BLOCK 16
#define RTW_SUM_UNIT_BLOCKS 8

typedef enum rtw_status {
    RTW_OK = 0,
    RTW_ERR_INVALID_ARG = -1,
    RTW_ERR_BAD_SCENE = -2,
    RTW_ERR_NO_SCENE = -3,
    RTW_ERR_DEVICE = -4,
    RTW_ERR_OOM = -5,
    RTW_ERR_UNSUPPORTED = -6
} rtw_status;

/* Primitive kinds. One per reference intersection program
 * (Director.h ProgramIdentifier PROGRAM_ID_IS_*; geometry/sphere.cu, movingSphere.cu,
 * shaders/aarect{x,y,z}.cu, geometry/volumeBox.cu, volumeSphere.cu). */
typedef enum rtw_prim_type {
    RTW_PRIM_SPHERE = 0,        /* p[0..2] centre, p[3] radius                                   */
    RTW_PRIM_MOVING_SPHERE = 1, /* p[0..2] centre0, p[3] radius, p[4..6] centre1, p[7] t0, p[8] t1;
                                   carries the reference's matrix-motion transform translate(C0)->translate(C1)
                                   (geometry/ioMovingSphere.h:161-203) on top of its xform             */
    RTW_PRIM_RECT_X = 2,        /* p[0] a0 p[1] a1 p[2] b0 p[3] b1 p[4] k ; a=y b=z (aarectx.cu)  */
    RTW_PRIM_RECT_Y = 3,        /*                                          a=x b=z (aarecty.cu)  */
    RTW_PRIM_RECT_Z = 4,        /*                                          a=x b=y (aarectz.cu)  */
    RTW_PRIM_VOLUME_BOX = 5,    /* p[0..2] boxMin, p[3..5] boxMax, p[6] density                   */
    RTW_PRIM_VOLUME_SPHERE = 6  /* p[0..2] centre, p[3] radius, p[4] density                      */
} rtw_prim_type;

/* Same numbering as MaterialType, lib/raydata.cuh:22-29. */
typedef enum rtw_material_type {
    RTW_MAT_LAMBERTIAN = 0,
    RTW_MAT_DIFFUSE_LIGHT = 1,
    RTW_MAT_METAL = 2,
    RTW_MAT_DIELECTRIC = 3,
    RTW_MAT_ISOTROPIC = 4,
    RTW_MAT_NORMAL = 5
} rtw_material_type;

/* Same numbering as TexCallFunction, shaders/FunctionIdx.h:8-15. */
typedef enum rtw_texture_type {
    RTW_TEX_CHECKER = 0,
    RTW_TEX_CONSTANT = 1,
    RTW_TEX_IMAGE = 2,
    RTW_TEX_NOISE = 3,
    RTW_TEX_NULL = 4
} rtw_texture_type;

/* Same numbering as PDFCallFunction generate ids, shaders/FunctionIdx.h:27-33. */
typedef enum rtw_pdf_gen {
    RTW_PDF_COSINE = 0,
    RTW_PDF_MIXTURE_BIAS = 1,
    RTW_PDF_MIXTURE = 2,
    RTW_PDF_RECT_X = 3,
    RTW_PDF_RECT_Y = 4,
    RTW_PDF_RECT_Z = 5
} rtw_pdf_gen;

/* Camera draws (pixel = the stream key width * y + x, sample = the absolute sample index):
 *   RTW_RNG_TEA_LCG takes no seed. In order: jitter x, jitter y, the two lens draws (perspective camera only, see
 *     rtw_camera_type), the gather-time draw. The first ray time is the same LCG output as the gather-time draw: raygen.cu:100
 *     copies the seed into the payload before raygen.cu:103 draws the gather time, and rayColor starts from the copy.
 *   RTW_RNG_PHILOX: a word w gives the 24-bit uniform (w >> 8) / 2^24. Words 0-3 of block (pixel, sample, 0, 0) are jitter x,
 *     jitter y and the two lens draws, for every camera kind. The gather-time draw is the fifth uniform of that block,
 *     ((w0 & 0xff) << 16 | (w1 & 0xff) << 8 | (w2 & 0xff)) / 2^24: the low bytes the four uniforms leave unused. The camera
 *     ray's time is word 0 of block (pixel, sample, 0, 2), the first draw of stream 2; later segments go on in that stream.
 *   The gather time is time0 + draw * (time1 - time0) of the camera in use. A ray time is the raw uniform in [0, 1), as
 *   raygen.cu:48 hands rnd(seed) to optixTraverse: it does not span time0 / time1. */
typedef enum rtw_rng_kind {
    RTW_RNG_PHILOX = 0,  /* Philox4x32-10, key=(seed,0), counter=(pixel, sample, block, stream)        */
    RTW_RNG_TEA_LCG = 1  /* the reference's own: tea<64>(pixel, sample) + 24-bit LCG rnd() + xorshift
                            randf() (lib/random.cuh:7-38, raygen/raygen.cu:129)                       */
} rtw_rng_kind;

typedef struct rtw_prim {
    int32_t type;     /* rtw_prim_type                                                             */
    int32_t material; /* index into materials[] (== OptixInstance.instanceId, closehit.cu:50,63)  */
    int32_t xform;    /* index into xforms[]; 0 is the identity                                   */
    int32_t flip;     /* rects: hitRectData.flip                                                   */
    float p[12];
} rtw_prim; /* 64 B */

/* Object->world 3x4 row-major (OptixInstance.transform) and its inverse (world->object). */
typedef struct rtw_xform {
    float m[12];
    float inv[12];
} rtw_xform; /* 96 B */

typedef struct rtw_material {
    int32_t type;       /* rtw_material_type                        */
    int32_t texture;    /* index into textures[] or -1              */
    float fuzz_or_eta;  /* MaterialParams union{fuzz,eta}           */
    int32_t bsdf_eval;  /* MaterialParams.lightreflectIdx - CALLABLE_ID_LIGHT_SAMPLE_PDF: 0 diffuse, 1 dielectric, 2 metal, -1 none */
} rtw_material; /* 16 B */

/* textureParam (lib/raydata.cuh:127-138) without its device pointers: tables and texels live in the blob's texture
 * data section (rtw_scene_header.off_texdata), addressed in 4-byte words from the start of that section.
 *   RTW_TEX_CONSTANT  color                                  (texture/constantTexture.cu)
 *   RTW_TEX_CHECKER   odd / even = indices into textures[]   (texture/checkeredTexture.cu; the reference stores the
 *                     children's callable ids and so never shows a checker - here the children are evaluated)
 *   RTW_TEX_NOISE     scale; data -> float ranvec[256][3], int32 perm_x[256], perm_y[256], perm_z[256]
 *                     (texture/noiseTexture.cu, ioTexture.h:118-222)
 *   RTW_TEX_IMAGE     data -> uint32 width, height, then width*height texels r | g<<8 | b<<16 | a<<24, row 0 at
 *                     v = 0 (texture/imageTexture.cu; ioTexture.h:225-262 flips the file's rows the same way);
 *                     sampled bilinearly, clamped, texel centres at (i + 0.5) / width                        */
typedef struct rtw_texture {
    int32_t type; /* rtw_texture_type */
    float color[3];
    int32_t odd, even;
    float scale;
    uint32_t data; /* word offset into the texture data section (noise, image), else 0 */
} rtw_texture; /* 32 B */

typedef struct rtw_light {
    float position[3];
    float vec_u[3];
    float vec_v[3];
    float normal[3];
    float area;
    float emission[3];
} rtw_light; /* 64 B */

typedef struct rtw_pdf {
    int32_t gen;     /* top-level generate id (rtw_pdf_gen), e.g. RTW_PDF_MIXTURE */
    int32_t p0_gen;  /* mixture child 0 (cosine) or -1                          */
    int32_t p1_gen;  /* mixture child 1 (rect x/y/z) or -1                      */
    int32_t flip;
    float rect[5];   /* p1's hitRectData a0,a1,b0,b1,k                          */
    float bias;
} rtw_pdf; /* 40 B */

/* Camera kinds: the reference's scene/camera.cuh:35-56 `cameraType` values (its OptiX-7 path only ever builds type 0,
 * shaders/camera.cu:11-19; the other two are defined by scene/ioCamera.h:118-179 and never instantiated).
 *   RTW_CAM_PERSPECTIVE   origin (+ lens offset), direction = lower_left + s*horizontal + t*vertical - origin
 *   RTW_CAM_ENVIRONMENT   origin; a = (cos(2 pi s) sin(pi t), -cos(pi t), sin(2 pi s) sin(pi t)); direction = normalize(a.x u + a.y v + a.z w)
 *   RTW_CAM_ORTHOGRAPHIC  origin = lower_left + s*horizontal + t*vertical + camera origin (as camera.cuh:52 states it: the origin
 *                         enters twice when lower_left is built the way ioOrthographicCamera builds it); direction = -normalize(w)
 * Only the perspective camera draws a lens sample (two draws, consumed even at lens radius 0: camera.cu:11-19); the other
 * two take no seed in the reference and draw nothing (visible in the TEA+LCG stream; Philox raygen draws are positional).
 * time0 / time1 are the shutter of every kind: the reference's environment and orthographic constructors take t0, t1 and drop
 * them (scene/ioCamera.h:126-128, 149-151; neither is ever built there), the host description's pass them on. */
typedef enum rtw_camera_type { RTW_CAM_PERSPECTIVE = 0, RTW_CAM_ENVIRONMENT = 1, RTW_CAM_ORTHOGRAPHIC = 2 } rtw_camera_type;

typedef struct rtw_camera {
    float origin[3];
    float u[3], v[3], w[3];
    float lower_left[3];
    float horizontal[3];
    float vertical[3];
    float lens_radius; /* SysParamter.cameraLensRadius (never set by the reference: 0) */
    float time0, time1;
} rtw_camera; /* 96 B */

/* The scene blob is this header followed by the arrays at the given byte offsets
 * (all offsets relative to the start of the header, 16-byte aligned). */
typedef struct rtw_scene_header {
    uint32_t magic;   /* RTW_SCENE_MAGIC */
    uint32_t version; /* RTW_SCENE_VERSION */
    uint32_t total_bytes;
    uint32_t n_prims, n_xforms, n_materials, n_textures, n_lights;
    uint32_t off_prims, off_xforms, off_materials, off_textures, off_lights;
    int32_t sky_light; /* SysParamter.skyLight */
    uint32_t off_texdata;   /* byte offset of the texture data section (0 = none)  */
    uint32_t texdata_bytes; /* its size; rtw_texture.data counts 4-byte words in it */
    rtw_camera camera;
    rtw_pdf pdf;
    int32_t camera_type; /* rtw_camera_type (these 8 bytes were rtw_pdf.reserved, always 0, before the cameras of SURVEY 8f rank 4) */
    uint32_t reserved;
} rtw_scene_header;

/* Estimators. The default reproduces the reference, including what makes its images
 * physically off: the stray factor 2 in the cosine sampler, light samples weighted by the power heuristic
 * while emitter hits are counted in full (Q3), the pdf rectangle of the scene instead of the chosen light's own (Q12,
 * and every light but the first), an un-normalised incoming direction in the metal reflection (Q5).
 * RTW_EST_CORRECTED fixes those: cosine-weighted scattering, each listed light sampled over its own parallelogram with
 * the plain area-measure estimator, emitter hits of listed lights counted only where no light sample stood in for them,
 * media that scatter only inside their extent (Q9), rays started 1e-3 (not 1e-6) away from the hit point.
 * RTW_EST_CORRECTED_NO_NEE is the same integrand estimated without light sampling (every emitter hit counts): slow to
 * converge, but an independent check - both converge to the same image.
 * RTW_EST_MIXTURE is the same integrand again, estimated the way the reference's pdf/ callables set out to ("The Rest of
 * Your Life", mixture_pdf): at a diffuse vertex the scattered direction is drawn from the light list or
 * from the cosine lobe with probability 1/2 each, the throughput carries albedo * p_cos / (p_cos / 2 + p_light / 2) with
 * p_light the true solid-angle density of the light list (the reference's rect_*_value stubs return constants), no
 * shadow probe is traced and every emitter hit counts - one-sample multiple importance sampling, balance heuristic.
 * What the three corrected estimators share beside the integrand:
 *   Listed emitters. A light definition describes a primitive when that primitive is an untransformed rectangle
 *     (xform 0) with a diffuse-light material, vec_u and vec_v are exactly its edges (a1 - a0 along its first in-plane
 *     axis, b1 - b0 along its second, in x, y, z order), position is exactly its (a0, b0) corner in those two axes, and
 *     |position[axis] - k| <= 0.01 * max(a1 - a0, b1 - b0). The first such primitive in scene order is taken. The
 *     definition is then sampled on the primitive's plane (position[axis] = k; Cornell: 554 -> 554.9) and
 *     the primitive is a listed emitter: under RTW_EST_CORRECTED its hit is dropped after a vertex that took a light
 *     sample and counts in full at the camera and after a specular vertex. Emitters that no definition describes
 *     always count. RTW_EST_REFERENCE reads the definitions as they are and knows no listed emitters.
 *   The shadow probe runs along the unit direction over (5e-5, r - 5e-5) under RTW_EST_REFERENCE (closehit.cu:100) and
 *     over (1e-3, r - 1e-3) under RTW_EST_CORRECTED, like every ray the corrected estimators start: whatever lies
 *     within 1e-3 of either end does not shadow. It is traced where the light sample's pdf and the BSDF's are positive
 *     and the BSDF value is not zero (closehit.cu:89-95: none at a black surface). It is a traversal like any other:
 *     a medium on its way draws a free flight from the path's generator and blocks it with probability 1 - T.
 *   p_light of RTW_EST_MIXTURE counts a light from either side: the light branch aims at the drawn point whichever
 *     way the definition's normal looks, so the density of a direction is the sum over the parallelograms it crosses of
 *     r^2 / (n_lights * area * |cos|). */
typedef enum rtw_estimator {
    RTW_EST_REFERENCE = 0,
    RTW_EST_CORRECTED = 1,
    RTW_EST_CORRECTED_NO_NEE = 2,
    RTW_EST_MIXTURE = 3
} rtw_estimator;

typedef struct rtw_params {
    int32_t width, height;     /* full image (launch dimensions of the reference's optixLaunch) */
    int32_t spp;               /* samples per pixel rendered by this call                       */
    int32_t max_depth;         /* SysParamter.maxRayDepth                                       */
    uint32_t seed;
    int32_t row0, row1;        /* rows [row0,row1) of the full image are rendered (row shard of one GPU)      */
    int32_t rng_kind;          /* rtw_rng_kind                                                  */
    int32_t sample_offset;     /* first sample index (progressive / resumed renders)            */
    int32_t samples_per_pass;  /* paths kept in flight = rows*width*samples_per_pass; 0 = auto  */
    int32_t row_stride;        /* 0 or 1: every row of [row0,row1). k > 1: rows row0, row0+k, row0+2k ... < row1
                                  (interleaved shard: rank g of N uses row0=g, row1=height, row_stride=N, which
                                  balances the ranks); the output holds those rows consecutively               */
    int32_t estimator;         /* rtw_estimator: 0 = the reference's estimator, quirks and all (the parity mode)  */
} rtw_params;

/* kernels of the wavefront loop, index into the per-kernel arrays of rtw_stats */
enum { RTW_K_FIRST = 0, RTW_K_SHADE = 1, RTW_K_TRACE = 2, RTW_K_BOUNCE = 3, RTW_K_PATH = 4, RTW_K_COUNT = 5 };

typedef struct rtw_stats {
    uint64_t samples;           /* camera paths started                                              */
    uint64_t segments;          /* radiance ray segments traced (one optixTraverse of raygen.cu:41) */
    uint64_t shadow_rays;       /* occlusion probes traced (closehit.cu:95-101)                     */
    uint64_t algorithmic_bytes; /* 128*segments + 32*samples                 */
    uint64_t bounce_launches;   /* launches of the wavefront-loop kernels (all four kinds)          */
    uint64_t reserved;
    double seconds;             /* device time of the whole render call (events on the stream)     */
    double bounce_seconds;      /* device time inside the wavefront loops (first launch to last)   */
    /* per kernel kind, measured with HIP events recorded on the launch stream around every launch */
    double kernel_seconds[RTW_K_COUNT];
    uint64_t kernel_launches[RTW_K_COUNT];
    uint64_t kernel_segments[RTW_K_COUNT]; /* radiance segments shaded by that kernel (k_trace: path slots traced = a radiance ray and / or its queued probe).
                                            * Segments the host counts without a kernel - the one-segment samples of pixels that certainly see nothing,
                                            * see RTW_CULL below - are in `segments` and in no entry here. */
} rtw_stats;

typedef struct rtw_ctx rtw_ctx;

int rtw_abi_version(void);

/* Replaces Director::initContext (Director.cpp:106-122).
 * n_devices == 1: one context on device_ids[0] (NULL: device 0).
 * n_devices  > 1: a group. rtw_upload_scene copies the scene to every device; rtw_render / rtw_render_device split the
 * rows of the call into n_devices interleaved shards (shard g: every n_devices-th row of the call's rows, starting at its
 * g-th), render shard g on device_ids[g] from that device's own host thread (created here, alive until rtw_destroy: no
 * thread is created per call), every device pushes its float4 shard to device_ids[0] with one hipMemcpyPeerAsync on its
 * own stream as soon as it is done (n concurrent xGMI transfers) and the rows are interleaved there: the caller sees one
 * frame, bit-identical to the single-device render. Entries of device_ids may repeat (two shards on one GPU). The caller
 * stays single-threaded; a worker that fails or throws reports through the call's return code. */
int rtw_create(rtw_ctx** out, int n_devices, const int* device_ids);

/* Replaces createSBT + initLaunchParams + the per-primitive optixAccelBuild calls
 * (Director.cpp:628-885, 483-553; geometry/io*.h init()). Copies the blob, builds the BVH. */
int rtw_upload_scene(rtw_ctx* ctx, const void* scene_blob, size_t bytes);

/* Replaces optixLaunch + the D2H copy (Director.cpp:982-984, 999-1000).
 * rgba_out: host, rows*width float4 (rows = the rows of [row0,row1) the shard owns: all of them, or every
 * row_stride-th), LINEAR mean radiance of samples [sample_offset, sample_offset+spp), alpha 1; row r of the output is
 * image row row0 + r*max(row_stride,1); image row 0 is the bottom row, like the reference's frame buffer.
 * A sample is the loop of raygen.cu:28-87 (tests/path_ref.py holds the oracle and every kernel to it):
 *   At most max_depth segments are traced (max_depth = 0: none, the sample is 0). Every segment adds radiance * T - an emitter's
 *     or the sky's radiance, a light sample - to the sample, T the throughput, 1 at the camera. A miss, an emitter, a
 *     cancelled scatter and the max_depth-th segment end the sample; otherwise T *= attenuation of the vertex.
 *   Russian roulette after the third hit and after every later one (raygen.cu:74-82), on the throughput that already holds
 *     that hit's attenuation: p = max(T.x, T.y, T.z), under RTW_EST_MIXTURE (whose weights reach 2) capped at 1; one draw xi is
 *     consumed - also after the last allowed hit, where it decides nothing -, the sample ends when p < xi, else T *= 1 / p. A
 *     black throughput (p = 0) therefore ends the sample at that hit.
 *   removeNaNs (raygen.cu:17-24) per sample and per channel: a NaN channel counts as 0, the other channels stay (an infinite
 *     emitter behind a vertex with a zero channel gives inf, inf, 0), and the sample still counts in spp.
 *   Spheres: a negative radius is allowed and turns the shading normal (P - C) / radius inwards (a hollow sphere, a room seen
 *     from inside); the intersection depends on radius * radius alone and the bounds use |radius|. */
int rtw_render(rtw_ctx* ctx, const rtw_params* params, float* rgba_out, rtw_stats* stats);

/* Same render, result left in device memory (d_rgba: device pointer on device_ids[0], same layout). The work is ordered
 * on hip_stream (a hipStream_t passed as void*): the render starts after what that stream holds and the final frame is
 * written on it. NULL (which is also HIP's legacy default stream handle) selects the context's own non-blocking stream,
 * which is NOT ordered with the default stream: pass a stream of your own (or hipStreamLegacy / hipStreamPerThread) when
 * d_rgba has pending work. Returns when done. rtw_stats.kernel_seconds is filled from HIP events recorded on the launch
 * streams around every kernel (only when stats != NULL; RTW_KERNEL_TIMING=0 turns the events off).
 * Tuning knobs are environment variables read per call (csrc/rtw_plan.h lists them); none changes the image or the counts.
 * RTW_CULL=0 makes renders of scenes without a sky light trace the pixels whose camera rays cannot reach any primitive
 * as well (by default such pixels are black and their samples counted without being traced). */
int rtw_render_device(rtw_ctx* ctx, const rtw_params* params, void* d_rgba, void* hip_stream,
                      rtw_stats* stats);

/* Replaces Director::destroy (Director.cpp:66-104). */
int rtw_destroy(rtw_ctx* ctx);

/* Message of the last failing call on this context (what OPTIX_CHECK / CUDA_CHECK would have thrown,
 * sutil/Exception.h); valid until the next call on the context. */
const char* rtw_last_error(rtw_ctx* ctx);

/* Stand-in for the reference's output stage, the OptiX AI denoiser (Director::initDenoiser, Director.cpp:887-949,
 * invoked at :986-997 on the beauty layer alone, LDR model, no albedo / normal guides). The AI model is closed; this is
 * an edge-avoiding a-trous wavelet filter on the same input (Dammertz et al. 2010, colour edge-stopping only):
 * `iterations` passes with a 5x5 B3-spline kernel at hole sizes 1, 2, 4 ..., each tap weighted by
 * 1 / (1 + |c_p - c_q|^2 / sigma_i^2), sigma_i = sigma * 2^-i. rgba_in / rgba_out: host, width*height float4, may not
 * alias; alpha is copied. Meant for display-encoded values in [0, 1] (the reference's LDR model sees sqrt(colour));
 * not part of rtw_render: 4096-spp frames need none. iterations in 1..8, sigma > 0. */
int rtw_denoise(rtw_ctx* ctx, const float* rgba_in, float* rgba_out, int32_t width, int32_t height, int32_t iterations, float sigma);

/* Guide buffers (AOVs) of the first hit, for denoisers and compositing (the guide layers - albedo, normal - that the OptiX
 * denoiser under the reference's Director::initDenoiser, Director.cpp:887-949, accepts and the reference never fills).
 * Every pointer is host memory of the shard's rows*width pixels (same rows, same order as rtw_render's output), or NULL
 * for a buffer the caller does not want. */
typedef struct rtw_guides {
    float* albedo;  /* rows*width float4: mean first-hit albedo; alpha = fraction of the samples that hit something      */
    float* normal;  /* rows*width float4: mean first-hit world-space shading normal (not renormalised); alpha as albedo */
    float* depth;   /* rows*width float: t * |d| of sample sample_offset's camera ray (distance to the hit), +inf: miss */
    int32_t* prim;  /* rows*width int32: primitive index hit by sample sample_offset's camera ray, -1: miss            */
} rtw_guides;

/* First-hit guides of samples [sample_offset, sample_offset+spp) of the rows rtw_render would render with the same params.
 *   Rays: the same camera rays as rtw_render (raygen: jitter, lens sample, ray time and gather time from the same draws
 *     of the same generator, row0 / row1 / row_stride / seed / rng_kind honoured), so guide edges line up with the beauty's.
 *     max_depth, estimator and samples_per_pass are ignored; the ray starts at the reference's 1e-6.
 *   Normal: the world-space shading normal at the first hit, exactly the vector the closest-hit code hands to the material
 *     (the one RTW_MAT_NORMAL turns into a colour): rectangles +-axis by their flip flag, spheres (p - c) / r.
 *   Albedo: lambertian, metal, isotropic: the texture value at the hit (the shading code's texture evaluation, same
 *     arguments); dielectric: (1,1,1); normal material: its colour n * 0.5 + 0.5 (fma); diffuse light: the emitted value
 *     under the shading code's front-face rule (dot(n, d) < 0; 0 on the back), clamped to [0,1].
 *   Means: albedo and normal are summed over the samples in the summation order of RTW_SUM_BLOCK / RTW_SUM_UNIT_BLOCKS
 *     (plain ascending order for spp <= 16), then divided by spp. A miss adds 0 (the sky is not a hit).
 *   Depth and prim come from the first sample (sample_offset) alone; a miss gives depth +inf, prim -1.
 *   Participating media are transparent to the guides (volume primitives are skipped): a medium's first scatter is random
 *     and a guide must not be noisy.
 *   Groups (n_devices > 1): the guides are rendered on device_ids[0]; the bits are those of a single-device context.
 *   Errors: RTW_ERR_NO_SCENE without a scene; RTW_ERR_INVALID_ARG for bad params or when all four pointers are NULL.
 *   stats (may be NULL): samples = segments = rows*width*spp (one camera segment per sample), seconds = device time. */
int rtw_render_guides(rtw_ctx* ctx, const rtw_params* params, const rtw_guides* out, rtw_stats* stats);

/* rtw_denoise steered by guides (edge-avoiding a-trous with albedo and normal edge-stopping, Dammertz et al. 2010): the
 * same 25 taps, tap order, border clamp, B3 kernel and colour weight as rtw_denoise, the colour weight then divided by
 * (1 + |a_p - a_q|^2 / sigma_albedo^2) and by (1 + |n_p - n_q|^2 / sigma_normal^2), squared norms summed as
 * (x^2 + y^2) + z^2 over the first three channels. The colour sigma halves per pass as in rtw_denoise; the guide sigmas
 * stay fixed. With constant guides both divisors are exactly 1 and the result is bit-identical to rtw_denoise.
 * rgba_in, albedo, normal, rgba_out: host, width*height float4 (albedo and normal as rtw_render_guides writes them);
 * rgba_out may alias none of them; alpha is copied. iterations in 1..8; sigma, sigma_albedo, sigma_normal > 0. */
int rtw_denoise_guided(rtw_ctx* ctx, const float* rgba_in, const float* albedo, const float* normal, float* rgba_out,
                       int32_t width, int32_t height, int32_t iterations, float sigma, float sigma_albedo, float sigma_normal);

/* Adaptive sampling: every pixel renders until its noise estimate falls below a target, or up to a sample cap.
 *   Cap and layout: params->spp is the cap, a multiple of RTW_SUM_BLOCK. Every other field of rtw_params means what it means
 *     for rtw_render (rows, row_stride, seed, rng_kind, sample_offset, estimator, samples_per_pass); the outputs use rtw_render's
 *     row layout. rgba_out is required (rows*width float4); spp_out (rows*width int32) and error_out (rows*width float) may be NULL.
 *   Checkpoints: a fixed sequence that depends on (min_spp, step_spp, params->spp) alone: n_0 = min_spp,
 *     n_{k+1} = min(cap, n_k + step), step = step_spp or, when step_spp is 0, n_k / 2 rounded up to a multiple of RTW_SUM_BLOCK
 *     (64 to 4096: 64 96 144 224 336 512 768 1152 1728 2592 3888 4096). It never depends on the device, tuning knobs or timing.
 *   Samples per pixel: pixel p renders samples [sample_offset, sample_offset + n_p), n_p a checkpoint; a pixel that stopped never
 *     resumes. Its colour is, bit for bit, rtw_render's colour of that pixel with spp = n_p.
 *   Error estimate: batch means over the pixel's RTW_SUM_BLOCK-sample block sums S_b (the bits both pipelines form):
 *     y_b = ((0.2126f*S.x + 0.7152f*S.y) + 0.0722f*S.z) * 0.0625f in fp32, no contraction; M1 = sum y_b and M2 = sum y_b*y_b in
 *     fp64, in block order; with B = n / RTW_SUM_BLOCK: m = M1 / B, v = max(0, (M2 - M1*m) / (B - 1)), se = sqrt(v / B),
 *     err = se / (2 sqrt(max(m, 1e-3))) in fp64, rounded to fp32. err is the standard error of the display value sqrt(Y), so a
 *     threshold reads as a fraction of full display scale. A NaN err compares false: that pixel goes on.
 *   Stop rule: at checkpoint n_k an active pixel stops if n_k is the cap; otherwise if its own err < threshold and, with dilate = 1,
 *     every still-active pixel of its 3x3 neighbourhood (in the output's own rows, clamped at the edges) has err < threshold too.
 *     A pixel that stopped earlier never blocks a neighbour.
 *   Shards: with dilate = 0 every row of a shard (row0 / row1 / row_stride) equals the same row of the full-frame adaptive render;
 *     with dilate = 1 that holds for whole frames only (the neighbourhood is the shard's own rows).
 *   error_out: the pixel's err at its last checkpoint.
 *   Groups (n_devices > 1): the render runs on device_ids[0], as rtw_render_guides does.
 *   stats (may be NULL): samples = sum of n_p; segments, shadow_rays, kernel_seconds and kernel_launches summed over the passes
 *     (the list kernels count under their base kinds); seconds = device time from the call's first event to its last;
 *     algorithmic_bytes = 128*segments + 32*samples.
 *   Errors: RTW_ERR_NO_SCENE without a scene; RTW_ERR_INVALID_ARG for bad params, a cap or min_spp that is not a multiple of
 *     RTW_SUM_BLOCK, min_spp < 2*RTW_SUM_BLOCK or above the cap, step_spp < 0 or not a multiple of RTW_SUM_BLOCK, a negative or
 *     NaN threshold, dilate not 0 or 1. The context stays usable after an error. */
typedef struct rtw_adaptive {
    int32_t min_spp;   /* samples every pixel gets; a multiple of RTW_SUM_BLOCK, >= 2 * RTW_SUM_BLOCK, <= params->spp      */
    int32_t step_spp;  /* 0: each pass adds half of what the pixel has (rounded up to RTW_SUM_BLOCK); else a fixed multiple */
    float threshold;   /* a pixel stops once its error estimate is below this (strict <); 0: no pixel stops early; +inf ok   */
    int32_t dilate;    /* 0: each pixel decides alone; 1: a pixel also continues while an active 3x3 neighbour is above it  */
} rtw_adaptive;     /* 16 B */

int rtw_render_adaptive(rtw_ctx* ctx, const rtw_params* params, const rtw_adaptive* ad, float* rgba_out, int32_t* spp_out,
                        float* error_out, rtw_stats* stats);

/* Accumulation sessions: a device-resident running sum of a shard's samples that the caller adds to as often as it likes, reads
 * whenever it likes and saves to or restores from host memory - progressive previews, checkpoints, "another 256 spp". The frame
 * after n samples is rtw_render's frame with spp = n, bit for bit, whatever the schedule of adds: the session keeps the summation
 * order of RTW_SUM_BLOCK / RTW_SUM_UNIT_BLOCKS (blocks of 16, units of 128 counted from sample_offset, units in order) by carrying
 * the open unit from add to add.
 *   One session per context. Groups (n_devices > 1): the session runs on device_ids[0], as rtw_render_guides does.
 *   rtw_accum_begin: params means what it means for rtw_render (rows, row_stride, seed, rng_kind, sample_offset, estimator,
 *     samples_per_pass), except that params->spp is the CAP, the most samples per pixel the session may ever hold: a positive
 *     multiple of RTW_SUM_BLOCK with sample_offset + cap <= INT32_MAX (the cap costs nothing: the state does not depend on it).
 *     flags: 0 or RTW_ACCUM_ERROR (keep the batch-means moments, 16 more bytes per pixel, so that a read can return the error map;
 *     every block sum then reaches memory, as in rtw_render_adaptive's passes). The state starts at zero samples.
 *     Errors: RTW_ERR_NO_SCENE without a scene; RTW_ERR_INVALID_ARG for bad params or flags, an empty shard, or a session that is
 *     already active.
 *   rtw_accum_add: renders samples [sample_offset + done, sample_offset + done + spp) of every pixel of the shard into the state and
 *     returns when done. spp is a positive multiple of RTW_SUM_BLOCK with done + spp <= cap, else RTW_ERR_INVALID_ARG (and the session
 *     is as it was). The launches are rtw_render's (tuning knobs as there). stats (may be NULL) describes this add alone; samples,
 *     segments and shadow_rays summed over the adds equal the counts of the one-shot render (rtw_accum_status keeps the sums).
 *     An add that fails on the device ends the session.
 *   rtw_accum_read / rtw_accum_read_device: the frame of the done samples - rtw_render's / rtw_render_device's output with spp = done,
 *     same layout, bit for bit; read_device is ordered on hip_stream as rtw_render_device is (NULL: the context's own stream) and
 *     returns when the frame is written. Reading changes nothing: add, read, add is fine. error_out (may be NULL; rows*width float)
 *     is rtw_render_adaptive's error_out for spp = min_spp = done (one checkpoint), bit for bit: the same formula over the same block
 *     sums in the same fp64 order. Errors: RTW_ERR_INVALID_ARG without a session, at done = 0, with a NULL frame pointer, and for
 *     error_out on a session without RTW_ACCUM_ERROR or with done < 2 * RTW_SUM_BLOCK.
 *   rtw_accum_status: fills *out; without a session active = 0 and everything else is 0. Never fails on a valid context.
 *   rtw_accum_save: copies the session into blob (host memory), bytes == state_bytes of rtw_accum_status: a 128-byte header (magic,
 *     version, flags, the params of begin, done, the three running counts, a 64-bit FNV-1a fingerprint of the uploaded scene blob)
 *     followed by the per-pixel arrays: the closed units' sums, the open unit's sums (rows*width float4 each) and, with
 *     RTW_ACCUM_ERROR, the moments (rows*width pairs of doubles). Native byte order. The session goes on.
 *   rtw_accum_restore: starts a session from such a blob, in this or any other context or process: it needs an uploaded scene with
 *     the same fingerprint and no active session. The restored session continues exactly. RTW_ERR_INVALID_ARG for a blob that is
 *     not a saved session (magic, version), whose size, params or counts do not fit together, or that belongs to another scene; the
 *     context then stays usable and without a session.
 *   rtw_accum_end: frees the session (RTW_ERR_INVALID_ARG when there is none). rtw_upload_scene and rtw_destroy end it too.
 *   Independence: the session owns its state. Between two adds rtw_render, rtw_render_device, rtw_render_guides, rtw_render_adaptive
 *     and rtw_denoise* on the same context work as before and do not change it. */
enum { RTW_ACCUM_ERROR = 1 };
typedef struct rtw_accum_info {
    int32_t active;       /* 1: a session exists                                                    */
    int32_t done;         /* samples per pixel it holds                                             */
    int32_t cap;          /* params.spp of begin                                                    */
    uint32_t flags;
    uint64_t state_bytes; /* what rtw_accum_save writes                                             */
    uint64_t samples, segments, shadow_rays; /* summed over the adds (restored sessions: and over those before the save) */
    rtw_params params;    /* as given to begin                                                      */
} rtw_accum_info;      /* 96 B */

int rtw_accum_begin(rtw_ctx* ctx, const rtw_params* params, uint32_t flags);
int rtw_accum_add(rtw_ctx* ctx, int32_t spp, rtw_stats* stats);
int rtw_accum_read(rtw_ctx* ctx, float* rgba_out, float* error_out);
int rtw_accum_read_device(rtw_ctx* ctx, void* d_rgba, void* hip_stream);
int rtw_accum_status(rtw_ctx* ctx, rtw_accum_info* out);
int rtw_accum_save(rtw_ctx* ctx, void* blob, size_t bytes);
int rtw_accum_restore(rtw_ctx* ctx, const void* blob, size_t bytes);
int rtw_accum_end(rtw_ctx* ctx);

/* Ray queries: closest-hit and occlusion queries on the caller's own rays, in batches (what an OptiX user does with a raygen
 * program of their own over optixTrace: visibility and ambient-occlusion passes, picking, range and lidar simulation, form
 * factors). Nothing here starts from the scene's camera.
 *   Rays: `rays` holds n*8 floats (ox, oy, oz, dx, dy, dz, tmin, tmax), rtw_debug_intersect's layout. Directions need not be
 *     normalised: t is the ray parameter. ray_time and gather_time hold n floats each or are NULL (0 for every ray); they mean what
 *     they mean for rtw_debug_intersect: the ray time places a moving sphere's motion transform, the gather time its centre.
 *     Participating media are transparent, as they are for the guides (volume primitives are skipped: a medium's hit is a random draw).
 *   Outputs: every pointer of rtw_hits holds n entries, or is NULL for an output the caller does not want. Outputs may not alias
 *     the inputs or each other.
 *   RTW_CAST_CLOSEST: the candidates are the non-volume primitives with tmin < t < tmax, the hit is the minimum over (t, primitive
 *     index). t[i] and prim[i] carry the bits rtw_debug_intersect returns for that ray: t = tmax and prim = -1 on a miss.
 *     material[i] = prims[prim].material, -1 on a miss. normal[i].xyz is the world-space shading normal, exactly the vector the
 *     closest-hit code hands to the materials: rectangles +-axis by their flip flag, taken to world space, unit length; spheres
 *     (P_world - C_object) / r through the inverse transpose, NOT normalised; moving spheres with the centre at the
 *     gather time. normal[i].w = 1.0f when dot(normal, d) < 0 (the shading code's front-face rule), else 0.0f. uv[i] are the texture
 *     coordinates the image textures are fetched at (spheres from the shading normal, rectangles from the object-space hit point).
 *     On a miss normal = (0, 0, 0, 0) and uv = (0, 0).
 *   RTW_CAST_ANY: prim[i] = -1 when no candidate lies in the interval, else the index of a non-volume primitive that does - which
 *     one is unspecified, but it is the same from call to call for one uploaded scene and one set of upload knobs. t[i] = tmax.
 *     material, normal and uv must be NULL (RTW_ERR_INVALID_ARG otherwise). Guarantee: prim[i] >= 0 exactly when RTW_CAST_CLOSEST
 *     returns a hit for the same ray - the two walks are identical up to the first accepted candidate - NaN and inf rays included.
 *   The result for ray i depends on ray i alone: not on n, the launch geometry or how rtw_cast cuts the batch into chunks.
 *   rtw_cast: host pointers. The rays are staged through device buffers the context keeps and grows (no allocation per call once
 *     they are large enough), in chunks of at most RTW_CAST_CHUNK rays (an environment variable read per call, csrc/rtw_plan.h).
 *   rtw_cast_device: device pointers on the context's device; rays and normal 16-byte aligned, uv 8-byte aligned. Ordered on
 *     hip_stream exactly as rtw_render_device is; returns when the results are written. NULL selects the context's own
 *     non-blocking stream, NOT the legacy default stream (whose handle NULL also is): a caller whose rays are still being written
 *     on stream 0 passes hipStreamLegacy, or a stream of its own, or synchronises first. It allocates nothing per call. One persistent launch: the grid is what the device holds at once, lanes stride over
 *     64-bit ray indices.
 *   Groups (n_devices > 1): the query runs on device_ids[0], as rtw_render_guides does; the bits are a single-device context's.
 *   An accumulation session on the context is not disturbed.
 *   stats (may be NULL): segments = n (closest) or shadow_rays = n (any), samples = 0, seconds = device time from the call's first
 *     event to its last; the per-kernel arrays are 0.
 *   Errors: RTW_ERR_NO_SCENE without a scene; RTW_ERR_INVALID_ARG for a mode other than the two, n > 2^31 - 1, with n > 0 a NULL
 *     rays or out or an rtw_hits whose pointers are all NULL, outputs RTW_CAST_ANY does not have, and (rtw_cast_device) a
 *     misaligned rays, normal or uv. n = 0 is RTW_OK and launches nothing. The context stays usable after an error. */
enum { RTW_CAST_CLOSEST = 0, RTW_CAST_ANY = 1 };
typedef struct rtw_hits {
    float* t;          /* n floats                                                   */
    int32_t* prim;     /* n int32                                                    */
    int32_t* material; /* n int32                                                    */
    float* normal;     /* n float4: xyz shading normal, w = 1.0f front face / 0.0f   */
    float* uv;         /* n float2                                                   */
} rtw_hits;            /* 40 B */

int rtw_cast(rtw_ctx* ctx, const float* rays, const float* ray_time, const float* gather_time, size_t n, int32_t mode,
             const rtw_hits* out, rtw_stats* stats);
int rtw_cast_device(rtw_ctx* ctx, const float* rays, const float* ray_time, const float* gather_time, size_t n, int32_t mode,
                    const rtw_hits* out, void* hip_stream, rtw_stats* stats);

/* Radiance queries: the light arriving along the caller's own rays, estimated by whole paths, in batches (what an OptiX user does
 * with a raygen program of their own: irradiance and light probes, lightmap texels, cameras the library does not know, foveated or
 * importance-driven pixel sets, radiance fields with the tensors left on the device). A radiance query is a camera path of rtw_render
 * whose camera ray is replaced: everything after the camera ray - traversal (media included), closest-hit and miss programs, light
 * sampling with its shadow probe, removeNaNs, Russian roulette - is rtw_render's, operation for operation.
 *   Rays: `rays` holds n*8 floats in rtw_cast's layout (ox, oy, oz, dx, dy, dz, tmin, tmax); directions of any length. tmin and tmax
 *     bound the FIRST segment only; later segments use the estimator's own start distance (1e-6, or 1e-3 for estimators other than
 *     RTW_EST_REFERENCE) and 1e27f, as a render does. A first segment that finds nothing inside (tmin, tmax) is a miss (sky or black).
 *   Draws: sample s of ray i consumes exactly what a perspective camera path of rtw_render consumes for the pixel with stream key
 *     k = key_offset + i (mod 2^32; a render's key is width*y + x) and sample index sample_offset + s. Philox: block (k, sample, 0, 0),
 *     whose words 0-3 (jitter, lens) are drawn and unused and whose low bytes give the gather-time draw, then stream 1 from draw 0 and
 *     ray times from stream 2. TEA+LCG: tea<64>(k, sample), four LCG draws discarded, the path's two generator words, then the
 *     gather-time draw. The gather time spans the uploaded scene's camera.time0 / time1; ray times are the raw uniforms in [0, 1)
 *     (rtw_rng_kind above).
 *     Hence: a scene whose header carries ray i as a perspective camera with horizontal = vertical = 0 and lens_radius = 0 (origin = o,
 *     lower_left with lower_left - o = d in float32), rendered by rtw_render at a pixel with stream key k, gives ray i's result, bit for bit.
 *   Output: rgba_out[i] = the sum of the samples' radiance in the summation order of RTW_SUM_BLOCK / RTW_SUM_UNIT_BLOCKS counted from
 *     sample_offset, divided by (float)spp, alpha 1.0f. The result for ray i depends on its ray, its key and the params alone: not on
 *     n, the launch geometry, how the batch is cut into chunks or ranges, or tuning knobs.
 *   rtw_radiance: host pointers. The rays are staged through a slab the context keeps and grows, in chunks of at most
 *     RTW_RADIANCE_CHUNK rays (an environment variable read per call, csrc/rtw_plan.h); chunk c runs with the key of its first ray.
 *   rtw_radiance_device: device pointers on the context's device, both 16-byte aligned. Ordered on hip_stream exactly as
 *     rtw_cast_device is; returns when the results are written. NULL selects the context's own non-blocking stream, NOT the legacy
 *     default stream: a caller whose rays are still being written on stream 0 passes hipStreamLegacy, or a stream of its own, or
 *     synchronises first. Persistent launches: the grid is what the device holds at once, waves take jobs of consecutive (ray,
 *     128-sample unit) pairs from a queue. Calls of at most 128 spp write the means directly; longer ones keep one 16-byte sum per ray
 *     and unit in a scratch slab of the context (n * ceil(spp / 128) * 16 B, capped by RTW_RADIANCE_SLAB_BYTES: a larger batch runs as
 *     consecutive ray ranges) and add them in order. It allocates nothing per call once the context's scratch is large enough.
 *   Groups (n_devices > 1): the query runs on device_ids[0], as rtw_render_guides does; the bits are a single-device context's.
 *   An accumulation session on the context is not disturbed.
 *   stats (may be NULL): samples = n*spp, segments and shadow_rays as counted by the kernel (a render's counts of the same paths),
 *     seconds = device time from the call's first event to its last, algorithmic_bytes = 128*segments + 32*samples; the per-kernel
 *     arrays are 0.
 *   Errors: RTW_ERR_NO_SCENE without a scene; RTW_ERR_INVALID_ARG for NULL params, spp <= 0, max_depth < 0, a bad rng_kind or
 *     estimator, sample_offset < 0 or sample_offset + spp > INT32_MAX, reserved != 0, n > 2^31 - 1, with n > 0 a NULL rays or output,
 *     and (rtw_radiance_device) a misaligned rays or output. n = 0 is RTW_OK and launches nothing. The context stays usable after an
 *     error. */
typedef struct rtw_radiance_params {
    int32_t spp;            /* samples per ray, > 0                                          */
    int32_t max_depth;      /* as rtw_params.max_depth (0: every ray returns 0)              */
    uint32_t seed;
    int32_t rng_kind;       /* rtw_rng_kind                                                  */
    int32_t sample_offset;  /* first sample index; sample_offset + spp <= INT32_MAX          */
    int32_t estimator;      /* rtw_estimator                                                 */
    uint32_t key_offset;    /* ray i draws from the stream of "pixel" key_offset + i (mod 2^32) */
    uint32_t reserved;      /* 0, else RTW_ERR_INVALID_ARG                                   */
} rtw_radiance_params;      /* 32 B */

int rtw_radiance(rtw_ctx* ctx, const float* rays, size_t n, const rtw_radiance_params* params, float* rgba_out, rtw_stats* stats);
int rtw_radiance_device(rtw_ctx* ctx, const float* rays, size_t n, const rtw_radiance_params* params, void* d_rgba, void* hip_stream,
                        rtw_stats* stats);

/* Probes: irradiance and ambient occlusion at surface points, integrated by the library (what a lightmap baker, an irradiance cache
 * or an ambient-occlusion pass calls). rtw_cast and rtw_radiance take one fixed ray per index; a probe takes a different direction
 * for every sample, drawn on the device from the sample's own random stream.
 *   Probes: `probes` holds n*8 floats (px, py, pz, nx, ny, nz, tmin, tmax): rtw_cast's ray layout with the normal (any non-zero
 *     length) in the direction's place, so a tensor built from rtw_cast's hit points and normals is a probe tensor.
 *   Direction: for sample s of probe i take the stream key k = key_offset + i (mod 2^32) and the sample index S = sample_offset + s.
 *     r1 and r2 are the first two raygen uniforms of that path, the ones rtw_radiance consumes and drops - Philox: the 24-bit
 *     uniforms of words 0 and 1 of block (k, S, 0, 0) under key (seed, 0); TEA+LCG: the first two lcg_rnd values of tea<64>(k, S).
 *     The direction is the Lambertian material's own basis and lobe in its corrected (cosine-weighted) form, operation for operation
 *     as the closest-hit code writes it:
 *       w = normalize3(n); a = (w.x > 0.9f || w.x < -0.9f) ? (0,1,0) : (1,0,0); v = normalize3(cross3(w, a)); u = cross3(w, v);
 *       sincos2pi(r1, sn, cs); sq = sqrt(r2); lx = cs * sq; ly = sn * sq; lz = sqrt(1 - r2);
 *       d = normalize3(fma(lz, w, fma(ly, v, lx * u)))
 *     whichever estimator is chosen (the stray factor 2 of the reference estimator is not part of a probe). A degenerate normal
 *     gives whatever the equivalent ray gives: there is no special case.
 *   RTW_PROBE_IRRADIANCE: the sample's value is the radiance of the rtw_radiance sample of ray (p, d, tmin, tmax) at key k, sample
 *     index S and the same seed, generator, estimator and max_depth: the path after the first direction, its draws, media, light
 *     sampling, removeNaNs and roulette are unchanged. rgb = (sum / (float)spp) * 3.14159265f, alpha 1.0f, the sum taken in the
 *     order of RTW_SUM_BLOCK / RTW_SUM_UNIT_BLOCKS counted from sample_offset. The density is cos / pi, so this is the irradiance.
 *     max_depth = 0 gives zeros. stats: samples = n*spp, segments and shadow_rays as the kernel counts them, algorithmic_bytes and
 *     seconds as rtw_radiance reports them.
 *   RTW_PROBE_OCCLUSION: sample s is unoccluded when RTW_CAST_ANY finds nothing for ray (p, d, tmin, tmax) with NULL ray and gather
 *     times (volumes are skipped, as in rtw_cast). rgb = (float)unoccluded / (float)spp in all three channels, alpha 1.0f: an
 *     integer count, so no summation order is involved; counts are combined with integer arithmetic only. max_depth and estimator
 *     are validated but unused. stats: samples = shadow_rays = n*spp, segments = 0, seconds as above.
 *   The result for probe i depends on its probe, its key and the params alone: not on n, the launch geometry, how the batch is cut
 *     into chunks or ranges, or tuning knobs.
 *   rtw_probe: host pointers, staged as rtw_radiance stages its rays (the same slab, in chunks of at most RTW_RADIANCE_CHUNK probes;
 *     chunk c runs with the key of its first probe).
 *   rtw_probe_device: device pointers on the context's device, both 16-byte aligned. Ordered on hip_stream exactly as
 *     rtw_radiance_device is; returns when the results are written. NULL selects the context's own non-blocking stream, NOT the
 *     legacy default stream. Calls beyond 128 spp keep their unit sums (or unit counts) in rtw_radiance's scratch slab, capped by
 *     RTW_RADIANCE_SLAB_BYTES in the same way: a larger batch runs as consecutive probe ranges.
 *   Groups (n_devices > 1): the query runs on device_ids[0]; the bits are a single-device context's.
 *   An accumulation session on the context is not disturbed.
 *   Errors: rtw_radiance's list (RTW_ERR_NO_SCENE without a scene; RTW_ERR_INVALID_ARG for NULL params, spp <= 0, max_depth < 0, a
 *     bad rng_kind or estimator, sample_offset < 0 or sample_offset + spp > INT32_MAX, n > 2^31 - 1, with n > 0 a NULL probes or
 *     output, and (rtw_probe_device) a misaligned probes or output) and a mode other than the two. A refused call writes nothing and
 *     leaves *stats alone. n = 0 is RTW_OK and launches nothing. The context stays usable after an error. */
enum { RTW_PROBE_IRRADIANCE = 0, RTW_PROBE_OCCLUSION = 1 };
typedef struct rtw_probe_params {
    int32_t spp;            /* samples per probe, > 0                                        */
    int32_t max_depth;      /* as rtw_radiance_params.max_depth (irradiance only)            */
    uint32_t seed;
    int32_t rng_kind;       /* rtw_rng_kind                                                  */
    int32_t sample_offset;  /* first sample index; sample_offset + spp <= INT32_MAX          */
    int32_t estimator;      /* rtw_estimator (irradiance only)                               */
    uint32_t key_offset;    /* probe i draws from the stream of key_offset + i (mod 2^32)    */
    int32_t mode;           /* RTW_PROBE_IRRADIANCE or RTW_PROBE_OCCLUSION                   */
} rtw_probe_params;         /* 32 B */

int rtw_probe(rtw_ctx* ctx, const float* probes, size_t n, const rtw_probe_params* params, float* rgba_out, rtw_stats* stats);
int rtw_probe_device(rtw_ctx* ctx, const float* probes, size_t n, const rtw_probe_params* params, void* d_rgba, void* hip_stream,
                     rtw_stats* stats);

/* Probes sampled to a noise target: rtw_probe with rtw_render_adaptive's stop rule. Every probe takes samples until its own error
 * estimate falls below a threshold, or up to a cap - a lightmap whose open texels stop after a few dozen samples while its penumbrae
 * go on to the cap.
 *   Inputs: the probes, the keys (key_offset + i mod 2^32), the sample indices (sample_offset + s) and the directions are rtw_probe's;
 *     both modes are supported. params->spp is the cap. `ad` is rtw_render_adaptive's rtw_adaptive; dilate must be 0 (a probe batch
 *     has no neighbourhood).
 *   Checkpoints: rtw_render_adaptive's sequence, a function of (min_spp, step_spp, params->spp) alone.
 *   Result: probe i takes samples [sample_offset, sample_offset + n_i), n_i a checkpoint; a probe that stopped never resumes.
 *     rgba_out[i] is, bit for bit, rtw_probe's result for that probe with spp = n_i and everything else equal - irradiance:
 *     (sum / (float)n_i) * 3.14159265f, alpha 1.0f, the sum in the order of RTW_SUM_BLOCK / RTW_SUM_UNIT_BLOCKS counted from
 *     sample_offset; occlusion: (float)unoccluded / (float)n_i, alpha 1.0f. spp_out[i] = n_i. spp_out (n int32) and error_out
 *     (n float) may be NULL; rgba_out (n float4) is required.
 *   Error estimate: rtw_render_adaptive's statistic, formula and fp64 order. Irradiance: over the probe's radiance block sums S_b
 *     (the sums before the division and the factor pi). Occlusion: y_b = (float)c_b * 0.0625f, c_b the unoccluded count of block b;
 *     the rest of the formula is the same. error_out[i] is err at the probe's last checkpoint.
 *   Stop rule: at checkpoint n_k an active probe stops if n_k is the cap, or if its own err < threshold (strict; a NaN err compares
 *     false: that probe goes on).
 *   Independence: the three outputs of probe i depend on its probe, its key and the params alone: not on n, the launch geometry,
 *     chunks, slab ranges or tuning knobs.
 *   rtw_probe_adaptive: host pointers, staged through rtw_radiance's slab in chunks of at most RTW_RADIANCE_CHUNK probes; chunk c
 *     runs with the key of its first probe.
 *   rtw_probe_adaptive_device: device pointers on the context's device; probes and rgba 16-byte aligned, spp and error 4-byte
 *     aligned. Ordered on hip_stream exactly as rtw_probe_device is (NULL selects the context's own non-blocking stream, NOT the
 *     legacy default stream); returns when the results are written. The per-probe state and the lists live in buffers the context
 *     owns, grows and keeps: nothing is allocated per call once they are large enough. The block sums of a pass live in
 *     rtw_radiance's scratch slab, capped by RTW_RADIANCE_SLAB_BYTES: a larger pass runs as consecutive ranges of the active list.
 *     One 4-byte count is read back per checkpoint on the stream.
 *   stats (may be NULL): samples = sum of n_i. Irradiance: segments and shadow_rays of those samples' paths; occlusion:
 *     shadow_rays = samples, segments = 0. algorithmic_bytes and seconds as rtw_probe reports them; the per-kernel arrays are 0.
 *   Groups (n_devices > 1): the query runs on device_ids[0]. An accumulation session on the context is not disturbed.
 *   Errors: rtw_probe's refusals; also RTW_ERR_INVALID_ARG for a NULL ad, rtw_render_adaptive's refusals for the cap, min_spp,
 *     step_spp and threshold, dilate != 0, a NULL rgba_out with n > 0, and (rtw_probe_adaptive_device) a misaligned pointer. A
 *     refused call writes nothing and leaves *stats alone. n = 0 is RTW_OK and launches nothing. The context stays usable after an
 *     error. */
int rtw_probe_adaptive(rtw_ctx* ctx, const float* probes, size_t n, const rtw_probe_params* params, const rtw_adaptive* ad,
                       float* rgba_out, int32_t* spp_out, float* error_out, rtw_stats* stats);
int rtw_probe_adaptive_device(rtw_ctx* ctx, const float* d_probes, size_t n, const rtw_probe_params* params, const rtw_adaptive* ad,
                              void* d_rgba, void* d_spp, void* d_error, void* hip_stream, rtw_stats* stats);

/* Spherical-harmonic light probes at free points: the radiance arriving at a point from every direction, projected onto the nine
 * real spherical harmonics of bands 0 to 2 (an irradiance volume's probe; what lights things that move through a baked scene).
 * rtw_probe needs a normal and returns one number per channel; this needs none and returns nine coefficients per channel, which
 * the caller evaluates for any normal at run time.
 *   Points: `points` holds n*8 floats (px, py, pz, -, -, -, tmin, tmax): rtw_cast's layout, so a probe tensor is a valid point
 *     tensor. Floats 3..5 are loaded and never used: a NaN there changes nothing. tmin and tmax bound the first segment only.
 *   Direction: sample s of point i uses the key k = key_offset + i (mod 2^32), the sample index S = sample_offset + s and rtw_probe's
 *     two raygen uniforms r1, r2 of that path. The direction is uniform over the whole sphere, in world axes, in fp32 without
 *     contraction:
 *       z = 1.0f - 2.0f * r2 (exact); s2 = fma(-z, z, 1.0f); sq = sqrt(s2); sincos2pi(r1, sn, cs); d = (cs * sq, sn * sq, z),
 *     not normalised.
 *   Basis: with (x, y, z) = d, one rounding per operation, parenthesised as written:
 *       Y0 = 0.282094792f
 *       Y1 = 0.488602512f * y        Y2 = 0.488602512f * z        Y3 = 0.488602512f * x
 *       Y4 = 1.092548431f * (x * y)  Y5 = 1.092548431f * (y * z)
 *       Y6 = 0.315391565f * (3.0f * (z * z) - 1.0f)
 *       Y7 = 1.092548431f * (x * z)  Y8 = 0.546274215f * ((x * x) - (y * y))
 *   Sample value: L is the radiance of the rtw_radiance sample of ray (p, d, tmin, tmax) at key k, sample index S and the same
 *     seed, generator, estimator and max_depth, after removeNaNs; the sample adds Y_j * L_c to coefficient j, channel c.
 *   Output: sh_out[i * 9 + j] is a float4: rgb = (sum / (float)spp) * 12.5663706f (the float nearest 4 pi; the density is
 *     1 / (4 pi)), each of the 27 sums taken on its own in the order of RTW_SUM_BLOCK / RTW_SUM_UNIT_BLOCKS counted from
 *     sample_offset; w = 0.0f. max_depth = 0 gives zeros. The result for point i depends on its point, its key and the params
 *     alone: not on n, the launch geometry, how the batch is cut into chunks or ranges, or tuning knobs.
 *   Everything else is rtw_radiance's: the same params and validation (reserved == 0) and the same refusals, which write nothing
 *     and leave *stats alone; n = 0 is RTW_OK; rtw_probe_sh takes host pointers and stages in chunks of RTW_RADIANCE_CHUNK points,
 *     rtw_probe_sh_device takes 16-byte aligned device pointers (d_sh: n * 9 float4) and the same stream rule (NULL selects the
 *     context's own non-blocking stream). Calls beyond 128 spp keep nine 16-byte sums per point and unit in rtw_radiance's scratch
 *     slab (n * ceil(spp / 128) * 144 B, capped by RTW_RADIANCE_SLAB_BYTES: a larger batch runs as consecutive point ranges).
 *     Groups answer on device_ids[0]; an accumulation session is not disturbed. stats: samples = n*spp, segments and shadow_rays
 *     those of the same paths, algorithmic_bytes and seconds as rtw_radiance reports them. */
int rtw_probe_sh(rtw_ctx* ctx, const float* points, size_t n, const rtw_radiance_params* params, float* sh_out, rtw_stats* stats);
int rtw_probe_sh_device(rtw_ctx* ctx, const float* points, size_t n, const rtw_radiance_params* params, void* d_sh, void* hip_stream,
                        rtw_stats* stats);

/* Views: batched frames from the caller's own cameras (turntables, stereo pairs, the six faces of a cube map at many positions, a
 * few thousand small training views), in one call, from the uploaded scene. The scene blob carries one camera and only
 * rtw_upload_scene changes it; rtw_radiance takes fixed rays, so no jitter inside the pixel and no lens sample. Here the camera
 * ray is generated on the device, from a record per view.
 *   Views: `views` holds n_views records. camera is rtw_scene_header.camera, time0 / time1 included; camera_type its
 *     rtw_camera_type; seed that view's rtw_params.seed; reserved is 0. All views of a call share width, height and the sampling.
 *   Equivalence: frame v is, bit for bit, the frame rtw_render makes of the uploaded scene with the header's camera and camera_type
 *     replaced by views[v]'s, under rtw_params {width, height, spp, max_depth, seed = views[v].seed, all rows, rng_kind,
 *     sample_offset, estimator}. The stream key of pixel (x, y) is width * y + x; the pixel jitter, the lens sample (drawn by the
 *     TEA+LCG stream for a perspective camera only), the environment and orthographic formulas, the gather-time draw over the view's
 *     own time0 / time1 and the first ray time are that render's, operation for operation; the first segment uses the estimator's
 *     start distance and 1e27f. Views that share a seed share their random streams, as frames rendered one after another with one
 *     seed do: the caller decorrelates views with `seed`.
 *   Output: n_views * height * width float4; pixel (x, y) of view v at (v * height + y) * width + x, row 0 the bottom row: the sum
 *     of the samples' radiance in the order of RTW_SUM_BLOCK / RTW_SUM_UNIT_BLOCKS counted from sample_offset, divided by
 *     (float)spp, alpha 1.0f. A pixel depends on its view record, its (x, y) and the params alone: not on n_views, its view's
 *     index, the launch geometry, how the call is cut into chunks or ranges, or tuning knobs.
 *   rtw_views: host pointers. The records are copied to a device buffer the context keeps and grows; the frames are staged out
 *     through rtw_radiance's staging slab in chunks of at most RTW_RADIANCE_CHUNK pixels of the flattened (view, y, x) index (a chunk
 *     may begin and end mid-row and mid-view). It reads the records: a camera_type outside 0..2 or a non-zero view `reserved` is
 *     RTW_ERR_INVALID_ARG.
 *   rtw_views_device: device pointers on the context's device, both 16-byte aligned. Ordered on hip_stream exactly as
 *     rtw_radiance_device is; returns when the frames are written. NULL selects the context's own non-blocking stream, NOT the
 *     legacy default stream. It does not read the records back: on the device a camera_type that is neither RTW_CAM_ENVIRONMENT nor
 *     RTW_CAM_ORTHOGRAPHIC is a perspective camera (lens draws included), and `reserved` is ignored. Calls beyond 128 spp keep one
 *     16-byte sum per pixel and unit in rtw_radiance's scratch slab, capped by RTW_RADIANCE_SLAB_BYTES: a larger call runs as
 *     consecutive ranges of flattened pixels. It allocates nothing per call once the context's scratch is large enough.
 *   Groups (n_devices > 1): the call runs on device_ids[0]; the bits are a single-device context's.
 *   An accumulation session on the context is not disturbed.
 *   stats (may be NULL): samples = n_views*width*height*spp; segments and shadow_rays = the sums of those renders' counts (a render
 *     counts the one-segment samples of the pixels it culls; this call traces them); algorithmic_bytes and seconds as rtw_radiance
 *     reports them; the per-kernel arrays are 0.
 *   Errors: RTW_ERR_NO_SCENE without a scene; RTW_ERR_INVALID_ARG for NULL params, width, height or spp <= 0, max_depth < 0, a bad
 *     rng_kind or estimator, sample_offset < 0 or sample_offset + spp > INT32_MAX, params reserved != 0,
 *     n_views * width * height > 2^31 - 1, with n_views > 0 a NULL views or output, (rtw_views_device) a misaligned views or output,
 *     and (rtw_views) a bad record as above. A refused call writes nothing and leaves *stats alone. n_views = 0 is RTW_OK and
 *     launches nothing. The context stays usable after an error. */
typedef struct rtw_view {
    rtw_camera camera;     /* as rtw_scene_header.camera, time0 / time1 included */
    int32_t camera_type;   /* rtw_camera_type */
    uint32_t seed;         /* this view's rtw_params.seed */
    uint32_t reserved[2];  /* 0 */
} rtw_view;                /* 112 B */

typedef struct rtw_view_params {
    int32_t width, height;  /* of every view of the call */
    int32_t spp;            /* samples per pixel, > 0 */
    int32_t max_depth;      /* as rtw_params.max_depth */
    int32_t rng_kind;       /* rtw_rng_kind */
    int32_t sample_offset;  /* first sample index; sample_offset + spp <= INT32_MAX */
    int32_t estimator;      /* rtw_estimator */
    uint32_t reserved;      /* 0, else RTW_ERR_INVALID_ARG */
} rtw_view_params;          /* 32 B */

int rtw_views(rtw_ctx* ctx, const rtw_view* views, size_t n_views, const rtw_view_params* params, float* rgba_out, rtw_stats* stats);
int rtw_views_device(rtw_ctx* ctx, const rtw_view* d_views, size_t n_views, const rtw_view_params* params, void* d_rgba, void* hip_stream,
                     rtw_stats* stats);

/* Views sampled to a noise target: rtw_views with rtw_render_adaptive's stop rule. Every pixel of every view takes samples until its
 * error estimate falls below a threshold, or up to a cap - cube-map faces, turntables and training views whose open pixels stop
 * after a few dozen samples while penumbrae and glass go on to the cap - without one rtw_upload_scene + rtw_render_adaptive per camera.
 *   Inputs: the views and the params are rtw_views' own; params->spp is the cap. `ad` is rtw_render_adaptive's rtw_adaptive; dilate
 *     may be 0 or 1. The checkpoints are rtw_render_adaptive's sequence, a function of (min_spp, step_spp, params->spp) alone.
 *   Equivalence: the three outputs of view v are, bit for bit, the rgba_out, spp_out and error_out that rtw_render_adaptive writes
 *     for the uploaded scene with the header's camera and camera_type replaced by views[v]'s, under rtw_params {width, height,
 *     spp = cap, max_depth, seed = views[v].seed, all rows, rng_kind, sample_offset, estimator} and the same rtw_adaptive. So pixel
 *     (x, y) of view v stops at a checkpoint n; its colour is rtw_views' colour of that pixel with spp = n; its err is the
 *     batch-means statistic over its own RTW_SUM_BLOCK-sample block sums (rtw_render_adaptive's formula, fp64 in block order).
 *   Dilation: with dilate = 1 the 3x3 neighbourhood is clamped to the pixel's own view: a tap never reads another view. An active
 *     neighbour is one that is active at this checkpoint, as in rtw_render_adaptive.
 *   Layout: rgba_out holds n_views * height * width float4 in rtw_views' layout (pixel (x, y) of view v at
 *     (v * height + y) * width + x); spp_out (int32) and error_out (float) use the same layout and may be NULL; rgba_out is required.
 *   Independence: a pixel's three outputs depend on its view record, its (x, y), the params and `ad` alone: not on n_views, its
 *     view's index, how the call is cut into batches or slab ranges, the launch geometry or tuning knobs.
 *   rtw_views_adaptive: host pointers. The records go to the device buffer rtw_views keeps. Because of the dilation the call is cut
 *     into batches of whole views, max(1, RTW_RADIANCE_CHUNK / (width * height)) views each, whose three results are staged out
 *     through rtw_radiance's staging slab. It reads the records: a camera_type outside 0..2 or a non-zero view `reserved` is
 *     RTW_ERR_INVALID_ARG.
 *   rtw_views_adaptive_device: device pointers on the context's device; views and rgba 16-byte aligned, spp and error 4-byte
 *     aligned. Ordered on hip_stream exactly as rtw_views_device is (NULL selects the context's own non-blocking stream, NOT the
 *     legacy default stream); returns when the results are written. It does not read the records back (rtw_views_device's rule for
 *     camera_type and `reserved`). The per-pixel state and the lists live in the buffer rtw_probe_adaptive keeps, which the context
 *     owns, grows and keeps: nothing is allocated per call once it is large enough. The block sums of a pass live in rtw_radiance's
 *     scratch slab, capped by RTW_RADIANCE_SLAB_BYTES: a larger pass runs as consecutive ranges of the active list. One 4-byte
 *     count is read back per checkpoint on the stream.
 *   stats (may be NULL): samples = sum of n_p; segments and shadow_rays those of the sampled paths: summed over the views they
 *     equal the per-view rtw_render_adaptive counts, the pixels a render culls included. algorithmic_bytes and seconds as rtw_views
 *     reports them; the per-kernel arrays are 0.
 *   Groups (n_devices > 1): the call runs on device_ids[0]. An accumulation session on the context is not disturbed.
 *   Errors: rtw_views' refusals; rtw_render_adaptive's refusals for the cap, min_spp, step_spp, threshold and a dilate that is not
 *     0 or 1; RTW_ERR_INVALID_ARG for a NULL ad, a NULL rgba_out with n_views > 0, and (rtw_views_adaptive_device) a misaligned
 *     pointer. A refused call writes nothing and leaves *stats alone. n_views = 0 is RTW_OK and launches nothing. The context stays
 *     usable after an error. */
int rtw_views_adaptive(rtw_ctx* ctx, const rtw_view* views, size_t n_views, const rtw_view_params* params, const rtw_adaptive* ad,
                       float* rgba_out, int32_t* spp_out, float* error_out, rtw_stats* stats);
int rtw_views_adaptive_device(rtw_ctx* ctx, const rtw_view* d_views, size_t n_views, const rtw_view_params* params, const rtw_adaptive* ad,
                              void* d_rgba, void* d_spp, void* d_error, void* hip_stream, rtw_stats* stats);

/* Guides of batched views: rtw_render_guides' buffers for every view of an rtw_views call, in one call, from the uploaded scene.
 * rtw_render_guides reads the one camera of the scene blob; here the camera ray comes from the view's record, on the device.
 *   Views and params: rtw_views' records and rtw_view_params. max_depth and estimator are validated as rtw_views validates them and
 *     unused: a guide ray is one camera segment, and it starts at the scene's own 1e-6 whatever the estimator.
 *   Equivalence: the guides of view v are, bit for bit, what rtw_render_guides writes for the uploaded scene with the header's
 *     camera and camera_type replaced by views[v]'s, under rtw_params {width, height, spp, seed = views[v].seed, all rows, rng_kind,
 *     sample_offset}: the camera rays (pixel jitter, lens draws, all three camera kinds), the gather time over the view's own time0 /
 *     time1 and the first ray time, participating media skipped, the albedo rules per material, alpha = the fraction of the samples
 *     that hit, the summation order of RTW_SUM_BLOCK / RTW_SUM_UNIT_BLOCKS, depth and prim from sample sample_offset alone.
 *   Output: rtw_guides as it is. Every non-NULL pointer holds n_views * height * width entries in rtw_views' layout: pixel (x, y) of
 *     view v at (v * height + y) * width + x, row 0 the bottom row; a NULL pointer is a buffer the caller does not want and does not
 *     change the others. A pixel depends on its view record, its (x, y) and the params alone: not on n_views, its view's index, how
 *     the call is cut into chunks, the launch geometry or tuning knobs.
 *   rtw_views_guides: host pointers. The records go to the device buffer rtw_views keeps; only the requested buffers are staged out,
 *     through rtw_radiance's staging slab, in chunks of at most RTW_RADIANCE_CHUNK pixels of the flattened (view, y, x) index (a chunk
 *     may begin and end mid-row and mid-view). It reads the records: a camera_type outside 0..2 or a non-zero view `reserved` is
 *     RTW_ERR_INVALID_ARG.
 *   rtw_views_guides_device: d_views and the pointers inside *d_out (the struct itself is host memory) are device pointers on the
 *     context's device: d_views, albedo and normal 16-byte aligned, depth and prim 4-byte aligned. Ordered on hip_stream exactly as
 *     rtw_views_device is; returns when the buffers are written. NULL selects the context's own non-blocking stream, NOT the legacy
 *     default stream. It does not read the records back: a camera_type that is neither RTW_CAM_ENVIRONMENT nor RTW_CAM_ORTHOGRAPHIC
 *     is a perspective camera, and `reserved` is ignored. It allocates nothing per call.
 *   Groups (n_devices > 1): the call runs on device_ids[0]; the bits are a single-device context's.
 *   An accumulation session on the context is not disturbed.
 *   stats (may be NULL): samples = segments = n_views*width*height*spp (one camera segment per sample); seconds = the device time
 *     from the call's first event to its last; everything else is 0.
 *   Errors: rtw_views' (RTW_ERR_NO_SCENE without a scene; RTW_ERR_INVALID_ARG for NULL params, width, height or spp <= 0,
 *     max_depth < 0, a bad rng_kind or estimator, sample_offset < 0 or sample_offset + spp > INT32_MAX, params reserved != 0,
 *     n_views * width * height > 2^31 - 1, with n_views > 0 NULL views, (rtw_views_guides) a bad record as above), and: `out` NULL or
 *     all four of its pointers NULL, (rtw_views_guides_device) a misaligned d_views or buffer. A refused call writes nothing and
 *     leaves *stats alone. n_views = 0 is RTW_OK and launches nothing. The context stays usable after an error. */
int rtw_views_guides(rtw_ctx* ctx, const rtw_view* views, size_t n_views, const rtw_view_params* params, const rtw_guides* out, rtw_stats* stats);
int rtw_views_guides_device(rtw_ctx* ctx, const rtw_view* d_views, size_t n_views, const rtw_view_params* params, const rtw_guides* d_out,
                            void* hip_stream, rtw_stats* stats);

/* rtw_denoise_guided over batched views: n_views frames of width x height, each filtered on its own, in one call.
 *   Layout: rgba_in, albedo, normal, rgba_out hold n_views * height * width float4 in rtw_views' layout (albedo and normal as
 *     rtw_views_guides writes them).
 *   Equivalence: frame v of rgba_out is, bit for bit, rtw_denoise_guided of frame v alone: the 25 taps and their order, the border
 *     clamp per frame (a tap never reads another view), the B3 kernel, the three divisors, the colour sigma halving per pass, alpha
 *     copied.
 *   rtw_denoise_views: host pointers. rtw_denoise_views_device: device pointers on the context's device, 16-byte aligned; ordered on
 *     hip_stream as rtw_views_device is (NULL: the context's own non-blocking stream); returns when the frames are written.
 *   Scratch: the passes alternate between rgba_out and one buffer of the context's (the host entry keeps its device copies beside
 *     it); the buffer grows on demand and is kept: nothing is allocated per call once it is large enough.
 *   Groups (n_devices > 1): the call runs on device_ids[0]. Needs no scene. An accumulation session is not disturbed.
 *   Errors: RTW_ERR_INVALID_ARG for width or height <= 0, iterations outside 1..8, a sigma that is not > 0 (or whose inverse square
 *     is not finite), width * height > 2^28 (rtw_denoise_guided's limit), n_views * width * height > 2^31 - 1, with n_views > 0 a NULL buffer or an rgba_out that is or overlaps an
 *     input, (rtw_denoise_views_device) a misaligned buffer. A refused call writes nothing. n_views = 0 is RTW_OK. */
int rtw_denoise_views(rtw_ctx* ctx, const float* rgba_in, const float* albedo, const float* normal, float* rgba_out, size_t n_views,
                      int32_t width, int32_t height, int32_t iterations, float sigma, float sigma_albedo, float sigma_normal);
int rtw_denoise_views_device(rtw_ctx* ctx, const float* rgba_in, const float* albedo, const float* normal, float* rgba_out, size_t n_views,
                             int32_t width, int32_t height, int32_t iterations, float sigma, float sigma_albedo, float sigma_normal,
                             void* hip_stream);

/* Path records: replay samples and return every vertex of their paths (which of a pixel's 4096 samples is the firefly and what it
 * bounced off; direct against indirect light, per-bounce layers, per-light contributions and path-length histograms as folds over the
 * vertices; (position, direction, throughput, contribution) tuples for path guiding, left on the device). Every other entry point
 * reduces a path to three floats and the samples to a mean; these return the samples themselves, one head per sample and one vertex
 * per traced segment.
 *   Same path as rtw_radiance: sample s of ray i is the rtw_radiance sample of that ray (rtw_cast's eight floats; tmin and tmax bound
 *     the first segment only) at stream key key_offset + i (mod 2^32) and sample index sample_offset + s: the same draws, media,
 *     light sampling, shadow probe, roulette and depth limit, operation for operation. rtw_paths_views replays rtw_views' samples
 *     in the same way: pixels [first, first + count) of rtw_views' flattened index (view * height + y) * width + x, the camera ray
 *     generated on the device from the pixel's view record, the stream key width * y + x, the seed the view's own. To replay sample
 *     s of pixel (x, y) of view v: first = (v * height + y) * width + x, count = 1, sample_offset = s, spp = 1.
 *   Head: radiance carries the bits rtw_radiance (rtw_views) returns in rgb for spp = 1 at that sample index - the sample after
 *     removeNaNs, added to +0 as that call's sums add it, so a -0 comes back as +0. Hence the sum of a ray's head radiances in the
 *     order of RTW_SUM_BLOCK / RTW_SUM_UNIT_BLOCKS counted from sample_offset, divided by (float)spp, is rtw_radiance's result for
 *     that spp. segments counts the segments traced (it may exceed max_records), shadow_rays the light-sample probes traced,
 *     gather_time is the sample's gather time, key and sample its stream key and its absolute sample index.
 *   Vertices: vertex j is segment j of the path. o and d are the segment's origin and direction as traced (d is not normalised;
 *     record 0 of rtw_paths carries the caller's o and d), t the hit parameter (the segment's tmax on a miss: the caller's tmax for
 *     segment 0 of rtw_paths, else 1e27f), prim the primitive hit, volume primitives included, -1 on a miss. throughput is the
 *     path's throughput T that weighted this segment ((1, 1, 1) at the first), contribution the term the segment added to the
 *     sample: (emitted or sky radiance + the light sample where its probe came back unoccluded) * T. ray_time is the segment's ray
 *     time. flags = the segment's event (RTW_PATH_MISS: nothing hit, the path ends; RTW_PATH_SCATTER: the material scattered, the
 *     path goes on unless the roulette or the depth limit ends it; RTW_PATH_END: an emitter or an absorbing event, the path ends;
 *     RTW_PATH_CANCEL: the material cancelled the path) | RTW_PATH_LIGHT_SAMPLED where a light-sample probe was traced from this
 *     segment's hit | RTW_PATH_LIGHT_ADDED where that probe came back unoccluded. Whenever segments <= max_records: adding the
 *     contributions in float32 in order from +0 and replacing NaN channels by 0 gives head.radiance bit for bit, and the number of
 *     RTW_PATH_LIGHT_SAMPLED records is head.shadow_rays.
 *   Layout: heads_out[i * spp + s]; vertices_out[(i * spp + s) * max_records + j] for j < min(segments, max_records). Entries
 *     beyond that are not written. i counts rays, or pixels from `first`.
 *   max_depth = 0 gives segments = 0, radiance 0 and no records. max_records = 0 returns the heads alone - the cheap way to find
 *     an outlier among thousands of samples - and vertices_out must then be NULL.
 *   Independence: a head and its records depend on the ray (or the pixel and its view record), the key and the params alone: not on
 *     n, count, how the call is cut into chunks, the launch geometry or tuning knobs.
 *   rtw_paths / rtw_paths_views: host pointers. Rays, heads and records are staged through rtw_radiance's staging slab in chunks of
 *     whole rays (pixels): as many as keep a chunk's heads and records within RTW_PATHS_CHUNK_BYTES (an environment variable read
 *     per call, csrc/rtw_plan.h), at least one; chunk c runs with the key of its first ray, or from its first pixel. A chunk's
 *     records come back whole, so the caller's bytes go up first: vertices_out is read, and an entry that is not written keeps
 *     what it held. rtw_paths_views reads and checks its records as rtw_views does.
 *   rtw_paths_device / rtw_paths_views_device: device pointers on the context's device, all 16-byte aligned. Ordered on hip_stream
 *     exactly as rtw_radiance_device is; returns when the results are written. NULL selects the context's own non-blocking stream,
 *     NOT the legacy default stream. One persistent launch: a lane owns one (ray, sample) pair at a time. It allocates nothing per
 *     call. rtw_paths_views_device does not read the records back (rtw_views_device's rule for camera_type and `reserved`).
 *   Groups (n_devices > 1): the call runs on device_ids[0]; the bits are a single-device context's.
 *   An accumulation session on the context is not disturbed.
 *   stats (may be NULL): samples = n * spp (count * spp), segments = the sum of head.segments, shadow_rays = the sum of
 *     head.shadow_rays, algorithmic_bytes and seconds as rtw_radiance reports them; the per-kernel arrays are 0.
 *   Errors: rtw_radiance's list (rtw_paths_views: rtw_views' list, for the params built from view_params and the whole of
 *     n_views * width * height) and RTW_ERR_INVALID_ARG for max_records < 0 or > max_depth, a non-zero reserved word,
 *     n * spp > 2^31 - 1 (count * spp), with n > 0 a NULL heads_out, a NULL vertices_out with max_records > 0 or a non-NULL one
 *     with max_records = 0, first + count beyond the call's pixels, and (the device variants) a misaligned pointer. A refused call
 *     writes nothing and leaves *stats alone. n = 0 (count = 0) is RTW_OK and launches nothing. The context stays usable after an
 *     error. */
enum { RTW_PATH_MISS = 0, RTW_PATH_SCATTER = 1, RTW_PATH_END = 2, RTW_PATH_CANCEL = 3 };
enum { RTW_PATH_EVENT_MASK = 3, RTW_PATH_LIGHT_SAMPLED = 4, RTW_PATH_LIGHT_ADDED = 8 };

typedef struct rtw_path_vertex {
    float o[3];            /* the segment's origin                                                   */
    float t;               /* the hit parameter; the segment's tmax on a miss                        */
    float d[3];            /* its direction as traced (not normalised)                               */
    int32_t prim;          /* the primitive hit (volumes included), -1: miss                         */
    float contribution[3]; /* radiance * T: what the segment added to the sample                     */
    uint32_t flags;        /* event | RTW_PATH_LIGHT_*                                               */
    float throughput[3];   /* T that weighted this segment, (1, 1, 1) at the first                   */
    float ray_time;        /* the segment's ray time                                                 */
} rtw_path_vertex;         /* 64 B */

typedef struct rtw_path_head {
    float radiance[3];     /* the sample after removeNaNs: what joins the block sum                  */
    int32_t segments;      /* segments traced (may exceed max_records)                               */
    float gather_time;
    int32_t shadow_rays;   /* light-sample probes traced                                             */
    uint32_t key, sample;  /* the stream key and the absolute sample index                           */
} rtw_path_head;           /* 32 B */

typedef struct rtw_paths_params {
    int32_t spp;            /* samples per ray (pixel), > 0                                  */
    int32_t max_depth;      /* as rtw_radiance_params.max_depth                              */
    uint32_t seed;          /* (rtw_paths_views: unused, the seed is the view's)             */
    int32_t rng_kind;       /* rtw_rng_kind                                                  */
    int32_t sample_offset;  /* first sample index; sample_offset + spp <= INT32_MAX          */
    int32_t estimator;      /* rtw_estimator                                                 */
    uint32_t key_offset;    /* ray i draws from the stream of key_offset + i (mod 2^32)      */
    int32_t max_records;    /* vertices kept per sample, 0 .. max_depth (0: heads only)      */
    uint32_t reserved[2];   /* 0, else RTW_ERR_INVALID_ARG                                   */
} rtw_paths_params;         /* 40 B */

int rtw_paths(rtw_ctx* ctx, const float* rays, size_t n, const rtw_paths_params* params, rtw_path_head* heads_out,
              rtw_path_vertex* vertices_out, rtw_stats* stats);
int rtw_paths_device(rtw_ctx* ctx, const float* rays, size_t n, const rtw_paths_params* params, void* d_heads, void* d_vertices,
                     void* hip_stream, rtw_stats* stats);
int rtw_paths_views(rtw_ctx* ctx, const rtw_view* views, size_t n_views, const rtw_view_params* view_params, uint64_t first, uint64_t count,
                    int32_t max_records, rtw_path_head* heads_out, rtw_path_vertex* vertices_out, rtw_stats* stats);
int rtw_paths_views_device(rtw_ctx* ctx, const rtw_view* d_views, size_t n_views, const rtw_view_params* view_params, uint64_t first,
                           uint64_t count, int32_t max_records, void* d_heads, void* d_vertices, void* hip_stream, rtw_stats* stats);

/* Test hooks (no reference counterpart): one closest-hit query per ray on the GPU accel structure,
 * used by the parity tests to compare BVH traversal with the oracle's brute force.
 * rays: n*8 floats (ox,oy,oz,dx,dy,dz,tmin,tmax); ray_time: n floats or NULL;
 * out_t: n floats (tmax if miss); out_prim: n int32 (-1 if miss). All host pointers. */
int rtw_debug_intersect(rtw_ctx* ctx, const float* rays, const float* ray_time, const float* gather_time,
                        int n, float* out_t, int32_t* out_prim);

/* Test hook: the proof that the short reciprocal / root forms of csrc/rtw_math.h equal the compiler's correctly rounded forms
 * on this device. Runs all 2^32 bit patterns x through both. op: 0 = 1.0f / x, 1 = sqrtf(x), 2 = 1.0f / sqrtf(x) as the renderer
 * takes them; for the record, whatever the header's switches say: 3 / 4 = 1.0f / x with one / two refinement steps, 5 / 6 = sqrtf(x)
 * without / with the coupled step.
 * out[0] = patterns inside the form's range window whose results differ (NaN equals NaN), out[1] = patterns inside the window,
 * out[2] = the lowest differing pattern, or 2^64 - 1 when there is none. Needs no scene. */
int rtw_debug_math(rtw_ctx* ctx, int op, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* RTW_H */
