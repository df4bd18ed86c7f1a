// rtw_hip.hip — Monte-Carlo path tracer for MI355X (gfx950) behind the C ABI of include/rtw.h.
//
// What the reference does in ONE OptiX megakernel launch (Director.cpp:982-984: raygen -> traverse ->
// closest-hit/miss -> callables, one thread per pixel, one sample) is done here by one of two pipelines:
//
//   k_path (scenes walked with the candidate lists: <= 24 primitives)
//     one persistent launch per pass over the samples: whole paths in registers, a lane owns a (pixel, 64-sample block)
//     unit, regenerates camera rays as its paths end and stores one 16-byte sum per block; k_resolve_blocks adds the
//     block sums per pixel in order
//
//   wavefront kernels (tree scenes), batches of S samples per pixel, P = pixels*S paths in flight in HBM:
//     k_first                     primary rays, their closest hit and closest-hit program (light sample queued)
//     repeat for the wide bounces (1..19):
//       k_trace_bvh               radiance ray + queued shadow probe of every surviving path, surfaces only
//       k_shade                   (volume pass,) material scatter, light sample (probe queued), roulette, compaction
//     k_bounce x few              thin tail: several fused bounces per launch, in registers
//     two batches are in flight on two streams ("lanes"); the resolves stay ordered on the caller's stream
//     k_resolve                   sums the S sample slots of each pixel in the spec's blocked order (deterministic)
//
//   k_finish (once)               mean radiance -> float4 framebuffer tile
//   n_devices > 1: one host thread + context per device, interleaved row shards, peer-copy gather, k_interleave
//
//   accumulation sessions (rtw_accum_*): the same launches over a range of samples, resolved into a state the session owns
//     (rtw_accum.h) that keeps the summation unit open between adds; splitting and the saved form: rtw_accum_state.h
//
//   the query family (rtw_cast, rtw_radiance, rtw_probe, rtw_probe_sh, rtw_views, rtw_views_guides, rtw_denoise_views, rtw_probe_adaptive,
//     rtw_views_adaptive, rtw_paths, rtw_paths_views, each with a _device variant): the caller's rays, probes, points or cameras through kernels of their own
//     translation units. On the host they share one scaffold: QueryCall
//     (query_open / query_close: device context, stream, the two timing events, the control words), query_chunks for the host
//     variants' upload / issue / copy-back loop through one staging slab (laid out by rtw_stage_plan.h), query_stats for the tail,
//     and list_pass, a pass of the two adaptive queries
//
//   the adaptive family (rtw_render_adaptive, rtw_probe_adaptive, rtw_views_adaptive): one per-entry state (rtw_adaptive_plan.h) and one
//     checkpoint loop, adaptive_run, over the kernels of rtw_adaptive.h; a family hands in its pass and its results
//
// render_single picks the pipeline; render_path and render_wavefront issue what rtw_plan.h's plan_path / plan_wavefront decide
// (unit and batch sizes, passes, lanes, trace workgroup, launch schedule: host arithmetic on sizes, checked on the CPU), through the
// schedules they share with the adaptive renderer and the sessions (issue_path_pass, run_batches).
// rtw_upload_scene prepares the blob once on the host (rtw_scene.h prepare_scene: validation, hit records, candidate lists, tree, one
// staged image, likewise checked on the CPU) and copies the image to each device.
//
// Device memory has one owner type, DevBuf (rtw_devbuf.h: grow on demand, freed with its owner): every buffer of a context, grown where a call
// first needs it and kept until rtw_destroy, and every call's own scratch, freed on whichever path the call returns.
//
// No OptiX, no CUDA shims, no Triton, no MFMA (divergent scalar fp32). Results do not depend on
// scheduling: every path owns a counter-based RNG stream and every (pixel, block) its own sum.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <exception>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rtw.h"
#include "rtw_bvh.h"
#include "rtw_devbuf.h"
#include "rtw_scene.h"
#include "rtw_device.h"
#include "rtw_plan.h"
#include "rtw_accum_state.h"
#include "rtw_kernels.h"
#include "rtw_guides.h"
#include "rtw_cast.h"
#include "rtw_radiance.h"
#include "rtw_radiance_plan.h"
#include "rtw_stage_plan.h"
#include "rtw_probe.h"
#include "rtw_probe_sh.h"
#include "rtw_view.h"
#include "rtw_view_guides_plan.h"
#include "rtw_adaptive.h"
#include "rtw_probe_adaptive.h"
#include "rtw_probe_adaptive_plan.h"
#include "rtw_view_adaptive.h"
#include "rtw_view_adaptive_plan.h"
#include "rtw_paths.h"
#include "rtw_paths_plan.h"
#include "rtw_accum.h"
#include "rtw_variants.h"

using namespace rtwdev;
using namespace rtwk;

// The template kernels' rows (rtw_variants.h) are instantiated in translation units of their own (rtw_inst_*.hip) and only declared
// here; k_trace and k_trace_bvh are instantiated by this unit. Each list once more as the rows' addresses, indexed by the row (the
// null address behind the last row: what a selector that finds no row picks, a launch error)
namespace rtwk {
#define RTW_DECL(K_, name, ...) extern template __global__ void K_<__VA_ARGS__> RTW_SIG_##K_;
RTW_K_PATH_ROWS(RTW_DECL) RTW_K_FIRST_ROWS(RTW_DECL) RTW_K_SHADE_ROWS(RTW_DECL) RTW_K_BOUNCE_ROWS(RTW_DECL) RTW_K_CLASSIFY_ROWS(RTW_DECL)
#undef RTW_DECL
typedef void (*Kernel)(const KArgs);
typedef void (*ClassifyKernel)(const KArgs, uint32_t*, uint32_t*, uint32_t);
#define RTW_ADDR(K_, name, ...) K_<__VA_ARGS__>,
const Kernel kPathKernels[] = {RTW_K_PATH_ROWS(RTW_ADDR) nullptr}, kFirstKernels[] = {RTW_K_FIRST_ROWS(RTW_ADDR) nullptr},
             kShadeKernels[] = {RTW_K_SHADE_ROWS(RTW_ADDR) nullptr}, kBounceKernels[] = {RTW_K_BOUNCE_ROWS(RTW_ADDR) nullptr},
             kTraceKernels[] = {RTW_K_TRACE_ROWS(RTW_ADDR) nullptr}, kTraceBvhKernels[] = {RTW_K_TRACE_BVH_ROWS(RTW_ADDR) nullptr};
const ClassifyKernel kClassifyKernels[] = {RTW_K_CLASSIFY_ROWS(RTW_ADDR) nullptr};
#undef RTW_ADDR
}  // namespace rtwk

// =============================================================================================
// host side of the library
struct rtw_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // scene
    bool has_scene = false;
    DScene sc{};
    DevBuf d_scene;            // one allocation holding all scene tables
    SceneInfo info{};          // its host-side facts, overwritten as a whole by every upload (rtw_scene.h)
    // render pool
    // Two independent "lanes" (stream + path pool): consecutive batches alternate between them so that the
    // bandwidth-bound kernels of one batch overlap the compute- and latency-bound kernels of the other.
    struct Lane {
        hipStream_t st = nullptr;
        hipEvent_t ev_done = nullptr, ev_free = nullptr;
        PathBuf buf[2] = {};
        uint2* hit[2] = {nullptr, nullptr};
        DevBuf slab[2];        // one allocation per ping-pong set: six planes + hit records
        DevBuf lbuf;           // float4 per path
        DevBuf cnt;            // the region counters, in words
        size_t paths = 0;
        bool probes = false;   // the slabs hold the planes of scenes with listed lights (p2, a full p5) as well
    } lane[4];
    DevBuf accum;              // float4 per pixel: sum of the finished sample blocks
    DevBuf part;               // float4 per pixel: running sum of the current block (wavefront pipeline)
    DevBuf upart;              // float4 per pixel: running sum of the current summation unit's finished blocks (wavefront pipeline)
    DevBuf blocksum;           // k_path: [block][pixel] float4 unit sums of one pass
    DevBuf d_queue;            // k_path: 16 words, job counter [0], k_classify's two counters [1], [2]
    DevBuf d_order;            // k_path: job order of the pixel groups (k_classify's three lists), in groups of 64 pixels
    hipStream_t stream2 = nullptr;  // k_path: the stream of the fine-grained end-game launch
    std::vector<hipEvent_t> ev_pool;  // timing events, reused across launches and calls
    DevBuf d_stats;            // kStatRows + 1 rows of 8 counters
    DevBuf d_out;              // float4 per pixel: the frame of a call that returns it to the host
    int n_cu = 256;
    // n_devices > 1: this context is a group; kids[g] renders the g-th interleaved sub-shard on device_ids[g], the
    // shards are gathered on device_ids[0] (this->device) into `stage` and interleaved into the caller's frame
    std::vector<rtw_ctx*> kids;
    DevBuf stage;              // in pixels: the gathered shards, then the shards' row offsets
    size_t pool_cap = ~(size_t)0;  // paths in flight this device has room for (halved when a pool allocation fails: render_wavefront)
    struct Worker* worker = nullptr;  // a kid's host thread: created with the group, lives until rtw_destroy
    // rtw_render_adaptive's per-pixel state, one allocation made on first use: the adaptive family's layout with `part`
    // (rtw_adaptive_plan.h adaptive_layout(npix, true))
    DevBuf adapt;
    // the accumulation session (rtw.h rtw_accum_*; a group's lives in kids[0]). It owns its per-pixel state, one allocation: accum,
    // upart, part (rtw_accum.h), with RTW_ACCUM_ERROR mom and the error map a read computes. An add borrows the context's scratch
    // (blocksum, job order, queue, lanes, stats rows: all dead again when the add returns), never its accum / upart / part / adapt.
    struct Accum {
        bool active = false;
        rtw_params P{};
        uint32_t flags = 0;
        int32_t done = 0;
        uint64_t samples = 0, segments = 0, shadow_rays = 0;
        size_t npix = 0;
        DevBuf slab;
        float4 *accum = nullptr, *upart = nullptr, *part = nullptr;
        double2* mom = nullptr;
        float* err = nullptr;
    } acc;
    // The query family's scratch (rtw_cast ... rtw_views_adaptive), each grown on demand and kept until rtw_destroy.
    // The host variants' staging slab: one chunk's inputs and results, laid out per call by rtw_stage_plan.h. Every call that uses it
    // returns synchronised, so one slab serves them all.
    DevBuf stage_slab;         // (in bytes, like the next three)
    DevBuf rad_slab;           // the unit sums [unit][ray] of calls beyond 128 spp; the block sums of an adaptive pass
    DevBuf view_buf;           // the view records of a host call
    DevBuf dn_buf;             // rtw_denoise_views: the ping-pong buffer, and the host variant's colour, guides and output beside it
    DevBuf rad_ctl;            // the control words: kStatRows rows of 8 counters, then the queue word (query_open)
    // rtw_probe_adaptive's per-probe state (rtw_adaptive_plan.h adaptive_layout(n, false)), one allocation grown on demand and kept;
    // rtw_views_adaptive's per-pixel state as well (the same layout over the pixels of a call or batch: a call initialises what it uses)
    DevBuf padapt;             // (in probes)
    uint64_t scene_fp = 0;  // accum_fingerprint of the uploaded blob (on the context the caller holds)
};

// One persistent host thread per kid context of a group (n_devices > 1). The caller's thread hands it one shard per render
// call and waits; no thread is created or joined per call.
struct Worker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    bool has_job = false, done = false, quit = false;
    // the job (written by the caller's thread before has_job is set, read by the worker; results the other way)
    rtw_params P{};
    size_t npix = 0;
    float4* gather_dst = nullptr;  // where the shard goes on the group's first device
    int gather_dev = 0;
    bool want_stats = false;
    rtw_stats st{};
    int rc = RTW_OK;
};

namespace {

int fail(rtw_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(ctx, e_ == hipErrorOutOfMemory ? RTW_ERR_OOM : RTW_ERR_DEVICE,             \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                        \
    } while (0)

constexpr size_t kQueueBytes = 64;                                                   // rtw_ctx::d_queue
constexpr size_t kStatsBytes = (kStatRows + 1) * 8 * sizeof(unsigned long long);      // rtw_ctx::d_stats
constexpr size_t kCtlBytes = (kStatRows * 8 + 2) * sizeof(unsigned long long);        // rtw_ctx::rad_ctl

void free_lane(rtw_ctx::Lane& L) {
    for (int b = 0; b < 2; b++) {
        L.slab[b].release();
        L.buf[b] = PathBuf{};
        L.hit[b] = nullptr;
    }
    L.lbuf.release();
    L.paths = 0;
    L.probes = false;
}
void free_pool(rtw_ctx* c) {
    for (auto& L : c->lane) {
        free_lane(L);
        L.cnt.release();
    }
}

// Streams that must run side by side get DIFFERENT priorities. The runtime maps streams onto a few hardware queues
// (GPU_MAX_HW_QUEUES, default 4) round-robin in creation order, and two streams that land on one queue serialise: whether the
// two lanes overlapped used to depend on how many streams the process (torch, an earlier render) had created before them
// (measured: scene 1 at 3.3 instead of 4.1 Gsamples/s after one small k_path render). Queues are pooled per priority class,
// so a normal- and a high-priority stream never share one.
hipError_t create_stream(hipStream_t* st, int cls /* 0 normal, 1 high, 2 low */) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest) return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    const int normal = (least + greatest) / 2;
    const int prio = cls == 1 ? greatest : (cls == 2 ? least : normal);
    return hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio);
}

int ensure_lane(rtw_ctx* c, rtw_ctx::Lane& L, size_t paths, size_t cnt_words, bool probes) {
    if (!L.st) {
        const int idx = (int)(&L - c->lane);
        HIP_TRY(c, create_stream(&L.st, idx & 1));
        HIP_TRY(c, hipEventCreateWithFlags(&L.ev_done, hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&L.ev_free, hipEventDisableTiming));
    }
    if (paths > L.paths || (probes && !L.probes)) {
        paths = std::max(paths, L.paths);
        free_lane(L);
        // the state planes and the hit records of one ping-pong set live in one slab, page-aligned: with listed lights six
        // 16-byte planes + the 8-byte hit records (104 B per path); without (no probe is ever queued: rtw_kernels.h store_path)
        // p2 is not there and p5 is a plane of dwords: 76 B per path - a third less of what decides how large a batch can be
        auto al = [](size_t v) { return (v + 4095) & ~(size_t)4095; };
        const size_t full = al(paths * sizeof(float4));
        const size_t sz[7] = {full, full, probes ? full : 0, full, full, probes ? full : al(paths * sizeof(uint32_t)), al(paths * sizeof(uint2))};
        size_t off[8] = {0};
        for (int k = 0; k < 7; k++) off[k + 1] = off[k] + sz[k];
        for (int b = 0; b < 2; b++) {
            HIP_TRY(c, L.slab[b].grow(paths, off[7] + 4096));
            char* base = L.slab[b].as<char>();
            L.buf[b].p0 = (float4*)(base + off[0]); L.buf[b].p1 = (float4*)(base + off[1]); L.buf[b].p2 = (float4*)(base + off[2]);
            L.buf[b].p3 = (float4*)(base + off[3]); L.buf[b].p4 = (float4*)(base + off[4]); L.buf[b].p5 = (uint4*)(base + off[5]);
            L.hit[b] = (uint2*)(base + off[6]);
        }
        HIP_TRY(c, L.lbuf.grow(paths, paths * sizeof(float4)));
        L.paths = paths;
        L.probes = probes;
    }
    HIP_TRY(c, L.cnt.grow(cnt_words, cnt_words * sizeof(uint32_t)));
    return RTW_OK;
}

int ensure_pool(rtw_ctx* c, int n_lanes, size_t paths, size_t npix, size_t cnt_words, bool probes = true) {
    for (int l = 0; l < n_lanes; l++) {
        int rc = ensure_lane(c, c->lane[l], paths, cnt_words, probes);
        if (rc) return rc;
    }
    if (n_lanes == 0) HIP_TRY(c, c->d_queue.grow(kQueueBytes, kQueueBytes));
    for (DevBuf* b : {&c->accum, &c->part, &c->upart}) HIP_TRY(c, b->grow(npix, npix * sizeof(float4)));
    HIP_TRY(c, c->d_stats.grow(kStatsBytes, kStatsBytes));
    return RTW_OK;
}

// which: RTW_K_FIRST, RTW_K_SHADE, RTW_K_TRACE, RTW_K_BOUNCE or RTW_K_PATH. list: k_first / k_path over a.list (LIST = 1).
// walk_shape: k_path only, the uploaded scene's SceneInfo::walk_shape. The row is rtw_variants.h's choice.
void launch(int which, int rng_kind, const KArgs& a, int grid, size_t lds, hipStream_t s, int block = kBlock, bool list = false, int walk_shape = 0) {
    Kernel k;
    switch (which) {
    case RTW_K_FIRST: k = kFirstKernels[first_row(rng_kind, a.sc.has_tex, list)]; break;
    case RTW_K_SHADE: k = kShadeKernels[shade_row(rng_kind, a.sc.has_tex)]; lds = 0; break;
    case RTW_K_TRACE: k = a.sc.use_bvh ? kTraceBvhKernels[trace_bvh_row(block, trace_bvh_mode(a.sc))] : kTraceKernels[trace_row(a.sc)]; break;
    case RTW_K_PATH: k = kPathKernels[path_row(rng_kind, a.sc, walk_shape, list)]; break;
    default: k = kBounceKernels[bounce_row(rng_kind, a.sc.has_tex)]; break;
    }
    hipLaunchKernelGGL(k, dim3(grid), dim3(which == RTW_K_TRACE && a.sc.use_bvh ? block : kBlock), lds, s, a);
}

// ---- the exception barrier of the C ABI (include/rtw.h: "no exceptions cross this ABI") -------------------------------
// The implementations below use std::vector / std::string / std::thread and may throw (bad_alloc, system_error). Every
// extern "C" entry point runs its implementation inside guarded(): an exception becomes an error code and a message, as the
// reference's OPTIX_CHECK / CUDA_CHECK exceptions (Director.cpp:106-122) become the Director's exit path.
int fail_nothrow(rtw_ctx* c, int code, const char* msg) noexcept {
    if (c) {
        try { c->err.assign(msg); } catch (...) { c->err.clear(); }  // (clear() does not allocate)
    }
    return code;
}
// Test hook (tests/test_abi.py, tests/test_gpu_round3.py): RTW_TEST_FAULT="<where>:<kind>" makes the named point of the library
// throw (kind bad_alloc | runtime), so that the barrier and the worker threads' containment can be exercised on purpose.
// where: entry (every entry point, before its arguments are looked at), upload (after the scene tables are staged),
// worker (inside a group's worker thread, before its render).
void test_fault(const char* where) {
    const char* e = getenv("RTW_TEST_FAULT");
    if (!e || !*e) return;
    const size_t n = strlen(where);
    if (strncmp(e, where, n) != 0 || e[n] != ':') return;
    if (strcmp(e + n + 1, "bad_alloc") == 0) throw std::bad_alloc();
    throw std::runtime_error(std::string("injected fault at ") + where);
}
template <class F>
int guarded(rtw_ctx* c, F&& f) noexcept {
    try {
        test_fault("entry");
        return f();
    } catch (const std::bad_alloc&) {
        return fail_nothrow(c, RTW_ERR_OOM, "out of host memory (std::bad_alloc)");
    } catch (const std::exception& e) {
        return fail_nothrow(c, RTW_ERR_DEVICE, e.what());
    } catch (...) {
        return fail_nothrow(c, RTW_ERR_DEVICE, "unknown exception");
    }
}

int impl_destroy(rtw_ctx* c);
void accum_free(rtw_ctx* c);
int impl_render_device(rtw_ctx* c, const rtw_params* P, void* d_rgba, void* hip_stream, rtw_stats* stats);
void worker_main(rtw_ctx* kc);

int create_single(rtw_ctx** out, int device) {
    rtw_ctx* c = new (std::nothrow) rtw_ctx();
    if (!c) return RTW_ERR_OOM;
    c->device = device;
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return RTW_ERR_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
    *out = c;
    return RTW_OK;
}

int impl_create(rtw_ctx** out, int n_devices, const int* device_ids) {
    if (n_devices < 1 || n_devices > 64) return RTW_ERR_INVALID_ARG;
    rtw_ctx* c = nullptr;
    int rc = create_single(&c, device_ids ? device_ids[0] : 0);
    if (rc) return rc;
    if (n_devices > 1) {
        // a group: one single-device context per entry of device_ids (entries may repeat: two shards on one GPU)
        for (int g = 0; g < n_devices; g++) {
            rtw_ctx* k = nullptr;
            rc = create_single(&k, device_ids ? device_ids[g] : g);
            if (rc) { impl_destroy(c); return rc; }
            try {
                c->kids.push_back(k);
            } catch (...) { impl_destroy(k); impl_destroy(c); throw; }
            // the kid's host thread, for the lifetime of the group (std::thread's constructor may throw std::system_error:
            // the caller's guard turns that into an error code once the half-built group is gone)
            try {
                k->worker = new Worker();
                k->worker->th = std::thread(worker_main, k);
            } catch (...) { impl_destroy(c); throw; }
            if (k->device != c->device) {  // direct peer copies for the gather where the link allows them; not an error if not
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, c->device, k->device) == hipSuccess && can) {
                    (void)hipSetDevice(c->device);
                    (void)hipDeviceEnablePeerAccess(k->device, 0);
                    (void)hipGetLastError();  // hipErrorPeerAccessAlreadyEnabled is fine
                }
            }
        }
        (void)hipSetDevice(c->device);
    }
    *out = c;
    return RTW_OK;
}

int impl_destroy(rtw_ctx* c) {
    if (!c) return RTW_ERR_INVALID_ARG;
    for (rtw_ctx* k : c->kids) (void)impl_destroy(k);
    c->kids.clear();
    if (c->worker) {
        if (c->worker->th.joinable()) {
            {
                std::lock_guard<std::mutex> lk(c->worker->m);
                c->worker->quit = true;
            }
            c->worker->cv.notify_all();
            c->worker->th.join();
        }
        delete c->worker;
        c->worker = nullptr;
    }
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& L : c->lane) {
        if (L.ev_done) (void)hipEventDestroy(L.ev_done);
        if (L.ev_free) (void)hipEventDestroy(L.ev_free);
        if (L.st) (void)hipStreamDestroy(L.st);
    }
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;  // its buffers go with it, while its device is the current one
    return RTW_OK;
}

// one device's share of an upload: the staged image copied, DScene bound to it
int upload_prepared(rtw_ctx* c, const PreparedScene& ps) {
    test_fault("upload");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->d_scene.release();
    c->has_scene = false;
    accum_free(c);  // a session belongs to the scene it was begun with
    HIP_TRY(c, c->d_scene.grow(ps.image.size(), ps.image.size()));
    HIP_TRY(c, hipMemcpy(c->d_scene.as<void>(), ps.image.data(), ps.image.size(), hipMemcpyHostToDevice));
    const char* d = c->d_scene.as<char>();
    const SceneScalars& v = ps.sc;
    const SceneFacts& f = ps.info.facts;
    DScene sc{};
    sc.prims = (const rtw_prim*)(d + ps.off[ST_PRIMS]);
    sc.xforms = (const rtw_xform*)(d + ps.off[ST_XFORMS]);
    sc.hitrec = (const HitRec*)(d + ps.off[ST_HITREC]);
    sc.lights = (const rtw_light*)(d + ps.off[ST_LIGHTS]);
    sc.clights = (const rtw_light*)(d + ps.off[ST_CLIGHTS]);
    sc.nodes = (const u32x4*)(d + ps.off[ST_NODES]);
    sc.wnodes = (const u32x4*)(d + ps.off[ST_WNODES]);
    sc.leaves = (const u32x4*)(d + ps.off[ST_LEAVES]);
    sc.order = (const int32_t*)(d + ps.off[ST_ORDER]);
    sc.groups = (const BruteGroup*)(d + ps.off[ST_GROUPS]);
    sc.recs = (const BruteRec*)(d + ps.off[ST_RECS]);
    sc.texs = (const rtw_texture*)(d + ps.off[ST_TEXS]);
    sc.texdata = (const uint32_t*)(d + ps.off[ST_TEXDATA]);
    sc.walk = (const u32x4*)(d + ps.off[ST_WALK]);
    sc.n_prims = v.n_prims; sc.n_tree = v.n_tree; sc.n_lights = v.n_lights; sc.sky_light = v.sky_light; sc.has_motion = v.has_motion;
    sc.n_groups = v.n_groups; sc.n_generic = v.n_generic; sc.n_walk_words = v.n_walk_words; sc.n_lds_nodes = v.n_lds_nodes; sc.has_tex = v.has_tex;
    sc.noise_lds_data = v.noise_lds_data; sc.n_lds_leaves = v.n_lds_leaves; sc.cam_type = v.cam_type;
    sc.use_bvh = f.use_bvh ? 1 : 0; sc.n_vol = f.n_vol; sc.stack_depth = f.stack_depth; sc.stack_wide = f.stack_wide ? 1 : 0; sc.n_nodes = (int32_t)f.n_tree_nodes;
    sc.estimator = RTW_EST_REFERENCE; sc.ray_tmin = 1e-6f; sc.probe_eps = 500 * 1.0e-7f;  // set per render
    for (int a = 0; a < 3; a++) { sc.bmin[a] = v.bmin[a]; sc.bmax[a] = v.bmax[a]; }
    sc.cam = v.cam;
    sc.pdf = v.pdf;
    c->sc = sc;
    c->info = ps.info;
    c->has_scene = true;
    return RTW_OK;
}

// The blob is prepared once on the host (rtw_scene.h: nothing of the context changes when it is refused); every device of a group
// then gets its own copy of the staged image.
int impl_upload_scene(rtw_ctx* c, const void* blob, size_t bytes) {
    if (!c) return RTW_ERR_INVALID_ARG;
    if (!c->kids.empty()) c->has_scene = false;
    PreparedScene ps;
    std::string err;
    const int prc = prepare_scene(blob, bytes, read_tuning(), ps, err);
    if (prc) return fail(c, prc, err);
    c->scene_fp = accum_fingerprint(blob, bytes);
    if (c->kids.empty()) return upload_prepared(c, ps);
    for (rtw_ctx* k : c->kids) {
        const int rc = upload_prepared(k, ps);
        if (rc) return fail(c, rc, k->err);
    }
    c->has_scene = true;
    return RTW_OK;
}

int check_render_args(rtw_ctx* c, const rtw_params* P) {
    if (!c->has_scene) return fail(c, RTW_ERR_NO_SCENE, "rtw_render before rtw_upload_scene");
    if (!P) return fail(c, RTW_ERR_INVALID_ARG, "null params");
    if (P->width <= 0 || P->height <= 0 || P->spp <= 0 || P->max_depth < 0 || P->row0 < 0 || P->row1 > P->height || P->row0 > P->row1)
        return fail(c, RTW_ERR_INVALID_ARG, "bad render params");
    if (P->rng_kind != RTW_RNG_PHILOX && P->rng_kind != RTW_RNG_TEA_LCG) return fail(c, RTW_ERR_INVALID_ARG, "bad rng_kind");
    if (P->sample_offset < 0 || P->samples_per_pass < 0 || P->row_stride < 0) return fail(c, RTW_ERR_INVALID_ARG, "bad sample_offset/samples_per_pass/row_stride");
    if (P->estimator < RTW_EST_REFERENCE || P->estimator > RTW_EST_MIXTURE) return fail(c, RTW_ERR_INVALID_ARG, "bad estimator");
    return RTW_OK;
}

size_t shard_rows(const rtw_params* P) {
    const size_t k = P->row_stride > 1 ? (size_t)P->row_stride : 1;
    return ((size_t)(P->row1 - P->row0) + k - 1) / k;
}

unsigned pixel_grid(const rtw_ctx* c, size_t npix) { return (unsigned)std::min<size_t>((npix + kBlock - 1) / kBlock, (size_t)c->n_cu * 8); }

// kernel arguments that every kernel of a render shares: the scene as uploaded, the shard, the seed, depth and sample count
KArgs shard_args(const DScene& sc, const rtw_params* P, size_t npix) {
    KArgs a{};
    a.sc = sc;
    a.npix = (uint32_t)npix;
    a.width = (uint32_t)P->width;
    a.height = (uint32_t)P->height;
    a.row0 = (uint32_t)P->row0;
    a.row_stride = P->row_stride > 1 ? (uint32_t)P->row_stride : 1u;
    magic_div((uint32_t)P->width, a.divw_m, a.divw_s1, a.divw_s2);
    magic_div(a.row_stride, a.divs_m, a.divs_s1, a.divs_s2);
    a.seed = P->seed;
    a.max_depth = (uint32_t)P->max_depth;
    a.stack_stride = kBlock;
    a.spp = (uint32_t)P->spp;
    a.cull_x0 = 0; a.cull_x1 = P->width; a.cull_y0 = 0; a.cull_y1 = P->height;  // nothing culled (path_cull sets the rectangle)
    return a;
}

// One render call's record: timing events from a pool kept in the context (reused across launches and calls), the (kernel kind,
// start, stop) triples of its timed launches, and the launches rtw_stats.bounce_launches counts
struct CallLog {
    rtw_ctx* c;
    int rng_kind;
    bool timing;  // per-launch events: the caller asked for rtw_stats and RTW_KERNEL_TIMING is not 0
    struct Timed { int kind; hipEvent_t a, b; };
    std::vector<Timed> timed;
    size_t ev_used = 0;
    hipEvent_t begin = nullptr, end = nullptr;
    uint64_t launches = 0;
    uint64_t culled_segments = 0;  // k_path renders: one segment per sample of the pixels no kernel was given (rtw_plan.h cull_rect)

    hipError_t event(hipEvent_t& e) {
        if (ev_used == c->ev_pool.size()) {
            hipEvent_t n = nullptr;
            hipError_t er = hipEventCreate(&n);
            if (er != hipSuccess) return er;
            c->ev_pool.push_back(n);
        }
        e = c->ev_pool[ev_used++];
        return hipSuccess;
    }
    // work issued on stream s between open() and close() is timed as one launch of `kind`
    hipError_t open(Timed& t, int kind, hipStream_t s) {
        t = Timed{kind, nullptr, nullptr};
        if (!timing) return hipSuccess;
        hipError_t er = event(t.a);
        if (er == hipSuccess) er = event(t.b);
        if (er == hipSuccess) er = hipEventRecord(t.a, s);
        return er;
    }
    hipError_t close(const Timed& t, hipStream_t s) {
        if (!timing) return hipSuccess;
        timed.push_back(t);
        return hipEventRecord(t.b, s);
    }
    hipError_t launch(hipStream_t s, int kind, const KArgs& a, int grid, size_t lds, int block = kBlock, bool list = false) {
        Timed t;
        hipError_t er = open(t, kind, s);
        if (er != hipSuccess) return er;
        ::launch(kind, rng_kind, a, grid, lds, s, block, list);
        return close(t, s);
    }
};

// the context's two timing events, out of its pool (no event is created once a context has timed anything)
hipError_t timing_events(rtw_ctx* d, hipEvent_t ev[2]) {
    while (d->ev_pool.size() < 2) {
        hipEvent_t n = nullptr;
        const hipError_t e = hipEventCreate(&n);
        if (e != hipSuccess) return e;
        d->ev_pool.push_back(n);
    }
    ev[0] = d->ev_pool[0]; ev[1] = d->ev_pool[1];
    return hipSuccess;
}

// ---- the launch schedules that rtw_render, rtw_render_adaptive and rtw_accum_add share. Each renderer plans its own launches (rtw_plan.h)
// and resolves them with its own kernel; how a planned pass or batch is issued, how the pool is fitted and how a call's counters
// become rtw_stats is written once, here.

// Workgroups per CU of a persistent launch of `kernel` with `lds` bytes of dynamic LDS: `override` where it is set (> 0), else what the
// occupancy query admits, at most 8, and 4 where the query fails (that only costs occupancy: these launches draw from a queue or stride
// over the grid, any grid computes the same)
int path_wg_per_cu(const void* kernel, size_t lds, int override) {
    if (override > 0) return override;
    int nb = 0;
    const hipError_t qe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, kBlock, lds);
    return (qe == hipSuccess && nb > 0) ? std::min(nb, 8) : 4;
}

// Groups of 64 pixels that certainly see nothing get no job: a miss adds +0 (no sky light), so their pixels stay at 0 and their
// samples - one segment each, as the oracle counts them - are added to the call's counts on the host (culled_pixels x samples).
// Sets base.cull_*; rcull is the same rectangle for the resolve kernels.
struct PathCull { size_t live_groups, culled_pixels; ResolveCull rcull; };
PathCull path_cull(const rtw_ctx* c, const rtw_params* P, const Tuning& tune, KArgs& base, size_t npix) {
    PathCull pc{~(size_t)0, 0, {}};
    if (tune.cull && c->info.cull_ok) {
        const CullRect r = cull_rect(c->sc.cam, c->sc.cam_type, c->sc.sky_light, c->info.cull_bmin, c->info.cull_bmax, P->width, P->height);
        base.cull_x0 = r.x0; base.cull_x1 = r.x1; base.cull_y0 = r.y0; base.cull_y1 = r.y1;
        pc.live_groups = cull_live_groups(r, npix, base.width, base.row0, base.row_stride, &pc.culled_pixels);
    }
    pc.rcull = ResolveCull{base.cull_x0, base.cull_x1, base.cull_y0, base.cull_y1, base.width, base.row0, base.row_stride, base.divw_m, base.divw_s1, base.divw_s2};
    return pc;
}

// job order: longest units first (k_classify), into c->d_order with the lists' lengths at c->d_queue + 1
int classify_jobs(rtw_ctx* c, const KArgs& base, size_t n_groups, hipStream_t s) {
    uint32_t* const order = c->d_order.as<uint32_t>();
    uint32_t* const counts = c->d_queue.as<uint32_t>() + 1;
    HIP_TRY(c, hipMemsetAsync(c->d_queue.as<void>(), 0, kQueueBytes, s));
    const dim3 cg((unsigned)std::min<size_t>((n_groups + 3) / 4, (size_t)c->n_cu * 8));
    hipLaunchKernelGGL(kClassifyKernels[classify_row(c->sc)], cg, dim3(kBlock), 0, s, base, order, counts, (uint32_t)n_groups);
    return RTW_OK;
}

// what one k_path pass runs over: the shard's pixels in k_classify's order, or the pixels of an active list (rtw_adaptive.h)
struct PathTarget {
    size_t n_items;                // pixels of the shard, or of the list: the stride of the sums' buffer
    const uint32_t* order;         // the job order (c->d_order), or the list
    const uint32_t* order_counts;  // the lengths of the order's three lists; null for a list
    bool list;                     // k_path's LIST = 1 twin
    uint32_t blk0;                 // absolute index of the plan's block 0 (the samples before it are done: adaptive passes, accum adds)
    uint32_t spp_end;              // KArgs::spp: the last sample of the range, counted from sample0
    int rng_kind;
    uint32_t sample0;
};

// One pass of a PathPlan: the bulk launch on s and the fine-grained end-game launch beside it on stream2, which starts after what s held
// before the pass and which s waits for. The caller resolves c->blocksum on s afterwards. unit_sums: the plan's, for the bulk launch.
int issue_path_pass(rtw_ctx* c, CallLog& log, const KArgs& base, const PathPass& ps, bool unit_sums, const PathTarget& target, hipStream_t s) {
    // render_path and accum_add_path have d_queue from ensure_pool before they point target.order_counts into it; only the list caller,
    // whose order_counts is null, can arrive here without one. A caller that needs the counts must allocate d_queue first.
    HIP_TRY(c, c->d_queue.grow(kQueueBytes, kQueueBytes));
    uint32_t* const queue = c->d_queue.as<uint32_t>();
    // low priority: it fills the slots the bulk launch vacates. Created by a context's first pass, after the call's begin event: that
    // one call's stats.seconds includes the stream's creation
    if (!c->stream2) HIP_TRY(c, create_stream(&c->stream2, 2));
    HIP_TRY(c, hipMemsetAsync(queue, 0, 4, s));
    HIP_TRY(c, hipMemsetAsync(queue + 4, 0, 4, s));
    hipEvent_t ev_a = nullptr, ev_b = nullptr;  // (from the call's event pool, like the wavefront lanes' start event)
    HIP_TRY(c, log.event(ev_a));
    HIP_TRY(c, log.event(ev_b));
    HIP_TRY(c, hipEventRecord(ev_a, s));
    // the two launches of a pass overlap, so they are timed as one: from before the first to after both (on s, which waits
    // for the second stream's launch below); rocprofv3 lists them as two dispatches whose durations both span the pass
    CallLog::Timed tp;
    HIP_TRY(c, log.open(tp, RTW_K_PATH, s));
    for (int part = 0; part < 2; part++) {
        const PathLaunch& l = ps.part[part];
        if (l.count == 0) continue;
        KArgs a = base;
        a.stats = c->d_stats.as<unsigned long long>();
        a.sample0 = target.sample0;
        a.spp = target.spp_end;
        a.queue = queue + (part == 0 ? 0 : 4);
        a.order = target.order;
        a.order_counts = target.order_counts;
        a.blocksum = c->blocksum.as<float4>() + (part == 0 ? 0 : ps.slots_coarse) * target.n_items;
        a.unit_sums = (part == 0 && unit_sums) ? 1u : 0u;
        a.n_jobs = (uint32_t)l.n_jobs; a.n_ranges = (uint32_t)l.n_ranges; a.units_per_job = (uint32_t)l.jb;
        a.block0 = target.blk0 + (uint32_t)(ps.b0 + l.first); a.n_blocks_pass = (uint32_t)l.count; a.unit_blocks = (uint32_t)l.unit_blocks;
        hipStream_t ls = part == 0 ? s : c->stream2;
        if (part == 1) HIP_TRY(c, hipStreamWaitEvent(ls, ev_a, 0));
        launch(RTW_K_PATH, target.rng_kind, a, l.grid, 0, ls, kBlock, target.list, c->info.walk_shape);
        log.launches++;
        if (part == 1) {
            HIP_TRY(c, hipEventRecord(ev_b, ls));
            HIP_TRY(c, hipStreamWaitEvent(s, ev_b, 0));
        }
    }
    HIP_TRY(c, log.close(tp, s));
    return RTW_OK;
}

// One batch of the wavefront pipeline on lane L, once `ready` has happened: k_first starts `paths` camera paths (Sb samples of each
// pixel; list: of each listed pixel), then the plan's schedule. a: the batch's arguments (the render's, with sample0 of the batch)
int issue_batch(rtw_ctx* c, const WavefrontPlan& w, const Tuning& tune, KArgs a, rtw_ctx::Lane& L, size_t paths, size_t Sb, hipEvent_t ready,
                CallLog& log, bool list) {
    const size_t lds = c->info.lds_bytes;
    const uint32_t regions = w.grid_for(paths);
    HIP_TRY(c, hipStreamWaitEvent(L.st, ready, 0));
    uint32_t* const cnt = L.cnt.as<uint32_t>();
    HIP_TRY(c, hipMemsetAsync(cnt, 0, (size_t)regions * (w.sched.size() + 2) * sizeof(uint32_t), L.st));
    a.lbuf = L.lbuf.as<float4>();
    a.stats = c->d_stats.as<unsigned long long>();
    a.n_regions = regions;
    a.n_paths = (uint32_t)paths;
    a.region_cap = (uint32_t)w.cap_for(paths);
    a.trace_first = w.split_first ? 1u : 0u;
    a.first_group_log2 = 0;
    while (a.first_group_log2 < (uint32_t)tune.first_group_log2 && (Sb >> (a.first_group_log2 + 1)) << (a.first_group_log2 + 1) == Sb) a.first_group_log2++;
    // k_first fills buffer 0 (and the hit buffer); every compacting launch then flips the buffers
    int cur = 0;
    size_t ci = 0;  // index of the region-counter row describing buffer `cur`
    a.out = L.buf[0];
    a.hit_out = L.hit[0];
    a.cnt_out = cnt;
    a.depth = 0; a.n_iter = 1;
    log.launches++;
    // every compacting launch uses exactly this grid: workgroup b owns region b
    HIP_TRY(c, log.launch(L.st, RTW_K_FIRST, a, (int)regions, c->sc.use_bvh ? (size_t)(kBlock / 64) * (size_t)c->info.facts.stack_depth * sizeof(uint32_t) : 0, kBlock, list));
    for (const Step& st : w.sched) {
        a.in = L.buf[cur];
        a.hit = L.hit[cur];
        a.hit_out = L.hit[cur];  // k_trace fills the records of the buffer it reads
        a.cnt_in = cnt + ci * regions;
        a.depth = (uint32_t)st.depth;
        a.n_iter = (uint32_t)st.n_iter;
        if (st.kind == RTW_K_TRACE) {
            if (c->sc.use_bvh) {  // its own workgroup size, LDS image and grid: waves own streams of chunks, not regions
                KArgs at = a;
                at.sc.n_lds_nodes = w.trace_nodes; at.sc.n_lds_leaves = w.trace_leaves;
                HIP_TRY(c, log.launch(L.st, RTW_K_TRACE, at, w.trace_grid, w.trace_lds, w.trace_block));
            } else {
                HIP_TRY(c, log.launch(L.st, RTW_K_TRACE, a, (int)regions, lds));
            }
        } else {
            a.out = L.buf[cur ^ 1];
            a.hit_out = L.hit[cur ^ 1];
            a.cnt_out = cnt + (ci + 1) * regions;
            HIP_TRY(c, log.launch(L.st, st.kind, a, (int)regions, st.kind == RTW_K_BOUNCE ? lds : 0));
            cur ^= 1;
            ci++;
        }
        log.launches++;
    }
    return RTW_OK;
}
// Plans the wavefront batches (plan_fn: the caller's plan_wavefront call, which reads c->pool_cap) and sizes the pool for them: paths_fn(w)
// paths per lane, counters and accumulators for npix pixels. A trace launch beyond the default dynamic-LDS limit gets its attribute raised.
template <class PlanFn, class PathsFn>
int fit_wavefront_pool(rtw_ctx* c, const Tuning& tune, int samples_per_pass, size_t npix, PlanFn plan_fn, PathsFn paths_fn, WavefrontPlan& w) {
    for (;;) {
        w = plan_fn();
        if (w.trace_lds > 48 * 1024) {  // beyond the default dynamic-LDS limit of a launch
            DScene ts = c->sc;
            ts.n_lds_nodes = w.trace_nodes;
            const void* f = (const void*)kTraceBvhKernels[trace_bvh_row(w.trace_block, trace_bvh_mode(ts))];
            HIP_TRY(c, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.trace_lds));
        }
        const int rc = ensure_pool(c, w.n_lanes, paths_fn(w), npix, w.cnt_words, c->sc.n_lights > 0);
        if (rc == RTW_OK) return RTW_OK;
        if (rc != RTW_ERR_OOM || samples_per_pass > 0 || w.S <= 1) return rc;
        // The pool is sized for an MI355X to itself (2^29 paths: up to 120 GiB). A device with less to give - another process on
        // it, a smaller part - gets half as many paths in flight, and half again, until the allocation fits: smaller batches,
        // the same image (a path's draws and a pixel's summation order do not depend on the batch size).
        free_pool(c);
        (void)hipGetLastError();
        c->pool_cap = std::max<size_t>((size_t)tune.lanes * npix, npix * w.S * (size_t)tune.lanes / 2);
    }
}

// The batches of `step` samples per item (a pixel of the shard; list: a pixel of the list) alternate between the lanes; batch b holds
// samples [s0, s0 + Sb) of the step and draws from first_sample + s0 on. The lanes start after what s holds now; resolve(L, Sb, s0)
// launches the caller's resolve kernel for lane L's batch on s, in batch order.
template <class Resolve>
int run_batches(rtw_ctx* c, const WavefrontPlan& w, const Tuning& tune, const KArgs& base, size_t items, size_t step, int first_sample,
                const uint32_t* list, hipStream_t s, CallLog& log, Resolve resolve) {
    if (base.max_depth == 0) return RTW_OK;  // no segment is traced: nothing to launch
    hipEvent_t ev_ready = nullptr;
    HIP_TRY(c, log.event(ev_ready));
    HIP_TRY(c, hipEventRecord(ev_ready, s));
    for (size_t s0 = 0, b = 0; s0 < step; b++) {
        const size_t Sb = w.batch_size(b, s0);
        rtw_ctx::Lane& L = c->lane[b % (size_t)w.n_lanes];
        KArgs a = base;
        a.sample0 = (uint32_t)(first_sample + (int)s0);
        if (list) a.order = list;
        // this lane's pool is free again once the resolve of its previous batch has run on the main stream
        const int rc = issue_batch(c, w, tune, a, L, items * Sb, Sb, b < (size_t)w.n_lanes ? ev_ready : L.ev_free, log, list != nullptr);
        if (rc) return rc;
        // batches are resolved in order, on the main stream
        HIP_TRY(c, hipEventRecord(L.ev_done, L.st));
        HIP_TRY(c, hipStreamWaitEvent(s, L.ev_done, 0));
        resolve(L, Sb, s0);
        HIP_TRY(c, hipEventRecord(L.ev_free, s));
        s0 += Sb;
    }
    return RTW_OK;
}

// hs: the column sums of the kStatRows rows of 8 counters at d_rows (segments, shadow rays, then the segments by kernel kind)
int sum_stat_rows(rtw_ctx* c, const unsigned long long* d_rows, unsigned long long hs[8]) {
    unsigned long long rows_[kStatRows * 8];
    HIP_TRY(c, hipMemcpy(rows_, d_rows, sizeof rows_, hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; k++) hs[k] = 0;
    for (uint32_t r = 0; r < kStatRows; r++)
        for (int k = 0; k < 8; k++) hs[k] += rows_[r * 8 + k];
    return RTW_OK;
}

// a finished call's rtw_stats (zeroed by the caller): its times from the log's events, its counts from the summed rows
int fill_stats(rtw_ctx* c, const CallLog& log, const unsigned long long hs[8], uint64_t samples, uint64_t segments, rtw_stats* stats) {
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, log.begin, log.end));
    stats->seconds = (double)ms * 1e-3;
    stats->bounce_seconds = stats->seconds;  // the lanes overlap: the loop time is the elapsed time of the call
    for (const CallLog::Timed& t : log.timed) {
        float m = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&m, t.a, t.b));
        stats->kernel_seconds[t.kind] += (double)m * 1e-3;
        stats->kernel_launches[t.kind]++;
    }
    for (int k = 0; k < RTW_K_COUNT; k++) stats->kernel_segments[k] = hs[2 + k];  // (what the kernels shaded themselves)
    stats->bounce_launches = log.launches;
    stats->samples = samples;
    stats->segments = segments;
    stats->shadow_rays = hs[1];
    stats->algorithmic_bytes = 128ull * segments + 32ull * samples;
    return RTW_OK;
}

// ---- k_path: paths in registers, lanes regenerate; only the unit sums (16 B per pixel and 64 samples) reach HBM
int render_path(rtw_ctx* c, const rtw_params* P, const Tuning& tune, const KArgs& base_in, float4* out, hipStream_t s, CallLog& log) {
    const size_t npix = base_in.npix;
    int rc = ensure_pool(c, 0, 0, npix, 0);
    if (rc) return rc;
    KArgs base = base_in;
    const PathCull cull = path_cull(c, P, tune, base, npix);
    log.culled_segments = (uint64_t)cull.culled_pixels * (uint64_t)P->spp;
    const int wg_per_cu = path_wg_per_cu((const void*)kPathKernels[path_row(P->rng_kind, base.sc, c->info.walk_shape, false)], 0, tune.path_grid_mult);
    const PathPlan plan = plan_path(tune, npix, P->spp, c->n_cu, wg_per_cu, cull.live_groups);
    if (plan.too_many_jobs) return fail(c, RTW_ERR_UNSUPPORTED, "too many k_path jobs");
    HIP_TRY(c, c->d_order.grow(plan.n_groups, 3 * plan.n_groups * sizeof(uint32_t)));  // k_classify's three job lists
    HIP_TRY(c, c->blocksum.grow(plan.need_slots * npix, plan.need_slots * npix * sizeof(float4)));
    float4* const accum = c->accum.as<float4>();
    const float4* const blocksum = c->blocksum.as<float4>();
    HIP_TRY(c, hipEventRecord(log.begin, s));
    HIP_TRY(c, hipMemsetAsync(accum, 0, npix * sizeof(float4), s));
    HIP_TRY(c, hipMemsetAsync(c->d_stats.as<void>(), 0, kStatsBytes, s));
    if ((rc = classify_jobs(c, base, plan.n_groups, s)) != RTW_OK) return rc;
    const unsigned pix_grid = pixel_grid(c, npix);
    const PathTarget target{npix, c->d_order.as<uint32_t>(), c->d_queue.as<uint32_t>() + 1, false, 0u, (uint32_t)P->spp, P->rng_kind, (uint32_t)P->sample_offset};
    for (const PathPass& ps : plan.passes) {
        if (cull.live_groups == 0) break;  // the frame looks past everything: black, nothing to launch
        if ((rc = issue_path_pass(c, log, base, ps, plan.unit_sums, target, s)) != RTW_OK) return rc;
        // coarse region: whole unit sums (unit_sums) or block sums from block b0 on; fine region: block sums from b0 + nb_coarse on
        if (plan.unit_sums)
            hipLaunchKernelGGL(k_resolve_blocks, dim3(pix_grid), dim3(kBlock), 0, s, blocksum, accum, (uint32_t)npix, (uint32_t)ps.slots_coarse,
                               (uint32_t)(ps.nb - ps.nb_coarse), (uint32_t)(ps.b0 + ps.nb_coarse), cull.rcull);
        else
            hipLaunchKernelGGL(k_resolve_blocks, dim3(pix_grid), dim3(kBlock), 0, s, blocksum, accum, (uint32_t)npix, 0u, (uint32_t)ps.nb, (uint32_t)ps.b0, cull.rcull);
    }
    hipLaunchKernelGGL(k_finish, dim3(pix_grid), dim3(kBlock), 0, s, (const float4*)accum, (const float4*)nullptr, (const float4*)nullptr, out, (uint32_t)npix, (float)P->spp);
    return RTW_OK;
}

// ---- wavefront pipeline (tree scenes; RTW_PATH=0): batches of S samples per pixel alternate between the lanes
int render_wavefront(rtw_ctx* c, const rtw_params* P, const Tuning& tune, const KArgs& base, float4* out, hipStream_t s, CallLog& log) {
    const size_t npix = base.npix;
    WavefrontPlan w;
    int rc = fit_wavefront_pool(c, tune, P->samples_per_pass, npix,
                                [&] { return plan_wavefront(tune, npix, P->spp, P->samples_per_pass, P->max_depth, c->pool_cap, c->n_cu, c->info.facts); },
                                [](const WavefrontPlan& p) { return (size_t)p.regions_max * p.region_cap_max; }, w);
    if (rc) return rc;
    float4 *const accum = c->accum.as<float4>(), *const upart = c->upart.as<float4>(), *const part = c->part.as<float4>();
    HIP_TRY(c, hipEventRecord(log.begin, s));
    HIP_TRY(c, hipMemsetAsync(accum, 0, npix * sizeof(float4), s));
    HIP_TRY(c, hipMemsetAsync(part, 0, npix * sizeof(float4), s));
    HIP_TRY(c, hipMemsetAsync(upart, 0, npix * sizeof(float4), s));
    HIP_TRY(c, hipMemsetAsync(c->d_stats.as<void>(), 0, kStatsBytes, s));
    const unsigned pix_grid = pixel_grid(c, npix);
    // the lanes start once the accumulators are cleared
    rc = run_batches(c, w, tune, base, npix, (size_t)P->spp, P->sample_offset, nullptr, s, log, [&](rtw_ctx::Lane& L, size_t Sb, size_t s0) {
        hipLaunchKernelGGL(k_resolve, dim3(pix_grid), dim3(kBlock), 0, s, L.lbuf.as<const float4>(), accum, upart, part, (uint32_t)npix, (uint32_t)Sb, (uint32_t)s0);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_finish, dim3(pix_grid), dim3(kBlock), 0, s, (const float4*)accum, (const float4*)upart, (const float4*)part, out, (uint32_t)npix, (float)P->spp);
    return RTW_OK;
}

// Diagnostic builds only (scripts/build_variant.sh with -DRTW_PHASE_TIMERS, -DRTW_SUBPHASE_TIMERS or -DRTW_TRACE_COUNT): the kernels'
// extra counters, printed to stderr once the render has ended. hs: the summed stats rows.
int print_diagnostics(rtw_ctx* c, bool path, const unsigned long long* hs) {
#ifdef RTW_PHASE_TIMERS
    if (path) {
        unsigned long long ph[8];
        HIP_TRY(c, hipMemcpy(ph, c->d_stats.as<unsigned long long>() + kStatRows * 8, sizeof ph, hipMemcpyDeviceToHost));
        double tot = 0;
        for (int q = 0; q < 6; q++) tot += (double)ph[q];
        const char* nm[6] = {"refill", "regen", "walk_r", "shade_a", "walk_s", "shade_b"};
        fprintf(stderr, "[rtw] k_path wave-cycles by phase:");
        for (int q = 0; q < 6; q++) fprintf(stderr, " %s %.1f%%", nm[q], 100.0 * (double)ph[q] / tot);
        fprintf(stderr, " (total %.3g wave-cycles, %.0f per 64 segments)\n", tot, tot / ((double)hs[0] / 64.0));
    }
#endif
#ifdef RTW_SUBPHASE_TIMERS
    if (path) {
        static std::vector<unsigned long long> tab((size_t)kSubWaves * kSubRows);
        HIP_TRY(c, hipMemcpyFromSymbol(tab.data(), HIP_SYMBOL(g_sub_cyc), tab.size() * sizeof(unsigned long long)));
        double sum[kSubRows] = {0};
        for (size_t w = 0; w < (size_t)kSubWaves; w++) for (int q = 0; q < 14; q++) sum[q] += (double)tab[w * kSubRows + q];
        double tot = 0;
        for (int q = 0; q < 14; q++) tot += sum[q];
        const char* nm[9] = {"outside", "hitrec+philox", "lambert", "light", "metal", "diel", "iso", "nee", "entry"};
        fprintf(stderr, "[rtw] k_path wave-cycles by sub-phase of the closest-hit program:");
        for (int q = 0; q < 9; q++) fprintf(stderr, " %s %.1f%%", nm[q], 100.0 * sum[q] / tot);
        fprintf(stderr, " (total %.3g)\n", tot);
        std::fill(tab.begin(), tab.end(), 0ull);
        HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(g_sub_cyc), tab.data(), tab.size() * sizeof(unsigned long long)));
    }
#endif
#ifdef RTW_TRACE_COUNT
    {
        unsigned long long w[7];
        HIP_TRY(c, hipMemcpy(w, c->d_stats.as<unsigned long long>() + kStatRows * 8, sizeof w, hipMemcpyDeviceToHost));
        const double rays = (double)w[6];
        fprintf(stderr, "[rtw] k_trace_bvh: rays %.4g; per ray: node visits %.2f, primitive tests %.2f; wave steps per 64 rays: inner %.2f (lanes busy %.2f), leaf %.2f (lanes busy %.2f), outer %.2f\n",
                rays, (double)hs[6] / rays, (double)hs[7] / rays, (double)w[0] * 64.0 / rays, (double)hs[6] / ((double)w[0] * 64.0), (double)w[1] * 64.0 / rays,
                (double)hs[7] / ((double)w[1] * 64.0), (double)hs[2 + RTW_K_BOUNCE] * 64.0 / rays);
        const double tt = (double)(w[2] + w[3] + w[4] + w[5]);
        fprintf(stderr, "[rtw] k_trace_bvh wave-cycles: refill %.1f%% inner %.1f%% leaf %.1f%% finish %.1f%% (%.0f per 64 rays; per inner wave step %.0f, per leaf wave step %.0f)\n",
                100.0 * (double)w[2] / tt, 100.0 * (double)w[3] / tt, 100.0 * (double)w[4] / tt, 100.0 * (double)w[5] / tt, tt * 64.0 / rays,
                (double)w[3] / (double)w[0], (double)w[4] / (double)w[1]);
    }
#endif
    (void)c; (void)path; (void)hs;
    return RTW_OK;
}

// the kernel arguments of a render: shard_args, and the corrected estimators' settings
KArgs render_args(const rtw_ctx* c, const rtw_params* P, size_t npix) {
    KArgs base = shard_args(c->sc, P, npix);
    apply_estimator(base.sc, P->estimator);
    return base;
}

// One device: the whole render of the shard P describes, result in d_rgba (device memory of c->device).
int render_single(rtw_ctx* c, const rtw_params* P, void* d_rgba, hipStream_t s, rtw_stats* stats) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (!s) s = c->stream;
    const size_t npix = shard_rows(P) * (size_t)P->width;
    if (stats) memset(stats, 0, sizeof *stats);
    if (npix == 0) return RTW_OK;
    if (npix > 0xffffffffull / 2) return fail(c, RTW_ERR_UNSUPPORTED, "tile too large");

    const Tuning tune = read_tuning();
    CallLog log{c, P->rng_kind, stats != nullptr && tune.kernel_timing};
    HIP_TRY(c, log.event(log.begin));
    HIP_TRY(c, log.event(log.end));
    const KArgs base = render_args(c, P, npix);
    const bool use_path = path_pipeline(c->sc, P->width, P->height, P->max_depth, tune);
    int rc = use_path ? render_path(c, P, tune, base, (float4*)d_rgba, s, log) : render_wavefront(c, P, tune, base, (float4*)d_rgba, s, log);
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(log.end, s));
    HIP_TRY(c, hipEventSynchronize(log.end));

    unsigned long long hs[8];
    if ((rc = sum_stat_rows(c, c->d_stats.as<unsigned long long>(), hs)) != RTW_OK) return rc;
    rc = print_diagnostics(c, use_path, hs);
    if (rc) return rc;
    if (stats) return fill_stats(c, log, hs, (uint64_t)npix * (uint64_t)P->spp, hs[0] + log.culled_segments, stats);
    return RTW_OK;
}

// rows of the gathered shards -> rows of the frame: frame row r is row r / n of shard r % n
__global__ void __launch_bounds__(256) k_interleave(const float4* __restrict__ stage, float4* __restrict__ out, uint32_t width, uint32_t rows, uint32_t n,
                                                    const uint32_t* __restrict__ shard_off) {
    const size_t total = (size_t)rows * width;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / width), x = (uint32_t)(i - (size_t)r * width);
        const uint32_t g = r % n, l = r / n;
        out[i] = stage[((size_t)shard_off[g] + l) * width + x];
    }
}

// n_devices > 1: kid g renders rows row0 + g*k, row0 + (g + n)*k ... of the shard (k = the caller's row stride) on its own
// device from its own (persistent) host thread and then PUSHES its float4 shard to device_ids[0] with one
// hipMemcpyPeerAsync on its own stream - n concurrent transfers, one per inbound xGMI link of the gathering device (single
// process: a peer copy is the xGMI transfer an RCCL send/recv pair would issue) - and the rows are interleaved there.
int run_shard(rtw_ctx* kc, Worker& w) {
    test_fault("worker");
    if (hipSetDevice(kc->device) != hipSuccess) return fail(kc, RTW_ERR_DEVICE, "hipSetDevice failed");
    if (w.npix == 0) return RTW_OK;
    if (kc->d_out.grow(w.npix, w.npix * sizeof(float4)) != hipSuccess) return fail(kc, RTW_ERR_OOM, "shard buffer");
    const int rc = render_single(kc, &w.P, kc->d_out.as<void>(), nullptr, w.want_stats ? &w.st : nullptr);
    if (rc) return rc;
    HIP_TRY(kc, hipMemcpyPeerAsync(w.gather_dst, w.gather_dev, kc->d_out.as<void>(), kc->device, w.npix * sizeof(float4), kc->stream));
    HIP_TRY(kc, hipStreamSynchronize(kc->stream));
    return RTW_OK;
}
void worker_main(rtw_ctx* kc) {
    Worker& w = *kc->worker;
    for (;;) {
        try {
            std::unique_lock<std::mutex> lk(w.m);
            w.cv.wait(lk, [&] { return w.has_job || w.quit; });
            if (w.quit) return;
            lk.unlock();
            int rc;
            try {
                rc = run_shard(kc, w);
            } catch (const std::bad_alloc&) {
                rc = fail_nothrow(kc, RTW_ERR_OOM, "out of host memory in a worker thread (std::bad_alloc)");
            } catch (const std::exception& e) {
                rc = fail_nothrow(kc, RTW_ERR_DEVICE, e.what());
            } catch (...) {
                rc = fail_nothrow(kc, RTW_ERR_DEVICE, "unknown exception in a worker thread");
            }
            lk.lock();
            w.rc = rc; w.has_job = false; w.done = true;
            lk.unlock();
            w.cv.notify_all();
        } catch (...) {
            // a failing lock: nothing sane is left to do with this thread's queue; report once and leave
            w.rc = RTW_ERR_DEVICE; w.has_job = false; w.done = true;
            w.cv.notify_all();
            return;
        }
    }
}
int render_group(rtw_ctx* c, const rtw_params* P, void* d_rgba, hipStream_t s, rtw_stats* stats) {
    const size_t n = c->kids.size();
    const size_t k = P->row_stride > 1 ? (size_t)P->row_stride : 1;
    const size_t rows = shard_rows(P);
    if (stats) memset(stats, 0, sizeof *stats);
    if (rows == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!s) s = c->stream;
    const size_t npix = rows * (size_t)P->width;
    HIP_TRY(c, c->stage.grow(npix, npix * sizeof(float4) + (n + 1) * sizeof(uint32_t) + 256));
    std::vector<uint32_t> off(n + 1, 0);
    std::vector<size_t> krows(n, 0);
    for (size_t g = 0; g < n; g++) {
        krows[g] = rows > g ? (rows - g + n - 1) / n : 0;
        off[g + 1] = off[g] + (uint32_t)krows[g];
    }
    // hand every kid its shard, then wait for all of them (a failing or throwing kid reports through its rc)
    for (size_t g = 0; g < n; g++) {
        Worker& w = *c->kids[g]->worker;
        std::lock_guard<std::mutex> lk(w.m);
        w.P = *P;
        w.P.row0 = P->row0 + (int32_t)(g * k);
        w.P.row_stride = (int32_t)(k * n);
        if (w.P.row0 > w.P.row1) w.P.row0 = w.P.row1;
        w.npix = krows[g] * (size_t)P->width;
        w.gather_dst = c->stage.as<float4>() + (size_t)off[g] * P->width;
        w.gather_dev = c->device;
        w.want_stats = stats != nullptr;
        memset(&w.st, 0, sizeof w.st);
        w.rc = RTW_OK; w.done = false; w.has_job = true;
    }
    for (size_t g = 0; g < n; g++) c->kids[g]->worker->cv.notify_all();
    int first_rc = RTW_OK;
    size_t first_bad = 0;
    for (size_t g = 0; g < n; g++) {
        Worker& w = *c->kids[g]->worker;
        std::unique_lock<std::mutex> lk(w.m);
        w.cv.wait(lk, [&] { return w.done; });
        if (w.rc != RTW_OK && first_rc == RTW_OK) { first_rc = w.rc; first_bad = g; }
    }
    if (first_rc != RTW_OK)
        return fail(c, first_rc, std::string("device ") + std::to_string(c->kids[first_bad]->device) + ": " + c->kids[first_bad]->err);
    HIP_TRY(c, hipSetDevice(c->device));
    uint32_t* d_off = (uint32_t*)(c->stage.as<char>() + ((npix * sizeof(float4) + 255) & ~(size_t)255));
    HIP_TRY(c, hipMemcpyAsync(d_off, off.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_interleave, dim3((unsigned)std::min<size_t>((npix + 255) / 256, (size_t)c->n_cu * 8)), dim3(256), 0, s, c->stage.as<const float4>(),
                       (float4*)d_rgba, (uint32_t)P->width, (uint32_t)rows, (uint32_t)n, (const uint32_t*)d_off);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(s));
    if (stats) {
        for (size_t g = 0; g < n; g++) {
            const rtw_stats& ks = c->kids[g]->worker->st;
            stats->samples += ks.samples; stats->segments += ks.segments; stats->shadow_rays += ks.shadow_rays;
            stats->algorithmic_bytes += ks.algorithmic_bytes; stats->bounce_launches += ks.bounce_launches;
            stats->seconds = std::max(stats->seconds, ks.seconds);
            stats->bounce_seconds = std::max(stats->bounce_seconds, ks.bounce_seconds);
            for (int q = 0; q < RTW_K_COUNT; q++) {
                stats->kernel_seconds[q] += ks.kernel_seconds[q]; stats->kernel_launches[q] += ks.kernel_launches[q];
                stats->kernel_segments[q] += ks.kernel_segments[q];
            }
        }
    }
    return RTW_OK;
}

int impl_render_device(rtw_ctx* c, const rtw_params* P, void* d_rgba, void* hip_stream, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    int rc = check_render_args(c, P);
    if (rc) return rc;
    if (!d_rgba) return fail(c, RTW_ERR_INVALID_ARG, "null params or output");
    if (!c->kids.empty()) return render_group(c, P, d_rgba, (hipStream_t)hip_stream, stats);
    return render_single(c, P, d_rgba, (hipStream_t)hip_stream, stats);
}

int impl_render(rtw_ctx* c, const rtw_params* P, float* rgba_out, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    if (!rgba_out) return fail(c, RTW_ERR_INVALID_ARG, "null output");
    if (!P) return fail(c, RTW_ERR_INVALID_ARG, "null params");
    if (P->width <= 0 || P->row0 < 0 || P->row1 < P->row0) return fail(c, RTW_ERR_INVALID_ARG, "bad render params");
    const size_t npix = shard_rows(P) * (size_t)P->width;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_out.grow(npix, std::max<size_t>(npix, 1) * sizeof(float4)));
    int rc = impl_render_device(c, P, c->d_out.as<void>(), nullptr, stats);
    if (rc) return rc;
    if (npix) HIP_TRY(c, hipMemcpy(rgba_out, c->d_out.as<void>(), npix * sizeof(float4), hipMemcpyDeviceToHost));  // Director.cpp:999-1000
    return RTW_OK;
}

// ---- the adaptive family (rtw.h: rtw_render_adaptive, rtw_probe_adaptive, rtw_views_adaptive): one state, one checkpoint loop
// (rtw_adaptive.h, rtw_adaptive_plan.h). An entry is a shard pixel, a probe or a pixel of the views at hand.
struct AdaptiveState {
    float4 *accum, *upart, *part;  // part: null unless the layout has it
    double2* mom;
    uint32_t *n, *total, *list[2], *offsets;
    float* err;
    unsigned long long* masks;
};

// the state for n entries in `buf`, a context-owned allocation grown on demand and kept (the layout for n fits in an allocation made
// for more entries); drain: DevBuf::grow's
int adaptive_state(rtw_ctx* c, DevBuf& buf, size_t n, bool want_part, const hipStream_t* drain, AdaptiveState& st) {
    typedef AdaptiveLayout AL;
    const AL l = adaptive_layout(n, want_part);
    HIP_TRY(c, buf.grow(n, (size_t)l.bytes(), drain));
    char* b = buf.as<char>();
    st.accum = (float4*)(b + l.off[AL::kAccum]); st.upart = (float4*)(b + l.off[AL::kUpart]); st.part = want_part ? (float4*)(b + l.off[AL::kPart]) : nullptr;
    st.mom = (double2*)(b + l.off[AL::kMom]); st.n = (uint32_t*)(b + l.off[AL::kN]); st.err = (float*)(b + l.off[AL::kErr]);
    st.total = (uint32_t*)(b + l.off[AL::kTotal]); st.list[0] = (uint32_t*)(b + l.off[AL::kList0]); st.list[1] = (uint32_t*)(b + l.off[AL::kList1]);
    st.masks = (unsigned long long*)(b + l.off[AL::kMasks]); st.offsets = (uint32_t*)(b + l.off[AL::kOffsets]);
    return RTW_OK;
}

// the stop rule's frames: n_views views of width x height (the renderer: one view of width x rows; probes: one view of n x 1, dilate 0)
AdaptDecideArgs adaptive_frames(uint32_t width, uint32_t height, size_t n_views, float threshold, int dilate) {
    AdaptDecideArgs da{};
    da.width = width; da.height = height; da.npix = (uint32_t)(n_views * width * height);
    magic_div(width, da.divw_m, da.divw_s1, da.divw_s2);
    magic_div(width * height, da.divf_m, da.divf_s1, da.divf_s2);
    da.dilate = (uint32_t)dilate; da.threshold = threshold;
    return da;
}

// RTW_VERBOSE=1, rtw_render_adaptive: a row of the pass table, timed from before the pass to after the compaction
struct AdaptivePassRec { int n_from, n_to; size_t active; hipEvent_t a, b; };

// The checkpoint loop over the da.npix entries of state st, on stream s of device context d (c: the context the caller holds, for
// errors): the start, then per checkpoint one pass over the list of the active entries, the decision, the compaction and one count
// read-back - the next pass is planned on the active count - and at last the results. It returns when `finish` has been issued.
// `samples` receives the sum of the entries' sample counts. What a family hands in:
//   pass(list, n_active, n_from, n_to)   samples [n_from, n_to) of the n_active entries of `list`, resolved into the state; -> RTW_OK or an error
//   finish(grid)                         the results
// table: where not null, every pass leaves a row, its events taken from log.
template <class Pass, class Finish>
int adaptive_run(rtw_ctx* c, rtw_ctx* d, const AdaptiveState& st, AdaptDecideArgs da, const std::vector<int>& cps, hipStream_t s, uint64_t& samples,
                 CallLog* log, std::vector<AdaptivePassRec>* table, Pass pass, Finish finish) {
    const size_t n = da.npix;
    const unsigned all_grid = pixel_grid(d, n);
    const uint32_t n_waves = (uint32_t)((n + 63) / 64);
    hipLaunchKernelGGL(k_adapt_init, dim3(all_grid), dim3(kBlock), 0, s, st.list[0], st.accum, st.upart, st.part, st.mom, st.n, st.err, st.total, (uint32_t)n);
    HIP_TRY(c, hipGetLastError());
    size_t n_active = n;
    int cur = 0, n_prev = 0;
    for (size_t k = 0; k < cps.size() && n_active > 0; k++) {
        const int n_k = cps[k];
        if (table) {
            table->push_back(AdaptivePassRec{n_prev, n_k, n_active, nullptr, nullptr});
            HIP_TRY(c, log->event(table->back().a));
            HIP_TRY(c, log->event(table->back().b));
            HIP_TRY(c, hipEventRecord(table->back().a, s));
        }
        const int rc = pass(st.list[cur], n_active, n_prev, n_k);
        if (rc) return rc;
        samples += (uint64_t)n_active * (uint64_t)(n_k - n_prev);
        da.B = (uint32_t)n_k / kSumBlock; da.at_cap = k + 1 == cps.size() ? 1u : 0u;
        hipLaunchKernelGGL(k_adapt_decide, dim3(std::min<unsigned>((n_waves + 3) / 4, (unsigned)d->n_cu * 8)), dim3(kBlock), 0, s, (const double2*)st.mom,
                           (const uint32_t*)st.n, st.err, st.masks, da);
        hipLaunchKernelGGL(k_adapt_scan, dim3(1), dim3(1024), 0, s, (const unsigned long long*)st.masks, st.offsets, n_waves, st.list[cur ^ 1]);
        hipLaunchKernelGGL(k_adapt_compact, dim3(all_grid), dim3(kBlock), 0, s, (const unsigned long long*)st.masks, (const uint32_t*)st.offsets, st.n,
                           st.list[cur ^ 1], (uint32_t)n, (uint32_t)n_k);
        HIP_TRY(c, hipGetLastError());
        if (table) HIP_TRY(c, hipEventRecord(table->back().b, s));
        uint32_t cnt = 0;  // one read-back, one host synchronisation per checkpoint
        HIP_TRY(c, hipMemcpyAsync(&cnt, st.list[cur ^ 1], sizeof cnt, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        n_active = cnt;
        cur ^= 1;
        n_prev = n_k;
    }
    finish(all_grid);
    HIP_TRY(c, hipGetLastError());
    return RTW_OK;
}

// ---- rtw_render_adaptive (rtw.h): the family's loop over the shard's pixels; a pass is k_path's or the wavefront pipeline's
// k_path over the n_list pixels of `list` (length word, then the pixels: rtw_adaptive.h): blocks [n_from / 16, n_to / 16) of each, resolved into the state
int adaptive_path_pass(rtw_ctx* c, const rtw_params* P, const Tuning& tune, const KArgs& base, const AdaptiveState& st, const uint32_t* list,
                       size_t n_list, int n_from, int n_to, hipStream_t s, CallLog& log) {
    // every block's sum must reach memory (the moments are taken over blocks): no lane unit may be a whole summation unit
    Tuning t = tune;
    if (t.path_unit_blocks % (int)kSumUnitBlocks == 0) t.path_unit_blocks = 4;
    const int wg_per_cu = path_wg_per_cu((const void*)kPathKernels[path_row(P->rng_kind, base.sc, c->info.walk_shape, true)], 0, t.path_grid_mult);
    const PathPlan plan = plan_path(t, n_list, n_to - n_from, c->n_cu, wg_per_cu);
    if (plan.too_many_jobs) return fail(c, RTW_ERR_UNSUPPORTED, "too many k_path jobs");
    HIP_TRY(c, c->blocksum.grow(plan.need_slots * n_list, plan.need_slots * n_list * sizeof(float4)));
    int rc;
    const uint32_t blk0 = (uint32_t)n_from / kSumBlock;
    const PathTarget target{n_list, list, nullptr, true, blk0, (uint32_t)n_to, P->rng_kind, (uint32_t)P->sample_offset};
    for (const PathPass& ps : plan.passes) {
        if ((rc = issue_path_pass(c, log, base, ps, false, target, s)) != RTW_OK) return rc;
        hipLaunchKernelGGL(k_adapt_resolve_blocks, dim3(pixel_grid(c, n_list)), dim3(kBlock), 0, s, c->blocksum.as<const float4>(), list, (uint32_t)n_list,
                           (uint32_t)ps.nb, blk0 + (uint32_t)ps.b0, st.accum, st.upart, st.mom);
    }
    return RTW_OK;
}

// the wavefront pipeline over the n_list pixels of `list`: samples [n_from, n_to) of each. Path ids keep the shard's stride
// (slot * npix + pixel), so a batch's radiance buffer needs Sb * npix slots: a list batch takes at most the samples per pixel that a
// full-frame batch would (the pool's share per lane over npix), and the lane's buffers are sized for that many slots.
int adaptive_wavefront_pass(rtw_ctx* c, const rtw_params* P, const Tuning& tune, const KArgs& base, const AdaptiveState& st, const uint32_t* list,
                            size_t n_list, int n_from, int n_to, hipStream_t s, CallLog& log) {
    const size_t npix = base.npix;
    const size_t step = (size_t)(n_to - n_from);
    WavefrontPlan w;
    int rc = fit_wavefront_pool(c, tune, P->samples_per_pass, npix,
                                [&] {  // the batch size is chosen here, over npix, and handed to the plan (whose w.S is then this S)
                                    size_t S = P->samples_per_pass > 0 ? (size_t)P->samples_per_pass : std::max<size_t>(1, std::min(tune.pool_paths, c->pool_cap) / (size_t)tune.lanes / npix);
                                    S = std::min(S, step);
                                    while (S > 1 && npix * S > 0xfffffff0ull) S--;
                                    return plan_wavefront(tune, n_list, (int)step, (int)S, P->max_depth, c->pool_cap, c->n_cu, c->info.facts);
                                },
                                [&](const WavefrontPlan& p) { return std::max((size_t)p.regions_max * p.region_cap_max, p.S * npix); }, w);
    if (rc) return rc;
    const unsigned grid = pixel_grid(c, n_list);
    // the lanes start after the previous checkpoint's decision (the list) on s
    return run_batches(c, w, tune, base, n_list, step, P->sample_offset + n_from, list, s, log, [&](rtw_ctx::Lane& L, size_t Sb, size_t s0) {
        hipLaunchKernelGGL(k_adapt_resolve_samples, dim3(grid), dim3(kBlock), 0, s, L.lbuf.as<const float4>(), list, (uint32_t)n_list, (uint32_t)npix,
                           (uint32_t)Sb, (uint32_t)(n_from + (int)s0), st.accum, st.upart, st.part, st.mom);
    });
}

// one device (a group's first): the checkpoints, a pass and a decision per checkpoint, the final image
int render_adaptive_single(rtw_ctx* c, const rtw_params* P, const rtw_adaptive* AD, const std::vector<int>& cps, float* rgba_out, int32_t* spp_out,
                           float* error_out, rtw_stats* stats) {
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t rows = shard_rows(P), npix = rows * (size_t)P->width;
    if (stats) memset(stats, 0, sizeof *stats);
    if (npix == 0) return RTW_OK;
    if (npix > 0xffffffffull / 2) return fail(c, RTW_ERR_UNSUPPORTED, "tile too large");
    const Tuning tune = read_tuning();
    CallLog log{c, P->rng_kind, stats != nullptr && tune.kernel_timing};
    HIP_TRY(c, log.event(log.begin));
    HIP_TRY(c, log.event(log.end));
    const KArgs base = render_args(c, P, npix);
    const bool use_path = path_pipeline(c->sc, P->width, P->height, P->max_depth, tune);
    AdaptiveState st{};
    int rc = adaptive_state(c, c->adapt, npix, true, nullptr, st);
    if (rc) return rc;
    HIP_TRY(c, c->d_stats.grow(kStatsBytes, kStatsBytes));
    HIP_TRY(c, c->d_out.grow(npix, npix * sizeof(float4)));
    HIP_TRY(c, hipEventRecord(log.begin, s));
    HIP_TRY(c, hipMemsetAsync(c->d_stats.as<void>(), 0, kStatsBytes, s));
    uint64_t samples = 0;
    std::vector<AdaptivePassRec> passes;  // RTW_VERBOSE=1: the pass table, printed to stderr at the end
    rc = adaptive_run(
        c, c, st, adaptive_frames((uint32_t)P->width, (uint32_t)rows, 1, AD->threshold, AD->dilate), cps, s, samples, &log, tune.verbose ? &passes : nullptr,
        [&](const uint32_t* list, size_t n_active, int n_from, int n_to) {
            return use_path ? adaptive_path_pass(c, P, tune, base, st, list, n_active, n_from, n_to, s, log)
                            : adaptive_wavefront_pass(c, P, tune, base, st, list, n_active, n_from, n_to, s, log);
        },
        [&](unsigned grid) {  // (n and err are copied out of the state below)
            hipLaunchKernelGGL(k_adapt_finish, dim3(grid), dim3(kBlock), 0, s, (const float4*)st.accum, (const float4*)st.upart, (const uint32_t*)st.n,
                               (const float*)st.err, c->d_out.as<float4>(), (int32_t*)nullptr, (float*)nullptr, (uint32_t)npix, 0u);
        });
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(log.end, s));
    HIP_TRY(c, hipMemcpyAsync(rgba_out, c->d_out.as<void>(), npix * sizeof(float4), hipMemcpyDeviceToHost, s));
    if (spp_out) HIP_TRY(c, hipMemcpyAsync(spp_out, st.n, npix * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (error_out) HIP_TRY(c, hipMemcpyAsync(error_out, st.err, npix * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    for (size_t k = 0; k < passes.size(); k++) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, passes[k].a, passes[k].b));
        const double smp = (double)passes[k].active * (double)(passes[k].n_to - passes[k].n_from);
        fprintf(stderr, "[rtw] adaptive pass %zu: spp %d -> %d, active %zu, samples %.0f, seconds %.6f, Msamples/s %.1f\n", k, passes[k].n_from,
                passes[k].n_to, passes[k].active, smp, ms * 1e-3, smp / std::max(ms * 1e-3, 1e-12) / 1e6);
    }
    if (stats) {
        unsigned long long hs[8];
        if ((rc = sum_stat_rows(c, c->d_stats.as<unsigned long long>(), hs)) != RTW_OK) return rc;
        return fill_stats(c, log, hs, samples, hs[0], stats);
    }
    return RTW_OK;
}

int impl_render_adaptive(rtw_ctx* c, const rtw_params* P, const rtw_adaptive* AD, float* rgba_out, int32_t* spp_out, float* error_out, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    int rc = check_render_args(c, P);
    if (rc) return rc;
    if (!AD || !rgba_out) return fail(c, RTW_ERR_INVALID_ARG, "rtw_render_adaptive: null settings or output");
    std::vector<int> cps;
    if (const char* why = adaptive_checkpoints(AD->min_spp, AD->step_spp, P->spp, AD->threshold, AD->dilate, cps))
        return fail(c, RTW_ERR_INVALID_ARG, std::string("rtw_render_adaptive: ") + why);
    rtw_ctx* d = c->kids.empty() ? c : c->kids[0];  // a group renders on device_ids[0]
    rc = render_adaptive_single(d, P, AD, cps, rgba_out, spp_out, error_out, stats);
    if (rc && d != c) return fail(c, rc, d->err);
    return rc;
}

// ---- accumulation sessions (rtw.h rtw_accum_*): the uniform launches of render_path / render_wavefront over samples [done, done + spp),
// resolved into the session's own state by the kernels of rtw_accum.h, which keep the summation unit open from add to add
void accum_free(rtw_ctx* c) {
    if (c->acc.slab) (void)hipSetDevice(c->device);
    c->acc = rtw_ctx::Accum{};  // (the slab with it)
}

// the session's allocation for npix pixels: accum, upart, part, with RTW_ACCUM_ERROR mom and err
int accum_alloc(rtw_ctx* c, size_t npix, uint32_t flags) {
    rtw_ctx::Accum& A = c->acc;
    const bool em = (flags & RTW_ACCUM_ERROR) != 0;
    const size_t sz[5] = {npix * 16, npix * 16, npix * 16, em ? npix * 16 : 0, em ? npix * 4 : 0};
    size_t off[6] = {0};
    for (int k = 0; k < 5; k++) off[k + 1] = off[k] + ((sz[k] + 255) & ~(size_t)255);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, A.slab.grow(off[5], off[5]));
    char* b = A.slab.as<char>();
    A.accum = (float4*)(b + off[0]); A.upart = (float4*)(b + off[1]); A.part = (float4*)(b + off[2]);
    A.mom = em ? (double2*)(b + off[3]) : nullptr;
    A.err = em ? (float*)(b + off[4]) : nullptr;
    A.npix = npix;
    A.flags = flags;
    const hipError_t e = hipMemsetAsync(b, 0, off[5], c->stream);
    if (e != hipSuccess) { accum_free(c); return fail(c, RTW_ERR_DEVICE, std::string("rtw_accum: ") + hipGetErrorString(e)); }
    return RTW_OK;
}

// k_path over samples [n_from, n_to) of every pixel (both multiples of kSumBlock, counted from sample_offset): render_path's launches -
// k_classify's job order, the cull, the bulk launch and the end-game launch beside it, unit sums where plan_path picks 8-block units -
// split where a unit-sum launch would not start on a unit boundary (rtw_accum_state.h accum_split)
int accum_add_path(rtw_ctx* c, const Tuning& tune, const KArgs& base_in, int n_from, int n_to, hipStream_t s, CallLog& log) {
    const rtw_ctx::Accum& A = c->acc;
    const rtw_params* P = &A.P;
    const size_t npix = base_in.npix;
    int rc = ensure_pool(c, 0, 0, npix, 0);
    if (rc) return rc;
    KArgs base = base_in;
    const PathCull cull = path_cull(c, P, tune, base, npix);
    log.culled_segments = (uint64_t)cull.culled_pixels * (uint64_t)(n_to - n_from);
    const int wg_per_cu = path_wg_per_cu((const void*)kPathKernels[path_row(P->rng_kind, base.sc, c->info.walk_shape, false)], 0, tune.path_grid_mult);
    const size_t n_groups = (npix + 63) / 64;
    HIP_TRY(c, c->d_order.grow(n_groups, 3 * n_groups * sizeof(uint32_t)));
    HIP_TRY(c, hipEventRecord(log.begin, s));
    HIP_TRY(c, hipMemsetAsync(c->d_stats.as<void>(), 0, kStatsBytes, s));
    if (cull.live_groups == 0) return RTW_OK;  // the frame looks past everything: the state stays black
    if ((rc = classify_jobs(c, base, n_groups, s)) != RTW_OK) return rc;  // once per add
    const unsigned pix_grid = pixel_grid(c, npix);
    // one plan per run (rtw_accum_state.h accum_runs: the head on its own, the whole units and the open tail behind them together),
    // all planned before the first launch so that the sums' buffer is sized once, as render_path sizes it
    const AccumRuns runs = accum_runs(accum_split(n_from, n_to, A.mom != nullptr), A.mom != nullptr);
    PathPlan plans[2];
    size_t need_slots = 0;
    for (int k = 0; k < runs.n; k++) {
        Tuning t = tune;  // every block's sum must reach memory (adaptive_path_pass): no lane unit may be a whole summation unit
        if (!runs.run[k].units_ok && t.path_unit_blocks % (int)kSumUnitBlocks == 0) t.path_unit_blocks = 4;
        plans[k] = plan_path(t, npix, runs.run[k].n_to - runs.run[k].n_from, c->n_cu, wg_per_cu, cull.live_groups);
        if (plans[k].too_many_jobs) return fail(c, RTW_ERR_UNSUPPORTED, "too many k_path jobs");
        if (plans[k].unit_sums && !runs.run[k].units_ok) return fail(c, RTW_ERR_UNSUPPORTED, "rtw_accum_add: unit sums off a unit boundary");
        need_slots = std::max(need_slots, plans[k].need_slots);
    }
    HIP_TRY(c, c->blocksum.grow(need_slots * npix, need_slots * npix * sizeof(float4)));
    for (int k = 0; k < runs.n; k++) {
        const PathPlan& plan = plans[k];
        const uint32_t blk0 = (uint32_t)runs.run[k].n_from / kSumBlock;
        const PathTarget target{npix, c->d_order.as<uint32_t>(), c->d_queue.as<uint32_t>() + 1, false, blk0, (uint32_t)runs.run[k].n_to, P->rng_kind, (uint32_t)P->sample_offset};
        for (const PathPass& ps : plan.passes) {
            if ((rc = issue_path_pass(c, log, base, ps, plan.unit_sums, target, s)) != RTW_OK) return rc;
            // coarse region: whole unit sums (unit_sums) or block sums from block b0 of the run on; fine region: block sums
            const uint32_t n_unit = plan.unit_sums ? (uint32_t)ps.slots_coarse : 0u;
            const uint32_t n_blk = plan.unit_sums ? (uint32_t)(ps.nb - ps.nb_coarse) : (uint32_t)ps.nb;
            const uint32_t first = blk0 + (uint32_t)(plan.unit_sums ? ps.b0 + ps.nb_coarse : ps.b0);
            hipLaunchKernelGGL(k_accum_resolve_blocks, dim3(pix_grid), dim3(kBlock), 0, s, c->blocksum.as<const float4>(), (uint32_t)npix, n_unit, n_blk, first,
                               A.accum, A.upart, A.mom, cull.rcull);
        }
    }
    return RTW_OK;
}

// the wavefront pipeline over samples [n_from, n_to) of every pixel: render_wavefront's batches, resolved into the session's state
int accum_add_wavefront(rtw_ctx* c, const Tuning& tune, const KArgs& base, int n_from, int n_to, hipStream_t s, CallLog& log) {
    const rtw_ctx::Accum& A = c->acc;
    const rtw_params* P = &A.P;
    const size_t npix = base.npix;
    const size_t step = (size_t)(n_to - n_from);
    WavefrontPlan w;
    const int rc = fit_wavefront_pool(c, tune, P->samples_per_pass, npix,
                                      [&] { return plan_wavefront(tune, npix, (int)step, P->samples_per_pass, P->max_depth, c->pool_cap, c->n_cu, c->info.facts); },
                                      [](const WavefrontPlan& p) { return (size_t)p.regions_max * p.region_cap_max; }, w);
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(log.begin, s));
    HIP_TRY(c, hipMemsetAsync(c->d_stats.as<void>(), 0, kStatsBytes, s));
    const unsigned pix_grid = pixel_grid(c, npix);
    return run_batches(c, w, tune, base, npix, step, P->sample_offset + n_from, nullptr, s, log, [&](rtw_ctx::Lane& L, size_t Sb, size_t s0) {
        hipLaunchKernelGGL(k_accum_resolve_samples, dim3(pix_grid), dim3(kBlock), 0, s, L.lbuf.as<const float4>(), (uint32_t)npix, (uint32_t)Sb,
                           (uint32_t)(n_from + (int)s0), A.accum, A.upart, A.part, A.mom);
    });
}

// one device (a group's first): one add, its counts and times
int accum_add_single(rtw_ctx* c, int32_t spp, rtw_stats* stats) {
    rtw_ctx::Accum& A = c->acc;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t npix = A.npix;
    const Tuning tune = read_tuning();
    CallLog log{c, A.P.rng_kind, stats != nullptr && tune.kernel_timing};
    HIP_TRY(c, log.event(log.begin));
    HIP_TRY(c, log.event(log.end));
    const KArgs base = render_args(c, &A.P, npix);
    const bool use_path = path_pipeline(c->sc, A.P.width, A.P.height, A.P.max_depth, tune);
    const int n_from = A.done, n_to = A.done + spp;
    int rc = use_path ? accum_add_path(c, tune, base, n_from, n_to, s, log) : accum_add_wavefront(c, tune, base, n_from, n_to, s, log);
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(log.end, s));
    HIP_TRY(c, hipEventSynchronize(log.end));
    unsigned long long hs[8];
    if ((rc = sum_stat_rows(c, c->d_stats.as<unsigned long long>(), hs)) != RTW_OK) return rc;
    const uint64_t samples = (uint64_t)npix * (uint64_t)spp, segments = hs[0] + log.culled_segments;
    if (stats && (rc = fill_stats(c, log, hs, samples, segments, stats)) != RTW_OK) return rc;
    A.done = n_to;
    A.samples += samples; A.segments += segments; A.shadow_rays += hs[1];
    return RTW_OK;
}

// the context that holds the session: a group's first kid
rtw_ctx* accum_ctx(rtw_ctx* c) { return c->kids.empty() ? c : c->kids[0]; }
// an error of the session's context, reported on the caller's
int accum_up(rtw_ctx* c, rtw_ctx* d, int rc) { return rc && d != c ? fail(c, rc, d->err) : rc; }

int impl_accum_begin(rtw_ctx* c, const rtw_params* P, uint32_t flags) {
    if (!c) return RTW_ERR_INVALID_ARG;
    if (!c->has_scene) return fail(c, RTW_ERR_NO_SCENE, "rtw_accum_begin before rtw_upload_scene");
    if (!P) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_begin: null params");
    if (const char* why = accum_check_params(*P, flags)) return fail(c, RTW_ERR_INVALID_ARG, std::string("rtw_accum_begin: ") + why);
    rtw_ctx* d = accum_ctx(c);
    if (d->acc.active) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_begin: a session is active (rtw_accum_end it first)");
    const size_t npix = shard_rows(P) * (size_t)P->width;
    if (npix == 0) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_begin: the shard has no rows");
    if (npix > 0xffffffffull / 2) return fail(c, RTW_ERR_UNSUPPORTED, "rtw_accum_begin: tile too large");
    int rc = accum_alloc(d, npix, flags);
    if (rc == RTW_OK && hipStreamSynchronize(d->stream) != hipSuccess) rc = fail(d, RTW_ERR_DEVICE, "rtw_accum_begin: clearing the state failed");
    if (rc) { accum_free(d); return accum_up(c, d, rc); }
    d->acc.P = *P;
    d->acc.active = true;
    return RTW_OK;
}

int impl_accum_add(rtw_ctx* c, int32_t spp, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    if (stats) memset(stats, 0, sizeof *stats);
    if (!c->has_scene) return fail(c, RTW_ERR_NO_SCENE, "rtw_accum_add before rtw_upload_scene");
    rtw_ctx* d = accum_ctx(c);
    if (!d->acc.active) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_add: no active session");
    if (spp <= 0 || spp % (int)kSumBlock != 0) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_add: spp must be a positive multiple of RTW_SUM_BLOCK");
    if ((int64_t)d->acc.done + spp > (int64_t)d->acc.P.spp) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_add: more samples than the session's cap");
    const int rc = accum_add_single(d, spp, stats);
    if (rc) {  // some of the add may have reached the state: the session is not to be continued
        (void)hipStreamSynchronize(d->stream);
        (void)hipGetLastError();
        accum_free(d);
    }
    return accum_up(c, d, rc);
}

// the frame of the done samples into d_rgba on stream s (and the error map into the session's err); returns when it is written
int accum_read_single(rtw_ctx* c, float4* d_rgba, bool want_err, hipStream_t s) {
    const rtw_ctx::Accum& A = c->acc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!s) s = c->stream;
    const unsigned pix_grid = pixel_grid(c, A.npix);
    hipLaunchKernelGGL(k_accum_read, dim3(pix_grid), dim3(kBlock), 0, s, (const float4*)A.accum, (const float4*)A.upart, d_rgba, (uint32_t)A.npix, (float)A.done);
    if (want_err) hipLaunchKernelGGL(k_accum_error, dim3(pix_grid), dim3(kBlock), 0, s, (const double2*)A.mom, A.err, (uint32_t)A.npix, (uint32_t)A.done / kSumBlock);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(s));
    return RTW_OK;
}

int accum_read_check(rtw_ctx* c, rtw_ctx* d, const void* frame, bool want_err) {
    if (!d->acc.active) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_read: no active session");
    if (!frame) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_read: null output");
    if (d->acc.done <= 0) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_read: the session holds no samples yet");
    if (want_err && !d->acc.mom) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_read: the session was begun without RTW_ACCUM_ERROR");
    if (want_err && d->acc.done < 2 * (int)kSumBlock) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_read: the error map needs 2 * RTW_SUM_BLOCK samples");
    return RTW_OK;
}

int impl_accum_read_device(rtw_ctx* c, void* d_rgba, void* hip_stream) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_ctx* d = accum_ctx(c);
    int rc = accum_read_check(c, d, d_rgba, false);
    if (rc) return rc;
    return accum_up(c, d, accum_read_single(d, (float4*)d_rgba, false, (hipStream_t)hip_stream));
}

int impl_accum_read(rtw_ctx* c, float* rgba_out, float* error_out) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_ctx* d = accum_ctx(c);
    int rc = accum_read_check(c, d, rgba_out, error_out != nullptr);
    if (rc) return rc;
    const size_t npix = d->acc.npix;
    HIP_TRY(c, hipSetDevice(d->device));
    HIP_TRY(c, d->d_out.grow(npix, npix * sizeof(float4)));
    rc = accum_read_single(d, d->d_out.as<float4>(), error_out != nullptr, nullptr);
    if (rc) return accum_up(c, d, rc);
    HIP_TRY(c, hipMemcpy(rgba_out, d->d_out.as<void>(), npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (error_out) HIP_TRY(c, hipMemcpy(error_out, d->acc.err, npix * sizeof(float), hipMemcpyDeviceToHost));
    return RTW_OK;
}

int impl_accum_status(rtw_ctx* c, rtw_accum_info* out) {
    if (!c) return RTW_ERR_INVALID_ARG;
    if (!out) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_status: null output");
    memset(out, 0, sizeof *out);
    const rtw_ctx::Accum& A = accum_ctx(c)->acc;
    if (!A.active) return RTW_OK;
    out->active = 1; out->done = A.done; out->cap = A.P.spp; out->flags = A.flags;
    out->state_bytes = (uint64_t)accum_state_bytes(A.npix, A.flags);
    out->samples = A.samples; out->segments = A.segments; out->shadow_rays = A.shadow_rays;
    out->params = A.P;
    return RTW_OK;
}

int impl_accum_save(rtw_ctx* c, void* blob, size_t bytes) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_ctx* d = accum_ctx(c);
    const rtw_ctx::Accum& A = d->acc;
    if (!A.active) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_save: no active session");
    if (!blob || bytes != accum_state_bytes(A.npix, A.flags)) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_save: the blob must be state_bytes long");
    const AccumHeader h = accum_pack(A.P, A.flags, A.done, A.samples, A.segments, A.shadow_rays, c->scene_fp);
    memcpy(blob, &h, sizeof h);
    char* at = (char*)blob + sizeof h;
    const size_t arr = A.npix * 16;
    HIP_TRY(c, hipSetDevice(d->device));
    HIP_TRY(c, hipMemcpy(at, A.accum, arr, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(at + arr, A.upart, arr, hipMemcpyDeviceToHost));
    if (A.mom) HIP_TRY(c, hipMemcpy(at + 2 * arr, A.mom, arr, hipMemcpyDeviceToHost));
    return RTW_OK;
}

int impl_accum_restore(rtw_ctx* c, const void* blob, size_t bytes) {
    if (!c) return RTW_ERR_INVALID_ARG;
    if (!c->has_scene) return fail(c, RTW_ERR_NO_SCENE, "rtw_accum_restore before rtw_upload_scene");
    rtw_ctx* d = accum_ctx(c);
    if (d->acc.active) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_restore: a session is active (rtw_accum_end it first)");
    AccumHeader h;
    std::string why;
    if (!accum_validate(blob, bytes, c->scene_fp, h, why)) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_restore: " + why);
    const size_t npix = (size_t)h.npix;
    if (npix == 0) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_restore: the shard has no rows");
    if (npix > 0xffffffffull / 2) return fail(c, RTW_ERR_UNSUPPORTED, "rtw_accum_restore: tile too large");
    int rc = accum_alloc(d, npix, h.flags);
    if (rc) { accum_free(d); return accum_up(c, d, rc); }
    rtw_ctx::Accum& A = d->acc;
    const char* at = (const char*)blob + sizeof h;
    const size_t arr = npix * 16;
    hipError_t e = hipStreamSynchronize(d->stream);  // (the allocation's clear)
    if (e == hipSuccess) e = hipMemcpy(A.accum, at, arr, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(A.upart, at + arr, arr, hipMemcpyHostToDevice);
    if (e == hipSuccess && A.mom) e = hipMemcpy(A.mom, at + 2 * arr, arr, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        accum_free(d);
        return fail(c, RTW_ERR_DEVICE, std::string("rtw_accum_restore: ") + hipGetErrorString(e));
    }
    A.P = h.params; A.done = h.done;
    A.samples = h.samples; A.segments = h.segments; A.shadow_rays = h.shadow_rays;
    A.active = true;
    return RTW_OK;
}

int impl_accum_end(rtw_ctx* c) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_ctx* d = accum_ctx(c);
    if (!d->acc.active) return fail(c, RTW_ERR_INVALID_ARG, "rtw_accum_end: no active session");
    accum_free(d);
    return RTW_OK;
}

// rtw_denoise and rtw_denoise_guided on the context's device: the colour image (and the guides) in, `iterations` a-trous passes
// that ping-pong between two buffers, the result out. pass(grid, in, out, albedo, normal, step, inv_sigma2) issues one pass.
template <class Pass>
int denoise_passes(rtw_ctx* c, const char* what, const float* rgba_in, const float* albedo, const float* normal, float* rgba_out, int32_t width,
                   int32_t height, int32_t iterations, float sigma, Pass&& pass) {
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)width * height * sizeof(float4);
    const float* src[4] = {rgba_in, nullptr, albedo, normal};
    const int n_buf = albedo ? 4 : 2;
    DevBuf buf[4];  // ping, pong, albedo, normal
    float4* d[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < n_buf; k++) {
        HIP_TRY(c, buf[k].grow(bytes, bytes));
        d[k] = buf[k].as<float4>();
    }
    hipError_t e = hipSuccess;
    for (int k = 0; k < n_buf && e == hipSuccess; k++)
        if (src[k]) e = hipMemcpyAsync(d[k], src[k], bytes, hipMemcpyHostToDevice, c->stream);
    const unsigned grid = pixel_grid(c, (size_t)width * height);
    int cur = 0;
    float s_i = sigma;
    for (int it = 0; it < iterations && e == hipSuccess; it++) {
        pass(grid, (const float4*)d[cur], d[cur ^ 1], (const float4*)d[2], (const float4*)d[3], 1 << it, 1.0f / (s_i * s_i));
        e = hipGetLastError();
        cur ^= 1;
        s_i = s_i * 0.5f;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(rgba_out, d[cur], bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, RTW_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return RTW_OK;
}

int impl_denoise(rtw_ctx* c, const float* rgba_in, float* rgba_out, int32_t width, int32_t height, int32_t iterations, float sigma) {
    if (!c) return RTW_ERR_INVALID_ARG;
    if (!rgba_in || !rgba_out || rgba_in == rgba_out || width <= 0 || height <= 0 || iterations < 1 || iterations > 8 || !(sigma > 0.f) ||
        (int64_t)width * height > (1 << 28))
        return fail(c, RTW_ERR_INVALID_ARG, "rtw_denoise: bad argument");
    return denoise_passes(c, "rtw_denoise", rgba_in, nullptr, nullptr, rgba_out, width, height, iterations, sigma,
                          [&](unsigned grid, const float4* in, float4* out, const float4*, const float4*, int step, float inv_s2) {
                              hipLaunchKernelGGL(k_atrous, dim3(grid), dim3(kBlock), 0, c->stream, in, out, (int)width, (int)height, step, inv_s2);
                          });
}

// rtw.h rtw_render_guides: one k_guides launch on the context's device (a group's: device_ids[0], with that device's copy of the scene)
int impl_render_guides(rtw_ctx* c, const rtw_params* P, const rtw_guides* G, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    int rc = check_render_args(c, P);
    if (rc) return rc;
    if (!G || (!G->albedo && !G->normal && !G->depth && !G->prim)) return fail(c, RTW_ERR_INVALID_ARG, "rtw_render_guides: no output buffer");
    rtw_ctx* d = c->kids.empty() ? c : c->kids[0];
    if (stats) memset(stats, 0, sizeof *stats);
    const size_t rows = shard_rows(P);
    const size_t npix = rows * (size_t)P->width;
    if (npix == 0) return RTW_OK;
    if (npix > 0xffffffffull / 2) return fail(c, RTW_ERR_UNSUPPORTED, "rtw_render_guides: tile too large");
    HIP_TRY(c, hipSetDevice(d->device));
    KArgs a = shard_args(d->sc, P, npix);  // the uploaded scene as it is: the reference's ray tmin whatever P->estimator says
    a.sample0 = (uint32_t)P->sample_offset;
    // one device allocation: albedo, normal (16 B per pixel each), depth, prim (4 B each), whichever were asked for
    const size_t sz[4] = {G->albedo ? npix * 16 : 0, G->normal ? npix * 16 : 0, G->depth ? npix * 4 : 0, G->prim ? npix * 4 : 0};
    size_t off[5] = {0};
    for (int k = 0; k < 4; k++) off[k + 1] = off[k] + ((sz[k] + 255) & ~(size_t)255);
    DevBuf buf;
    HIP_TRY(c, buf.grow(off[4], off[4]));
    char* const slab = buf.as<char>();
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t e = hipSuccess;
    GuideOut g;
    g.albedo = sz[0] ? (float4*)(slab + off[0]) : nullptr;
    g.normal = sz[1] ? (float4*)(slab + off[1]) : nullptr;
    g.depth = sz[2] ? (float*)(slab + off[2]) : nullptr;
    g.prim = sz[3] ? (int32_t*)(slab + off[3]) : nullptr;
    g.rng_kind = P->rng_kind;
    if (stats) {
        e = timing_events(d, ev);
        if (e == hipSuccess) e = hipEventRecord(ev[0], d->stream);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_guides, dim3(pixel_grid(d, npix)), dim3(kBlock), d->info.lds_bytes, d->stream, a, g);
        e = hipGetLastError();
    }
    if (e == hipSuccess && stats) e = hipEventRecord(ev[1], d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    void* dst[4] = {G->albedo, G->normal, G->depth, G->prim};
    for (int k = 0; k < 4 && e == hipSuccess; k++)
        if (sz[k]) e = hipMemcpy(dst[k], slab + off[k], sz[k], hipMemcpyDeviceToHost);
    if (e == hipSuccess && stats) {
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, ev[0], ev[1]);
        stats->samples = stats->segments = (uint64_t)npix * (uint64_t)P->spp;
        stats->seconds = ms * 1e-3;
    }
    if (e != hipSuccess) return fail(c, RTW_ERR_DEVICE, std::string("rtw_render_guides: ") + hipGetErrorString(e));
    return RTW_OK;
}

// rtw.h rtw_denoise_guided: rtw_denoise's passes with k_atrous_guided
int impl_denoise_guided(rtw_ctx* c, const float* rgba_in, const float* albedo, const float* normal, float* rgba_out, int32_t width, int32_t height,
                        int32_t iterations, float sigma, float sigma_albedo, float sigma_normal) {
    if (!c) return RTW_ERR_INVALID_ARG;
    const float inv_a = 1.0f / (sigma_albedo * sigma_albedo), inv_n = 1.0f / (sigma_normal * sigma_normal);
    if (!rgba_in || !albedo || !normal || !rgba_out || rgba_out == rgba_in || rgba_out == albedo || rgba_out == normal || width <= 0 ||
        height <= 0 || iterations < 1 || iterations > 8 || !(sigma > 0.f) || !(sigma_albedo > 0.f) || !(sigma_normal > 0.f) ||
        !std::isfinite(inv_a) || !std::isfinite(inv_n) || (int64_t)width * height > (1 << 28))
        return fail(c, RTW_ERR_INVALID_ARG, "rtw_denoise_guided: bad argument");
    return denoise_passes(c, "rtw_denoise_guided", rgba_in, albedo, normal, rgba_out, width, height, iterations, sigma,
                          [&](unsigned grid, const float4* in, float4* out, const float4* alb, const float4* nrm, int step, float inv_s2) {
                              hipLaunchKernelGGL(k_atrous_guided, dim3(grid), dim3(kBlock), 0, c->stream, in, alb, nrm, out, (int)width, (int)height, step,
                                                 inv_s2, inv_a, inv_n);
                          });
}

int impl_debug_intersect(rtw_ctx* c, const float* rays, const float* ray_time, const float* gather_time, int n, float* out_t, int32_t* out_prim) {
    if (!c) return RTW_ERR_INVALID_ARG;
    if (!c->has_scene) return fail(c, RTW_ERR_NO_SCENE, "no scene");
    if (n < 0 || (n > 0 && (!rays || !out_t || !out_prim))) return fail(c, RTW_ERR_INVALID_ARG, "bad arguments");
    if (n == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t words = (size_t)n * 4;  // the bytes of n floats or n int32
    DevBuf d_rays, d_rt, d_gt, d_t, d_p;  // (d_rt, d_gt: null unless given)
    HIP_TRY(c, d_rays.grow(8 * words, 8 * words));
    HIP_TRY(c, d_t.grow(words, words));
    HIP_TRY(c, d_p.grow(words, words));
    HIP_TRY(c, hipMemcpy(d_rays.as<void>(), rays, 8 * words, hipMemcpyHostToDevice));
    if (ray_time) { HIP_TRY(c, d_rt.grow(words, words)); HIP_TRY(c, hipMemcpy(d_rt.as<void>(), ray_time, words, hipMemcpyHostToDevice)); }
    if (gather_time) { HIP_TRY(c, d_gt.grow(words, words)); HIP_TRY(c, hipMemcpy(d_gt.as<void>(), gather_time, words, hipMemcpyHostToDevice)); }
    const size_t lds = c->info.lds_bytes;
    hipLaunchKernelGGL(k_debug_intersect, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), lds, c->stream, c->sc, d_rays.as<const float>(),
                       d_rt.as<const float>(), d_gt.as<const float>(), n, d_t.as<float>(), d_p.as<int32_t>(), (uint32_t)kBlock);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out_t, d_t.as<void>(), words, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(out_prim, d_p.as<void>(), words, hipMemcpyDeviceToHost));
    return RTW_OK;
}

// ---- rtw_cast / rtw_cast_device (rtw.h): the caller's rays through k_cast
typedef void (*CastKernel)(const DScene, const CastArgs);

// one persistent launch of n rays on stream s of device context d (device pointers): as many workgroups as the device holds at once
// (the occupancy query with the scene's dynamic LDS x the CU count), never more than the rays fill
hipError_t cast_launch(rtw_ctx* d, int32_t mode, const CastArgs& a, hipStream_t s) {
    const bool attr = a.material || a.normal || a.uv;
    const CastKernel k = mode == RTW_CAST_ANY ? k_cast<true, false> : attr ? k_cast<false, true> : k_cast<false, false>;
    const size_t lds = d->info.lds_bytes;
    // workgroups per CU: what the query admits (registers allow 6 or 7 of these 4-wave workgroups, a tree's LDS image up to 10), or
    // RTW_CAST_GRID_MULT (rtw_plan.h)
    const size_t per_cu = (size_t)path_wg_per_cu((const void*)k, lds, read_tuning().cast_grid_mult);
    const size_t grid = std::min<size_t>(((size_t)a.n + kBlock - 1) / kBlock, (size_t)d->n_cu * per_cu);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kBlock), lds, s, d->sc, a);
    return hipGetLastError();
}

// the checks the two variants share (c: the context the caller holds; a group's has_scene covers its devices)
int cast_check(rtw_ctx* c, const char* what, const float* rays, size_t n, int32_t mode, const rtw_hits* out) {
    if (!c->has_scene) return fail(c, RTW_ERR_NO_SCENE, std::string(what) + " before rtw_upload_scene");
    if (mode != RTW_CAST_CLOSEST && mode != RTW_CAST_ANY) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": bad mode");
    if (n > 0x7fffffffull) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": more than 2^31 - 1 rays");
    if (n == 0) return RTW_OK;
    if (!rays || !out) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": null rays or outputs");
    if (!out->t && !out->prim && !out->material && !out->normal && !out->uv) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": no output buffer");
    if (mode == RTW_CAST_ANY && (out->material || out->normal || out->uv))
        return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": RTW_CAST_ANY has no material, normal or uv");
    return RTW_OK;
}

// ---- the host scaffold of the query family (everything from here to rtw_views_adaptive): the buffers a context grows on demand, the
// scope of one call (device context, stream, the two timing events, the control words, the staging slab), the chunk loop of the host
// variants, the view records and the stats tail. What is specific to an entry point is its checks, what it stages and what it issues.

// One call of the family, from the last refusal to the return.
struct QueryCall {
    rtw_ctx* d = nullptr;     // the device context it runs on (a group's first device)
    hipStream_t s = nullptr;  // the caller's stream, or the context's
    hipEvent_t ev[2] = {};    // ev[0] before the first thing the call puts on s, ev[1] after the last launch
    char* stage = nullptr;    // the context's staging slab (host variants)
    bool ended = false;       // ev[1] is recorded and waited for (query_chunks does that)
};

// Opens a call on `hip_stream` (null: the context's own). stage_bytes: what the call needs of the staging slab (rtw_stage_plan.h), 0 for
// none; it is grown before anything is timed, and never while something reads it: every call that uses it returns synchronised.
// ctl: the call counts in d->rad_ctl (kStatRows rows of 8 counters, then the queue word), whose rows are zeroed on the stream.
// timed = false leaves ev[0] alone: the call only waits for ev[1].
int query_open(rtw_ctx* c, QueryCall& q, void* hip_stream, size_t stage_bytes, bool ctl, bool timed = true) {
    rtw_ctx* const d = q.d = c->kids.empty() ? c : c->kids[0];
    HIP_TRY(c, hipSetDevice(d->device));
    q.s = hip_stream ? (hipStream_t)hip_stream : d->stream;
    HIP_TRY(c, d->stage_slab.grow(stage_bytes, stage_bytes));
    q.stage = d->stage_slab.as<char>();
    HIP_TRY(c, timing_events(d, q.ev));
    if (ctl) HIP_TRY(c, d->rad_ctl.grow(kCtlBytes, kCtlBytes));
    if (timed) HIP_TRY(c, hipEventRecord(q.ev[0], q.s));
    if (ctl) HIP_TRY(c, hipMemsetAsync(d->rad_ctl.as<void>(), 0, kStatRows * 8 * sizeof(unsigned long long), q.s));
    return RTW_OK;
}

// Closes it: records ev[1] and waits for it, unless the chunk loop has done so; `seconds` (where not null) receives the device time
// between the two events.
int query_close(rtw_ctx* c, QueryCall& q, double* seconds) {
    if (!q.ended) {
        HIP_TRY(c, hipEventRecord(q.ev[1], q.s));
        HIP_TRY(c, hipEventSynchronize(q.ev[1]));
        q.ended = true;
    }
    if (seconds) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, q.ev[0], q.ev[1]));
        *seconds = (double)ms * 1e-3;
    }
    return RTW_OK;
}

// The host variants' loop over chunks of at most `chunk` of the call's n items, all through the one staging slab: upload(i0, m),
// issue(i0, m), ev[1] after the last chunk's issue, download(i0, m), and a wait, because the next chunk reuses the slab (and the
// caller's memory is his again when the call returns). Each callable returns an RTW code.
template <class Upload, class Issue, class Download>
int query_chunks(rtw_ctx* c, QueryCall& q, size_t n, size_t chunk, Upload upload, Issue issue, Download download) {
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        int rc;
        if ((rc = upload(i0, m)) != RTW_OK || (rc = issue(i0, m)) != RTW_OK) return rc;
        if (i0 + m >= n) HIP_TRY(c, hipEventRecord(q.ev[1], q.s));
        if ((rc = download(i0, m)) != RTW_OK) return rc;
        HIP_TRY(c, hipStreamSynchronize(q.s));
    }
    q.ended = true;
    return RTW_OK;
}
int no_upload(size_t, size_t) { return RTW_OK; }  // (the views: their records are uploaded once, before the loop)

// The view records of a host entry, which the host can read: `what` names the entry point.
int view_records_check(rtw_ctx* c, const char* what, const rtw_view* views, size_t n_views) {
    for (size_t v = 0; v < n_views; v++) {
        if (views[v].camera_type < RTW_CAM_PERSPECTIVE || views[v].camera_type > RTW_CAM_ORTHOGRAPHIC)
            return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": view " + std::to_string(v) + ": bad camera_type");
        if (views[v].reserved[0] != 0u || views[v].reserved[1] != 0u)
            return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": view " + std::to_string(v) + ": reserved must be 0");
    }
    return RTW_OK;
}
// ... and their copy to the context's record buffer, on the call's stream (after ev[0]: the upload is part of the call's time)
int view_records_upload(rtw_ctx* c, QueryCall& q, const rtw_view* views, size_t n_views) {
    const size_t bytes = n_views * sizeof(rtw_view);
    HIP_TRY(c, q.d->view_buf.grow(bytes, bytes));
    HIP_TRY(c, hipMemcpyAsync(q.d->view_buf.as<void>(), views, bytes, hipMemcpyHostToDevice, q.s));
    return RTW_OK;
}

// The stats tail of the calls that trace paths or occlusion rays: closes the call, then the samples taken, the counters of the rows
// (occlusion: every sample is one occlusion ray, nothing else is traced) and the device time.
int query_stats(rtw_ctx* c, QueryCall& q, rtw_stats* stats, uint64_t samples, bool occlusion) {
    double seconds = 0.0;
    int rc = query_close(c, q, stats ? &seconds : nullptr);
    if (rc != RTW_OK || !stats) return rc;
    memset(stats, 0, sizeof *stats);
    stats->samples = samples;
    if (occlusion) {
        stats->shadow_rays = samples;
    } else {
        unsigned long long hs[8];
        if ((rc = sum_stat_rows(c, q.d->rad_ctl.as<unsigned long long>(), hs)) != RTW_OK) return rc;
        stats->segments = hs[0]; stats->shadow_rays = hs[1];
        stats->algorithmic_bytes = 128ull * stats->segments + 32ull * stats->samples;
    }
    stats->seconds = seconds;
    return RTW_OK;
}

void cast_stats(rtw_stats* stats, size_t n, int32_t mode) {
    memset(stats, 0, sizeof *stats);
    (mode == RTW_CAST_ANY ? stats->shadow_rays : stats->segments) = (uint64_t)n;
}

int impl_cast_device(rtw_ctx* c, const float* rays, const float* ray_time, const float* gather_time, size_t n, int32_t mode, const rtw_hits* out,
                     void* hip_stream, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    int rc = cast_check(c, "rtw_cast_device", rays, n, mode, out);
    if (rc) return rc;
    if (n > 0 && (((uintptr_t)rays & 15) || ((uintptr_t)out->normal & 15) || ((uintptr_t)out->uv & 7)))
        return fail(c, RTW_ERR_INVALID_ARG, "rtw_cast_device: rays and normal must be 16-byte aligned, uv 8-byte aligned");
    if (stats) cast_stats(stats, n, mode);  // (after every refusal: a refused call leaves *stats alone)
    if (n == 0) return RTW_OK;
    QueryCall q;
    if ((rc = query_open(c, q, hip_stream, 0, false)) != RTW_OK) return rc;
    const CastArgs a{(const float4*)rays, ray_time, gather_time, (uint64_t)n, out->t, out->prim, out->material, (float4*)out->normal, (float2*)out->uv};
    HIP_TRY(c, cast_launch(q.d, mode, a, q.s));
    return query_close(c, q, stats ? &stats->seconds : nullptr);
}

int impl_cast(rtw_ctx* c, const float* rays, const float* ray_time, const float* gather_time, size_t n, int32_t mode, const rtw_hits* out,
              rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    int rc = cast_check(c, "rtw_cast", rays, n, mode, out);
    if (rc) return rc;
    if (stats) cast_stats(stats, n, mode);
    if (n == 0) return RTW_OK;
    const size_t chunk = std::min(n, read_tuning().cast_chunk);
    // staged per ray: 32 B of ray, the two times the caller gave, and those of the five outputs he wants (4 + 4 + 4 + 16 + 8 B)
    const uint64_t width[8] = {32, 4, 4, 4, 4, 4, 16, 8};
    void* const dst[5] = {out->t, out->prim, out->material, out->normal, out->uv};
    const bool want[8] = {true, ray_time != nullptr, gather_time != nullptr, dst[0] != nullptr, dst[1] != nullptr, dst[2] != nullptr, dst[3] != nullptr,
                          dst[4] != nullptr};
    const StagePlan st = stage_plan(chunk, 8, width, want);
    QueryCall q;
    if ((rc = query_open(c, q, nullptr, (size_t)st.bytes, false)) != RTW_OK) return rc;
    char* sec[8];
    for (int k = 0; k < 8; k++) sec[k] = want[k] ? q.stage + st.off[k] : nullptr;
    rc = query_chunks(
        c, q, n, chunk,
        [&](size_t i0, size_t m) -> int {
            HIP_TRY(c, hipMemcpyAsync(sec[0], rays + 8 * i0, m * 32, hipMemcpyHostToDevice, q.s));
            if (ray_time) HIP_TRY(c, hipMemcpyAsync(sec[1], ray_time + i0, m * 4, hipMemcpyHostToDevice, q.s));
            if (gather_time) HIP_TRY(c, hipMemcpyAsync(sec[2], gather_time + i0, m * 4, hipMemcpyHostToDevice, q.s));
            return RTW_OK;
        },
        [&](size_t, size_t m) -> int {
            const CastArgs a{(const float4*)sec[0], (const float*)sec[1], (const float*)sec[2], (uint64_t)m, (float*)sec[3],
                             (int32_t*)sec[4],      (int32_t*)sec[5],     (float4*)sec[6],      (float2*)sec[7]};
            HIP_TRY(c, cast_launch(q.d, mode, a, q.s));
            return RTW_OK;
        },
        [&](size_t i0, size_t m) -> int {
            for (int k = 0; k < 5; k++)
                if (dst[k]) HIP_TRY(c, hipMemcpyAsync((char*)dst[k] + i0 * width[3 + k], sec[3 + k], m * width[3 + k], hipMemcpyDeviceToHost, q.s));
            return RTW_OK;
        });
    if (rc != RTW_OK) return rc;
    return query_close(c, q, stats ? &stats->seconds : nullptr);
}

// ---- rtw_radiance / rtw_radiance_device and rtw_probe / rtw_probe_device (rtw.h): whole paths along the caller's rays through
// k_radiance, or from the caller's probes through k_probe / k_probe_occlusion, or from the caller's points through k_probe_sh
// (rtw_probe_sh / rtw_probe_sh_device), or from the caller's cameras through k_view (rtw_views / rtw_views_device: the "rays" are
// the pixels of the flattened (view, y, x) index). The families share everything on the host but the kernels and the size of a
// result: `query` says which one a call serves.
typedef void (*RadianceKernel)(const DScene, const RadianceArgs);
typedef void (*RadianceResolve)(const float4*, float4*, uint32_t, uint32_t, float);
typedef void (*OcclusionKernel)(const DScene, const OcclusionArgs);
constexpr int kQueryRadiance = -1;  // (else rtw_probe's mode: RTW_PROBE_IRRADIANCE or RTW_PROBE_OCCLUSION)
constexpr int kQueryProbeSh = -2;   // rtw_probe_sh: nine float4 per point
constexpr int kQueryViews = -3;     // rtw_views: d_rays holds the view records, n counts pixels
typedef void (*ViewKernel)(const DScene, const ViewArgs);
// what a views call adds to a query: the frame and the flattened pixel that ray 0 of the issue is
struct ViewFrame { int32_t width, height; uint64_t first; };
// float4 of one result: the output stride of a query
constexpr size_t query_stride(int query) { return query == kQueryProbeSh ? 9 : 1; }

// launch()'s rule for the family's shading kernels: the instantiation K_<generator, feature level> (0 hot, 1 cold features, 2 cold
// features + the mixture estimator) for a call's rng_kind and the scene's level
#define RTW_PICK_F(K_, R_, FEAT_) ((FEAT_) == 2 ? K_<R_, 2> : (FEAT_) == 1 ? K_<R_, 1> : K_<R_, 0>)
#define RTW_PICK(K_, RNG_, FEAT_) ((RNG_) == RTW_RNG_TEA_LCG ? RTW_PICK_F(K_, RTW_RNG_TEA_LCG, FEAT_) : RTW_PICK_F(K_, RTW_RNG_PHILOX, FEAT_))

// width, height, first and the exact divisions of a frame as view_split / view_raygen read them: what every ViewArgs of the family has
ViewArgs view_frame_args(const void* d_views, int32_t width, int32_t height, uint64_t first) {
    ViewArgs va{};
    va.rays = (const float4*)d_views;
    va.width = (uint32_t)width; va.height = (uint32_t)height; va.first = (uint32_t)first;
    magic_div(va.width, va.divw_m, va.divw_s1, va.divw_s2);
    magic_div(va.width * va.height, va.divf_m, va.divf_s1, va.divf_s2);
    return va;
}

// the checks the variants share (c: the context the caller holds; a group's has_scene covers its devices)
int radiance_check(rtw_ctx* c, const char* what, const float* rays, size_t n, const rtw_radiance_params* RP, const void* out) {
    if (!c->has_scene) return fail(c, RTW_ERR_NO_SCENE, std::string(what) + " before rtw_upload_scene");
    if (!RP) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": null params");
    if (RP->spp <= 0 || RP->max_depth < 0) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": bad spp or max_depth");
    if (RP->rng_kind != RTW_RNG_PHILOX && RP->rng_kind != RTW_RNG_TEA_LCG) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": bad rng_kind");
    if (RP->estimator < RTW_EST_REFERENCE || RP->estimator > RTW_EST_MIXTURE) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": bad estimator");
    if (RP->sample_offset < 0 || (int64_t)RP->sample_offset + (int64_t)RP->spp > (int64_t)INT32_MAX)
        return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": sample_offset + spp beyond INT32_MAX");
    if (RP->reserved != 0u) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": reserved must be 0");
    if (n > 0x7fffffffull) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": more than 2^31 - 1 rays");
    if (n > 0 && (!rays || !out)) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": null rays or output");
    return RTW_OK;
}

// the context's unit slab, at least `need` bytes: grown after the stream's pending work, which may still read the old one
int radiance_slab(rtw_ctx* c, rtw_ctx* d, uint64_t need, hipStream_t s) {
    HIP_TRY(c, d->rad_slab.grow((size_t)need, (size_t)need, &s));
    return RTW_OK;
}

// RTW_PROBE_OCCLUSION: n probes at d_probes (device) -> their unoccluded fractions at d_out, issued on stream s and not waited for.
// One k_probe_occlusion launch per probe range; the ranges are rtw_radiance_plan.h's (the counts [unit][probe] of a call beyond 128
// spp take 4 of the 16 bytes the plan reserves per unit in the context's slab).
int occlusion_issue(rtw_ctx* c, rtw_ctx* d, const Tuning& tune, const float* d_probes, size_t n, const rtw_radiance_params* RP, uint32_t key_offset,
                    float4* d_out, hipStream_t s) {
    const OcclusionKernel k = RP->rng_kind == RTW_RNG_TEA_LCG ? k_probe_occlusion<RTW_RNG_TEA_LCG> : k_probe_occlusion<RTW_RNG_PHILOX>;
    const size_t lds = d->info.lds_bytes;
    const size_t per_cu = (size_t)path_wg_per_cu((const void*)k, lds, 0);
    const uint32_t units = radiance_units(RP->spp);
    const uint64_t per = radiance_range_rays(n, RP->spp, tune.radiance_slab_bytes);
    if (units > 1) {
        const int rc = radiance_slab(c, d, radiance_slab_bytes(per, RP->spp), s);
        if (rc != RTW_OK) return rc;
    }
    for (uint64_t r = 0, nr = radiance_n_ranges(n, per); r < nr; r++) {
        const RadianceRange rg = radiance_range(n, per, r);
        OcclusionArgs a{};
        a.probes = (const float4*)d_probes + 2 * rg.first;
        a.out = d_out + rg.first;
        a.counts = d->rad_slab.as<uint32_t>();
        a.n = (uint32_t)rg.count; a.units_per_probe = units; a.n_units = (uint32_t)(rg.count * units);
        magic_div(a.n, a.divn_m, a.divn_s1, a.divn_s2);
        a.spp = (uint32_t)RP->spp; a.sample0 = (uint32_t)RP->sample_offset; a.seed = RP->seed;
        a.key0 = radiance_key(key_offset, rg.first);
        const size_t grid = std::min<size_t>(((size_t)a.n_units + kBlock - 1) / kBlock, (size_t)d->n_cu * per_cu);
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kBlock), lds, s, d->sc, a);
        HIP_TRY(c, hipGetLastError());
        if (units > 1) {
            hipLaunchKernelGGL(k_probe_occlusion_resolve, dim3(pixel_grid(d, rg.count)), dim3(kBlock), 0, s, d->rad_slab.as<const uint32_t>(), d_out + rg.first, a.n,
                               units, (float)RP->spp);
            HIP_TRY(c, hipGetLastError());
        }
    }
    return RTW_OK;
}

// n rays (or probes) at d_rays (device) -> their means at d_out, issued on stream s of device context d and not waited for: one
// k_radiance (k_probe) launch per ray range (rtw_radiance_plan.h: all the rays unless the unit-sum slab would pass its cap), ray i on
// the stream of key_offset + i. The counters add up in d->rad_ctl's rows, which the caller zeroed on s. A result is `stride` float4
// (query_stride: nine for rtw_probe_sh, whose slab and ranges are the plan's 144-byte variants). kQueryViews: d_rays holds the view
// records of the whole call and ray i is flattened pixel vf->first + i (k_view; keys and seeds come from the pixel, not from here).
int radiance_issue(rtw_ctx* c, rtw_ctx* d, const Tuning& tune, const float* d_rays, size_t n, const rtw_radiance_params* RP, uint32_t key_offset,
                   float4* d_out, hipStream_t s, int query, const ViewFrame* vf = nullptr) {
    if (query == RTW_PROBE_OCCLUSION) return occlusion_issue(c, d, tune, d_rays, n, RP, key_offset, d_out, s);
    uint32_t* const queue = (uint32_t*)(d->rad_ctl.as<unsigned long long>() + kStatRows * 8);
    const bool sh = query == kQueryProbeSh;
    const size_t stride = query_stride(query);
    if (RP->max_depth == 0 && sh) {  // no segment is traced: every coefficient is 0 (n <= 2^31 - 1: the launch goes by ranges as well)
        const uint64_t per = probe_sh_range_points(n, 1, 0);
        for (uint64_t r = 0, nr = radiance_n_ranges(n, per); r < nr; r++) {
            const RadianceRange rg = radiance_range(n, per, r);
            hipLaunchKernelGGL(k_probe_sh_resolve, dim3(pixel_grid(d, rg.count * stride)), dim3(kBlock), 0, s, (const float4*)nullptr, d_out + rg.first * stride,
                               (uint32_t)rg.count, 0u, (float)RP->spp);
            HIP_TRY(c, hipGetLastError());
        }
        return RTW_OK;
    }
    if (RP->max_depth == 0) {  // no segment is traced: every mean is 0
        hipLaunchKernelGGL(k_radiance_resolve, dim3(pixel_grid(d, n)), dim3(kBlock), 0, s, (const float4*)nullptr, d_out, (uint32_t)n, 0u, (float)RP->spp);
        HIP_TRY(c, hipGetLastError());
        return RTW_OK;
    }
    DScene sc = d->sc;
    apply_estimator(sc, RP->estimator);
    const bool probe = query == RTW_PROBE_IRRADIANCE;
    const bool views = query == kQueryViews;
    const RadianceKernel k = sh      ? RTW_PICK(k_probe_sh, RP->rng_kind, sc.has_tex)
                             : probe ? RTW_PICK(k_probe, RP->rng_kind, sc.has_tex)
                                     : RTW_PICK(k_radiance, RP->rng_kind, sc.has_tex);
    const ViewKernel kv = RTW_PICK(k_view, RP->rng_kind, sc.has_tex);
    const RadianceResolve resolve = sh ? k_probe_sh_resolve : probe ? k_probe_resolve : k_radiance_resolve;
    const size_t lds = d->info.lds_bytes;
    const size_t per_cu = (size_t)path_wg_per_cu(views ? (const void*)kv : (const void*)k, lds, 0);
    const uint32_t units = radiance_units(RP->spp);
    const uint64_t per = sh ? probe_sh_range_points(n, RP->spp, tune.radiance_slab_bytes) : radiance_range_rays(n, RP->spp, tune.radiance_slab_bytes);
    if (units > 1) {
        const int rc = radiance_slab(c, d, sh ? probe_sh_slab_bytes(per, RP->spp) : radiance_slab_bytes(per, RP->spp), s);
        if (rc != RTW_OK) return rc;
    }
    for (uint64_t r = 0, nr = radiance_n_ranges(n, per); r < nr; r++) {
        const RadianceRange rg = radiance_range(n, per, r);
        RadianceArgs a{};
        a.rays = views ? (const float4*)d_rays : (const float4*)d_rays + 2 * rg.first;
        a.out = units > 1 ? d->rad_slab.as<float4>() : d_out + rg.first * stride;
        a.queue = queue;
        a.stats = d->rad_ctl.as<unsigned long long>();
        a.n = (uint32_t)rg.count; a.units_per_ray = units; a.n_units = (uint32_t)(rg.count * units);
        const size_t grid = std::min<size_t>(((size_t)a.n_units + kBlock - 1) / kBlock, (size_t)d->n_cu * per_cu);
        a.job_units = radiance_job_units(RP->spp, a.n_units, grid * (kBlock / 64));
        a.n_jobs = (uint32_t)radiance_n_jobs(a.n_units, a.job_units);
        magic_div(a.n, a.divn_m, a.divn_s1, a.divn_s2);
        a.spp = (uint32_t)RP->spp; a.sample0 = (uint32_t)RP->sample_offset; a.seed = RP->seed; a.max_depth = (uint32_t)RP->max_depth;
        a.key0 = radiance_key(key_offset, rg.first);
        HIP_TRY(c, hipMemsetAsync(queue, 0, sizeof(uint32_t), s));
        if (views) {
            ViewArgs va = view_frame_args(a.rays, vf->width, vf->height, vf->first + rg.first);
            va.out = a.out; va.queue = a.queue; va.stats = a.stats;
            va.n = a.n; va.units_per_ray = a.units_per_ray; va.n_units = a.n_units; va.job_units = a.job_units; va.n_jobs = a.n_jobs;
            va.divn_m = a.divn_m; va.divn_s1 = a.divn_s1; va.divn_s2 = a.divn_s2;
            va.spp = a.spp; va.sample0 = a.sample0; va.max_depth = a.max_depth;
            hipLaunchKernelGGL(kv, dim3((unsigned)grid), dim3(kBlock), lds, s, sc, va);
        } else {
            hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kBlock), lds, s, sc, a);
        }
        HIP_TRY(c, hipGetLastError());
        if (units > 1) {
            hipLaunchKernelGGL(resolve, dim3(pixel_grid(d, rg.count * stride)), dim3(kBlock), 0, s, d->rad_slab.as<const float4>(), d_out + rg.first * stride, a.n, units,
                               (float)RP->spp);
            HIP_TRY(c, hipGetLastError());
        }
    }
    return RTW_OK;
}

// the device variant of either family: `what` names the entry point in messages
int query_device(rtw_ctx* c, const char* what, const float* rays, size_t n, const rtw_radiance_params* RP, void* d_rgba, void* hip_stream,
                 rtw_stats* stats, int query) {
    int rc = radiance_check(c, what, rays, n, RP, d_rgba);
    if (rc) return rc;
    if (n > 0 && (((uintptr_t)rays & 15) || ((uintptr_t)d_rgba & 15)))
        return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": rays and the output must be 16-byte aligned");
    if (stats) memset(stats, 0, sizeof *stats);  // (after every refusal: a refused call leaves *stats alone)
    if (n == 0) return RTW_OK;
    QueryCall q;
    if ((rc = query_open(c, q, hip_stream, 0, true)) != RTW_OK) return rc;
    if ((rc = radiance_issue(c, q.d, read_tuning(), rays, n, RP, RP->key_offset, (float4*)d_rgba, q.s, query)) != RTW_OK) return rc;
    return query_stats(c, q, stats, (uint64_t)n * (uint64_t)RP->spp, query == RTW_PROBE_OCCLUSION);
}

// the host variant of either family
int query_host(rtw_ctx* c, const char* what, const float* rays, size_t n, const rtw_radiance_params* RP, float* rgba_out, rtw_stats* stats, int query) {
    int rc = radiance_check(c, what, rays, n, RP, rgba_out);
    if (rc) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n == 0) return RTW_OK;
    const Tuning tune = read_tuning();
    const size_t chunk = std::min(n, tune.radiance_chunk);
    // staged per ray: 32 B of ray and 16 B of result per float4 of the query's stride
    const size_t stride = query_stride(query);
    const uint64_t width[2] = {32, 16 * stride};
    const bool want[2] = {true, true};
    const StagePlan st = stage_plan(chunk, 2, width, want);
    QueryCall q;
    if ((rc = query_open(c, q, nullptr, (size_t)st.bytes, true)) != RTW_OK) return rc;
    float* const st_rays = (float*)(q.stage + st.off[0]);
    float4* const st_out = (float4*)(q.stage + st.off[1]);
    rc = query_chunks(
        c, q, n, chunk,
        [&](size_t i0, size_t m) -> int {
            HIP_TRY(c, hipMemcpyAsync(st_rays, rays + 8 * i0, m * 32, hipMemcpyHostToDevice, q.s));
            return RTW_OK;
        },
        // chunk c runs with the key of its first ray: the bits do not depend on the chunk size
        [&](size_t i0, size_t m) { return radiance_issue(c, q.d, tune, st_rays, m, RP, radiance_key(RP->key_offset, i0), st_out, q.s, query); },
        [&](size_t i0, size_t m) -> int {
            HIP_TRY(c, hipMemcpyAsync(rgba_out + 4 * stride * i0, st_out, m * 16 * stride, hipMemcpyDeviceToHost, q.s));
            return RTW_OK;
        });
    if (rc != RTW_OK) return rc;
    return query_stats(c, q, stats, (uint64_t)n * (uint64_t)RP->spp, query == RTW_PROBE_OCCLUSION);
}

int impl_radiance_device(rtw_ctx* c, const float* rays, size_t n, const rtw_radiance_params* RP, void* d_rgba, void* hip_stream, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    return query_device(c, "rtw_radiance_device", rays, n, RP, d_rgba, hip_stream, stats, kQueryRadiance);
}

int impl_radiance(rtw_ctx* c, const float* rays, size_t n, const rtw_radiance_params* RP, float* rgba_out, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    return query_host(c, "rtw_radiance", rays, n, RP, rgba_out, stats, kQueryRadiance);
}

// rtw_probe_params is rtw_radiance_params with the mode in the reserved word's place: the sampling fields go through
// rtw_radiance's checks as they are, the mode through its own
static_assert(sizeof(rtw_probe_params) == sizeof(rtw_radiance_params) && offsetof(rtw_probe_params, mode) == offsetof(rtw_radiance_params, reserved),
              "rtw_probe_params mirrors rtw_radiance_params");
const rtw_radiance_params* probe_sampling(const rtw_probe_params* PP, rtw_radiance_params& rp) {
    if (!PP) return nullptr;
    memcpy(&rp, PP, sizeof rp);
    rp.reserved = 0u;
    return &rp;
}
bool probe_mode_ok(const rtw_probe_params* PP) { return !PP || PP->mode == RTW_PROBE_IRRADIANCE || PP->mode == RTW_PROBE_OCCLUSION; }

int impl_probe_device(rtw_ctx* c, const float* probes, size_t n, const rtw_probe_params* PP, void* d_rgba, void* hip_stream, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    if (c->has_scene && !probe_mode_ok(PP)) return fail(c, RTW_ERR_INVALID_ARG, "rtw_probe_device: bad mode");
    rtw_radiance_params rp;
    return query_device(c, "rtw_probe_device", probes, n, probe_sampling(PP, rp), d_rgba, hip_stream, stats, PP ? PP->mode : 0);
}

int impl_probe(rtw_ctx* c, const float* probes, size_t n, const rtw_probe_params* PP, float* rgba_out, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    if (c->has_scene && !probe_mode_ok(PP)) return fail(c, RTW_ERR_INVALID_ARG, "rtw_probe: bad mode");
    rtw_radiance_params rp;
    return query_host(c, "rtw_probe", probes, n, probe_sampling(PP, rp), rgba_out, stats, PP ? PP->mode : 0);
}

// rtw_probe_sh takes rtw_radiance's params as they are (reserved == 0 included)
int impl_sh_probe_device(rtw_ctx* c, const float* points, size_t n, const rtw_radiance_params* RP, void* d_sh, void* hip_stream, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    return query_device(c, "rtw_probe_sh_device", points, n, RP, d_sh, hip_stream, stats, kQueryProbeSh);
}

int impl_sh_probe(rtw_ctx* c, const float* points, size_t n, const rtw_radiance_params* RP, float* sh_out, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    return query_host(c, "rtw_probe_sh", points, n, RP, sh_out, stats, kQueryProbeSh);
}

// ---- rtw_views / rtw_views_device (rtw.h): a radiance query whose rays are the pixels of the call's frames
static_assert(sizeof(rtw_view) == 112 && sizeof(rtw_view_params) == 32, "rtw.h states these sizes");

int views_check(rtw_ctx* c, const char* what, const rtw_view* views, size_t n_views, const rtw_view_params* VP, const void* out, rtw_radiance_params& rp) {
    if (!c->has_scene) return fail(c, RTW_ERR_NO_SCENE, std::string(what) + " before rtw_upload_scene");
    if (!VP) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": null params");
    if (VP->width <= 0 || VP->height <= 0) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": bad width or height");
    rp = rtw_radiance_params{VP->spp, VP->max_depth, 0u, VP->rng_kind, VP->sample_offset, VP->estimator, 0u, VP->reserved};
    const int rc = radiance_check(c, what, nullptr, 0, &rp, nullptr);  // the sampling fields; the count and the pointers are checked here
    if (rc) return rc;
    if (!view_pixels_ok(n_views, VP->width, VP->height)) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": more than 2^31 - 1 pixels");
    if (n_views > 0 && (!views || !out)) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": null views or output");
    return RTW_OK;
}

int impl_views_device(rtw_ctx* c, const rtw_view* d_views, size_t n_views, const rtw_view_params* VP, void* d_rgba, void* hip_stream, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_radiance_params rp;
    int rc = views_check(c, "rtw_views_device", d_views, n_views, VP, d_rgba, rp);
    if (rc) return rc;
    if (n_views > 0 && (((uintptr_t)d_views & 15) || ((uintptr_t)d_rgba & 15)))
        return fail(c, RTW_ERR_INVALID_ARG, "rtw_views_device: views and the output must be 16-byte aligned");
    if (stats) memset(stats, 0, sizeof *stats);  // (after every refusal: a refused call leaves *stats alone)
    if (n_views == 0) return RTW_OK;
    const size_t n = (size_t)view_pixels(n_views, VP->width, VP->height);
    QueryCall q;
    if ((rc = query_open(c, q, hip_stream, 0, true)) != RTW_OK) return rc;
    const ViewFrame vf{VP->width, VP->height, 0};
    if ((rc = radiance_issue(c, q.d, read_tuning(), (const float*)d_views, n, &rp, 0u, (float4*)d_rgba, q.s, kQueryViews, &vf)) != RTW_OK) return rc;
    return query_stats(c, q, stats, (uint64_t)n * (uint64_t)rp.spp, false);
}

int impl_views(rtw_ctx* c, const rtw_view* views, size_t n_views, const rtw_view_params* VP, float* rgba_out, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_radiance_params rp;
    int rc = views_check(c, "rtw_views", views, n_views, VP, rgba_out, rp);
    if (rc || (rc = view_records_check(c, "rtw_views", views, n_views))) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_views == 0) return RTW_OK;
    const size_t n = (size_t)view_pixels(n_views, VP->width, VP->height);
    const Tuning tune = read_tuning();
    const size_t chunk = std::min(n, tune.radiance_chunk);
    const uint64_t width[1] = {16};  // staged: a chunk's results alone
    const bool want[1] = {true};
    QueryCall q;
    if ((rc = query_open(c, q, nullptr, (size_t)stage_plan(chunk, 1, width, want).bytes, true)) != RTW_OK) return rc;
    if ((rc = view_records_upload(c, q, views, n_views)) != RTW_OK) return rc;
    float4* const st_out = (float4*)q.stage;
    rc = query_chunks(
        c, q, n, chunk, no_upload,
        [&](size_t i0, size_t m) {  // a chunk may begin and end mid-row and mid-view: a pixel knows its own index
            const ViewFrame vf{VP->width, VP->height, (uint64_t)i0};
            return radiance_issue(c, q.d, tune, q.d->view_buf.as<const float>(), m, &rp, 0u, st_out, q.s, kQueryViews, &vf);
        },
        [&](size_t i0, size_t m) -> int {
            HIP_TRY(c, hipMemcpyAsync(rgba_out + 4 * i0, st_out, m * 16, hipMemcpyDeviceToHost, q.s));
            return RTW_OK;
        });
    if (rc != RTW_OK) return rc;
    return query_stats(c, q, stats, (uint64_t)n * (uint64_t)rp.spp, false);
}

// ---- rtw_views_guides / rtw_views_guides_device (rtw.h): k_guides' pass over the pixels of the call's frames, the camera from the
// pixel's view record (k_view_guides)
int views_guides_check(rtw_ctx* c, const char* what, const rtw_view* views, size_t n_views, const rtw_view_params* VP, const rtw_guides* G) {
    rtw_radiance_params rp;
    static const char some = 0;  // views_check's null test of the output is made here, on the struct
    const int rc = views_check(c, what, views, n_views, VP, &some, rp);
    if (rc) return rc;
    if (!G || (!G->albedo && !G->normal && !G->depth && !G->prim)) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": no output buffer");
    return RTW_OK;
}

// one k_view_guides launch on stream s of device context d: n flattened pixels from pixel `first` of the call, entry i of g's
// buffers pixel first + i; the scene as uploaded (the reference's ray tmin whatever VP->estimator says)
hipError_t views_guides_launch(rtw_ctx* d, const void* d_views, const rtw_view_params* VP, uint64_t first, size_t n, const GuideOut& g, hipStream_t s) {
    ViewArgs va = view_frame_args(d_views, VP->width, VP->height, first);
    va.n = (uint32_t)n;
    va.spp = (uint32_t)VP->spp; va.sample0 = (uint32_t)VP->sample_offset;
    hipLaunchKernelGGL(k_view_guides, dim3(pixel_grid(d, n)), dim3(kBlock), d->info.lds_bytes, s, d->sc, va, g);
    return hipGetLastError();
}

// closes the call; its stats where they are wanted
int views_guides_close(rtw_ctx* c, QueryCall& q, rtw_stats* stats, size_t n, const rtw_view_params* VP) {
    const int rc = query_close(c, q, stats ? &stats->seconds : nullptr);
    if (rc == RTW_OK && stats) stats->samples = stats->segments = (uint64_t)n * (uint64_t)VP->spp;  // one camera segment per sample
    return rc;
}

int impl_views_guides_device(rtw_ctx* c, const rtw_view* d_views, size_t n_views, const rtw_view_params* VP, const rtw_guides* G, void* hip_stream,
                             rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    int rc = views_guides_check(c, "rtw_views_guides_device", d_views, n_views, VP, G);
    if (rc) return rc;
    if (n_views > 0 && (((uintptr_t)d_views & 15) || ((uintptr_t)G->albedo & 15) || ((uintptr_t)G->normal & 15) || ((uintptr_t)G->depth & 3) ||
                        ((uintptr_t)G->prim & 3)))
        return fail(c, RTW_ERR_INVALID_ARG, "rtw_views_guides_device: views, albedo and normal must be 16-byte aligned, depth and prim 4-byte aligned");
    if (stats) memset(stats, 0, sizeof *stats);  // (after every refusal: a refused call leaves *stats alone)
    if (n_views == 0) return RTW_OK;
    const size_t n = (size_t)view_pixels(n_views, VP->width, VP->height);
    QueryCall q;
    if ((rc = query_open(c, q, hip_stream, 0, false)) != RTW_OK) return rc;
    const GuideOut g{(float4*)G->albedo, (float4*)G->normal, G->depth, G->prim, VP->rng_kind};
    HIP_TRY(c, views_guides_launch(q.d, d_views, VP, 0, n, g, q.s));
    return views_guides_close(c, q, stats, n, VP);
}

int impl_views_guides(rtw_ctx* c, const rtw_view* views, size_t n_views, const rtw_view_params* VP, const rtw_guides* G, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    int rc = views_guides_check(c, "rtw_views_guides", views, n_views, VP, G);
    if (rc || (rc = view_records_check(c, "rtw_views_guides", views, n_views))) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_views == 0) return RTW_OK;
    const size_t n = (size_t)view_pixels(n_views, VP->width, VP->height);
    const size_t chunk = (size_t)view_guides_chunk(n, read_tuning().radiance_chunk);
    void* const dst[4] = {G->albedo, G->normal, G->depth, G->prim};
    const bool want[4] = {G->albedo != nullptr, G->normal != nullptr, G->depth != nullptr, G->prim != nullptr};
    const ViewGuideStage stage = view_guides_stage(chunk, want);  // staged: a chunk's requested guides alone
    QueryCall q;
    if ((rc = query_open(c, q, nullptr, (size_t)stage.bytes, false)) != RTW_OK) return rc;
    if ((rc = view_records_upload(c, q, views, n_views)) != RTW_OK) return rc;
    char* const st = q.stage;
    const GuideOut g{want[0] ? (float4*)(st + stage.off[0]) : nullptr, want[1] ? (float4*)(st + stage.off[1]) : nullptr,
                     want[2] ? (float*)(st + stage.off[2]) : nullptr, want[3] ? (int32_t*)(st + stage.off[3]) : nullptr, VP->rng_kind};
    rc = query_chunks(
        c, q, n, chunk, no_upload,
        [&](size_t i0, size_t m) -> int {  // a chunk may begin and end mid-row and mid-view: a pixel knows its own index
            HIP_TRY(c, views_guides_launch(q.d, q.d->view_buf.as<void>(), VP, (uint64_t)i0, m, g, q.s));
            return RTW_OK;
        },
        [&](size_t i0, size_t m) -> int {
            for (int k = 0; k < 4; k++)
                if (want[k])
                    HIP_TRY(c, hipMemcpyAsync((char*)dst[k] + i0 * kGuideEntryBytes[k], st + stage.off[k], m * kGuideEntryBytes[k], hipMemcpyDeviceToHost, q.s));
            return RTW_OK;
        });
    if (rc != RTW_OK) return rc;
    return views_guides_close(c, q, stats, n, VP);
}

// ---- rtw_denoise_views / rtw_denoise_views_device (rtw.h): rtw_denoise_guided's passes over all frames at once (k_atrous_guided_views)
int denoise_views_check(rtw_ctx* c, const char* what, const float* rgba_in, const float* albedo, const float* normal, float* rgba_out, size_t n_views,
                        int32_t width, int32_t height, int32_t iterations, float sigma, float sigma_albedo, float sigma_normal) {
    const float inv_a = 1.0f / (sigma_albedo * sigma_albedo), inv_n = 1.0f / (sigma_normal * sigma_normal);
    if (width <= 0 || height <= 0 || iterations < 1 || iterations > 8 || !(sigma > 0.f) || !(sigma_albedo > 0.f) || !(sigma_normal > 0.f) ||
        !std::isfinite(inv_a) || !std::isfinite(inv_n) || !denoise_views_frame_ok(width, height))
        return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": bad argument");
    if (!view_pixels_ok(n_views, width, height)) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": more than 2^31 - 1 pixels");
    if (n_views > 0 && (!rgba_in || !albedo || !normal || !rgba_out || rgba_out == rgba_in || rgba_out == albedo || rgba_out == normal))
        return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": a null buffer, or an output that is an input");
    // an output that begins inside an input, or an input inside the output, is an alias as well
    const uintptr_t o0 = (uintptr_t)rgba_out, bytes = (uintptr_t)view_pixels(n_views, width, height) * 16u;
    for (const float* p : {rgba_in, albedo, normal})
        if (n_views > 0 && o0 < (uintptr_t)p + bytes && (uintptr_t)p < o0 + bytes)
            return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": the output overlaps an input");
    return RTW_OK;
}

// the context's denoiser scratch, at least `need` bytes: grown after the stream's pending work, which may still read the old one
int denoise_views_scratch(rtw_ctx* c, rtw_ctx* d, uint64_t need, hipStream_t s) {
    if (need <= d->dn_buf.cap()) return RTW_OK;
    HIP_TRY(c, hipStreamSynchronize(s));
    if (d->dn_buf.grow((size_t)need, (size_t)need) != hipSuccess)
        return fail(c, RTW_ERR_OOM, "rtw_denoise_views: device allocation failed");
    return RTW_OK;
}

// the passes on stream s, not waited for: device buffers of n pixels, `scratch` one more (unused by a single pass)
hipError_t denoise_views_issue(rtw_ctx* d, const float4* in, const float4* alb, const float4* nrm, float4* out, float4* scratch, size_t n, int32_t width,
                               int32_t height, int32_t iterations, float sigma, float sigma_albedo, float sigma_normal, hipStream_t s) {
    const float inv_a = 1.0f / (sigma_albedo * sigma_albedo), inv_n = 1.0f / (sigma_normal * sigma_normal);
    uint32_t fm, f1, f2;
    magic_div((uint32_t)width * (uint32_t)height, fm, f1, f2);
    const unsigned grid = pixel_grid(d, n);
    const float4* src = in;
    float s_i = sigma;
    for (int it = 0; it < iterations; it++) {
        float4* const dst = denoise_views_writes_output(iterations, it) ? out : scratch;
        hipLaunchKernelGGL(k_atrous_guided_views, dim3(grid), dim3(kBlock), 0, s, src, alb, nrm, dst, (uint32_t)n, (int)width, (int)height, fm, f1, f2, 1 << it,
                           1.0f / (s_i * s_i), inv_a, inv_n);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        src = dst;
        s_i = s_i * 0.5f;
    }
    return hipSuccess;
}

int impl_denoise_views_device(rtw_ctx* c, const float* rgba_in, const float* albedo, const float* normal, float* rgba_out, size_t n_views, int32_t width,
                              int32_t height, int32_t iterations, float sigma, float sigma_albedo, float sigma_normal, void* hip_stream) {
    if (!c) return RTW_ERR_INVALID_ARG;
    int rc = denoise_views_check(c, "rtw_denoise_views_device", rgba_in, albedo, normal, rgba_out, n_views, width, height, iterations, sigma, sigma_albedo,
                                 sigma_normal);
    if (rc) return rc;
    if (n_views > 0 && (((uintptr_t)rgba_in & 15) || ((uintptr_t)albedo & 15) || ((uintptr_t)normal & 15) || ((uintptr_t)rgba_out & 15)))
        return fail(c, RTW_ERR_INVALID_ARG, "rtw_denoise_views_device: the buffers must be 16-byte aligned");
    if (n_views == 0) return RTW_OK;
    const size_t n = (size_t)view_pixels(n_views, width, height);
    QueryCall q;  // (untimed: ev[1] is the completion wait alone)
    if ((rc = query_open(c, q, hip_stream, 0, false, false)) != RTW_OK) return rc;
    if ((rc = denoise_views_scratch(c, q.d, denoise_views_scratch_bytes(n, iterations, false), q.s)) != RTW_OK) return rc;
    HIP_TRY(c, denoise_views_issue(q.d, (const float4*)rgba_in, (const float4*)albedo, (const float4*)normal, (float4*)rgba_out, q.d->dn_buf.as<float4>(), n,
                                   width, height, iterations, sigma, sigma_albedo, sigma_normal, q.s));
    return query_close(c, q, nullptr);
}

int impl_denoise_views(rtw_ctx* c, const float* rgba_in, const float* albedo, const float* normal, float* rgba_out, size_t n_views, int32_t width,
                       int32_t height, int32_t iterations, float sigma, float sigma_albedo, float sigma_normal) {
    if (!c) return RTW_ERR_INVALID_ARG;
    int rc = denoise_views_check(c, "rtw_denoise_views", rgba_in, albedo, normal, rgba_out, n_views, width, height, iterations, sigma, sigma_albedo, sigma_normal);
    if (rc) return rc;
    if (n_views == 0) return RTW_OK;
    const size_t n = (size_t)view_pixels(n_views, width, height);
    rtw_ctx* d = c->kids.empty() ? c : c->kids[0];
    HIP_TRY(c, hipSetDevice(d->device));
    if ((rc = denoise_views_scratch(c, d, denoise_views_scratch_bytes(n, iterations, true), d->stream)) != RTW_OK) return rc;
    const size_t each = (size_t)denoise_views_buffer_bytes(n);
    char* const b = d->dn_buf.as<char>();  // colour, albedo, normal, output, then the ping-pong buffer
    const float* const src[3] = {rgba_in, albedo, normal};
    for (int k = 0; k < 3; k++) HIP_TRY(c, hipMemcpyAsync(b + k * each, src[k], n * 16, hipMemcpyHostToDevice, d->stream));
    HIP_TRY(c, denoise_views_issue(d, (const float4*)b, (const float4*)(b + each), (const float4*)(b + 2 * each), (float4*)(b + 3 * each),
                                   (float4*)(b + 4 * each), n, width, height, iterations, sigma, sigma_albedo, sigma_normal, d->stream));
    HIP_TRY(c, hipMemcpyAsync(rgba_out, b + 3 * each, n * 16, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(c, hipStreamSynchronize(d->stream));
    return RTW_OK;
}

// ---- rtw_probe_adaptive / rtw_probe_adaptive_device (rtw.h): rtw_probe's samples taken from checkpoint to checkpoint over the list of
// the probes that are still active (rtw_probe_adaptive.h; the plan of a pass is rtw_probe_adaptive_plan.h's)
typedef void (*ProbeListKernel)(const DScene, const ProbeListArgs);

// One pass of rtw_probe_adaptive / rtw_views_adaptive, adaptive_run's `pass` for the list kernels: samples [n_from, n_to) of the
// n_active entries of `list` on stream s of device context d, cut into ranges of list positions that fit the slab cap
// (rtw_probe_adaptive_plan.h: runs, ranges, jobs), each range sampled into d->rad_slab and resolved from there. The counters add up
// in d->rad_ctl's rows, which the caller zeroed on s. What a family hands in: max_grid, the workgroups its sampling kernel keeps
// resident; zero_depth, no segment is traced and every block sum is 0; use_queue, the kernel takes its jobs from the queue word; and
//   sample(p, grid)                the sampling kernel over range p (rtw_list_body.h ListPass), block sums to p.out
//   resolve(list, count, nb, blk0) the block sums of a range into the listed entries' sums and moments
template <class Sample, class Resolve>
int list_pass(rtw_ctx* c, rtw_ctx* d, const Tuning& tune, size_t max_grid, bool zero_depth, bool use_queue, const uint32_t* list0, size_t n_active, int n_from,
              int n_to, hipStream_t s, Sample sample, Resolve resolve) {
    uint32_t* const queue = (uint32_t*)(d->rad_ctl.as<unsigned long long>() + kStatRows * 8);
    const uint32_t nb = probe_adaptive_pass_blocks(n_from, n_to), blk0 = probe_adaptive_first_block(n_from);
    const uint32_t run_blocks = probe_adaptive_run_blocks(n_active, nb, max_grid * kBlock);
    const uint32_t runs = probe_adaptive_runs(nb, run_blocks);
    const uint64_t per = probe_adaptive_range_positions(n_active, nb, run_blocks, tune.radiance_slab_bytes);
    int rc;
    if ((rc = radiance_slab(c, d, probe_adaptive_slab_bytes(per, nb), s)) != RTW_OK) return rc;
    for (uint64_t r = 0, nr = radiance_n_ranges(n_active, per); r < nr; r++) {
        const RadianceRange rg = radiance_range(n_active, per, r);
        const uint32_t* const list = list0 + rg.first;
        if (zero_depth) {
            HIP_TRY(c, hipMemsetAsync(d->rad_slab.as<void>(), 0, (size_t)probe_adaptive_slab_bytes(rg.count, nb), s));
        } else {
            ListPass p{};
            p.list = list;
            p.out = d->rad_slab.as<float4>();
            p.queue = queue;
            p.stats = d->rad_ctl.as<unsigned long long>();
            p.n = (uint32_t)rg.count; p.n_blocks = nb; p.run_blocks = run_blocks; p.n_units = (uint32_t)(rg.count * runs);
            const unsigned grid = (unsigned)std::min<size_t>(((size_t)p.n_units + kBlock - 1) / kBlock, max_grid);
            p.job_units = probe_adaptive_job_units(run_blocks, p.n_units, (size_t)grid * (kBlock / 64));
            p.n_jobs = (uint32_t)radiance_n_jobs(p.n_units, p.job_units);
            magic_div(p.n, p.divn_m, p.divn_s1, p.divn_s2);
            p.s_from = (uint32_t)n_from;
            if (use_queue) HIP_TRY(c, hipMemsetAsync(queue, 0, sizeof(uint32_t), s));
            sample(p, grid);
            HIP_TRY(c, hipGetLastError());
        }
        resolve(list, (uint32_t)rg.count, nb, blk0);
        HIP_TRY(c, hipGetLastError());
    }
    return RTW_OK;
}

// n probes at d_probes (device) -> their results at d_out (and d_spp, d_err where not null); probe i on the stream of key_offset + i.
// The family's loop over a frame of n x 1 probes with dilate 0; the state is the context's d->padapt, grown after the stream's
// pending work and kept until rtw_destroy.
int probe_adaptive_issue(rtw_ctx* c, rtw_ctx* d, const Tuning& tune, const float* d_probes, size_t n, const rtw_radiance_params* RP, int mode,
                         const rtw_adaptive* AD, const std::vector<int>& cps, uint32_t key_offset, float4* d_out, int32_t* d_spp, float* d_err,
                         hipStream_t s, uint64_t& samples) {
    const bool occ = mode == RTW_PROBE_OCCLUSION;
    DScene sc = d->sc;
    if (!occ) apply_estimator(sc, RP->estimator);
    const ProbeListKernel k = occ ? (RP->rng_kind == RTW_RNG_TEA_LCG ? k_probe_occlusion_list<RTW_RNG_TEA_LCG> : k_probe_occlusion_list<RTW_RNG_PHILOX>)
                                  : RTW_PICK(k_probe_list, RP->rng_kind, sc.has_tex);
    AdaptiveState st{};
    const int rc = adaptive_state(c, d->padapt, n, false, &s, st);
    if (rc) return rc;
    const size_t max_grid = (size_t)d->n_cu * (size_t)path_wg_per_cu((const void*)k, d->info.lds_bytes, 0);
    ProbeListArgs a{};
    a.probes = (const float4*)d_probes;
    a.sample0 = (uint32_t)RP->sample_offset; a.seed = RP->seed; a.max_depth = (uint32_t)RP->max_depth; a.key0 = key_offset;
    return adaptive_run(
        c, d, st, adaptive_frames((uint32_t)n, 1u, 1, AD->threshold, 0), cps, s, samples, nullptr, nullptr,
        [&](const uint32_t* list, size_t n_active, int n_from, int n_to) {
            return list_pass(
                c, d, tune, max_grid, !occ && RP->max_depth == 0, !occ, list, n_active, n_from, n_to, s,
                [&](const ListPass& p, unsigned grid) {
                    a.p = p;
                    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), d->info.lds_bytes, s, sc, a);
                },
                [&](const uint32_t* range, uint32_t count, uint32_t nb, uint32_t blk0) {
                    if (occ)
                        hipLaunchKernelGGL(k_probe_adapt_resolve_counts, dim3(pixel_grid(d, count)), dim3(kBlock), 0, s, d->rad_slab.as<const uint32_t>(), range, count,
                                           nb, st.total, st.mom);
                    else
                        hipLaunchKernelGGL(k_adapt_resolve_blocks, dim3(pixel_grid(d, count)), dim3(kBlock), 0, s, d->rad_slab.as<const float4>(), range, count, nb,
                                           blk0, st.accum, st.upart, st.mom);
                });
        },
        [&](unsigned grid) {
            if (occ)
                hipLaunchKernelGGL(k_probe_adapt_finish_occlusion, dim3(grid), dim3(kBlock), 0, s, (const uint32_t*)st.total, (const uint32_t*)st.n,
                                   (const float*)st.err, d_out, d_spp, d_err, (uint32_t)n);
            else  // (sum / (float)n_i) * pi
                hipLaunchKernelGGL(k_adapt_finish, dim3(grid), dim3(kBlock), 0, s, (const float4*)st.accum, (const float4*)st.upart, (const uint32_t*)st.n,
                                   (const float*)st.err, d_out, d_spp, d_err, (uint32_t)n, 1u);
        });
}

// the checks both variants share; fills the sampling params and the checkpoints
int probe_adaptive_check(rtw_ctx* c, const char* what, const float* probes, size_t n, const rtw_probe_params* PP, const rtw_adaptive* AD, const void* out,
                         rtw_radiance_params& rp, std::vector<int>& cps) {
    if (c->has_scene && !probe_mode_ok(PP)) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": bad mode");
    const int rc = radiance_check(c, what, probes, n, probe_sampling(PP, rp), out);
    if (rc) return rc;
    if (!AD) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": null adaptive settings");
    if (const char* why = adaptive_checkpoints(AD->min_spp, AD->step_spp, PP->spp, AD->threshold, AD->dilate, cps))
        return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": " + why);
    if (AD->dilate != 0) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": dilate must be 0 (a probe batch has no neighbourhood)");
    return RTW_OK;
}

int impl_adaptive_probe_device(rtw_ctx* c, const float* probes, size_t n, const rtw_probe_params* PP, const rtw_adaptive* AD, void* d_rgba, void* d_spp,
                               void* d_error, void* hip_stream, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_radiance_params rp;
    std::vector<int> cps;
    int rc = probe_adaptive_check(c, "rtw_probe_adaptive_device", probes, n, PP, AD, d_rgba, rp, cps);
    if (rc) return rc;
    if (n > 0 && (((uintptr_t)probes & 15) || ((uintptr_t)d_rgba & 15) || ((uintptr_t)d_spp & 3) || ((uintptr_t)d_error & 3)))
        return fail(c, RTW_ERR_INVALID_ARG, "rtw_probe_adaptive_device: probes and rgba must be 16-byte aligned, spp and error 4-byte aligned");
    if (stats) memset(stats, 0, sizeof *stats);  // (after every refusal: a refused call leaves *stats alone)
    if (n == 0) return RTW_OK;
    QueryCall q;
    if ((rc = query_open(c, q, hip_stream, 0, true)) != RTW_OK) return rc;
    uint64_t samples = 0;
    if ((rc = probe_adaptive_issue(c, q.d, read_tuning(), probes, n, &rp, PP->mode, AD, cps, rp.key_offset, (float4*)d_rgba, (int32_t*)d_spp, (float*)d_error,
                                   q.s, samples)) != RTW_OK)
        return rc;
    return query_stats(c, q, stats, samples, PP->mode == RTW_PROBE_OCCLUSION);
}

int impl_adaptive_probe(rtw_ctx* c, const float* probes, size_t n, const rtw_probe_params* PP, const rtw_adaptive* AD, float* rgba_out, int32_t* spp_out,
                        float* error_out, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_radiance_params rp;
    std::vector<int> cps;
    int rc = probe_adaptive_check(c, "rtw_probe_adaptive", probes, n, PP, AD, rgba_out, rp, cps);
    if (rc) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n == 0) return RTW_OK;
    const Tuning tune = read_tuning();
    const size_t chunk = std::min(n, tune.radiance_chunk);
    // staged per probe: 32 B of probe, then its results: 16 B of rgba, 4 B of spp, 4 B of err
    const uint64_t width[4] = {32, 16, 4, 4};
    const bool want[4] = {true, true, true, true};
    const StagePlan st = stage_plan(chunk, 4, width, want);
    QueryCall q;
    if ((rc = query_open(c, q, nullptr, (size_t)st.bytes, true)) != RTW_OK) return rc;
    char* const base = q.stage;
    const size_t o_rgba = (size_t)st.off[1], o_spp = (size_t)st.off[2], o_err = (size_t)st.off[3];
    uint64_t samples = 0;
    rc = query_chunks(
        c, q, n, chunk,
        [&](size_t i0, size_t m) -> int {
            HIP_TRY(c, hipMemcpyAsync(base, probes + 8 * i0, m * 32, hipMemcpyHostToDevice, q.s));
            return RTW_OK;
        },
        [&](size_t i0, size_t m) {  // chunk c runs with the key of its first probe: the bits do not depend on the chunk size
            return probe_adaptive_issue(c, q.d, tune, (const float*)base, m, &rp, PP->mode, AD, cps, radiance_key(rp.key_offset, i0), (float4*)(base + o_rgba),
                                        (int32_t*)(base + o_spp), (float*)(base + o_err), q.s, samples);
        },
        [&](size_t i0, size_t m) -> int {
            HIP_TRY(c, hipMemcpyAsync(rgba_out + 4 * i0, base + o_rgba, m * 16, hipMemcpyDeviceToHost, q.s));
            if (spp_out) HIP_TRY(c, hipMemcpyAsync(spp_out + i0, base + o_spp, m * 4, hipMemcpyDeviceToHost, q.s));
            if (error_out) HIP_TRY(c, hipMemcpyAsync(error_out + i0, base + o_err, m * 4, hipMemcpyDeviceToHost, q.s));
            return RTW_OK;
        });
    if (rc != RTW_OK) return rc;
    return query_stats(c, q, stats, samples, PP->mode == RTW_PROBE_OCCLUSION);
}

// ---- rtw_views_adaptive / rtw_views_adaptive_device (rtw.h): rtw_views' samples taken from checkpoint to checkpoint over the list of
// the pixels that are still active (rtw_view_adaptive.h). The family's loop over the flattened pixels of the views at hand, the rule
// dilated inside each view; a pass is list_pass with k_view_list, and the per-pixel state lives in the allocation the probes use.
typedef void (*ViewListKernel)(const DScene, const ViewListArgs);

// n_views views at d_views (device) -> their frames at d_out (and d_spp, d_err where not null): pixel i of the outputs is flattened
// pixel i of these views
int view_adaptive_issue(rtw_ctx* c, rtw_ctx* d, const Tuning& tune, const rtw_view* d_views, size_t n_views, const rtw_view_params* VP,
                        const rtw_radiance_params* RP, const rtw_adaptive* AD, const std::vector<int>& cps, float4* d_out, int32_t* d_spp, float* d_err,
                        hipStream_t s, uint64_t& samples) {
    const size_t n = (size_t)view_pixels(n_views, VP->width, VP->height);
    DScene sc = d->sc;
    apply_estimator(sc, RP->estimator);
    const ViewListKernel k = RTW_PICK(k_view_list, RP->rng_kind, sc.has_tex);
    AdaptiveState st{};
    const int rc = adaptive_state(c, d->padapt, n, false, &s, st);
    if (rc) return rc;
    const size_t max_grid = (size_t)d->n_cu * (size_t)path_wg_per_cu((const void*)k, d->info.lds_bytes, 0);
    ViewListArgs a{};
    a.v = view_frame_args(d_views, VP->width, VP->height, 0);  // pixel i of the list is pixel i of these views
    a.sample0 = (uint32_t)RP->sample_offset; a.max_depth = (uint32_t)RP->max_depth;
    return adaptive_run(
        c, d, st, adaptive_frames(a.v.width, a.v.height, n_views, AD->threshold, AD->dilate), cps, s, samples, nullptr, nullptr,
        [&](const uint32_t* list, size_t n_active, int n_from, int n_to) {
            return list_pass(
                c, d, tune, max_grid, RP->max_depth == 0, true, list, n_active, n_from, n_to, s,
                [&](const ListPass& p, unsigned grid) {
                    a.p = p;
                    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), d->info.lds_bytes, s, sc, a);
                },
                [&](const uint32_t* range, uint32_t count, uint32_t nb, uint32_t blk0) {
                    hipLaunchKernelGGL(k_adapt_resolve_blocks, dim3(pixel_grid(d, count)), dim3(kBlock), 0, s, d->rad_slab.as<const float4>(), range, count, nb, blk0,
                                       st.accum, st.upart, st.mom);
                });
        },
        [&](unsigned grid) {
            hipLaunchKernelGGL(k_adapt_finish, dim3(grid), dim3(kBlock), 0, s, (const float4*)st.accum, (const float4*)st.upart, (const uint32_t*)st.n,
                               (const float*)st.err, d_out, d_spp, d_err, (uint32_t)n, 0u);
        });
}

// the checks both variants share: rtw_views' and rtw_render_adaptive's; fills the sampling params and the checkpoints
int views_adaptive_check(rtw_ctx* c, const char* what, const rtw_view* views, size_t n_views, const rtw_view_params* VP, const rtw_adaptive* AD,
                         const void* out, rtw_radiance_params& rp, std::vector<int>& cps) {
    const int rc = views_check(c, what, views, n_views, VP, out, rp);
    if (rc) return rc;
    if (!AD) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": null adaptive settings");
    if (const char* why = adaptive_checkpoints(AD->min_spp, AD->step_spp, VP->spp, AD->threshold, AD->dilate, cps))
        return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": " + why);
    return RTW_OK;
}

int impl_adaptive_views_device(rtw_ctx* c, const rtw_view* d_views, size_t n_views, const rtw_view_params* VP, const rtw_adaptive* AD, void* d_rgba,
                               void* d_spp, void* d_error, void* hip_stream, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_radiance_params rp;
    std::vector<int> cps;
    int rc = views_adaptive_check(c, "rtw_views_adaptive_device", d_views, n_views, VP, AD, d_rgba, rp, cps);
    if (rc) return rc;
    if (n_views > 0 && (((uintptr_t)d_views & 15) || ((uintptr_t)d_rgba & 15) || ((uintptr_t)d_spp & 3) || ((uintptr_t)d_error & 3)))
        return fail(c, RTW_ERR_INVALID_ARG, "rtw_views_adaptive_device: views and rgba must be 16-byte aligned, spp and error 4-byte aligned");
    if (stats) memset(stats, 0, sizeof *stats);  // (after every refusal: a refused call leaves *stats alone)
    if (n_views == 0) return RTW_OK;
    QueryCall q;
    if ((rc = query_open(c, q, hip_stream, 0, true)) != RTW_OK) return rc;
    uint64_t samples = 0;
    if ((rc = view_adaptive_issue(c, q.d, read_tuning(), d_views, n_views, VP, &rp, AD, cps, (float4*)d_rgba, (int32_t*)d_spp, (float*)d_error, q.s,
                                  samples)) != RTW_OK)
        return rc;
    return query_stats(c, q, stats, samples, false);
}

int impl_adaptive_views(rtw_ctx* c, const rtw_view* views, size_t n_views, const rtw_view_params* VP, const rtw_adaptive* AD, float* rgba_out,
                        int32_t* spp_out, float* error_out, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_radiance_params rp;
    std::vector<int> cps;
    int rc = views_adaptive_check(c, "rtw_views_adaptive", views, n_views, VP, AD, rgba_out, rp, cps);
    if (rc || (rc = view_records_check(c, "rtw_views_adaptive", views, n_views))) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_views == 0) return RTW_OK;
    const Tuning tune = read_tuning();
    // batches of whole views (the dilated rule reads a pixel's neighbours inside its view): chunks of per * frame pixels are
    // view_adaptive_batch's views [i0 / frame, (i0 + m) / frame) (rtw_view_adaptive_plan.h view_adaptive_chunk)
    const size_t frame = (size_t)view_pixels(1, VP->width, VP->height), n = n_views * frame;
    const size_t per = (size_t)std::min<uint64_t>(view_adaptive_batch_views(VP->width, VP->height, tune.radiance_chunk), n_views);
    const size_t chunk = (size_t)view_adaptive_chunk(per, VP->width, VP->height);
    const uint64_t width[3] = {16, 4, 4};  // staged: a batch's results, 16 B of rgba, 4 B of spp, 4 B of err per pixel
    const bool want[3] = {true, true, true};
    const StagePlan st = stage_plan(chunk, 3, width, want);
    QueryCall q;
    if ((rc = query_open(c, q, nullptr, (size_t)st.bytes, true)) != RTW_OK) return rc;
    if ((rc = view_records_upload(c, q, views, n_views)) != RTW_OK) return rc;
    char* const base = q.stage;
    const size_t o_spp = (size_t)st.off[1], o_err = (size_t)st.off[2];
    uint64_t samples = 0;
    rc = query_chunks(
        c, q, n, chunk, no_upload,
        [&](size_t i0, size_t m) {  // a batch's pixels start at its first view's first
            return view_adaptive_issue(c, q.d, tune, q.d->view_buf.as<const rtw_view>() + i0 / frame, m / frame, VP, &rp, AD, cps, (float4*)base,
                                       (int32_t*)(base + o_spp), (float*)(base + o_err), q.s, samples);
        },
        [&](size_t i0, size_t m) -> int {
            HIP_TRY(c, hipMemcpyAsync(rgba_out + 4 * i0, base, m * 16, hipMemcpyDeviceToHost, q.s));
            if (spp_out) HIP_TRY(c, hipMemcpyAsync(spp_out + i0, base + o_spp, m * 4, hipMemcpyDeviceToHost, q.s));
            if (error_out) HIP_TRY(c, hipMemcpyAsync(error_out + i0, base + o_err, m * 4, hipMemcpyDeviceToHost, q.s));
            return RTW_OK;
        });
    if (rc != RTW_OK) return rc;
    return query_stats(c, q, stats, samples, false);
}

// ---- rtw_paths / rtw_paths_device / rtw_paths_views / rtw_paths_views_device (rtw.h): rtw_radiance's (rtw_views') samples replayed
// one by one through k_paths, a head per sample and a vertex per segment
typedef void (*PathsKernel)(const DScene, const PathsArgs);
// k_paths by its source, under names RTW_PICK can instantiate
template <int KIND, int TEX> constexpr PathsKernel k_paths_rays = k_paths<KIND, TEX, kPathsRays>;
template <int KIND, int TEX> constexpr PathsKernel k_paths_views = k_paths<KIND, TEX, kPathsViews>;

// n rays at d_src (device), or with vf n pixels from flattened pixel vf->first of the view records at d_src -> their n * spp heads
// and, K > 0, records, issued on stream s of device context d and not waited for: one persistent k_paths launch sized as k_cast's,
// ray i on the stream of key0 + i. The counters add up in d->rad_ctl's rows, which the caller zeroed on s. n * spp <= 2^31 - 1.
int paths_issue(rtw_ctx* c, rtw_ctx* d, const void* d_src, size_t n, const rtw_radiance_params* RP, uint32_t key0, int32_t K, float4* d_heads,
                float4* d_vertices, hipStream_t s, const ViewFrame* vf) {
    DScene sc = d->sc;
    apply_estimator(sc, RP->estimator);
    const PathsKernel k = vf ? RTW_PICK(k_paths_views, RP->rng_kind, sc.has_tex) : RTW_PICK(k_paths_rays, RP->rng_kind, sc.has_tex);
    PathsArgs a{};
    if (vf) a.v = view_frame_args(d_src, vf->width, vf->height, vf->first);
    else a.v.rays = (const float4*)d_src;
    a.v.stats = d->rad_ctl.as<unsigned long long>();
    a.v.n = (uint32_t)n; a.v.spp = (uint32_t)RP->spp; a.v.sample0 = (uint32_t)RP->sample_offset; a.v.seed = RP->seed;
    a.v.max_depth = (uint32_t)RP->max_depth; a.v.key0 = key0;
    a.heads = d_heads; a.vertices = d_vertices;
    a.n_pairs = (uint32_t)((uint64_t)n * (uint64_t)RP->spp); a.max_records = (uint32_t)K;
    magic_div(a.v.spp, a.divs_m, a.divs_s1, a.divs_s2);
    const size_t lds = d->info.lds_bytes;
    const size_t per_cu = (size_t)path_wg_per_cu((const void*)k, lds, 0);
    const size_t grid = std::min<size_t>(((size_t)a.n_pairs + kBlock - 1) / kBlock, (size_t)d->n_cu * per_cu);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kBlock), lds, s, sc, a);
    HIP_TRY(c, hipGetLastError());
    return RTW_OK;
}

// what the four variants check after rtw_radiance's (rtw_views') own list, in rtw.h's order; n counts rays, or the pixels asked for
int paths_check(rtw_ctx* c, const char* what, size_t n, const rtw_radiance_params& rp, int32_t K, const uint32_t* reserved, const void* heads,
                const void* vertices, bool device) {
    if (K < 0 || K > rp.max_depth) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": max_records outside 0 .. max_depth");
    if (reserved && (reserved[0] != 0u || reserved[1] != 0u)) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": reserved must be 0");
    if (!paths_pairs_ok(n, rp.spp)) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": more than 2^31 - 1 samples");
    if (n == 0) return RTW_OK;
    if (!heads) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": null heads");
    if ((K > 0) != (vertices != nullptr)) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": vertices must be NULL exactly when max_records is 0");
    if (device && (((uintptr_t)heads & 15) || ((uintptr_t)vertices & 15)))
        return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": heads and vertices must be 16-byte aligned");
    return RTW_OK;
}

// rtw_paths_params' sampling fields as rtw_radiance's params (the two reserved words are checked by paths_check)
const rtw_radiance_params* paths_sampling(const rtw_paths_params* PP, rtw_radiance_params& rp) {
    if (!PP) return nullptr;
    rp = rtw_radiance_params{PP->spp, PP->max_depth, PP->seed, PP->rng_kind, PP->sample_offset, PP->estimator, PP->key_offset, 0u};
    return &rp;
}

// the window [first, first + count) of a views call lies inside its pixels (views_check has bounded their number)
int paths_window_check(rtw_ctx* c, const char* what, size_t n_views, const rtw_view_params* VP, uint64_t first, uint64_t count) {
    const uint64_t total = view_pixels(n_views, VP->width, VP->height);
    if (first > total || count > total - first) return fail(c, RTW_ERR_INVALID_ARG, std::string(what) + ": first + count beyond the call's pixels");
    return RTW_OK;
}

// the device variants: d_src holds the rays, or with vf the view records
int paths_device(rtw_ctx* c, const void* d_src, size_t n, const rtw_radiance_params& rp, int32_t K, void* d_heads, void* d_vertices, void* hip_stream,
                 rtw_stats* stats, const ViewFrame* vf) {
    if (stats) memset(stats, 0, sizeof *stats);  // (after every refusal: a refused call leaves *stats alone)
    if (n == 0) return RTW_OK;
    QueryCall q;
    int rc;
    if ((rc = query_open(c, q, hip_stream, 0, true)) != RTW_OK) return rc;
    if ((rc = paths_issue(c, q.d, d_src, n, &rp, rp.key_offset, K, (float4*)d_heads, (float4*)d_vertices, q.s, vf)) != RTW_OK) return rc;
    return query_stats(c, q, stats, (uint64_t)n * (uint64_t)rp.spp, false);
}

// the host variants: chunks of whole rays (rtw_paths_plan.h) through the staging slab - a chunk's rays (not for views, whose records
// are uploaded once), heads and records
int paths_host(rtw_ctx* c, const float* rays, size_t n, const rtw_radiance_params& rp, int32_t K, rtw_path_head* heads_out, rtw_path_vertex* vertices_out,
               rtw_stats* stats, const rtw_view* views, size_t n_views, const ViewFrame* vf) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (n == 0) return RTW_OK;
    const PathsPlan pl = paths_plan(n, rp.spp, K, read_tuning().paths_chunk_bytes);
    const uint64_t spp = (uint64_t)rp.spp;
    const uint64_t width[3] = {32, spp * sizeof(rtw_path_head), spp * (uint64_t)K * sizeof(rtw_path_vertex)};
    const bool want[3] = {views == nullptr, true, K > 0};
    const StagePlan st = stage_plan(pl.rays, 3, width, want);
    QueryCall q;
    int rc;
    if ((rc = query_open(c, q, nullptr, (size_t)st.bytes, true)) != RTW_OK) return rc;
    if (views && (rc = view_records_upload(c, q, views, n_views)) != RTW_OK) return rc;
    float* const st_rays = (float*)(q.stage + st.off[0]);
    float4* const st_heads = (float4*)(q.stage + st.off[1]);
    float4* const st_vertices = K > 0 ? (float4*)(q.stage + st.off[2]) : nullptr;
    rc = query_chunks(
        c, q, n, (size_t)pl.rays,
        [&](size_t i0, size_t m) -> int {
            if (!views) HIP_TRY(c, hipMemcpyAsync(st_rays, rays + 8 * i0, m * 32, hipMemcpyHostToDevice, q.s));
            // the kernel writes a sample's first min(segments, K) records alone and the chunk comes back whole: the caller's own
            // bytes go up first, so that what is not written comes back as it was
            if (K > 0) {
                const PathsChunk ch = paths_chunk(n, rp.spp, K, pl, i0 / pl.rays);
                HIP_TRY(c, hipMemcpyAsync(st_vertices, (const char*)vertices_out + ch.vertex_off, m * width[2], hipMemcpyHostToDevice, q.s));
            }
            return RTW_OK;
        },
        // chunk c runs with the key of its first ray, or from its first pixel: the bits do not depend on the chunk size
        [&](size_t i0, size_t m) -> int {
            if (!views) return paths_issue(c, q.d, st_rays, m, &rp, radiance_key(rp.key_offset, i0), K, st_heads, st_vertices, q.s, nullptr);
            const ViewFrame f{vf->width, vf->height, vf->first + (uint64_t)i0};
            return paths_issue(c, q.d, q.d->view_buf.as<const void>(), m, &rp, 0u, K, st_heads, st_vertices, q.s, &f);
        },
        [&](size_t i0, size_t m) -> int {
            const PathsChunk ch = paths_chunk(n, rp.spp, K, pl, i0 / pl.rays);
            HIP_TRY(c, hipMemcpyAsync((char*)heads_out + ch.head_off, st_heads, m * width[1], hipMemcpyDeviceToHost, q.s));
            if (K > 0) HIP_TRY(c, hipMemcpyAsync((char*)vertices_out + ch.vertex_off, st_vertices, m * width[2], hipMemcpyDeviceToHost, q.s));
            return RTW_OK;
        });
    if (rc != RTW_OK) return rc;
    return query_stats(c, q, stats, (uint64_t)n * spp, false);
}

int impl_paths_device(rtw_ctx* c, const float* rays, size_t n, const rtw_paths_params* PP, void* d_heads, void* d_vertices, void* hip_stream,
                      rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_radiance_params rp;
    static const char some = 0;  // radiance_check's null test of the output is made by paths_check, on heads and vertices
    int rc = radiance_check(c, "rtw_paths_device", rays, n, paths_sampling(PP, rp), &some);
    if (rc || (rc = paths_check(c, "rtw_paths_device", n, rp, PP->max_records, PP->reserved, d_heads, d_vertices, true))) return rc;
    if (n > 0 && ((uintptr_t)rays & 15)) return fail(c, RTW_ERR_INVALID_ARG, "rtw_paths_device: rays must be 16-byte aligned");
    return paths_device(c, rays, n, rp, PP->max_records, d_heads, d_vertices, hip_stream, stats, nullptr);
}

int impl_paths(rtw_ctx* c, const float* rays, size_t n, const rtw_paths_params* PP, rtw_path_head* heads_out, rtw_path_vertex* vertices_out,
               rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_radiance_params rp;
    static const char some = 0;
    int rc = radiance_check(c, "rtw_paths", rays, n, paths_sampling(PP, rp), &some);
    if (rc || (rc = paths_check(c, "rtw_paths", n, rp, PP->max_records, PP->reserved, heads_out, vertices_out, false))) return rc;
    return paths_host(c, rays, n, rp, PP->max_records, heads_out, vertices_out, stats, nullptr, 0, nullptr);
}

int impl_paths_views_device(rtw_ctx* c, const rtw_view* d_views, size_t n_views, const rtw_view_params* VP, uint64_t first, uint64_t count,
                            int32_t K, void* d_heads, void* d_vertices, void* hip_stream, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_radiance_params rp;
    static const char some = 0;
    int rc = views_check(c, "rtw_paths_views_device", d_views, n_views, VP, &some, rp);
    if (rc || (rc = paths_window_check(c, "rtw_paths_views_device", n_views, VP, first, count)) ||
        (rc = paths_check(c, "rtw_paths_views_device", (size_t)count, rp, K, nullptr, d_heads, d_vertices, true)))
        return rc;
    if (count > 0 && ((uintptr_t)d_views & 15)) return fail(c, RTW_ERR_INVALID_ARG, "rtw_paths_views_device: views must be 16-byte aligned");
    const ViewFrame vf{VP->width, VP->height, first};
    return paths_device(c, d_views, (size_t)count, rp, K, d_heads, d_vertices, hip_stream, stats, &vf);
}

int impl_paths_views(rtw_ctx* c, const rtw_view* views, size_t n_views, const rtw_view_params* VP, uint64_t first, uint64_t count, int32_t K,
                     rtw_path_head* heads_out, rtw_path_vertex* vertices_out, rtw_stats* stats) {
    if (!c) return RTW_ERR_INVALID_ARG;
    rtw_radiance_params rp;
    static const char some = 0;
    int rc = views_check(c, "rtw_paths_views", views, n_views, VP, &some, rp);
    if (rc || (rc = view_records_check(c, "rtw_paths_views", views, n_views)) ||
        (rc = paths_window_check(c, "rtw_paths_views", n_views, VP, first, count)) ||
        (rc = paths_check(c, "rtw_paths_views", (size_t)count, rp, K, nullptr, heads_out, vertices_out, false)))
        return rc;
    const ViewFrame vf{VP->width, VP->height, first};
    return paths_host(c, nullptr, (size_t)count, rp, K, heads_out, vertices_out, stats, views, n_views, &vf);
}

int impl_debug_math(rtw_ctx* c, int op, uint64_t* out) {
    if (!c) return RTW_ERR_INVALID_ARG;
    if (op < 0 || op > 6 || !out) return fail(c, RTW_ERR_INVALID_ARG, "bad arguments");
    HIP_TRY(c, hipSetDevice(c->device));
    const unsigned long long init[3] = {0ull, 0ull, ~0ull};
    unsigned long long got[3];
    DevBuf buf;
    HIP_TRY(c, buf.grow(sizeof init, sizeof init));
    unsigned long long* const d = buf.as<unsigned long long>();
    hipError_t e = hipMemcpy(d, init, sizeof init, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        // 2^16 blocks of 256 threads: 256 patterns per thread
        hipLaunchKernelGGL(k_debug_math, dim3(65536), dim3(kBlock), 0, c->stream, op, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(got, d, sizeof got, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, RTW_ERR_DEVICE, std::string("rtw_debug_math: ") + hipGetErrorString(e));
    for (int i = 0; i < 3; i++) out[i] = got[i];
    return RTW_OK;
}

}  // namespace

extern "C" {

int rtw_abi_version(void) { return RTW_ABI_VERSION; }

const char* rtw_last_error(rtw_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int rtw_create(rtw_ctx** out, int n_devices, const int* device_ids) {
    if (!out) return RTW_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded(nullptr, [&] { return impl_create(out, n_devices, device_ids); });
}
int rtw_destroy(rtw_ctx* c) { return guarded(nullptr, [&] { return impl_destroy(c); }); }
int rtw_upload_scene(rtw_ctx* c, const void* blob, size_t bytes) { return guarded(c, [&] { return impl_upload_scene(c, blob, bytes); }); }
int rtw_render_device(rtw_ctx* c, const rtw_params* P, void* d_rgba, void* hip_stream, rtw_stats* stats) {
    return guarded(c, [&] { return impl_render_device(c, P, d_rgba, hip_stream, stats); });
}
int rtw_render(rtw_ctx* c, const rtw_params* P, float* rgba_out, rtw_stats* stats) { return guarded(c, [&] { return impl_render(c, P, rgba_out, stats); }); }
int rtw_denoise(rtw_ctx* c, const float* rgba_in, float* rgba_out, int32_t width, int32_t height, int32_t iterations, float sigma) {
    return guarded(c, [&] { return impl_denoise(c, rgba_in, rgba_out, width, height, iterations, sigma); });
}
int rtw_debug_intersect(rtw_ctx* c, const float* rays, const float* ray_time, const float* gather_time, int n, float* out_t, int32_t* out_prim) {
    return guarded(c, [&] { return impl_debug_intersect(c, rays, ray_time, gather_time, n, out_t, out_prim); });
}
int rtw_debug_math(rtw_ctx* c, int op, uint64_t* out) { return guarded(c, [&] { return impl_debug_math(c, op, out); }); }
int rtw_render_guides(rtw_ctx* c, const rtw_params* P, const rtw_guides* out, rtw_stats* stats) {
    return guarded(c, [&] { return impl_render_guides(c, P, out, stats); });
}
int rtw_render_adaptive(rtw_ctx* c, const rtw_params* P, const rtw_adaptive* ad, float* rgba_out, int32_t* spp_out, float* error_out, rtw_stats* stats) {
    return guarded(c, [&] { return impl_render_adaptive(c, P, ad, rgba_out, spp_out, error_out, stats); });
}
int rtw_denoise_guided(rtw_ctx* c, const float* rgba_in, const float* albedo, const float* normal, float* rgba_out, int32_t width, int32_t height,
                       int32_t iterations, float sigma, float sigma_albedo, float sigma_normal) {
    return guarded(c, [&] { return impl_denoise_guided(c, rgba_in, albedo, normal, rgba_out, width, height, iterations, sigma, sigma_albedo, sigma_normal); });
}
int rtw_accum_begin(rtw_ctx* c, const rtw_params* P, uint32_t flags) { return guarded(c, [&] { return impl_accum_begin(c, P, flags); }); }
int rtw_accum_add(rtw_ctx* c, int32_t spp, rtw_stats* stats) { return guarded(c, [&] { return impl_accum_add(c, spp, stats); }); }
int rtw_accum_read(rtw_ctx* c, float* rgba_out, float* error_out) { return guarded(c, [&] { return impl_accum_read(c, rgba_out, error_out); }); }
int rtw_accum_read_device(rtw_ctx* c, void* d_rgba, void* hip_stream) { return guarded(c, [&] { return impl_accum_read_device(c, d_rgba, hip_stream); }); }
int rtw_accum_status(rtw_ctx* c, rtw_accum_info* out) { return guarded(c, [&] { return impl_accum_status(c, out); }); }
int rtw_accum_save(rtw_ctx* c, void* blob, size_t bytes) { return guarded(c, [&] { return impl_accum_save(c, blob, bytes); }); }
int rtw_accum_restore(rtw_ctx* c, const void* blob, size_t bytes) { return guarded(c, [&] { return impl_accum_restore(c, blob, bytes); }); }
int rtw_accum_end(rtw_ctx* c) { return guarded(c, [&] { return impl_accum_end(c); }); }
int rtw_cast(rtw_ctx* c, const float* rays, const float* ray_time, const float* gather_time, size_t n, int32_t mode, const rtw_hits* out, rtw_stats* stats) {
    return guarded(c, [&] { return impl_cast(c, rays, ray_time, gather_time, n, mode, out, stats); });
}
int rtw_cast_device(rtw_ctx* c, const float* rays, const float* ray_time, const float* gather_time, size_t n, int32_t mode, const rtw_hits* out,
                    void* hip_stream, rtw_stats* stats) {
    return guarded(c, [&] { return impl_cast_device(c, rays, ray_time, gather_time, n, mode, out, hip_stream, stats); });
}
int rtw_radiance(rtw_ctx* c, const float* rays, size_t n, const rtw_radiance_params* RP, float* rgba_out, rtw_stats* stats) {
    return guarded(c, [&] { return impl_radiance(c, rays, n, RP, rgba_out, stats); });
}
int rtw_radiance_device(rtw_ctx* c, const float* rays, size_t n, const rtw_radiance_params* RP, void* d_rgba, void* hip_stream, rtw_stats* stats) {
    return guarded(c, [&] { return impl_radiance_device(c, rays, n, RP, d_rgba, hip_stream, stats); });
}
int rtw_probe(rtw_ctx* c, const float* probes, size_t n, const rtw_probe_params* PP, float* rgba_out, rtw_stats* stats) {
    return guarded(c, [&] { return impl_probe(c, probes, n, PP, rgba_out, stats); });
}
int rtw_probe_device(rtw_ctx* c, const float* probes, size_t n, const rtw_probe_params* PP, void* d_rgba, void* hip_stream, rtw_stats* stats) {
    return guarded(c, [&] { return impl_probe_device(c, probes, n, PP, d_rgba, hip_stream, stats); });
}
int rtw_probe_sh(rtw_ctx* c, const float* points, size_t n, const rtw_radiance_params* RP, float* sh_out, rtw_stats* stats) {
    return guarded(c, [&] { return impl_sh_probe(c, points, n, RP, sh_out, stats); });
}
int rtw_probe_sh_device(rtw_ctx* c, const float* points, size_t n, const rtw_radiance_params* RP, void* d_sh, void* hip_stream, rtw_stats* stats) {
    return guarded(c, [&] { return impl_sh_probe_device(c, points, n, RP, d_sh, hip_stream, stats); });
}
int rtw_probe_adaptive(rtw_ctx* c, const float* probes, size_t n, const rtw_probe_params* PP, const rtw_adaptive* ad, float* rgba_out, int32_t* spp_out,
                       float* error_out, rtw_stats* stats) {
    return guarded(c, [&] { return impl_adaptive_probe(c, probes, n, PP, ad, rgba_out, spp_out, error_out, stats); });
}
int rtw_probe_adaptive_device(rtw_ctx* c, const float* d_probes, size_t n, const rtw_probe_params* PP, const rtw_adaptive* ad, void* d_rgba, void* d_spp,
                              void* d_error, void* hip_stream, rtw_stats* stats) {
    return guarded(c, [&] { return impl_adaptive_probe_device(c, d_probes, n, PP, ad, d_rgba, d_spp, d_error, hip_stream, stats); });
}
int rtw_views(rtw_ctx* c, const rtw_view* views, size_t n_views, const rtw_view_params* VP, float* rgba_out, rtw_stats* stats) {
    return guarded(c, [&] { return impl_views(c, views, n_views, VP, rgba_out, stats); });
}
int rtw_views_device(rtw_ctx* c, const rtw_view* d_views, size_t n_views, const rtw_view_params* VP, void* d_rgba, void* hip_stream, rtw_stats* stats) {
    return guarded(c, [&] { return impl_views_device(c, d_views, n_views, VP, d_rgba, hip_stream, stats); });
}
int rtw_views_guides(rtw_ctx* c, const rtw_view* views, size_t n_views, const rtw_view_params* VP, const rtw_guides* out, rtw_stats* stats) {
    return guarded(c, [&] { return impl_views_guides(c, views, n_views, VP, out, stats); });
}
int rtw_views_guides_device(rtw_ctx* c, const rtw_view* d_views, size_t n_views, const rtw_view_params* VP, const rtw_guides* d_out, void* hip_stream,
                            rtw_stats* stats) {
    return guarded(c, [&] { return impl_views_guides_device(c, d_views, n_views, VP, d_out, hip_stream, stats); });
}
int rtw_views_adaptive(rtw_ctx* c, const rtw_view* views, size_t n_views, const rtw_view_params* VP, const rtw_adaptive* ad, float* rgba_out, int32_t* spp_out,
                       float* error_out, rtw_stats* stats) {
    return guarded(c, [&] { return impl_adaptive_views(c, views, n_views, VP, ad, rgba_out, spp_out, error_out, stats); });
}
int rtw_views_adaptive_device(rtw_ctx* c, const rtw_view* d_views, size_t n_views, const rtw_view_params* VP, const rtw_adaptive* ad, void* d_rgba, void* d_spp,
                              void* d_error, void* hip_stream, rtw_stats* stats) {
    return guarded(c, [&] { return impl_adaptive_views_device(c, d_views, n_views, VP, ad, d_rgba, d_spp, d_error, hip_stream, stats); });
}
int rtw_denoise_views(rtw_ctx* c, const float* rgba_in, const float* albedo, const float* normal, float* rgba_out, size_t n_views, int32_t width,
                      int32_t height, int32_t iterations, float sigma, float sigma_albedo, float sigma_normal) {
    return guarded(c, [&] { return impl_denoise_views(c, rgba_in, albedo, normal, rgba_out, n_views, width, height, iterations, sigma, sigma_albedo, sigma_normal); });
}
int rtw_denoise_views_device(rtw_ctx* c, const float* rgba_in, const float* albedo, const float* normal, float* rgba_out, size_t n_views, int32_t width,
                             int32_t height, int32_t iterations, float sigma, float sigma_albedo, float sigma_normal, void* hip_stream) {
    return guarded(c, [&] {
        return impl_denoise_views_device(c, rgba_in, albedo, normal, rgba_out, n_views, width, height, iterations, sigma, sigma_albedo, sigma_normal, hip_stream);
    });
}

int rtw_paths(rtw_ctx* c, const float* rays, size_t n, const rtw_paths_params* PP, rtw_path_head* heads_out, rtw_path_vertex* vertices_out, rtw_stats* stats) {
    return guarded(c, [&] { return impl_paths(c, rays, n, PP, heads_out, vertices_out, stats); });
}
int rtw_paths_device(rtw_ctx* c, const float* rays, size_t n, const rtw_paths_params* PP, void* d_heads, void* d_vertices, void* hip_stream, rtw_stats* stats) {
    return guarded(c, [&] { return impl_paths_device(c, rays, n, PP, d_heads, d_vertices, hip_stream, stats); });
}
int rtw_paths_views(rtw_ctx* c, const rtw_view* views, size_t n_views, const rtw_view_params* VP, uint64_t first, uint64_t count, int32_t max_records,
                    rtw_path_head* heads_out, rtw_path_vertex* vertices_out, rtw_stats* stats) {
    return guarded(c, [&] { return impl_paths_views(c, views, n_views, VP, first, count, max_records, heads_out, vertices_out, stats); });
}
int rtw_paths_views_device(rtw_ctx* c, const rtw_view* d_views, size_t n_views, const rtw_view_params* VP, uint64_t first, uint64_t count,
                           int32_t max_records, void* d_heads, void* d_vertices, void* hip_stream, rtw_stats* stats) {
    return guarded(c, [&] { return impl_paths_views_device(c, d_views, n_views, VP, first, count, max_records, d_heads, d_vertices, hip_stream, stats); });
}

}  // extern "C"
