// Director.h — host driver with the reference's public surface (RestOfLife/Director.h:115-126):
//   init / createScene / renderFrame / printPPM / destroy.
// Everything OptiX inside the reference's Director (context, 26 modules, 36 program groups, pipeline,
// SBT, launch params, denoiser) is replaced by calls into the C ABI of include/rtw.h.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/rtw.h"
#include "ioScene.h"

class Director {
public:
    // edge-stopping sigmas of the guided denoiser (the defaults of raytracing_weekend_amd.abi.Renderer.denoise_guided, where they
    // are measured)
    static constexpr float kDenoiseSigmaAlbedo = 0.4f;
    static constexpr float kDenoiseSigmaNormal = 0.5f;

    Director(bool verbose, bool debug) : _verbose(verbose), _debug(debug) {}

    void init(unsigned int width, unsigned int height, unsigned int samples);
    void destroy();

    void createScene(unsigned int sceneNumber);
    void renderFrame();
    // a turntable through rtw_views, one call for all n frames: view 0 is the scene's camera, view k that camera turned rigidly by
    // 360 k / n degrees about its v axis through the centre of its frame (raytracing_weekend_amd.bake.orbit_views, operation for
    // operation in double precision); every view renders with the seed. onFrame(k) is called with frame k in hostBuffer(), in order.
    // With an -aov prefix or a guided denoiser the views' guides come from one rtw_views_guides call (frame k's are what writeGuides
    // writes inside onFrame(k)), and a guided denoiser filters all frames in one rtw_denoise_views call, with renderFrame's display
    // encoding and sigmas. After setAdaptive the frames come from one rtw_views_adaptive call (renderFrame's settings, dilate 1), and
    // frame k's sample counts and errors are what writeGuides writes beside its guides.
    void renderOrbit(int n, const std::function<void(int)>& onFrame);
    static void orbitViews(const rtw_camera& camera, int cameraType, uint32_t seed, int n, std::vector<rtw_view>& out);
    void printPPM();
    // additions: an 8K frame is ~400 MB as ASCII P3; P6 is 100 MB, PFM keeps the linear floats
    bool writeBinaryPPM(const std::string& path) const;  // P6, same sqrt + 255.99 quantisation as printPPM
    bool writePFM(const std::string& path) const;        // "PF", little-endian, linear radiance, rows bottom-up
    bool writePNG(const std::string& path) const;        // 8-bit RGB, same quantisation; stored (uncompressed) deflate blocks

    // additions over the reference (its depth is hard-wired to 20 at Director.cpp:42, its RNG to tea+lcg)
    void setMaxDepth(int depth) { m_maxRayDepth = depth; }
    void setSeed(uint32_t seed) { m_seed = seed; }
    void setRngKind(int kind) { m_rngKind = kind; }
    void setDevice(int device) { m_devices.assign(1, device); }
    // n GPUs of this node, devices first .. first + n - 1: the frame is split into n interleaved row shards inside the library
    // (rtw_create with n_devices = n) and gathered on the first device; the image does not depend on n
    void setDevices(int n, int first = 0, bool same = false) { m_devices.clear(); for (int i = 0; i < n; i++) m_devices.push_back(same ? first : first + i); }
    void setEstimator(int estimator) { m_estimator = estimator; }  // rtw_estimator
    void setCameraKind(int kind) { m_cameraKind = kind; }          // rtw_camera_type (the reference only ever builds the perspective one)
    // the reference's renderFrame ends with the OptiX AI denoiser (Director.cpp:986-997); iterations > 0 runs the
    // a-trous stand-in (rtw_denoise) on the frame instead
    void setDenoise(int iterations, float sigma) { m_denoiseIterations = iterations; m_denoiseSigma = sigma; }
    // guide buffers (rtw_render_guides) of `spp` samples (0: min(Ns, 16)), rendered by renderFrame when an -aov prefix is set or the
    // denoiser is guided; guided: the denoiser pass is rtw_denoise_guided, steered by the albedo and normal guides
    void setGuides(const std::string& aovPrefix, int spp, bool guided) { m_aovPrefix = aovPrefix; m_guideSpp = spp; m_guided = guided; }
    // adaptive sampling (rtw_render_adaptive): renderFrame renders until every pixel's error estimate is below `threshold` or it has
    // the -ns cap; minSpp samples first, then checkpoints `stepSpp` apart (0: half of what a pixel has); dilate 1
    void setAdaptive(float threshold, int minSpp, int stepSpp) { m_adaptive = true; m_adThreshold = threshold; m_adMinSpp = minSpp; m_adStepSpp = stepSpp; }
    // accumulation session (rtw_accum_*): renderFrame renders in adds of `step` samples (0: one add) and calls onFrame(done) with the
    // frame of the samples so far in hostBuffer() after every add; the final frame is the one-shot frame, bit for bit. -ns must be
    // a multiple of 16.
    void setProgressive(int step, std::function<void(int)> onFrame) { m_session = true; m_progStep = step; m_onFrame = std::move(onFrame); }
    // the session's state is written to `path` when the render ends / the render starts from the state in `path` (-ns is then the
    // new total, at least what the state holds; scene, size and parameters must be the checkpoint's)
    void setCheckpoint(const std::string& path) { m_session = true; m_checkpoint = path; }
    void setResume(const std::string& path) { m_session = true; m_resume = path; }
    // PREFIX_albedo.pfm, PREFIX_normal.pfm (PF, rgb) and PREFIX_depth.pfm (Pf), rows bottom-up as writePFM; after an adaptive
    // frame also PREFIX_spp.pfm and PREFIX_error.pfm (Pf: each pixel's sample count and error estimate)
    bool writeGuides(const std::string& prefix) const;
    // the samples [0, Ns) of pixel (x, y) (row 0 the bottom row) of the frame renderFrame renders, replayed through rtw_paths_views
    // with the blob's own view and the frame's seed, generator, estimator and depth: one text line per sample ("sample S key K
    // segments N shadow_rays M gather_time .. radiance ..") followed by one per recorded vertex ("vertex S J prim P flags F o .. t ..
    // d .. contribution .. throughput .. ray_time .."), every float as the 8 hex digits of its bits followed by %.9g. Verbose: the
    // sample with the largest luminance is named on stderr.
    bool writePaths(int x, int y, const std::string& path);
    const rtw_stats& stats() const { return m_stats; }
    const std::vector<float>& hostBuffer() const { return m_hostBuffer; }  // linear RGBA, row 0 = bottom row

private:
    void marshalAndUpload();  // createSBT + initLaunchParams of the reference
    void renderSession(const rtw_params& p);  // renderFrame's render through an accumulation session

    int m_Nx = 0, m_Ny = 0, m_Ns = 0;
    int m_maxRayDepth = 20;
    uint32_t m_seed = 0x6314759u;
    int m_rngKind = RTW_RNG_PHILOX;
    std::vector<int> m_devices{0};
    int m_estimator = RTW_EST_REFERENCE;
    int m_cameraKind = RTW_CAM_PERSPECTIVE;
    int m_denoiseIterations = 0;
    float m_denoiseSigma = 0.5f;
    std::string m_aovPrefix;
    int m_guideSpp = 0;
    bool m_guided = false;
    std::vector<float> m_albedo, m_normal, m_depth;  // guide buffers of the last renderFrame (empty when none were rendered)
    bool m_adaptive = false;
    float m_adThreshold = 0.f;
    int m_adMinSpp = 64, m_adStepSpp = 0;
    std::vector<float> m_sppMap, m_errMap;  // the last adaptive frame's sample counts and error estimates
    bool m_session = false;
    int m_progStep = 0;
    std::function<void(int)> m_onFrame;
    std::string m_checkpoint, m_resume;
    rtw_camera m_camera{};  // the uploaded blob's camera and its kind (renderOrbit turns it)
    int m_blobCameraType = RTW_CAM_PERSPECTIVE;
    rtw_ctx* m_ctx = nullptr;
    rtwhost::ioScene m_scene;
    std::vector<float> m_hostBuffer;
    rtw_stats m_stats{};
    bool _verbose = false;
    bool _debug = false;
};
