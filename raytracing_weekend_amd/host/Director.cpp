// Director.cpp — see Director.h. Reference call sites replaced:
//   Director::init          Director.cpp:33-64    -> rtw_create
//   Director::createScene   Director.cpp:951-969  -> ioScene::init + marshalScene + rtw_upload_scene
//   Director::renderFrame   Director.cpp:971-1008 -> rtw_render (optixLaunch + D2H copy; no AI denoiser), or an accumulation
//                                                    session (rtw_accum_*: what the accum_buffer left commented out at :485-488 was for)
//   Director::renderOrbit   (no counterpart)      -> rtw_views: n frames of a turntable in one call (rtw_views_adaptive with -adaptive)
//   Director::writePaths    (no counterpart)      -> rtw_paths_views: the samples of one pixel of the frame, replayed, as text
//   Director::printPPM      Director.cpp:1010-1031
//   Director::destroy       Director.cpp:66-104   -> rtw_destroy
#include "Director.h"

#include <cmath>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>

#include "../csrc/rtw_accum_state.h"  // kAccumCapMax (host-only, no HIP)
#include "../csrc/rtw_plan.h"  // adaptive_checkpoints (host-only planning, no HIP)
#include "PfmWriter.h"
#include "SceneMarshal.h"

namespace {
[[noreturn]] void die(rtw_ctx* ctx, const char* what, int rc) {
    std::cerr << "ERROR: " << what << " failed (" << rc << "): " << (ctx ? rtw_last_error(ctx) : "") << std::endl;
    std::exit(EXIT_FAILURE);  // the reference lets OPTIX_CHECK/CUDA_CHECK exceptions terminate the process
}
}  // namespace

void Director::init(unsigned int width, unsigned int height, unsigned int samples) {
    m_Nx = static_cast<int>(width);
    m_Ny = static_cast<int>(height);
    m_Ns = static_cast<int>(samples);
    if (m_devices.empty()) m_devices.assign(1, 0);
    int rc = rtw_create(&m_ctx, static_cast<int>(m_devices.size()), m_devices.data());
    if (rc != RTW_OK) die(nullptr, "rtw_create", rc);
    m_hostBuffer.assign(static_cast<size_t>(m_Nx) * m_Ny * 4, 0.f);
}

void Director::destroy() {
    m_scene.destroy();
    if (m_ctx) rtw_destroy(m_ctx);
    m_ctx = nullptr;
    m_hostBuffer.clear();
}

void Director::createScene(unsigned int sceneNumber) {
    int error = m_scene.init(m_Nx, m_Ny, m_Ns, m_maxRayDepth, static_cast<int>(sceneNumber));
    if (error) std::exit(EXIT_FAILURE);  // Director.cpp:954-958
    m_scene.setCameraKind(m_cameraKind);
    marshalAndUpload();
    if (_verbose) std::cerr << "INFO: Scene description: " << m_scene.getDescription() << std::endl;
}

void Director::marshalAndUpload() {
    std::vector<uint8_t> blob = rtwhost::marshalScene(m_scene);
    if (blob.size() >= sizeof(rtw_scene_header)) {
        rtw_scene_header h;
        std::memcpy(&h, blob.data(), sizeof h);
        m_camera = h.camera;
        m_blobCameraType = h.camera_type;
    }
    int rc = rtw_upload_scene(m_ctx, blob.data(), blob.size());
    if (rc != RTW_OK) die(m_ctx, "rtw_upload_scene", rc);
}

void Director::renderFrame() {
    rtw_params p{};
    p.width = m_Nx;
    p.height = m_Ny;
    p.spp = m_Ns;
    p.max_depth = m_maxRayDepth;
    p.seed = m_seed;
    p.row0 = 0;
    p.row1 = m_Ny;
    p.rng_kind = m_rngKind;
    p.estimator = m_estimator;
    int rc = RTW_OK;
    if (m_session) {
        if (m_adaptive) {
            std::cerr << "ERROR: -progressive / -checkpoint / -resume do not combine with -adaptive" << std::endl;
            std::exit(EXIT_FAILURE);
        }
        renderSession(p);
    } else if (m_adaptive) {
        const size_t npix = static_cast<size_t>(m_Nx) * m_Ny;
        std::vector<int32_t> spp(npix);
        m_errMap.assign(npix, 0.f);
        const rtw_adaptive ad{m_adMinSpp, m_adStepSpp, m_adThreshold, 1};
        rc = rtw_render_adaptive(m_ctx, &p, &ad, m_hostBuffer.data(), spp.data(), m_errMap.data(), &m_stats);
        if (rc != RTW_OK) die(m_ctx, "rtw_render_adaptive", rc);
        m_sppMap.assign(spp.begin(), spp.end());
        if (_verbose) {
            int lo = m_Ns, hi = 0;
            for (int32_t n : spp) { lo = std::min(lo, n); hi = std::max(hi, n); }
            std::vector<int> cps;  // the library's own schedule: one pass per checkpoint up to the largest count
            (void)rtwk::adaptive_checkpoints(m_adMinSpp, m_adStepSpp, m_Ns, m_adThreshold, 1, cps);
            const long passes = std::count_if(cps.begin(), cps.end(), [&](int n) { return n <= hi; });
            const double uniform = static_cast<double>(npix) * m_Ns;
            std::cerr << "INFO: adaptive: " << passes << " passes, spp mean " << static_cast<double>(m_stats.samples) / npix << " min " << lo
                      << " max " << hi << ", " << uniform - static_cast<double>(m_stats.samples) << " samples saved against uniform "
                      << m_Ns << " spp (" << 100.0 * (1.0 - static_cast<double>(m_stats.samples) / uniform) << " %)" << std::endl;
        }
    } else {
        rc = rtw_render(m_ctx, &p, m_hostBuffer.data(), &m_stats);
        if (rc != RTW_OK) die(m_ctx, "rtw_render", rc);
    }
    const bool guidedDenoise = m_guided && m_denoiseIterations > 0;
    if (!m_aovPrefix.empty() || guidedDenoise) {
        // the guide layers the reference's OptiX denoiser could take (Director.cpp:887-949 sets up the beauty layer alone)
        const size_t npix = static_cast<size_t>(m_Nx) * m_Ny;
        m_albedo.assign(npix * 4, 0.f);
        m_normal.assign(npix * 4, 0.f);
        m_depth.assign(npix, 0.f);
        rtw_params g = p;
        g.spp = m_guideSpp > 0 ? m_guideSpp : std::min(m_Ns, 16);
        rtw_guides out{m_albedo.data(), m_normal.data(), m_depth.data(), nullptr};
        rtw_stats gs{};
        rc = rtw_render_guides(m_ctx, &g, &out, &gs);
        if (rc != RTW_OK) die(m_ctx, "rtw_render_guides", rc);
        if (_verbose) std::cerr << "INFO: guides: " << g.spp << " spp in " << gs.seconds << " s on the GPU" << std::endl;
    }
    if (m_denoiseIterations > 0) {
        // Director.cpp:986-997: the denoiser pass closes the frame. The reference feeds its LDR model the display-encoded
        // image (raygen.cu:151-155 writes sqrt(colour)); the stand-in filters the same encoding, clamped to [0, 1], and
        // the buffer goes back to linear for the writers.
        std::vector<float> enc(m_hostBuffer.size()), filtered(m_hostBuffer.size());
        for (size_t i = 0; i < enc.size(); i++) {
            float c = m_hostBuffer[i];
            if ((i & 3) != 3) { c = !(c == c) || c < 0.f ? 0.f : (c > 1.f ? 1.f : c); c = std::sqrt(c); }
            enc[i] = c;
        }
        if (guidedDenoise) {
            rc = rtw_denoise_guided(m_ctx, enc.data(), m_albedo.data(), m_normal.data(), filtered.data(), m_Nx, m_Ny, m_denoiseIterations,
                                    m_denoiseSigma, kDenoiseSigmaAlbedo, kDenoiseSigmaNormal);
            if (rc != RTW_OK) die(m_ctx, "rtw_denoise_guided", rc);
        } else {
            rc = rtw_denoise(m_ctx, enc.data(), filtered.data(), m_Nx, m_Ny, m_denoiseIterations, m_denoiseSigma);
            if (rc != RTW_OK) die(m_ctx, "rtw_denoise", rc);
        }
        for (size_t i = 0; i < enc.size(); i++) m_hostBuffer[i] = (i & 3) != 3 ? filtered[i] * filtered[i] : filtered[i];
    }
    if (_verbose) {
        const double s = m_stats.seconds > 0 ? m_stats.seconds : 1e-9;
        std::cerr << "INFO: " << m_stats.samples << " samples, " << m_stats.segments << " segments, " << m_stats.shadow_rays
                  << " shadow rays in " << m_stats.seconds << " s on the GPU = " << m_stats.samples / s / 1e6 << " Msamples/s, "
                  << m_stats.algorithmic_bytes / s / 1e9 << " GB/s algorithmic" << std::endl;
    }
}

// bake.orbit_views in C++: the same operations in the same order in double precision, rounded to float once, so that the views -
// and with them the frames - are the ones Python makes
void Director::orbitViews(const rtw_camera& camera, int cameraType, uint32_t seed, int n, std::vector<rtw_view>& out) {
    typedef double V3[3];
    auto view = [&](const rtw_camera& c) {
        rtw_view v{};
        v.camera = c;
        v.camera_type = cameraType;
        v.seed = seed;
        return v;
    };
    out.assign(1, view(camera));  // view 0: the camera itself, copied
    const float* fields[7] = {camera.origin, camera.u, camera.v, camera.w, camera.lower_left, camera.horizontal, camera.vertical};
    V3 c[7], pivot, axis;
    for (int f = 0; f < 7; f++)
        for (int i = 0; i < 3; i++) c[f][i] = static_cast<double>(fields[f][i]);
    for (int i = 0; i < 3; i++) pivot[i] = (c[4][i] + c[5][i] / 2.0) + c[6][i] / 2.0;
    const double norm = std::sqrt((c[2][0] * c[2][0] + c[2][1] * c[2][1]) + c[2][2] * c[2][2]);
    for (int i = 0; i < 3; i++) axis[i] = c[2][i] / norm;
    for (int k = 1; k < n; k++) {
        const double ang = (2.0 * M_PI * static_cast<double>(k)) / static_cast<double>(n);
        const double cs = std::cos(ang), sn = std::sin(ang), omc = 1.0 - cs;
        auto rot = [&](const V3 x, V3 r) {
            const V3 cr = {axis[1] * x[2] - axis[2] * x[1], axis[2] * x[0] - axis[0] * x[2], axis[0] * x[1] - axis[1] * x[0]};
            const double d = (axis[0] * x[0] + axis[1] * x[1]) + axis[2] * x[2];
            for (int i = 0; i < 3; i++) r[i] = (x[i] * cs + cr[i] * sn) + axis[i] * (d * omc);
        };
        rtw_camera t = camera;
        float* dst[7] = {t.origin, t.u, t.v, t.w, t.lower_left, t.horizontal, t.vertical};
        for (int f = 0; f < 7; f++) {
            const bool point = f == 0 || f == 4;  // points turn about the pivot, vectors about the origin
            V3 x, r;
            for (int i = 0; i < 3; i++) x[i] = point ? c[f][i] - pivot[i] : c[f][i];
            rot(x, r);
            for (int i = 0; i < 3; i++) dst[f][i] = static_cast<float>(point ? pivot[i] + r[i] : r[i]);
        }
        out.push_back(view(t));
    }
}

void Director::renderOrbit(int n, const std::function<void(int)>& onFrame) {
    std::vector<rtw_view> views;
    orbitViews(m_camera, m_blobCameraType, m_seed, n, views);
    rtw_view_params vp{};
    vp.width = m_Nx;
    vp.height = m_Ny;
    vp.spp = m_Ns;
    vp.max_depth = m_maxRayDepth;
    vp.rng_kind = m_rngKind;
    vp.estimator = m_estimator;
    const size_t frame = static_cast<size_t>(m_Nx) * m_Ny * 4;
    std::vector<float> frames(frame * views.size());
    const size_t npix = static_cast<size_t>(m_Nx) * m_Ny;
    std::vector<int32_t> spp;
    std::vector<float> err;
    if (m_adaptive) {  // renderFrame's adaptive settings (dilate 1), every view stopping on its own pixels
        spp.resize(npix * views.size());
        err.resize(npix * views.size());
        const rtw_adaptive ad{m_adMinSpp, m_adStepSpp, m_adThreshold, 1};
        const int rc = rtw_views_adaptive(m_ctx, views.data(), views.size(), &vp, &ad, frames.data(), spp.data(), err.data(), &m_stats);
        if (rc != RTW_OK) die(m_ctx, "rtw_views_adaptive", rc);
        if (_verbose) {
            const double uniform = static_cast<double>(npix) * static_cast<double>(views.size()) * m_Ns;
            std::cerr << "INFO: adaptive: spp mean " << static_cast<double>(m_stats.samples) / (static_cast<double>(npix) * views.size()) << ", "
                      << 100.0 * (1.0 - static_cast<double>(m_stats.samples) / uniform) << " % of uniform " << m_Ns << " spp saved" << std::endl;
        }
    } else {
        const int rc = rtw_views(m_ctx, views.data(), views.size(), &vp, frames.data(), &m_stats);
        if (rc != RTW_OK) die(m_ctx, "rtw_views", rc);
    }
    if (_verbose) {
        const double s = m_stats.seconds > 0 ? m_stats.seconds : 1e-9;
        std::cerr << "INFO: orbit: " << views.size() << " views, " << m_stats.samples << " samples, " << m_stats.segments << " segments, "
                  << m_stats.shadow_rays << " shadow rays in " << m_stats.seconds << " s on the GPU = " << m_stats.samples / s / 1e6 << " Msamples/s"
                  << std::endl;
    }
    const bool guidedDenoise = m_guided && m_denoiseIterations > 0;
    const bool guides = !m_aovPrefix.empty() || guidedDenoise;
    std::vector<float> albedo, normal, depth;
    if (guides) {  // renderFrame's guide layers, for every view in one call
        albedo.resize(frame * views.size());
        normal.resize(frame * views.size());
        depth.resize(npix * views.size());
        rtw_view_params g = vp;
        g.spp = m_guideSpp > 0 ? m_guideSpp : std::min(m_Ns, 16);
        rtw_guides out{albedo.data(), normal.data(), depth.data(), nullptr};
        rtw_stats gs{};
        const int grc = rtw_views_guides(m_ctx, views.data(), views.size(), &g, &out, &gs);
        if (grc != RTW_OK) die(m_ctx, "rtw_views_guides", grc);
        if (_verbose) std::cerr << "INFO: guides: " << views.size() << " views, " << g.spp << " spp in " << gs.seconds << " s on the GPU" << std::endl;
    }
    if (guidedDenoise) {  // renderFrame's denoiser pass: the display encoding in, linear values back, every view on its own
        std::vector<float> enc(frames.size()), filtered(frames.size());
        for (size_t i = 0; i < enc.size(); i++) {
            float c = frames[i];
            if ((i & 3) != 3) { c = !(c == c) || c < 0.f ? 0.f : (c > 1.f ? 1.f : c); c = std::sqrt(c); }
            enc[i] = c;
        }
        const int drc = rtw_denoise_views(m_ctx, enc.data(), albedo.data(), normal.data(), filtered.data(), views.size(), m_Nx, m_Ny, m_denoiseIterations,
                                          m_denoiseSigma, kDenoiseSigmaAlbedo, kDenoiseSigmaNormal);
        if (drc != RTW_OK) die(m_ctx, "rtw_denoise_views", drc);
        for (size_t i = 0; i < enc.size(); i++) frames[i] = (i & 3) != 3 ? filtered[i] * filtered[i] : filtered[i];
    }
    for (size_t k = 0; k < views.size(); k++) {
        auto slice = [k](const std::vector<float>& all, size_t each, std::vector<float>& one) {
            one.assign(all.begin() + static_cast<std::ptrdiff_t>(k * each), all.begin() + static_cast<std::ptrdiff_t>((k + 1) * each));
        };
        slice(frames, frame, m_hostBuffer);
        if (guides) { slice(albedo, frame, m_albedo); slice(normal, frame, m_normal); slice(depth, npix, m_depth); }
        if (m_adaptive) {  // what writeGuides puts beside the guides: the view's sample counts and errors
            m_sppMap.assign(spp.begin() + static_cast<std::ptrdiff_t>(k * npix), spp.begin() + static_cast<std::ptrdiff_t>((k + 1) * npix));
            slice(err, npix, m_errMap);
        }
        onFrame(static_cast<int>(k));
    }
}

// The frame through an accumulation session (rtw.h rtw_accum_*): adds of m_progStep samples (or one add), the frame read back after
// each, the state loaded from / written to a file. The session's cap is the largest there is (it costs nothing), so that a
// checkpoint can be resumed to any total.
void Director::renderSession(const rtw_params& frame) {
    auto bad = [](const std::string& what) {
        std::cerr << "ERROR: " << what << std::endl;
        std::exit(EXIT_FAILURE);
    };
    if (m_Ns % RTW_SUM_BLOCK != 0 || m_progStep < 0 || m_progStep % RTW_SUM_BLOCK != 0)
        bad("-progressive / -checkpoint / -resume need -ns (and the -progressive step) to be multiples of " + std::to_string(RTW_SUM_BLOCK));
    if (m_devices.size() > 1)
        std::cerr << "WARNING: -progressive / -checkpoint / -resume render on the first of the " << m_devices.size()
                  << " devices alone (a session is not sharded across devices)" << std::endl;
    rtw_params p = frame;
    p.spp = rtwk::kAccumCapMax;
    rtw_accum_info info{};
    int rc = RTW_OK;
    if (!m_resume.empty()) {
        std::ifstream f(m_resume, std::ios::binary);
        std::vector<char> blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (!f || blob.empty()) bad("cannot read the checkpoint " + m_resume);
        rc = rtw_accum_restore(m_ctx, blob.data(), blob.size());
        if (rc != RTW_OK) die(m_ctx, "rtw_accum_restore", rc);
        rc = rtw_accum_status(m_ctx, &info);
        if (rc != RTW_OK) die(m_ctx, "rtw_accum_status", rc);
        const rtw_params& q = info.params;
        if (q.width != p.width || q.height != p.height || q.max_depth != p.max_depth || q.seed != p.seed || q.row0 != p.row0 || q.row1 != p.row1 ||
            q.rng_kind != p.rng_kind || q.sample_offset != p.sample_offset || q.row_stride != p.row_stride || q.estimator != p.estimator || info.flags != 0)
            bad("the checkpoint " + m_resume + " was rendered with other parameters (" + std::to_string(q.width) + "x" + std::to_string(q.height) + ", depth " +
                std::to_string(q.max_depth) + ", seed " + std::to_string(q.seed) + ", rng " + std::to_string(q.rng_kind) + ", estimator " +
                std::to_string(q.estimator) + ")");
        if (info.done > m_Ns) bad("the checkpoint " + m_resume + " holds " + std::to_string(info.done) + " samples per pixel, more than -ns " + std::to_string(m_Ns));
        if (_verbose) std::cerr << "INFO: resumed " << m_resume << " at " << info.done << " spp" << std::endl;
    } else {
        rc = rtw_accum_begin(m_ctx, &p, 0);
        if (rc != RTW_OK) die(m_ctx, "rtw_accum_begin", rc);
    }
    m_stats = rtw_stats{};
    int done = info.done;
    bool fresh = false;  // m_hostBuffer holds the frame of `done` samples
    while (done < m_Ns) {
        const int n = m_progStep > 0 ? std::min(m_progStep, m_Ns - done) : m_Ns - done;
        rtw_stats st{};
        rc = rtw_accum_add(m_ctx, n, &st);
        if (rc != RTW_OK) die(m_ctx, "rtw_accum_add", rc);
        done += n;
        m_stats.samples += st.samples; m_stats.segments += st.segments; m_stats.shadow_rays += st.shadow_rays;
        m_stats.algorithmic_bytes += st.algorithmic_bytes; m_stats.bounce_launches += st.bounce_launches;
        m_stats.seconds += st.seconds; m_stats.bounce_seconds += st.bounce_seconds;
        for (int k = 0; k < RTW_K_COUNT; k++) {
            m_stats.kernel_seconds[k] += st.kernel_seconds[k]; m_stats.kernel_launches[k] += st.kernel_launches[k];
            m_stats.kernel_segments[k] += st.kernel_segments[k];
        }
        fresh = false;
        if (m_progStep > 0) {
            rc = rtw_accum_read(m_ctx, m_hostBuffer.data(), nullptr);
            if (rc != RTW_OK) die(m_ctx, "rtw_accum_read", rc);
            fresh = true;
            if (_verbose) std::cerr << "INFO: progressive: " << done << " of " << m_Ns << " spp" << std::endl;
            if (m_onFrame) m_onFrame(done);
        }
    }
    if (!fresh) {
        if (done <= 0) bad("nothing to render");
        rc = rtw_accum_read(m_ctx, m_hostBuffer.data(), nullptr);
        if (rc != RTW_OK) die(m_ctx, "rtw_accum_read", rc);
    }
    if (!m_checkpoint.empty()) {
        rc = rtw_accum_status(m_ctx, &info);
        if (rc != RTW_OK) die(m_ctx, "rtw_accum_status", rc);
        std::vector<char> blob(static_cast<size_t>(info.state_bytes));
        rc = rtw_accum_save(m_ctx, blob.data(), blob.size());
        if (rc != RTW_OK) die(m_ctx, "rtw_accum_save", rc);
        std::ofstream f(m_checkpoint, std::ios::binary);
        f.write(blob.data(), static_cast<std::streamsize>(blob.size()));
        if (!f) bad("cannot write the checkpoint " + m_checkpoint);
        if (_verbose) std::cerr << "INFO: checkpoint " << m_checkpoint << ": " << done << " spp, " << blob.size() << " bytes" << std::endl;
    }
    rc = rtw_accum_end(m_ctx);
    if (rc != RTW_OK) die(m_ctx, "rtw_accum_end", rc);
}

// P3 ASCII PPM on stdout, rows top to bottom, gamma 2 then int(255.99*clamp) — Director.cpp:1010-1031.
// The reference applies sqrt on the device (raygen.cu:151-155); rtw_render returns linear radiance,
// so the square root is taken here.
void Director::printPPM() {
    std::cout << "P3\n" << m_Nx << " " << m_Ny << "\n255\n";
    auto enc = [](float c) {
        float g = std::sqrt(c);
        g = g < 0.f ? 0.f : (g > 1.f ? 1.f : g);
        if (!(g == g)) g = 0.f;
        return static_cast<int>(255.99f * g);
    };
    std::string line;
    for (int j = m_Ny - 1; j >= 0; j--) {
        line.clear();
        for (int i = 0; i < m_Nx; i++) {
            const float* px = &m_hostBuffer[(static_cast<size_t>(m_Nx) * j + i) * 4];
            line += std::to_string(enc(px[0]));
            line += ' ';
            line += std::to_string(enc(px[1]));
            line += ' ';
            line += std::to_string(enc(px[2]));
            line += '\n';
        }
        std::cout << line;
    }
}

bool Director::writeBinaryPPM(const std::string& path) const {
    std::ofstream f(path, std::ios::binary);
    if (!f) return false;
    f << "P6\n" << m_Nx << " " << m_Ny << "\n255\n";
    auto enc = [](float c) {
        float g = std::sqrt(c);
        g = g < 0.f ? 0.f : (g > 1.f ? 1.f : g);
        if (!(g == g)) g = 0.f;
        return static_cast<unsigned char>(static_cast<int>(255.99f * g));
    };
    std::vector<unsigned char> row(static_cast<size_t>(m_Nx) * 3);
    for (int j = m_Ny - 1; j >= 0; j--) {  // the buffer is bottom-up like the reference's, image files are top-down
        for (int i = 0; i < m_Nx; i++) {
            const float* px = &m_hostBuffer[(static_cast<size_t>(m_Nx) * j + i) * 4];
            row[3 * i] = enc(px[0]); row[3 * i + 1] = enc(px[1]); row[3 * i + 2] = enc(px[2]);
        }
        f.write(reinterpret_cast<const char*>(row.data()), static_cast<std::streamsize>(row.size()));
    }
    return static_cast<bool>(f);
}

bool Director::writePFM(const std::string& path) const {
    return rtwhost::writePfm(path, m_hostBuffer.data(), m_Nx, m_Ny, 4, 3);  // linear radiance, little-endian, rows bottom-up
}

// One text line per sample and per vertex; every float as the 8 hex digits of its bits, then %.9g.
bool Director::writePaths(int x, int y, const std::string& path) {
    if (x < 0 || x >= m_Nx || y < 0 || y >= m_Ny) {
        std::cerr << "ERROR: -paths pixel (" << x << ", " << y << ") outside the " << m_Nx << 'x' << m_Ny << " frame" << std::endl;
        return false;
    }
    rtw_view view{};
    view.camera = m_camera;
    view.camera_type = m_blobCameraType;
    view.seed = m_seed;
    rtw_view_params vp{};
    vp.width = m_Nx; vp.height = m_Ny; vp.spp = m_Ns; vp.max_depth = m_maxRayDepth;
    vp.rng_kind = m_rngKind; vp.sample_offset = 0; vp.estimator = m_estimator;
    const size_t K = static_cast<size_t>(m_maxRayDepth);
    std::vector<rtw_path_head> heads(static_cast<size_t>(m_Ns));
    std::vector<rtw_path_vertex> vertices(heads.size() * K);
    const uint64_t first = static_cast<uint64_t>(y) * static_cast<uint64_t>(m_Nx) + static_cast<uint64_t>(x);
    const int rc = rtw_paths_views(m_ctx, &view, 1, &vp, first, 1, m_maxRayDepth, heads.data(), vertices.data(), nullptr);
    if (rc != RTW_OK) die(m_ctx, "rtw_paths_views", rc);
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    auto put = [&](const char* name, const float* v, int n) {
        std::fprintf(f, " %s", name);
        for (int i = 0; i < n; i++) {
            uint32_t bits;
            std::memcpy(&bits, v + i, sizeof bits);
            std::fprintf(f, " %08x %.9g", bits, static_cast<double>(v[i]));
        }
    };
    size_t brightest = 0;
    float top = -1.f;
    for (size_t s = 0; s < heads.size(); s++) {
        const rtw_path_head& h = heads[s];
        std::fprintf(f, "sample %u key %u segments %d shadow_rays %d", h.sample, h.key, h.segments, h.shadow_rays);
        put("gather_time", &h.gather_time, 1);
        put("radiance", h.radiance, 3);
        std::fputc('\n', f);
        const size_t m = std::min(static_cast<size_t>(std::max(h.segments, 0)), K);
        for (size_t j = 0; j < m; j++) {
            const rtw_path_vertex& v = vertices[s * K + j];
            std::fprintf(f, "vertex %u %zu prim %d flags %u", h.sample, j, v.prim, v.flags);
            put("o", v.o, 3); put("t", &v.t, 1); put("d", v.d, 3); put("contribution", v.contribution, 3);
            put("throughput", v.throughput, 3); put("ray_time", &v.ray_time, 1);
            std::fputc('\n', f);
        }
        const float lum = 0.2126f * h.radiance[0] + 0.7152f * h.radiance[1] + 0.0722f * h.radiance[2];
        if (lum > top) { top = lum; brightest = s; }
    }
    const bool ok = std::fclose(f) == 0;
    if (_verbose)
        std::cerr << "INFO: Pixel (" << x << ", " << y << "): the brightest of " << heads.size() << " samples is sample " << heads[brightest].sample
                  << " (luminance " << top << ", " << heads[brightest].segments << " segments)" << std::endl;
    return ok;
}

bool Director::writeGuides(const std::string& prefix) const {
    if (m_albedo.empty()) return false;
    if (m_adaptive && (!rtwhost::writePfm(prefix + "_spp.pfm", m_sppMap.data(), m_Nx, m_Ny, 1, 1) ||
                       !rtwhost::writePfm(prefix + "_error.pfm", m_errMap.data(), m_Nx, m_Ny, 1, 1)))
        return false;
    return rtwhost::writePfm(prefix + "_albedo.pfm", m_albedo.data(), m_Nx, m_Ny, 4, 3) &&
           rtwhost::writePfm(prefix + "_normal.pfm", m_normal.data(), m_Nx, m_Ny, 4, 3) &&
           rtwhost::writePfm(prefix + "_depth.pfm", m_depth.data(), m_Nx, m_Ny, 1, 1);
}

// PNG without a compression library: zlib stream of stored deflate blocks (the reference vendors stb_image_write.h for
// this and never calls it, main.cpp:9). CRC-32 and Adler-32 as in RFC 1950 / the PNG specification.
bool Director::writePNG(const std::string& path) const {
    std::ofstream f(path, std::ios::binary);
    if (!f) return false;
    uint32_t crcTable[256];
    for (uint32_t n = 0; n < 256; n++) {
        uint32_t c = n;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
        crcTable[n] = c;
    }
    auto be32 = [](std::vector<unsigned char>& v, uint32_t x) {
        v.push_back(static_cast<unsigned char>(x >> 24)); v.push_back(static_cast<unsigned char>(x >> 16));
        v.push_back(static_cast<unsigned char>(x >> 8)); v.push_back(static_cast<unsigned char>(x));
    };
    auto chunk = [&](const char* type, const std::vector<unsigned char>& data) {
        std::vector<unsigned char> c;
        be32(c, static_cast<uint32_t>(data.size()));
        c.insert(c.end(), type, type + 4);
        c.insert(c.end(), data.begin(), data.end());
        uint32_t crc = 0xffffffffu;
        for (size_t i = 4; i < c.size(); i++) crc = crcTable[(crc ^ c[i]) & 0xffu] ^ (crc >> 8);
        be32(c, crc ^ 0xffffffffu);
        f.write(reinterpret_cast<const char*>(c.data()), static_cast<std::streamsize>(c.size()));
    };
    auto enc = [](float c) {
        float g = std::sqrt(c);
        g = g < 0.f ? 0.f : (g > 1.f ? 1.f : g);
        if (!(g == g)) g = 0.f;
        return static_cast<unsigned char>(static_cast<int>(255.99f * g));
    };
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    f.write(reinterpret_cast<const char*>(sig), 8);
    std::vector<unsigned char> ihdr;
    be32(ihdr, static_cast<uint32_t>(m_Nx)); be32(ihdr, static_cast<uint32_t>(m_Ny));
    ihdr.push_back(8); ihdr.push_back(2); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);  // 8 bit, RGB, no interlace
    chunk("IHDR", ihdr);
    // raw scanlines (filter byte 0 + RGB), top row first
    std::vector<unsigned char> raw;
    raw.reserve((static_cast<size_t>(m_Nx) * 3 + 1) * m_Ny);
    for (int j = m_Ny - 1; j >= 0; j--) {
        raw.push_back(0);
        for (int i = 0; i < m_Nx; i++) {
            const float* px = &m_hostBuffer[(static_cast<size_t>(m_Nx) * j + i) * 4];
            raw.push_back(enc(px[0])); raw.push_back(enc(px[1])); raw.push_back(enc(px[2]));
        }
    }
    std::vector<unsigned char> z;
    z.push_back(0x78); z.push_back(0x01);
    uint32_t a = 1, b = 0;
    for (size_t pos = 0; pos < raw.size() || pos == 0;) {
        const size_t n = std::min<size_t>(65535, raw.size() - pos);
        z.push_back(pos + n >= raw.size() ? 1 : 0);  // BFINAL, BTYPE = 00 (stored)
        z.push_back(static_cast<unsigned char>(n)); z.push_back(static_cast<unsigned char>(n >> 8));
        z.push_back(static_cast<unsigned char>(~n)); z.push_back(static_cast<unsigned char>((~n) >> 8));
        for (size_t i = 0; i < n; i++) { a = (a + raw[pos + i]) % 65521u; b = (b + a) % 65521u; }
        z.insert(z.end(), raw.begin() + static_cast<std::ptrdiff_t>(pos), raw.begin() + static_cast<std::ptrdiff_t>(pos + n));
        pos += n;
        if (n == 0) break;
    }
    be32(z, (b << 16) | a);
    chunk("IDAT", z);
    chunk("IEND", {});
    return static_cast<bool>(f);
}
