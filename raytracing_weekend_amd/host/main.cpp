// main.cpp — command-line front end, same flow and flags as the reference (RestOfLife/main.cpp:29-165):
//   -s scene  -ns samples  -dx width  -dy height  -h  -v  -g
// plus what the benchmark configurations need and the reference hard-wires:
//   -d depth (reference: 20, Director.cpp:42)   -seed N   -rng philox|lcg   -gpu id   -gpus N   -o file.ppm|file.png|file.pfm
//   -progressive N   -checkpoint file   -resume file   (accumulation sessions: previews, checkpoints, resumed renders)
//   -orbit N   (a turntable of N views through rtw_views, or rtw_views_adaptive with -adaptive, one file per view)
//   -paths X Y FILE   (the samples of one pixel of the frame replayed through rtw_paths_views, as text)
// The reference's resolution / sample clamps (main.cpp:21-27) are widened so that 200x200 and
// 7680x4320 are reachable, and its scene range bug (only scene 4 selectable, main.cpp:69) is not kept.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>

#include "Director.h"
#include "InputParser.h"

#define Nx_MIN (16)
#define Ny_MIN (16)
#define Nx_MAX (16384)
#define Ny_MAX (16384)
#define Nscene_MAX (4)
#define Ns_MAX (1024 * 1024)

namespace {
// parse an integer option; returns false (and leaves `out`) when absent or malformed
bool intOption(const InputParser& in, const char* flag, const char* what, int& out) {
    const std::string& v = in.getCmdOption(flag);
    if (v.empty()) return false;
    try {
        out = std::stoi(v, nullptr, 0);
        return true;
    } catch (const std::exception&) {
        std::cerr << "Invalid " << what << ": " << v << std::endl;
        return false;
    }
}
int clampWarn(const char* what, int x, int lo, int hi) {
    if (x >= lo && x <= hi) return x;
    int y = x < lo ? lo : hi;
    std::cerr << "WARNING: " << what << " " << x << " out of range. Using a value of " << y << std::endl;
    return y;
}
}  // namespace

int main(int argc, char* argv[]) {
    int Nx = 1200, Ny = 600, Nscene = 4, Ns = 20, depth = 20, gpu = 0, gpus = 1;  // the reference's defaults (main.cpp:32-37)
    uint32_t seed = 0x6314759u;
    int rng = RTW_RNG_PHILOX;

    InputParser cl_input(argc, argv);
    if (cl_input.cmdOptionExists("-h") || cl_input.cmdOptionExists("--help")) {
        std::cerr << "\n HELP - " << argv[0] << "\n"
                  << R"(
    -s N           Scene Selection number N (0 Cornell box, 1 moving spheres, 2 spheres with a light,
                   3 Cornell box with volumes, 4 The Next Week final scene)
    -ns N          Sample each pixel N times (N: 1, 2, etc.)
    -dx Nx         Output image width (x dimension)
    -dy Ny         Output image height (y dimension)
    -d N           Maximum path depth (reference: 20)
    -seed N        RNG seed
    -rng K         philox (default) or lcg (the reference's tea+lcg generator)
    -denoise N     N passes (1..8) of the a-trous filter that stands in for the reference's AI denoiser (default: off)
    -est K         reference (default: the reference's estimator, quirks included), corrected, brute
                   (corrected without light sampling) or mixture (the book's 50/50 mixture of light and cosine sampling)
    -cam K         perspective (default), environment or orthographic (the reference's two unused camera kinds, scene/ioCamera.h:118-179)
    -guided        With -denoise: steer the filter with the albedo and normal guides (rtw_denoise_guided)
    -aov PREFIX    Also write the guide buffers: PREFIX_albedo.pfm, PREFIX_normal.pfm (PF) and PREFIX_depth.pfm (Pf)
    -guide_spp N   Samples per pixel of the guide buffers (default: min(Ns, 16))
    -adaptive T    Adaptive sampling: a pixel stops once its error estimate (standard error of the display value) is below T;
                   -ns becomes the cap (a multiple of 16). With -aov also PREFIX_spp.pfm and PREFIX_error.pfm (Pf)
    -min_spp N     With -adaptive: samples every pixel gets first (default 64; a multiple of 16, at least 32)
    -step N        With -adaptive: samples added per checkpoint (default: half of what a pixel has, rounded up to 16)
    -progressive N Render in adds of N samples (a multiple of 16, as -ns must then be) and rewrite the -o file after every add;
                   the final file is the file of the same command without the flag
    -checkpoint F  Write the accumulation session's state to F when the render ends (-ns a multiple of 16)
    -resume F      Start from the state in F instead of from zero: -ns is the new total (at least what F holds); scene, size
                   and parameters must be those F was rendered with
    -orbit N       Render a turntable of N views in one call (rtw_views): view 0 is the scene's camera, view k that camera turned by
                   360 k / N degrees about its vertical axis through the centre of its frame. Needs -o NAME.ext and writes
                   NAME_000.ext, NAME_001.ext, ... with the writer of that extension; -seed applies to every view. With
                   -aov PREFIX also PREFIX_000_albedo.pfm, PREFIX_000_normal.pfm, PREFIX_000_depth.pfm, ... (rtw_views_guides);
                   with -denoise N -guided every view is filtered on its own (rtw_denoise_views). With -adaptive T [-min_spp M]
                   [-step N] every view is sampled to the noise target (rtw_views_adaptive) and -aov PREFIX also writes
                   PREFIX_000_spp.pfm and PREFIX_000_error.pfm, ... It does not combine with -denoise without -guided,
                   -progressive, -checkpoint or -resume
    -paths X Y F   After the render, replay the -ns samples of pixel (X, Y) of the frame (Y counts rows from the bottom, as a PFM
                   does) and write them to F (rtw_paths_views): one line per sample - its index, stream key, segment and shadow-ray
                   counts, gather time and radiance - and one per vertex of its path; every float as the 8 hex digits of its bits
                   and in decimal. The samples' radiances, added in the library's order and divided by -ns, are the frame's
                   pixel. With -v the brightest sample is named. It does not combine with -orbit, -adaptive, -denoise or the
                   session flags
    -gpu N         Device ordinal (the first one with -gpus)
    -gpus N        Render on N GPUs of this node: interleaved row shards, one gather onto the first device (default 1)
    -o FILE        Write FILE instead of ASCII P3 on stdout: *.ppm = binary P6, *.png = 8-bit PNG, *.pfm = linear float PFM

    -h             This help message.
    -v             Verbose output.
    -g             Debug output.

)";
        return EXIT_SUCCESS;
    }
    const bool Qverbose = cl_input.cmdOptionExists("-v");
    const bool Qdebug = cl_input.cmdOptionExists("-g");

    int x;
    if (intOption(cl_input, "-s", "scene number", x)) {
        if (x >= 0 && x <= Nscene_MAX) Nscene = x;
        else {
            std::cerr << "WARNING: Scene number " << x << " out of range. Maximum scene number: " << Nscene_MAX << std::endl;
            std::cerr << "WARNING: Using a scene value of " << Nscene << std::endl;
        }
    }
    if (intOption(cl_input, "-ns", "number of samples", x)) Ns = clampWarn("Number of samples", x, 1, Ns_MAX);
    if (intOption(cl_input, "-dx", "image width (-dx)", x)) Nx = clampWarn("Width (-dx)", x, Nx_MIN, Nx_MAX);
    if (intOption(cl_input, "-dy", "image height (-dy)", x)) Ny = clampWarn("Height (-dy)", x, Ny_MIN, Ny_MAX);
    if (intOption(cl_input, "-d", "depth (-d)", x)) depth = clampWarn("Depth (-d)", x, 1, 1 << 20);
    if (intOption(cl_input, "-gpu", "device (-gpu)", x)) gpu = x;
    if (intOption(cl_input, "-gpus", "number of devices (-gpus)", x)) gpus = clampWarn("Number of devices (-gpus)", x, 1, 64);
    if (intOption(cl_input, "-seed", "seed", x)) seed = static_cast<uint32_t>(x);
    const std::string& rngName = cl_input.getCmdOption("-rng");
    if (rngName == "lcg") rng = RTW_RNG_TEA_LCG;
    else if (!rngName.empty() && rngName != "philox") std::cerr << "WARNING: unknown -rng " << rngName << ", using philox" << std::endl;

    int estimator = RTW_EST_REFERENCE;
    const std::string& estName = cl_input.getCmdOption("-est");
    if (estName == "corrected") estimator = RTW_EST_CORRECTED;
    else if (estName == "brute") estimator = RTW_EST_CORRECTED_NO_NEE;
    else if (estName == "mixture") estimator = RTW_EST_MIXTURE;
    else if (!estName.empty() && estName != "reference") std::cerr << "WARNING: unknown -est " << estName << ", using reference" << std::endl;

    int camKind = RTW_CAM_PERSPECTIVE;
    const std::string& camName = cl_input.getCmdOption("-cam");
    if (camName == "environment") camKind = RTW_CAM_ENVIRONMENT;
    else if (camName == "orthographic") camKind = RTW_CAM_ORTHOGRAPHIC;
    else if (!camName.empty() && camName != "perspective") std::cerr << "WARNING: unknown -cam " << camName << ", using perspective" << std::endl;

    Director director(Qverbose, Qdebug);
    director.setCameraKind(camKind);
    // RTW_SAME_DEVICE=1 (tests on a one-GPU box): all -gpus N shards render on device -gpu
    if (gpus > 1) director.setDevices(gpus, gpu, std::getenv("RTW_SAME_DEVICE") != nullptr);
    else director.setDevice(gpu);
    director.setMaxDepth(depth);
    director.setSeed(seed);
    director.setRngKind(rng);
    director.setEstimator(estimator);
    if (intOption(cl_input, "-denoise", "denoise passes", x)) director.setDenoise(clampWarn("Denoise passes", x, 0, 8), 0.5f);
    const std::string& aovPrefix = cl_input.getCmdOption("-aov");
    int guideSpp = 0;
    if (intOption(cl_input, "-guide_spp", "guide samples (-guide_spp)", x)) guideSpp = clampWarn("Guide samples (-guide_spp)", x, 1, Ns_MAX);
    director.setGuides(aovPrefix, guideSpp, cl_input.cmdOptionExists("-guided"));
    if (cl_input.cmdOptionExists("-adaptive")) {
        const std::string& t = cl_input.getCmdOption("-adaptive");
        char* end = nullptr;
        const float thr = std::strtof(t.c_str(), &end);
        if (t.empty() || *end != '\0') {
            std::cerr << "ERROR: -adaptive needs a threshold (a number >= 0)" << std::endl;
            return EXIT_FAILURE;
        }
        int minSpp = 64, step = 0;
        if (intOption(cl_input, "-min_spp", "adaptive minimum samples (-min_spp)", x)) minSpp = x;
        if (intOption(cl_input, "-step", "adaptive step (-step)", x)) step = x;
        director.setAdaptive(thr, minSpp, step);
    }

    std::string outPath = cl_input.getCmdOption("-o");
    auto writeOutput = [&]() {
        auto ends = [&](const char* ext) { return outPath.size() > 4 && outPath.compare(outPath.size() - 4, 4, ext) == 0; };
        return ends(".pfm") ? director.writePFM(outPath) : ends(".png") ? director.writePNG(outPath) : director.writeBinaryPPM(outPath);
    };
    if (cl_input.cmdOptionExists("-progressive")) {
        int step = 0;
        if (!intOption(cl_input, "-progressive", "progressive step (-progressive)", step) || step <= 0) {
            std::cerr << "ERROR: -progressive needs a sample count (a positive multiple of 16)" << std::endl;
            return EXIT_FAILURE;
        }
        director.setProgressive(step, [&](int) {
            if (!outPath.empty() && !writeOutput()) std::cerr << "WARNING: cannot write " << outPath << std::endl;
        });
    }
    if (cl_input.cmdOptionExists("-checkpoint")) {
        const std::string& f = cl_input.getCmdOption("-checkpoint");
        if (f.empty()) { std::cerr << "ERROR: -checkpoint needs a file name" << std::endl; return EXIT_FAILURE; }
        director.setCheckpoint(f);
    }
    if (cl_input.cmdOptionExists("-resume")) {
        const std::string& f = cl_input.getCmdOption("-resume");
        if (f.empty()) { std::cerr << "ERROR: -resume needs a file name" << std::endl; return EXIT_FAILURE; }
        director.setResume(f);
    }

    int orbit = 0;
    if (cl_input.cmdOptionExists("-orbit")) {
        if (!intOption(cl_input, "-orbit", "number of views (-orbit)", orbit) || orbit <= 0) {
            std::cerr << "ERROR: -orbit needs a number of views (a positive integer)" << std::endl;
            return EXIT_FAILURE;
        }
        if (outPath.empty()) { std::cerr << "ERROR: -orbit needs -o NAME.ext (it writes NAME_000.ext ...)" << std::endl; return EXIT_FAILURE; }
        for (const char* flag : {"-progressive", "-checkpoint", "-resume"})
            if (cl_input.cmdOptionExists(flag)) { std::cerr << "ERROR: -orbit does not combine with " << flag << std::endl; return EXIT_FAILURE; }
        // the views' denoiser is the guided one (rtw_denoise_views)
        if (cl_input.cmdOptionExists("-denoise") && !cl_input.cmdOptionExists("-guided")) {
            std::cerr << "ERROR: -orbit does not combine with -denoise without -guided" << std::endl;
            return EXIT_FAILURE;
        }
        if (cl_input.cmdOptionExists("-aov") && aovPrefix.empty()) { std::cerr << "ERROR: -aov needs a prefix" << std::endl; return EXIT_FAILURE; }
    }

    int pathsX = 0, pathsY = 0;
    std::string pathsFile;
    if (cl_input.cmdOptionExists("-paths")) {
        // -paths X Y FILE: three values after the flag
        int at = 0;
        for (int i = 1; i < argc; i++)
            if (std::string(argv[i]) == "-paths") at = i;
        bool ok = at > 0 && at + 3 < argc && argv[at + 3][0] != '\0';
        if (ok) {
            try {
                pathsX = std::stoi(argv[at + 1], nullptr, 0);
                pathsY = std::stoi(argv[at + 2], nullptr, 0);
                pathsFile = argv[at + 3];
            } catch (const std::exception&) {
                ok = false;
            }
        }
        if (!ok) { std::cerr << "ERROR: -paths needs a pixel and a file name: -paths X Y FILE" << std::endl; return EXIT_FAILURE; }
        for (const char* flag : {"-orbit", "-adaptive", "-denoise", "-progressive", "-checkpoint", "-resume"})
            if (cl_input.cmdOptionExists(flag)) { std::cerr << "ERROR: -paths does not combine with " << flag << std::endl; return EXIT_FAILURE; }
        if (pathsX < 0 || pathsX >= Nx || pathsY < 0 || pathsY >= Ny) {
            std::cerr << "ERROR: -paths pixel (" << pathsX << ", " << pathsY << ") outside the " << Nx << 'x' << Ny << " frame" << std::endl;
            return EXIT_FAILURE;
        }
    }

    auto start = std::chrono::system_clock::now();
    director.init(Nx, Ny, Ns);
    if (Qverbose) {
        std::cerr << "INFO: Output image dimensions: " << Nx << 'x' << Ny << std::endl;
        std::cerr << "INFO: Number of rays sent per pixel: " << Ns << std::endl;
        std::cerr << "INFO: Scene number selected: " << Nscene << std::endl;
    }
    director.createScene(Nscene);
    if (orbit > 0) {
        const size_t dot = outPath.find_last_of('.');
        const std::string stem = dot == std::string::npos ? outPath : outPath.substr(0, dot), ext = dot == std::string::npos ? "" : outPath.substr(dot);
        const std::string whole = outPath;
        bool ok = true;
        director.renderOrbit(orbit, [&](int k) {
            char idx[16];
            std::snprintf(idx, sizeof idx, "_%03d", k);
            outPath = stem + idx + ext;  // (writeOutput picks the writer by the name's extension)
            if (!writeOutput()) { std::cerr << "ERROR: cannot write " << outPath << std::endl; ok = false; }
            if (!aovPrefix.empty() && !director.writeGuides(aovPrefix + idx)) {
                std::cerr << "ERROR: cannot write the guide files " << aovPrefix << idx << "_*.pfm" << std::endl;
                ok = false;
            }
        });
        outPath = whole;
        auto stop = std::chrono::system_clock::now();
        std::cerr << "INFO: Took " << std::chrono::duration<float>(stop - start).count() << " seconds." << std::endl;
        director.destroy();
        return ok ? EXIT_SUCCESS : EXIT_FAILURE;
    }
    director.renderFrame();
    auto stop = std::chrono::system_clock::now();
    std::cerr << "INFO: Took " << std::chrono::duration<float>(stop - start).count() << " seconds." << std::endl;

    if (outPath.empty()) {
        director.printPPM();
    } else {
        if (!writeOutput()) {
            std::cerr << "ERROR: cannot write " << outPath << std::endl;
            director.destroy();
            return EXIT_FAILURE;
        }
    }
    if (!pathsFile.empty() && !director.writePaths(pathsX, pathsY, pathsFile)) {
        std::cerr << "ERROR: cannot write " << pathsFile << std::endl;
        director.destroy();
        return EXIT_FAILURE;
    }
    if (!aovPrefix.empty() && !director.writeGuides(aovPrefix)) {
        std::cerr << "ERROR: cannot write the guide files " << aovPrefix << "_*.pfm" << std::endl;
        director.destroy();
        return EXIT_FAILURE;
    }
    director.destroy();
    return EXIT_SUCCESS;
}
