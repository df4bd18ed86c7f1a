// ref_programs_main.cpp — TEST INFRASTRUCTURE. Stand-alone driver of ref_programs_wrap.cpp for sanitizer runs on the CPU
// (`make -C oracle ref_asan` builds both with -fsanitize=address,undefined): the emulation carries raw pointers through
// payload words. Usage: ref_programs_asan SCENE.blob WIDTH HEIGHT DEPTH   (a blob as abi.build_scene writes it).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" int ref_launch(const void* blob, size_t bytes, int width, int height, int max_depth, float* frame, uint32_t* counts);
extern "C" int ref_launch_rows(const void* blob, size_t bytes, int width, int height, int row0, int row1, int max_depth, float* frame, float* linear,
                               uint32_t* counts);
extern "C" int ref_camera(const void* blob, size_t bytes, const float* s, const float* t, const uint32_t* seed, int n, float* origin, float* direction,
                          uint32_t* seed_out);
extern "C" int ref_texture(const void* blob, size_t bytes, int tex, const float* uv, const float* points, int n, float* rgb);
extern "C" int ref_intersect(const void* blob, size_t bytes, const float* rays, const float* ray_time, const float* gather_time, int n,
                             float* out11, int32_t* out_prim, int32_t* out_reported);

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s scene.blob width height depth\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint32_t> blob;
    uint32_t word;
    while (fread(&word, 4, 1, f) == 1) blob.push_back(word);
    fclose(f);
    const int w = atoi(argv[2]), h = atoi(argv[3]), depth = atoi(argv[4]);
    std::vector<float> frame((size_t)w * h * 4);
    std::vector<uint32_t> counts((size_t)w * h * 3);
    int rc = ref_launch(blob.data(), blob.size() * 4, w, h, depth, frame.data(), counts.data());
    if (rc) { fprintf(stderr, "ref_launch: %d\n", rc); return 1; }
    double sum = 0.0;
    unsigned long long trav = 0, shadow = 0, draws = 0;
    for (size_t i = 0; i < frame.size(); i++) sum += frame[i];
    for (size_t i = 0; i < counts.size(); i += 3) { trav += counts[i]; shadow += counts[i + 1]; draws += counts[i + 2]; }
    const float rays[16] = {278.f, 278.f, -800.f, 0.f, 0.f, 1.f, 1e-6f, 1e27f, 278.f, 278.f, -800.f, 0.3f, 0.1f, 1.f, 1e-6f, 1e27f};
    float out[22];
    int32_t prim[2], rep[2];
    rc = ref_intersect(blob.data(), blob.size() * 4, rays, nullptr, nullptr, 2, out, prim, rep);
    if (rc) { fprintf(stderr, "ref_intersect: %d\n", rc); return 1; }
    // the other entry points: a shard of rows with the linear sample, the camera callable, texture 0
    const int r0 = h / 3, r1 = h - h / 4;
    std::vector<float> part((size_t)w * (r1 - r0) * 4), lin((size_t)w * (r1 - r0) * 3);
    std::vector<uint32_t> pc((size_t)w * (r1 - r0) * 3);
    rc = ref_launch_rows(blob.data(), blob.size() * 4, w, h, r0, r1, depth, part.data(), lin.data(), pc.data());
    if (rc) { fprintf(stderr, "ref_launch_rows: %d\n", rc); return 1; }
    for (size_t i = 0; i < part.size(); i++)
        if (part[i] != frame[(size_t)r0 * w * 4 + i]) { fprintf(stderr, "rows differ from the frame at %zu\n", i); return 1; }
    const float cs[2] = {0.25f, 0.75f}, ct[2] = {0.5f, 0.125f};
    const uint32_t seeds[2] = {1u, 0xC0FFEEu};
    float co[6], cd[6], uv[4] = {0.f, 0.f, 0.5f, 0.5f}, pts[6] = {1.f, 2.f, 3.f, 100.f, 200.f, 300.f}, rgb[6];
    uint32_t so[2];
    rc = ref_camera(blob.data(), blob.size() * 4, cs, ct, seeds, 2, co, cd, so);
    if (rc) { fprintf(stderr, "ref_camera: %d\n", rc); return 1; }
    rc = ref_texture(blob.data(), blob.size() * 4, 0, uv, pts, 2, rgb);
    if (rc) { fprintf(stderr, "ref_texture: %d\n", rc); return 1; }
    printf("camera direction %.4f %.4f %.4f, texture 0 %.3f %.3f %.3f, linear[0] %.6f; ", cd[0], cd[1], cd[2], rgb[0], rgb[1], rgb[2], lin[0]);
    printf("frame sum %.6f, traversals %llu, shadow traversals %llu, rnd calls %llu; rays hit %d (t %.4f), %d (t %.4f)\n", sum, trav, shadow, draws,
           prim[0], out[0], prim[1], out[11]);
    return 0;
}
