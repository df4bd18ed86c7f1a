// CPU check of the cut of an rtw_paths / rtw_paths_views host call into chunks of whole rays (raytracing_weekend_amd/csrc/
// rtw_paths_plan.h), compiled with g++ -fsanitize=address,undefined and run by tests/test_paths_cpu.py. Over n from 0 to 2^31 - 1,
// spp * K from 0 to 2^20 and budgets from 1 byte up: the chunks tile [0, n) without a gap or an overlap, every chunk fits the
// budget or is a single ray, the byte offsets of a chunk's heads and records are those of its first (ray, sample) pair, and nothing
// wraps 64 bits (every product is taken again in 128). Prints "paths_plan_check ok" and returns 0, or says what failed.
#include <cstdio>

#include "../../raytracing_weekend_amd/csrc/rtw_paths_plan.h"
using namespace rtwk;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

typedef unsigned __int128 u128;

// every chunk where there are few, else the first, the last and a spread of the ones between
static void check(uint64_t n, int32_t spp, int32_t K, uint64_t budget) {
    const PathsPlan pl = paths_plan(n, spp, K, budget);
    const u128 ray_bytes = (u128)(uint32_t)spp * (32 + (u128)(uint32_t)K * 64);
    CHECK((u128)paths_ray_bytes(spp, K) == ray_bytes);
    CHECK(pl.rays >= 1 && pl.rays <= (n > 0 ? n : 1));
    CHECK((u128)pl.rays * ray_bytes <= budget || pl.rays == 1);                          // it fits, or it is a single ray
    CHECK(pl.rays == (n > 0 ? n : 1) || (u128)(pl.rays + 1) * ray_bytes > budget);        // and no larger chunk would fit
    CHECK(pl.n_chunks == (n + pl.rays - 1) / pl.rays && (n == 0) == (pl.n_chunks == 0));
    CHECK((u128)pl.n_chunks * pl.rays >= n && (pl.n_chunks == 0 || (u128)(pl.n_chunks - 1) * pl.rays < n));
    const uint64_t step = pl.n_chunks <= 4096 ? 1 : pl.n_chunks / 1021;
    for (uint64_t c = 0; c < pl.n_chunks;) {
        const PathsChunk ch = paths_chunk(n, spp, K, pl, c);
        CHECK(ch.first == c * pl.rays && ch.count >= 1 && ch.first + ch.count <= n);      // it begins where the one before ends
        CHECK(ch.count == pl.rays || c + 1 == pl.n_chunks);                               // whole chunks but the last
        CHECK(c + 1 < pl.n_chunks || ch.first + ch.count == n);                           // the last one ends at n
        CHECK((u128)ch.count * ray_bytes <= budget || ch.count == 1);
        const u128 pairs = (u128)ch.first * (uint32_t)spp;
        CHECK((u128)ch.head_off == pairs * 32 && (u128)ch.vertex_off == pairs * (uint32_t)K * 64);
        // its last byte lies inside the caller's arrays, which are n * spp heads and n * spp * K records
        CHECK((u128)ch.head_off + (u128)ch.count * (uint32_t)spp * 32 <= (u128)n * (uint32_t)spp * 32);
        CHECK((u128)ch.vertex_off + (u128)ch.count * (uint32_t)spp * (uint32_t)K * 64 <= (u128)n * (uint32_t)spp * (uint32_t)K * 64);
        if (c + 1 < pl.n_chunks) {
            const PathsChunk next = paths_chunk(n, spp, K, pl, c + 1);
            CHECK(next.first == ch.first + ch.count);
            CHECK((u128)next.head_off == (u128)ch.head_off + (u128)ch.count * (uint32_t)spp * 32);
        }
        if (c + 1 == pl.n_chunks) break;
        c = std::min<uint64_t>(c + step, pl.n_chunks - 1);
    }
    const PathsChunk past = paths_chunk(n, spp, K, pl, pl.n_chunks);
    CHECK(past.first == n && past.count == 0);
}

int main() {
    const uint64_t ns[] = {0, 1, 2, 3, 63, 64, 65, 1000, 65539, (1ull << 20) + 1, 0x7fffffffull};
    const int32_t spps[] = {1, 2, 3, 16, 48, 1024, 1 << 20};
    const int32_t Ks[] = {0, 1, 2, 8, 1024, 1 << 20};
    const uint64_t budgets[] = {1, 31, 32, 95, 96, 97, 336, 1000, 4096, 1ull << 20, 256ull << 20, 1ull << 40, ~0ull};
    for (uint64_t n : ns)
        for (int32_t spp : spps)
            for (int32_t K : Ks) {
                if ((u128)spp * (u128)(K > 0 ? K : 1) > (1u << 20)) continue;  // spp * K from 0 to 2^20
                if (!paths_pairs_ok(n, spp)) {                                  // a call the library refuses
                    CHECK((u128)n * (uint32_t)spp > kPathsMaxPairs);
                    continue;
                }
                CHECK((u128)n * (uint32_t)spp <= kPathsMaxPairs);
                for (uint64_t b : budgets) check(n, spp, K, b);
            }
    {   // by hand: 10 rays of 3 samples and 2 records each are 10 * 3 * (32 + 128) = 10 * 480 bytes
        CHECK(paths_ray_bytes(3, 2) == 480 && paths_ray_bytes(3, 0) == 96);
        const PathsPlan a = paths_plan(10, 3, 2, 480), b = paths_plan(10, 3, 2, 1680), c = paths_plan(10, 3, 2, 479), d = paths_plan(10, 3, 2, 1ull << 30);
        CHECK(a.rays == 1 && a.n_chunks == 10);   // one ray's bytes
        CHECK(b.rays == 3 && b.n_chunks == 4);    // 3.5 rays' bytes: three whole rays
        CHECK(c.rays == 1 && c.n_chunks == 10);   // less than one ray: one ray all the same
        CHECK(d.rays == 10 && d.n_chunks == 1);
        const PathsChunk last = paths_chunk(10, 3, 2, b, 3);
        CHECK(last.first == 9 && last.count == 1 && last.head_off == 27 * 32 && last.vertex_off == 27 * 2 * 64);
        // the largest call: 2^31 - 1 pairs of 2^20 records end below 2^58
        const PathsPlan big = paths_plan(2047, 1 << 20, 1, 1);
        const PathsChunk end = paths_chunk(2047, 1 << 20, 1, big, 2046);
        CHECK(big.rays == 1 && end.first == 2046 && end.vertex_off == 2046ull * (1ull << 20) * 64);
        CHECK(paths_pairs_ok(0x7fffffffull, 1) && !paths_pairs_ok(0x80000000ull, 1) && paths_pairs_ok(2047, 1 << 20) && !paths_pairs_ok(2048, 1 << 20));
        CHECK(paths_pairs_ok(0, 1 << 30) && !paths_pairs_ok(~0ull, 2));
    }
    if (fails) return 1;
    printf("paths_plan_check ok\n");
    return 0;
}
