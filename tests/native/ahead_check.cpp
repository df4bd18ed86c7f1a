// CPU check of k_path's camera-ray reserve and of its gated bounds test (raytracing_weekend_amd/csrc/rtw_ahead.h): a wave of 64 lanes
// runs k_path's loop - refill, fill phase, regeneration from the reserve, one segment, block and unit bookkeeping - over the header's
// functions, with random path lengths and a "ray" that is the triple (pixel, sample, unit it was generated in). A stand-alone program:
// tests/test_ahead_cpu.py builds it with g++ (once with -fsanitize=address,undefined) and runs it; it prints "ahead_check ok" and
// returns 0, or says what failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../raytracing_weekend_amd/csrc/rtw_ahead.h"

using namespace rtwk;

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (g_failed++ < 20) {                        \
                fprintf(stderr, "FAILED %s: ", #cond);    \
                fprintf(stderr, __VA_ARGS__);             \
                fprintf(stderr, "\n");                    \
            }                                             \
        }                                                 \
    } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545f4914f6cdd1dull) >> 32);
}

constexpr uint32_t kSB = RTW_SUM_BLOCK;
struct Entry { uint32_t pixel, sample, serial; };
struct Unit { uint32_t pixel, b, serial; };
struct Lane {
    bool need = true, alive = false;
    uint32_t pixel = 0, blk = 0, word = 0, s_cur = 0, left = 0, serial = 0, unit_lo = 0, expect = 0;
    Entry ring[kAheadMaxK] = {{~0u, ~0u, ~0u}, {~0u, ~0u, ~0u}, {~0u, ~0u, ~0u}};  // never cleared: a stale entry stays readable
};

// One launch of k_path: blocks [0, nbp) of a pass whose first block is block0 of a call of spp samples, n_pix pixels, units of ub
// blocks, mean path length `mean` segments. consumed[pixel * spp + sample] counts the camera paths started.
static void run_launch(uint32_t K, uint32_t spp, uint32_t ub, uint32_t block0, uint32_t nbp, uint32_t n_pix, uint32_t mean, std::vector<uint32_t>& consumed,
                       uint32_t& serial, uint64_t& fills, uint64_t& iters) {
    std::vector<Unit> queue;
    for (uint32_t b = 0; b < nbp; b += ub)
        for (uint32_t p = 0; p < n_pix; p++) queue.push_back({p, b, serial++});
    size_t next = 0;
    Lane lane[64];
    for (;;) {
        bool any = false;
        for (Lane& l : lane) {  // the refill: a new unit starts with an empty reserve
            if (l.need && next < queue.size()) {
                const Unit u = queue[next++];
                l.need = false; l.pixel = u.pixel; l.serial = u.serial; l.blk = u.b;
                l.word = u.b + ub < nbp ? u.b + ub : nbp;
                l.s_cur = (block0 + u.b) * kSB; l.unit_lo = l.s_cur; l.expect = l.s_cur; l.alive = false;
                CHECK(ahead_count(l.word) == 0 && ahead_blk_end(l.word) == l.word, "a fresh blk_end word %u", l.word);
            }
            any |= !l.need;
        }
        if (!any) break;
        iters++;
        bool starved = false;
        for (Lane& l : lane) starved |= ahead_starved(!l.need, l.alive, ahead_count(l.word));
        if (starved) {  // the fill phase
            fills++;
            for (Lane& l : lane) {
                const uint32_t cnt = ahead_count(l.word);
                const uint32_t first = ahead_first_uncached(l.s_cur, l.alive, cnt);
                const uint32_t end = ahead_unit_end(block0, ahead_blk_end(l.word), spp);
                if (!l.need && ahead_room(cnt, K, first, end)) {
                    CHECK(first < spp, "K %u spp %u: entry for sample %u", K, spp, first);
                    CHECK(first >= l.unit_lo && first < (block0 + ahead_blk_end(l.word)) * kSB, "K %u spp %u ub %u: sample %u outside unit [%u, %u)", K, spp, ub, first,
                          l.unit_lo, (block0 + ahead_blk_end(l.word)) * kSB);
                    CHECK(ahead_slot(first, K) < K, "slot %u", ahead_slot(first, K));
                    l.ring[ahead_slot(first, K)] = {l.pixel, first, l.serial};
                    l.word = ahead_pushed(l.word);
                    CHECK(ahead_count(l.word) == cnt + 1 && ahead_count(l.word) <= K, "count %u after a push at K %u", ahead_count(l.word), K);
                }
            }
        }
        for (Lane& l : lane) {
            if (l.need) continue;
            if (!l.alive) {  // regeneration from the reserve
                CHECK(ahead_count(l.word) > 0, "K %u spp %u ub %u: lane needs sample %u and has no entry", K, spp, ub, l.s_cur);
                const Entry e = l.ring[ahead_slot(l.s_cur, K)];
                CHECK(e.pixel == l.pixel && e.sample == l.s_cur, "K %u spp %u ub %u: pixel %u sample %u got the ray of pixel %u sample %u", K, spp, ub, l.pixel, l.s_cur,
                      e.pixel, e.sample);
                CHECK(e.serial == l.serial, "K %u spp %u ub %u: pixel %u sample %u: entry of unit %u read in unit %u", K, spp, ub, l.pixel, l.s_cur, e.serial, l.serial);
                const uint32_t blk_end = ahead_blk_end(l.word);
                l.word = ahead_popped(l.word);
                CHECK(ahead_blk_end(l.word) == blk_end, "a pop changed blk_end");
                CHECK(l.s_cur == l.expect, "pixel %u: sample %u started where %u was due", l.pixel, l.s_cur, l.expect);
                l.expect = l.s_cur + 1;
                consumed[(size_t)l.pixel * spp + l.s_cur]++;
                l.alive = true;
                l.left = 1;
                while (rnd() % mean != 0) l.left++;  // 1 + geometric
            }
            if (--l.left == 0) {  // the path ended: the sample is done
                l.alive = false;
                l.s_cur++;
                if (l.s_cur % kSB == 0 || l.s_cur >= spp) {
                    l.blk++;
                    l.need = l.blk >= ahead_blk_end(l.word) || l.s_cur >= spp;
                    if (l.need) CHECK(ahead_count(l.word) == 0, "K %u spp %u ub %u: unit ends with %u entries left", K, spp, ub, ahead_count(l.word));
                }
            }
        }
    }
    CHECK(next == queue.size(), "units left in the queue");
}

static void check_ring() {
    const uint32_t spps[] = {1, 2, 15, 16, 17, 20, 33, 130, 256};
    const uint32_t ubs[] = {1, 2, 4, 8};
    for (uint32_t K = 1; K <= kAheadMaxK; K++)
        for (uint32_t spp : spps)
            for (uint32_t ub : ubs)
                for (uint32_t pass_blocks : {0u, 1u, 8u})      // 0: one pass; else passes of that many blocks (block0 > 0)
                    for (uint32_t n_pix : {5u, 150u})         // fewer pixels than lanes; lanes move on to other pixels
                        for (uint32_t mean : {1u, 3u}) {      // every path one segment; mean 1 + 2
                            const uint32_t n_blocks = (spp + kSB - 1) / kSB;
                            const uint32_t pb = pass_blocks ? pass_blocks : n_blocks;
                            if (pass_blocks && pb >= n_blocks && pass_blocks != 1) continue;  // the same as one pass
                            std::vector<uint32_t> consumed((size_t)n_pix * spp, 0);
                            uint32_t serial = 0;
                            uint64_t fills = 0, iters = 0;
                            for (uint32_t b0 = 0; b0 < n_blocks; b0 += pb)
                                run_launch(K, spp, ub, b0, b0 + pb < n_blocks ? pb : n_blocks - b0, n_pix, mean, consumed, serial, fills, iters);
                            size_t bad = 0;
                            for (uint32_t c : consumed) bad += c != 1;
                            CHECK(bad == 0, "K %u spp %u ub %u pass %u pixels %u: %zu samples not started exactly once", K, spp, ub, pass_blocks, n_pix, bad);
                            CHECK(fills <= iters, "more fills than iterations");
                        }
}

// the packing of the blk_end word and the predicates at their edges
static void check_word() {
    for (uint32_t blk_end : {0u, 1u, 8u, 12345u, (1u << kAheadShift) - 1u}) {
        uint32_t w = blk_end;
        for (uint32_t c = 0; c < kAheadMaxK; c++) {
            CHECK(ahead_count(w) == c && ahead_blk_end(w) == blk_end, "word %08x", w);
            w = ahead_pushed(w);
        }
        CHECK(ahead_count(w) == kAheadMaxK && ahead_blk_end(w) == blk_end, "word %08x", w);
        for (uint32_t c = kAheadMaxK; c > 0; c--) w = ahead_popped(w);
        CHECK(w == blk_end, "word %08x after as many pops", w);
    }
    CHECK(ahead_unit_end(0, 1, 20) == 16 && ahead_unit_end(1, 1, 20) == 20 && ahead_unit_end(0, 8, 33) == 33 && ahead_unit_end(2, 0, 33) == 32, "unit ends");
    CHECK(ahead_first_uncached(7, false, 0) == 7 && ahead_first_uncached(7, true, 0) == 8 && ahead_first_uncached(7, true, 2) == 10, "first uncached");
    CHECK(!ahead_room(2, 2, 5, 16) && ahead_room(1, 2, 15, 16) && !ahead_room(1, 2, 16, 16) && !ahead_room(0, 1, 20, 20), "room");
}

// Part A: the parent's decision ballot(busy && (deep || may)) != 0 against the gated one, which evaluates `may` only when no busy lane
// is deep. Per-lane booleans: all 8^4 waves of four lanes, then random waves of 64 at several densities (an all-idle wave included).
static bool parent_decision(uint64_t busy, uint64_t deep, uint64_t may) { return (busy & (deep | may)) != 0; }
static bool gated_decision(uint64_t busy, uint64_t deep, uint64_t may, bool& tested) {
    tested = bounds_test_decides(busy & deep);
    bool walk = !tested;
    if (!walk) walk = (busy & may) != 0;
    return walk;
}
static void check_gate() {
    bool tested;
    for (uint32_t code = 0; code < 8 * 8 * 8 * 8; code++) {
        uint64_t busy = 0, deep = 0, may = 0;
        for (int l = 0; l < 4; l++) {
            const uint32_t t = (code >> (3 * l)) & 7u;
            busy |= (uint64_t)(t & 1u) << (l * 17); deep |= (uint64_t)((t >> 1) & 1u) << (l * 17); may |= (uint64_t)((t >> 2) & 1u) << (l * 17);
        }
        CHECK(parent_decision(busy, deep, may) == gated_decision(busy, deep, may, tested), "wave %x", code);
    }
    size_t n_tested = 0;
    for (int k = 0; k < 8000; k++) {
        uint64_t m[3];
        for (uint64_t& v : m) {
            v = ((uint64_t)rnd() << 32) | rnd();
            for (uint32_t thin = rnd() % 7; thin > 0; thin--) v &= ((uint64_t)rnd() << 32) | rnd();  // densities 1/2 ... 1/128
        }
        if (k % 100 == 0) m[0] = 0;
        if (k % 100 == 1) m[0] = ~0ull;
        CHECK(parent_decision(m[0], m[1], m[2]) == gated_decision(m[0], m[1], m[2], tested), "wave %d", k);
        n_tested += tested;
    }
    CHECK(n_tested > 100 && n_tested < 7900, "the random waves take both branches: %zu", n_tested);
}

int main() {
    check_word();
    check_ring();
    check_gate();
    if (g_failed) {
        fprintf(stderr, "ahead_check: %d checks failed\n", g_failed);
        return 1;
    }
    printf("ahead_check ok\n");
    return 0;
}
