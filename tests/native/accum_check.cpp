// CPU check of the accumulation sessions' host arithmetic (raytracing_weekend_amd/csrc/rtw_accum_state.h): the splitter of an add, the
// saved session's header (round trip and every refusal) and the scene fingerprint. A stand-alone program: tests/test_accum_cpu.py
// builds it with g++ -fsanitize=address,undefined and runs it; it prints "accum_check ok" and returns 0, or says what failed.
// "accum_check split <from> <to> <every_block>" prints the pieces of one add instead ("from to unit_sums open_tail head" per line).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracing_weekend_amd/csrc/rtw_accum_state.h"

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

static void check_split(int n_from, int n_to, bool every_block) {
    const AccumSplit s = accum_split(n_from, n_to, every_block);
    CHECK(s.n >= 1 && s.n <= 3, "[%d, %d): %d pieces", n_from, n_to, s.n);
    int at = n_from, heads = 0, tails = 0;
    for (int k = 0; k < s.n; k++) {
        const AccumPiece& p = s.piece[k];
        CHECK(p.n_from == at && p.n_to > p.n_from, "[%d, %d): piece %d is [%d, %d), expected to start at %d", n_from, n_to, k, p.n_from, p.n_to, at);
        CHECK(p.n_from % 16 == 0 && p.n_to % 16 == 0, "[%d, %d): piece %d is not whole blocks", n_from, n_to, k);
        if (p.unit_sums) CHECK(p.n_from % 128 == 0 && p.n_to % 128 == 0, "[%d, %d): unit-sum piece [%d, %d)", n_from, n_to, p.n_from, p.n_to);
        CHECK(!(every_block && p.unit_sums), "[%d, %d): unit sums in an every-block split", n_from, n_to);
        CHECK(p.head == (p.n_from % 128 != 0), "[%d, %d): piece %d head flag", n_from, n_to, k);
        CHECK(p.open_tail == (p.n_to % 128 != 0), "[%d, %d): piece %d tail flag", n_from, n_to, k);
        if (p.head) {
            heads++;
            CHECK(k == 0, "[%d, %d): a head that is not first", n_from, n_to);
            // a head ends with its unit (or with the add)
            CHECK(every_block || p.n_to <= (p.n_from / 128 + 1) * 128, "[%d, %d): head [%d, %d) crosses a unit boundary", n_from, n_to, p.n_from, p.n_to);
        }
        if (p.open_tail) {
            tails++;
            CHECK(k == s.n - 1, "[%d, %d): an open tail that is not last", n_from, n_to);
        }
        at = p.n_to;
    }
    CHECK(at == n_to, "[%d, %d): the pieces end at %d", n_from, n_to, at);
    CHECK(heads <= 1 && tails <= 1, "[%d, %d): %d heads, %d tails", n_from, n_to, heads, tails);
    if (every_block) CHECK(s.n == 1, "[%d, %d): every-block split in %d pieces", n_from, n_to, s.n);
    // what the host launches: at most two runs, contiguous, covering the add; a run that may store unit sums starts on a unit
    // boundary and is made of whole pieces (a body, a tail, or a body with its tail); only the last run leaves a unit open
    const AccumRuns r = accum_runs(s, every_block);
    CHECK(r.n >= 1 && r.n <= 2, "[%d, %d): %d runs", n_from, n_to, r.n);
    at = n_from;
    for (int k = 0; k < r.n; k++) {
        const AccumRun& q = r.run[k];
        CHECK(q.n_from == at && q.n_to > q.n_from, "[%d, %d): run %d is [%d, %d)", n_from, n_to, k, q.n_from, q.n_to);
        CHECK(q.units_ok == (!every_block && q.n_from % 128 == 0), "[%d, %d): run %d [%d, %d) units_ok %d", n_from, n_to, k, q.n_from, q.n_to, (int)q.units_ok);
        CHECK(q.open_tail == (q.n_to % 128 != 0), "[%d, %d): run %d tail flag", n_from, n_to, k);
        if (k + 1 < r.n) CHECK(!q.open_tail || q.n_to == n_to, "[%d, %d): run %d leaves a unit open before the last run", n_from, n_to, k);
        at = q.n_to;
    }
    CHECK(at == n_to, "[%d, %d): the runs end at %d", n_from, n_to, at);
    if (r.n == 2) CHECK(r.run[0].n_from % 128 != 0 && r.run[0].n_to % 128 == 0, "[%d, %d): two runs without a head", n_from, n_to);
}

static rtw_params params() {
    rtw_params P;
    memset(&P, 0, sizeof P);
    P.width = 24; P.height = 10; P.spp = 256; P.max_depth = 8; P.seed = 7u; P.row0 = 1; P.row1 = 10; P.rng_kind = RTW_RNG_TEA_LCG;
    P.sample_offset = 48; P.row_stride = 2; P.estimator = RTW_EST_CORRECTED;
    return P;
}

static std::vector<unsigned char> blob_of(const AccumHeader& h) {
    std::vector<unsigned char> b((size_t)h.total_bytes, 0x5a);
    memcpy(b.data(), &h, sizeof h);
    return b;
}

static bool refused(std::vector<unsigned char> b, uint64_t scene, const char* what) {
    AccumHeader out;
    std::string why;
    const bool ok = accum_validate(b.data(), b.size(), scene, out, why);
    CHECK(!ok, "%s was accepted", what);
    CHECK(ok || !why.empty(), "%s: refused without a reason", what);
    return !ok;
}

int main(int argc, char** argv) {
    if (argc == 5 && strcmp(argv[1], "split") == 0) {  // "split <from> <to> <every_block>": the pieces, one per line
        const AccumSplit s = accum_split(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]) != 0);
        for (int k = 0; k < s.n; k++) printf("%d %d %d %d %d\n", s.piece[k].n_from, s.piece[k].n_to, (int)s.piece[k].unit_sums, (int)s.piece[k].open_tail, (int)s.piece[k].head);
        return 0;
    }
    // ---- the splitter, exhaustively
    for (int from = 0; from < 1024; from += 16)
        for (int to = from + 16; to <= 1024; to += 16) {
            check_split(from, to, false);
            check_split(from, to, true);
        }
    {   // the cases of the header's comment
        AccumSplit s = accum_split(48, 512, false);
        CHECK(s.n == 2 && s.piece[0].head && s.piece[0].n_to == 128 && s.piece[1].unit_sums && s.piece[1].n_to == 512 && !s.piece[1].open_tail, "split 48..512");
        s = accum_split(48, 464, false);
        CHECK(s.n == 3 && s.piece[0].n_from == 48 && s.piece[0].n_to == 128 && s.piece[1].unit_sums && s.piece[1].n_to == 384 && s.piece[2].n_to == 464 &&
                  s.piece[2].open_tail, "split 48..464");
        s = accum_split(112, 144, false);
        CHECK(s.n == 2 && s.piece[0].n_to == 128 && !s.piece[1].unit_sums, "split 112..144");
        s = accum_split(0, 4096, false);
        CHECK(s.n == 1 && s.piece[0].unit_sums, "split 0..4096");
        s = accum_split(16, 32, false);
        CHECK(s.n == 1 && s.piece[0].head && s.piece[0].open_tail, "split 16..32");
        CHECK(accum_split(64, 64, false).n == 0, "an empty add has no piece");
    }

    // ---- FNV-1a 64: offset basis 0xcbf29ce484222325, prime 0x100000001b3
    CHECK(accum_fingerprint("", 0) == 0xcbf29ce484222325ull, "fingerprint of nothing");
    // "a": (basis ^ 0x61) * prime mod 2^64, by hand: 0xaf63dc4c8601ec8c (the value the FNV authors publish for "a")
    CHECK(accum_fingerprint("a", 1) == 0xaf63dc4c8601ec8cull, "fingerprint of \"a\": %llx", (unsigned long long)accum_fingerprint("a", 1));
    CHECK(accum_fingerprint("a", 1) == (0xcbf29ce484222325ull ^ 0x61ull) * 0x100000001b3ull, "fingerprint of \"a\", one step");
    CHECK(accum_fingerprint("foobar", 6) == 0x85944171f73967e8ull, "fingerprint of \"foobar\": %llx", (unsigned long long)accum_fingerprint("foobar", 6));
    CHECK(accum_fingerprint("ab", 2) != accum_fingerprint("ba", 2), "fingerprint ignores order");

    // ---- header round trip
    const rtw_params P = params();
    const uint64_t scene = 0x1234567890abcdefull;
    const size_t npix = 5 * 24;  // rows 1, 3, 5, 7, 9
    CHECK(accum_shard_rows(P) == 5, "shard rows %zu", accum_shard_rows(P));
    for (uint32_t flags = 0; flags <= 1; flags++) {
        const AccumHeader h = accum_pack(P, flags, 48, (uint64_t)npix * 48, 1000, 200, scene);
        CHECK(h.total_bytes == 128 + npix * 16 * (flags ? 3 : 2), "total bytes %llu", (unsigned long long)h.total_bytes);
        CHECK(accum_state_bytes(npix, flags) == h.total_bytes, "state bytes");
        const std::vector<unsigned char> b = blob_of(h);
        AccumHeader out;
        std::string why;
        CHECK(accum_validate(b.data(), b.size(), scene, out, why), "round trip refused: %s", why.c_str());
        CHECK(memcmp(&out, &h, sizeof h) == 0, "round trip changed the header");
        CHECK(memcmp(&out.params, &P, sizeof P) == 0 && out.done == 48 && out.flags == flags && out.segments == 1000 && out.shadow_rays == 200 &&
                  out.samples == npix * 48 && out.scene == scene && out.npix == npix, "round trip fields");

        // ---- every refusal
        std::vector<unsigned char> t = b;
        t[0] ^= 1;
        refused(t, scene, "a wrong magic");
        AccumHeader g = h;
        g.version = kAccumVersion + 1;
        refused(blob_of(g), scene, "a wrong version");
        t = b;
        t.resize(b.size() - 16);
        refused(t, scene, "a truncated blob");
        t.resize(64);
        refused(t, scene, "a blob shorter than the header");
        t = b;
        t.resize(b.size() + 16, 0);
        refused(t, scene, "an oversized blob");
        g = h; g.params.width = 25;  // the arrays no longer fit the frame
        refused(blob_of(g), scene, "params of another width");
        g = h; g.params.row_stride = 1;
        refused(blob_of(g), scene, "params of another shard");
        g = h; g.params.rng_kind = 7;
        refused(blob_of(g), scene, "an unknown generator");
        g = h; g.params.spp = 250;
        refused(blob_of(g), scene, "a cap that is not whole blocks");
        g = h; g.params.spp = 32;  // below done
        refused(blob_of(g), scene, "a cap below the sample count");
        g = h; g.done = 40; g.samples = (uint64_t)npix * 40;
        refused(blob_of(g), scene, "a sample count that is not whole blocks");
        g = h; g.params.sample_offset = 0x7fffff00;
        refused(blob_of(g), scene, "an overflowing sample range");
        g = h; g.flags = flags ^ 1u;  // the moments are there but not announced, or the other way round
        refused(blob_of(g), scene, "flags that do not match the arrays");
        g = h; g.flags = flags | 2u;
        refused(blob_of(g), scene, "unknown flags");
        refused(b, scene + 1, "another scene's fingerprint");
        CHECK(!accum_validate(nullptr, 0, scene, out, why), "a null blob was accepted");
    }
    CHECK(accum_check_params(P, 0) == nullptr && accum_check_params(P, RTW_ACCUM_ERROR) == nullptr, "good params refused");
    {
        rtw_params Q = P;
        Q.spp = 0;
        CHECK(accum_check_params(Q, 0) != nullptr, "cap 0 accepted");
        Q.spp = kAccumCapMax; Q.sample_offset = 0;
        CHECK(accum_check_params(Q, 0) == nullptr, "the largest cap refused");
        Q.sample_offset = 16;
        CHECK(accum_check_params(Q, 0) != nullptr, "an overflowing cap accepted");
    }
    if (g_failed) {
        fprintf(stderr, "accum_check: %d checks failed\n", g_failed);
        return 1;
    }
    printf("accum_check ok\n");
    return 0;
}
