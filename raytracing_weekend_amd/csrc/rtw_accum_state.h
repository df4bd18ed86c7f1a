// rtw_accum_state.h — host arithmetic of the accumulation sessions (include/rtw.h rtw_accum_*): how an add is split into pieces, the
// header of a saved session, its validation and the scene fingerprint. No HIP in here: tests/native/accum_check.cpp compiles it with
// g++ and checks it on the CPU, in the manner of rtw_plan.h and rtw_scene.h.
#pragma once
#include <stdint.h>

#include <cstddef>
#include <cstring>
#include <string>

#include "../../include/rtw.h"

namespace rtwk {

constexpr int kAccumUnit = RTW_SUM_BLOCK * RTW_SUM_UNIT_BLOCKS;  // samples of a summation unit (128)
constexpr int32_t kAccumCapMax = 0x7ffffff0;                       // the largest multiple of RTW_SUM_BLOCK an int32 holds

// ---- an add [n_from, n_to) (samples counted from sample_offset, both multiples of RTW_SUM_BLOCK) in pieces
// k_path stores ONE sum per summation unit where the planner picks 8-block lane units (rtw_plan.h plan_path: unit_sums), and such a
// launch must start on a unit boundary: slot [block / 8] is then a whole unit of the render. So:
//   head   [n_from, next unit boundary or n_to)  when n_from is inside a unit: every block's sum is stored (planned the way
//          rtw_render_adaptive plans a pass) and joins the unit the session holds open
//   body   the whole units that follow: unit sums allowed
//   tail   [last unit boundary, n_to)  when n_to is inside a unit: block sums; the unit stays open in the session
// every_block (sessions with RTW_ACCUM_ERROR: the moments are taken over block sums, so every block's sum must reach memory): one
// piece without unit sums - alignment is then no concern.
// The host issues body and tail as ONE plan_path call: accum_runs below turns the pieces into what is launched.
struct AccumPiece {
    int n_from, n_to;
    bool unit_sums;  // the launches of this piece may store whole unit sums: n_from and n_to are unit boundaries
    bool open_tail;  // this piece ends inside a unit, which stays open
    bool head;       // this piece starts inside a unit
};
struct AccumSplit {
    int n;
    AccumPiece piece[3];
};
inline AccumSplit accum_split(int n_from, int n_to, bool every_block) {
    AccumSplit s{};
    if (n_from >= n_to) return s;
    if (every_block) {
        s.piece[s.n++] = AccumPiece{n_from, n_to, false, n_to % kAccumUnit != 0, n_from % kAccumUnit != 0};
        return s;
    }
    int at = n_from;
    if (at % kAccumUnit != 0) {
        const int up = (at / kAccumUnit + 1) * kAccumUnit;
        const int to = up < n_to ? up : n_to;
        s.piece[s.n++] = AccumPiece{at, to, false, to % kAccumUnit != 0, true};
        at = to;
    }
    const int down = n_to / kAccumUnit * kAccumUnit;
    if (at < down) {
        s.piece[s.n++] = AccumPiece{at, down, true, false, false};
        at = down;
    }
    if (at < n_to) s.piece[s.n++] = AccumPiece{at, n_to, false, true, false};
    return s;
}

// What the host issues for a split: one plan_path call per run. The head is a run of its own; the body and the open tail behind it
// are ONE run (plan_path hands a pass's trailing blocks out, and stores them, one by one, so a run that may use unit sums needs a unit
// boundary at its start only, and the tail costs no launch of its own). units_ok: the run's bulk launch may store whole unit sums.
struct AccumRun { int n_from, n_to; bool units_ok, open_tail; };
struct AccumRuns {
    int n;
    AccumRun run[2];
};
inline AccumRuns accum_runs(const AccumSplit& s, bool every_block) {
    AccumRuns r{};
    for (int k = 0; k < s.n; k++) {
        const AccumPiece& p = s.piece[k];
        if (r.n > 0 && !s.piece[k - 1].head) {  // the tail joins the body before it
            r.run[r.n - 1].n_to = p.n_to;
            r.run[r.n - 1].open_tail = p.open_tail;
        } else {
            r.run[r.n++] = AccumRun{p.n_from, p.n_to, !p.head && !every_block, p.open_tail};
        }
    }
    return r;
}

// ---- FNV-1a, 64 bit, over the bytes of the uploaded scene blob: what a saved session remembers of its scene
inline uint64_t accum_fingerprint(const void* data, size_t bytes) {
    const unsigned char* p = (const unsigned char*)data;
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; i++) {
        h ^= p[i];
        h *= 0x100000001b3ull;
    }
    return h;
}

// ---- a saved session: this header, then npix float4 closed-units sums, npix float4 open-unit sums and, with RTW_ACCUM_ERROR, npix
// (double, double) moments. Native byte order; every array starts 16-byte aligned (the header is 128 bytes).
constexpr uint32_t kAccumMagic = 0x41575452u;  // "RTWA"
constexpr uint32_t kAccumVersion = 1;
struct AccumHeader {
    uint32_t magic, version;
    uint32_t header_bytes;  // sizeof(AccumHeader)
    uint32_t flags;         // RTW_ACCUM_*
    rtw_params params;      // as given to rtw_accum_begin (spp = the cap)
    int32_t done;           // samples per pixel the state holds
    int32_t reserved;
    uint64_t npix;          // pixels of the shard: rows * width
    uint64_t samples, segments, shadow_rays;  // summed over the adds
    uint64_t scene;         // accum_fingerprint of the scene blob
    uint64_t total_bytes;   // header + arrays
    uint64_t reserved2;     // 0
};
static_assert(sizeof(rtw_params) == 48, "rtw_params layout");
static_assert(sizeof(AccumHeader) == 128, "AccumHeader layout");

inline size_t accum_shard_rows(const rtw_params& P) {
    const size_t k = P.row_stride > 1 ? (size_t)P.row_stride : 1;
    return ((size_t)(P.row1 - P.row0) + k - 1) / k;
}
inline size_t accum_state_bytes(size_t npix, uint32_t flags) { return sizeof(AccumHeader) + npix * 16 * ((flags & RTW_ACCUM_ERROR) ? 3 : 2); }

// what rtw_accum_begin asks of its params beyond rtw_render's checks; nullptr when fine
inline const char* accum_check_params(const rtw_params& P, uint32_t flags) {
    if (flags & ~(uint32_t)RTW_ACCUM_ERROR) return "unknown flags";
    if (P.width <= 0 || P.height <= 0 || P.max_depth < 0 || P.row0 < 0 || P.row1 > P.height || P.row0 > P.row1) return "bad render params";
    if (P.rng_kind != RTW_RNG_PHILOX && P.rng_kind != RTW_RNG_TEA_LCG) return "bad rng_kind";
    if (P.sample_offset < 0 || P.samples_per_pass < 0 || P.row_stride < 0) return "bad sample_offset/samples_per_pass/row_stride";
    if (P.estimator < RTW_EST_REFERENCE || P.estimator > RTW_EST_MIXTURE) return "bad estimator";
    if (P.spp <= 0 || P.spp % RTW_SUM_BLOCK != 0) return "the cap (params->spp) must be a positive multiple of RTW_SUM_BLOCK";
    if ((int64_t)P.sample_offset + (int64_t)P.spp > (int64_t)INT32_MAX) return "sample_offset + cap overflows";
    return nullptr;
}

inline AccumHeader accum_pack(const rtw_params& P, uint32_t flags, int32_t done, uint64_t samples, uint64_t segments, uint64_t shadow_rays,
                              uint64_t scene) {
    AccumHeader h;
    memset(&h, 0, sizeof h);
    h.magic = kAccumMagic; h.version = kAccumVersion; h.header_bytes = (uint32_t)sizeof(AccumHeader); h.flags = flags;
    h.params = P; h.done = done;
    h.npix = (uint64_t)(accum_shard_rows(P) * (size_t)P.width);
    h.samples = samples; h.segments = segments; h.shadow_rays = shadow_rays; h.scene = scene;
    h.total_bytes = (uint64_t)accum_state_bytes((size_t)h.npix, flags);
    return h;
}

// Reads and checks the header of a saved session of `bytes` bytes against the fingerprint of the scene in place. false: `why` says
// what is wrong and `out` is not to be used.
inline bool accum_validate(const void* blob, size_t bytes, uint64_t scene, AccumHeader& out, std::string& why) {
    if (!blob || bytes < sizeof(AccumHeader)) { why = "shorter than a session header"; return false; }
    AccumHeader h;
    memcpy(&h, blob, sizeof h);
    if (h.magic != kAccumMagic) { why = "not a saved session (magic)"; return false; }
    if (h.version != kAccumVersion || h.header_bytes != sizeof(AccumHeader)) { why = "saved by another version"; return false; }
    if (const char* bad = accum_check_params(h.params, h.flags)) { why = std::string("its params: ") + bad; return false; }
    if (h.done < 0 || h.done > h.params.spp || h.done % RTW_SUM_BLOCK != 0) { why = "its sample count does not fit its cap"; return false; }
    const size_t npix = accum_shard_rows(h.params) * (size_t)h.params.width;
    if (h.npix != (uint64_t)npix) { why = "its pixel count does not match its params"; return false; }
    if (h.total_bytes != (uint64_t)accum_state_bytes(npix, h.flags) || (uint64_t)bytes != h.total_bytes) {
        why = "its size does not match its params (truncated or padded)";
        return false;
    }
    if (h.samples != (uint64_t)npix * (uint64_t)h.done) { why = "its counts do not match its sample count"; return false; }
    if (h.scene != scene) { why = "it was saved with another scene"; return false; }
    out = h;
    return true;
}

}  // namespace rtwk
