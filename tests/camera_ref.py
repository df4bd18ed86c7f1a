"""A float64 numpy reference for the camera ray: how a pixel and a sample index become an origin, a direction, a gather time and a
first ray time. A second reading of include/rtw.h (rtw_camera_type, rtw_camera, rtw_rng_kind, the "Draws" paragraph of rtw_radiance,
rtw_views) and of the reference's scene/camera.cuh, shaders/camera.cu, raygen/raygen.cu, lib/sampling.cuh and scene/ioCamera.h,
written without looking at oracle/rtw_oracle.c, raygen<> or view_raygen<>. Two things the reference does not have are the
project's own and are restated from include/rtw.h (rtw_rng_kind, "Camera draws"): how a Philox word becomes a 24-bit uniform
and where the Philox gather-time draw and the camera ray's time come from. The shutter cases below tell that statement from
another one: a different layout moves the moving sphere's silhouette by many pixels. Shared by test_camera_cpu.py
(the oracle and the camera builders against this file) and test_gpu_camera.py (the kernels against this file, then against the
oracle's bits). The fourth of four such references: geometry_ref.py (closest hits), shading_ref.py (scatter events, media,
textures), lighting_ref.py (direct lighting); all three start from rays the test supplies, this one makes the ray.

The law
  Generators    tea<N>(v0, v1), the 24-bit LCG rnd() (OptiX SDK cuda/random.h: state = 1664525 state + 1013904223, the low 24 bits
                over 2^24), Philox4x32-10 (Random123), all in numpy integer arithmetic; a Philox word w gives (w >> 8) / 2^24.
  Draws         per (stream key = width * y + x, sample index, seed). TEA+LCG (takes no seed): state = tea<64>(key, sample)
                (raygen.cu:129 with the sample index for the reference's 0), then in this order r0 = jitter x, r1 = jitter y
                (raygen.cu:134-135), r2, r3 = the lens draws - taken by the perspective camera only (camera.cuh:35-56: the
                other two take no seed), and taken at lens radius 0 too (camera.cu:11-19, sampling.cuh:15-22) -, r4 = the gather
                draw (raygen.cu:103). The first ray time is THE SAME LCG output as the gather draw: color() copies the seed into
                the payload (raygen.cu:100) before it draws the gather time from its own copy, and rayColor starts from the
                payload's (raygen.cu:33) and hands its first rnd() to optixTraverse (raygen.cu:48). Philox: block (key, sample, 0, 0)
                under key (seed, 0); words 0 to 3 are r0 ... r3 for every camera kind (the draws are positional); the gather draw
                is ((w0 & 255) << 16 | (w1 & 255) << 8 | (w2 & 255)) / 2^24 of the same block; the first ray time is word 0 of
                block (key, sample, 0, 2) (rtw.h).
  Image plane   s = (x + r0) / width, t = (y + r1) / height (raygen.cu:134-135), y the row of the FULL image whatever row0 / row1 /
                row_stride say, row 0 at the bottom (rtw.h rtw_render).
  Perspective   a = r2 * 2 * pi, lens point = lens_radius * sqrt(r3) * (sin a, cos a) on (u, v) (sampling.cuh:15-22,
                camera.cu:14-16); origin = camera origin + lens point; d = lower_left + s horizontal + t vertical - origin, not
                normalised (camera.cu:17-18).
  Environment   the origin enters alone; d = normalize(cos(2 pi s) sin(pi t) u - cos(pi t) v + sin(2 pi s) sin(pi t) w)
                (camera.cuh:35-47).
  Orthographic  origin = lower_left + s horizontal + t vertical + camera origin: the origin enters twice when lower_left is built
                the way ioOrthographicCamera builds it (camera.cuh:52, ioCamera.h:155-158); d = -normalize(w).
  First segment tmin 1e-6 (camera.cuh:71, raygen.cu:45), tmax 1e27 (rtw.h).
  Times         gather = time0 + r4 (time1 - time0) from the camera's own times (raygen.cu:103), the view's own for rtw_views. The
                ray time is the raw uniform in [0, 1): raygen.cu:48 hands rnd(seed) to optixTraverse as it is. It is what
                geometry_ref clamps to the motion keys' [0, 1].
  Builders      ioCamera, ioPerspectiveCamera, ioEnvironmentCamera, ioOrthographicCamera (ioCamera.h:15-34, :64-90, :121-128,
                :143-162) in float64 from float32 arguments. The reference's environment and orthographic constructors take t0, t1
                and do not pass them on (ioCamera.h:126-128, :149-151), so those cameras' shutters are always 0 .. 0; the reference
                never instantiates either. The project's host/ioCamera.h passes them on, and so does this law: rtw_views promises
                a gather time over the view's own time0 / time1 for every camera kind, which a builder that drops the times
                could not feed (Cameras).

How a ray is observed (all three are the project's own techniques; every case has max_depth = 1 and one sample per render)
  Sky decoder   sky_light = 1 and one rectangle a million units below and to the side that no ray meets (checked with geometry_ref): red = 1 - 0.25
                (u.y + 1), u.y = 3 - 4 red (shading_ref.sky_red / decode_uy). Each camera kind is uploaded in three frames (FRAMES_OF
                _AXES) that put v, w and -u in turn along world y, so the three renders read the whole unit direction. The
                perspective camera's focus distance is 1 and its lens radius 0.5, so the direction carries the lens offset;
                sky-pinhole-* is the same camera without the lens, the reference's own kind and the only one k_path's hot
                instantiation (LDS frame, rays made ahead of time) serves: lens_free_reference_camera(). The
                orthographic camera's one direction, -w, is tilted off the axes by (0.3, -0.2, 0.1) so that its three frames
                read three inexact numbers.
  Tile wall     axis-aligned diffuse-light rectangles in the plane z = 0, each with its own constant colour in exact fractions; no
                sky. The sample's colour names the primitive exactly (0: a miss); expected is geometry_ref.closest_hit on the
                law's ray. wall24: 6 x 4 tiles (24 primitives: the default upload walks k_path's lists); wall300: 20 x 15 tiles
                (the tree). The pitches (2.03 x 1.99, 0.61 x 0.53) are incommensurate with the pixel pitch at the wall (0.455), so
                tile edges cross most pixels. Cameras: perspective without a lens, perspective with lens radius 0.6 focused at 4
                (the wall is 10 away: the lens offset moves the hit by up to 0.9), environment, orthographic.
  Moving sphere a Lambertian moving sphere (radius 1.4, centres (0, 0, 0) -> (9, 0, 0), keys t0, t1 = 0.5, 2.0) under the sky, shutter
                0.25 .. 0.75: a hit is exactly 0, a miss never is. By geometry_ref's moving-sphere law the ray time carries the
                centre over 9 units (3.2 diameters) and the gather time over another 3 around it, so the two act differently
                and any wrong time moves the silhouette by many pixels. The frame is 14.4 x 3 at the sphere, so that at least
                MIN_HIT_SHARE = 10 % of the samples hit (asserted on the 24 x 16 frame from key 0; the top rows that the far
                corner and the shifted keys render look past the sphere). The orthographic window is the same 14.4 x 3; the
                environment camera stands 0.5 beside the centre's track, so that for a fifth of the time the sphere holds it and
                every ray hits from inside. On a miss the red is held to the sky decoder's direction too.
  Guides        rtw_render_guides / rtw_views_guides at spp = 1 on the walls: prim exact, depth held to t64 |d|.

Conditioning. A sample is left out of the exact comparisons (tile identity, hit or miss) when geometry_ref marks its ray
ill-conditioned, or when the law's decision differs between its float64 and its float32 evaluation. Nothing is left out of the
direction comparisons. At most MAX_LEFT_OUT = 2 % of a case's samples may be left out, counted per frame over the frame's sample
offsets (check_run, pooled: asserted and printed by both test files; a single 96-sample shard frame may leave out two). The law
alone leaves out at most 1.04 % (`python tests/camera_ref.py`; the walls' tile edges are nearly all of it).

Error units (first-order forward errors of the reference's formulas in fp32, in units of 2^-24; `e_x` bounds a component of x)
  s, t          e_s = (x + 1) / width + s: x + r0 is rounded at the size of x + 1, the quotient at its own size. e_t likewise.
  perspective   e_lens = lens_radius (a + 6): the angle a = r2 * 2 * pi is rounded at its own size, 6 for the root, sine, cosine and
                products. e_o = |origin| + e_lens + 2 lens_radius. e_d = e_s |horizontal| + e_t |vertical| + 3 (|lower_left| +
                s |horizontal| + t |vertical| + |origin|) + e_o (|.| the largest component).
  environment   e_d = 3 (2 pi s) + 3 (pi t) + 8: the arguments s * 2 * pi and t * pi carry their own rounding, s's (twice its size)
                and pi's; 8 for the sines, products, sums and the normalisation. e_o = 0 (the origin is copied).
  orthographic  e_o = e_s |horizontal| + e_t |vertical| + 3 (|lower_left| + s |horizontal| + t |vertical| + |origin|); e_d = 4.
  decoded y     4 for the decode (four times the rounding of a red in [0.5, 1]) + 4 for the sky's normalisation + 2 e_d / |d|.
  depth         |d| (geometry_ref's unit of t + (e_o + t e_d) / |d_z|) + t |d| (e_d / |d| + 3): the ray's own error carried into
                t = (k - o_z) / d_z, then the length's and the product's.
  mean of 144   the per-sample bound of a red (a quarter of decoded y's) plus the summation term sum_units(144) = 14.33: reds are at
                most 1, so partial sum j of a block of RTW_SUM_BLOCK = 16 is rounded at no more than j (sum_{2..16} j = 135 per
                block), block sum k of a unit of RTW_SUM_UNIT_BLOCKS = 8 at no more than 16 k (16 * 35 = 560), the two unit sums
                at 144, all over 144, plus 1 for the division.
The tolerance is K_FACTOR * MEASURED_CONSTANT_* * 2^-24 * unit, K_FACTOR = 4 being geometry_ref's (fused multiply-adds and other,
equally valid operation orders). MEASURED_CONSTANT_* is the largest |fp32 - fp64| / (2^-24 unit) of THIS FILE evaluated at two
precisions over the inputs of the tests, on the CPU (`python tests/camera_ref.py` prints them; test_camera_cpu.py re-measures them
and holds them to the recorded values). The float64 evaluation uses pi, the float32 one its float32 rounding, the reference's
CUDART_PI_F; the constants carry the difference. Recorded: direction 0.1767 (perspective), 0.2051 (environment), 0.0637
(orthographic); depth 0.1863; builders 0.1955. No number here comes from the oracle or the kernels.

Frames and draws. Every case is rendered at the seven sample offsets 0, 1, 15, 16, 127, 128, 4095 on a frame of 24 x 16, and at the
first and the last of them on its row shards [5, 12) at row_stride 2 and [3, 9) and on rows [4318, 4320) of a 7680 x 4320 image
(large x, keys near 2^25). Philox runs under two seeds; TEA+LCG, which takes no seed, on the keys from 0 and - rows [43691, 43707) of
a 24-wide image - on the keys from shading_ref.KEY_SHIFT (that frame alone: the others would repeat the first draw's samples). One mean of 144 samples per camera kind (MEAN_CASES).
"""
import ctypes as C
import functools
import os
import sys
from collections import namedtuple

import numpy as np

if __name__ == "__main__":  # `python tests/camera_ref.py` from anywhere: the package lies one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import geometry_ref as G
import shading_ref as S
from raytracing_weekend_amd import abi

U, K_FACTOR = G.U, G.K_FACTOR
PHILOX, TEA_LCG = abi.RTW_RNG_PHILOX, abi.RTW_RNG_TEA_LCG
PERSP, ENV, ORTHO = abi.RTW_CAM_PERSPECTIVE, abi.RTW_CAM_ENVIRONMENT, abi.RTW_CAM_ORTHOGRAPHIC
KIND_NAMES = {PERSP: "perspective", ENV: "environment", ORTHO: "orthographic"}
RNGS = S.RNGS
SEEDS = S.SEEDS
SAMPLE_OFFSETS = (0, 1, 15, 16, 127, 128, 4095)
MEAN_SPP = 144                     # crosses a block of 16 and a unit of 128
SUM_BLOCK, SUM_UNIT_BLOCKS = 16, 8  # RTW_SUM_BLOCK, RTW_SUM_UNIT_BLOCKS (include/rtw.h)
MAX_LEFT_OUT = 0.02
MIN_HIT_SHARE = 0.10
TMIN, TMAX = 1e-6, 1e27
_HDR = C.sizeof(abi.SceneHeader)
_M32 = np.uint64(0xFFFFFFFF)

# `python tests/camera_ref.py`: this file at float32 against itself at float64, in the units of the module text
MEASURED_CONSTANT_DIR = {PERSP: 0.1767, ENV: 0.2051, ORTHO: 0.0637}  # decoded y of the sky cases, per camera kind
MEASURED_CONSTANT_DEPTH = 0.1863   # t |d| on the walls
MEASURED_CONSTANT_BUILD = 0.1955   # the camera builders (BUILDER_INPUTS)


# ---------------------------------------------------------------- generators, in integer arithmetic
def _u64(a):
    return np.asarray(a).astype(np.uint64) & _M32


def tea(rounds, v0, v1):
    """tea<rounds>(v0, v1) of the OptiX SDK's cuda/random.h, elementwise."""
    v0, v1 = np.broadcast_arrays(_u64(v0), _u64(v1))
    v0, v1, s0 = v0.copy(), v1.copy(), np.uint64(0)
    k = [np.uint64(c) for c in (0xA341316C, 0xC8013EA4, 0xAD90777D, 0x7E95761E)]
    for _ in range(rounds):
        s0 = (s0 + np.uint64(0x9E3779B9)) & _M32
        v0 = (v0 + ((((v1 << np.uint64(4)) + k[0]) ^ (v1 + s0) ^ ((v1 >> np.uint64(5)) + k[1])) & _M32)) & _M32
        v1 = (v1 + ((((v0 << np.uint64(4)) + k[2]) ^ (v0 + s0) ^ ((v0 >> np.uint64(5)) + k[3])) & _M32)) & _M32
    return v0


def lcg(state):
    """One step of rnd(): (the new state, the uniform in [0, 1) as float64 - 24 bits, exact in float32 too)."""
    state = (np.uint64(1664525) * _u64(state) + np.uint64(1013904223)) & _M32
    return state, (state & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Random123): four counter words and two key words (arrays or integers) -> four output words."""
    c = [a.copy() for a in np.broadcast_arrays(*[_u64(a) for a in ctr])]
    k0, k1 = _u64(key[0]), _u64(key[1])
    m0, m1, w0, w1, sh = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(32)
    for r in range(10):
        if r:
            k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & _M32, (p0 >> sh) ^ c[3] ^ k1, p0 & _M32]
    return c


def u24(word):
    """The 24-bit uniform of a Philox word (rtw.h rtw_rng_kind)."""
    return (_u64(word) >> np.uint64(8)).astype(np.float64) / 16777216.0


def draws(key, sample, seed, rng_kind, camera_type, lens_draws_for_all=False, ray_time_own_draw=False):
    """The uniforms of the camera path of stream key `key` and sample index `sample` (arrays broadcast against each other), as
    float64: r0, r1 (jitter), r2, r3 (lens; 0 where none is drawn), r4 (the gather draw), rt (the first ray time).
    Negative controls, both under TEA+LCG: lens_draws_for_all - every camera kind takes the lens draws; ray_time_own_draw - the
    first ray time is the LCG output after the gather draw."""
    key, sample = np.broadcast_arrays(_u64(key), _u64(sample))
    if rng_kind == TEA_LCG:
        st = tea(64, key, sample)
        out = {}
        names = ["r0", "r1"] + (["r2", "r3"] if camera_type == PERSP or lens_draws_for_all else []) + ["r4"]
        for n in names:
            st, out[n] = lcg(st)
        for n in ("r2", "r3"):
            out.setdefault(n, np.zeros(key.shape))
        out["rt"] = out["r4"]  # the payload's seed was copied before the gather draw: rayColor's first rnd() repeats it
        if ray_time_own_draw:
            st, out["rt"] = lcg(st)
        return out
    zero = np.zeros(key.shape, np.uint64)
    w = philox4x32_10((key, sample, zero, zero), (seed, 0))
    out = {f"r{i}": u24(w[i]) for i in range(4)}
    b = np.uint64(255)
    out["r4"] = (((w[0] & b) << np.uint64(16)) | ((w[1] & b) << np.uint64(8)) | (w[2] & b)).astype(np.float64) / 16777216.0
    out["rt"] = u24(philox4x32_10((key, sample, zero, zero + np.uint64(2)), (seed, 0))[0])
    return out


# ---------------------------------------------------------------- frames: which pixels a render call holds
class Frame(namedtuple("Frame", "width height row0 row1 row_stride")):
    def rows(self):
        return np.arange(self.row0, self.row1, max(self.row_stride, 1))

    def xy(self):
        y, x = np.meshgrid(self.rows(), np.arange(self.width), indexing="ij")
        return x, y

    def keys(self):
        x, y = self.xy()
        return (np.uint64(self.width) * y.astype(np.uint64) + x.astype(np.uint64)) & _M32

    def params(self, spp, sample_offset, seed, rng_kind):
        return abi.make_params(self.width, self.height, spp, 1, seed=seed, row0=self.row0, row1=self.row1, rng_kind=rng_kind,
                               sample_offset=sample_offset, row_stride=self.row_stride)


FULL = Frame(24, 16, 0, 16, 0)
_SHIFT_ROW = -(-S.KEY_SHIFT // 24)  # the first row of a 24-wide image whose keys lie beyond shading_ref.KEY_SHIFT
FRAMES = {
    "full": FULL,
    "stride": Frame(24, 16, 5, 12, 2),   # rows 5, 7, 9, 11
    "shard": Frame(24, 16, 3, 9, 0),
    "corner": Frame(7680, 4320, 4318, 4320, 0),  # large x, keys near 2^25, the float conversion of x and y
    "shifted": Frame(24, _SHIFT_ROW + 16, _SHIFT_ROW, _SHIFT_ROW + 16, 0),  # TEA+LCG's second draw: the keys from KEY_SHIFT
}
# generator -> the (seed, frame of the seven sample offsets) of its two independent draws: Philox under two seeds, TEA+LCG (which
# takes no seed) on the keys from 0 and from KEY_SHIFT
DRAWS = {PHILOX: ((SEEDS[0], "full"), (SEEDS[1], "full")), TEA_LCG: ((SEEDS[0], "full"), (SEEDS[0], "shifted"))}
OTHER_FRAMES = ("stride", "shard", "corner")  # rendered at the first and the last sample offset


def runs(rng_kind, draw):
    """The (frame name, sample offset) pairs of one draw of a generator. TEA+LCG's second draw is the shifted frame alone: the
    other frames have the first draw's keys and, without a seed, its samples."""
    seed, main = DRAWS[rng_kind][draw]
    others = () if rng_kind == TEA_LCG and draw == 1 else OTHER_FRAMES
    return seed, [(main, s) for s in SAMPLE_OFFSETS] + [(f, s) for f in others for s in (SAMPLE_OFFSETS[0], SAMPLE_OFFSETS[-1])]


# ---------------------------------------------------------------- the camera ray
def _vmax(v):
    return float(np.abs(np.asarray(v, np.float64)).max())


def _unit(v):
    return v / np.sqrt((v * v).sum(-1))[..., None]


def camera_rays(cam, camera_type, frame, d, ft=np.float64, swap_jitter=False, rows_from_top=False, shard_local_rows=False,
                lens_sin_cos_swapped=False, plus_cos=False, ortho_origin_once=False):
    """Origin and direction (R, W, 3) at precision ft of every pixel of `frame` for the draws `d`, with the error bounds e_o, e_d
    (R, W; units of 2^-24, module text). cam: the 24 float32 of an rtw_camera. The keyword flags are negative controls."""
    cam = np.asarray(cam, np.float32).astype(ft)
    o, u, v, w, ll, hz, vt = (cam[3 * i:3 * i + 3] for i in range(7))
    lens = cam[21]
    x, y = frame.xy()
    if rows_from_top:
        y = frame.height - 1 - y
    if shard_local_rows:
        y = np.broadcast_to(np.arange(len(frame.rows()))[:, None], y.shape)
    r0, r1 = (d["r1"], d["r0"]) if swap_jitter else (d["r0"], d["r1"])
    s = (x.astype(ft) + r0.astype(ft)) / ft(frame.width)
    t = (y.astype(ft) + r1.astype(ft)) / ft(frame.height)
    e_s = (x + 1.0) / frame.width + s.astype(np.float64)
    e_t = (y + 1.0) / frame.height + t.astype(np.float64)
    pi = ft(np.pi)
    plane = 3.0 * (_vmax(ll) + s.astype(np.float64) * _vmax(hz) + t.astype(np.float64) * _vmax(vt) + _vmax(o))
    if camera_type == PERSP:
        a = d["r2"].astype(ft) * ft(2.0) * pi
        rho = np.sqrt(d["r3"].astype(ft))
        px, py = np.sin(a) * rho, np.cos(a) * rho
        if lens_sin_cos_swapped:
            px, py = py, px
        off = u * (lens * px)[..., None] + v * (lens * py)[..., None]
        origin = o + off
        direction = ((ll + s[..., None] * hz) + t[..., None] * vt) - origin
        e_o = _vmax(o) + float(lens) * (a.astype(np.float64) + 6.0) + 2.0 * float(lens)
        e_d = e_s * _vmax(hz) + e_t * _vmax(vt) + plane + e_o
    elif camera_type == ENV:
        ax, ay = s * ft(2.0) * pi, t * pi
        cy = np.cos(ay) if plus_cos else -np.cos(ay)
        ang = (np.cos(ax) * np.sin(ay), cy, np.sin(ax) * np.sin(ay))
        direction = _unit((ang[0][..., None] * u + ang[1][..., None] * v) + ang[2][..., None] * w)
        origin = np.broadcast_to(o, direction.shape).copy()
        e_o = np.zeros(s.shape)
        e_d = 3.0 * ax.astype(np.float64) + 3.0 * ay.astype(np.float64) + 8.0
    else:
        origin = (ll + s[..., None] * hz) + t[..., None] * vt
        if not ortho_origin_once:
            origin = origin + o
        direction = np.broadcast_to(-_unit(w), origin.shape).copy()
        e_o = e_s * _vmax(hz) + e_t * _vmax(vt) + plane
        e_d = np.full(s.shape, 4.0)
    return origin, direction, np.broadcast_to(e_o, s.shape), np.broadcast_to(e_d, s.shape)


def fp32_ray_units(origin, direction, e_o, e_d):
    """The units (2^-24) in which a float32 ray is compared with camera_rays' float64 origin and direction, per pixel: the forward
    bounds e_o, e_d, and no less than the size of the value itself - a bound of 0 (an origin that is a copy of the camera's) still
    leaves the rounding of the float64 value to float32, half an ulp of its largest component."""
    return (np.maximum(e_o, np.abs(np.asarray(origin, np.float64)).max(-1)),
            np.maximum(e_d, np.abs(np.asarray(direction, np.float64)).max(-1)))


def times(cam, d, ft=np.float64, times_swapped=False, ray_time_over_shutter=False, gather_raw=False):
    """(gather time, first ray time) at precision ft. The keyword flags are negative controls."""
    cam = np.asarray(cam, np.float32).astype(ft)
    t0, t1 = cam[22], cam[23]
    g, r = (d["rt"], d["r4"]) if times_swapped else (d["r4"], d["rt"])
    g, r = g.astype(ft), r.astype(ft)
    gather = g if gather_raw else t0 + g * (t1 - t0)
    ray_time = t0 + r * (t1 - t0) if ray_time_over_shutter else r
    return gather, ray_time


def rays8(origin, direction):
    """(n, 8) float32 rays in rtw_cast's layout, the first segment's tmin and tmax: the law's ray rounded to float32."""
    n = origin.reshape(-1, 3).shape[0]
    return np.concatenate([origin.reshape(-1, 3), direction.reshape(-1, 3), np.full((n, 1), TMIN), np.full((n, 1), TMAX)], 1).astype(np.float32)


def sum_units(spp):
    """The summation term of a mean of spp values of at most 1, in units of 2^-24 of the mean (module text)."""
    unit = SUM_BLOCK * SUM_UNIT_BLOCKS
    total, units = 0.0, 0
    for u0 in range(0, spp, unit):
        n = min(unit, spp - u0)
        blocks = [min(SUM_BLOCK, n - b0) for b0 in range(0, n, SUM_BLOCK)]
        total += sum(sum(range(2, b + 1)) for b in blocks)               # partial sum j of a block is at most j
        total += sum(sum(blocks[:k]) for k in range(2, len(blocks) + 1))  # the running sum of the block sums
        units += 1
        if units > 1:
            total += u0 + n                                                # the running sum of the unit sums
    return total / spp + 1.0                                               # the division


# ---------------------------------------------------------------- the float64 ioCamera builders
def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], a.dtype)


def _f32in(*vs):
    return [np.asarray(v, np.float64).astype(np.float32) for v in vs]


def io_camera(frm, to, up, ft=np.float64):
    """ioCamera (ioCamera.h:15-34): origin, u, v, w from float32 arguments."""
    frm, to, up = (a.astype(ft).reshape(3) for a in _f32in(frm, to, up))
    w = _unit(frm - to)
    u = _unit(_cross(up, w))
    return frm, u, _cross(w, u), w


def _camera24(o, u, v, w, ll, hz, vt, lens, t0, t1):
    return np.concatenate([o, u, v, w, ll, hz, vt, [lens, t0, t1]]).astype(np.float64)


def io_perspective(frm, to, up, vfov, aspect, aperture=0.0, focus_dist=1.0, t0=0.0, t1=0.0, ft=np.float64):
    """ioPerspectiveCamera (ioCamera.h:64-90) as the 24 numbers of an rtw_camera."""
    o, u, v, w = io_camera(frm, to, up, ft)
    vfov, aspect, aperture, fd, t0, t1 = (ft(a) for a in _f32in(vfov, aspect, aperture, focus_dist, t0, t1))
    theta = vfov * ft(np.pi) / ft(180.0)
    hh = np.tan(theta / ft(2.0))
    hw = aspect * hh
    ll = o - (hw * fd) * u - (hh * fd) * v - fd * w
    return _camera24(o, u, v, w, ll, (ft(2.0) * hw * fd) * u, (ft(2.0) * hh * fd) * v, aperture / ft(2.0), t0, t1)


def io_environment(frm, to, up, t0=0.0, t1=0.0, ft=np.float64):
    """ioEnvironmentCamera (ioCamera.h:118-138) with the times passed on (module text)."""
    o, u, v, w = io_camera(frm, to, up, ft)
    z = np.zeros(3, ft)
    t0, t1 = (ft(a) for a in _f32in(t0, t1))
    return _camera24(o, u, v, w, z, z, z, 0.0, t0, t1)


def io_orthographic(frm, to, up, height, width, t0=0.0, t1=0.0, ft=np.float64):
    """ioOrthographicCamera (ioCamera.h:140-179) with the times passed on (module text)."""
    o, u, v, w = io_camera(frm, to, up, ft)
    height, width, t0, t1 = (ft(a) for a in _f32in(height, width, t0, t1))
    hh, hw = height / ft(2.0), width / ft(2.0)
    ll = o - hw * u - hh * v - w
    return _camera24(o, u, v, w, ll, (ft(2.0) * hw) * u, (ft(2.0) * hh) * v, 0.0, t0, t1)


def builder_units(c64, at_size=0.0):
    """Error units of the 24 numbers of a built camera. A frame vector's component: e_f = 8 (two normalisations and a cross product
    of components no larger than 1) + 3 at_size, where at_size is the size of `to` when the frame is re-derived from a target
    to = origin - w of the size of the origin (the host description's setCameraKind: `to` and from - to are rounded at that size,
    w is of size 1). horizontal and vertical: e_f times their length. lower_left: 8 times the sum of the sizes of its four terms
    plus e_f times the three that carry a frame vector. The origin, the lens radius and the times are copied or halved: they
    must be equal."""
    c = np.asarray(c64, np.float64)
    o, hz, vt = c[0:3], c[15:18], c[18:21]
    n_h, n_v = np.linalg.norm(hz), np.linalg.norm(vt)
    # the distance from the origin to the frame: what is left of lower_left - origin after half the horizontal and vertical
    f = np.linalg.norm(c[12:15] + 0.5 * hz + 0.5 * vt - o)
    e_f = 8.0 + 3.0 * at_size
    unit = np.zeros(24)
    unit[3:12] = e_f
    unit[12:15] = 8.0 * (np.abs(o).max() + 0.5 * n_h + 0.5 * n_v + f) + e_f * (0.5 * n_h + 0.5 * n_v + f)
    unit[15:18], unit[18:21] = e_f * n_h, e_f * n_v
    return unit


def builder_error(got, c64, at_size=0.0):
    """max |got - c64| / (2^-24 unit) over the numbers with a unit; the others must be equal to the float32 rounding of the law's."""
    got, c64 = np.asarray(got, np.float64), np.asarray(c64, np.float64)
    unit = builder_units(c64, at_size)
    exact = unit == 0
    assert np.array_equal(got[exact], c64[exact].astype(np.float32).astype(np.float64)), (got[exact], c64[exact])
    return float((np.abs(got - c64)[~exact] / (U * unit[~exact])).max())


# (builder, arguments): the inputs over which MEASURED_CONSTANT_BUILD is measured - the cameras the CPU test holds to the law
def _scene_camera_args(k, nx=200, ny=100):
    """The arguments of the host description's perspective camera of scene k (host/ioScene.h, the reference's ioScene.h)."""
    aspect = float(np.float32(nx) / np.float32(ny))
    return {0: ((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, aspect, 1.0, 10.0),
            1: ((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, aspect, 0.1, 10.0),
            3: ((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, aspect, 0.1, 10.0)}[k]


def scene_camera(k, kind, ft=np.float64):
    """The header camera of abi.build_scene(100 * kind + k, 200, 100): the scene's perspective camera, or the environment or
    orthographic camera the host description puts in its place - at the same position and frame (to = origin - w, up = v), the
    orthographic window being the perspective frame (height = |vertical|, width = |horizontal|) with lower_left taken relative to
    the position, since the device adds the position back (host/ioScene.h setCameraKind). The marshalled header carries lens radius
    0 and the shutter 0 .. 1 for every scene (host/SceneMarshal.h)."""
    p = io_perspective(*_scene_camera_args(k), ft=ft)
    if ft is np.float32:
        p = p.astype(np.float32).astype(np.float64)  # the chain continues from the float32 camera
    o, v, w, hz, vt = p[0:3], p[6:9], p[9:12], p[15:18], p[18:21]
    if kind == ENV:
        c = io_environment(o, (o.astype(ft) - w.astype(ft)), v, ft=ft)
    elif kind == ORTHO:
        nrm = lambda a: np.sqrt((a.astype(ft) * a.astype(ft)).sum())
        c = io_orthographic(o, (o.astype(ft) - w.astype(ft)), v, nrm(vt), nrm(hz), ft=ft)
        c[12:15] = c[12:15].astype(ft) - c[0:3].astype(ft)
    else:
        c = p
    c = c.copy()
    c[21:24] = (0.0, 0.0, 1.0)
    return c


def at_size(k, kind):
    """builder_units' at_size of scene_camera(k, kind): the size of the position where the frame goes through to = origin - w."""
    return 0.0 if kind == PERSP else float(np.abs(np.asarray(_scene_camera_args(k)[0], np.float64)).max())


BUILDER_INPUTS = {
    "look_at": (io_perspective, ((13.0, 2.0, 3.0), (1.0, 0.5, -2.0), (0, 1, 0), 35.0, 1.5, 0.2, 9.0, 0.25, 0.5)),
    "look_at_cornell": (io_perspective, ((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, 2.0, 1.0, 10.0, 0.0, 1.0)),
    "environment": (io_environment, ((0.3, 2.1, -0.7), (4.0, 1.0, 0.2), (0, 1, 0), 0.25, 0.75)),
    "orthographic": (io_orthographic, ((3.1, 4.2, 1.5), (3.0, 3.0, 1.4), (0, 0, 1), 12.0, 9.5, 0.1, 0.9)),
}


def measure_builder_constant():
    worst = 0.0
    for fn, args in BUILDER_INPUTS.values():
        worst = max(worst, builder_error(fn(*args, ft=np.float32).astype(np.float32), fn(*args)))
    for k in (0, 1, 3):
        for kind in (PERSP, ENV, ORTHO):
            worst = max(worst, builder_error(scene_camera(k, kind, np.float32).astype(np.float32), scene_camera(k, kind), at_size(k, kind)))
    return worst


# ---------------------------------------------------------------- scenes
def _with_camera(blob, cam, camera_type):
    h = abi.SceneHeader.from_buffer_copy(blob[:_HDR])
    h.camera = abi.Camera.from_buffer_copy(np.asarray(cam, np.float64).astype(np.float32).tobytes())
    h.camera_type = camera_type
    return bytes(h) + blob[_HDR:]


def camera_of(blob):
    """The 24 float32 of the blob's camera and its camera type."""
    h = abi.SceneHeader.from_buffer_copy(blob[:_HDR])
    return np.frombuffer(bytes(h.camera), np.float32).copy(), int(h.camera_type)


WALL_CENTRE = (0.37, -0.21)
WALLS = {"wall24": (6, 4, 2.03, 1.99, 8, 8, 0.5), "wall300": (20, 15, 0.61, 0.53, 32, 16, 1.0)}  # nx, ny, pitches, colour denominators, blue


def wall_scene(name):
    """nx x ny abutting z-rectangles in the plane z = 0 centred on WALL_CENTRE, tile (ix, iy) = primitive iy * nx + ix, emitting
    ((ix + 1) / den_x, (iy + 1) / den_y, blue) towards +z. No sky."""
    nx, ny, px, py, dx, dy, blue = WALLS[name]
    x0, y0 = WALL_CENTRE[0] - 0.5 * nx * px, WALL_CENTRE[1] - 0.5 * ny * py
    prims, mats, texs = [], [], []
    for iy in range(ny):
        for ix in range(nx):
            # one float32 edge per line of the grid, shared by the tiles on either side of it
            e = [float(np.float32(v)) for v in (x0 + ix * px, x0 + (ix + 1) * px, y0 + iy * py, y0 + (iy + 1) * py)]
            prims.append(S._prim(abi.PRIM_RECT_Z, (e[0], e[1], e[2], e[3], 0.0), material=len(mats)))
            mats.append(abi.Material(type=abi.MAT_DIFFUSE_LIGHT, texture=len(texs), fuzz_or_eta=0.0, bsdf_eval=-1))
            texs.append(S._constant(((ix + 1) / dx, (iy + 1) / dy, blue)))
    return S._scene(0, prims, mats, texs)


def wall_colours(name):
    """(n_prims + 1, 3) float32: the colour of every tile, and black for a miss at index -1."""
    nx, ny, _, _, dx, dy, blue = WALLS[name]
    col = np.array([((ix + 1) / dx, (iy + 1) / dy, blue) for iy in range(ny) for ix in range(nx)] + [(0.0, 0.0, 0.0)], np.float32)
    assert len(np.unique(col, axis=0)) == len(col)
    return col


SPHERE = dict(c0=(0.0, 0.0, 0.0), c1=(9.0, 0.0, 0.0), radius=1.4, t0=0.5, t1=2.0)
SHUTTER = (0.25, 0.75)


def sphere_scene():
    """The Lambertian moving sphere of the module text under the sky."""
    s = SPHERE
    return S._scene(1, [S._prim(abi.PRIM_MOVING_SPHERE, s["c0"] + (s["radius"],) + s["c1"] + (s["t0"], s["t1"]))],
                    [abi.Material(type=abi.MAT_LAMBERTIAN, texture=0, fuzz_or_eta=0.0, bsdf_eval=0)], [S._constant((1.0, 1.0, 1.0))])


# the three frames of the sky cases: (to - from, up, the camera axis that lies along world y and its sign)
FRAMES_OF_AXES = {"v": ((0, 0, -1), (0, 1, 0), (6, 1.0)), "w": ((0, -1, 0), (0, 0, 1), (9, 1.0)), "u": ((0, 0, -1), (1, 0, 0), (3, -1.0))}
SKY_FROM = (1.3, 2.7, -0.9)


def _sky_camera(kind, axes):
    look, up, _ = FRAMES_OF_AXES[axes]
    to = tuple(a + b for a, b in zip(SKY_FROM, look))
    if kind == "pinhole":
        return io_perspective(SKY_FROM, to, up, 50.0, 1.5, 0.0, 1.0, *SHUTTER)
    if kind == PERSP:
        return io_perspective(SKY_FROM, to, up, 50.0, 1.5, 1.0, 1.0, *SHUTTER)
    if kind == ENV:
        return io_environment(SKY_FROM, to, up, *SHUTTER)
    # its direction is -w for every pixel: tilted off the axes, so that the three frames read three inexact components
    return io_orthographic(SKY_FROM, tuple(a + b for a, b in zip(to, (0.3, -0.2, 0.1))), up, 3.0, 4.5, *SHUTTER)


def _wall_camera(which):
    cx, cy = WALL_CENTRE
    if which == "pinhole":
        return PERSP, io_perspective((cx, cy, 10.0), (cx, cy, 0.0), (0, 1, 0), 40.0, 1.5, 0.0, 10.0)
    if which == "lens":
        return PERSP, io_perspective((cx, cy, 10.0), (cx, cy, 0.0), (0, 1, 0), 40.0, 1.5, 1.2, 4.0)
    if which == "environment":
        return ENV, io_environment((cx, cy, 3.0), (cx, cy, 0.0), (0, 1, 0))
    # the origin enters twice: the window is centred on 2 * from - w
    return ORTHO, io_orthographic((0.5 * cx, 0.5 * cy, 5.0), (0.5 * cx, 0.5 * cy, 0.0), (0, 1, 0), 7.28, 10.92)


def _sphere_camera(which, shutter=SHUTTER):
    if which == "perspective":  # a frame of 14.4 x 3 at the sphere, 20 away
        vfov = float(np.degrees(2.0 * np.arctan(1.5 / 20.0)))
        return PERSP, io_perspective((4.5, 0.1, 20.0), (4.5, 0.1, 0.0), (0, 1, 0), vfov, 4.8, 0.0, 20.0, *shutter)
    if which == "environment":
        # 0.5 beside the centre's track: for a fifth of the time the sphere holds the camera and every ray hits it from inside
        return ENV, io_environment((4.5, 0.1, -0.5), (4.5, 0.1, -3.0), (0, 1, 0), *shutter)
    return ORTHO, io_orthographic((2.25, 0.05, 10.0), (2.25, 0.05, 0.0), (0, 1, 0), 3.0, 14.4, *shutter)


class Case:
    """One scene with one camera and one way of reading its samples: kind "sky", "wall" or "shutter"."""

    def __init__(self, kind, blob, cam, camera_type, wall=None, axes=None):
        self.kind, self.wall, self.axes = kind, wall, axes
        self.blob = _with_camera(blob, cam, camera_type)
        self.cam, self.camera_type = camera_of(self.blob)
        if wall:
            self.colours = wall_colours(wall)


def _cases():
    out = {}
    for kind in (PERSP, ENV, ORTHO):
        for axes in FRAMES_OF_AXES:
            out[f"sky-{KIND_NAMES[kind]}-{axes}"] = lambda kind=kind, axes=axes: Case("sky", _sky_blob(), _sky_camera(kind, axes), kind, axes=axes)
    for axes in FRAMES_OF_AXES:  # the reference's own camera: perspective, no lens
        out[f"sky-pinhole-{axes}"] = lambda axes=axes: Case("sky", _sky_blob(), _sky_camera("pinhole", axes), PERSP, axes=axes)
    for wall in WALLS:
        for which in ("pinhole", "lens", "environment", "orthographic"):
            out[f"{wall}-{which}"] = lambda wall=wall, which=which: Case("wall", _wall_blob(wall), _wall_camera(which)[1], _wall_camera(which)[0], wall=wall)
    for which in ("perspective", "environment", "orthographic"):
        out[f"shutter-{which}"] = lambda which=which: Case("shutter", _sphere_blob(), _sphere_camera(which)[1], _sphere_camera(which)[0])
    return out


@functools.lru_cache(maxsize=None)
def _sky_blob():
    """Sky and, a million units below and as far to the side, a rectangle of two by two that no ray of the tests meets
    (check_expectation and mean_expect assert it; straight below the camera the environment camera's pole would find it)."""
    return S._scene(1, [S._prim(abi.PRIM_RECT_Y, (1.0e6, 1.0e6 + 2.0, 3.0e5, 3.0e5 + 2.0, -1.0e6))],
                    [abi.Material(type=abi.MAT_LAMBERTIAN, texture=0, fuzz_or_eta=0.0, bsdf_eval=0)], [S._constant((1.0, 1.0, 1.0))])


@functools.lru_cache(maxsize=None)
def _wall_blob(name):
    return wall_scene(name)


@functools.lru_cache(maxsize=None)
def _sphere_blob():
    return sphere_scene()


CASES = _cases()
# one mean of MEAN_SPP samples per camera kind, and the lens-free perspective camera's in all three frames: the whole direction of
# the rays k_path's hot instantiation makes ahead of time
MEAN_CASES = tuple(f"sky-{KIND_NAMES[k]}-v" for k in (PERSP, ENV, ORTHO)) + tuple(f"sky-pinhole-{a}" for a in FRAMES_OF_AXES)


def lens_free_reference_camera(name):
    """True for the cases whose scene and camera are the reference's own kind: a perspective camera without a lens over static
    surfaces with constant textures and no media. The scene preparation gives every other case - a lens, another camera kind, the
    moving sphere - to the kernel instantiations that hold the cold features (csrc/rtw_scene.h, has_tex), so these are the cases
    that reach k_path's LDS frame and, under Philox, its reserve of camera rays: sky-pinhole-* and wall24-pinhole (wall300 renders
    through the tree and k_first)."""
    c = case(name)
    parts = abi.parse_scene(c.blob)
    plain = all(p.type in (abi.PRIM_SPHERE, abi.PRIM_RECT_X, abi.PRIM_RECT_Y, abi.PRIM_RECT_Z) for p in parts["prims"])
    constant = all(t.type == abi.TEX_CONSTANT for t in parts["textures"])
    return c.camera_type == PERSP and c.cam[21] == 0.0 and plain and constant


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ---------------------------------------------------------------- what the law expects of a frame of one-sample pixels
def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def expect_of(c, frame, sample, seed, rng_kind, key=None, **wrong):
    """The law's answer for every pixel of `frame` at sample index `sample` for a Case-like object (cam, camera_type, blob, kind).
    `key` overrides the frame's own stream keys (rtw_views: the pixel within the view). Returns a dict of (R, W) arrays:
      y, unit        the world y of the unit direction and its error unit (decoded y)
      red, rays      the sky's red along the float64 direction; the ray's float32 rounding (n, 8)
      prim, well     geometry_ref's closest hit of the float32-rounded ray (sky: all -1), the conditioning mask of the module text
      depth, depth_unit   t |d| and its error unit (inf on a miss)
    **wrong: the negative controls of camera_rays, times and draws."""
    dkw = {k: wrong.pop(k) for k in ("lens_draws_for_all", "ray_time_own_draw") if k in wrong}
    tkw = {k: wrong.pop(k) for k in ("times_swapped", "ray_time_over_shutter", "gather_raw") if k in wrong}
    d = draws(frame.keys() if key is None else key, sample, seed, rng_kind, c.camera_type, **dkw)
    out = {}
    per_ft = {}
    for ft in (np.float64, np.float32):
        o, dr, e_o, e_d = camera_rays(c.cam, c.camera_type, frame, d, ft, **wrong)
        g, rt = times(c.cam, d, ft, **tkw)
        rays = rays8(o, dr)
        hit = G.closest_hit(c.blob, rays, rt.ravel().astype(np.float32), g.ravel().astype(np.float32))
        per_ft[ft] = (o, dr, e_o, e_d, g, rt, rays, hit)
    o, dr, e_o, e_d, g, rt, rays, hit = per_ft[np.float64]
    shape = o.shape[:-1]
    length = np.sqrt((dr * dr).sum(-1))
    prim32 = per_ft[np.float32][7]["prim"].reshape(shape)
    prim = hit["prim"].reshape(shape)
    t = hit["t"].reshape(shape)
    out.update(red=S.sky_red(dr), rays=rays, prim=prim.astype(np.int32), y=dr[..., 1] / length, unit=8.0 + 2.0 * e_d / length,
               well=~hit["ill"].reshape(shape) & (prim == prim32))
    miss = prim < 0
    with np.errstate(invalid="ignore", divide="ignore"):
        dz = np.abs(dr[..., 2])
        out["depth"] = np.where(miss, np.inf, t * length)
        out["depth_unit"] = np.where(miss, np.inf, length * (hit["unit"].reshape(shape) + (e_o + t * e_d) / dz) + t * length * (e_d / length + 3.0))
    # the float32 evaluation of the same things, for the measured constants only (depth32 finishes it where it is wanted)
    out["y32"] = S.decode_uy(S.sky_red(per_ft[np.float32][1], np.float32))
    out["rays32"] = per_ft[np.float32][6]
    return _freeze(out)


def depth32(c, e):
    """t |d| of the law's float32 ray by geometry_ref's algebra in float32 (inf on a miss): measure_constants' other side."""
    shape = e["prim"].shape
    h32 = G.closest_hit_fp32(c.blob, e["rays32"])
    d32 = e["rays32"][:, 3:6]
    len32 = np.sqrt((d32 * d32).sum(-1, dtype=np.float32))
    return np.where(h32["prim"] < 0, np.inf, (h32["t"].astype(np.float32) * len32).astype(np.float64)).reshape(shape)


@functools.lru_cache(maxsize=None)
def _expect_small(name, frame, sample, seed, rng_kind):
    return expect_of(case(name), frame, sample, seed, rng_kind)


@functools.lru_cache(maxsize=64)
def _expect_large(name, frame, sample, seed, rng_kind):
    return expect_of(case(name), frame, sample, seed, rng_kind)


def expect(name, frame, sample, seed, rng_kind):
    """expect_of for a named case, computed once: every frame of 24 x 16 and its shards is kept (40 KB each), of the far corner's
    (1.4 MB each) the last 64."""
    small = len(frame.rows()) * frame.width <= 4096
    return (_expect_small if small else _expect_large)(name, frame, sample, seed, rng_kind)


def _share(mask):
    return float(1.0 - mask.mean())


Result = namedtuple("Result", "fig left n hits")


def check_expectation(c, e, img, what=""):
    """The assertions on one frame of one-sample pixels img (R, W, >= 3) against the expectation e. Returns the figures, how many
    samples were left out of the exact comparisons, of how many, and how many the law sees hit; check_run holds the pooled share."""
    img = np.asarray(img)
    red = img[..., 0].astype(np.float64)
    k_dir = K_FACTOR * MEASURED_CONSTANT_DIR[c.camera_type]
    well = e["well"]
    law_miss = e["prim"] < 0
    fig = f"{what}left out {int((~well).sum())} of {well.size}"
    res = lambda: Result(fig, int((~well).sum()), well.size, int((~law_miss).sum()))
    if c.kind == "wall":
        want = c.colours[e["prim"]]
        differ = (img[..., :3] != want).any(-1) & well
        fig += f", {int(differ.sum())} tiles differ, {int((~law_miss).sum())} samples on the wall"
        assert not differ.any(), fig
        return res()
    if c.kind == "sky":
        assert law_miss.all(), "a ray of a sky case meets the far rectangle"
        assert (red != 0).all(), fig + ": a lost sample"
    else:
        differ = ((red == 0) != ~law_miss) & well
        fig += f", {int(differ.sum())} of hit-or-miss differ, {int((~law_miss).sum())} hits"
        assert not differ.any(), fig
    seen = law_miss & (red != 0)  # nothing is left out of the direction comparison: every sample both sides call a miss
    err = np.abs(S.decode_uy(red) - e["y"])[seen] / (U * e["unit"][seen])
    worst = float(err.max()) if seen.any() else 0.0
    fig += f", decoded y off by {worst:.3f} units over {int(seen.sum())} directions (K = {k_dir:.3f})"
    assert worst <= k_dir, fig
    return res()


def check(name, frame, sample, seed, rng_kind, img, **wrong):
    c = case(name)
    e = expect_of(c, frame, sample, seed, rng_kind, **wrong) if wrong else expect(name, frame, sample, seed, rng_kind)
    return check_expectation(c, e, img, f"{name} {tuple(frame)} sample {sample}: ")


def check_run(name, rng_kind, draw, render, frames=None, **wrong):
    """Every (frame, sample offset) of one draw of a generator (runs) for case `name`: render(frame, sample, seed) -> (R, W, >= 3)
    one-sample pixels. Each frame is checked on its own; the share left out of the exact comparisons is pooled over the sample
    offsets of a frame and held to MAX_LEFT_OUT, and the moving sphere must be hit by MIN_HIT_SHARE of the samples of the frames
    that show it whole (those of 24 x 16 from key 0). `frames` restricts the run to some frame names. Returns the figures."""
    seed, todo = runs(rng_kind, draw)
    pool, figs = {}, []
    for fname, sample in todo:
        if frames is not None and fname not in frames:
            continue
        frame = FRAMES[fname]
        r = check(name, frame, sample, seed, rng_kind, render(frame, sample, seed), **wrong)
        figs.append(r.fig)
        a = pool.setdefault(fname, [0, 0, 0])
        a[0], a[1], a[2] = a[0] + r.left, a[1] + r.n, a[2] + r.hits
    for fname, (left, n, hits) in pool.items():
        line = f"{name} {fname}: left out {left} of {n} ({100 * left / n:.2f} %, cap {100 * MAX_LEFT_OUT:.0f} %), hit share {hits / n:.3f}"
        figs.append(line)
        assert left <= MAX_LEFT_OUT * n, line
        if case(name).kind == "shutter" and fname == "full":
            assert hits >= MIN_HIT_SHARE * n, line
    return "\n".join(figs)


def check_guides(c, e, prim, depth, what=""):
    """rtw_render_guides / rtw_views_guides at spp = 1 on a wall: prim exact on the well-conditioned samples, depth within the
    tolerance wherever the guide's primitive is the law's. Returns a Result; the caller pools the share left out (pooled)."""
    prim, depth = np.asarray(prim), np.asarray(depth, np.float64)
    well = e["well"]
    differ = (prim != e["prim"]) & well
    same = (prim == e["prim"]) & (prim >= 0)
    err = np.abs(depth[same] - e["depth"][same]) / (U * e["depth_unit"][same])
    worst = float(err.max()) if same.any() else 0.0
    k = K_FACTOR * MEASURED_CONSTANT_DEPTH
    fig = (f"{what}left out {int((~well).sum())} of {well.size}, {int(differ.sum())} primitives differ, depth off by {worst:.3f} units over "
           f"{int(same.sum())} hits (K = {k:.3f})")
    assert not differ.any(), fig
    assert np.isinf(depth[(prim < 0)]).all() and (depth[prim < 0] > 0).all(), fig + ": a miss without depth +inf"
    assert worst <= k, fig
    return Result(fig, int((~well).sum()), well.size, int((e["prim"] >= 0).sum()))


def pooled(results, what=""):
    """The share left out of the exact comparisons over a list of Results (the sample offsets of one frame), held to MAX_LEFT_OUT."""
    left, n = sum(r.left for r in results), sum(r.n for r in results)
    line = f"{what}left out {left} of {n} ({100 * left / n:.2f} %, cap {100 * MAX_LEFT_OUT:.0f} %)"
    assert left <= MAX_LEFT_OUT * n, line
    return line


def mean_expect(name, seed, rng_kind, frame=FULL, spp=MEAN_SPP, one_sample_late=False):
    """(the float64 mean of the law's reds over samples 0 .. spp - 1, the largest per-sample unit of decoded y) per pixel.
    one_sample_late is a negative control: sample spp stands in for sample 0, as if a ray made ahead of time were handed out one
    sample late."""
    reds, unit = 0.0, 0.0
    for s in range(1, spp + 1) if one_sample_late else range(spp):
        e = expect(name, frame, s, seed, rng_kind)
        assert (e["prim"] < 0).all(), "a ray of a sky case meets the far rectangle"
        reds = reds + e["red"]
        unit = np.maximum(unit, e["unit"])
    return reds / spp, unit


def check_mean(name, seed, rng_kind, img, spp=MEAN_SPP, **wrong):
    """A pixel of spp samples of a sky case: red is affine in u.y, so the pixel is held to the float64 mean of the law's reds within
    the per-sample bound of a red plus the summation term."""
    c = case(name)
    want, unit = mean_expect(name, seed, rng_kind, spp=spp, **wrong)
    tol = U * (K_FACTOR * MEASURED_CONSTANT_DIR[c.camera_type] * unit / 4.0 + sum_units(spp))
    err = np.abs(np.asarray(img)[..., 0].astype(np.float64) - want)
    fig = f"{name} mean of {spp}: red off by at most {float((err / U).max()):.2f} units of 2^-24, {float((err / tol).max()):.3f} of the tolerance"
    assert (err <= tol).all(), fig
    return fig


# ---------------------------------------------------------------- the oracle's samples
@functools.lru_cache(maxsize=None)
def oracle_frame(name, frame, sample, seed, rng_kind, spp=1):
    """(R, W, 4) float32: the oracle's render of case `name`, computed once and left unchanged."""
    import oracle
    img, _ = oracle.render(case(name).blob, frame.params(spp, sample, seed, rng_kind))
    img.setflags(write=False)
    return img


# ---------------------------------------------------------------- the measurement behind the MEASURED_CONSTANT_* values
def measure_constants(verbose=False):
    """This file at float32 against itself at float64 over the frames, sample offsets and draws of the tests, in the stated units:
    ({camera kind: direction constant}, depth constant, {case: the largest share left out of a frame's pooled sample offsets})."""
    dirs, depth, left = {k: 0.0 for k in KIND_NAMES}, 0.0, {}
    for name in CASES:
        c = case(name)
        k_dir = k_depth = worst_left = 0.0
        for rng in RNGS:
            for draw in range(2):
                seed, todo = runs(rng, draw)
                pool = {}
                for fname, s in todo:
                    e = expect(name, FRAMES[fname], s, seed, rng)
                    a = pool.setdefault(fname, [0, 0])
                    a[0], a[1] = a[0] + int((~e["well"]).sum()), a[1] + e["well"].size
                    miss = e["prim"] < 0
                    if c.kind != "wall" and miss.any():
                        k_dir = max(k_dir, float((np.abs(e["y32"] - e["y"])[miss] / (U * e["unit"][miss])).max()))
                    if c.kind == "wall" and (~miss).any():
                        d32 = depth32(c, e)
                        hit = ~miss & e["well"] & np.isfinite(d32)
                        if hit.any():
                            k_depth = max(k_depth, float((np.abs(d32[hit] - e["depth"][hit]) / (U * e["depth_unit"][hit])).max()))
                worst_left = max([worst_left] + [a[0] / a[1] for a in pool.values()])
        if verbose:
            print(f"{name:26s} direction {k_dir:.4f}  depth {k_depth:.4f}  largest left-out share {100 * worst_left:.2f} %")
        dirs[c.camera_type] = max(dirs[c.camera_type], k_dir)
        depth = max(depth, k_depth)
        left[name] = worst_left
    return dirs, depth, left


def self_checks():
    """Checks that need no quadrature: the generators against their published answers, the summation term, the frames of the sky
    cases, the builders' orthonormal frames."""
    assert int(tea(64, 0, 0)) == 0x437C1053 and int(tea(16, 0, 0)) == 0x741C187D
    assert [int(w) for w in philox4x32_10((0, 0, 0, 0), (0, 0))] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert abs(sum_units(144) - ((8 * 135 + 560) + 135 + 144) / 144 - 1.0) < 1e-12 and sum_units(1) == 1.0
    for axes, (_, _, (at, sign)) in FRAMES_OF_AXES.items():
        cam = _sky_camera(ENV, axes)
        assert np.allclose(cam[at:at + 3], (0.0, sign, 0.0), atol=1e-15), axes
    for fn, args in BUILDER_INPUTS.values():
        cam = fn(*args)
        m = cam[3:12].reshape(3, 3)
        assert np.allclose(m @ m.T, np.eye(3), atol=1e-12) and np.allclose(np.cross(m[0], m[1]), m[2], atol=1e-12)
    return "tea, philox, the summation term, the sky frames and the builders' frames: as stated"


if __name__ == "__main__":
    print(self_checks())
    dirs_, depth_, left_ = measure_constants(verbose=True)
    print("MEASURED_CONSTANT_DIR = {" + ", ".join(f"{KIND_NAMES[k]}: {v:.4f}" for k, v in dirs_.items()) + "}")
    print(f"MEASURED_CONSTANT_DEPTH = {depth_:.4f}")
    print(f"MEASURED_CONSTANT_BUILD = {measure_builder_constant():.4f}")
    print(f"largest left-out share {100 * max(left_.values()):.2f} % (cap {100 * MAX_LEFT_OUT:.0f} %)")
    print(f"sum_units({MEAN_SPP}) = {sum_units(MEAN_SPP):.4f}")
