"""ctypes mirror of include/rtw.h and loaders for the in-tree shared libraries.

Plumbing only: scene blobs come from the C++ host description (librtw_host.so), rendering is
done by the HIP library (librtw_hip.so) through its C ABI. There is no Python or CPU fallback:
`load_hip()` raises if the HIP library has not been built.
"""
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
HOST_LIB = os.path.join(PKG_DIR, "host", "librtw_host.so")
HIP_LIB = os.environ.get("RTW_HIP_LIB") or os.path.join(PKG_DIR, "csrc", "librtw_hip.so")

RTW_ABI_VERSION = 5
RTW_SCENE_VERSION = 1
RTW_SCENE_MAGIC = 0x57545221
RTW_RNG_PHILOX = 0
RTW_RNG_TEA_LCG = 1
RTW_EST_REFERENCE, RTW_EST_CORRECTED, RTW_EST_CORRECTED_NO_NEE, RTW_EST_MIXTURE = range(4)

# rtw_prim_type
PRIM_SPHERE, PRIM_MOVING_SPHERE, PRIM_RECT_X, PRIM_RECT_Y, PRIM_RECT_Z, PRIM_VOLUME_BOX, PRIM_VOLUME_SPHERE = range(7)
# rtw_material_type
MAT_LAMBERTIAN, MAT_DIFFUSE_LIGHT, MAT_METAL, MAT_DIELECTRIC, MAT_ISOTROPIC, MAT_NORMAL = range(6)
# rtw_pdf_gen
RTW_PDF_COSINE, RTW_PDF_MIXTURE_BIAS, RTW_PDF_MIXTURE, RTW_PDF_RECT_X, RTW_PDF_RECT_Y, RTW_PDF_RECT_Z = range(6)
# rtw_camera_type
RTW_CAM_PERSPECTIVE, RTW_CAM_ENVIRONMENT, RTW_CAM_ORTHOGRAPHIC = range(3)
# rtw_texture_type
TEX_CHECKER, TEX_CONSTANT, TEX_IMAGE, TEX_NOISE, TEX_NULL = range(5)


class Prim(C.Structure):
    _fields_ = [("type", C.c_int32), ("material", C.c_int32), ("xform", C.c_int32), ("flip", C.c_int32),
                ("p", C.c_float * 12)]


class Xform(C.Structure):
    _fields_ = [("m", C.c_float * 12), ("inv", C.c_float * 12)]


class Material(C.Structure):
    _fields_ = [("type", C.c_int32), ("texture", C.c_int32), ("fuzz_or_eta", C.c_float), ("bsdf_eval", C.c_int32)]


class Texture(C.Structure):
    _fields_ = [("type", C.c_int32), ("color", C.c_float * 3), ("odd", C.c_int32), ("even", C.c_int32),
                ("scale", C.c_float), ("data", C.c_uint32)]


class Light(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("vec_u", C.c_float * 3), ("vec_v", C.c_float * 3),
                ("normal", C.c_float * 3), ("area", C.c_float), ("emission", C.c_float * 3)]


class Pdf(C.Structure):
    _fields_ = [("gen", C.c_int32), ("p0_gen", C.c_int32), ("p1_gen", C.c_int32), ("flip", C.c_int32),
                ("rect", C.c_float * 5), ("bias", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("w", C.c_float * 3),
                ("lower_left", C.c_float * 3), ("horizontal", C.c_float * 3), ("vertical", C.c_float * 3),
                ("lens_radius", C.c_float), ("time0", C.c_float), ("time1", C.c_float)]


class SceneHeader(C.Structure):
    _fields_ = [("magic", C.c_uint32), ("version", C.c_uint32), ("total_bytes", C.c_uint32),
                ("n_prims", C.c_uint32), ("n_xforms", C.c_uint32), ("n_materials", C.c_uint32),
                ("n_textures", C.c_uint32), ("n_lights", C.c_uint32),
                ("off_prims", C.c_uint32), ("off_xforms", C.c_uint32), ("off_materials", C.c_uint32),
                ("off_textures", C.c_uint32), ("off_lights", C.c_uint32),
                ("sky_light", C.c_int32), ("off_texdata", C.c_uint32), ("texdata_bytes", C.c_uint32),
                ("camera", Camera), ("pdf", Pdf), ("camera_type", C.c_int32), ("reserved", C.c_uint32)]


class Params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32),
                ("seed", C.c_uint32), ("row0", C.c_int32), ("row1", C.c_int32), ("rng_kind", C.c_int32),
                ("sample_offset", C.c_int32), ("samples_per_pass", C.c_int32), ("row_stride", C.c_int32), ("estimator", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("segments", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("algorithmic_bytes", C.c_uint64), ("bounce_launches", C.c_uint64), ("reserved", C.c_uint64),
                ("seconds", C.c_double), ("bounce_seconds", C.c_double),
                ("kernel_seconds", C.c_double * 5), ("kernel_launches", C.c_uint64 * 5), ("kernel_segments", C.c_uint64 * 5)]

    KERNELS = ("k_first", "k_shade", "k_trace", "k_bounce", "k_path")

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class Guides(C.Structure):
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("prim", C.c_void_p)]


class Adaptive(C.Structure):
    """rtw_adaptive (include/rtw.h): the schedule and stop rule of rtw_render_adaptive."""
    _fields_ = [("min_spp", C.c_int32), ("step_spp", C.c_int32), ("threshold", C.c_float), ("dilate", C.c_int32)]


class AccumInfo(C.Structure):
    """rtw_accum_info (include/rtw.h): what rtw_accum_status reports."""
    _fields_ = [("active", C.c_int32), ("done", C.c_int32), ("cap", C.c_int32), ("flags", C.c_uint32), ("state_bytes", C.c_uint64),
                ("samples", C.c_uint64), ("segments", C.c_uint64), ("shadow_rays", C.c_uint64), ("params", Params)]


class Hits(C.Structure):
    """rtw_hits (include/rtw.h): the output pointers of rtw_cast / rtw_cast_device, NULL for an output nobody wants."""
    _fields_ = [("t", C.c_void_p), ("prim", C.c_void_p), ("material", C.c_void_p), ("normal", C.c_void_p), ("uv", C.c_void_p)]


class RadianceParams(C.Structure):
    """rtw_radiance_params (include/rtw.h): the sampling of rtw_radiance / rtw_radiance_device."""
    _fields_ = [("spp", C.c_int32), ("max_depth", C.c_int32), ("seed", C.c_uint32), ("rng_kind", C.c_int32),
                ("sample_offset", C.c_int32), ("estimator", C.c_int32), ("key_offset", C.c_uint32), ("reserved", C.c_uint32)]


class ProbeParams(C.Structure):
    """rtw_probe_params (include/rtw.h): the sampling and the mode of rtw_probe / rtw_probe_device."""
    _fields_ = [("spp", C.c_int32), ("max_depth", C.c_int32), ("seed", C.c_uint32), ("rng_kind", C.c_int32),
                ("sample_offset", C.c_int32), ("estimator", C.c_int32), ("key_offset", C.c_uint32), ("mode", C.c_int32)]


class View(C.Structure):
    """rtw_view (include/rtw.h): one camera of rtw_views / rtw_views_device and the seed of its frame."""
    _fields_ = [("camera", Camera), ("camera_type", C.c_int32), ("seed", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class ViewParams(C.Structure):
    """rtw_view_params (include/rtw.h): the frame size and the sampling all views of a call share."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32), ("rng_kind", C.c_int32),
                ("sample_offset", C.c_int32), ("estimator", C.c_int32), ("reserved", C.c_uint32)]


class PathVertex(C.Structure):
    """rtw_path_vertex (include/rtw.h): one traced segment of a replayed path."""
    _fields_ = [("o", C.c_float * 3), ("t", C.c_float), ("d", C.c_float * 3), ("prim", C.c_int32), ("contribution", C.c_float * 3),
                ("flags", C.c_uint32), ("throughput", C.c_float * 3), ("ray_time", C.c_float)]


class PathHead(C.Structure):
    """rtw_path_head (include/rtw.h): one replayed sample."""
    _fields_ = [("radiance", C.c_float * 3), ("segments", C.c_int32), ("gather_time", C.c_float), ("shadow_rays", C.c_int32),
                ("key", C.c_uint32), ("sample", C.c_uint32)]


class PathsParams(C.Structure):
    """rtw_paths_params (include/rtw.h): rtw_radiance's sampling and the number of vertices kept per sample."""
    _fields_ = [("spp", C.c_int32), ("max_depth", C.c_int32), ("seed", C.c_uint32), ("rng_kind", C.c_int32),
                ("sample_offset", C.c_int32), ("estimator", C.c_int32), ("key_offset", C.c_uint32), ("max_records", C.c_int32),
                ("reserved", C.c_uint32 * 2)]


# the two records as numpy sees them: structured dtypes with rtw.h's field names, sizes and offsets
PATH_VERTEX = np.dtype([("o", np.float32, 3), ("t", np.float32), ("d", np.float32, 3), ("prim", np.int32), ("contribution", np.float32, 3),
                        ("flags", np.uint32), ("throughput", np.float32, 3), ("ray_time", np.float32)])
PATH_HEAD = np.dtype([("radiance", np.float32, 3), ("segments", np.int32), ("gather_time", np.float32), ("shadow_rays", np.int32),
                      ("key", np.uint32), ("sample", np.uint32)])
# rtw_path_vertex.flags: the event in the low two bits, then the light sample's two bits
RTW_PATH_MISS, RTW_PATH_SCATTER, RTW_PATH_END, RTW_PATH_CANCEL = range(4)
RTW_PATH_EVENT_MASK, RTW_PATH_LIGHT_SAMPLED, RTW_PATH_LIGHT_ADDED = 3, 4, 8

_PTR, _STATS = C.c_void_p, C.POINTER(Stats)
_DENOISE = [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float]  # two sizes, iterations, the three sigmas


def _query(params, *outputs):
    """The argtypes of a query call and of its _device variant (the stream before the stats): context, batch, n, the parameter
    structs, the outputs, stats."""
    head = [_PTR, _PTR, C.c_size_t] + [C.POINTER(p) for p in params] + list(outputs)
    return head + [_STATS], head + [_PTR, _STATS]


# include/rtw.h's entry points: name -> argtypes. All return int but rtw_last_error, a C string.
HIP_SIGNATURES = {
    "rtw_abi_version": [],
    "rtw_create": [C.POINTER(_PTR), C.c_int, C.POINTER(C.c_int)],
    "rtw_upload_scene": [_PTR, _PTR, C.c_size_t],
    "rtw_render": [_PTR, C.POINTER(Params), _PTR, _STATS],
    "rtw_render_device": [_PTR, C.POINTER(Params), _PTR, _PTR, _STATS],
    "rtw_destroy": [_PTR],
    "rtw_last_error": [_PTR],
    "rtw_debug_intersect": [_PTR, _PTR, _PTR, _PTR, C.c_int, _PTR, _PTR],
    "rtw_denoise": [_PTR, _PTR, _PTR, C.c_int32, C.c_int32, C.c_int32, C.c_float],
    "rtw_render_guides": [_PTR, C.POINTER(Params), C.POINTER(Guides), _STATS],
    "rtw_denoise_guided": [_PTR, _PTR, _PTR, _PTR, _PTR] + _DENOISE,
    "rtw_render_adaptive": [_PTR, C.POINTER(Params), C.POINTER(Adaptive), _PTR, _PTR, _PTR, _STATS],
    "rtw_debug_math": [_PTR, C.c_int, C.POINTER(C.c_uint64)],
    "rtw_accum_begin": [_PTR, C.POINTER(Params), C.c_uint32],
    "rtw_accum_add": [_PTR, C.c_int32, _STATS],
    "rtw_accum_read": [_PTR, _PTR, _PTR],
    "rtw_accum_read_device": [_PTR, _PTR, _PTR],
    "rtw_accum_status": [_PTR, C.POINTER(AccumInfo)],
    "rtw_accum_save": [_PTR, _PTR, C.c_size_t],
    "rtw_accum_restore": [_PTR, _PTR, C.c_size_t],
    "rtw_accum_end": [_PTR],
    "rtw_cast": [_PTR, _PTR, _PTR, _PTR, C.c_size_t, C.c_int32, C.POINTER(Hits), _STATS],
    "rtw_cast_device": [_PTR, _PTR, _PTR, _PTR, C.c_size_t, C.c_int32, C.POINTER(Hits), _PTR, _STATS],
    "rtw_denoise_views": [_PTR, _PTR, _PTR, _PTR, _PTR, C.c_size_t] + _DENOISE,
    "rtw_denoise_views_device": [_PTR, _PTR, _PTR, _PTR, _PTR, C.c_size_t] + _DENOISE + [_PTR],
}
for _name, _sig in (("rtw_radiance", _query([RadianceParams], _PTR)), ("rtw_probe", _query([ProbeParams], _PTR)),
                    ("rtw_probe_sh", _query([RadianceParams], _PTR)), ("rtw_views", _query([ViewParams], _PTR)),
                    ("rtw_probe_adaptive", _query([ProbeParams, Adaptive], _PTR, _PTR, _PTR)),
                    ("rtw_views_guides", _query([ViewParams, Guides])),
                    ("rtw_views_adaptive", _query([ViewParams, Adaptive], _PTR, _PTR, _PTR)),
                    ("rtw_paths", _query([PathsParams], _PTR, _PTR)),
                    ("rtw_paths_views", _query([ViewParams], C.c_uint64, C.c_uint64, C.c_int32, _PTR, _PTR))):
    HIP_SIGNATURES[_name], HIP_SIGNATURES[_name + "_device"] = _sig
HIP_SYMBOLS = list(HIP_SIGNATURES)
PROBE_MODES = {"irradiance": 0, "occlusion": 1}  # RTW_PROBE_IRRADIANCE, RTW_PROBE_OCCLUSION
CAST_MODES = {"closest": 0, "any": 1}  # RTW_CAST_CLOSEST, RTW_CAST_ANY
# rtw_hits' outputs: name -> (numpy dtype, trailing shape)
CAST_OUTPUTS = {"t": (np.float32, ()), "prim": (np.int32, ()), "material": (np.int32, ()), "normal": (np.float32, (4,)), "uv": (np.float32, (2,))}
RTW_ACCUM_ERROR = 1  # rtw_accum_begin's flag: keep the moments, so that accum_read can return the error map
MATH_OPS = {"rcp": 0, "sqrt": 1, "rcp_sqrt": 2, "rcp_one_step": 3, "rcp_two_steps": 4, "sqrt_residual_only": 5, "sqrt_coupled": 6}  # rtw_debug_math's op
GUIDES = ("albedo", "normal", "depth", "prim")
# a guide buffer: name -> (trailing shape, dtype name) after the leading (rows, w) or (n, h, w)
GUIDE_LAYOUT = {"albedo": ((4,), "float32"), "normal": ((4,), "float32"), "depth": ((), "float32"), "prim": ((), "int32")}
# Default edge-stopping sigmas of Renderer.denoise_guided (see there)
DENOISE_SIGMA_ALBEDO = 0.4
DENOISE_SIGMA_NORMAL = 0.5

_host = None
_hip = None


def load_host():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise RuntimeError(f"{HOST_LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(HOST_LIB)
        lib.rtw_host_build_scene.restype = C.c_int
        lib.rtw_host_build_scene.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        _host = lib
    return _host


def load_hip():
    """Load librtw_hip.so. Fails loudly when it is absent: there is no fallback path."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB):
            raise RuntimeError(f"{HIP_LIB} is missing: the HIP extension must be built "
                               "(`python -c 'import __graft_entry__ as g; g.build()'`); no CPU fallback exists")
        lib = C.CDLL(HIP_LIB)
        for name, argtypes in HIP_SIGNATURES.items():
            f = getattr(lib, name)
            f.restype, f.argtypes = (C.c_char_p if name == "rtw_last_error" else C.c_int), argtypes
        if lib.rtw_abi_version() != RTW_ABI_VERSION:
            raise RuntimeError("librtw_hip.so ABI version mismatch")
        _hip = lib
    return _hip


def build_scene(scene, nx, ny):
    """Scene blob (bytes) of reference scene 0/1/3 for an nx x ny image, from the C++ host description."""
    lib = load_host()
    need = C.c_size_t(0)
    rc = lib.rtw_host_build_scene(scene, nx, ny, None, 0, C.byref(need))
    if rc == -1:
        raise ValueError(f"unknown scene {scene}")
    buf = C.create_string_buffer(need.value)
    rc = lib.rtw_host_build_scene(scene, nx, ny, buf, need.value, C.byref(need))
    if rc != 0:
        raise RuntimeError(f"rtw_host_build_scene failed: {rc}")
    return buf.raw


def parse_scene(blob):
    """Decode a scene blob into ctypes views (header, prims, xforms, materials, textures, lights)."""
    h = SceneHeader.from_buffer_copy(blob[:C.sizeof(SceneHeader)])

    def arr(t, off, n):
        return (t * n).from_buffer_copy(blob[off:off + n * C.sizeof(t)])
    return {
        "header": h,
        "prims": arr(Prim, h.off_prims, h.n_prims),
        "xforms": arr(Xform, h.off_xforms, h.n_xforms),
        "materials": arr(Material, h.off_materials, h.n_materials),
        "textures": arr(Texture, h.off_textures, h.n_textures),
        "lights": arr(Light, h.off_lights, h.n_lights),
        "texdata": bytes(blob[h.off_texdata:h.off_texdata + h.texdata_bytes]) if h.off_texdata else b"",
    }


def assemble_scene(parts):
    """Inverse of parse_scene: serialise {"header", "prims", "xforms", "materials", "textures", "lights"[, "texdata"]}
    (ctypes arrays or lists of the structs, texdata = bytes of the texture data section) into a blob; counts, offsets
    and total_bytes are recomputed."""
    src = parts["header"]
    h = SceneHeader.from_buffer_copy(bytes(src))
    tables = [list(parts[k]) for k in ("prims", "xforms", "materials", "textures", "lights")]
    h.n_prims, h.n_xforms, h.n_materials, h.n_textures, h.n_lights = (len(t) for t in tables)
    sizes = [C.sizeof(t) for t in (Prim, Xform, Material, Texture, Light)]
    offs = [(C.sizeof(SceneHeader) + 15) // 16 * 16]
    for t, sz in zip(tables, sizes):
        offs.append((offs[-1] + len(t) * sz + 15) // 16 * 16)
    h.off_prims, h.off_xforms, h.off_materials, h.off_textures, h.off_lights = offs[:5]
    texdata = bytes(parts.get("texdata", b""))
    h.off_texdata, h.texdata_bytes = (offs[5], len(texdata)) if texdata else (0, 0)
    h.total_bytes = (offs[5] + len(texdata) + 15) // 16 * 16
    buf = bytearray(h.total_bytes)
    buf[offs[5]:offs[5] + len(texdata)] = texdata
    buf[0:C.sizeof(SceneHeader)] = bytes(h)
    for t, sz, off in zip(tables, sizes, offs):
        for i, obj in enumerate(t):
            buf[off + i * sz:off + (i + 1) * sz] = bytes(obj)
    return bytes(buf)


def _positive(prefix, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
        raise ValueError(f"{prefix}: {name} = {v!r}, expected a positive integer")


def _batch(prefix, name, a):
    """The (n, 8) float32 batch of a query, contiguous. Anything that is not a float32 ndarray already is refused, not converted."""
    if not isinstance(a, np.ndarray) or a.dtype != np.float32:
        raise ValueError(f"{prefix}: {name} must be a float32 numpy array")
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError(f"{prefix}: {name} of shape {a.shape}, expected (n, 8)")
    return np.ascontiguousarray(a)


def _check_pixels(prefix, n, width, height):
    if n * int(width) * int(height) > 0x7fffffff:
        raise ValueError(f"{prefix}: more than 2^31 - 1 pixels in one call")


def _view_batch(prefix, views, width, height, spp, max_depth, rng_kind, sample_offset, estimator):
    """(the View array, the rtw_view_params) of a host call on views, refused when it has too many pixels."""
    arr = view_array(views)
    vp = make_view_params(width, height, spp, max_depth, rng_kind, sample_offset, estimator)
    _check_pixels(prefix, len(arr), width, height)
    return arr, vp


def _guide_names(prefix, which):
    which = tuple(which)
    bad = [k for k in which if k not in GUIDES]
    if bad or not which:
        raise ValueError(f"{prefix}: unknown or no guide names {bad or which}")
    return which


def _guide_buffers(which, lead):
    """({name: array of shape lead + the guide's own}, the Guides that points at them)"""
    out = {k: np.empty(lead + GUIDE_LAYOUT[k][0], GUIDE_LAYOUT[k][1]) for k in which}
    return out, Guides(**{k: v.ctypes.data for k, v in out.items()})


def _adaptive_outputs(lead):
    """(values, sample counts, errors) of an adaptive call over `lead` pixels or probes"""
    return np.empty(lead + (4,), dtype=np.float32), np.empty(lead, dtype=np.int32), np.empty(lead, dtype=np.float32)


def _ref(stats):
    return None if stats is None else C.byref(stats)


def _ptr(a):
    return None if a is None else a.ctypes.data


def make_params(width, height, spp, max_depth, seed=0x6314759, row0=0, row1=None, rng_kind=RTW_RNG_PHILOX,
                sample_offset=0, samples_per_pass=0, row_stride=0, estimator=0):
    p = Params()
    p.width, p.height, p.spp, p.max_depth = width, height, spp, max_depth
    p.seed = seed
    p.row0 = row0
    p.row1 = height if row1 is None else row1
    p.rng_kind = rng_kind
    p.sample_offset = sample_offset
    p.samples_per_pass = samples_per_pass
    p.row_stride = row_stride
    p.estimator = estimator
    return p


def make_radiance_params(spp, max_depth, seed=0x6314759, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0, key_offset=0):
    """rtw_radiance_params; spp must be a positive integer (the library checks the rest)."""
    _positive("radiance", "spp", spp)
    return RadianceParams(int(spp), int(max_depth), seed & 0xffffffff, rng_kind, sample_offset, estimator, key_offset & 0xffffffff, 0)


def make_probe_params(spp, max_depth, seed=0x6314759, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0, key_offset=0, mode="irradiance"):
    """rtw_probe_params; spp must be a positive integer and mode "irradiance" or "occlusion" (the library checks the rest)."""
    _positive("probe", "spp", spp)
    if mode not in PROBE_MODES:
        raise ValueError(f"probe: mode {mode!r} is neither 'irradiance' nor 'occlusion'")
    return ProbeParams(int(spp), int(max_depth), seed & 0xffffffff, rng_kind, sample_offset, estimator, key_offset & 0xffffffff, PROBE_MODES[mode])


def make_paths_params(spp, max_depth, max_records=None, seed=0x6314759, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0, key_offset=0):
    """rtw_paths_params; spp must be a positive integer and max_records (None: max_depth, every vertex) an integer in 0 .. max_depth."""
    _positive("paths", "spp", spp)
    k = _max_records("paths", max_records, max_depth)
    return PathsParams(int(spp), int(max_depth), seed & 0xffffffff, rng_kind, sample_offset, estimator, key_offset & 0xffffffff, k, (C.c_uint32 * 2)(0, 0))


def _max_records(prefix, max_records, max_depth):
    if max_records is None:
        return max(int(max_depth), 0)
    if isinstance(max_records, bool) or not isinstance(max_records, (int, np.integer)) or not 0 <= max_records <= max(int(max_depth), 0):
        raise ValueError(f"{prefix}: max_records = {max_records!r}, expected an integer in 0 .. max_depth")
    return int(max_records)


def _check_pairs(prefix, n, spp):
    if n * int(spp) > 0x7fffffff:
        raise ValueError(f"{prefix}: more than 2^31 - 1 samples in one call")


def _path_window(prefix, first, count, total):
    """`first` of a window [first, first + count) of `total` flattened pixels, refused when it does not lie inside them."""
    for name, v in (("first", first), ("count", count)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"{prefix}: {name} = {v!r}, expected a non-negative integer")
    if first + count > total:
        raise ValueError(f"{prefix}: pixels [{first}, {first + count}) of {total}")
    return int(first)


def _path_buffers(n, spp, k):
    """(heads (n, spp), vertices (n, spp, k), zeroed: the library writes the first min(segments, k) of a sample alone)"""
    return np.zeros((n, int(spp)), dtype=PATH_HEAD), np.zeros((n, int(spp), k), dtype=PATH_VERTEX)


def make_view(camera, camera_type=RTW_CAM_PERSPECTIVE, seed=0x6314759):
    """rtw_view of a Camera (copied) or of anything Camera's 24 floats can be read from (bake.look_at's array): the camera, its
    rtw_camera_type and the seed of its frame."""
    if isinstance(camera, Camera):
        cam = Camera.from_buffer_copy(bytes(camera))
    else:
        a = np.ascontiguousarray(camera, dtype=np.float32)
        if a.shape != (24,):
            raise ValueError(f"make_view: camera of shape {a.shape}, expected a Camera or 24 floats")
        cam = Camera.from_buffer_copy(a.tobytes())
    if isinstance(camera_type, bool) or not isinstance(camera_type, (int, np.integer)) or not 0 <= camera_type <= 2:
        raise ValueError(f"make_view: camera_type = {camera_type!r}, expected 0, 1 or 2")
    v = View()
    v.camera = cam
    v.camera_type = int(camera_type)
    v.seed = int(seed) & 0xffffffff
    return v


def scene_view(blob, seed=0x6314759):
    """The scene blob's own camera and camera type as an rtw_view: its frame is render()'s frame of that blob under `seed`."""
    h = SceneHeader.from_buffer_copy(blob[:C.sizeof(SceneHeader)])
    return make_view(h.camera, h.camera_type, seed)


def view_array(views):
    """A contiguous ctypes array of View from a View, a sequence of them or such an array."""
    if isinstance(views, View):
        views = [views]
    if isinstance(views, C.Array) and views._type_ is View:
        return views
    views = list(views)
    if not all(isinstance(v, View) for v in views):
        raise ValueError("views: expected abi.View records (abi.make_view, abi.scene_view, bake.cube_views, bake.orbit_views)")
    return (View * len(views))(*views)


def make_view_params(width, height, spp, max_depth, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0):
    """rtw_view_params; width, height and spp must be positive integers (the library checks the rest)."""
    for name, v in (("width", width), ("height", height), ("spp", spp)):
        _positive("views", name, v)
    return ViewParams(int(width), int(height), int(spp), int(max_depth), rng_kind, sample_offset, estimator, 0)


def local_rows(params):
    """Number of image rows a render with these params produces."""
    k = max(1, params.row_stride)
    return max(0, (params.row1 - params.row0 + k - 1) // k)


class Renderer:
    """Thin owner of one rtw_ctx: one GPU (device=i) or an in-library group (device=[i, j, ...]: rtw_create with
    n_devices > 1, one interleaved row shard per entry, gathered on the first device)."""

    def __init__(self, device=0):
        self.lib = load_hip()
        self.ctx = C.c_void_p()
        ids = list(device) if isinstance(device, (list, tuple)) else [device]
        self.devices = ids  # a group's queries (guides, adaptive, sessions, casts) run on ids[0]
        dev = (C.c_int * len(ids))(*ids)
        rc = self.lib.rtw_create(C.byref(self.ctx), len(ids), dev)
        if rc != 0:
            raise RuntimeError(f"rtw_create failed: {rc}")

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.rtw_last_error(self.ctx)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def upload_scene(self, blob):
        self._check(self.lib.rtw_upload_scene(self.ctx, blob, len(blob)), "rtw_upload_scene")

    def render(self, params):
        rows = local_rows(params)
        out = np.empty((rows, params.width, 4), dtype=np.float32)
        st = Stats()
        self._check(self.lib.rtw_render(self.ctx, C.byref(params), out.ctypes.data, C.byref(st)), "rtw_render")
        return out, st

    def render_device(self, params, device_ptr, stream_ptr=0):
        st = Stats()
        self._check(self.lib.rtw_render_device(self.ctx, C.byref(params), C.c_void_p(device_ptr),
                                               C.c_void_p(stream_ptr), C.byref(st)), "rtw_render_device")
        return st

    def denoise(self, img, iterations=5, sigma=0.5):
        """rtw_denoise on an (h, w, 4) float32 image; returns the filtered image."""
        src = np.ascontiguousarray(img, dtype=np.float32)
        h, w = src.shape[:2]
        out = np.empty_like(src)
        self._check(self.lib.rtw_denoise(self.ctx, src.ctypes.data, out.ctypes.data, w, h, iterations, sigma), "rtw_denoise")
        return out

    def render_guides(self, params, which=GUIDES, stats=None):
        """rtw_render_guides: first-hit guide buffers of the rows `params` renders, as a dict of the requested names:
        albedo and normal (rows, w, 4) float32 (alpha = fraction of the samples that hit), depth (rows, w) float32,
        prim (rows, w) int32. `stats`: a Stats to fill, or None."""
        out, g = _guide_buffers(_guide_names("render_guides", which), (local_rows(params), params.width))
        self._check(self.lib.rtw_render_guides(self.ctx, C.byref(params), C.byref(g), _ref(stats)), "rtw_render_guides")
        return out

    def denoise_guided(self, img, albedo, normal, iterations=5, sigma=0.5, sigma_albedo=DENOISE_SIGMA_ALBEDO,
                       sigma_normal=DENOISE_SIGMA_NORMAL):
        """rtw_denoise_guided on an (h, w, 4) float32 image with (h, w, 3 or 4) albedo and normal guides; returns the
        filtered image. The colour sigma is rtw_denoise's (display-encoded input in [0, 1]). The default guide sigmas,
        0.4 for the albedo and 0.5 for the normal, are the best of a sweep (scripts/guide_sweep.py: sigma_albedo
        0.05 ... 1, sigma_normal 0.1 ... 1) on 8-spp display-encoded renders of scenes 0 and 2 at 256 x 256 against
        1024-spp references: RMSE 4.5 % (scene 0) and 1.8 % (scene 2) below the colour-only filter's."""
        src = np.ascontiguousarray(img, dtype=np.float32)
        h, w = src.shape[:2]

        def guide(g):
            g = np.asarray(g, dtype=np.float32)
            if g.shape[:2] != (h, w) or g.ndim != 3 or g.shape[2] not in (3, 4):
                raise ValueError(f"denoise_guided: guide of shape {g.shape} for a {h}x{w} image")
            if g.shape[2] == 3:
                g = np.concatenate([g, np.zeros((h, w, 1), np.float32)], axis=2)
            return np.ascontiguousarray(g)
        a, n = guide(albedo), guide(normal)
        out = np.empty_like(src)
        self._check(self.lib.rtw_denoise_guided(self.ctx, src.ctypes.data, a.ctypes.data, n.ctypes.data, out.ctypes.data, w, h,
                                                iterations, sigma, sigma_albedo, sigma_normal), "rtw_denoise_guided")
        return out

    def render_adaptive(self, params, threshold, min_spp=64, step_spp=0, dilate=1):
        """rtw_render_adaptive: params.spp is the cap. Returns (img, spp, err, stats): the (rows, w, 4) float32 image, the
        (rows, w) int32 sample count of every pixel, the (rows, w) float32 error estimate at its last checkpoint and the Stats.
        Pixel p of img is, bit for bit, pixel p of render(params with spp = spp[p])."""
        img, spp, err = _adaptive_outputs((local_rows(params), params.width))
        ad = Adaptive(min_spp, step_spp, threshold, dilate)
        st = Stats()
        self._check(self.lib.rtw_render_adaptive(self.ctx, C.byref(params), C.byref(ad), img.ctypes.data, spp.ctypes.data,
                                                 err.ctypes.data, C.byref(st)), "rtw_render_adaptive")
        return img, spp, err, st

    # ---- accumulation sessions (include/rtw.h rtw_accum_*): begin, add samples as often as you like, read whenever you like
    def accum_begin(self, params, error=False):
        """Start the context's session: params as for render, params.spp = the cap (a multiple of 16). error=True keeps the
        moments, so that accum_read(error=True) works."""
        self._check(self.lib.rtw_accum_begin(self.ctx, C.byref(params), RTW_ACCUM_ERROR if error else 0), "rtw_accum_begin")

    def accum_add(self, spp):
        """Render the next spp samples (a multiple of 16) of every pixel into the session; the Stats of this add alone."""
        st = Stats()
        self._check(self.lib.rtw_accum_add(self.ctx, spp, C.byref(st)), "rtw_accum_add")
        return st

    def accum_read(self, error=False):
        """The frame of the samples added so far: bit for bit render(spp = done). error=True: (img, err), err the (rows, w)
        float32 error map of render_adaptive(spp = min_spp = done)."""
        info = self.accum_status()
        rows, w = local_rows(info.params), info.params.width
        img = np.empty((rows, w, 4), dtype=np.float32)
        err = np.empty((rows, w), dtype=np.float32) if error else None
        self._check(self.lib.rtw_accum_read(self.ctx, img.ctypes.data, err.ctypes.data if error else None), "rtw_accum_read")
        return (img, err) if error else img

    def accum_read_device(self, device_ptr, stream_ptr=0):
        self._check(self.lib.rtw_accum_read_device(self.ctx, C.c_void_p(device_ptr), C.c_void_p(stream_ptr)), "rtw_accum_read_device")

    def accum_status(self):
        info = AccumInfo()
        self._check(self.lib.rtw_accum_status(self.ctx, C.byref(info)), "rtw_accum_status")
        return info

    def accum_save(self):
        """The session as bytes (header + per-pixel state); the session goes on."""
        buf = C.create_string_buffer(self.accum_status().state_bytes)
        self._check(self.lib.rtw_accum_save(self.ctx, buf, len(buf)), "rtw_accum_save")
        return buf.raw

    def accum_restore(self, blob):
        """Start a session from accum_save's bytes: same scene uploaded, no session active. It continues exactly."""
        self._check(self.lib.rtw_accum_restore(self.ctx, bytes(blob), len(blob)), "rtw_accum_restore")

    def accum_end(self):
        self._check(self.lib.rtw_accum_end(self.ctx), "rtw_accum_end")

    # ---- ray queries on the caller's own rays (include/rtw.h rtw_cast / rtw_cast_device)
    @staticmethod
    def cast_outputs(mode, want):
        """The outputs a cast returns: `want` in rtw_hits' order, without the ones the mode does not have."""
        if mode not in CAST_MODES:
            raise ValueError(f"cast: mode {mode!r} is neither 'closest' nor 'any'")
        want = tuple(want)
        bad = [k for k in want if k not in CAST_OUTPUTS]
        if bad or not want:
            raise ValueError(f"cast: unknown or no output names {bad or want}")
        names = [k for k in CAST_OUTPUTS if k in want and (mode == "closest" or k in ("t", "prim"))]
        if not names:
            raise ValueError(f"cast: mode 'any' has t and prim only, not {want}")
        return names

    def cast(self, rays, ray_time=None, gather_time=None, mode="closest", want=("t", "prim", "material", "normal", "uv"), stats=None):
        """rtw_cast on (n, 8) float32 rays (origin, direction, tmin, tmax) with optional (n,) ray and gather times: a dict of the
        requested outputs as numpy arrays - t (n,) float32, prim and material (n,) int32, normal (n, 4) float32 (w = 1 front face),
        uv (n, 2) float32. mode "any" answers occlusion: prim >= 0 where something lies in (tmin, tmax); it has t and prim only (the
        other names of the default `want` are dropped). `stats`: a Stats to fill, or None."""
        names = self.cast_outputs(mode, want)
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        if rays.ndim != 2 or rays.shape[1] != 8:
            raise ValueError(f"cast: rays of shape {rays.shape}, expected (n, 8)")
        n = rays.shape[0]

        def times(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != (n,):
                raise ValueError(f"cast: times of shape {a.shape} for {n} rays")
            return a
        rt, gt = times(ray_time), times(gather_time)
        out = {k: np.empty((n,) + CAST_OUTPUTS[k][1], CAST_OUTPUTS[k][0]) for k in names}
        h = Hits(**{k: v.ctypes.data for k, v in out.items()})
        self._check(self.lib.rtw_cast(self.ctx, rays.ctypes.data, _ptr(rt), _ptr(gt), n, CAST_MODES[mode], C.byref(h), _ref(stats)), "rtw_cast")
        return out

    def cast_device(self, n, rays_ptr, out_ptrs, ray_time_ptr=0, gather_time_ptr=0, mode="closest", stream_ptr=0, stats=None):
        """rtw_cast_device on raw device pointers, as render_device takes them: n rays at rays_ptr (16-byte aligned), out_ptrs a
        dict name -> device pointer of the outputs wanted, stream_ptr a hipStream_t (0: the context's own stream)."""
        h = Hits(**{k: C.c_void_p(v) for k, v in out_ptrs.items()})
        self._check(self.lib.rtw_cast_device(self.ctx, C.c_void_p(rays_ptr), C.c_void_p(ray_time_ptr), C.c_void_p(gather_time_ptr), n,
                                             CAST_MODES[mode], C.byref(h), C.c_void_p(stream_ptr), _ref(stats)), "rtw_cast_device")

    # ---- path-traced radiance along the caller's own rays (include/rtw.h rtw_radiance / rtw_radiance_device)
    def radiance(self, rays, spp, max_depth, seed=0x6314759, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0, key_offset=0, stats=None):
        """rtw_radiance on (n, 8) float32 rays (origin, direction, tmin, tmax: tmin and tmax bound the first segment): the (n, 4)
        float32 mean radiance of spp paths along every ray, alpha 1. Ray i draws from the stream of key_offset + i, samples
        sample_offset ... sample_offset + spp - 1. `stats`: a Stats to fill, or None."""
        rays = _batch("radiance", "rays", rays)
        rp = make_radiance_params(spp, max_depth, seed, rng_kind, sample_offset, estimator, key_offset)
        out = np.empty((rays.shape[0], 4), dtype=np.float32)
        self._check(self.lib.rtw_radiance(self.ctx, rays.ctypes.data, rays.shape[0], C.byref(rp), out.ctypes.data, _ref(stats)), "rtw_radiance")
        return out

    def radiance_device(self, n, rays_ptr, out_ptr, spp, max_depth, seed=0x6314759, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0,
                        key_offset=0, stream_ptr=0, stats=None):
        """rtw_radiance_device on raw device pointers, as cast_device takes them: n rays at rays_ptr, n float4 means written at out_ptr
        (both 16-byte aligned), stream_ptr a hipStream_t (0: the context's own stream)."""
        rp = make_radiance_params(spp, max_depth, seed, rng_kind, sample_offset, estimator, key_offset)
        self._check(self.lib.rtw_radiance_device(self.ctx, C.c_void_p(rays_ptr), n, C.byref(rp), C.c_void_p(out_ptr), C.c_void_p(stream_ptr),
                                                 _ref(stats)), "rtw_radiance_device")

    # ---- irradiance and ambient occlusion at surface points (include/rtw.h rtw_probe / rtw_probe_device)
    def probe(self, probes, spp, max_depth, seed=0x6314759, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0, key_offset=0,
              mode="irradiance", stats=None):
        """rtw_probe on (n, 8) float32 probes (position, normal, tmin, tmax): the (n, 4) float32 result of spp samples per probe, alpha
        1 - mode "irradiance": the irradiance (cosine-weighted paths, mean radiance times pi); mode "occlusion": the fraction of the
        same directions that reach tmax unoccluded, in all three channels. Probe i draws from the stream of key_offset + i, samples
        sample_offset ... sample_offset + spp - 1. `stats`: a Stats to fill, or None."""
        probes = _batch("probe", "probes", probes)
        pp = make_probe_params(spp, max_depth, seed, rng_kind, sample_offset, estimator, key_offset, mode)
        out = np.empty((probes.shape[0], 4), dtype=np.float32)
        self._check(self.lib.rtw_probe(self.ctx, probes.ctypes.data, probes.shape[0], C.byref(pp), out.ctypes.data, _ref(stats)), "rtw_probe")
        return out

    def probe_device(self, n, probes_ptr, out_ptr, spp, max_depth, seed=0x6314759, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0,
                     key_offset=0, mode="irradiance", stream_ptr=0, stats=None):
        """rtw_probe_device on raw device pointers, as radiance_device takes them: n probes at probes_ptr, n float4 results written at
        out_ptr (both 16-byte aligned), stream_ptr a hipStream_t (0: the context's own stream)."""
        pp = make_probe_params(spp, max_depth, seed, rng_kind, sample_offset, estimator, key_offset, mode)
        self._check(self.lib.rtw_probe_device(self.ctx, C.c_void_p(probes_ptr), n, C.byref(pp), C.c_void_p(out_ptr), C.c_void_p(stream_ptr),
                                              _ref(stats)), "rtw_probe_device")

    # ---- probes sampled to a noise target (include/rtw.h rtw_probe_adaptive / rtw_probe_adaptive_device)
    def probe_adaptive(self, probes, cap, max_depth, threshold, min_spp=64, step_spp=0, seed=0x6314759, rng_kind=RTW_RNG_PHILOX, sample_offset=0,
                       estimator=0, key_offset=0, mode="irradiance", stats=None):
        """rtw_probe_adaptive on (n, 8) float32 probes: every probe takes samples until its error estimate is below `threshold`, at
        most `cap`. Returns (out, spp, err): the (n, 4) float32 results, the (n,) int32 sample counts n_i and the (n,) float32 errors
        at each probe's last checkpoint. Row i of out is, bit for bit, row 0 of probe(probes[i:i + 1], spp[i], ..., key_offset + i)."""
        probes = _batch("probe_adaptive", "probes", probes)
        pp = make_probe_params(cap, max_depth, seed, rng_kind, sample_offset, estimator, key_offset, mode)
        ad = Adaptive(min_spp, step_spp, threshold, 0)
        n = probes.shape[0]
        out, spp, err = _adaptive_outputs((n,))
        self._check(self.lib.rtw_probe_adaptive(self.ctx, probes.ctypes.data, n, C.byref(pp), C.byref(ad), out.ctypes.data, spp.ctypes.data,
                                                err.ctypes.data, _ref(stats)), "rtw_probe_adaptive")
        return out, spp, err

    def probe_adaptive_device(self, n, probes_ptr, out_ptr, spp_ptr, err_ptr, cap, max_depth, threshold, min_spp=64, step_spp=0, seed=0x6314759,
                              rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0, key_offset=0, mode="irradiance", stream_ptr=0, stats=None):
        """rtw_probe_adaptive_device on raw device pointers: n probes at probes_ptr, n float4 at out_ptr (both 16-byte aligned), n int32
        at spp_ptr and n float at err_ptr (4-byte aligned; 0: not wanted), stream_ptr a hipStream_t (0: the context's own stream)."""
        pp = make_probe_params(cap, max_depth, seed, rng_kind, sample_offset, estimator, key_offset, mode)
        ad = Adaptive(min_spp, step_spp, threshold, 0)
        self._check(self.lib.rtw_probe_adaptive_device(self.ctx, C.c_void_p(probes_ptr), n, C.byref(pp), C.byref(ad), C.c_void_p(out_ptr),
                                                       C.c_void_p(spp_ptr), C.c_void_p(err_ptr), C.c_void_p(stream_ptr),
                                                       _ref(stats)), "rtw_probe_adaptive_device")

    # ---- spherical-harmonic light probes at free points (include/rtw.h rtw_probe_sh / rtw_probe_sh_device)
    def probe_sh(self, points, spp, max_depth, seed=0x6314759, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0, key_offset=0, stats=None):
        """rtw_probe_sh on (n, 8) float32 points (position, three unused floats, tmin, tmax): the (n, 9, 4) float32 coefficients of the
        radiance arriving at every point on the nine real spherical harmonics of bands 0 to 2, spp samples per point, w = 0
        (bake.sh_irradiance evaluates them for a normal). Point i draws from the stream of key_offset + i, samples sample_offset ...
        sample_offset + spp - 1. `stats`: a Stats to fill, or None."""
        points = _batch("probe_sh", "points", points)
        rp = make_radiance_params(spp, max_depth, seed, rng_kind, sample_offset, estimator, key_offset)
        out = np.empty((points.shape[0], 9, 4), dtype=np.float32)
        self._check(self.lib.rtw_probe_sh(self.ctx, points.ctypes.data, points.shape[0], C.byref(rp), out.ctypes.data, _ref(stats)), "rtw_probe_sh")
        return out

    def probe_sh_device(self, n, points_ptr, out_ptr, spp, max_depth, seed=0x6314759, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0,
                        key_offset=0, stream_ptr=0, stats=None):
        """rtw_probe_sh_device on raw device pointers, as radiance_device takes them: n points at points_ptr, n * 9 float4 coefficients
        written at out_ptr (both 16-byte aligned), stream_ptr a hipStream_t (0: the context's own stream)."""
        rp = make_radiance_params(spp, max_depth, seed, rng_kind, sample_offset, estimator, key_offset)
        self._check(self.lib.rtw_probe_sh_device(self.ctx, C.c_void_p(points_ptr), n, C.byref(rp), C.c_void_p(out_ptr), C.c_void_p(stream_ptr),
                                                 _ref(stats)), "rtw_probe_sh_device")

    # ---- batched frames from the caller's own cameras (include/rtw.h rtw_views / rtw_views_device)
    def views(self, views, width, height, spp, max_depth, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0, stats=None):
        """rtw_views on View records (make_view, scene_view, bake.cube_views, bake.orbit_views): the (n, height, width, 4) float32
        frames, row 0 the bottom row, alpha 1. Frame v is render()'s frame of the uploaded scene with views[v]'s camera in its
        header and views[v].seed as the seed. `stats`: a Stats to fill, or None."""
        arr, vp = _view_batch("views", views, width, height, spp, max_depth, rng_kind, sample_offset, estimator)
        out = np.empty((len(arr), int(height), int(width), 4), dtype=np.float32)
        self._check(self.lib.rtw_views(self.ctx, C.cast(arr, C.c_void_p), len(arr), C.byref(vp), out.ctypes.data, _ref(stats)), "rtw_views")
        return out

    def views_device(self, n, views_ptr, out_ptr, width, height, spp, max_depth, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0,
                     stream_ptr=0, stats=None):
        """rtw_views_device on raw device pointers, as radiance_device takes them: n rtw_view records (112 B each) at views_ptr,
        n * height * width float4 written at out_ptr (both 16-byte aligned), stream_ptr a hipStream_t (0: the context's own stream)."""
        vp = make_view_params(width, height, spp, max_depth, rng_kind, sample_offset, estimator)
        self._check(self.lib.rtw_views_device(self.ctx, C.c_void_p(views_ptr), n, C.byref(vp), C.c_void_p(out_ptr), C.c_void_p(stream_ptr),
                                              _ref(stats)), "rtw_views_device")

    # ---- batched views sampled to a noise target (include/rtw.h rtw_views_adaptive / rtw_views_adaptive_device)
    def views_adaptive(self, views, width, height, cap, max_depth, threshold, min_spp=64, step_spp=0, dilate=1, rng_kind=RTW_RNG_PHILOX,
                       sample_offset=0, estimator=0, stats=None):
        """rtw_views_adaptive on View records: every pixel of every view takes samples until its error estimate is below `threshold`,
        at most `cap`. Returns (frames, spp, err): the (n, height, width, 4) float32 frames, the (n, height, width) int32 sample counts
        and the (n, height, width) float32 errors at each pixel's last checkpoint. View v's three arrays are, bit for bit,
        render_adaptive's of the uploaded scene with views[v]'s camera in its header and views[v].seed as the seed; with dilate = 1
        the 3x3 neighbourhood stays inside the pixel's own view. `stats`: a Stats to fill, or None."""
        arr, vp = _view_batch("views_adaptive", views, width, height, cap, max_depth, rng_kind, sample_offset, estimator)
        ad = Adaptive(min_spp, step_spp, threshold, dilate)
        out, spp, err = _adaptive_outputs((len(arr), int(height), int(width)))
        self._check(self.lib.rtw_views_adaptive(self.ctx, C.cast(arr, C.c_void_p), len(arr), C.byref(vp), C.byref(ad), out.ctypes.data,
                                                spp.ctypes.data, err.ctypes.data, _ref(stats)), "rtw_views_adaptive")
        return out, spp, err

    def views_adaptive_device(self, n, views_ptr, out_ptr, spp_ptr, err_ptr, width, height, cap, max_depth, threshold, min_spp=64, step_spp=0,
                              dilate=1, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0, stream_ptr=0, stats=None):
        """rtw_views_adaptive_device on raw device pointers: n rtw_view records at views_ptr, n * height * width float4 at out_ptr (both
        16-byte aligned), as many int32 at spp_ptr and float at err_ptr (4-byte aligned; 0: not wanted), stream_ptr a hipStream_t
        (0: the context's own stream)."""
        vp = make_view_params(width, height, cap, max_depth, rng_kind, sample_offset, estimator)
        ad = Adaptive(min_spp, step_spp, threshold, dilate)
        self._check(self.lib.rtw_views_adaptive_device(self.ctx, C.c_void_p(views_ptr), n, C.byref(vp), C.byref(ad), C.c_void_p(out_ptr),
                                                       C.c_void_p(spp_ptr), C.c_void_p(err_ptr), C.c_void_p(stream_ptr),
                                                       _ref(stats)), "rtw_views_adaptive_device")

    # ---- replayed samples and the vertices of their paths (include/rtw.h rtw_paths / rtw_paths_views and their _device variants)
    def paths(self, rays, spp, max_depth, max_records=None, seed=0x6314759, rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0, key_offset=0,
              stats=None):
        """rtw_paths on (n, 8) float32 rays: (heads, vertices), structured arrays of dtype PATH_HEAD, shape (n, spp), and PATH_VERTEX,
        shape (n, spp, max_records). Sample s of ray i is radiance()'s sample of that ray at key key_offset + i and sample index
        sample_offset + s; heads["radiance"][i, s] carries the bits radiance(spp=1, sample_offset=sample_offset + s) returns.
        vertices[i, s, j] is segment j of that path, written for j < min(heads["segments"][i, s], max_records); the rest stays zero.
        max_records None keeps every vertex (max_depth of them), 0 returns the heads alone. `stats`: a Stats to fill, or None."""
        rays = _batch("paths", "rays", rays)
        pp = make_paths_params(spp, max_depth, max_records, seed, rng_kind, sample_offset, estimator, key_offset)
        n = rays.shape[0]
        _check_pairs("paths", n, spp)
        heads, vertices = _path_buffers(n, spp, pp.max_records)
        self._check(self.lib.rtw_paths(self.ctx, rays.ctypes.data, n, C.byref(pp), heads.ctypes.data, vertices.ctypes.data if pp.max_records else None,
                                       _ref(stats)), "rtw_paths")
        return heads, vertices

    def paths_device(self, n, rays_ptr, heads_ptr, vertices_ptr, spp, max_depth, max_records=None, seed=0x6314759, rng_kind=RTW_RNG_PHILOX,
                     sample_offset=0, estimator=0, key_offset=0, stream_ptr=0, stats=None):
        """rtw_paths_device on raw device pointers, as radiance_device takes them: n rays at rays_ptr, n * spp heads (32 B) written at
        heads_ptr and up to max_records vertices (64 B) per sample at vertices_ptr (0 with max_records = 0), all 16-byte aligned,
        stream_ptr a hipStream_t (0: the context's own stream)."""
        pp = make_paths_params(spp, max_depth, max_records, seed, rng_kind, sample_offset, estimator, key_offset)
        self._check(self.lib.rtw_paths_device(self.ctx, C.c_void_p(rays_ptr), n, C.byref(pp), C.c_void_p(heads_ptr), C.c_void_p(vertices_ptr),
                                              C.c_void_p(stream_ptr), _ref(stats)), "rtw_paths_device")

    def paths_views(self, views, width, height, first, count, spp, max_depth, max_records=None, rng_kind=RTW_RNG_PHILOX, sample_offset=0,
                    estimator=0, stats=None):
        """rtw_paths_views on View records: paths()'s two arrays, shapes (count, spp) and (count, spp, max_records), for pixels
        [first, first + count) of views()'s flattened (view, y, x) index: the samples views() averages, one by one. Pixel (x, y) of
        view v is first = (v * height + y) * width + x. `stats`: a Stats to fill, or None."""
        arr, vp = _view_batch("paths_views", views, width, height, spp, max_depth, rng_kind, sample_offset, estimator)
        first = _path_window("paths_views", first, count, len(arr) * int(width) * int(height))
        count, k = int(count), _max_records("paths_views", max_records, max_depth)
        _check_pairs("paths_views", count, spp)
        heads, vertices = _path_buffers(count, spp, k)
        self._check(self.lib.rtw_paths_views(self.ctx, C.cast(arr, C.c_void_p), len(arr), C.byref(vp), first, count, k, heads.ctypes.data,
                                             vertices.ctypes.data if k else None, _ref(stats)), "rtw_paths_views")
        return heads, vertices

    def paths_views_device(self, n, views_ptr, heads_ptr, vertices_ptr, width, height, first, count, spp, max_depth, max_records=None,
                           rng_kind=RTW_RNG_PHILOX, sample_offset=0, estimator=0, stream_ptr=0, stats=None):
        """rtw_paths_views_device on raw device pointers: n rtw_view records at views_ptr, count * spp heads at heads_ptr and up to
        max_records vertices per sample at vertices_ptr (0 with max_records = 0), all 16-byte aligned, stream_ptr a hipStream_t (0:
        the context's own stream)."""
        vp = make_view_params(width, height, spp, max_depth, rng_kind, sample_offset, estimator)
        k = _max_records("paths_views", max_records, max_depth)
        self._check(self.lib.rtw_paths_views_device(self.ctx, C.c_void_p(views_ptr), n, C.byref(vp), int(first), int(count), k, C.c_void_p(heads_ptr),
                                                    C.c_void_p(vertices_ptr), C.c_void_p(stream_ptr), _ref(stats)), "rtw_paths_views_device")

    # ---- guides of batched views and their denoiser (include/rtw.h rtw_views_guides / rtw_denoise_views)
    def views_guides(self, views, width, height, spp=16, which=GUIDES, rng_kind=RTW_RNG_PHILOX, sample_offset=0, stats=None):
        """rtw_views_guides on View records: the dict render_guides returns with a leading view axis - albedo and normal
        (n, height, width, 4) float32 (alpha = fraction of the samples that hit), depth (n, height, width) float32, prim
        (n, height, width) int32 - of the requested names. View v's guides are render_guides' of the uploaded scene with views[v]'s
        camera in its header and views[v].seed as the seed. `stats`: a Stats to fill, or None."""
        which = _guide_names("views_guides", which)
        arr, vp = _view_batch("views_guides", views, width, height, spp, 0, rng_kind, sample_offset, 0)  # no paths: no depth, no estimator
        out, g = _guide_buffers(which, (len(arr), int(height), int(width)))
        self._check(self.lib.rtw_views_guides(self.ctx, C.cast(arr, C.c_void_p), len(arr), C.byref(vp), C.byref(g), _ref(stats)), "rtw_views_guides")
        return out

    def views_guides_device(self, n, views_ptr, out_ptrs, width, height, spp=16, rng_kind=RTW_RNG_PHILOX, sample_offset=0, stream_ptr=0,
                            stats=None):
        """rtw_views_guides_device on raw device pointers: n rtw_view records at views_ptr (16-byte aligned), out_ptrs a dict of
        guide name -> device pointer (albedo, normal: n * height * width float4, 16-byte aligned; depth, prim: as many 4-byte
        entries), stream_ptr a hipStream_t (0: the context's own stream)."""
        bad = [k for k in out_ptrs if k not in GUIDES]
        if bad:
            raise ValueError(f"views_guides_device: unknown guide names {bad}")
        vp = make_view_params(width, height, spp, 0, rng_kind, sample_offset, 0)
        g = Guides(**{k: int(v) for k, v in out_ptrs.items()})
        self._check(self.lib.rtw_views_guides_device(self.ctx, C.c_void_p(views_ptr), n, C.byref(vp), C.byref(g), C.c_void_p(stream_ptr),
                                                     _ref(stats)), "rtw_views_guides_device")

    def denoise_views(self, frames, albedo, normal, iterations=5, sigma=0.5, sigma_albedo=DENOISE_SIGMA_ALBEDO,
                      sigma_normal=DENOISE_SIGMA_NORMAL):
        """rtw_denoise_views on (n, h, w, 4) float32 frames with (n, h, w, 4) albedo and normal guides (views_guides'); returns the
        filtered frames: frame v is denoise_guided of frame v alone. Sigmas as denoise_guided's."""
        src = np.ascontiguousarray(frames, dtype=np.float32)
        if src.ndim != 4 or src.shape[3] != 4:
            raise ValueError(f"denoise_views: frames of shape {src.shape}, expected (n, h, w, 4)")

        def guide(g):
            g = np.ascontiguousarray(g, dtype=np.float32)
            if g.shape != src.shape:
                raise ValueError(f"denoise_views: guide of shape {g.shape} for frames of shape {src.shape}")
            return g
        a, nm = guide(albedo), guide(normal)
        n, h, w = src.shape[:3]
        out = np.empty_like(src)
        self._check(self.lib.rtw_denoise_views(self.ctx, src.ctypes.data, a.ctypes.data, nm.ctypes.data, out.ctypes.data, n, w, h,
                                               iterations, sigma, sigma_albedo, sigma_normal), "rtw_denoise_views")
        return out

    def denoise_views_device(self, n, in_ptr, albedo_ptr, normal_ptr, out_ptr, width, height, iterations=5, sigma=0.5,
                             sigma_albedo=DENOISE_SIGMA_ALBEDO, sigma_normal=DENOISE_SIGMA_NORMAL, stream_ptr=0):
        """rtw_denoise_views_device on raw device pointers (n * height * width float4 each, 16-byte aligned), stream_ptr a
        hipStream_t (0: the context's own stream)."""
        self._check(self.lib.rtw_denoise_views_device(self.ctx, C.c_void_p(in_ptr), C.c_void_p(albedo_ptr), C.c_void_p(normal_ptr),
                                                      C.c_void_p(out_ptr), n, width, height, iterations, sigma, sigma_albedo, sigma_normal,
                                                      C.c_void_p(stream_ptr)), "rtw_denoise_views_device")

    def debug_intersect(self, rays, ray_time=None, gather_time=None):
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        n = rays.shape[0]
        rt = None if ray_time is None else np.ascontiguousarray(ray_time, dtype=np.float32)
        gt = None if gather_time is None else np.ascontiguousarray(gather_time, dtype=np.float32)
        t = np.empty(n, dtype=np.float32)
        prim = np.empty(n, dtype=np.int32)
        self._check(self.lib.rtw_debug_intersect(self.ctx, rays.ctypes.data, _ptr(rt), _ptr(gt), n, t.ctypes.data, prim.ctypes.data),
                    "rtw_debug_intersect")
        return t, prim

    def debug_math(self, op):
        """All 2^32 bit patterns through a short form of csrc/rtw_math.h and the compiler's form (include/rtw.h rtw_debug_math):
        (differing patterns, patterns inside the range window, lowest differing pattern or None)."""
        out = (C.c_uint64 * 3)()
        self._check(self.lib.rtw_debug_math(self.ctx, MATH_OPS[op], out), "rtw_debug_math")
        return int(out[0]), int(out[1]), (None if out[2] == 2 ** 64 - 1 else int(out[2]))

    def close(self):
        if self.ctx:
            self.lib.rtw_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
