"""Shared by the guide tests (test_guides_cpu.py, test_gpu_guides.py) and scripts/guide_sweep.py: a float32 numpy restatement of
rtw_denoise_guided with its operation order written out, and the synthetic scenes the guide identities are checked on."""
import numpy as np

from raytracing_weekend_amd import abi

F32 = np.float32


def atrous_guided(img, albedo, normal, iterations=5, sigma=0.5, sigma_albedo=abi.DENOISE_SIGMA_ALBEDO,
                  sigma_normal=abi.DENOISE_SIGMA_NORMAL):
    """rtw_denoise_guided (rtw_guides.hip k_atrous_guided), tap for tap in float32."""
    cur = np.ascontiguousarray(img, dtype=F32).copy()
    alb = np.asarray(albedo, dtype=F32)
    nrm = np.asarray(normal, dtype=F32)
    h, w = cur.shape[:2]
    kern = [F32(1.0) / F32(16.0), F32(1.0) / F32(4.0), F32(3.0) / F32(8.0), F32(1.0) / F32(4.0), F32(1.0) / F32(16.0)]
    inv_a = F32(1.0) / (F32(sigma_albedo) * F32(sigma_albedo))
    inv_n = F32(1.0) / (F32(sigma_normal) * F32(sigma_normal))
    ys, xs = np.mgrid[0:h, 0:w]
    s_i = F32(sigma)
    one = F32(1.0)
    for it in range(iterations):
        step = 1 << it
        inv = one / (s_i * s_i)
        c, ca, cn = cur, alb, nrm
        sr, sg, sb, sw = (np.zeros((h, w), F32) for _ in range(4))
        for dy in range(-2, 3):
            yy = np.clip(ys + dy * step, 0, h - 1)
            for dx in range(-2, 3):
                xx = np.clip(xs + dx * step, 0, w - 1)
                q, qa, qn = c[yy, xx], ca[yy, xx], cn[yy, xx]
                dr, dg, db = c[..., 0] - q[..., 0], c[..., 1] - q[..., 1], c[..., 2] - q[..., 2]
                d2 = (dr * dr + dg * dg) + db * db
                ar, ag, ab = ca[..., 0] - qa[..., 0], ca[..., 1] - qa[..., 1], ca[..., 2] - qa[..., 2]
                a2 = (ar * ar + ag * ag) + ab * ab
                nx, ny, nz = cn[..., 0] - qn[..., 0], cn[..., 1] - qn[..., 1], cn[..., 2] - qn[..., 2]
                n2 = (nx * nx + ny * ny) + nz * nz
                wt = (kern[dy + 2] * kern[dx + 2]) / (one + d2 * inv)
                wt = wt / (one + a2 * inv_a)
                wt = wt / (one + n2 * inv_n)
                sr = sr + wt * q[..., 0]
                sg = sg + wt * q[..., 1]
                sb = sb + wt * q[..., 2]
                sw = sw + wt
        cur = np.stack([sr / sw, sg / sw, sb / sw, c[..., 3]], axis=-1).astype(F32)
        s_i = s_i * F32(0.5)
    return cur


def encode(img):
    """Display encoding the Director feeds the denoiser: sqrt of the colour clamped to [0, 1] (NaN -> 0), alpha kept."""
    out = np.array(img, dtype=F32, copy=True)
    c = np.nan_to_num(out[..., :3], nan=0.0)
    out[..., :3] = np.sqrt(np.clip(c, 0.0, 1.0))
    return out


def with_camera(blob, scene_code, w, h, lens_radius=0.0):
    """blob with the camera (and camera kind) of build_scene(scene_code) - 0 perspective, 100 environment, 200 orthographic
    views of the Cornell box - and the given lens radius."""
    parts = dict(abi.parse_scene(blob))
    cam = abi.parse_scene(abi.build_scene(scene_code, w, h))["header"]
    hdr = abi.SceneHeader.from_buffer_copy(bytes(parts["header"]))
    hdr.camera = cam.camera
    hdr.camera_type = cam.camera_type
    hdr.camera.lens_radius = lens_radius
    parts["header"] = hdr
    return abi.assemble_scene(parts)


def all_emitters(blob, colours=None):
    """Every primitive of blob made a diffuse light. colours=None: the lights show the scene's textures that lie in [0, 1]
    (constants, checker, noise, image), cycling over primitives; colours = list of rgb: primitive i shows constant colours[i].
    No light list, sky off."""
    parts = dict(abi.parse_scene(blob))
    hdr = abi.SceneHeader.from_buffer_copy(bytes(parts["header"]))
    hdr.sky_light = 0
    textures = list(parts["textures"])
    prims = list(parts["prims"])
    materials = []
    if colours is None:
        ok = [i for i, t in enumerate(textures) if t.type != abi.TEX_CONSTANT or max(t.color) <= 1.0]
        for i in ok:
            materials.append(abi.Material(type=abi.MAT_DIFFUSE_LIGHT, texture=i, fuzz_or_eta=0.0, bsdf_eval=-1))
        for k, pr in enumerate(prims):
            pr.material = k % len(materials)
    else:
        for k, pr in enumerate(prims):
            t = abi.Texture(type=abi.TEX_CONSTANT)
            t.color[0], t.color[1], t.color[2] = (float(v) for v in colours[k])
            textures.append(t)
            materials.append(abi.Material(type=abi.MAT_DIFFUSE_LIGHT, texture=len(textures) - 1, fuzz_or_eta=0.0, bsdf_eval=-1))
            pr.material = k
    parts.update(header=hdr, prims=prims, materials=materials, textures=textures, lights=[])
    return abi.assemble_scene(parts)


def contract_mean(frames):
    """Mean of per-sample frames (frames[s] = sample s) in rtw.h's summation order: blocks of 16, units of 8 blocks."""
    a = np.zeros_like(frames[0])
    u = np.zeros_like(frames[0])
    b = np.zeros_like(frames[0])
    for s, f in enumerate(frames):
        if s and s % 16 == 0:
            u = u + b
            b = np.zeros_like(b)
            if s % 128 == 0:
                a = a + u
                u = np.zeros_like(u)
        b = b + f
    u = u + b
    a = a + u
    return a / F32(len(frames))
