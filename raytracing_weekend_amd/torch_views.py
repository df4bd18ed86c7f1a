"""rtw_views_device on torch tensors: cameras in, frames out, everything stays on the device (include/rtw.h rtw_views_device); the
views' guides and denoiser, and the views sampled to a noise target (rtw_views_adaptive_device), likewise."""
import ctypes as C

import numpy as np

from . import _torch_call as T, abi


def views_tensor(views, device):
    """The (n, 28) float32 tensor of abi.View records (112 B each, bit for bit) on `device`: what views_torch takes."""
    import torch

    arr = abi.view_array(views)
    host = np.frombuffer(bytes(arr), dtype=np.float32).reshape(len(arr), C.sizeof(abi.View) // 4).copy()
    return torch.from_numpy(host).to(device)


def views_torch(renderer, views, width, height, spp, max_depth, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, estimator=0, stats=None):
    """Frames of an abi.Renderer from an (n, 28) float32 CUDA tensor of rtw_view records (views_tensor; the integer fields keep their
    bits): the (n, height, width, 4) float32 tensor of the frames (row 0 the bottom row, alpha 1) on the records' device, allocated
    here, written on torch's current stream; the call returns when it is written. The tensor must be contiguous and live on the
    renderer's device. No host copy is made, and the records are not read back: a camera type other than environment or
    orthographic is a perspective camera. torch's default stream has the null handle, which rtw_views_device reads as "the
    context's own stream" - a stream that does not wait for the default stream's pending work - so under the default stream that
    work is waited for here, before the call."""
    lead = _check_views("views_torch", renderer, views, width, height, spp, max_depth)
    return T.run(views, lead[0], lambda: T.empty(views, lead + (4,)),
                 lambda out, stream: renderer.views_device(lead[0], views.data_ptr(), out.data_ptr(), width, height, spp, max_depth, rng_kind=rng_kind,
                                                           sample_offset=sample_offset, estimator=estimator, stream_ptr=stream, stats=stats))


def _check_views(what, renderer, views, width, height, spp, max_depth=0):
    """The checks of a tensor of view records and of the sizes; the (n, height, width) its outputs lead with."""
    n = T.check_tensor(what, "views", views, (C.sizeof(abi.View) // 4,), renderer)
    abi.make_view_params(width, height, spp, max_depth)  # (the sizes are checked even when there is nothing to render)
    abi._check_pixels(what, n, width, height)
    return n, int(height), int(width)


def views_guides_torch(renderer, views, width, height, spp=16, which=abi.GUIDES, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, stats=None):
    """Guides of an abi.Renderer from an (n, 28) float32 CUDA tensor of rtw_view records (views_tensor), in views_torch's shape: the
    dict of the requested names - albedo and normal (n, height, width, 4) float32, depth (n, height, width) float32, prim
    (n, height, width) int32 - on the records' device, allocated here, written on torch's current stream; the call returns when
    they are written. Under torch's default stream (the null handle, which the library reads as "the context's own stream") the
    stream's pending work is waited for here, before the call."""
    which = abi._guide_names("views_guides_torch", which)
    lead = _check_views("views_guides_torch", renderer, views, width, height, spp)
    return T.run(views, lead[0], lambda: {k: T.empty(views, lead + abi.GUIDE_LAYOUT[k][0], abi.GUIDE_LAYOUT[k][1]) for k in which},
                 lambda out, stream: renderer.views_guides_device(lead[0], views.data_ptr(), {k: v.data_ptr() for k, v in out.items()}, width, height,
                                                                  spp, rng_kind=rng_kind, sample_offset=sample_offset, stream_ptr=stream,
                                                                  stats=stats))


def views_adaptive_torch(renderer, views, width, height, cap, max_depth, threshold, min_spp=64, step_spp=0, dilate=1,
                         rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, estimator=0, stats=None):
    """rtw_views_adaptive_device on an (n, 28) float32 CUDA tensor of rtw_view records (views_tensor): (frames, spp, err), the
    (n, height, width, 4) float32 frames, the (n, height, width) int32 sample counts and the (n, height, width) float32 errors, on
    the records' device, allocated here, written on torch's current stream; the call returns when they are written. Every pixel
    takes samples until its error estimate is below `threshold`, at most `cap`. The default stream is waited for as in views_torch."""
    lead = _check_views("views_adaptive_torch", renderer, views, width, height, cap)
    return T.run(views, lead[0], lambda: T.empty_adaptive(views, lead),
                 lambda out, stream: renderer.views_adaptive_device(lead[0], views.data_ptr(), *(t.data_ptr() for t in out), width, height, cap,
                                                                    max_depth, threshold, min_spp=min_spp, step_spp=step_spp, dilate=dilate,
                                                                    rng_kind=rng_kind, sample_offset=sample_offset, estimator=estimator,
                                                                    stream_ptr=stream, stats=stats))


def denoise_views_torch(renderer, frames, albedo, normal, iterations=5, sigma=0.5, sigma_albedo=abi.DENOISE_SIGMA_ALBEDO,
                        sigma_normal=abi.DENOISE_SIGMA_NORMAL):
    """rtw_denoise_views_device on (n, height, width, 4) float32 CUDA tensors (frames, and the albedo and normal of
    views_guides_torch): the filtered frames, allocated here, written on torch's current stream; the call returns when they are
    written. Frame v is denoise_guided of frame v alone. The default stream is waited for as in views_torch."""
    if frames.dim() != 4 or frames.shape[3] != 4:
        raise ValueError(f"denoise_views_torch: frames of shape {tuple(frames.shape)}, expected (n, height, width, 4)")
    for name, t in (("frames", frames), ("albedo", albedo), ("normal", normal)):
        if tuple(t.shape) != tuple(frames.shape):
            raise ValueError(f"denoise_views_torch: {name} of shape {tuple(t.shape)} for frames of shape {tuple(frames.shape)}")
        T.check_tensor("denoise_views_torch", name, t, None, renderer)
    n, h, w = (int(v) for v in frames.shape[:3])
    return T.run(frames, n and h and w, lambda: T.empty(frames, frames.shape),
                 lambda out, stream: renderer.denoise_views_device(n, frames.data_ptr(), albedo.data_ptr(), normal.data_ptr(), out.data_ptr(), w, h,
                                                                   iterations, sigma, sigma_albedo, sigma_normal, stream_ptr=stream))
