"""rtw_views_device on torch tensors: cameras in, frames out, everything stays on the device (include/rtw.h rtw_views_device)."""
import ctypes as C

import numpy as np

from . import abi


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
    import torch

    if views.dim() != 2 or views.shape[1] != C.sizeof(abi.View) // 4:
        raise ValueError(f"views_torch: views of shape {tuple(views.shape)}, expected (n, {C.sizeof(abi.View) // 4})")
    n = views.shape[0]
    if not views.is_cuda or views.device.index != renderer.devices[0]:
        raise ValueError(f"views_torch: views on {views.device}, the renderer answers on cuda:{renderer.devices[0]}")
    if views.dtype != torch.float32 or not views.is_contiguous():
        raise ValueError("views_torch: views must be a contiguous float32 CUDA tensor")
    abi.make_view_params(width, height, spp, max_depth)  # (the sizes are checked even when there is nothing to render)
    if n * int(width) * int(height) > 0x7fffffff:
        raise ValueError("views_torch: more than 2^31 - 1 pixels in one call")
    with torch.cuda.device(views.device):
        out = torch.empty((n, int(height), int(width), 4), dtype=torch.float32, device=views.device)
        stream = torch.cuda.current_stream()
        if n and stream.cuda_stream == 0:
            stream.synchronize()
        if n:
            renderer.views_device(n, views.data_ptr(), out.data_ptr(), width, height, spp, max_depth, rng_kind=rng_kind,
                                  sample_offset=sample_offset, estimator=estimator, stream_ptr=stream.cuda_stream, stats=stats)
    return out
