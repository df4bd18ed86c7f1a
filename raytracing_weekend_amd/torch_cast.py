"""rtw_cast_device on torch tensors: rays in, hits out, everything stays on the device (include/rtw.h rtw_cast_device)."""
from . import _torch_call as T, abi

def cast_torch(renderer, rays, ray_time=None, gather_time=None, mode="closest", want=("t", "prim", "material", "normal", "uv"), stats=None):
    """Closest-hit (mode "closest") or occlusion (mode "any") queries of an abi.Renderer on an (n, 8) float32 CUDA tensor of rays
    (origin, direction, tmin, tmax), with optional (n,) ray and gather times. The tensors must be contiguous and live on the
    renderer's device. Returns a dict of torch tensors on that device - t (n,), prim and material (n,) int32, normal (n, 4), uv (n, 2) -
    allocated here, written on torch's current stream; the call returns when they are written. No host copy is made.
    torch's default stream has the null handle, which rtw_cast_device reads as "the context's own stream" - a stream that does not
    wait for the default stream's pending work - so under the default stream that work is waited for here, before the call."""
    import torch

    names = renderer.cast_outputs(mode, want)
    if rays.dim() != 2 or rays.shape[1] != 8:
        raise ValueError(f"cast_torch: rays of shape {tuple(rays.shape)}, expected (n, 8)")
    n = rays.shape[0]
    T.check_device("cast_torch", "rays", rays, renderer)
    for name, a in (("rays", rays), ("ray_time", ray_time), ("gather_time", gather_time)):
        if a is None:
            continue
        if not a.is_cuda or a.dtype != torch.float32 or not a.is_contiguous() or a.device != rays.device:
            raise ValueError(f"cast_torch: {name} must be a contiguous float32 CUDA tensor on the rays' device")
        if name != "rays" and tuple(a.shape) != (n,):
            raise ValueError(f"cast_torch: {name} of shape {tuple(a.shape)} for {n} rays")
    return T.run(rays, n, lambda: {k: T.empty(rays, (n,) + abi.CAST_OUTPUTS[k][1], abi.CAST_OUTPUTS[k][0].__name__) for k in names},
                 lambda out, stream: renderer.cast_device(n, rays.data_ptr(), {k: v.data_ptr() for k, v in out.items()},
                                                          0 if ray_time is None else ray_time.data_ptr(),
                                                          0 if gather_time is None else gather_time.data_ptr(),
                                                          mode=mode, stream_ptr=stream, stats=stats))
