"""rtw_radiance_device on torch tensors: rays in, mean radiance out, everything stays on the device (include/rtw.h rtw_radiance_device)."""
from . import _torch_call as T, abi


def radiance_torch(renderer, rays, spp, max_depth, seed=0x6314759, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, estimator=0, key_offset=0,
                   stats=None):
    """Path-traced radiance of an abi.Renderer along an (n, 8) float32 CUDA tensor of rays (origin, direction, tmin, tmax): the
    (n, 4) float32 tensor of the mean of spp paths per ray (alpha 1) on the rays' device, allocated here, written on torch's current
    stream; the call returns when it is written. The tensor must be contiguous and live on the renderer's device. No host copy is
    made. torch's default stream has the null handle, which rtw_radiance_device reads as "the context's own stream" - a stream that
    does not wait for the default stream's pending work - so under the default stream that work is waited for here, before the call."""
    n = T.check_tensor("radiance_torch", "rays", rays, (8,), renderer)
    abi.make_radiance_params(spp, max_depth)  # (spp is checked even when there is nothing to trace)
    return T.run(rays, n, lambda: T.empty(rays, (n, 4)),
                 lambda out, stream: renderer.radiance_device(n, rays.data_ptr(), out.data_ptr(), spp, max_depth, seed=seed, rng_kind=rng_kind,
                                                              sample_offset=sample_offset, estimator=estimator, key_offset=key_offset,
                                                              stream_ptr=stream, stats=stats))
