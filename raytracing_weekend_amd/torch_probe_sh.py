"""rtw_probe_sh_device on torch tensors: points in, spherical-harmonic coefficients out, everything stays on the device
(include/rtw.h rtw_probe_sh_device)."""
from . import _torch_call as T, abi


def probe_sh_torch(renderer, points, spp, max_depth, seed=0x6314759, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, estimator=0, key_offset=0,
                   stats=None):
    """The light probes of an abi.Renderer at an (n, 8) float32 CUDA tensor of points (position, three unused floats, tmin, tmax): the
    (n, 9, 4) float32 tensor of coefficients on the nine real spherical harmonics of bands 0 to 2 (w = 0), spp samples per point, on
    the points' device, allocated here, written on torch's current stream; the call returns when it is written. The tensor must be
    contiguous and live on the renderer's device. No host copy is made. torch's default stream has the null handle, which
    rtw_probe_sh_device reads as "the context's own stream" - a stream that does not wait for the default stream's pending work - so
    under the default stream that work is waited for here, before the call."""
    n = T.check_tensor("probe_sh_torch", "points", points, (8,), renderer)
    abi.make_radiance_params(spp, max_depth)  # (spp is checked even when there is nothing to trace)
    return T.run(points, n, lambda: T.empty(points, (n, 9, 4)),
                 lambda out, stream: renderer.probe_sh_device(n, points.data_ptr(), out.data_ptr(), spp, max_depth, seed=seed, rng_kind=rng_kind,
                                                              sample_offset=sample_offset, estimator=estimator, key_offset=key_offset,
                                                              stream_ptr=stream, stats=stats))
