"""rtw_probe_device and rtw_probe_adaptive_device on torch tensors: probes in, irradiance or ambient occlusion out, everything stays on
the device (include/rtw.h rtw_probe_device, rtw_probe_adaptive_device)."""
from . import _torch_call as T, abi


def probe_torch(renderer, probes, spp, max_depth, seed=0x6314759, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, estimator=0, key_offset=0,
                mode="irradiance", stats=None):
    """Irradiance (mode "irradiance") or unoccluded fraction (mode "occlusion") of an abi.Renderer at an (n, 8) float32 CUDA tensor of
    probes (position, normal, tmin, tmax): the (n, 4) float32 tensor of spp samples per probe (alpha 1) on the probes' device,
    allocated here, written on torch's current stream; the call returns when it is written. The tensor must be contiguous and live on
    the renderer's device. No host copy is made. torch's default stream has the null handle, which rtw_probe_device reads as "the
    context's own stream" - a stream that does not wait for the default stream's pending work - so under the default stream that
    work is waited for here, before the call."""
    n = T.check_tensor("probe_torch", "probes", probes, (8,), renderer)
    abi.make_probe_params(spp, max_depth, mode=mode)  # (spp and mode are checked even when there is nothing to trace)
    return T.run(probes, n, lambda: T.empty(probes, (n, 4)),
                 lambda out, stream: renderer.probe_device(n, probes.data_ptr(), out.data_ptr(), spp, max_depth, seed=seed, rng_kind=rng_kind,
                                                           sample_offset=sample_offset, estimator=estimator, key_offset=key_offset, mode=mode,
                                                           stream_ptr=stream, stats=stats))


def probe_adaptive_torch(renderer, probes, cap, max_depth, threshold, min_spp=64, step_spp=0, seed=0x6314759, rng_kind=abi.RTW_RNG_PHILOX,
                         sample_offset=0, estimator=0, key_offset=0, mode="irradiance", stats=None):
    """probe_torch sampled to a noise target (rtw_probe_adaptive_device): three tensors on the probes' device, allocated here - the
    (n, 4) float32 results, the (n,) int32 sample counts and the (n,) float32 errors at each probe's last checkpoint - written on
    torch's current stream under probe_torch's stream rule; the call returns when they are written."""
    n = T.check_tensor("probe_adaptive_torch", "probes", probes, (8,), renderer)
    abi.make_probe_params(cap, max_depth, mode=mode)  # (the cap and the mode are checked even when there is nothing to trace)
    return T.run(probes, n, lambda: T.empty_adaptive(probes, (n,)),
                 lambda out, stream: renderer.probe_adaptive_device(n, probes.data_ptr(), *(t.data_ptr() for t in out), cap, max_depth, threshold,
                                                                    min_spp=min_spp, step_spp=step_spp, seed=seed, rng_kind=rng_kind,
                                                                    sample_offset=sample_offset, estimator=estimator, key_offset=key_offset,
                                                                    mode=mode, stream_ptr=stream, stats=stats))
