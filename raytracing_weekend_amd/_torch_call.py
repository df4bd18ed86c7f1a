"""What the *_torch wrappers share: the checks of an input tensor and the allocate / pick the stream / call step. torch is imported
inside the functions, so the package imports without it."""


def check_device(prefix, name, t, renderer):
    if not t.is_cuda or t.device.index != renderer.devices[0]:
        raise ValueError(f"{prefix}: {name} on {t.device}, the renderer answers on cuda:{renderer.devices[0]}")


def check_tensor(prefix, name, t, tail, renderer):
    """`t` is (n,) + tail (tail None: the caller has checked the shape), on the renderer's device, float32 and contiguous - checked
    in this order. Returns n."""
    import torch

    if tail is not None and (t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail):
        raise ValueError(f"{prefix}: {name} of shape {tuple(t.shape)}, expected (n, {', '.join(str(k) for k in tail)})")
    check_device(prefix, name, t, renderer)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{prefix}: {name} must be a contiguous float32 CUDA tensor")
    return t.shape[0]


def empty(like, shape, dtype="float32"):
    import torch

    return torch.empty(tuple(shape), dtype=getattr(torch, dtype), device=like.device)


def empty_adaptive(like, lead):
    """(values, sample counts, errors) of an adaptive call over `lead` pixels or probes"""
    return empty(like, lead + (4,)), empty(like, lead, "int32"), empty(like, lead)


def run(like, work, alloc, call):
    """alloc() on `like`'s device, then - only when there is work - call(outputs, handle of torch's current stream). The default
    stream's null handle means "the context's own stream" to the library, which does not wait for the default stream's pending
    work: that work is waited for here first."""
    import torch

    with torch.cuda.device(like.device):
        out = alloc()
        stream = torch.cuda.current_stream()
        if work:
            if stream.cuda_stream == 0:
                stream.synchronize()
            call(out, stream.cuda_stream)
    return out
