"""rtw_paths_device and rtw_paths_views_device on torch tensors: rays or cameras in, the replayed samples' heads and path vertices out,
everything stays on the device (include/rtw.h rtw_paths_device / rtw_paths_views_device)."""
import ctypes as C

from . import _torch_call as T, abi

HEAD_FLOATS, VERTEX_FLOATS = C.sizeof(abi.PathHead) // 4, C.sizeof(abi.PathVertex) // 4  # 8 and 16
# the float32 columns of the two tensors, by rtw.h's field names; the integer fields (segments, shadow_rays, key, sample; prim,
# flags) keep their bits and are read with .view(torch.int32)
HEAD_COLUMNS = {"radiance": slice(0, 3), "segments": 3, "gather_time": 4, "shadow_rays": 5, "key": 6, "sample": 7}
VERTEX_COLUMNS = {"o": slice(0, 3), "t": 3, "d": slice(4, 7), "prim": 7, "contribution": slice(8, 11), "flags": 11, "throughput": slice(12, 15),
                  "ray_time": 15}


def _alloc(like, n, spp, k):
    """(heads, vertices), zeroed as abi.Renderer.paths' arrays are: the library writes a sample's first min(segments, k) vertices alone"""
    import torch

    return (torch.zeros((n, int(spp), HEAD_FLOATS), dtype=torch.float32, device=like.device),
            torch.zeros((n, int(spp), k, VERTEX_FLOATS), dtype=torch.float32, device=like.device))


def paths_torch(renderer, rays, spp, max_depth, max_records=None, seed=0x6314759, rng_kind=abi.RTW_RNG_PHILOX, sample_offset=0, estimator=0,
                key_offset=0, stats=None):
    """Replayed samples of an abi.Renderer along an (n, 8) float32 CUDA tensor of rays: (heads, vertices), float32 tensors of shapes
    (n, spp, 8) and (n, spp, max_records, 16) on the rays' device - rtw_path_head and rtw_path_vertex word for word (HEAD_COLUMNS,
    VERTEX_COLUMNS; the integer fields through .view(torch.int32)) - allocated here, written on torch's current stream; the call
    returns when they are written. Sample s of ray i is radiance_torch's sample at key key_offset + i and sample index
    sample_offset + s. max_records None keeps every vertex, 0 returns the heads alone. The tensor must be contiguous and live on the
    renderer's device. Under torch's default stream (the null handle, which the library reads as "the context's own stream") the
    stream's pending work is waited for here, before the call."""
    n = T.check_tensor("paths_torch", "rays", rays, (8,), renderer)
    k = abi.make_paths_params(spp, max_depth, max_records).max_records  # (spp and max_records are checked even when there is nothing to trace)
    abi._check_pairs("paths_torch", n, spp)
    return T.run(rays, n, lambda: _alloc(rays, n, spp, k),
                 lambda out, stream: renderer.paths_device(n, rays.data_ptr(), out[0].data_ptr(), out[1].data_ptr() if k else 0, spp, max_depth, k,
                                                           seed=seed, rng_kind=rng_kind, sample_offset=sample_offset, estimator=estimator,
                                                           key_offset=key_offset, stream_ptr=stream, stats=stats))


def paths_views_torch(renderer, views, width, height, first, count, spp, max_depth, max_records=None, rng_kind=abi.RTW_RNG_PHILOX,
                      sample_offset=0, estimator=0, stats=None):
    """Replayed samples of pixels [first, first + count) of views_torch's flattened (view, y, x) index, from an (n, 28) float32 CUDA
    tensor of rtw_view records (torch_views.views_tensor): paths_torch's two tensors, shapes (count, spp, 8) and
    (count, spp, max_records, 16), allocated here, written on torch's current stream; the call returns when they are written. The
    records are not read back (views_torch's rule for the camera type). The default stream is waited for as in paths_torch."""
    n = T.check_tensor("paths_views_torch", "views", views, (C.sizeof(abi.View) // 4,), renderer)
    abi.make_view_params(width, height, spp, max_depth)
    abi._check_pixels("paths_views_torch", n, width, height)
    first = abi._path_window("paths_views_torch", first, count, n * int(width) * int(height))
    count, k = int(count), abi._max_records("paths_views_torch", max_records, max_depth)
    abi._check_pairs("paths_views_torch", count, spp)
    return T.run(views, count, lambda: _alloc(views, count, spp, k),
                 lambda out, stream: renderer.paths_views_device(n, views.data_ptr(), out[0].data_ptr(), out[1].data_ptr() if k else 0, width, height,
                                                                 first, count, spp, max_depth, k, rng_kind=rng_kind, sample_offset=sample_offset,
                                                                 estimator=estimator, stream_ptr=stream, stats=stats))
