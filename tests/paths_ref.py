"""Helper of the path-record tests (include/rtw.h rtw_paths / rtw_paths_views), not a test: what the header says a sample's vertices
add up to, in numpy. The referees of the records themselves are the library's older entry points (rtw_radiance, rtw_views, rtw_cast)
and the oracle behind them (radiance_ref.py)."""
import numpy as np

from raytracing_weekend_amd import abi

F0 = np.float32(0)


def scrub(L):
    """removeNaNs: NaN channels become 0."""
    L = np.asarray(L, np.float32)
    return np.where(np.isnan(L), F0, L).astype(np.float32)


def fold(vertices):
    """head.radiance of one sample from its written records (a 1-d PATH_VERTEX array, in order): the contributions added in float32 in
    order from +0, then NaN channels replaced by 0."""
    L = np.zeros(3, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in np.asarray(vertices)["contribution"].reshape(-1, 3):
            L = (L + c).astype(np.float32)
    return scrub(L)


def fold_all(heads, vertices):
    """fold() of every sample of a (heads, vertices) pair at once: record j of a sample counts where j < its segments. Only
    meaningful where segments <= max_records (complete())."""
    c, seg = vertices["contribution"], heads["segments"]
    L = np.zeros(heads.shape + (3,), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(vertices.shape[-1]):
            L = np.where((j < seg)[..., None], (L + c[..., j, :]).astype(np.float32), L)
    return scrub(L)


def complete(heads, vertices):
    """where every segment of the sample has its record"""
    return heads["segments"] <= vertices.shape[-1]


def written(heads, vertices):
    """mask over vertices: the records the library wrote, j < min(segments, max_records)"""
    k = vertices.shape[-1]
    return np.arange(k) < np.minimum(heads["segments"], k)[..., None]


def light_sampled(heads, vertices):
    """per sample, the number of written records with RTW_PATH_LIGHT_SAMPLED"""
    return (((vertices["flags"] & abi.RTW_PATH_LIGHT_SAMPLED) != 0) & written(heads, vertices)).sum(-1)


def event(vertices):
    return vertices["flags"] & abi.RTW_PATH_EVENT_MASK


def luminance(rgb):
    rgb = np.asarray(rgb, np.float32)
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]
