"""Helper of the adaptive-view tests (include/rtw.h rtw_views_adaptive), not a test: the referee of the stop rule, the sample counts,
the errors and the frames, from block sums.

View v of rtw_views_adaptive is defined as rtw_render_adaptive of the uploaded scene with views[v]'s camera in its header, so the
referee is adaptive_ref.adaptive applied to every view on its own: with dilate = 1 the 3x3 neighbourhood is that view's frame,
clamped at its edges, and never a pixel of the view before or after it in the flattened layout."""
import numpy as np

import adaptive_ref as A

SUM_BLOCK = A.SUM_BLOCK


def reference(S, threshold, min_spp, step_spp, cap, dilate):
    """((n, h, w, 4) float32 frames, (n, h, w) int32 n_p, (n, h, w) float32 err) from S[b, v, y, x, 3], the float32 block sums of block b
    (samples [16 b, 16 b + 16) counted from sample_offset) of pixel (x, y) of view v; b >= cap / 16."""
    S = np.asarray(S, np.float32)
    assert S.ndim == 5 and S.shape[4] == 3 and S.shape[0] * SUM_BLOCK >= cap
    nv, h, w = S.shape[1:4]
    img, n, err = np.empty((nv, h, w, 4), np.float32), np.empty((nv, h, w), np.int32), np.empty((nv, h, w), np.float32)
    for v in range(nv):
        with np.errstate(invalid="ignore"):
            img[v], n[v], err[v] = A.adaptive(S[:, v], threshold, min_spp, step_spp, cap, dilate)
    return img, n, err


def checkpoint_errors(S, min_spp, step_spp, cap):
    """{n_k: (n, h, w) float32 err at checkpoint n_k} of every pixel, whether it is still active there or not."""
    S = np.asarray(S, np.float32)
    out = {}
    for nk in A.checkpoints(min_spp, step_spp, cap):
        m1, m2 = A.moments(S, nk // SUM_BLOCK)
        out[nk] = A.error(m1, m2, nk // SUM_BLOCK)
    return out


def near_ties(S, threshold, min_spp, step_spp, cap, rel=1e-6):
    """(n, h, w) bool: pixels one of whose checkpoint errors lies within `rel` (relative) of the threshold, so that a last-bit
    difference in a block sum could move their decision (test_gpu_adaptive.py's tie exclusion). With dilation a tie also reaches the
    3x3 neighbours inside the view."""
    tie = np.zeros(np.asarray(S).shape[1:4], bool)
    for e in checkpoint_errors(S, min_spp, step_spp, cap).values():
        with np.errstate(invalid="ignore"):
            tie |= np.abs(e.astype(np.float64) - float(threshold)) <= rel * float(threshold)
    return tie


def spread(tie):
    """the ties and their 3x3 neighbours inside each view (clamped at its edges)"""
    nv, h, w = tie.shape
    out = tie.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys = np.clip(np.arange(h) + dy, 0, h - 1)
            xs = np.clip(np.arange(w) + dx, 0, w - 1)
            out |= tie[:, ys][:, :, xs]
    return out


def histogram(n):
    """{n_p: pixels} in ascending n_p."""
    v, c = np.unique(np.asarray(n), return_counts=True)
    return {int(a): int(b) for a, b in zip(v, c)}
