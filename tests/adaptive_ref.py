"""numpy reference of rtw_render_adaptive's arithmetic (include/rtw.h): the checkpoint schedule, the per-pixel sums in the
summation contract's order, the batch-means error estimate and the stop rule with and without dilation. It takes a stack of
16-sample block sums S[b, y, x, 3] (block b = samples [16 b, 16 b + 16) of the render) and returns the image, n_p and err."""
import math

import numpy as np

SUM_BLOCK = 16
UNIT_BLOCKS = 8


def checkpoints(min_spp, step_spp, cap):
    """The checkpoint sequence, or ValueError for settings rtw_render_adaptive rejects (threshold / dilate aside)."""
    if cap <= 0 or cap % SUM_BLOCK:
        raise ValueError("cap")
    if min_spp < 2 * SUM_BLOCK or min_spp % SUM_BLOCK or min_spp > cap:
        raise ValueError("min_spp")
    if step_spp < 0 or step_spp % SUM_BLOCK:
        raise ValueError("step_spp")
    out, n = [], min_spp
    while True:
        out.append(n)
        if n >= cap:
            return out
        half = (n // 2 + SUM_BLOCK - 1) // SUM_BLOCK * SUM_BLOCK
        n = min(cap, n + (step_spp if step_spp > 0 else half))


def block_y(S):
    """y_b of block sums S[..., 3] in fp32, in the contract's order and without contraction."""
    S = np.asarray(S, np.float32)
    a = np.float32(0.2126) * S[..., 0]
    b = np.float32(0.7152) * S[..., 1]
    c = np.float32(0.0722) * S[..., 2]
    return ((a + b) + c) * np.float32(0.0625)


def moments(S, nb):
    """(M1, M2) in fp64 over the first nb blocks, in block order."""
    m1 = np.zeros(S.shape[1:-1], np.float64)
    m2 = np.zeros(S.shape[1:-1], np.float64)
    for b in range(nb):
        y = block_y(S[b]).astype(np.float64)
        m1 = m1 + y
        m2 = m2 + y * y
    return m1, m2


def error(m1, m2, B):
    """err = standard error of sqrt(Y) (fp64, rounded to fp32); NaN stays NaN."""
    b = float(B)
    mean = m1 / b
    v = (m2 - m1 * mean) / (b - 1.0)
    v = np.where(v < 0.0, 0.0, v)
    se = np.sqrt(v / b)
    mm = np.where(mean < 1e-3, 1e-3, mean)
    return (se / (2.0 * np.sqrt(mm))).astype(np.float32)


def mean_image(S, n):
    """Mean radiance of the first n samples of every pixel (n: int or per-pixel array of multiples of 16), in the summation
    contract's order: block sums in order inside aligned units of 8 blocks, unit sums in order, fp32, divided by (float)n."""
    nblk = S.shape[0]
    shape = S.shape[1:-1]
    n = np.broadcast_to(np.asarray(n), shape)
    acc = np.zeros(shape + (3,), np.float32)
    unit = np.zeros(shape + (3,), np.float32)
    for b in range(nblk):
        live = ((b + 1) * SUM_BLOCK <= n)[..., None]
        unit = np.where(live, unit + S[b].astype(np.float32), unit)
        if (b + 1) % UNIT_BLOCKS == 0:
            acc = np.where(live, acc + unit, acc)
            unit = np.where(live, np.float32(0), unit)
    acc = acc + unit  # the open unit (0 where it was just flushed: x + 0 = x)
    img = np.ones(shape + (4,), np.float32)
    img[..., :3] = acc / n[..., None].astype(np.float32)
    return img


def decide(err, active, threshold, dilate, at_cap):
    """Which active pixels stay active at a checkpoint (rtw.h stop rule)."""
    if at_cap:
        return np.zeros_like(active)
    ok = err < np.float32(threshold)
    stop = active & ok
    if dilate:
        h, w = err.shape
        blocked = active & ~ok  # an active pixel above the threshold blocks its neighbours
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ys = np.clip(np.arange(h) + dy, 0, h - 1)
                xs = np.clip(np.arange(w) + dx, 0, w - 1)
                stop &= ~blocked[ys][:, xs]
    return active & ~stop


def adaptive(S, threshold, min_spp, step_spp, cap, dilate):
    """(img, n, err) of an adaptive render whose block sums are S[b, y, x, 3] (at least cap / 16 blocks)."""
    cps = checkpoints(min_spp, step_spp, cap)
    shape = S.shape[1:-1]
    active = np.ones(shape, bool)
    n = np.zeros(shape, np.int64)
    err = np.zeros(shape, np.float32)
    for k, nk in enumerate(cps):
        m1, m2 = moments(S, nk // SUM_BLOCK)
        e = error(m1, m2, nk // SUM_BLOCK)
        err = np.where(active, e, err)
        keep = decide(e, active, threshold, dilate, k + 1 == len(cps))
        n = np.where(active & ~keep, nk, n)
        active = keep
        if not active.any():
            break
    return mean_image(S, n), n.astype(np.int32), err


def textbook_se(y, B):
    """Standard error of the mean of B iid draws with the sample variance of y (for the synthetic check)."""
    return math.sqrt(float(np.var(y, ddof=1)) / B)
