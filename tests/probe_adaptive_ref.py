"""Helper of the adaptive-probe tests (include/rtw.h rtw_probe_adaptive), not a test: the referee of the stop rule, the sample counts,
the errors and the values, from block sums (irradiance) or block counts (occlusion).

Irradiance is adaptive_ref.adaptive on the block sums as a frame of one row, [b, 1, n, 3], with dilate 0, followed by the multiply by
float32 pi. Occlusion walks the same checkpoints with adaptive_ref's error and decision over y_b = float32(c_b) * 0.0625f and
finishes with float32(open) / float32(n_i)."""
import numpy as np

import adaptive_ref as A

PI = np.float32(3.14159265)
SUM_BLOCK = A.SUM_BLOCK


def reference(S_or_counts, threshold, min_spp, step_spp, cap, mode="irradiance"):
    """((n, 4) float32 results, (n,) int32 n_i, (n,) float32 err). Irradiance: S_or_counts is (b, n, 3) float32 block sums, block b
    being samples [16 b, 16 b + 16) counted from sample_offset; occlusion: (b, n) integer unoccluded counts; b >= cap / 16."""
    if mode == "irradiance":
        S = np.asarray(S_or_counts, np.float32)
        assert S.ndim == 3 and S.shape[2] == 3 and S.shape[0] * SUM_BLOCK >= cap
        img, n, err = A.adaptive(S[:, None], threshold, min_spp, step_spp, cap, 0)
        out = np.ones((S.shape[1], 4), np.float32)
        with np.errstate(invalid="ignore"):
            out[:, :3] = img[0, :, :3] * PI
        return out, n[0].astype(np.int32), err[0].astype(np.float32)
    assert mode == "occlusion"
    cnt = np.asarray(S_or_counts).astype(np.int64)
    assert cnt.ndim == 2 and cnt.shape[0] * SUM_BLOCK >= cap
    cps = A.checkpoints(min_spp, step_spp, cap)
    m = cnt.shape[1]
    active = np.ones((1, m), bool)
    n = np.zeros((1, m), np.int64)
    err = np.zeros((1, m), np.float32)
    y = (cnt.astype(np.float32) * np.float32(0.0625)).astype(np.float64)
    for k, nk in enumerate(cps):
        nb = nk // SUM_BLOCK
        m1 = np.zeros(m, np.float64)
        m2 = np.zeros(m, np.float64)
        for b in range(nb):
            m1 = m1 + y[b]
            m2 = m2 + y[b] * y[b]
        e = A.error(m1, m2, nb)[None]
        err = np.where(active, e, err)
        keep = A.decide(e, active, threshold, 0, k + 1 == len(cps))
        n = np.where(active & ~keep, nk, n)
        active = keep
        if not active.any():
            break
    n = n[0]
    open_ = np.array([cnt[: n[i] // SUM_BLOCK, i].sum() for i in range(m)], np.int64)
    out = np.ones((m, 4), np.float32)
    out[:, :3] = (open_.astype(np.float32) / n.astype(np.float32))[:, None]
    return out, n.astype(np.int32), err[0].astype(np.float32)


def block_sums(samples):
    """(spp / 16, n, 3) float32 block sums of (spp, n, 3) sample radiances: the samples of a block added in order from zero."""
    s = np.asarray(samples, np.float32)
    nb = s.shape[0] // SUM_BLOCK
    out = np.zeros((nb,) + s.shape[1:], np.float32)
    for b in range(nb):
        for i in range(SUM_BLOCK):
            out[b] = out[b] + s[b * SUM_BLOCK + i]
    return out


def block_counts(open_):
    """(spp / 16, n) int64 counts of (spp, n) booleans."""
    o = np.asarray(open_, bool)
    return o.reshape(o.shape[0] // SUM_BLOCK, SUM_BLOCK, o.shape[1]).sum(1).astype(np.int64)


def histogram(n):
    """{n_i: probes} in ascending n_i."""
    v, c = np.unique(np.asarray(n), return_counts=True)
    return {int(a): int(b) for a, b in zip(v, c)}


def not_vacuous(n, lo, hi):
    """The tests' condition on a batch's n_i: at least four distinct values, at least 8 probes at the first checkpoint and 8 at the cap."""
    h = histogram(n)
    return len(h) >= 4 and h.get(lo, 0) >= 8 and h.get(hi, 0) >= 8
