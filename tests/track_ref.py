"""The numpy restatement of the keypoint tracker's definition (include/skp.h, skp_track_step and
skp_track_backtrace): float32 throughout, every product and the division rounded on their own, the
two stages as maxima over shifted slices taken in ascending offset order with a strict >, so the
first offset that attains a maximum wins; a pixel outside the plane is the sentinel −1, which no
product of non-negative values falls below, so it is never the maximum's source.

Also the synthetic sequence of the issue (a blob that moves, a brighter distractor that flashes) and
the brute-force path search that the reference is held to on a tiny grid."""
import numpy as np

F = np.float32


def weights(sigma, r):
    """exp(−k² / (2σ²)) in double, rounded once."""
    k = np.arange(r + 1, dtype=np.float64)
    return np.exp(-(k * k) / (2.0 * float(sigma) ** 2)).astype(F)


def _stage(m, w, axis):
    """max over d ∈ [−r, r] of shift(m, d along axis) · w[|d|] and the smallest d that attains it.
    ``m`` (n, S, S); out-of-plane sources are −1."""
    r, S = len(w) - 1, m.shape[-1]
    best = np.full(m.shape, -np.inf, dtype=F)
    off = np.zeros(m.shape, dtype=np.int64)
    for d in range(-r, r + 1):
        src = np.full(m.shape, -1.0, dtype=F)          # src[..., i, ...] = m[..., i + d, ...]
        lo, hi = max(0, -d), min(S, S - d)
        if lo < hi:
            dst, frm = [slice(None)] * 3, [slice(None)] * 3
            dst[axis], frm[axis] = slice(lo, hi), slice(lo + d, hi + d)
            src[tuple(dst)] = m[tuple(frm)]
        v = (src * w[abs(d)]).astype(F)
        take = v > best
        best = np.where(take, v, best)
        off = np.where(take, d, off)
    return best, off


def first_max(m):
    """(max, first row-major index attaining it) of every plane of (n, S, S)."""
    flat = m.reshape(m.shape[0], -1)
    idx = flat.argmax(axis=1)
    return flat[np.arange(flat.shape[0]), idx].astype(F), idx.astype(np.int32)


def step(avg, prev, w):
    """One frame: ``avg`` (n, S, S) float32, ``prev`` the previous frame's result or None.
    Returns (score, score_max, best, back int16)."""
    avg = np.ascontiguousarray(avg, dtype=F)
    r = len(w) - 1
    side = 2 * r + 1
    if prev is None:
        score = avg.copy()
        back = np.full(avg.shape, r * side + r, dtype=np.int16)
    else:
        m, M = prev[0], prev[1]
        live = (M != 0) & np.isfinite(M)
        with np.errstate(divide="ignore", invalid="ignore"):
            mt = (m / M[:, None, None]).astype(F)
        mt = np.where(live[:, None, None], mt, F(1.0)).astype(F)
        g, gdx = _stage(mt, w, axis=2)
        h, dy = _stage(g, w, axis=1)
        S = avg.shape[-1]
        rows = np.arange(S)[None, :, None] + dy
        dx = np.take_along_axis(gdx, rows, axis=1)
        score = (avg * h).astype(F)
        back = ((dy + r) * side + (dx + r)).astype(np.int16)
    M, best = first_max(score)
    return score, M, best, back


def backtrace(backs, best_last, r):
    """``backs`` (T, n, S, S), ``best_last`` (n) -> pos (T, n, 2) float32 = (row + 0.5, col + 0.5)."""
    T, n, S, _ = backs.shape
    side = 2 * r + 1
    pos = np.zeros((T, n, 2), dtype=F)
    for j in range(n):
        y, x = divmod(int(best_last[j]), S)
        for t in range(T - 1, -1, -1):
            pos[t, j] = (y + 0.5, x + 0.5)
            if t > 0:
                code = int(backs[t, j, y, x])
                y, x = y + code // side - r, x + code % side - r
                assert 0 <= y < S and 0 <= x < S, "a back-pointer left the plane"
    return pos


def track(frames, w):
    """Every frame's step and the backtrace: ``frames`` (T, n, S, S) -> (list of per-frame states, pos)."""
    states, prev = [], None
    for a in frames:
        prev = step(a, prev, w)
        states.append(prev)
    r = len(w) - 1
    return states, backtrace(np.stack([s[3] for s in states]), states[-1][2], r)


def synthetic(S=48, T=12, flashes=(3, 4, 8)):
    """The issue's sequence -> (frames (T, 1, S, S) float32, truth (T, 2) integer pixels): a Gaussian
    blob of height 1 that moves (2, 1) pixels per frame from (8, 10), and in ``flashes`` a blob of
    height 1.5 near the far corner."""
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    frames = np.zeros((T, 1, S, S), dtype=F)
    truth = np.zeros((T, 2), dtype=np.int64)
    for t in range(T):
        y, x = 8 + 2 * t, 10 + t
        truth[t] = (y, x)
        plane = np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * 2.0 ** 2))
        if t in flashes:
            plane = plane + 1.5 * np.exp(-((yy - 12) ** 2 + (xx - 38) ** 2) / (2 * 2.0 ** 2))
        frames[t, 0] = plane.astype(F)
    return frames, truth


def brute_force(frames, w):
    """All S^(2T) paths of one token on a tiny grid -> (the optimal value, the list of optimal paths as
    tuples of flat indices).  A path's value is the reference's own expression evaluated along it,
    Π_t a_t(p_t) · ((m̃ · w[|dx|]) · w[|dy|]) without the normalisation (inputs for which every product
    is exact make it path-order independent); steps longer than r are not paths."""
    T, S = frames.shape[0], frames.shape[-1]
    r = len(w) - 1
    P = S * S
    a = frames.reshape(T, P).astype(np.float64)
    w64 = np.concatenate([w.astype(np.float64), np.zeros(S)])      # a step longer than r: weight 0
    paths = np.indices((P,) * T).reshape(T, -1)                    # (T, P^T), every path a column
    v = a[0][paths[0]]
    ok = np.ones(paths.shape[1], dtype=bool)
    for t in range(1, T):
        dy, dx = np.abs(paths[t] // S - paths[t - 1] // S), np.abs(paths[t] % S - paths[t - 1] % S)
        ok &= (dy <= r) & (dx <= r)
        v = v * w64[dx] * w64[dy] * a[t][paths[t]]
    v = np.where(ok, v, -1.0)
    best = float(v.max())
    return best, [tuple(int(i) for i in paths[:, c]) for c in np.flatnonzero(v == best)]
