"""Numpy oracles of skp_match_topk and skp_label_vote (include/skp.h) and of eval.propagate_labels, with
the synthetic sequence that the CPU and GPU tests share.

match_topk: skp_match_field's norms, dots and keys (tests/match_field_ref.py: the exact fmaf, the chains
in token order).  The dots of every pair are formed, whether or not the pair lies in a window: the
window only decides which keys take part, and the keys that do are sorted (key descending, q
ascending).  ``window_dot`` forms only the dots inside the windows, by the same chain, for the callers
that need many frames; the CPU tests hold it to ``chain_dot``.

label_vote: the selection is exact; the weights come from the fp32 a_i of the definition, and the
exponentials, products, sums and the division are float64.
"""
import numpy as np

import match_field_ref as R

F32 = R.F32
NEG_INF = R.NEG_INF


def window(S, w):
    """allowed (S², S²) bool: allowed[p, q] where |qr − r| <= w and |qc − c| <= w."""
    r, c = np.divmod(np.arange(S * S), S)
    return (np.abs(r[None, :] - r[:, None]) <= w) & (np.abs(c[None, :] - c[:, None]) <= w)


def window_dot(x, y, w):
    """x, y (n, S, S) -> (S², S²) float32: chain_dot's value at every pair inside the window, 0 elsewhere."""
    n, S = x.shape[0], x.shape[-1]
    out = np.zeros((S, S, S, S), F32)
    for dr in range(-w, w + 1):
        for dc in range(-w, w + 1):
            r0, r1, c0, c1 = max(0, -dr), min(S, S - dr), max(0, -dc), min(S, S - dc)
            if r0 >= r1 or c0 >= c1:
                continue
            d = np.zeros((r1 - r0, c1 - c0), F32)
            for t in range(n):
                d = R.fmaf(x[t, r0:r1, c0:c1], y[t, r0 + dr:r1 + dr, c0 + dc:c1 + dc], d)
            rr, cc = np.meshgrid(np.arange(r0, r1), np.arange(c0, c1), indexing="ij")
            out[rr, cc, rr + dr, cc + dc] = d
    return out.reshape(S * S, S * S)


def match_topk_one(x, y, w, K, dot=None):
    """One image: x, y (n, S, S) float32 -> (index (K, S, S) int32, score (K, S, S) float32)."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    n, S = x.shape[0], x.shape[-1]
    P = S * S
    x, y = x.reshape(n, P), y.reshape(n, P)
    rx, okx = R.recip_norm(R.chain_norm(x))
    ry, oky = R.recip_norm(R.chain_norm(y))
    if dot is None:
        dot = R.chain_dot(x, y)
    with np.errstate(all="ignore"):
        key = (dot * ry[None, :]).astype(F32)
    key = np.where(np.isnan(key), NEG_INF, key)
    allowed = window(S, w) & oky[None, :]
    by_key = np.argsort(-key, axis=1, kind="stable")                      # key descending, q ascending
    out_last = np.argsort(~np.take_along_axis(allowed, by_key, axis=1), axis=1, kind="stable")
    order = np.take_along_axis(by_key, out_last, axis=1)                  # the pairs that take part first, in order
    count = allowed.sum(axis=1)
    index = np.full((K, P), -1, np.int32)
    score = np.full((K, P), NEG_INF, F32)
    for i in range(min(K, P)):
        q = order[:, i]
        ok = okx & (count > i)
        with np.errstate(all="ignore"):
            sc = (key[np.arange(P), q] * rx).astype(F32)
        index[i] = np.where(ok, q, -1)
        score[i] = np.where(ok, sc, NEG_INF)
    return index.reshape(K, S, S), score.reshape(K, S, S)


def match_topk(x, y, w, K, windowed=False):
    """x, y (B or 1, n, S, S) -> (index (B, K, S, S), score (B, K, S, S)); ``windowed`` forms the dots
    inside the windows only."""
    B = max(x.shape[0], y.shape[0])
    out = []
    for b in range(B):
        xb, yb = x[b if x.shape[0] > 1 else 0], y[b if y.shape[0] > 1 else 0]
        out.append(match_topk_one(xb, yb, w, K, window_dot(np.asarray(xb, F32), np.asarray(yb, F32), w) if windowed else None))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def inv_tau32(tau):
    """1 / tau rounded once to float32, as ops.label_vote passes it."""
    return F32(1.0 / float(tau))


def label_vote(index, score, labels, inv_tau, Kv):
    """index, score (M, K, S, S), labels (M, Cl, S, S) float32, inv_tau float32 ->
    (soft (Cl, S, S) float64, label (S, S) int32, confidence (S, S) float64, source (Kv, S, S) int32)."""
    index, score, labels = np.asarray(index), np.asarray(score, F32), np.asarray(labels, F32)
    M, K, S, _ = index.shape
    P, Cl = S * S, labels.shape[1]
    idx = index.reshape(M * K, P).T.astype(np.int64)                      # (P, M·K), c = j·K + i ascending in (j, i)
    sc = score.reshape(M * K, P).T
    valid = (idx >= 0) & (idx < P) & ~np.isnan(sc)
    by_score = np.argsort(-np.where(valid, sc, NEG_INF), axis=1, kind="stable")
    out_last = np.argsort(~np.take_along_axis(valid, by_score, axis=1), axis=1, kind="stable")
    order = np.take_along_axis(by_score, out_last, axis=1)[:, :Kv]        # (P, Kv) candidates by rank
    m = np.minimum(valid.sum(axis=1), Kv)
    live = np.arange(Kv)[None, :] < m[:, None]
    rows = np.arange(P)[:, None]
    j, q, s = order // K, np.where(live, idx[rows, order], 0), sc[rows, order]
    with np.errstate(all="ignore"):
        d = (s - s[:, :1]).astype(F32)
        a = (d * F32(inv_tau)).astype(F32)
    e = np.where(live, np.exp(a.astype(np.float64)), 0.0)
    Z = e.sum(axis=1)
    lab = labels.reshape(M, Cl, P)[j[:, :, None], np.arange(Cl)[None, None, :], q[:, :, None]].astype(np.float64)
    num = (e[:, :, None] * lab).sum(axis=1)                               # (P, Cl)
    soft = np.where((m > 0)[:, None], num / np.where(Z > 0, Z, 1.0)[:, None], 0.0)
    label = np.where(m > 0, soft.argmax(axis=1), -1).astype(np.int32)
    conf = np.where(m > 0, soft.max(axis=1), 0.0)
    source = np.where(live, j * P + q, -1).astype(np.int32)
    return soft.T.reshape(Cl, S, S), label.reshape(S, S), conf.reshape(S, S), source.T.reshape(Kv, S, S)


def one_hot(labels0):
    """(S, S) integers -> (Cl, S, S) float32: class c >= 0 a one-hot plane, −1 an all-zero column."""
    labels0 = np.asarray(labels0)
    Cl = max(int(labels0.max()) + 1, 1)
    return (labels0[None] == np.arange(Cl)[:, None, None]).astype(F32)


def context_of(t, memory):
    """The context frames of frame t >= 1: frame 0 and the last ``memory`` frames, distinct, in frame order."""
    return sorted({0, *range(max(t - memory, 0), t)})


def propagate(frames, labels0, w, K, tau, memory):
    """eval.propagate_labels with the oracles: frames (T, n, S, S), labels0 (S, S) integers ->
    (label (T, S, S) int32, confidence (T, S, S) float32, soft (T, Cl, S, S) float32); each frame's soft
    output, rounded to float32, is its label map for the frames after it."""
    frames = np.asarray(frames, F32)
    soft = [one_hot(labels0)]
    label = [np.asarray(labels0, np.int32)]
    conf = [(np.asarray(labels0) >= 0).astype(F32)]
    for t in range(1, len(frames)):
        ctx = context_of(t, memory)
        index, score = match_topk(frames[t][None], frames[ctx], w, K, windowed=True)
        s, l, c, _ = label_vote(index, score, np.stack([soft[j] for j in ctx]), inv_tau32(tau), K)
        soft.append(s.astype(F32))
        label.append(l)
        conf.append(c.astype(F32))
    return np.stack(label), np.stack(conf), np.stack(soft)


# ------------------------------------------------------------------------------------------ the synthetic sequence
SEQ = dict(n=48, S=32, T=8, canvas=96, sigma=3.0, radius=7, w=3, k=5, tau=0.02, memory=2)
ORIGIN, DISK = (28, 36), (19, 13)        # frame 0's window on the canvas; the disk's centre in frame 0


def sequence(seed):
    """-> (frames (T, n, S, S) float32, masks (T, S, S) bool): 48 Gaussian blobs (σ = 3) on a 96² canvas,
    frame t the 32² window at ORIGIN + t·(1, −1); the true mask of frame t is the disk of radius 7 around
    DISK − t·(1, −1), which stays inside every frame."""
    n, S, T, C = SEQ["n"], SEQ["S"], SEQ["T"], SEQ["canvas"]
    rng = np.random.default_rng(seed)
    cy, cx = rng.uniform(0, C, n), rng.uniform(0, C, n)
    gy, gx = np.mgrid[0:C, 0:C]
    canvas = np.exp(-((gy[None] - cy[:, None, None]) ** 2 + (gx[None] - cx[:, None, None]) ** 2)
                    / (2 * SEQ["sigma"] ** 2)).astype(F32)
    frames = np.stack([canvas[:, ORIGIN[0] + t:ORIGIN[0] + t + S, ORIGIN[1] - t:ORIGIN[1] - t + S] for t in range(T)])
    r, c = np.mgrid[0:S, 0:S]
    masks = np.stack([(r - (DISK[0] - t)) ** 2 + (c - (DISK[1] + t)) ** 2 <= SEQ["radius"] ** 2 for t in range(T)])
    return np.ascontiguousarray(frames), masks


def iou(a, b):
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    return float((a & b).sum()) / float(max((a | b).sum(), 1))
