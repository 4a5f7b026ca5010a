"""numpy restatement of the match outputs of skp_tta_reduce_match (include/skp.h, A18) on a given
average, and the shared cases of tests/test_tta_match_cpu.py and tests/test_gpu_tta_match.py.

Independent of product code.  With a (B, n, S, S) average ``avg`` in any float dtype and (Q, n)
``queries``, all in ``avg``'s own dtype: nrm = Σ_t a·a and dot_q = Σ_t a·d_q[t] in the contract's order
(chunk k holds tokens chunk·k … min(chunk·k + chunk − 1, n − 1), each chunk's sums start from 0 and add
in token order, the chunks' sums are added in chunk order, again from 0; every product and sum is an
array operation of its own, so none is fused), score = dot / sqrt(nrm), −inf where nrm is not > 0 or
the quotient is NaN, and per image and query the first row-major maximum.
"""
import numpy as np

import tta_ref

CHUNK = 10      # kTok of csrc/skp_tta.hip
# n = 1; one short chunk (2, 3, 5); exactly one full chunk (10); n = 29 runs passes of 10, 10, 8 and 1
# tokens, n = 26 passes of 10, 10, 4 and 2; S = 37 is odd, S = 64 spans several row bands; the last image
# of tta_ref.ALL_OUT_OF_VIEW has every copy out of view
MATCH_SHAPES = tta_ref.SHAPES + ((1, 3, 10, 37), (1, 2, 29, 37), (2, 2, 26, 37))
CHUNKED_SHAPES = tuple(s for s in MATCH_SHAPES if s[2] > CHUNK)
QS = (1, 3, 16)
TILE_W, TILE_H = 64, 4      # kTileW, kTileH


def sums(avg, queries, chunk=CHUNK):
    """avg (B, n, S, S), queries (Q, n) -> (nrm (B, S, S), dot (B, Q, S, S)) in ``avg``'s dtype and the
    chunked order."""
    avg = np.asarray(avg)
    d = np.asarray(queries).astype(avg.dtype)
    B, n, S, _ = avg.shape
    Q = d.shape[0]
    nrm = np.zeros((B, S, S), avg.dtype)
    dot = np.zeros((B, Q, S, S), avg.dtype)
    with np.errstate(invalid="ignore", over="ignore"):      # inf · 0 and inf − inf are NaN, as in fp32
        for t0 in range(0, n, chunk):
            part_n = np.zeros((B, S, S), avg.dtype)
            part_d = np.zeros((B, Q, S, S), avg.dtype)
            for t in range(t0, min(t0 + chunk, n)):
                a = avg[:, t]
                sq = a * a
                part_n = part_n + sq
                prod = a[:, None] * d[None, :, t, None, None]
                part_d = part_d + prod
            nrm = nrm + part_n
            dot = dot + part_d
    return nrm, dot


def scores_of(nrm, dot):
    """The contract's score: dot / sqrt(nrm), −inf where nrm is not > 0 or the quotient is NaN."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = dot / np.sqrt(nrm)[:, None]
    ok = (nrm > 0)[:, None] & ~np.isnan(s)
    return np.where(ok, s, -np.inf).astype(dot.dtype)


def match_ref(avg, queries, chunk=CHUNK):
    """avg (B, n, S, S), queries (Q, n) -> (match_pos (B, Q, 2), match_score (B, Q), score_map
    (B, Q, S, S)), all in ``avg``'s dtype."""
    avg = np.asarray(avg)
    B, n, S, _ = avg.shape
    score = scores_of(*sums(avg, queries, chunk))
    flat = score.reshape(B, score.shape[1], S * S)
    idx = flat.argmax(axis=2)                        # numpy: the first occurrence; no NaN by construction
    pos = np.stack([idx // S + 0.5, idx % S + 0.5], axis=-1).astype(avg.dtype)
    return pos, np.take_along_axis(flat, idx[..., None], 2)[..., 0], score


def sequential_scores(avg, queries):
    """The scores with the unchunked sums from 0 in token order (what the contract's are NOT for n > chunk)."""
    avg = np.asarray(avg)
    return scores_of(*sums(avg, queries, chunk=max(1, avg.shape[1])))


def queries_of(avg, Q, seed=0):
    """Q unit descriptors (Q, n) float32 read at seeded pixels of image 0 whose signature is finite and not
    zero (without repeats where there are Q such pixels), normalised in float64; also their pixels (Q,)."""
    sig = np.asarray(avg)[0].astype(np.float64)
    n, S, _ = sig.shape
    sig = sig.reshape(n, S * S).T
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt((sig * sig).sum(axis=1))
    good = np.flatnonzero(np.isfinite(length) & (length > 0))
    assert good.size > 0, "no pixel of image 0 has a finite non-zero signature"
    g = np.random.default_rng([seed, Q, n, S])
    pix = g.choice(good, size=Q, replace=good.size < Q)
    return (sig[pix] / length[pix, None]).astype(np.float32), pix


def tiles_of(pos, S):
    """The 64 × 4-pixel tile (row-major tile index) of each (row + 0.5, col + 0.5) position."""
    pos = np.asarray(pos)
    row, col = np.floor(pos[..., 0]).astype(np.int64), np.floor(pos[..., 1]).astype(np.int64)
    return (row // TILE_H) * (-(-S // TILE_W)) + col // TILE_W
