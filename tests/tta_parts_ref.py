"""numpy restatement of the per-pixel outputs of skp_tta_reduce_parts (include/skp.h, A18) on a given
average, and the shared cases of tests/test_tta_parts_cpu.py and tests/test_gpu_tta_parts.py.

Independent of product code.  With a (B, n, S, S) average ``avg`` in any float dtype:
label = the first token that attains the per-pixel maximum, value = that maximum, mass = the
tokens' sum in the contract's order, in ``avg``'s own dtype: chunk k holds tokens chunk·k …
min(chunk·k + chunk − 1, n − 1), each chunk's sum starts from 0 and adds in token order, and the
chunks' sums are added in chunk order, again from 0.
"""
import numpy as np

import tta_ref

CHUNK = 10      # kTok of csrc/skp_tta.hip
# n = 29 runs passes of 10, 10, 8 and 1 tokens, n = 26 passes of 10, 10, 4 and 2; S = 37 is odd; B = 2 gives
# image 1 a rotated and an out-of-view copy
PARTS_SHAPES = tta_ref.SHAPES + ((1, 2, 29, 37), (2, 2, 26, 37))
CHUNKED_SHAPES = tuple(s for s in PARTS_SHAPES if s[2] > CHUNK)


def parts_ref(avg, chunk=CHUNK):
    """avg (B, n, S, S) -> (label (B, S, S) int16, value (B, S, S), mass (B, S, S)), the last two in
    ``avg``'s dtype."""
    avg = np.asarray(avg)
    B, n, S, _ = avg.shape
    label = avg.argmax(axis=1).astype(np.int16)      # numpy: the first occurrence
    value = avg.max(axis=1)
    mass = np.zeros((B, S, S), avg.dtype)
    with np.errstate(invalid="ignore"):              # +inf and −inf in one pixel's tokens sum to NaN
        for t0 in range(0, n, chunk):
            part = np.zeros((B, S, S), avg.dtype)
            for t in range(t0, min(t0 + chunk, n)):
                part = part + avg[:, t]
            mass = mass + part
    return label, value, mass


def sequential_mass(avg):
    """The unchunked sum from 0 in token order, in ``avg``'s dtype (what the contract's mass is NOT
    for n > chunk)."""
    avg = np.asarray(avg)
    mass = np.zeros(avg[:, 0].shape, avg.dtype)
    for t in range(avg.shape[1]):
        mass = mass + avg[:, t]
    return mass


def pass_of(token, n, chunk=CHUNK):
    """Which pass of its chunk's walk a token falls in: 0 for a full pass of ``chunk`` tokens, and in a
    shorter last chunk the sub-passes of 8, 4, 2 and 1 tokens in turn, numbered by the walk's
    order over the whole token axis (tile_tokens of csrc/skp_tta.hip).  Returns (pass index over
    the whole axis, passes in all)."""
    bounds, t = [], 0
    while t + chunk <= n:
        bounds.append(t)
        t += chunk
    rest = n - t
    for width in (8, 4, 2, 1):
        if rest & width:
            bounds.append(t)
            t += width
    token = np.asarray(token)
    return np.searchsorted(np.asarray(bounds), token, side="right") - 1, len(bounds)


def tie_statistics(avg, chunk=CHUNK):
    """Of a (B, n, S, S) average: the share of pixels whose non-zero maximum is attained by more
    than one token, the share where two of those tokens lie in different passes, the number of
    distinct labels and the set of passes the winners fall in."""
    avg = np.asarray(avg)
    B, n, S, _ = avg.shape
    label, value, _ = parts_ref(avg, chunk)
    at_max = (avg == value[:, None]) & (value[:, None] != 0)
    tied = at_max.sum(axis=1) > 1
    passes, count = pass_of(np.arange(n), n, chunk)
    first = np.where(at_max, passes[None, :, None, None], count).min(axis=1)
    last = np.where(at_max, passes[None, :, None, None], -1).max(axis=1)
    across = tied & (last > first)
    winners = set(np.unique(pass_of(label[value != 0], n, chunk)[0]).tolist())
    return dict(tied=float(tied.mean()), across=float(across.mean()), labels=len(np.unique(label)), winners=winners,
                passes=count)
