"""ops.label_vote (skp_label_vote) against the numpy oracle of tests/propagate_ref.py.

``source`` is exact: the selection compares scores and (j, i) only.  ``soft`` and ``confidence`` are held
to a tolerance that is derived here, not measured.  The oracle takes the fp32 a_i of the definition (the
subtraction and the product by inv_tau are single correctly rounded operations, the same on both
sides) and is exact from there on (float64; its own error, about 2^-52, is not counted).  With
u = 2^-24, the unit roundoff of fp32, and m <= Kv ranks, on the device:
  e_i   expf's documented bound is 1 ulp (include/skp.h names it), and an ulp is at most 2^-23 = 2u of
        the value: relative error at most 2u.
  e_i·l_i   one product, rounded: 3u with the above.  Labels are non-negative, so are all terms.
  Σ e_i·l_i  in rank order: a term passes through at most m − 1 additions of non-negative numbers, each
        adding u relative to the partial sum: the sum is within (3 + Kv − 1)u = (Kv + 2)u of Σ e_i·l_i.
  Z     likewise without the product: (Kv + 1)u.
  the division: u more.
Together (2·Kv + 4)u to first order; the products of these errors are below u² · (2·Kv + 4)² < u for
Kv <= 16, so TOL(Kv) = (2·Kv + 5) · 2^-24 relative to the oracle's value bounds the difference.  Nothing
underflows: the scores lie in [−1, 1], so a_i >= −2 / 0.07 and e_i >= 3e-13, and the labels, random in
(0, 1) at float32's spacing, are 0 or at least 2^-24.

``label`` is compared where the oracle's greatest soft value exceeds its second by more than
2 · TOL · the greatest, which separates the two on the device whatever the rounding; with random
labels in (0, 1) at most 1 % of the pixels may fall out, which the CPU test checks on the oracle alone.

Shapes (M, K, Kv, S, Cl): (3, 5, 5, 24, 2); (1, 16, 16, 20, 7), both caps; (4, 4, 2, 16, 1), Kv < K and a
single class.  Each with empty lists, partly filled lists, indices outside [−1, S²) and scores on a grid
of 1 / 32, so that many tie within a context and across contexts.
"""
import functools

import numpy as np
import pytest
import torch

import propagate_ref as P

gpu = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((3, 5, 5, 24, 2), (1, 16, 16, 20, 7), (4, 4, 2, 16, 1))
TAU = 0.07


def tol(Kv):
    return (2 * Kv + 5) * 2.0 ** -24


@pytest.fixture
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@functools.lru_cache(maxsize=None)
def case(M, K, Kv, S, Cl):
    """-> (index, score, labels, the oracle's (soft, label, confidence, source))."""
    rng = np.random.default_rng([M, K, Kv, S, Cl])
    P2 = S * S
    index = rng.integers(0, P2, (M, K, S, S)).astype(np.int32)
    score = (rng.integers(-32, 33, (M, K, S, S)) / 32.0).astype(np.float32)
    score = -np.sort(-score, axis=1)                                   # lists as skp_match_topk writes them: descending
    filled = rng.integers(0, K + 1, (M, 1, S, S))                      # slots from `filled` on are empty
    filled[:, :, 0, :3] = 0                                            # three pixels without any candidate
    filled[:, :, 1, :] = K
    empty = np.arange(K)[None, :, None, None] >= filled
    index[empty], score[empty] = -1, -np.inf
    index[0, 0, 1, 0], index[0, K - 1, 1, 1], index[M - 1, 0, 1, 2], index[0, 0, 1, 3] = P2, 2 ** 31 - 1, -7, -2 ** 31
    labels = rng.random((M, Cl, S, S), dtype=np.float32)
    labels[:, :, 2, 2] = 0                                             # a pixel that votes for nothing
    return index, score, labels, P.label_vote(index, score, labels, P.inv_tau32(TAU), Kv)


def decided(soft, Kv):
    """Pixels whose oracle label the tolerance cannot change: the top value clear of the second."""
    Cl = soft.shape[0]
    if Cl == 1:
        return np.ones(soft.shape[1:], bool)
    top2 = np.sort(soft, axis=0)[-2:]
    return top2[1] - top2[0] > 2 * tol(Kv) * top2[1]


@pytest.mark.parametrize("M,K,Kv,S,Cl", SHAPES, ids=lambda v: str(v))
def test_the_oracle_leaves_at_most_one_percent_of_the_labels_undecided(M, K, Kv, S, Cl):
    index, score, labels, (soft, label, conf, source) = case(M, K, Kv, S, Cl)
    have = label >= 0
    assert (~have).sum() >= 3 and not have[0, :3].any() and (source[:, 0, :3] == -1).all()
    assert (~decided(soft, Kv) & have).sum() <= 0.01 * S * S
    assert (source >= 0).sum(axis=0).max() == Kv and 0 < ((source >= 0).sum(axis=0) < Kv).sum()
    live = source[source >= 0]
    assert live.max() < M * S * S and (soft >= 0).all() and np.array_equal(conf, soft.max(axis=0))


@gpu
@pytest.mark.parametrize("M,K,Kv,S,Cl", SHAPES, ids=lambda v: str(v))
def test_label_vote_against_the_oracle(need_gpu, M, K, Kv, S, Cl):
    from stablekeypoints_amd import ops
    index, score, labels, (soft, label, conf, source) = case(M, K, Kv, S, Cl)
    dev = [torch.as_tensor(a, device=DEV) for a in (index, score, labels)]
    gs, gl, gc, gsrc = ops.label_vote(*dev, TAU, k=Kv, return_source=True)
    plain = ops.label_vote(*dev, TAU, k=Kv)
    torch.cuda.synchronize()
    assert (gs.dtype, gl.dtype, gc.dtype, gsrc.dtype) == (torch.float32, torch.int32, torch.float32, torch.int32)
    assert tuple(gs.shape) == (Cl, S, S) and tuple(gl.shape) == (S, S) and tuple(gc.shape) == (S, S)
    assert tuple(gsrc.shape) == (Kv, S, S) and len(plain) == 3
    for a, b in zip(plain, (gs, gl, gc)):                              # the same with and without source
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    gs, gl, gc, gsrc = (t.cpu().numpy() for t in (gs, gl, gc, gsrc))
    bad = np.argwhere(gsrc != source)
    assert not len(bad), (len(bad), bad[0].tolist(), gsrc[tuple(bad[0])], source[tuple(bad[0])])
    err = np.abs(gs.astype(np.float64) - soft)
    worst = float((err / np.maximum(soft, 1e-300)).max())
    print(f"M={M} K={K} Kv={Kv} S={S} Cl={Cl}: worst relative error of soft {worst / 2.0 ** -24:.2f} u, bound "
          f"{tol(Kv) / 2.0 ** -24:.0f} u")
    assert (err <= tol(Kv) * soft).all(), worst
    assert (np.abs(gc.astype(np.float64) - conf) <= tol(Kv) * conf).all()
    sure = decided(soft, Kv)
    assert np.array_equal(gl[sure], label[sure])
    assert np.array_equal(gl < 0, label < 0)                           # a pixel has a label exactly where it has a candidate
    assert (gs[:, 0, :3] == 0).all() and (gl[0, :3] == -1).all() and (gc[0, :3] == 0).all()
    top = gs.max(axis=0)
    have = gl >= 0
    assert np.array_equal(gc[have], top[have])                         # confidence is the device's own greatest value
    assert np.array_equal(gl[have], gs.argmax(axis=0)[have])           # ... at its lowest class


@gpu
def test_one_candidate_gives_back_its_label_bit_for_bit_and_kv_below_k_is_a_prefix(need_gpu):
    from stablekeypoints_amd import ops
    M, K, Kv, S, Cl = SHAPES[0]
    index, score, labels, _ = case(M, K, Kv, S, Cl)
    one_i, one_s = np.full_like(index, -1), np.full_like(score, -np.inf)
    one_i[M - 1, 2], one_s[M - 1, 2] = index[M - 1, 2].clip(0), 0.5
    dev = [torch.as_tensor(a, device=DEV) for a in (one_i, one_s, labels)]
    soft, label, conf, source = ops.label_vote(*dev, TAU, return_source=True)
    q = torch.as_tensor(one_i[M - 1, 2].astype(np.int64), device=DEV).reshape(-1)
    want = dev[2][M - 1].reshape(Cl, S * S)[:, q].reshape(Cl, S, S)
    assert torch.equal(soft, want) and torch.equal(conf, want.max(dim=0).values)
    assert torch.equal(source[0].long().reshape(-1), (M - 1) * S * S + q) and bool((source[1:] == -1).all())
    full = [torch.as_tensor(a, device=DEV) for a in (index, score, labels)]
    long_src = ops.label_vote(*full, TAU, k=K, return_source=True)[3]
    short_src = ops.label_vote(*full, TAU, k=2, return_source=True)[3]
    assert torch.equal(long_src[:2], short_src)


@gpu
def test_argument_errors_name_the_argument(need_gpu):
    from stablekeypoints_amd import ops
    i = torch.zeros(2, 5, 8, 8, dtype=torch.int32, device=DEV)
    s, l = torch.zeros(2, 5, 8, 8, device=DEV), torch.zeros(2, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="index must be"):
        ops.label_vote(i.long(), s, l, TAU)
    with pytest.raises(ValueError, match="score must be"):
        ops.label_vote(i, s[:, :4], l, TAU)
    with pytest.raises(ValueError, match="labels must be"):
        ops.label_vote(i, s, l[:1], TAU)
    with pytest.raises(ValueError, match="labels must be contiguous"):
        ops.label_vote(i, s, torch.zeros(2, 3, 8, 16, device=DEV)[..., ::2], TAU)
    with pytest.raises(ValueError, match="k must be"):
        ops.label_vote(i, s, l, TAU, k=6)
    with pytest.raises(ValueError, match="tau must be"):
        ops.label_vote(i, s, l, 0.0)
    with pytest.raises(ValueError, match="M in"):
        ops.label_vote(i.repeat(40, 1, 1, 1), s.repeat(40, 1, 1, 1), l.repeat(40, 1, 1, 1), TAU)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.label_vote(i.cpu(), s, l, TAU)
