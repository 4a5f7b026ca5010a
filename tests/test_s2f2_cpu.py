"""The stride-2 minimal-product form behind skp_conv3x3s2_f2, stated in numpy: 2×2 output tiles at
input pitch 4, 25 products per tile and channel pair, with the matrices of include/skp.h.  Checked
against F.pad(x, (0, 1, 0, 1)) + conv2d(stride=2) in fp64 (no GPU needed)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

BT = np.array([[1, 0, -1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, -1], [0, 1, 0, 0, 0], [0, 0, 0, 1, 0]], np.float64)
G = np.array([[1, 0, 0], [1, 0, 1], [0, 0, 1], [0, 1, 0], [0, 1, 0]], np.float64)
AT = np.array([[1, 1, 0, 1, 0], [0, 1, -1, 0, 1]], np.float64)


def conv_s2_tiled(x, w):
    """x (C, H, W), w (K, C, 3, 3) → (K, H/2, W/2); H, W multiples of 4."""
    C, H, W = x.shape
    K = w.shape[0]
    xp = np.zeros((C, H + 1, W + 1))   # the (0, 1, 0, 1) pad: the row / column the kernel loads as zeros
    xp[:, :H, :W] = x
    U = np.einsum("ia,kcab,jb->kcij", G, w, G)              # (K, C, 5, 5)
    y = np.zeros((K, H // 2, W // 2))
    for ty in range(H // 4):
        for tx in range(W // 4):
            d = xp[:, 4 * ty:4 * ty + 5, 4 * tx:4 * tx + 5]
            V = np.einsum("ia,cab,jb->cij", BT, d, BT)      # (C, 5, 5)
            M = np.einsum("kcij,cij->kij", U, V)            # 25 products per (k, c)
            y[:, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = np.einsum("ri,kij,sj->krs", AT, M, AT)
    return y


@pytest.mark.parametrize("H,W", [(8, 8), (8, 12)])
def test_tiled_stride2_form_equals_padded_conv(H, W):
    rng = np.random.default_rng(H * 100 + W)
    C, K = 3, 2
    x = rng.standard_normal((C, H, W))
    # the last row and column 100× the interior: a wrong pad or an off-by-one at the right or
    # bottom edge cannot hide
    x[:, -1, :] *= 100.0
    x[:, :-1, -1] *= 100.0
    w = rng.standard_normal((K, C, 3, 3))
    ref = F.conv2d(F.pad(torch.from_numpy(x)[None], (0, 1, 0, 1)), torch.from_numpy(w), stride=2)[0].numpy()
    y = conv_s2_tiled(x, w)
    assert y.shape == ref.shape
    assert np.abs(y - ref).max() <= 1e-12


def test_one_dimensional_form_takes_five_products():
    """Two outputs at stride 2 from five inputs: F(2, 2) on the even inputs (3 products) and the
    middle tap on the odd ones (2)."""
    rng = np.random.default_rng(0)
    d, g = rng.standard_normal(5), rng.standard_normal(3)
    y = AT @ ((G @ g) * (BT @ d))
    assert np.allclose(y, [d[0:3] @ g, d[2:5] @ g], rtol=0, atol=1e-14)
    assert np.all(np.isin(BT, (-1, 0, 1)))
