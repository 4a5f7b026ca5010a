"""CPU-side checks of the convolution entry points' argument validation: every call below fails a
check before anything is launched (aligned dummy pointers, no GPU needed), and ``skp_last_error()``
names the entry point and the first failing check."""
import ctypes
import os

import pytest

A = 256   # an aligned non-null dummy address; 260 is 4-byte but not 16-byte (or 8-byte) aligned

# argument names of each entry point, in call order (include/skp.h)
SIGNATURES = {
    "skp_conv3x3_wino": "x U bias residual y B C K H W nsplit ws stream",
    "skp_conv3x3_wino2": "x U bias residual y B C K H W nsplit ws stream",
    "skp_conv3x3_wino2_gn": "x U bias residual y B C K H W nsplit ws gn_part stream",
    "skp_conv3x3_wino2_v": "x U bias residual y B C K H W nsplit ws stream",
    "skp_conv3x3_wino2_v_gn": "x U bias residual y B C K H W nsplit ws gn_part stream",
    "skp_conv3x3s2_f2": "x U bias y B C K H W nsplit ws stream",
    "skp_wino2_vtransform": "x V B C H W stream",
    "skp_wino2_vtransform_gn": "x stats gamma beta shift G act V B C H W stream",
    "skp_wino_weights": "w K C flip U stream",
    "skp_wino2_weights": "w K C flip U stream",
    "skp_wino2s2_weights": "w K C U stream",
}
POINTERS = {"x", "U", "V", "w", "y", "bias", "residual", "ws", "gn_part", "stats", "gamma", "beta", "shift"}
# a call every entry point accepts (for the V-staged entries ``x`` is V); each row overrides some of it
GOOD = dict(x=A, U=A, V=A, w=A, y=A, bias=None, residual=None, ws=None, gn_part=None, stream=None, stats=A, gamma=A,
            beta=A, shift=None, G=8, act=1, flip=0, B=4, C=64, K=64, H=32, W=32, nsplit=1)

# (entry point, overrides of GOOD, skp_last_error() of the rejected call)
REJECTED = [
    ("skp_conv3x3_wino", dict(x=None), "skp_conv3x3_wino: null pointer"),
    ("skp_conv3x3_wino", dict(y=None), "skp_conv3x3_wino: null pointer"),
    ("skp_conv3x3_wino", dict(B=0), "skp_conv3x3_wino: non-positive shape"),
    ("skp_conv3x3_wino", dict(W=0), "skp_conv3x3_wino: non-positive shape"),
    ("skp_conv3x3_wino", dict(C=6), "skp_conv3x3_wino: input channels must be a multiple of 4"),
    ("skp_conv3x3_wino", dict(K=0), "skp_conv3x3_wino: non-positive shape"),
    ("skp_conv3x3_wino", dict(K=48), "skp_conv3x3_wino: output channels must be a multiple of 32"),
    ("skp_conv3x3_wino", dict(H=18), "skp_conv3x3_wino: H and W must be multiples of 4"),
    ("skp_conv3x3_wino", dict(nsplit=0), "skp_conv3x3_wino: nsplit must divide C into multiples of 4"),
    ("skp_conv3x3_wino", dict(nsplit=3, ws=256), "skp_conv3x3_wino: nsplit must divide C into multiples of 4"),
    ("skp_conv3x3_wino", dict(nsplit=2), "skp_conv3x3_wino: split-K needs a workspace of nsplit·B·K·H·W floats"),
    ("skp_conv3x3_wino", dict(x=260), "skp_conv3x3_wino: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino", dict(U=260), "skp_conv3x3_wino: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino", dict(y=260), "skp_conv3x3_wino: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino", dict(nsplit=2, ws=260), "skp_conv3x3_wino: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino", dict(residual=260), "skp_conv3x3_wino: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino", dict(B=8, C=512, H=512, W=512), "skp_conv3x3_wino: input larger than 2 GiB (32-bit buffer offsets)"),
    ("skp_conv3x3_wino2", dict(x=None), "skp_conv3x3_wino2_gn: null pointer"),
    ("skp_conv3x3_wino2", dict(K=48), "skp_conv3x3_wino2_gn: output channels must be a multiple of 32"),
    ("skp_conv3x3_wino2", dict(nsplit=2), "skp_conv3x3_wino2_gn: split-K needs a workspace of nsplit·B·K·H·W floats"),
    ("skp_conv3x3_wino2_gn", dict(x=None), "skp_conv3x3_wino2_gn: null pointer"),
    ("skp_conv3x3_wino2_gn", dict(y=None), "skp_conv3x3_wino2_gn: null pointer"),
    ("skp_conv3x3_wino2_gn", dict(B=0), "skp_conv3x3_wino2_gn: non-positive shape"),
    ("skp_conv3x3_wino2_gn", dict(W=0), "skp_conv3x3_wino2_gn: non-positive shape"),
    ("skp_conv3x3_wino2_gn", dict(C=6), "skp_conv3x3_wino2_gn: input channels must be a multiple of 4"),
    ("skp_conv3x3_wino2_gn", dict(K=0), "skp_conv3x3_wino2_gn: non-positive shape"),
    ("skp_conv3x3_wino2_gn", dict(K=48), "skp_conv3x3_wino2_gn: output channels must be a multiple of 32"),
    ("skp_conv3x3_wino2_gn", dict(H=20), "skp_conv3x3_wino2_gn: H and W must be multiples of 32, or 16×16 with B a multiple of 4"),
    ("skp_conv3x3_wino2_gn", dict(W=48), "skp_conv3x3_wino2_gn: H and W must be multiples of 32, or 16×16 with B a multiple of 4"),
    ("skp_conv3x3_wino2_gn", dict(B=2, H=16, W=16), "skp_conv3x3_wino2_gn: H and W must be multiples of 32, or 16×16 with B a multiple of 4"),
    ("skp_conv3x3_wino2_gn", dict(nsplit=0), "skp_conv3x3_wino2_gn: nsplit must divide C into multiples of 4"),
    ("skp_conv3x3_wino2_gn", dict(nsplit=3, ws=256), "skp_conv3x3_wino2_gn: nsplit must divide C into multiples of 4"),
    ("skp_conv3x3_wino2_gn", dict(nsplit=2), "skp_conv3x3_wino2_gn: split-K needs a workspace of nsplit·B·K·H·W floats"),
    ("skp_conv3x3_wino2_gn", dict(x=260), "skp_conv3x3_wino2_gn: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino2_gn", dict(U=260), "skp_conv3x3_wino2_gn: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino2_gn", dict(y=260), "skp_conv3x3_wino2_gn: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino2_gn", dict(nsplit=2, ws=260), "skp_conv3x3_wino2_gn: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino2_gn", dict(residual=260), "skp_conv3x3_wino2_gn: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino2_gn", dict(B=8, C=512, H=512, W=512), "skp_conv3x3_wino2_gn: input larger than 2 GiB (32-bit buffer offsets)"),
    ("skp_conv3x3_wino2_gn", dict(gn_part=256, nsplit=2, ws=256), "skp_conv3x3_wino2_gn: gn_part: one split, H and W multiples of 32, 8-byte aligned"),
    ("skp_conv3x3_wino2_gn", dict(gn_part=260), "skp_conv3x3_wino2_gn: gn_part: one split, H and W multiples of 32, 8-byte aligned"),
    ("skp_conv3x3_wino2_gn", dict(gn_part=256, B=4, H=16, W=16), "skp_conv3x3_wino2_gn: gn_part: one split, H and W multiples of 32, 8-byte aligned"),
    ("skp_conv3x3_wino2_v", dict(x=None), "skp_conv3x3_wino2_v_gn: null pointer"),
    ("skp_conv3x3_wino2_v", dict(K=48), "skp_conv3x3_wino2_v_gn: output channels must be a multiple of 32"),
    ("skp_conv3x3_wino2_v", dict(nsplit=2), "skp_conv3x3_wino2_v_gn: split-K needs a workspace of nsplit·B·K·H·W floats"),
    ("skp_conv3x3_wino2_v_gn", dict(x=None), "skp_conv3x3_wino2_v_gn: null pointer"),
    ("skp_conv3x3_wino2_v_gn", dict(y=None), "skp_conv3x3_wino2_v_gn: null pointer"),
    ("skp_conv3x3_wino2_v_gn", dict(B=0), "skp_conv3x3_wino2_v_gn: non-positive shape"),
    ("skp_conv3x3_wino2_v_gn", dict(W=0), "skp_conv3x3_wino2_v_gn: non-positive shape"),
    ("skp_conv3x3_wino2_v_gn", dict(C=6), "skp_conv3x3_wino2_v_gn: input channels must be a multiple of 4"),
    ("skp_conv3x3_wino2_v_gn", dict(K=0), "skp_conv3x3_wino2_v_gn: non-positive shape"),
    ("skp_conv3x3_wino2_v_gn", dict(K=48), "skp_conv3x3_wino2_v_gn: output channels must be a multiple of 32"),
    ("skp_conv3x3_wino2_v_gn", dict(H=20), "skp_conv3x3_wino2_v_gn: H and W must be multiples of 32"),
    ("skp_conv3x3_wino2_v_gn", dict(W=48), "skp_conv3x3_wino2_v_gn: H and W must be multiples of 32"),
    ("skp_conv3x3_wino2_v_gn", dict(B=2, H=16, W=16), "skp_conv3x3_wino2_v_gn: H and W must be multiples of 32"),
    ("skp_conv3x3_wino2_v_gn", dict(nsplit=0), "skp_conv3x3_wino2_v_gn: nsplit must divide C into multiples of 4"),
    ("skp_conv3x3_wino2_v_gn", dict(nsplit=3, ws=256), "skp_conv3x3_wino2_v_gn: nsplit must divide C into multiples of 4"),
    ("skp_conv3x3_wino2_v_gn", dict(nsplit=2), "skp_conv3x3_wino2_v_gn: split-K needs a workspace of nsplit·B·K·H·W floats"),
    ("skp_conv3x3_wino2_v_gn", dict(x=260), "skp_conv3x3_wino2_v_gn: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino2_v_gn", dict(U=260), "skp_conv3x3_wino2_v_gn: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino2_v_gn", dict(y=260), "skp_conv3x3_wino2_v_gn: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino2_v_gn", dict(nsplit=2, ws=260), "skp_conv3x3_wino2_v_gn: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino2_v_gn", dict(residual=260), "skp_conv3x3_wino2_v_gn: tensors must be 16-byte aligned"),
    ("skp_conv3x3_wino2_v_gn", dict(gn_part=256, nsplit=2, ws=256), "skp_conv3x3_wino2_v_gn: gn_part: one split, 8-byte aligned"),
    ("skp_conv3x3_wino2_v_gn", dict(gn_part=260), "skp_conv3x3_wino2_v_gn: gn_part: one split, 8-byte aligned"),
    ("skp_conv3x3s2_f2", dict(x=None), "skp_conv3x3s2_f2: null pointer"),
    ("skp_conv3x3s2_f2", dict(y=None), "skp_conv3x3s2_f2: null pointer"),
    ("skp_conv3x3s2_f2", dict(B=0), "skp_conv3x3s2_f2: non-positive shape"),
    ("skp_conv3x3s2_f2", dict(W=0), "skp_conv3x3s2_f2: non-positive shape"),
    ("skp_conv3x3s2_f2", dict(C=6), "skp_conv3x3s2_f2: input channels must be a multiple of 4"),
    ("skp_conv3x3s2_f2", dict(K=0), "skp_conv3x3s2_f2: non-positive shape"),
    ("skp_conv3x3s2_f2", dict(K=48), "skp_conv3x3s2_f2: output channels must be a multiple of 32"),
    ("skp_conv3x3s2_f2", dict(H=20), "skp_conv3x3s2_f2: H and W must be multiples of 32"),
    ("skp_conv3x3s2_f2", dict(W=48), "skp_conv3x3s2_f2: H and W must be multiples of 32"),
    ("skp_conv3x3s2_f2", dict(B=2, H=16, W=16), "skp_conv3x3s2_f2: H and W must be multiples of 32"),
    ("skp_conv3x3s2_f2", dict(nsplit=0), "skp_conv3x3s2_f2: nsplit must divide C into multiples of 4"),
    ("skp_conv3x3s2_f2", dict(nsplit=3, ws=256), "skp_conv3x3s2_f2: nsplit must divide C into multiples of 4"),
    ("skp_conv3x3s2_f2", dict(nsplit=2), "skp_conv3x3s2_f2: split-K needs a workspace of nsplit·B·K·(H/2)·(W/2) floats"),
    ("skp_conv3x3s2_f2", dict(x=260), "skp_conv3x3s2_f2: tensors must be 16-byte aligned"),
    ("skp_conv3x3s2_f2", dict(U=260), "skp_conv3x3s2_f2: tensors must be 16-byte aligned"),
    ("skp_conv3x3s2_f2", dict(y=260), "skp_conv3x3s2_f2: tensors must be 16-byte aligned"),
    ("skp_conv3x3s2_f2", dict(nsplit=2, ws=260), "skp_conv3x3s2_f2: tensors must be 16-byte aligned"),
    ("skp_conv3x3s2_f2", dict(B=8, C=512, H=512, W=512), "skp_conv3x3s2_f2: input larger than 2 GiB (32-bit buffer offsets)"),
    ("skp_wino2_vtransform", dict(x=None), "skp_wino2_vtransform: null pointer"),
    ("skp_wino2_vtransform", dict(B=0), "skp_wino2_vtransform: non-positive shape"),
    ("skp_wino2_vtransform", dict(W=0), "skp_wino2_vtransform: non-positive shape"),
    ("skp_wino2_vtransform", dict(C=6), "skp_wino2_vtransform: input channels must be a multiple of 4"),
    ("skp_wino2_vtransform", dict(H=20), "skp_wino2_vtransform: H and W must be multiples of 32"),
    ("skp_wino2_vtransform", dict(W=48), "skp_wino2_vtransform: H and W must be multiples of 32"),
    ("skp_wino2_vtransform", dict(B=2, H=16, W=16), "skp_wino2_vtransform: H and W must be multiples of 32"),
    ("skp_wino2_vtransform", dict(x=260), "skp_wino2_vtransform: tensors must be 16-byte aligned"),
    ("skp_wino2_vtransform", dict(V=260), "skp_wino2_vtransform: tensors must be 16-byte aligned"),
    ("skp_wino2_vtransform_gn", dict(x=None), "skp_wino2_vtransform_gn: null pointer"),
    ("skp_wino2_vtransform_gn", dict(stats=None), "skp_wino2_vtransform_gn: null pointer"),
    ("skp_wino2_vtransform_gn", dict(B=0), "skp_wino2_vtransform_gn: non-positive shape"),
    ("skp_wino2_vtransform_gn", dict(W=0), "skp_wino2_vtransform_gn: non-positive shape"),
    ("skp_wino2_vtransform_gn", dict(C=6), "skp_wino2_vtransform_gn: input channels must be a multiple of 4"),
    ("skp_wino2_vtransform_gn", dict(H=20), "skp_wino2_vtransform_gn: H and W must be multiples of 32"),
    ("skp_wino2_vtransform_gn", dict(W=48), "skp_wino2_vtransform_gn: H and W must be multiples of 32"),
    ("skp_wino2_vtransform_gn", dict(B=2, H=16, W=16), "skp_wino2_vtransform_gn: H and W must be multiples of 32"),
    ("skp_wino2_vtransform_gn", dict(G=0), "skp_wino2_vtransform_gn: C must be divisible by G"),
    ("skp_wino2_vtransform_gn", dict(G=24), "skp_wino2_vtransform_gn: C must be divisible by G"),
    ("skp_wino2_vtransform_gn", dict(x=260), "skp_wino2_vtransform_gn: tensors must be 16-byte aligned"),
    ("skp_wino2_vtransform_gn", dict(V=260), "skp_wino2_vtransform_gn: tensors must be 16-byte aligned"),
    ("skp_wino_weights", dict(w=None), "skp_wino_weights: null pointer"),
    ("skp_wino_weights", dict(U=None), "skp_wino_weights: null pointer"),
    ("skp_wino_weights", dict(K=0), "skp_wino_weights: non-positive shape"),
    ("skp_wino_weights", dict(C=0), "skp_wino_weights: non-positive shape"),
    ("skp_wino_weights", dict(K=48), "skp_wino_weights: output channels must be a multiple of 32"),
    ("skp_wino2_weights", dict(w=None), "skp_wino2_weights: null pointer"),
    ("skp_wino2_weights", dict(U=None), "skp_wino2_weights: null pointer"),
    ("skp_wino2_weights", dict(K=0), "skp_wino2_weights: non-positive shape"),
    ("skp_wino2_weights", dict(C=0), "skp_wino2_weights: non-positive shape"),
    ("skp_wino2_weights", dict(K=48), "skp_wino2_weights: output channels must be a multiple of 32"),
    ("skp_wino2s2_weights", dict(w=None), "skp_wino2s2_weights: null pointer"),
    ("skp_wino2s2_weights", dict(U=None), "skp_wino2s2_weights: null pointer"),
    ("skp_wino2s2_weights", dict(K=0), "skp_wino2s2_weights: non-positive shape"),
    ("skp_wino2s2_weights", dict(C=0), "skp_wino2s2_weights: non-positive shape"),
    ("skp_wino2s2_weights", dict(K=48), "skp_wino2s2_weights: output channels must be a multiple of 32"),
    # the first failing check names the error: null before shape, gn_part before shape, C before K
    ("skp_conv3x3_wino", dict(x=None, B=0), "skp_conv3x3_wino: null pointer"),
    ("skp_conv3x3_wino", dict(C=6, K=48), "skp_conv3x3_wino: input channels must be a multiple of 4"),
    ("skp_conv3x3_wino2_gn", dict(gn_part=260, C=6), "skp_conv3x3_wino2_gn: gn_part: one split, H and W multiples of 32, 8-byte aligned"),
    ("skp_conv3x3_wino2_v_gn", dict(gn_part=260, C=6), "skp_conv3x3_wino2_v_gn: gn_part: one split, 8-byte aligned"),
    ("skp_conv3x3s2_f2", dict(H=20, nsplit=3), "skp_conv3x3s2_f2: H and W must be multiples of 32"),
]


@pytest.fixture(scope="module")
def L():
    from stablekeypoints_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libskp.so not built (run __graft_entry__.build())")
    return _lib.lib()


@pytest.mark.parametrize("entry", sorted(SIGNATURES))
def test_bad_arguments_rejected_with_their_message(L, entry):
    rows = [r for r in REJECTED if r[0] == entry]
    assert rows
    for _, over, message in rows:
        kw = dict(GOOD, **over)
        args = [ctypes.c_void_p(kw[n]) if n in POINTERS and kw[n] is not None else kw[n]
                for n in SIGNATURES[entry].split()]
        rc = getattr(L, entry)(*args)
        got = L.skp_last_error().decode()
        assert rc == -1 and message in got, (entry, over, rc, got)


def test_every_entry_point_has_rows():
    assert {r[0] for r in REJECTED} == set(SIGNATURES)
