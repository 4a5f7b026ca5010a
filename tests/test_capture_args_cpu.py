"""CPU-side checks of the capture entry points' argument validation and of the sparse backward's
workspace query: every call below fails a check before anything is launched (aligned dummy
pointers, no GPU needed), and ``skp_last_error()`` is the entry point's name and the first failing
check."""
import ctypes
import os

import pytest

A = 256   # an aligned non-null dummy address; 260 is 4-byte but not 16-byte aligned
A4, S4 = (A, A, A, A), (16, 16, 16, 32)

# argument names of each entry point, in call order (include/skp.h)
SIGNATURES = {
    "skp_capture_fwd": "z BH s N R attn stats1 stream",
    "skp_capture_bwd": "z BH s N R dattn group sb sp sn gscale stats1 dz ws stream",
    "skp_capture_maps_fwd": "zs sizes L B H N R maps statsL stream",
    "skp_capture_maps_bwd": "zs sizes L B H N R dmaps gscale statsL dzs ws stream",
    "skp_capture_maps_bwd_sel": "zs sizes L B H N R tok K gsel gscale statsL dzs ws stream",
    "skp_aggregate": "zs L BH RR N idx n_out out stream",
    "skp_resize_bilinear": "x C R Ro out stream",
    "skp_resize_bilinear_bwd": "x C R Ro out stream",
}
POINTERS = {"z", "attn", "stats1", "dattn", "dz", "ws", "maps", "dmaps", "tok", "gsel", "idx", "out", "x"}
POINTER_ARRAYS = {"zs", "statsL", "dzs"}   # one address per layer
# a call every entry point accepts; each row overrides some of it
GOOD = dict(z=A, attn=A, stats1=None, dattn=A, dz=A, ws=A, maps=A, dmaps=A, tok=A, gsel=A, idx=None, out=A, x=A,
            stream=None, zs=A4, statsL=A4, dzs=A4, sizes=S4, L=4, B=8, H=8, BH=64, s=16, N=500, R=128, RR=128 * 128,
            K=10, group=1, sb=128 * 128 * 500, sp=500, sn=1, gscale=1.0, n_out=500, C=4, Ro=256)

NULL, SHAPE, LRANGE = "null pointer", "non-positive shape", "L out of range"
NMAX = "N > 1024 tokens is not supported"
NULL_LAYER, LAYER_SIZE = "null layer pointer", "layer size must be in [1, R]"
Z_ALIGN, ZDZ_ALIGN = "z_low pointers must be 16-B aligned", "z_low / dz_low pointers must be 16-B aligned"
WS_ALIGN, TOO_LARGE = "workspace must be 16-B aligned", "shape too large"
first = lambda v, a=A4: (v,) + a[1:]   # noqa: E731  (a fault in the first layer)
last = lambda v, a=A4: a[:-1] + (v,)   # noqa: E731  (… in the last layer)

# (entry point, overrides of GOOD, the check that rejects the call): one row per SKP_CHECK_ARG,
# in each entry point's order of checks.  Not reachable from outside, so without a row:
# skp_capture_maps_bwd's "R * N too large for LDS" (R, N <= 1024 always fit) and the second half of
# its "shape too large" (B·H <= 65535 and R <= 1024 keep B·H·R below 2^31); skp_capture_maps_bwd_sel's
# "memset failed" and "internal: no sel_dense kernel for this shape" (after the first device call).
REJECTED = [
    ("skp_capture_fwd", dict(z=None), NULL),
    ("skp_capture_fwd", dict(attn=None), NULL),
    ("skp_capture_fwd", dict(BH=0), SHAPE),
    ("skp_capture_fwd", dict(s=0), SHAPE),
    ("skp_capture_fwd", dict(R=0), SHAPE),
    ("skp_capture_fwd", dict(N=0), SHAPE),
    ("skp_capture_fwd", dict(N=1025), NMAX),
    # s · (quads per lane) <= 160: the rows at N = 257 and 513 fail only with 2 and 4 quads per lane
    ("skp_capture_fwd", dict(N=256, s=161), "s*N too large for LDS"),
    ("skp_capture_fwd", dict(N=257, s=81), "s*N too large for LDS"),
    ("skp_capture_fwd", dict(N=513, s=41), "s*N too large for LDS"),
    ("skp_capture_fwd", dict(N=1024, s=41), "s*N too large for LDS"),
    ("skp_capture_bwd", dict(z=None), NULL),
    ("skp_capture_bwd", dict(dattn=None), NULL),
    ("skp_capture_bwd", dict(dz=None), NULL),
    ("skp_capture_bwd", dict(ws=None), NULL),
    ("skp_capture_bwd", dict(group=0), "group must be >= 1"),
    ("skp_capture_bwd", dict(BH=0), SHAPE),
    ("skp_capture_bwd", dict(s=0), SHAPE),
    ("skp_capture_bwd", dict(R=0), SHAPE),
    ("skp_capture_bwd", dict(N=0), SHAPE),
    ("skp_capture_bwd", dict(R=1025), "R > 1024 is not supported"),
    ("skp_capture_bwd", dict(BH=65536), "BH > 65535"),
    ("skp_capture_bwd", dict(N=1025), NMAX),
    # (s + 1) · Np + 5·R + 4 <= 40960 floats at the smallest chunk, Np = 512 · (tokens per thread):
    # the row at N = 513 fails only with 2 tokens per thread
    ("skp_capture_bwd", dict(N=512, s=78), "s*N too large for LDS"),
    ("skp_capture_bwd", dict(N=513, s=39), "s*N too large for LDS"),
    ("skp_capture_bwd", dict(N=1024, s=64), "s*N too large for LDS"),
    ("skp_capture_maps_fwd", dict(zs=None), NULL),
    ("skp_capture_maps_fwd", dict(sizes=None), NULL),
    ("skp_capture_maps_fwd", dict(maps=None), NULL),
    ("skp_capture_maps_fwd", dict(L=0), LRANGE),
    ("skp_capture_maps_fwd", dict(L=17), LRANGE),
    ("skp_capture_maps_fwd", dict(B=0), SHAPE),
    ("skp_capture_maps_fwd", dict(H=0), SHAPE),
    ("skp_capture_maps_fwd", dict(N=0), SHAPE),
    ("skp_capture_maps_fwd", dict(R=0), SHAPE),
    ("skp_capture_maps_fwd", dict(R=16385), TOO_LARGE),
    ("skp_capture_maps_fwd", dict(H=8192), TOO_LARGE),
    ("skp_capture_maps_fwd", dict(N=1025), NMAX),
    ("skp_capture_maps_fwd", dict(zs=first(None)), NULL_LAYER),
    ("skp_capture_maps_fwd", dict(zs=last(None)), NULL_LAYER),
    ("skp_capture_maps_fwd", dict(sizes=first(0, S4)), LAYER_SIZE),
    ("skp_capture_maps_fwd", dict(sizes=last(129, S4)), LAYER_SIZE),
    ("skp_capture_maps_fwd", dict(zs=first(260)), Z_ALIGN),
    ("skp_capture_maps_fwd", dict(zs=last(260)), Z_ALIGN),
    ("skp_capture_maps_fwd", dict(sizes=(128,) * 4, N=1024), "s*N too large for LDS"),
    ("skp_capture_maps_bwd", dict(zs=None), NULL),
    ("skp_capture_maps_bwd", dict(sizes=None), NULL),
    ("skp_capture_maps_bwd", dict(dmaps=None), NULL),
    ("skp_capture_maps_bwd", dict(dzs=None), NULL),
    ("skp_capture_maps_bwd", dict(ws=None), NULL),
    ("skp_capture_maps_bwd", dict(L=0), LRANGE),
    ("skp_capture_maps_bwd", dict(L=17), LRANGE),
    ("skp_capture_maps_bwd", dict(B=0), SHAPE),
    ("skp_capture_maps_bwd", dict(H=0), SHAPE),
    ("skp_capture_maps_bwd", dict(N=0), SHAPE),
    ("skp_capture_maps_bwd", dict(R=0), SHAPE),
    ("skp_capture_maps_bwd", dict(N=502), "N must be a multiple of 4 (use skp_capture_bwd)"),
    ("skp_capture_maps_bwd", dict(N=1028), NMAX),
    ("skp_capture_maps_bwd", dict(R=1028), "R > 1024 is not supported (capture_bwd_cols_kernel tap tables)"),
    ("skp_capture_maps_bwd", dict(H=8192), TOO_LARGE),
    ("skp_capture_maps_bwd", dict(ws=260), WS_ALIGN),
    ("skp_capture_maps_bwd", dict(zs=first(None)), NULL_LAYER),
    ("skp_capture_maps_bwd", dict(zs=last(None)), NULL_LAYER),
    ("skp_capture_maps_bwd", dict(dzs=first(None)), NULL_LAYER),
    ("skp_capture_maps_bwd", dict(dzs=last(None)), NULL_LAYER),
    ("skp_capture_maps_bwd", dict(sizes=first(0, S4)), LAYER_SIZE),
    ("skp_capture_maps_bwd", dict(sizes=last(129, S4)), LAYER_SIZE),
    ("skp_capture_maps_bwd", dict(zs=first(260)), Z_ALIGN),
    ("skp_capture_maps_bwd", dict(zs=last(260)), Z_ALIGN),
    ("skp_capture_maps_bwd_sel", dict(zs=None), NULL),
    ("skp_capture_maps_bwd_sel", dict(sizes=None), NULL),
    ("skp_capture_maps_bwd_sel", dict(tok=None), NULL),
    ("skp_capture_maps_bwd_sel", dict(gsel=None), NULL),
    ("skp_capture_maps_bwd_sel", dict(statsL=None), NULL),
    ("skp_capture_maps_bwd_sel", dict(dzs=None), NULL),
    ("skp_capture_maps_bwd_sel", dict(ws=None), NULL),
    ("skp_capture_maps_bwd_sel", dict(L=0), LRANGE),
    ("skp_capture_maps_bwd_sel", dict(L=17), LRANGE),
    ("skp_capture_maps_bwd_sel", dict(B=0), SHAPE),
    ("skp_capture_maps_bwd_sel", dict(H=0), SHAPE),
    ("skp_capture_maps_bwd_sel", dict(N=0), SHAPE),
    ("skp_capture_maps_bwd_sel", dict(R=0), SHAPE),
    ("skp_capture_maps_bwd_sel", dict(R=126), "R must be a multiple of 4"),
    ("skp_capture_maps_bwd_sel", dict(K=0), "K must be in [1, 32]"),
    ("skp_capture_maps_bwd_sel", dict(K=33), "K must be in [1, 32]"),
    ("skp_capture_maps_bwd_sel", dict(N=502), "N must be a multiple of 4, at most 1024"),
    ("skp_capture_maps_bwd_sel", dict(N=1028), "N must be a multiple of 4, at most 1024"),
    ("skp_capture_maps_bwd_sel", dict(H=8192), TOO_LARGE),
    ("skp_capture_maps_bwd_sel", dict(R=5796), TOO_LARGE),
    ("skp_capture_maps_bwd_sel", dict(ws=260), WS_ALIGN),
    ("skp_capture_maps_bwd_sel", dict(zs=first(None)), NULL_LAYER),
    ("skp_capture_maps_bwd_sel", dict(zs=last(None)), NULL_LAYER),
    ("skp_capture_maps_bwd_sel", dict(dzs=first(None)), NULL_LAYER),
    ("skp_capture_maps_bwd_sel", dict(dzs=last(None)), NULL_LAYER),
    ("skp_capture_maps_bwd_sel", dict(statsL=first(None)), NULL_LAYER),
    ("skp_capture_maps_bwd_sel", dict(statsL=last(None)), NULL_LAYER),
    ("skp_capture_maps_bwd_sel", dict(sizes=first(0, S4)), LAYER_SIZE),
    ("skp_capture_maps_bwd_sel", dict(sizes=last(129, S4)), LAYER_SIZE),
    ("skp_capture_maps_bwd_sel", dict(zs=first(260)), ZDZ_ALIGN),
    ("skp_capture_maps_bwd_sel", dict(zs=last(260)), ZDZ_ALIGN),
    ("skp_capture_maps_bwd_sel", dict(dzs=first(260)), ZDZ_ALIGN),
    ("skp_capture_maps_bwd_sel", dict(dzs=last(260)), ZDZ_ALIGN),
    ("skp_aggregate", dict(zs=None), NULL),
    ("skp_aggregate", dict(out=None), NULL),
    ("skp_aggregate", dict(L=0), LRANGE),
    ("skp_aggregate", dict(L=17), LRANGE),
    ("skp_aggregate", dict(BH=0), SHAPE),
    ("skp_aggregate", dict(RR=0), SHAPE),
    ("skp_aggregate", dict(N=0), SHAPE),
    ("skp_aggregate", dict(zs=first(None)), NULL_LAYER),
    ("skp_aggregate", dict(zs=last(None)), NULL_LAYER),
    ("skp_aggregate", dict(idx=A, n_out=0), "n_out must be positive with indices"),
    ("skp_resize_bilinear", dict(x=None), NULL),
    ("skp_resize_bilinear", dict(out=None), NULL),
    ("skp_resize_bilinear", dict(C=0), SHAPE),
    ("skp_resize_bilinear", dict(R=0), SHAPE),
    ("skp_resize_bilinear", dict(Ro=0), SHAPE),
    ("skp_resize_bilinear_bwd", dict(x=None), NULL),
    ("skp_resize_bilinear_bwd", dict(out=None), NULL),
    ("skp_resize_bilinear_bwd", dict(C=0), SHAPE),
    ("skp_resize_bilinear_bwd", dict(R=0), SHAPE),
    ("skp_resize_bilinear_bwd", dict(Ro=0), SHAPE),
    # two faults: the first failing check names the error
    ("skp_capture_fwd", dict(z=None, BH=0), NULL),
    ("skp_capture_fwd", dict(N=1025, s=200), NMAX),
    ("skp_capture_bwd", dict(z=None, group=0), NULL),
    ("skp_capture_bwd", dict(group=0, BH=0), "group must be >= 1"),
    ("skp_capture_bwd", dict(R=1025, BH=0), SHAPE),
    ("skp_capture_bwd", dict(BH=65536, N=1025), "BH > 65535"),
    ("skp_capture_maps_fwd", dict(L=0, B=0), LRANGE),
    ("skp_capture_maps_fwd", dict(H=8192, N=1025), TOO_LARGE),
    ("skp_capture_maps_fwd", dict(N=1025, zs=first(None)), NMAX),
    # the forward judges the alignment after its layer loop, the two backwards inside it
    ("skp_capture_maps_fwd", dict(zs=(260, A, A, None)), NULL_LAYER),
    ("skp_capture_maps_fwd", dict(zs=first(260), sizes=last(0, S4)), LAYER_SIZE),
    ("skp_capture_maps_fwd", dict(zs=first(None), sizes=first(0, S4)), NULL_LAYER),
    ("skp_capture_maps_fwd", dict(zs=last(None), sizes=first(0, S4)), LAYER_SIZE),
    ("skp_capture_maps_fwd", dict(zs=first(260), sizes=(128,) * 4, N=1024), Z_ALIGN),
    ("skp_capture_maps_bwd", dict(N=502, R=1028), "N must be a multiple of 4 (use skp_capture_bwd)"),
    ("skp_capture_maps_bwd", dict(R=1028, H=8192), "R > 1024 is not supported (capture_bwd_cols_kernel tap tables)"),
    ("skp_capture_maps_bwd", dict(H=8192, ws=260), TOO_LARGE),
    ("skp_capture_maps_bwd", dict(ws=260, zs=first(None)), WS_ALIGN),
    ("skp_capture_maps_bwd", dict(zs=(260, A, A, None)), Z_ALIGN),
    ("skp_capture_maps_bwd", dict(zs=last(260), sizes=first(0, S4)), LAYER_SIZE),
    ("skp_capture_maps_bwd", dict(zs=first(260), sizes=first(0, S4)), LAYER_SIZE),
    ("skp_capture_maps_bwd", dict(dzs=first(None), sizes=first(0, S4)), NULL_LAYER),
    ("skp_capture_maps_bwd_sel", dict(R=126, K=0), "R must be a multiple of 4"),
    ("skp_capture_maps_bwd_sel", dict(K=33, N=502), "K must be in [1, 32]"),
    ("skp_capture_maps_bwd_sel", dict(N=502, H=8192), "N must be a multiple of 4, at most 1024"),
    ("skp_capture_maps_bwd_sel", dict(ws=260, statsL=first(None)), WS_ALIGN),
    ("skp_capture_maps_bwd_sel", dict(zs=(260, A, A, None)), ZDZ_ALIGN),
    ("skp_capture_maps_bwd_sel", dict(dzs=first(260), statsL=first(None)), NULL_LAYER),
    ("skp_capture_maps_bwd_sel", dict(dzs=first(260), sizes=first(129, S4)), LAYER_SIZE),
    ("skp_aggregate", dict(zs=first(None), idx=A, n_out=0), NULL_LAYER),
    ("skp_aggregate", dict(L=17, N=0), LRANGE),
    ("skp_resize_bilinear", dict(x=None, C=0), NULL),
    ("skp_resize_bilinear_bwd", dict(out=None, Ro=0), NULL),
]


@pytest.fixture(scope="module")
def L():
    from stablekeypoints_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libskp.so not built (run __graft_entry__.build())")
    return _lib.lib()


def c_arg(name, v):
    if v is None:
        return None
    if name in POINTERS:
        return ctypes.c_void_p(v)
    if name in POINTER_ARRAYS:
        return ctypes.cast((ctypes.c_void_p * len(v))(*v), ctypes.POINTER(ctypes.c_void_p))
    if name == "sizes":
        return (ctypes.c_int * len(v))(*v)
    return v


@pytest.mark.parametrize("entry,over,message", REJECTED, ids=[f"{e}-{o}" for e, o, _ in REJECTED])
def test_bad_arguments_rejected_with_their_message(L, entry, over, message):
    kw = dict(GOOD, **over)
    rc = getattr(L, entry)(*[c_arg(n, kw[n]) for n in SIGNATURES[entry].split()])
    got = L.skp_last_error().decode()
    assert rc == -1 and got == f"{entry}: {message}", (rc, got)


def test_every_entry_point_has_rows():
    assert {r[0] for r in REJECTED} == set(SIGNATURES)


# ------------------------------------------------ skp_capture_maps_bwd_sel_workspace (floats)
def sel_workspace(L, sizes, B, H, N, R, K, n_layers=None):
    arr = None if sizes is None else (ctypes.c_int * len(sizes))(*sizes)
    return L.skp_capture_maps_bwd_sel_workspace(arr, len(sizes) if n_layers is None else n_layers, B, H, N, R, K)


def fast_floats(sizes, B, H, R, K):
    """zsel (the K selected logits of every layer, rounded up to 4 floats), sel_doth's Hs rows, the
    per-pixel (mb, d) pairs and es, the last three with the widest layer's pitch."""
    BH, smax, nl = B * H, max(sizes), len(sizes)
    r4 = lambda n: (n + 3) // 4 * 4   # noqa: E731
    return (r4(sum(BH * s * s * K for s in sizes)) + r4(nl * BH * K * R * smax) + nl * BH * R * R * 2
            + nl * BH * K * smax * smax)


def fallback_floats(sizes, B, H, N, R):
    """the dense (B, N, R²) gradient, skp_capture_maps_bwd's workspace behind it, 4 floats of slack."""
    from stablekeypoints_amd import ops
    return B * N * R * R + ops.capture_maps_bwd_ws_floats(B, H, N, R, sizes) + 4


def test_sel_workspace_closed_forms(L):
    assert sel_workspace(L, S4, 8, 8, 500, 128, 10) == fast_floats(S4, 8, 8, 128, 10) == 22642688
    assert sel_workspace(L, (5, 3), 2, 3, 36, 40, 4) == fallback_floats((5, 3), 2, 3, 36, 40) == 273604
    # the dense backward's share of it: the pixel-major gradient and the widest layer's row partials
    assert fallback_floats((5, 3), 2, 3, 36, 40) - 2 * 36 * 40 * 40 - 4 == 2 * 40 * 40 * 36 + 2 * 3 * 40 * 5 * 36


def test_sel_workspace_path_per_shape(L):
    """The fast path's size wherever a sel_dense kernel is compiled for every layer, the fallback's
    elsewhere (an odd N, a ratio R/s outside {4, 8, 16}, R > 256, one layer without a kernel)."""
    for R, s in [(128, 16), (128, 32), (128, 8), (64, 16), (64, 8), (64, 4), (32, 8), (32, 4)]:
        assert sel_workspace(L, (s,), 2, 3, 36, R, 17) == fast_floats((s,), 2, 3, R, 17), (R, s)
        assert sel_workspace(L, (s, s, s), 1, 2, 8, R, 3) == fast_floats((s, s, s), 1, 2, R, 3), (R, s)
    assert sel_workspace(L, (32, 16), 2, 2, 8, 128, 2) == fast_floats((32, 16), 2, 2, 128, 2)
    assert sel_workspace(L, S4, 8, 8, 501, 128, 10) == fallback_floats(S4, 8, 8, 501, 128)
    for R, sizes in [(128, (4,)), (128, (64,)), (64, (32,)), (32, (16,)), (32, (2,)), (16, (4,)), (512, (32,)),
                     (256, (16,)), (128, (16, 16, 24)), (128, (5, 16)), (40, (10,))]:
        assert sel_workspace(L, sizes, 2, 3, 36, R, 4) == fallback_floats(sizes, 2, 3, 36, R), (R, sizes)


def test_sel_workspace_refuses_bad_shapes(L):
    good = dict(sizes=S4, B=8, H=8, N=500, R=128, K=10)
    assert sel_workspace(L, **good) > 0
    for over in (dict(sizes=None), dict(B=0), dict(H=0), dict(N=0), dict(R=0), dict(K=0), dict(B=-1), dict(K=-3)):
        kw = dict(good, **over)
        n = 4 if kw["sizes"] is None else None
        assert sel_workspace(L, kw.pop("sizes"), n_layers=n, **kw) == -1, over
    assert sel_workspace(L, S4, 8, 8, 500, 128, 10, n_layers=0) == -1
    assert sel_workspace(L, S4 * 5, 8, 8, 500, 128, 10, n_layers=17) == -1
    assert sel_workspace(L, S4 * 4, 8, 8, 500, 128, 10) == fast_floats(S4 * 4, 8, 8, 128, 10)   # L = 16
