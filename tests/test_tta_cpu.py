"""CPU-side checks of the TTA reduce and the predict stage (no GPU needed): the float64
restatement tests/tta_ref.py against torch-CPU float64, the parser, and the argument checks of
skp_tta_reduce through the C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tta_abi
import tta_ref


def _torch_composition(maps, theta):
    """Σ_c grid_sample(maps) / Σ_c grid_sample(ones), NaN -> 0, in torch-CPU float64."""
    B, C, n, S, _ = maps.shape
    m = torch.from_numpy(maps).double()
    th = torch.from_numpy(theta).double()
    avg = torch.zeros(B, n, S, S, dtype=torch.float64)
    for b in range(B):
        grid = F.affine_grid(th[b], (C, n, S, S), align_corners=False)
        kw = dict(mode="bilinear", padding_mode="zeros", align_corners=False)
        tot = F.grid_sample(m[b], grid, **kw).sum(0)
        num = F.grid_sample(torch.ones_like(m[b]), grid, **kw).sum(0)
        a = tot / num
        a[a != a] = 0
        avg[b] = a
    return avg.numpy()


@pytest.mark.parametrize("S", [37, 64])
def test_tta_ref_matches_torch_float64(S):
    maps, theta, _ = tta_ref.make_case((2, 3, 2, S), special=False)
    pos, avg, _ = tta_ref.tta_ref(maps, theta)
    ref = _torch_composition(maps, theta)
    d = float(np.abs(avg - ref).max())
    print(f"S={S}: max |tta_ref - torch float64| = {d:.3e}")
    assert d <= 1e-12
    idx = avg.reshape(2, 2, -1).argmax(-1)
    assert np.array_equal(pos, np.stack([idx // S + 0.5, idx % S + 0.5], -1))


def test_tta_ref_identity_single_copy_is_the_map():
    # continuous values: the maximum is unique by far more than the float64 rounding of the grid
    maps = np.random.default_rng(3).random((1, 1, 3, 37, 37)).astype(np.float32)
    theta =np.broadcast_to(tta_ref.IDENTITY, (1, 1, 2, 3)).copy()
    pos, avg, num = tta_ref.tta_ref(maps, theta)
    assert np.abs(avg[0] - maps[0, 0]).max() <= 1e-12
    assert np.abs(num - 1.0).max() <= 1e-12
    idx = maps[0, 0].reshape(3, -1).argmax(-1)
    assert np.array_equal(pos[0], np.stack([idx // 37 + 0.5, idx % 37 + 0.5], -1))


def test_tta_ref_degenerate_cases():
    """Every copy out of view: num = 0, avg = 0, pos = (0.5, 0.5); so does an all-zero map."""
    maps, theta, _ = tta_ref.make_case(tta_ref.ALL_OUT_OF_VIEW)
    pos, avg, num = tta_ref.tta_ref(maps, theta)
    assert (num[-1] == 0).all() and (avg[-1] == 0).all() and (pos[-1] == 0.5).all()
    assert (avg[0, 0] == 0).all() and (pos[0, 0] == 0.5).all()


def test_parser_predict_stage():
    from stablekeypoints_amd.main import build_parser, ranks_to_start
    p = build_parser()
    assert p.parse_args(["--start_from_stage", "predict"]).start_from_stage == "predict"
    action = next(a for a in p._actions if a.dest == "start_from_stage")
    assert list(action.choices) == ["optimize", "find_indices", "precompute", "evaluate", "predict"]
    assert action.default == "optimize"
    # predict runs in one process on --device: no ranks, whatever is visible or asked for
    assert ranks_to_start(p.parse_args(["--start_from_stage", "predict"]), visible=8, env=None) == 1
    assert ranks_to_start(p.parse_args(["--start_from_stage", "predict", "--num_gpus", "4"]), visible=8, env=None) == 1
    assert ranks_to_start(p.parse_args(["--start_from_stage", "evaluate"]), visible=8, env=None) == 8


def test_predict_is_reachable_through_the_reference_names():
    import stablekeypoints_amd.eval as ev
    import unsupervised_keypoints.eval as ref_ev
    assert ref_ev.predict_keypoints is ev.predict_keypoints


def test_ops_tta_reduce_refuses_cpu_tensors():
    from stablekeypoints_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tta_reduce(torch.zeros(1, 1, 1, 4, 4), torch.zeros(1, 1, 2, 3))


@pytest.mark.parametrize("entry", list(tta_abi.ENTRY_POINTS))
def test_every_tta_reduce_rejects_bad_common_arguments_without_gpu(entry):
    """The checks that the five entry points share (check_common of skp_tta.hip), on each of them."""
    L = tta_abi.library()
    pointers = tta_abi.ENTRY_POINTS[entry][1]

    def rc_with(**kw):
        return tta_abi.rc_with(L, entry, **kw)

    for slot in pointers:       # maps, theta_inv, pos, the query's further outputs, workspace
        assert rc_with(**{f"a{slot}": None}) == -1 and b"null" in L.skp_last_error()
    for slot in (1, 2, 3, 4):   # B, C, n, S
        for bad in (0, -1):
            assert rc_with(**{f"a{slot}": bad}) == -1 and b"non-positive" in L.skp_last_error()
    assert rc_with(a4=1) == -1 and b"at least 2" in L.skp_last_error()
    assert rc_with(**{f"a{pointers[-1]}": ctypes.c_void_p(260)}) == -1 and b"aligned" in L.skp_last_error()
    # B·C·n·S² and the linear index must stay within int
    assert rc_with(a1=1, a2=1, a3=1, a4=46341) == -1 and b"2^31" in L.skp_last_error()
    assert rc_with(a1=8, a2=10, a3=10, a4=2048) == -1 and b"2^31" in L.skp_last_error()
    assert rc_with(a1=65536, a2=1, a3=1, a4=2) == -1 and b"65535 images" in L.skp_last_error()


def test_tta_reduce_rejects_bad_arguments_without_gpu():
    """The workspace query of skp_tta_reduce; its argument checks are the shared ones above."""
    L = tta_abi.library()
    # one (value, index) pair per image, token and 64 x 4-pixel tile
    assert L.skp_tta_reduce_workspace(1, 10, 512) == 10 * (8 * 128) * 8
    assert L.skp_tta_reduce_workspace(2, 5, 37) >= 2 * 5 * 8
    assert L.skp_tta_reduce_workspace(0, 1, 8) == -1 and L.skp_tta_reduce_workspace(1, 1, -3) == -1


@pytest.mark.parametrize("B,n,S", [(1, 1, 2), (2, 5, 37), (1, 10, 512), (4, 10, 512)])
def test_workspace_queries_equal_their_closed_forms(B, n, S):
    """The three layouts by value, T = ceil(S/64)·ceil(S/4) tiles per plane: a (value, index) pair per
    image, token and tile; scored adds a double per tile and 16 bytes per image and token; peaks
    adds an int per image, token and round, rounded up to 8 bytes."""
    from stablekeypoints_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libskp.so not built")
    L = _lib.lib()
    T = -(-S // 64) * -(-S // 4)
    assert L.skp_tta_reduce_workspace(B, n, S) == 8 * B * n * T
    assert L.skp_tta_reduce_scored_workspace(B, n, S) == B * n * (16 * T + 16)
    r2 = float(np.float32((0.05 * S) ** 2))
    for num in (1, 3, 16):
        assert L.skp_tta_reduce_peaks_workspace(B, n, S, num, r2) == 8 * B * n * T + (4 * B * n * num + 7) // 8 * 8
