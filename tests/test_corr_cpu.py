"""CPU-side checks of the correspondence selection (no GPU needed): the numpy restatement
tests/corr_ref.py against the reference's recorded outputs (tests/golden/corresponding_points.npz), the
conditions under which a ranking means something, the one-pass merged entropy formula that
skp_tta_reduce_entropy implements, its argument checks through the C ABI, and the parser."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

import corr_ref
import tta_abi

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corresponding_points.npz"))
IDS = ["x".join(map(str, s)) for s in corr_ref.CASES]


@pytest.mark.parametrize("shape", corr_ref.CASES, ids=IDS)
def test_corresponding_ref_is_the_reference(shape):
    tag = "x".join(map(str, shape))
    points, indices, total = corr_ref.corresponding_ref(corr_ref.planted_average(shape), corr_ref.K)
    assert indices.dtype == np.int64 and np.array_equal(indices, GOLDEN[f"{tag}_indices"])
    assert points.dtype == np.float32 and np.array_equal(points, GOLDEN[f"{tag}_points"])
    # the reference sums fp32 entropies; measured: within 3.4e-6 of the float64 sums on these cases
    assert np.abs(total - GOLDEN[f"{tag}_entropy"]).max() < 1e-5


@pytest.mark.parametrize("shape", corr_ref.CASES, ids=IDS)
def test_the_ranking_is_no_rounding_accident(shape):
    """On the float64 restatement: every adjacent gap of the sorted summed entropies is at least 1e-3
    (measured: 2.1e-2, 3.4e-3 and 1.7e-2 at the least; the fp32 sums are within 3.4e-6), and no softmax
    probability is below 2^-23, so the reference's clamp of the probabilities is inactive (measured:
    1.4e-4 at the least)."""
    avg = corr_ref.planted_average(shape)
    total = corr_ref.sum_in_order(corr_ref.entropy_ref(avg))
    gaps = np.diff(np.sort(total))
    print("smallest gap", gaps.min())
    assert gaps.min() >= 1e-3
    z = avg.astype(np.float64).reshape(avg.shape[0], avg.shape[1], -1)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    print("smallest probability", p.min())
    assert p.min() >= 2.0 ** -23


def _add(s0, t, mk, sk, tk, m, scale):
    """A partial (sk, tk) about mk enters sums about m >= mk (entropy_add of skp_tta.hip)."""
    if not mk > -math.inf:
        return s0, t
    with np.errstate(invalid="ignore"):
        d = np.float64(scale) * (np.float64(mk) - np.float64(m))
        r = np.exp(d)
    if r == 0.0:
        return s0, t
    return s0 + sk * r, t + (tk + d * sk) * r


def one_pass(plane, scale, cuts):
    """H = log S0 − T / S0 of a flat float32 plane, its pixels split at ``cuts`` into tiles: each tile
    summed about its own maximum, the tiles merged about the plane's."""
    parts = []
    for tile in np.split(np.asarray(plane, np.float32).reshape(-1), cuts):
        if tile.size == 0:
            continue
        mk = tile.max()
        with np.errstate(invalid="ignore"):
            d = np.float64(scale) * (tile.astype(np.float64) - np.float64(mk))
            d = np.where(tile > -np.inf, d, -np.inf)      # a −inf pixel: e = 0 whatever the maximum
            e = np.exp(d)
            t = np.where(e == 0.0, 0.0, d * e)
        parts.append((mk, e.sum(), t.sum()))
    m = max(p[0] for p in parts)
    s0 = t = np.float64(0.0)
    for mk, sk, tk in parts:
        s0, t = _add(s0, t, mk, sk, tk, m, scale)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.log(s0) - t / s0


@pytest.mark.parametrize("scale", (1.0, 7.5))
def test_one_pass_merged_entropy_is_the_direct_entropy(scale):
    g = np.random.default_rng(3)
    for shape in corr_ref.CASES:
        avg = corr_ref.planted_average(shape)
        S = shape[3]
        for plane in avg.reshape(-1, S, S)[::5]:
            cuts = np.sort(g.choice(np.arange(1, S * S), size=int(g.integers(0, 40)), replace=False))
            assert abs(one_pass(plane, scale, cuts) - corr_ref.entropy_ref(plane, scale)) < 1e-12
    wide = (g.standard_normal((64, 64)) * 40).astype(np.float32)      # tiles whose e^{d} underflows to 0
    assert abs(one_pass(wide, scale, [7, 100, 2048, 4000]) - corr_ref.entropy_ref(wide, scale)) < 1e-12


def test_one_pass_degenerate_planes():
    for S in (2, 37, 64):
        zeros = np.zeros((S, S), np.float32)
        assert abs(one_pass(zeros, 1.0, [S, 3 * S]) - math.log(S * S)) < 1e-12
        assert abs(corr_ref.entropy_ref(zeros, 7.5) - math.log(S * S)) < 1e-12
    plane = np.zeros((8, 8), np.float32)
    plane[2, 3] = -np.inf                                 # probability 0: the entropy is that of the 31 zeros
    plane[4:, :] = -np.inf
    assert abs(one_pass(plane, 1.0, [16, 40]) - math.log(31)) < 1e-12      # the tile [40, 64) holds only −inf
    assert abs(corr_ref.entropy_ref(plane) - math.log(31)) < 1e-12
    plane = np.zeros((8, 8), np.float32)
    plane[5, 5] = np.inf
    assert np.isnan(one_pass(plane, 1.0, [16, 40])) and np.isnan(corr_ref.entropy_ref(plane))


def test_ops_tta_reduce_entropy_refuses_cpu_tensors():
    from stablekeypoints_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tta_reduce_entropy(torch.zeros(1, 1, 1, 4, 4), torch.zeros(1, 1, 2, 3))
    assert ops.tta_reduce_entropy_bytes(1, 10, 500, 128) >= ops.tta_reduce_bytes(1, 10, 500, 128)


def test_tta_reduce_entropy_rejects_bad_arguments_without_gpu():
    """The scale and the workspace query; the checks every reduce shares are in tests/test_tta_cpu.py."""
    L = tta_abi.library()
    for bad in (0.0, -1.0, float("nan"), float("inf")):     # slot 6 of skp_tta_reduce_entropy
        assert tta_abi.rc_with(L, "skp_tta_reduce_entropy", a6=bad) == -1 and b"scale" in L.skp_last_error()
    # the workspace query: skp_tta_reduce's partials and two doubles per image, token and tile
    for B, n, S in ((1, 500, 128), (4, 500, 128), (1, 10, 512), (2, 5, 37), (1, 1, 2)):
        got = L.skp_tta_reduce_entropy_workspace(B, n, S)
        assert got >= L.skp_tta_reduce_workspace(B, n, S) > 0 and got % 8 == 0
    assert L.skp_tta_reduce_entropy_workspace(1, 500, 128) == 500 * (2 * 32) * (8 + 16)
    for bad in ((0, 1, 8), (1, 0, 8), (1, 1, -3), (1, 1, 1), (1 << 20, 1 << 10, 8)):
        assert L.skp_tta_reduce_entropy_workspace(*bad) == -1


def test_existing_tta_kernels_compile_to_what_they_did():
    """profiles/tta_entropy_resources.txt (tools/kernel_resources.py at the parent and at this tree): every
    kernel of the parent keeps its row, and the kernels the entropy reduce adds use no scratch."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                        "tta_entropy_resources.txt")
    tables = open(path).read().split("== ")[1:]
    assert len(tables) == 2
    rows = [{ln.split()[0]: ln.split()[1:] for ln in t.splitlines()[2:] if ln.strip()} for t in tables]
    head = tables[1].splitlines()[1].split()
    assert head == tables[0].splitlines()[1].split() and head[0] == "kernel"
    parent, new = rows
    assert len(parent) == 7 and all(new[k] == v for k, v in parent.items())
    added = sorted(set(new) - set(parent))
    assert added == ["tta_merge_kernel<(Variant)3>", "tta_tile_entropy_kernel"]
    for k in added:
        assert new[k][head.index("scratch_B") - 1] == "0"
    assert int(new["tta_tile_entropy_kernel"][head.index("waves_per_SIMD") - 1]) >= 4


def test_cli_correspond_flags(monkeypatch, capsys):
    from stablekeypoints_amd import main as cli, optimize_token

    def no_model(*a, **k):
        raise AssertionError("the model was built")

    monkeypatch.setattr(optimize_token, "load_ldm", no_model)
    args = cli.build_parser().parse_args([])
    assert args.correspond is False and args.correspond_size == 128 and args.entropy_scale == 1.0
    args = cli.build_parser().parse_args(["--start_from_stage", "predict", "--correspond", "--correspond_size", "64",
                                          "--entropy_scale", "2.5"])
    assert args.correspond is True and args.correspond_size == 64 and args.entropy_scale == 2.5
    base = ["--model_type", "tiny", "--dataset_name", "synthetic"]
    for bad, word in ((["--correspond"], "--correspond"),
                      (["--start_from_stage", "evaluate", "--correspond"], "--correspond"),
                      (["--start_from_stage", "predict", "--correspond", "--entropy_scale", "0"], "--entropy_scale"),
                      (["--start_from_stage", "predict", "--correspond", "--entropy_scale", "-1"], "--entropy_scale"),
                      (["--start_from_stage", "predict", "--correspond", "--entropy_scale", "nan"], "--entropy_scale"),
                      (["--start_from_stage", "predict", "--correspond", "--correspond_size", "1"],
                       "--correspond_size")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + bad)
        assert e.value.code not in (0, None)
        assert word in capsys.readouterr().err
    assert cli.STAGES == ("optimize", "find_indices", "precompute", "evaluate")
    stage = next(a for a in cli.build_parser()._actions if a.dest == "start_from_stage")
    assert list(stage.choices) == list(cli.STAGES) + ["predict"]


def test_find_corresponding_points_signature_and_alias():
    import stablekeypoints_amd.eval as ev
    import unsupervised_keypoints.eval as alias
    assert alias.find_corresponding_points is ev.find_corresponding_points
    params = inspect.signature(alias.find_corresponding_points).parameters
    assert list(params) == ["maps", "num_points"] and params["num_points"].default == 10
    assert ev.Correspondences._fields == ("indices", "points", "entropy", "image_entropy")
    assert alias.correspond_images is ev.correspond_images
    params = inspect.signature(ev.correspond_images).parameters
    assert params["num_points"].default == 10 and params["candidates"].default is None
    assert params["upscale_size"].default == 128 and params["entropy_scale"].default == 1.0
