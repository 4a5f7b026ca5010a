"""CPU-side checks of the part reduce and the predict stage's --part_maps (no GPU needed): the numpy
restatement tests/tta_parts_ref.py against torch on the CPU, the conditions its cases must keep
meeting, the parser, the alias, the argument checks and the workspace size of skp_tta_reduce_parts
through the C ABI, and eval.foreground_iou on hand-made arrays."""
import numpy as np
import pytest
import torch

import tta_abi
import tta_parts_ref
import tta_ref
from tta_parts_ref import CHUNKED_SHAPES, PARTS_SHAPES, parts_ref


def _avg64(shape):
    maps, theta, _ = tta_ref.make_case(shape, special=False)
    return tta_ref.tta_ref(maps, theta)[1]


@pytest.fixture(scope="module", params=CHUNKED_SHAPES, ids=lambda s: "B{}_C{}_n{}_S{}".format(*s))
def chunked(request):
    """One chunked shape's float64 average of the GPU tests' (special) inputs, computed once."""
    maps, theta, _ = tta_ref.make_case(request.param)
    return dict(shape=request.param, avg=tta_ref.tta_ref(maps, theta)[1])


@pytest.mark.parametrize("shape", PARTS_SHAPES, ids=lambda s: "B{}_C{}_n{}_S{}".format(*s))
def test_parts_ref_matches_torch(shape):
    avg = _avg64(shape)
    label, value, mass = parts_ref(avg)
    assert label.dtype == np.int16 and value.dtype == np.float64 and mass.dtype == np.float64
    tv, ti = torch.from_numpy(avg).max(dim=1)
    assert np.array_equal(value, tv.numpy())
    # torch.max leaves the index among equal maxima open: the values there must be the maximum, and ours the first
    assert np.array_equal(np.take_along_axis(avg, ti.numpy()[:, None], 1)[:, 0], value)
    first = (avg == value[:, None]).argmax(axis=1)
    assert np.array_equal(label, first)
    want = torch.from_numpy(avg).sum(dim=1).numpy()
    err = float(np.abs(mass - want).max())
    bound = avg.shape[1] * 2.0 ** -52 * float(np.abs(avg).sum(axis=1).max())    # a sum of n float64 terms, reordered
    print(f"{shape}: max |chunk-ordered mass - float64 sum| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # in fp32 the restatement keeps the array's dtype
    l32, v32, m32 = parts_ref(avg.astype(np.float32))
    assert v32.dtype == np.float32 and m32.dtype == np.float32 and l32.dtype == np.int16


def test_parts_ref_by_hand():
    avg = np.zeros((1, 12, 1, 2), np.float32)
    avg[0, :, 0, 0] = [1, 3, 3, 0, 0, 0, 0, 0, 0, 0, 3, 2]                    # tied across the chunks: the first wins
    avg[0, :, 0, 1] = [2.0 ** 24, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1]            # the order shows in fp32
    label, value, mass = parts_ref(avg)
    assert label.tolist() == [[[1, 0]]] and value.tolist() == [[[3.0, 2.0 ** 24]]]
    assert mass[0, 0, 0] == 12.0
    assert mass[0, 0, 1] == 2.0 ** 24 + 2.0          # chunk 0 rounds 2^24 + 1 + 1 to 2^24, chunk 1 holds 2
    assert tta_parts_ref.sequential_mass(avg)[0, 0, 1] == 2.0 ** 24
    assert parts_ref(avg[:, :10])[2][0, 0, 1] == tta_parts_ref.sequential_mass(avg[:, :10])[0, 0, 1]
    nothing = parts_ref(np.zeros((2, 3, 4, 4), np.float32))
    assert not nothing[0].any() and not nothing[1].any() and not nothing[2].any()
    low = parts_ref(np.full((1, 3, 2, 2), -np.inf, np.float32))
    assert not low[0].any() and np.isneginf(low[1]).all()


def test_pass_of():
    assert tta_parts_ref.pass_of(np.arange(29), 29)[0].tolist() == [0] * 10 + [1] * 10 + [2] * 8 + [3]
    assert tta_parts_ref.pass_of(np.arange(26), 26)[0].tolist() == [0] * 10 + [1] * 10 + [2] * 4 + [3] * 2
    assert tta_parts_ref.pass_of(np.arange(5), 5) [1] == 2 and tta_parts_ref.pass_of(np.arange(10), 10)[1] == 1


def test_cases_exercise_ties_and_the_carry(chunked):
    """The chunked cases keep exercising the tie rule and the carry across passes: tied maxima in
    different passes at more than 1 % of the pixels, and winners in every pass."""
    st = tta_parts_ref.tie_statistics(chunked["avg"])
    print(chunked["shape"], st)
    assert st["passes"] == 4
    assert st["across"] > 0.01
    assert st["winners"] == set(range(st["passes"]))


def test_cases_tell_the_chunked_mass_from_the_sequential(chunked):
    a32 = chunked["avg"].astype(np.float32)
    differ = float((parts_ref(a32)[2] != tta_parts_ref.sequential_mass(a32)).mean())
    print(chunked["shape"], "chunk-ordered mass differs from the sequential sum at", differ, "of the pixels")
    assert differ > 0.1


def test_parser_part_maps(capsys):
    from stablekeypoints_amd.main import build_parser, main
    p = build_parser()
    a = p.parse_args([])
    assert a.part_maps is False and a.part_size == 128 and a.part_tokens == "indices" and a.part_threshold == 0.0
    a = p.parse_args(["--start_from_stage", "predict", "--part_maps", "--part_size", "64", "--part_tokens", "all",
                      "--part_threshold", "0.25"])
    assert a.part_maps and a.part_size == 64 and a.part_tokens == "all" and a.part_threshold == 0.25
    with pytest.raises(SystemExit):
        p.parse_args(["--part_tokens", "some"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        main(["--part_maps"])
    assert "--part_maps belongs to --start_from_stage predict" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main(["--start_from_stage", "predict", "--part_maps", "--part_size", "1"])
    assert "--part_size must be at least 2" in capsys.readouterr().err


def test_part_maps_is_reachable_through_the_reference_names():
    import stablekeypoints_amd.eval as ev
    import unsupervised_keypoints.eval as ref_ev
    assert ref_ev.part_maps is ev.part_maps and ref_ev.foreground_iou is ev.foreground_iou
    assert ref_ev.PartMaps is ev.PartMaps and ev.PartMaps._fields == ("label", "value", "mass", "points", "area")


def test_ops_tta_reduce_parts_refuses_cpu_tensors():
    from stablekeypoints_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tta_reduce_parts(torch.zeros(1, 1, 1, 4, 4), torch.zeros(1, 1, 2, 3))


def test_byte_model():
    from stablekeypoints_amd import ops
    B, C, n, S = 4, 10, 10, 512
    assert ops.tta_reduce_parts_bytes(B, C, n, S) == 4 * B * C * n * S * S + 10 * B * S * S
    assert ops.tta_reduce_parts_bytes(B, C, n, S, avg=True) == 4 * B * C * n * S * S + 10 * B * S * S + 4 * B * n * S * S
    B, C, n, S = 4, 10, 500, 128
    Q = B * 50 * S * S
    assert ops.tta_reduce_parts_bytes(B, C, n, S) == 4 * B * C * n * S * S + 10 * B * S * S + 20 * Q
    assert ops.tta_reduce_parts_bytes(1, 2, 11, 8) == 4 * 2 * 11 * 64 + 10 * 64 + 20 * 2 * 64


_library = tta_abi.library


def test_tta_reduce_parts_rejects_bad_arguments_without_gpu():
    """The token bound and the workspace query; the checks every reduce shares are in tests/test_tta_cpu.py."""
    L = _library()
    # the label is int16
    assert tta_abi.rc_with(L, "skp_tta_reduce_parts", a1=1, a2=1, a3=32768, a4=2) == -1
    assert b"32767 tokens" in L.skp_last_error()
    assert L.skp_tta_reduce_parts_workspace(0, 1, 8) == -1 and L.skp_tta_reduce_parts_workspace(1, 1, -3) == -1
    assert L.skp_tta_reduce_parts_workspace(1, 0, 8) == -1 and L.skp_tta_reduce_parts_workspace(1, 1, 1) == -1
    # 2^31 bytes: 20 chunks of 4096² pixels are 10 · 20 · 2^24 bytes of partials
    assert L.skp_tta_reduce_parts_workspace(1, 200, 4096) == -1
    assert L.skp_tta_reduce_parts_workspace(1, 10, 4096) == 8 * 10 * 64 * 1024


@pytest.mark.parametrize("B,n,S", [(1, 1, 2), (2, 5, 37), (1, 10, 512), (1, 29, 37), (4, 500, 128)])
def test_parts_workspace_equals_its_closed_form(B, n, S):
    """skp_tta_reduce's partials and, with more than one chunk of 10 tokens, two floats and an int16
    per image, chunk and pixel, each array rounded up to 8 bytes."""
    L = _library()
    T = -(-S // 64) * -(-S // 4)
    chunks = -(-n // 10)
    Q = B * chunks * S * S
    r8 = lambda x: (x + 7) // 8 * 8
    assert L.skp_tta_reduce_parts_workspace(B, n, S) == 8 * B * n * T + (2 * r8(4 * Q) + r8(2 * Q) if chunks > 1 else 0)


def test_foreground_iou():
    from stablekeypoints_amd.eval import foreground_iou
    label = torch.full((5, 4, 4), -1, dtype=torch.int16)
    mask = torch.zeros(5, 4, 4)
    label[0, :2] = 3                 # identical
    mask[0, :2] = 1.0
    label[1, :2] = 0                 # disjoint
    mask[1, 2:] = 1.0
    #                                  image 2: both empty
    label[3, :2] = 1                 # half of the mask's pixels, and none outside it
    mask[3] = 1.0
    label[4, :, :3] = 2              # 12 labelled, 8 in the mask, 6 in both
    mask[4, :2] = 0.75
    mask[4, 2:] = 0.5                # 0.5 is not foreground
    iou = foreground_iou(label, mask)
    assert iou.dtype == torch.float64 and iou.shape == (5,)
    assert iou.tolist() == [1.0, 0.0, 1.0, 0.5, 6.0 / 14.0]
    # a trailing singleton axis, and a numpy mask
    assert torch.equal(foreground_iou(label, mask[..., None]), iou)
    assert torch.equal(foreground_iou(label, mask[..., None].numpy()), iou)
    # a mask of another size is resized to the labels' by nearest neighbour
    big = mask.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(foreground_iou(label, big), iou)
    assert torch.equal(foreground_iou(label, big[..., None]), iou)
    small = torch.zeros(1, 2, 2)
    small[0, 0] = 1.0                # the top half
    assert foreground_iou(label[:1], small).tolist() == [1.0]
    with pytest.raises(ValueError):
        foreground_iou(label, mask[:2])
