"""skp_tta_reduce_parts / ops.tta_reduce_parts, eval.part_maps and the CLI's predict stage with
--part_maps on the GPU.

The kernel's pos and avg are held to ops.tta_reduce bit for bit, and its label, value and mass, bit
for bit too, to the numpy restatement tests/tta_parts_ref.py applied to that average read back: the
average is the parent's kernel, not the code under test, and the restatement's first-occurrence
argmax and chunk-ordered fp32 sum are the contract's.  tests/test_tta_parts_cpu.py asserts that the
chunked cases hold tied maxima in different passes at more than 1 % of their pixels and winners in
every pass, and that the chunk-ordered sum differs from the sequential one on them.  Against the
float64 restatement tests/tta_ref.py, value and mass stay within twice the error the numpy
composition on the parent's average shows (the rule of tests/test_gpu_tta.py); labels are not
compared there, ties make them ill-conditioned.
"""
import numpy as np
import pytest
import torch

import tta_parts_ref
import tta_ref
import tta_tiny
from tta_parts_ref import PARTS_SHAPES, parts_ref
from tta_tiny import (DEV, N_TOK, S_UP, bits as _bits, cli as _cli, part_maps as _part_maps, same_bits as _same,
                      tiny)  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ------------------------------------------------------------------------------------------ the kernel
@pytest.fixture(scope="module", params=PARTS_SHAPES, ids=lambda s: "B{}_C{}_n{}_S{}".format(*s))
def case(request):
    """One shape's inputs, the plain reduce, the part reduce with and without the average, and the
    references, computed once and left unchanged."""
    from stablekeypoints_amd import ops
    shape = request.param
    maps_np, theta_np, finite = tta_ref.make_case(shape)
    maps, theta = torch.from_numpy(maps_np).to(DEV), torch.from_numpy(theta_np).to(DEV)
    plain_pos, plain_avg = ops.tta_reduce(maps, theta, return_avg=True)
    got = ops.tta_reduce_parts(maps, theta, return_avg=True)
    got_noavg = ops.tta_reduce_parts(maps, theta)
    # the finite tokens alone (the others' maps zeroed), for the float64 comparison
    fin_np = np.where(finite[:, None, :, None, None], maps_np, 0.0).astype(np.float32)
    fin = torch.from_numpy(fin_np).to(DEV)
    fin_avg = ops.tta_reduce(fin, theta, return_avg=True)[1]
    fin_got = ops.tta_reduce_parts(fin, theta)
    torch.cuda.synchronize()
    return dict(shape=shape, maps=maps, theta=theta, plain_pos=plain_pos, plain_avg=plain_avg, got=got,
                got_noavg=got_noavg, ref=parts_ref(plain_avg.cpu().numpy()), fin_ref=parts_ref(fin_avg.cpu().numpy()),
                fin_got=fin_got, ref64=parts_ref(tta_ref.tta_ref(fin_np, theta_np)[1]))


def test_pos_and_avg_are_tta_reduce_s(case):
    B, C, n, S = case["shape"]
    pos, label, value, mass, avg = case["got"]
    assert pos.shape == (B, n, 2) and avg.shape == (B, n, S, S)
    assert label.shape == (B, S, S) and label.dtype == torch.int16
    assert value.shape == (B, S, S) and value.dtype == torch.float32
    assert mass.shape == (B, S, S) and mass.dtype == torch.float32
    assert torch.equal(_bits(pos), _bits(case["plain_pos"]))
    assert torch.equal(_bits(avg), _bits(case["plain_avg"]))


def test_label_value_mass_are_the_restatement_on_the_average(case):
    _, label, value, mass, _ = case["got"]
    want_label, want_value, want_mass = case["ref"]
    assert want_value.dtype == np.float32 and want_mass.dtype == np.float32
    assert not np.isnan(want_value).any()
    print(case["shape"], "labels differ at", int((label.cpu().numpy() != want_label).sum()), "values at",
          int((value.cpu().numpy() != want_value).sum()), "masses at",
          int((mass.cpu().numpy().view(np.int32) != want_mass.view(np.int32)).sum()), "pixels")
    assert _same(value, want_value)
    assert _same(label, want_label)
    assert _same(mass, want_mass)


def test_results_do_not_depend_on_return_avg(case):
    assert case["got_noavg"][-1] is None
    for a, b in zip(case["got"][:4], case["got_noavg"][:4]):
        assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def test_workspace_reuse_after_another_shape(case):
    from stablekeypoints_amd import ops
    other = PARTS_SHAPES[-1] if case["shape"] != PARTS_SHAPES[-1] else PARTS_SHAPES[1]
    maps_np, theta_np, _ = tta_ref.make_case(other, seed=1)
    ops.tta_reduce_parts(torch.from_numpy(maps_np).to(DEV), torch.from_numpy(theta_np).to(DEV))
    again = ops.tta_reduce_parts(case["maps"], case["theta"])
    for a, b in zip(case["got"][:4], again[:4]):
        assert torch.equal(_bits(a), _bits(b))


def test_degenerate_cases(case):
    B, C, n, S = case["shape"]
    _, label, value, mass, avg = case["got"]
    if case["shape"] == tta_ref.ALL_OUT_OF_VIEW:     # the last image: every copy out of view
        assert (avg[-1] == 0).all()
        assert (label[-1] == 0).all() and (value[-1] == 0).all() and (mass[-1] == 0).all()
    if n == 1:
        assert (label == 0).all()
        assert torch.equal(_bits(value), _bits(avg[:, 0])) and torch.equal(_bits(mass), _bits(avg[:, 0]))
    assert int(label.min()) >= 0 and int(label.max()) < n


def test_against_float64_restatement(case):
    """value and mass of the finite tokens within twice the largest error the numpy restatement on
    the parent's average shows against the float64 one on the same inputs."""
    _, _, value, mass, _ = case["fin_got"]
    _, own_value, own_mass = case["fin_ref"]
    _, ref_value, ref_mass = case["ref64"]
    for name, got, own, ref in (("value", value, own_value, ref_value), ("mass", mass, own_mass, ref_mass)):
        own_err = float(np.abs(own.astype(np.float64) - ref).max())
        got_err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
        print(f"{case['shape']} {name}: numpy on the average vs float64 {own_err:.3e}, skp_tta_reduce_parts vs "
              f"float64 {got_err:.3e}")
        assert got_err <= 2 * own_err


def test_tta_reduce_parts_rejects_bad_shapes():
    from stablekeypoints_amd import ops
    m, th = torch.zeros(1, 2, 1, 8, 8, device=DEV), torch.zeros(1, 2, 2, 3, device=DEV)
    with pytest.raises(ValueError, match="theta_inv"):
        ops.tta_reduce_parts(m, torch.zeros(1, 3, 2, 3, device=DEV))
    with pytest.raises(ValueError, match="maps must be"):
        ops.tta_reduce_parts(torch.zeros(1, 2, 1, 8, 4, device=DEV), th)
    with pytest.raises(ValueError, match="maps must be"):
        ops.tta_reduce_parts(torch.zeros(2, 1, 8, 8, device=DEV), th)
    with pytest.raises(ValueError, match="32767"):
        ops.tta_reduce_parts(torch.zeros(1, 1, 32768, 2, 2, device=DEV), torch.zeros(1, 1, 2, 3, device=DEV))
    with pytest.raises(ValueError, match="bad shape"):
        ops.tta_reduce_parts(torch.zeros(1, 1, 1, 1, 1, device=DEV), torch.zeros(1, 1, 2, 3, device=DEV))


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("every", [False, True], ids=["five_indices", "all_tokens"])
def test_part_maps_tiny(tiny, every):
    """The five indices are one chunk of tokens, the whole context (n = 16) two."""
    from stablekeypoints_amd import eval as ev
    M, S = 2, S_UP
    indices = None if every else tiny[4]
    n = N_TOK if every else len(tiny[4])
    parts = _part_maps(tiny, indices)
    assert isinstance(parts, ev.PartMaps)
    assert parts.label.shape == (M, S, S) and parts.label.dtype == torch.int16
    assert parts.value.shape == (M, S, S) and parts.value.dtype == torch.float32
    assert parts.mass.shape == (M, S, S) and parts.mass.dtype == torch.float32
    assert parts.points.shape == (M, n, 2) and parts.points.dtype == torch.float32
    assert parts.area.shape == (M, n) and parts.area.dtype == torch.int64
    assert int(parts.label.min()) >= -1 and int(parts.label.max()) < n
    assert torch.equal(parts.area.sum(1), (parts.label >= 0).flatten(1).sum(1))
    for t in range(n):
        assert torch.equal(parts.area[:, t], (parts.label == t).flatten(1).sum(1))
    assert torch.equal(parts.label < 0, parts.mass <= 0)
    assert int(parts.area.sum()) > 0
    # the points are predict_keypoints', and the maps the restatement on its averages
    model = tiny[:4] + (torch.arange(N_TOK) if every else tiny[4],)
    kp, maps = tta_tiny.predict(model, tiny[2], augmentation_iterations=3, image_batch=2, return_maps=True)
    assert torch.equal(parts.points, kp)
    label, value, mass = parts_ref(maps.cpu().numpy())
    assert _same(parts.value, value) and _same(parts.mass, mass)
    assert _same(parts.label, np.where(mass <= 0, np.int16(-1), label).astype(np.int16))
    # a second call from the same seed gives the same bits
    again = _part_maps(tiny, indices)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(parts, again))
    # a threshold no pixel's mass reaches: everything is background
    none = _part_maps(tiny, indices, part_threshold=1e30)
    assert (none.label == -1).all() and (none.area == 0).all()
    assert torch.equal(_bits(none.mass), _bits(parts.mass)) and torch.equal(_bits(none.value), _bits(parts.value))
    assert torch.equal(none.points, parts.points)


def test_part_maps_refuses_a_process_group(tiny, monkeypatch):
    from stablekeypoints_amd import optimize
    monkeypatch.setattr(optimize, "_world", lambda: (2, 0))
    with pytest.raises(ValueError, match="single process"):
        _part_maps(tiny, tiny[4])


def _part_files(folder, M, n, S):
    lab = torch.load(folder / "part_labels.pt", weights_only=True)
    mass = torch.load(folder / "part_mass.pt", weights_only=True)
    area = torch.load(folder / "part_area.pt", weights_only=True)
    pts = torch.load(folder / "part_points.pt", weights_only=True)
    assert lab.shape == (M, S, S) and lab.dtype == torch.int16
    assert mass.shape == (M, S, S) and mass.dtype == torch.float32
    assert area.shape == (M, n) and area.dtype == torch.int64
    assert pts.shape == (M, n, 2) and pts.dtype == torch.float32 and ((pts > 0) & (pts < 1)).all()
    assert int(lab.min()) >= -1 and int(lab.max()) < n
    assert torch.equal(area.sum(1), (lab >= 0).flatten(1).sum(1)) and int(area.sum()) > 0
    assert torch.equal(lab < 0, mass <= 0)
    assert not (folder / "part_fg_iou.pt").exists()     # the synthetic dataset has no mask
    return lab


def test_cli_part_maps_tiny(tmp_path):
    from PIL import Image
    from stablekeypoints_amd import ops
    plain = tmp_path / "plain"
    kp_plain = _cli(plain)
    assert not (plain / "part_labels.pt").exists() and not (plain / "parts.png").exists()
    out = tmp_path / "parts"
    kp = _cli(out, "--part_maps", "--part_size", "64", "--visualize")
    assert torch.equal(kp.view(torch.int32), kp_plain.view(torch.int32))
    assert open(plain / "keypoints.csv").read() == open(out / "keypoints.csv").read()
    _part_files(out, 5, 5, 64)
    sheet = Image.open(out / "parts.png")
    assert sheet.size[::-1] == ops.sheet_shape(512, 512, 1, 5, downscale=2)
    assert np.asarray(sheet).std() > 0


def test_cli_part_tokens_all_tiny(tmp_path):
    out = tmp_path / "all"
    kp = _cli(out, "--part_maps", "--part_size", "64", "--part_tokens", "all")
    assert kp.shape == (5, 5, 2)
    lab = _part_files(out, 5, N_TOK, 64)
    assert 5 <= int(lab.max()) <= N_TOK - 1      # tokens beyond the five indices own pixels
    assert not (out / "parts.png").exists()
