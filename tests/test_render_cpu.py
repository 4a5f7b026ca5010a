"""CPU-side checks of the visualisation stage (A17): argument checks of skp_map_range /
skp_render_sheet before any HIP call, the colour and LUT defaults, the
``unsupervised_keypoints.visualize`` alias, the ``--visualize`` wiring of ``main`` and the
float32-vs-float64 self-agreement of the restatement on the GPU test's cases."""
import ctypes
import os

import numpy as np
import pytest
import torch

import render_ref as R


def _lib_or_skip():
    from stablekeypoints_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libskp.so not built")
    return _lib.lib()


def test_render_bad_arguments_rejected_without_gpu():
    L = _lib_or_skip()
    a = ctypes.c_void_p(256)   # aligned non-null dummy: every check below fails before any HIP call

    def sheet(images=a, n=5, H=16, W=16, maps=None, h=0, w=0, rng=None, lut=None, points=None, K=0, rows=2, cols=3,
              f=1, pad=1, out=a):
        return L.skp_render_sheet(images, n, H, W, maps, h, w, rng, lut, 0.7, points, K, 2.0, a, rows, cols, f, pad,
                                  out, None)

    assert sheet(images=None) == -1 and b"null" in L.skp_last_error()
    assert sheet(H=18, f=4) == -1 and b"multiple of f" in L.skp_last_error()
    assert sheet(n=7) == -1 and b"rows*cols" in L.skp_last_error()
    assert sheet(maps=a, h=8, w=8, rng=None, lut=a) == -1 and b"range" in L.skp_last_error()
    assert sheet(points=a, K=65) == -1 and b"64" in L.skp_last_error()
    assert sheet(H=1 << 15, W=1 << 15, n=1, rows=1, cols=1) == -1 and b"2^31" in L.skp_last_error()
    assert L.skp_map_range(None, 2, 4, 4, a, None) == -1 and b"null" in L.skp_last_error()
    assert L.skp_map_range(a, 2, 0, 4, a, None) == -1 and b"shape" in L.skp_last_error()


def test_render_sheet_refuses_cpu_tensors():
    from stablekeypoints_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.render_sheet(torch.zeros(1, 3, 8, 8), rows=1, cols=1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.map_range(torch.zeros(1, 8, 8))


@pytest.mark.parametrize("K", [3, 10, 30])
def test_default_colors_are_distinct(K):
    from stablekeypoints_amd import ops
    c = ops.default_colors(K)
    assert c.dtype == torch.uint8 and tuple(c.shape) == (K, 3)
    assert len({tuple(row) for row in c.tolist()}) == K


def test_luts_are_256x3_in_unit_range():
    from stablekeypoints_amd import ops
    for lut in (ops.fallback_lut(), ops.default_lut()):
        assert lut.dtype == torch.float32 and tuple(lut.shape) == (256, 3)
        assert float(lut.min()) >= 0.0 and float(lut.max()) <= 1.0
    # the fallback follows viridis: dark purple to yellow
    fb = ops.fallback_lut()
    assert fb[0, 2] > fb[0, 1] and fb[255, 0] > 0.9 and fb[255, 1] > 0.9


def test_sheet_shape_formula():
    from stablekeypoints_amd import ops
    assert ops.sheet_shape(512, 512, 11, 9, downscale=4, pad=2) == (11 * 130 + 2, 9 * 130 + 2)


def test_reference_visualize_import_line():
    from unsupervised_keypoints.visualize import create_vid, visualize_attn_maps
    import stablekeypoints_amd.visualize as impl
    assert visualize_attn_maps is impl.visualize_attn_maps and create_vid is impl.create_vid


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_agrees_with_itself_in_f32_and_f64(name):
    """The float32 restatement against the float64 one, under the rule of the GPU test: the
    test inputs satisfy the rule's conditions (range, circle margin, band share)."""
    from stablekeypoints_amd import ops
    case = R.make_case(name, ops.fallback_lut().numpy())
    ref = R.reference(case)
    R.check_conditions(case, ref)
    R.check(R.reference(case, np.float32)[0], ref, case["f"])
    kinds = set(np.unique(ref[2]))
    assert R.PAD in kinds and R.EMPTY in kinds
    if case["points"] is not None:
        assert R.DISC in kinds and R.OUTLINE in kinds


def test_restatement_markers():
    """Later marker wins, the NaN marker paints nothing, the corner marker is clipped to its tile."""
    from stablekeypoints_amd import ops
    case = R.make_case("d_points_only", ops.fallback_lut().numpy())
    out, _, kind, _ = R.reference(case)
    th, pad = 16, 1
    tile = out[pad:pad + th, pad:pad + th]
    assert (tile == R.COLORS[1]).all(axis=-1).sum() == 0                     # NaN marker
    assert (out[:pad] == 255).all() and (out[:, :pad] == 255).all()          # the corner disc stays inside
    py, px = case["points"][0, 3] * th
    assert tuple(tile[int(py), int(px)]) == tuple(R.COLORS[3])               # overlap: marker 3 over marker 2
    assert (kind[pad:pad + th, pad:pad + th] == R.DISC).sum() > 20


def _patched_main(monkeypatch, tmp_path, extra):
    """Run ``main`` with every stage patched out; returns the recorded visualize_attn_maps calls."""
    import stablekeypoints_amd.eval as ev
    import stablekeypoints_amd.keypoint_regressor as kr
    import stablekeypoints_amd.optimize as opt
    import stablekeypoints_amd.optimize_token as ot
    import stablekeypoints_amd.visualize as vis
    calls = []
    monkeypatch.setattr(ot, "load_ldm", lambda *a, **k: ("ldm", "controllers", 1))
    monkeypatch.setattr(opt, "optimize_embedding", lambda *a, **k: torch.zeros(1, 4, 8))
    monkeypatch.setattr(kr, "find_best_indices", lambda *a, **k: torch.arange(3))
    monkeypatch.setattr(kr, "precompute_all_keypoints",
                        lambda *a, **k: (torch.rand(6, 3, 2), torch.rand(6, 15, 2), None))
    monkeypatch.setattr(ev, "evaluate", lambda *a, **k: 0.0)
    monkeypatch.setattr(vis, "visualize_attn_maps", lambda *a, **k: calls.append((a, k)))
    monkeypatch.setattr(torch.cuda, "manual_seed", lambda *a, **k: None)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    from stablekeypoints_amd.main import main
    main(["--model_type", "tiny", "--dataset_name", "synthetic", "--save_folder", str(tmp_path), "--num_gpus", "1",
          "--device", "cpu", "--top_k", "3"] + extra)
    return calls


def test_main_visualize_flag_calls_visualize_twice(monkeypatch, tmp_path):
    calls = _patched_main(monkeypatch, tmp_path, ["--visualize"])
    assert len(calls) == 2
    (a0, k0), (a1, k1) = calls
    assert a0[0] == "ldm" and k0.get("regressor") is None and k0["num_points"] == 3
    assert k0["save_folder"] == str(tmp_path) and k0["controllers"] == "controllers"
    assert torch.is_tensor(k1["regressor"]) and tuple(k1["regressor"].shape) == (6, 30)
    assert os.path.exists(tmp_path / "regressor.pt")


def test_main_without_flag_never_visualizes(monkeypatch, tmp_path):
    assert _patched_main(monkeypatch, tmp_path, []) == []
