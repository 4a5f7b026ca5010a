"""eval.propagate_labels and eval.propagate_images on the device: the synthetic sequence of
tests/propagate_ref.py (48 blobs, 32² frames sliding by (1, −1), a disk of radius 7; w = 3, k = 5,
τ = 0.02, memory = 2) equals the loop of the public ops and carries the disk; tensor and iterable input
agree; on the tiny model of tests/tta_tiny.py ``propagate_images`` equals ``propagate_labels`` on the
averages that predict_keypoints(return_maps=True) gives for the same seed; and the CLI's ``--propagate``
writes its files."""
import numpy as np
import pytest
import torch

import propagate_ref as P
import tta_tiny
from tta_tiny import DEV, cli as _cli, tiny  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

KW = dict(radius=P.SEQ["w"], k=P.SEQ["k"], tau=P.SEQ["tau"], memory=P.SEQ["memory"])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _same(a, b):
    return all((s is None and t is None) or torch.equal(tta_tiny.bits(s), tta_tiny.bits(t)) for s, t in zip(a, b))


@pytest.fixture(scope="module")
def sequence():
    frames, masks = P.sequence(0)
    return torch.as_tensor(frames), masks


def test_propagate_labels_is_the_loop_of_the_public_ops_and_carries_the_disk(sequence):
    from stablekeypoints_amd import eval as ev, ops
    frames, masks = sequence
    labels0 = torch.as_tensor(masks[0].astype(np.int64))
    got = ev.propagate_labels(frames, labels0, device=DEV, return_soft=True, **KW)
    assert isinstance(got, ev.PropagatedLabels)
    T, n, S = frames.shape[0], frames.shape[1], frames.shape[-1]
    assert tuple(got.label.shape) == (T, S, S) and got.label.dtype == torch.int32
    assert tuple(got.confidence.shape) == (T, S, S) and got.confidence.dtype == torch.float32
    assert tuple(got.soft.shape) == (T, 2, S, S) and got.soft.dtype == torch.float32
    # the loop: one match_topk with x shared and the context stacked, one label_vote, per frame
    sig = frames.to(DEV)
    soft = [torch.as_tensor(P.one_hot(masks[0]), device=DEV)]
    assert torch.equal(got.soft[0], soft[0]) and torch.equal(got.label[0].cpu(), labels0.int())
    assert torch.equal(got.confidence[0], torch.ones(S, S, device=DEV))
    for t in range(1, T):
        ctx = P.context_of(t, KW["memory"])
        index, score = ops.match_topk(sig[t][None].contiguous(), sig[ctx].contiguous(), KW["radius"], KW["k"])
        s, l, c = ops.label_vote(index, score, torch.stack([soft[j] for j in ctx]), KW["tau"])
        soft.append(s)
        assert _same((got.soft[t], got.label[t], got.confidence[t]), (s, l, c)), t
    # the condition of the CPU test, on the device's own result
    last = got.label[-1].cpu().numpy()
    iou, still = P.iou(last == 1, masks[-1]), P.iou(masks[0], masks[-1])
    print(f"device: propagated {iou:.4f}, left in place {still:.4f}")
    assert iou >= 0.5 and iou >= still + 0.3
    assert (last >= 0).all()
    plain = ev.propagate_labels(frames, labels0, device=DEV, **KW)
    assert plain.soft is None and _same(plain[:2], got[:2])


def test_tensor_iterable_device_and_soft_inputs_agree(sequence):
    from stablekeypoints_amd import eval as ev
    frames, masks = sequence
    frames = frames[:4]
    labels0 = torch.as_tensor(masks[0].astype(np.int64))
    a = ev.propagate_labels(frames, labels0, device=DEV, return_soft=True, **KW)
    b = ev.propagate_labels((f for f in frames), labels0, device=DEV, return_soft=True, **KW)
    c = ev.propagate_labels(frames.to(DEV), labels0.to(DEV), return_soft=True, **KW)
    d = ev.propagate_labels(list(frames.numpy()), torch.as_tensor(P.one_hot(masks[0])), device=DEV, return_soft=True, **KW)
    assert _same(a, b) and _same(a, c) and _same(a[1:], d[1:]) and torch.equal(a.label[1:], d.label[1:])
    # a −1 casts no vote: with the background unlabelled every matched pixel is class 0
    e = ev.propagate_labels(frames, labels0 - 1, device=DEV, return_soft=True, **KW)
    assert tuple(e.soft.shape) == (4, 1, 32, 32) and int(e.label[0].min()) == -1
    assert bool((e.label[1:] == 0).all()) and float(e.soft[1].min()) < 0.5 and float(e.soft[1].max()) <= 1.0 + 1e-6
    # memory = 0: every frame against frame 0 alone
    f = ev.propagate_labels(frames, labels0, device=DEV, **dict(KW, memory=0))
    assert torch.equal(f.label[1], a.label[1]) and not torch.equal(f.label[3], a.label[3])
    with pytest.raises(ValueError, match="tokens"):
        ev.propagate_labels([frames[0], frames[1][:5]], labels0, device=DEV, **KW)


S_TINY = 32
TINY_KW = dict(device=DEV, layers=[0, 1, 2, 3], upscale_size=S_TINY, augmentation_iterations=3, **tta_tiny.AUG)


def test_propagate_images_is_propagate_labels_on_the_same_averages(tiny):
    from stablekeypoints_amd import eval as ev
    ldm, controllers, images, ctx, indices = tiny
    video = torch.cat([images, images.flip(-1), images.flip(-2)[:1]])          # five frames
    labels0 = (torch.arange(S_TINY * S_TINY).reshape(S_TINY, S_TINY) % 3 - 1)
    kw = dict(radius=4, k=3, tau=0.05, memory=1)
    tta_tiny.seed()
    got = ev.propagate_images(ldm, video, ctx, labels0, indices, controllers=controllers, image_batch=2,
                              return_soft=True, **TINY_KW, **kw)
    tta_tiny.seed()
    _, maps = ev.predict_keypoints(ldm, video, ctx, indices, controllers=controllers, image_batch=2, return_maps=True,
                                   **TINY_KW)
    want = ev.propagate_labels(maps, labels0, return_soft=True, **kw)
    assert tuple(got.label.shape) == (5, S_TINY, S_TINY) and tuple(got.soft.shape) == (5, 2, S_TINY, S_TINY)
    assert _same(got, want)
    assert bool((got.label[1:] >= 0).any())
    with pytest.raises(ValueError, match="upscale_size"):
        ev.propagate_images(ldm, video, ctx, labels0[:16, :16], indices, controllers=controllers, **TINY_KW)


def test_cli_propagate_writes_its_files(tmp_path):
    M, S = 5, 32
    labels = torch.zeros(128, 128, dtype=torch.int64)           # nearest-resized to 32
    labels[32:96, 32:96] = 1
    labels[:8] = -1
    torch.save(labels, tmp_path / "labels.pt")
    plain, out = tmp_path / "plain", tmp_path / "prop"
    kp_plain = _cli(plain)
    kp = _cli(out, "--propagate", str(tmp_path / "labels.pt"), "--propagate_size", str(S), "--propagate_radius", "4",
              "--propagate_k", "3", "--propagate_memory", "1", "--visualize")
    assert torch.equal(kp.view(torch.int32), kp_plain.view(torch.int32))      # the prediction draws what it drew
    label = torch.load(out / "propagated_labels.pt", weights_only=True)
    conf = torch.load(out / "propagated_confidence.pt", weights_only=True)
    assert tuple(label.shape) == (M, S, S) and label.dtype == torch.int32
    assert tuple(conf.shape) == (M, S, S) and conf.dtype == torch.float32
    assert torch.equal(label[0].long(), labels[::4, ::4])
    assert int(label.min()) >= -1 and int(label.max()) <= 1 and bool((label[1:] >= 0).any())
    assert float(conf.min()) >= 0.0 and float(conf.max()) <= 1.0 + 1e-6
    assert (out / "propagate.png").exists() and not (out / "propagated_fg_iou.pt").exists()
    with pytest.raises(SystemExit):
        _cli(tmp_path / "bad", "--propagate", str(tmp_path / "labels.pt"), "--propagate_radius", "17")
