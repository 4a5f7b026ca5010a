"""Generates tests/golden/corresponding_points.npz: what the reference's eval.find_corresponding_points
(eval.py:159-195) returns, on torch-CPU, for the selection cases of tests/corr_ref.py.

Inputs (not stored; tests rebuild them): the float32 casts of tta_ref.tta_ref(corr_ref.planted(shape))'s
averages, (B, n, S, S) read as (num_images, num_tokens, h, w), with num_points = corr_ref.K.  Stored per
case ``BxCxnxS``: ``*_indices`` (k,) int64, ``*_points`` (B, k, 2) float32 and ``*_entropy`` (n,) float32,
the reference's fp32 summed entropies (its own intermediate, recomputed with its statements).

Runs only where the reference is present (make_goldens.import_reference refuses otherwise).
Usage: python tests/golden/make_corr_golden.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_goldens  # noqa: E402

ref = make_goldens.import_reference()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import corr_ref  # noqa: E402


def main():
    out = {}
    for shape in corr_ref.CASES:
        B, C, n, S = shape
        maps = torch.from_numpy(np.array(corr_ref.planted_average(shape)))
        points, indices = ref.eval.find_corresponding_points(maps, num_points=corr_ref.K)
        soft = torch.softmax(maps.view(B * n, S * S), dim=-1)
        entropy = torch.distributions.Categorical(probs=soft).entropy().reshape(B, n).sum(dim=0)
        assert torch.equal(torch.argsort(entropy)[:corr_ref.K], indices)
        tag = "x".join(map(str, shape))
        out[f"{tag}_indices"] = indices.numpy().astype(np.int64)
        out[f"{tag}_points"] = points.numpy().astype(np.float32)
        out[f"{tag}_entropy"] = entropy.numpy().astype(np.float32)
        print(tag, indices.tolist(), flush=True)
    np.savez(os.path.join(HERE, "corresponding_points.npz"), **out)


if __name__ == "__main__":
    main()
