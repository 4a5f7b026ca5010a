"""Where ops.tta_reduce_match writes, and whether its results depend on what its buffers held before:
the memory contract of tests/test_gpu_memory_contract.py (its Case, its runs and its comparisons, as
tests/test_gpu_tta_parts_memory.py applies it) for skp_tta_reduce_match, on one shape of a single chunk
of tokens (the tile kernel forms the scores and leaves the queries' partials) and one of three chunks
(the per-chunk sums in the workspace and the per-pixel merge), with and without the score map.

Each case runs plainly and under the two poisons with every buffer of ops' making, the cached workspace
included, carved out of a poisoned allocation with guard bands (tests/guarded_alloc.py): no guard byte
may change, every result is bit-equal across the three runs, the inputs (the queries among them) are
unchanged and skp_tta_reduce_match was the only entry called.
"""
import numpy as np
import pytest
import torch

import tta_ref
from guarded_alloc import POISONS
from test_gpu_memory_contract import Case, T, _agree, _one_run

pytestmark = pytest.mark.gpu

SHAPES = ((2, 3, 5, 37), (1, 2, 29, 37))
Q = 5       # the bucket of 8 accumulators, three of them idle


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _cases():
    out = []
    for shape in SHAPES:
        def mk(shape=shape):
            maps, th, _ = tta_ref.make_case(shape, special=False)
            q = np.random.default_rng([5, *shape]).random((Q, shape[2])).astype(np.float32)
            q /= np.sqrt((q.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
            return dict(maps=T(maps), th=T(th), q=T(q))
        for scores in (False, True):
            def run(ops, i, g, scores=scores):
                res = ops.tta_reduce_match(i["maps"], i["th"], i["q"], return_scores=scores)
                assert len(res) == 5 and (res[3] is not None) == scores and res[4] is None
                return list(res)
            name = f"tta_reduce_match-{'x'.join(map(str, shape))}-scores{int(scores)}"
            out.append(pytest.param(Case(name, mk, run, kernels=["skp_tta_reduce_match"]), id=name))
    return out


@pytest.mark.parametrize("c", _cases())
def test_match_memory_contract(c, monkeypatch):
    from stablekeypoints_amd import ops
    names = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    inp = c.make()
    runs = {}
    try:
        base, _ = _one_run(ops, c, inp, None, names)
        assert names == ["skp_tta_reduce_match"]
        for poison in POISONS:
            runs[poison] = _one_run(ops, c, inp, poison, names)
            assert names == ["skp_tta_reduce_match"]
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # the device is in an error state: nothing that follows in this process would mean anything
            pytest.exit(f"{c.name}: GPU fault, session ended: {e}", returncode=3)
        raise
    reports = "\n".join(g.report() for _, g in runs.values())
    print(reports)
    for poison, (_, g) in runs.items():
        v = g.violations()
        assert not v, "guard bytes changed:\n" + "\n".join(v) + "\n" + reports
        assert not g.passed_on("cuda"), f"{c.name}: device buffers passed through unguarded\n" + reports
        # pos, match_pos, match_score, the workspace (the cache is emptied for the run) and the score map where asked for
        assert len(g.records) >= (5 if c.name.endswith("scores1") else 4), reports
        assert g.result_inside, f"{c.name}: no result inside a guarded allocation\n" + reports
    (ra, _), (rb, _) = runs[POISONS[0]], runs[POISONS[1]]
    _agree(c, "poison 0xFF", ra, "poison 0x7F", rb)
    _agree(c, "the plain run", base, "poison 0xFF", ra)
    _agree(c, "the plain run", base, "poison 0x7F", rb)
