"""Where ops.match_field writes, and whether its results depend on what its buffers held before: the
memory contract of tests/test_gpu_memory_contract.py (its Case, its runs and its comparisons, as
tests/test_gpu_tta_match_memory.py applies it) for skp_match_field, on a batch of two with a ragged P
tile and 11 splits of Q, both operands per image, and on one image of 11 × 11 tiles with one panel of
tokens plus one token, the operands given with a leading 1.

Each case runs plainly and under the two poisons with every buffer of ops' making, the cached workspace
included, carved out of a poisoned allocation with guard bands (tests/guarded_alloc.py): no guard byte
may change, every result is bit-equal across the three runs, the inputs are unchanged and
skp_match_field was the only entry called.
"""
import pytest
import torch

from guarded_alloc import POISONS
from test_gpu_memory_contract import Case, _agree, _one_run, rnd

pytestmark = pytest.mark.gpu

SHAPES = ((2, 5, 200, 1369), (1, 33, 1369, 1369))     # (B, n, P, Q)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _cases():
    out = []
    for B, n, P, Q in SHAPES:
        def mk(B=B, n=n, P=P, Q=Q):
            x, y = rnd(31, B, n, P), rnd(32, B, n, Q)
            x[0, :, 3] = 0                      # an unusable p and an unusable q: −1 / −inf are written, not skipped
            y[0, 0, Q - 1] = float("nan")
            return dict(x=x, y=y)

        def run(ops, i, g):
            res = ops.match_field(i["x"], i["y"])
            assert len(res) == 2 and res[0].dtype == torch.int32 and res[1].dtype == torch.float32
            return list(res)
        name = f"match_field-{B}x{n}x{P}x{Q}"
        out.append(pytest.param(Case(name, mk, run, kernels=["skp_match_field"]), id=name))
    return out


@pytest.mark.parametrize("c", _cases())
def test_match_field_memory_contract(c, monkeypatch):
    from stablekeypoints_amd import ops
    names = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    inp = c.make()
    runs = {}
    try:
        base, _ = _one_run(ops, c, inp, None, names)
        assert names == ["skp_match_field"]
        for poison in POISONS:
            runs[poison] = _one_run(ops, c, inp, poison, names)
            assert names == ["skp_match_field"]
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
        assert len(g.records) >= 3, reports      # index, score and the workspace (the cache is emptied for the run)
        assert g.result_inside, f"{c.name}: no result inside a guarded allocation\n" + reports
    (ra, _), (rb, _) = runs[POISONS[0]], runs[POISONS[1]]
    _agree(c, "poison 0xFF", ra, "poison 0x7F", rb)
    _agree(c, "the plain run", base, "poison 0xFF", ra)
    _agree(c, "the plain run", base, "poison 0x7F", rb)
    assert int(base[0][0, 3]) == -1 and float(base[1][0, 3]) == float("-inf")
    assert not bool((base[0][0] == inp["y"].shape[2] - 1).any())
