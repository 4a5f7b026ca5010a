"""Where ops.match_refine writes, and whether its results depend on what its buffers held before: the
memory contract of tests/test_gpu_memory_contract.py (its Case, its runs and its comparisons, as
tests/test_gpu_match_field_memory.py applies it) for skp_match_refine, on a batch of two with f = 4,
w = 5, 5 tokens and every border clipped, and on one image with f = 8, w = 8 and two panels of tokens
plus one token; each with an unusable p, a NaN in y and a prior of −1.

Each case runs plainly and under the two poisons with every buffer of ops' making, the cached workspace
included, carved out of a poisoned allocation with guard bands (tests/guarded_alloc.py): no guard byte
may change, every result is bit-equal across the three runs, the inputs are unchanged and
skp_match_refine was the only entry called.
"""
import pytest
import torch

from guarded_alloc import POISONS
from test_gpu_memory_contract import DEV, Case, _agree, _one_run, rnd

pytestmark = pytest.mark.gpu

SHAPES = ((2, 5, 24, 4, 5), (1, 33, 32, 8, 8))     # (B, n, S, f, w)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _cases():
    out = []
    for B, n, S, f, w in SHAPES:
        def mk(B=B, n=n, S=S, f=f):
            Sc = S // f
            x, y = rnd(41, B, n, S, S), rnd(42, B, n, S, S)
            coarse = torch.randint(0, Sc * Sc, (B, Sc, Sc), generator=torch.Generator().manual_seed(43),
                                   dtype=torch.int32).to(DEV)
            x[0, :, 0, 3] = 0                    # an unusable p, a NaN in y and a cell without a prior:
            y[0, 0, S - 1, S - 1] = float("nan")  # −1 / −inf are written, not skipped
            coarse[0, Sc - 1, Sc - 1] = -1
            return dict(x=x, y=y, coarse=coarse)

        def run(ops, i, g, w=w):
            res = ops.match_refine(i["x"], i["y"], i["coarse"], w)
            assert len(res) == 2 and res[0].dtype == torch.int32 and res[1].dtype == torch.float32
            return list(res)
        name = f"match_refine-{B}x{n}x{S}-f{f}-w{w}"
        out.append(pytest.param(Case(name, mk, run, kernels=["skp_match_refine"]), S, f, id=name))
    return out


@pytest.mark.parametrize("c,S,f", _cases())
def test_match_refine_memory_contract(c, S, f, monkeypatch):
    from stablekeypoints_amd import ops
    names = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    inp = c.make()
    runs = {}
    try:
        base, _ = _one_run(ops, c, inp, None, names)
        assert names == ["skp_match_refine"]
        for poison in POISONS:
            runs[poison] = _one_run(ops, c, inp, poison, names)
            assert names == ["skp_match_refine"]
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
    assert int(base[0][0, 0, 3]) == -1 and float(base[1][0, 0, 3]) == float("-inf")
    assert bool((base[0][0, S - f:, S - f:] == -1).all()) and bool(torch.isneginf(base[1][0, S - f:, S - f:]).all())
    assert not bool((base[0][0] == S * S - 1).any())
    assert int((base[0] >= 0).sum()) == base[0].numel() - 1 - f * f
