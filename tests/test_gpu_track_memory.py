"""Where ops.track_step and ops.track_backtrace write, and whether their results depend on what their
buffers held before: the memory contract of tests/test_gpu_memory_contract.py (its Case, its runs and
its comparisons, as tests/test_gpu_match_field_memory.py applies it) for skp_track_step — a frame 0
and a later frame, on ragged 32 × 32 tiles at the largest radius and on a plane smaller than the window
— and for skp_track_backtrace.

Each case runs plainly and under the two poisons with every buffer of ops' making, the cached workspace
included, carved out of a poisoned allocation with guard bands (tests/guarded_alloc.py): no guard byte
may change, every result is bit-equal across the three runs, the inputs are unchanged and only the
case's entry was called.
"""
import pytest
import torch

from guarded_alloc import POISONS
from test_gpu_memory_contract import DEV, Case, _agree, _one_run, rnd

pytestmark = pytest.mark.gpu

SHAPES = ((2, 70, 32), (3, 5, 8), (2, 37, 3), (1, 100, 3))     # (n, S, r); the last has tiles off the border


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _cases():
    from stablekeypoints_amd import ops
    out = []
    for n, S, r in SHAPES:
        w = ops.track_weights(r / 2.5, r)

        def mk0(n=n, S=S):
            return dict(avg=rnd(41, n, S, S).abs())

        def run0(ops, i, g, w=w):
            res = ops.track_step(i["avg"], None, w)
            assert [t.dtype for t in res] == [torch.float32, torch.float32, torch.int32, torch.int16]
            return list(res)

        def mk1(n=n, S=S):
            prev = rnd(42, n, S, S).abs()
            return dict(avg=rnd(43, n, S, S).abs(), prev=prev, prev_max=prev.reshape(n, -1).max(dim=1).values.contiguous())

        def run1(ops, i, g, w=w):
            return list(ops.track_step(i["avg"], (i["prev"], i["prev_max"], None, None), w))

        def mkb(n=n, S=S, r=r):
            gen = torch.Generator().manual_seed(44)
            back = torch.randint(0, (2 * r + 1) ** 2, (4, n, S, S), generator=gen).to(torch.int16)
            # random codes leave the plane: the entry clamps them, and must read nothing outside the stack
            return dict(back=back.to(DEV), best=torch.randint(0, S * S, (n,), generator=gen).to(torch.int32).to(DEV))

        def runb(ops, i, g, r=r):
            return [ops.track_backtrace(i["back"], i["best"], r)]

        for tag, mk, run, kernel, least in (("step0", mk0, run0, "skp_track_step", 5), ("step", mk1, run1, "skp_track_step", 5),
                                            ("backtrace", mkb, runb, "skp_track_backtrace", 1)):
            name = f"track_{tag}-{n}x{S}-r{r}"
            out.append(pytest.param(Case(name, mk, run, kernels=[kernel]), least, id=name))
    return out


@pytest.mark.parametrize("c,least", _cases())
def test_track_memory_contract(c, least, monkeypatch):
    from stablekeypoints_amd import ops
    names = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    inp = c.make()
    runs = {}
    try:
        base, _ = _one_run(ops, c, inp, None, names)
        assert names == list(c.kernels)
        for poison in POISONS:
            runs[poison] = _one_run(ops, c, inp, poison, names)
            assert names == list(c.kernels)
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
        # the step: score, score_max, best, back and the workspace (the cache is emptied for the run); the backtrace: pos
        assert len(g.records) >= least, reports
        assert g.result_inside, f"{c.name}: no result inside a guarded allocation\n" + reports
    (ra, _), (rb, _) = runs[POISONS[0]], runs[POISONS[1]]
    _agree(c, "poison 0xFF", ra, "poison 0x7F", rb)
    _agree(c, "the plain run", base, "poison 0xFF", ra)
    _agree(c, "the plain run", base, "poison 0x7F", rb)
    if c.kernels == ("skp_track_backtrace",):
        S = inp["back"].shape[-1]
        assert bool(((base[0] >= 0.5) & (base[0] <= S - 0.5)).all())
