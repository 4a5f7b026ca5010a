"""Where ops.match_topk and ops.label_vote write, and whether their results depend on what their buffers
held before: the memory contract of tests/test_gpu_memory_contract.py (its Case, its runs and its
comparisons, as tests/test_gpu_match_refine_memory.py applies it) for skp_match_topk on
(B, n, S, w, K) = (2, 5, 24, 3, 5) and (1, 33, 20, 8, 16), each with an unusable p and a NaN in y, and for
skp_label_vote on (M, K, Kv, S, Cl) = (3, 5, 5, 24, 2) and (1, 16, 16, 20, 7), each with empty lists, a
pixel without a candidate and indices outside the plane.

Each case runs plainly and under the two poisons with every buffer of ops' making, the cached workspace
included, carved out of a poisoned allocation with guard bands (tests/guarded_alloc.py): no guard byte
may change, every result is bit-equal across the three runs, the inputs are unchanged and the case's
entry was the only one called.
"""
import pytest
import torch

from guarded_alloc import POISONS
from test_gpu_memory_contract import DEV, Case, _agree, _one_run, rnd

pytestmark = pytest.mark.gpu

TOPK = ((2, 5, 24, 3, 5), (1, 33, 20, 8, 16))       # (B, n, S, w, K)
VOTE = ((3, 5, 5, 24, 2), (1, 16, 16, 20, 7))       # (M, K, Kv, S, Cl)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _cases():
    out = []
    for B, n, S, w, K in TOPK:
        def mk(B=B, n=n, S=S):
            x, y = rnd(41, B, n, S, S), rnd(42, B, n, S, S)
            x[0, :, 0, 3] = 0                     # an unusable p and a NaN in y: −1 / −inf are written, not skipped
            y[0, 0, S - 1, S - 1] = float("nan")
            return dict(x=x, y=y)

        def run(ops, i, g, w=w, K=K):
            res = ops.match_topk(i["x"], i["y"], w, K)
            assert len(res) == 2 and res[0].dtype == torch.int32 and res[1].dtype == torch.float32
            return list(res)

        def check(base, B=B, S=S, K=K):
            assert tuple(base[0].shape) == (B, K, S, S)
            assert bool((base[0][0, :, 0, 3] == -1).all()) and bool(torch.isneginf(base[1][0, :, 0, 3]).all())
            assert not bool((base[0][0] == S * S - 1).any())
            assert int(base[0].min()) >= -1 and int(base[0].max()) < S * S
        name = f"match_topk-{B}x{n}x{S}-w{w}-k{K}"
        out.append(pytest.param(Case(name, mk, run, kernels=["skp_match_topk"]), "skp_match_topk", 3, check, id=name))
    for M, K, Kv, S, Cl in VOTE:
        def mk(M=M, K=K, S=S, Cl=Cl):
            g = torch.Generator().manual_seed(43)
            index = torch.randint(0, S * S, (M, K, S, S), generator=g, dtype=torch.int32)
            score = torch.randint(-32, 33, (M, K, S, S), generator=g).to(torch.float32).div_(32).sort(dim=1, descending=True).values
            empty = torch.arange(K)[None, :, None, None] >= torch.randint(0, K + 1, (M, 1, S, S), generator=g)
            empty[:, :, 0, 0] = True              # a pixel without a candidate: 0, −1, 0 and −1 sources are written
            index[empty], score[empty] = -1, float("-inf")
            index[0, 0, 1, 0], index[0, 0, 1, 1], index[0, 0, 1, 2] = S * S, 2 ** 31 - 1, -9
            labels = torch.rand(M, Cl, S, S, generator=g)
            return dict(index=index.to(DEV), score=score.contiguous().to(DEV), labels=labels.to(DEV))

        def run(ops, i, g, Kv=Kv):
            res = ops.label_vote(i["index"], i["score"], i["labels"], 0.07, k=Kv, return_source=True)
            assert len(res) == 4 and [t.dtype for t in res] == [torch.float32, torch.int32, torch.float32, torch.int32]
            return list(res)

        def check(base, M=M, Kv=Kv, S=S, Cl=Cl):
            soft, label, conf, source = base
            assert tuple(soft.shape) == (Cl, S, S) and tuple(source.shape) == (Kv, S, S)
            assert bool((soft[:, 0, 0] == 0).all()) and int(label[0, 0]) == -1 and float(conf[0, 0]) == 0.0
            assert bool((source[:, 0, 0] == -1).all())
            assert int(source.min()) >= -1 and int(source.max()) < M * S * S
            assert int(label.min()) >= -1 and int(label.max()) < Cl and bool(torch.isfinite(soft).all())
        name = f"label_vote-{M}x{K}x{S}-kv{Kv}-c{Cl}"
        out.append(pytest.param(Case(name, mk, run, kernels=["skp_label_vote"]), "skp_label_vote", 4, check, id=name))
    return out


@pytest.mark.parametrize("c,entry,buffers,check", _cases())
def test_propagate_memory_contract(c, entry, buffers, check, monkeypatch):
    from stablekeypoints_amd import ops
    names = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    inp = c.make()
    runs = {}
    try:
        base, _ = _one_run(ops, c, inp, None, names)
        assert names == [entry]
        for poison in POISONS:
            runs[poison] = _one_run(ops, c, inp, poison, names)
            assert names == [entry]
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
        assert len(g.records) >= buffers, reports      # the results (and match_topk's workspace: the cache is emptied for the run)
        assert g.result_inside, f"{c.name}: no result inside a guarded allocation\n" + reports
    (ra, _), (rb, _) = runs[POISONS[0]], runs[POISONS[1]]
    _agree(c, "poison 0xFF", ra, "poison 0x7F", rb)
    _agree(c, "the plain run", base, "poison 0xFF", ra)
    _agree(c, "the plain run", base, "poison 0x7F", rb)
    check(base)
