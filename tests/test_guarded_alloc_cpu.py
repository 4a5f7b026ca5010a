"""tests/guarded_alloc.py on CPU tensors, with small fake ops written in torch: a correct op passes,
every planted violation is detected, and the patched functions come back.  Without this file
tests/test_gpu_memory_contract.py could pass while checking nothing.
"""
import pytest
import torch

from guarded_alloc import GUARD, POISONS, GuardedAlloc, bit_equal

REAL_EMPTY, REAL_EMPTY_LIKE = torch.empty, torch.empty_like


def _past(t, k):
    """The k-th element after (k >= 0) or before (k < 0) t's payload, through its backing storage —
    what a kernel's misplaced store reaches.  The guards are allocated bytes of the same storage."""
    flat = REAL_EMPTY(0, dtype=t.dtype).set_(t.untyped_storage())
    base = t.storage_offset()
    assert base == GUARD // t.element_size() and flat[base:].data_ptr() == t.data_ptr()
    return flat, (base + t.numel() + k) if k >= 0 else (base + k)


def op_correct(x):
    """out = 2·x through a workspace that is fully written before it is read."""
    ws = torch.empty(x.numel(), dtype=torch.float64)
    out = torch.empty_like(x)
    ws.copy_(x.reshape(-1))
    out.copy_((2.0 * ws).reshape(x.shape))
    return out


def op_writes_after(x):
    out = op_correct(x)
    flat, i = _past(out, 0)
    flat[i] = 1.0
    return out


def op_writes_before(x):
    out = op_correct(x)
    flat, i = _past(out, -1)
    flat[i] = 1.0
    return out


def op_unwritten_output(x):
    out = torch.empty_like(x)
    out.reshape(-1)[:-1] = 2.0 * x.reshape(-1)[:-1]      # the last element keeps what the buffer held
    return out


def op_unwritten_workspace(x):
    """A 'merge' that takes the maximum over a workspace whose last slot no 'tile' produced."""
    ws = torch.empty(x.numel() + 1, dtype=x.dtype)
    ws[:-1] = x.reshape(-1)
    best = ws[0].clone()
    for v in ws[1:]:
        if v > best:          # a NaN never wins this comparison; a huge finite value does
            best = v.clone()
    return best


def _run(op, x, poison):
    with GuardedAlloc(poison, "cpu", op=op.__name__) as g:
        out = op(x.clone())
    return out, g


X = torch.arange(12, dtype=torch.float32).reshape(3, 4) / 7.0


@pytest.mark.parametrize("poison", POISONS)
def test_correct_op_passes(poison):
    out, g = _run(op_correct, X, poison)
    assert g.violations() == []
    assert len(g.records) == 2 and g.passed == []
    assert [r.shape for r in g.records] == [(12,), (3, 4)]
    assert [r.dtype for r in g.records] == [torch.float64, torch.float32]
    assert "test_guarded_alloc_cpu.py" in g.records[0].site and "op_correct" in g.records[0].site
    assert torch.equal(out, 2.0 * X)
    assert out.data_ptr() % 256 == g.records[1].buf.data_ptr() % 256      # the guard keeps the alignment


def test_both_poisons_agree_on_a_correct_op():
    a, _ = _run(op_correct, X, POISONS[0])
    b, _ = _run(op_correct, X, POISONS[1])
    assert bit_equal(a, b) and bit_equal(a, op_correct(X))


def test_the_whole_buffer_is_poisoned():
    with GuardedAlloc(0xFF, "cpu") as g:
        f = torch.empty(5)
        i = torch.empty(3, dtype=torch.int64)
    assert torch.isnan(f).all() and (i == -1).all()
    assert (g.records[0].buf == 0xFF).all() and g.records[0].buf.numel() == 2 * GUARD + 20
    with GuardedAlloc(0x7F, "cpu"):
        f = torch.empty(5)
        d = torch.empty(2, dtype=torch.float64)
        i = torch.empty(3, dtype=torch.int32)
    assert (f > 3e38).all() and torch.isfinite(f).all()
    assert (d > 1e306).all() and torch.isfinite(d).all()
    assert (i == 0x7F7F7F7F).all()


@pytest.mark.parametrize("poison", POISONS)
def test_write_one_element_after_is_reported(poison):
    _, g = _run(op_writes_after, X, poison)
    v = g.violations()
    assert len(v) == 1, v
    assert "op_writes_after" in v[0] and "allocation 1" in v[0] and "shape=(3, 4)" in v[0]
    assert "torch.float32" in v[0] and "back guard" in v[0] and "offset +" in v[0]
    assert "test_guarded_alloc_cpu.py" in v[0]


@pytest.mark.parametrize("poison", POISONS)
def test_write_one_element_before_is_reported(poison):
    _, g = _run(op_writes_before, X, poison)
    v = g.violations()
    assert len(v) == 1, v
    assert "front guard" in v[0] and "allocation 1" in v[0] and "offset -" in v[0]


def test_first_offending_offset():
    with GuardedAlloc(0xFF, "cpu") as g:
        t = torch.empty(4, dtype=torch.float32)
    flat, i = _past(t, 2)                       # the third float past the end: bytes 8..11
    flat[i] = 0.0
    (v,) = g.violations()
    assert "offset +8 from the payload's end" in v and "(4 bytes changed)" in v
    flat[i - 2 - 4 - 1] = 0.0                   # one float before the start
    front = [m for m in g.violations() if "front" in m]
    assert len(front) == 1 and "offset -4 from the payload's start" in front[0]


def test_unwritten_output_element_differs_between_poisons():
    a, ga = _run(op_unwritten_output, X, POISONS[0])
    b, gb = _run(op_unwritten_output, X, POISONS[1])
    assert ga.violations() == [] and gb.violations() == []     # nothing out of bounds: only the values tell
    assert not bit_equal(a, b)
    assert bit_equal(a.reshape(-1)[:-1], b.reshape(-1)[:-1])   # ... and only in the unwritten element


def test_unwritten_workspace_element_differs_between_poisons():
    a, ga = _run(op_unwritten_workspace, X, POISONS[0])
    b, gb = _run(op_unwritten_workspace, X, POISONS[1])
    assert ga.violations() == [] and gb.violations() == []
    assert float(a) == float(X.max())      # the NaN poison alone is swallowed by the comparison
    assert not bit_equal(a, b)             # the huge finite one is not


def test_patches_are_restored():
    with GuardedAlloc(0xFF, "cpu"):
        assert torch.empty is not REAL_EMPTY and torch.empty_like is not REAL_EMPTY_LIKE
    assert torch.empty is REAL_EMPTY and torch.empty_like is REAL_EMPTY_LIKE


def test_patches_are_restored_on_an_exception():
    class Boom(Exception):
        pass

    holder = type("M", (), {"CACHE": {"k": 1}})
    with pytest.raises(Boom):
        with GuardedAlloc(0xFF, "cpu", caches=[(holder, "CACHE")]):
            assert holder.CACHE == {}
            holder.CACHE["ws"] = torch.empty(3)
            raise Boom()
    assert torch.empty is REAL_EMPTY and torch.empty_like is REAL_EMPTY_LIKE
    assert holder.CACHE == {"k": 1}


def test_pass_throughs_are_counted():
    with GuardedAlloc(0xFF, "cpu") as g:
        z = torch.empty(0)                                              # no elements
        m = torch.empty(3, 4, device="meta")                            # another device
        o = torch.empty(4, out=REAL_EMPTY(4))                           # out=
        nc = torch.empty_like(REAL_EMPTY(4, 6).t())                     # preserve_format: non-contiguous
        ok = torch.empty(2, 2)
    assert [p[0] for p in g.passed] == ["empty", "other device", "out=", "non-contiguous"]
    assert len(g.records) == 1 and g.records[0].shape == (2, 2)
    assert z.numel() == 0 and m.device.type == "meta" and o.shape == (4,) and not nc.is_contiguous()
    assert torch.isnan(ok).all()
    assert [p[0] for p in g.passed_on("cpu")] == ["out=", "non-contiguous"]
    assert "4 passed through" in g.report() and "1 guarded" in g.report()


def test_caller_guarded_buffer():
    with GuardedAlloc(0x7F, "cpu") as g:
        out = g.guarded((2, 3), torch.float32)
        out.copy_(torch.ones(2, 3))
        assert g.violations() == []
        flat, i = _past(out, 0)
        flat[i] = 0.0
    assert len(g.violations()) == 1 and len(g.records) == 1


def test_bad_guard_is_rejected():
    with pytest.raises(ValueError):
        GuardedAlloc(0xFF, "cpu", guard=100)
