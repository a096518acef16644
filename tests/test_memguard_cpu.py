"""tests/memguard.py on CPU tensors: the guard-and-poison helper must itself notice what the GPU contract tests rely on it to notice —
a write one element outside a buffer (either side, with the right offset in the message), a read of an element nobody wrote (different
bits under the two fills), and nothing at all for a function that writes what it reads — and must put torch back as it found it."""
import pytest
import torch

import memguard as MG

CPU = dict(device_types=("cpu",), callers="all")


@pytest.mark.parametrize("fill", MG.FILLS)
def test_shapes_dtypes_and_pass_through(monkeypatch, fill):
    real_empty, real_like = torch.empty, torch.empty_like
    with MG.MemGuard(monkeypatch, fill, **CPU) as g:
        assert torch.empty is not real_empty and torch.empty_like is not real_like
        a = torch.empty(3, 5, 7)
        b = torch.empty((), dtype=torch.float32)
        c = torch.empty((4, 6), dtype=torch.bfloat16, device="cpu")
        d = torch.empty([9], dtype=torch.uint8)
        e = torch.empty(torch.Size([2, 3]), dtype=torch.float32)
        f = torch.empty_like(a)
        h = torch.empty_like(a, dtype=torch.bfloat16)
        for t, shape, dt in [(a, (3, 5, 7), torch.float32), (b, (), torch.float32), (c, (4, 6), torch.bfloat16), (d, (9,), torch.uint8),
                             (e, (2, 3), torch.float32), (f, (3, 5, 7), torch.float32), (h, (3, 5, 7), torch.bfloat16)]:
            assert tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous()
            assert t.storage_offset() * t.element_size() == MG.TENSOR_GUARD and t.data_ptr() % 512 == t.untyped_storage().data_ptr() % 512
            assert bool((t.reshape(-1).view(torch.uint8) == fill).all())          # poisoned
        assert g.n_tensors == 7 and g.n_ws == 0
        if fill == 0xFF:
            assert bool(torch.isnan(a).all()) and bool(torch.isnan(c.float()).all())
        # int64 index lists: guarded, not poisoned
        i = torch.empty(5, 4, dtype=torch.int64)
        i.zero_()
        assert g.n_tensors == 8 and g.records[-1].poisoned is False and i.storage_offset() > 0
        # everything else goes to the real allocator
        n0 = g.n_tensors
        for t in (torch.empty(3, dtype=torch.float64), torch.empty(3, dtype=torch.float16), torch.empty(2, 2, dtype=torch.bool),
                  torch.empty(3, pin_memory=False), torch.empty_like(a.transpose(0, 2)), torch.empty_like(a, memory_format=torch.contiguous_format)):
            assert t.storage_offset() == 0
        z = torch.zeros(4, 4)
        assert z.storage_offset() == 0 and torch.zeros_like(a).storage_offset() == 0
        assert g.n_tensors == n0
        r = torch.empty(3, requires_grad=True)
        assert r.requires_grad and r.storage_offset() > 0
        g.check()
    assert torch.empty is real_empty and torch.empty_like is real_like and g.records == []


def test_other_devices_and_other_callers_pass_through(monkeypatch):
    with MG.MemGuard(monkeypatch, 0xFF) as g:                 # the GPU tests' settings: CUDA allocations made by the package
        assert torch.empty(8).storage_offset() == 0
    with MG.MemGuard(monkeypatch, 0xFF, device_types=("cpu",)) as g:
        assert torch.empty(8).storage_offset() == 0           # this file is not part of m3l_amd
        assert g.n_tensors == 0
        t = g.alloc((2, 3), torch.float32, "cpu")             # a test's own guarded buffer
        assert t.storage_offset() > 0 and g.n_tensors == 1 and g.records[-1].site[0] == __file__


@pytest.mark.parametrize("fill", MG.FILLS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
def test_one_element_overrun_is_reported_with_side_and_offset(monkeypatch, fill, dtype):
    def past(t, k):      # the bytes of element k past the payload's end (k < 0: in front of its start), through the shared storage
        at = t.storage_offset() + (t.numel() + k if k >= 0 else k)
        return torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage(), at * t.element_size(), (t.element_size(),))

    real = torch.empty
    item = real(0, dtype=dtype).element_size()
    with MG.MemGuard(monkeypatch, fill, **CPU) as g:
        t = torch.empty(6, 10, dtype=dtype); line = _line()
        t.fill_(1)
        g.check()
        past(t, 0).fill_(0x5A)
        with pytest.raises(MG.GuardViolation) as e:
            g.check("after the planted write")
        msg = str(e.value)
        assert "after the payload" in msg and "offset +0 " in msg and "(6, 10)" in msg and str(dtype) in msg
        assert f"{__file__}:{line}" in msg and "after the planted write" in msg
        v = g.violations()
        assert len(v) == 1 and v[0]["side"] == "after" and v[0]["offset"] == 0 and v[0]["count"] == item
    with MG.MemGuard(monkeypatch, fill, **CPU) as g:
        t = torch.empty(6, 10, dtype=dtype)
        u = torch.empty(4, dtype=dtype)
        past(t, -1).fill_(0x5A)
        v = g.violations()
        assert len(v) == 1 and v[0]["side"] == "before" and v[0]["offset"] == -item and tuple(v[0]["shape"]) == (6, 10)
        with pytest.raises(MG.GuardViolation, match="before the payload"):
            g.check()
        past(u, 2).fill_(0x5A)                                    # two elements further: reported at its own offset
        v = g.violations()
        assert len(v) == 2 and v[1]["side"] == "after" and v[1]["offset"] == 2 * item and tuple(v[1]["shape"]) == (4,)


def _line():
    import sys
    return sys._getframe(1).f_lineno


def test_workspace_seam_guard_size_and_size_bookkeeping(monkeypatch):
    import m3l_amd.dino as Dn
    import m3l_amd.functional as Fn
    real_ws = Fn._ws
    assert Dn._ws is real_ws
    with MG.MemGuard(monkeypatch, 0x00, **CPU) as g:
        assert Fn._ws is not real_ws and Dn._ws == Fn._ws          # every binding of the seam
        g.ws_sizes.append(("m3l_some_ws_bytes", 1000))             # what a recorded *_ws_bytes call leaves behind
        w = Fn._ws(1000, "cpu")
        assert w.dtype == torch.uint8 and w.numel() == 1000 and w.storage_offset() == MG.WS_GUARD and g.n_ws == 1
        assert g.ws_requests[-1][:2] == (1000, "m3l_some_ws_bytes") and not g.ws_unmatched
        g.ws_sizes.append(("m3l_some_ws_bytes", 1000))
        Dn._ws(744, "cpu")                                         # a request no size function stands behind
        assert g.n_ws == 2 and len(g.ws_unmatched) == 1 and g.ws_unmatched[0][0] == 744
        w[999] = 1
        g.check()
        torch.empty(0, dtype=torch.uint8).set_(w.untyped_storage(), w.storage_offset() + 1000, (1,)).fill_(1)
        with pytest.raises(MG.GuardViolation, match=r"ws \(1000,\).*after the payload.*offset \+0 "):
            g.check()
    assert Fn._ws is real_ws and Dn._ws is real_ws


def _reads_a_stale_element(x):
    """A 'kernel' that leaves the last workspace element unwritten and reads it."""
    ws = torch.empty(x.numel() + 1)
    ws[:x.numel()] = x.reshape(-1) * 2
    return {"y": ws.sum().reshape(())}


def _writes_all_it_reads(x):
    ws = torch.empty(x.numel())
    ws.copy_(x.reshape(-1) * 2)
    out = torch.empty_like(x)
    out.copy_(ws.view_as(x) + 1)
    return {"y": out, "s": ws.sum()}


def test_stale_read_gives_different_bits_under_the_two_fills(monkeypatch):
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    got = {}
    for fill in MG.FILLS:
        with MG.MemGuard(monkeypatch, fill, **CPU) as g:
            got[fill] = MG.clone_out(_reads_a_stale_element(x))
            g.check()                                              # it never left its buffer
    assert MG.differing(got[0xFF], got[0x00]) == ["y"]
    assert MG.nonfinite(got[0xFF]) == ["y"] and MG.nonfinite(got[0x00]) == []
    with pytest.raises(AssertionError, match="non-finite results with memory pre-filled with 0xFF"):
        MG.run_contract(monkeypatch, lambda g: _reads_a_stale_element(x), need_ws=False, **CPU)
    # a stale read that stays finite (poison x 0 is NaN only for 0xFF; an integer workspace read shows as different bits)
    def stale_bytes(g):
        ws = torch.empty(4, dtype=torch.uint8)
        ws[:3] = 1
        return {"n": ws.sum()}
    with pytest.raises(AssertionError, match="results depend on what memory held before the call"):
        MG.run_contract(monkeypatch, stale_bytes, need_ws=False, fills=(0x00, 0xFF), **CPU)


def test_clean_function_passes_the_contract(monkeypatch):
    x = torch.randn(5, 7)
    counts = MG.run_contract(monkeypatch, lambda g: _writes_all_it_reads(x), need_ws=False, **CPU)
    assert counts == [(0, 2), (0, 2)]
    with pytest.raises(AssertionError, match="no workspace request went through the guard"):
        MG.run_contract(monkeypatch, lambda g: _writes_all_it_reads(x), need_ws=True, **CPU)
    with pytest.raises(AssertionError, match="no tensor allocation went through the guard"):
        MG.run_contract(monkeypatch, lambda g: {"y": x * 2}, need_ws=False, **CPU)
    assert MG.differing({"a": x, "b": [x, None]}, {"a": x.clone(), "b": [x.clone(), None]}) == []
    assert MG.differing({"a": x}, {"a": x.double()}) == ["a"] and MG.differing({"a": x}, {}) == ["a"]


def test_overrun_inside_run_contract_fails_it(monkeypatch):
    def work(g):
        out = torch.empty(8)
        out.fill_(1.0)
        torch.empty(0).set_(out.untyped_storage(), out.storage_offset() + 8, (1,)).fill_(1.0)
        return {"y": out}
    with pytest.raises(MG.GuardViolation, match="after the payload"):
        MG.run_contract(monkeypatch, work, need_ws=False, **CPU)
    assert torch.empty is MG._REAL_EMPTY and torch.empty_like is MG._REAL_EMPTY_LIKE
