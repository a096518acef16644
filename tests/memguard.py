"""Guard-and-poison allocations for the memory-contract tests (test_memguard_cpu.py, test_memory_contract_gpu.py).

include/m3l_amd.h promises that every entry point allocates nothing, stays inside the workspace and outputs it was handed and does not
depend on what they held before.  Inside a `MemGuard` context every float32 / bfloat16 / uint8 allocation that m3l_amd makes on the guarded
device type — the workspace seam `functional._ws` (every binding of it), `torch.empty`, `torch.empty_like` — comes out of a larger uint8
block laid out as [guard | payload | guard] and filled with one byte value (0xFF: NaN in float32 and bf16; 0x00).  The tensor handed back
has the requested shape and dtype, is contiguous and shares the block's storage at a non-zero storage offset; the guards are multiples of
512 bytes, so the payload keeps the allocator's alignment and the kernels' 16-byte paths still apply.

  check()     synchronises the device (weight gradients run on the library's side stream) and asserts that every guard byte still holds
              the fill value; a failure names the allocation (shape, dtype, call site), the side and the offset of the first changed byte
  n_ws        workspace requests guarded;  n_tensors  torch.empty / empty_like allocations guarded
  ws_unmatched  workspace requests whose size is not what the `*_ws_bytes` call right in front of them returned (must stay empty)

A run that reads memory nobody wrote computes different bits under the two fills (`differing` finds them); a run that writes outside its
buffers changes a guard.  Integer tensors are guarded but never poisoned (a poisoned index would become a wild address); other dtypes,
other devices, torch.zeros / zeros_like and allocations made by code outside m3l_amd pass through to the real allocator."""
import os
import sys

import torch

WS_GUARD = 1 << 20          # bytes on each side of a workspace: more than one ragged 192-row tile of the widest row (192 x 1536 x 4 B)
TENSOR_GUARD = 256 << 10    # bytes on each side of any other tensor: output rows are at most 2352 floats
POISONED = (torch.float32, torch.bfloat16, torch.uint8)
GUARDED_ONLY = (torch.int64, torch.int32)      # guarded, left as the allocator returned them
FILLS = (0xFF, 0x00)

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.join(os.path.dirname(_HERE), "m3l_amd") + os.sep
_REAL_EMPTY = torch.empty
_REAL_EMPTY_LIKE = torch.empty_like


class GuardViolation(AssertionError):
    pass


class _Block:
    __slots__ = ("block", "guard", "nbytes", "shape", "dtype", "site", "poisoned", "kind")


def _site(skip_files):
    f = sys._getframe(2)
    while f is not None:
        fn = f.f_code.co_filename
        if fn not in skip_files and os.sep + "torch" + os.sep not in fn:
            return fn, f.f_lineno
        f = f.f_back
    return "?", 0


def _shape_of(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


class MemGuard:
    """with MemGuard(monkeypatch, fill) as g: ...; g.check().  device_types: which allocations are guarded ("cuda" for the GPU tests, "cpu"
    for the helper's own tests); callers: "m3l_amd" guards only allocations requested from files of the package, "all" every caller."""

    def __init__(self, monkeypatch, fill, device_types=("cuda",), callers="m3l_amd", ws_guard=WS_GUARD, tensor_guard=TENSOR_GUARD):
        assert fill in range(256) and ws_guard % 512 == 0 and tensor_guard % 512 == 0
        self.fill, self.device_types, self.callers = int(fill), tuple(device_types), callers
        self.ws_guard, self.tensor_guard = ws_guard, tensor_guard
        self._outer = monkeypatch
        self._mp = None
        self.records = []
        self.n_ws = self.n_tensors = 0
        self.ws_sizes = []           # (name of the *_ws_bytes function, bytes it returned) not yet claimed by a workspace request
        self.ws_requests = []        # (bytes, matching function name or None, site)
        self.ws_unmatched = []

    # ---- the guarded allocation
    def alloc(self, shape, dtype, device, kind="tensor", site=None):
        """A guarded tensor of this context (tests call it for buffers of their own)."""
        shape = _shape_of((shape,)) if not isinstance(shape, int) else (int(shape),)
        device = torch.device(device)
        itemsize = _REAL_EMPTY(0, dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * itemsize
        g = self.ws_guard if kind == "ws" else self.tensor_guard
        r = _Block()
        r.block = _REAL_EMPTY(g + nbytes + g, dtype=torch.uint8, device=device)
        r.guard, r.nbytes, r.shape, r.dtype, r.kind = g, nbytes, shape, dtype, kind
        r.site = site if site is not None else _site((__file__,))
        r.poisoned = dtype in POISONED
        if r.poisoned:
            r.block.fill_(self.fill)
        else:
            r.block[:g].fill_(self.fill)
            r.block[g + nbytes:].fill_(self.fill)
        t = _REAL_EMPTY(0, dtype=dtype, device=device)
        t.set_(r.block.untyped_storage(), g // itemsize, shape)
        assert t.is_contiguous() and (nbytes == 0 or t.data_ptr() == r.block.data_ptr() + g)
        self.records.append(r)
        if kind == "ws":
            self.n_ws += 1
        else:
            self.n_tensors += 1
        return t

    def _wanted(self, dtype, device, caller_file):
        if torch.device(device).type not in self.device_types or dtype not in POISONED + GUARDED_ONLY:
            return False
        return self.callers == "all" or caller_file.startswith(_PKG)

    # ---- replacements
    def _empty(self, *size, **kw):
        extra = set(kw) - {"dtype", "device", "requires_grad"}
        dtype = kw.get("dtype") or torch.get_default_dtype()
        device = kw.get("device")
        device = torch.device(device) if device is not None else _default_device()
        caller = sys._getframe(1).f_code.co_filename
        if extra or not size or not self._wanted(dtype, device, caller):
            return _REAL_EMPTY(*size, **kw)
        t = self.alloc(_shape_of(size), dtype, device, site=(caller, sys._getframe(1).f_lineno))
        return t.requires_grad_() if kw.get("requires_grad") else t

    def _empty_like(self, ref, **kw):
        extra = set(kw) - {"dtype", "device", "requires_grad"}
        dtype = kw.get("dtype") or ref.dtype
        device = torch.device(kw["device"]) if kw.get("device") is not None else ref.device
        caller = sys._getframe(1).f_code.co_filename
        if extra or not ref.is_contiguous() or ref.layout is not torch.strided or not self._wanted(dtype, device, caller):
            return _REAL_EMPTY_LIKE(ref, **kw)
        t = self.alloc(tuple(ref.shape), dtype, device, site=(caller, sys._getframe(1).f_lineno))
        return t.requires_grad_() if kw.get("requires_grad") else t

    def _ws(self, nbytes, device):
        f = sys._getframe(1)
        site = (f.f_code.co_filename, f.f_lineno)
        nbytes = int(nbytes)
        name = None
        if self.ws_sizes and self.ws_sizes[-1][1] == nbytes:      # sized by the *_ws_bytes call right in front of it
            name = self.ws_sizes[-1][0]
        pending, self.ws_sizes = self.ws_sizes[-3:], []
        self.ws_requests.append((nbytes, name, site))
        if name is None:
            self.ws_unmatched.append((nbytes, site, pending))
        if torch.device(device).type not in self.device_types:
            return _REAL_EMPTY(nbytes, dtype=torch.uint8, device=device)
        return self.alloc((nbytes,), torch.uint8, device, kind="ws", site=site)

    def _recording(self, name, fn):
        def ws_bytes(*a):
            n = int(fn(*a))
            self.ws_sizes.append((name, n))
            return n
        return ws_bytes

    # ---- context
    def __enter__(self):
        import m3l_amd.functional as Fn
        self._mp = self._outer.context()
        mp = self._mp.__enter__()
        orig_ws = Fn._ws
        for modname, mod in list(sys.modules.items()):
            if modname.startswith("m3l_amd") and mod is not None and getattr(mod, "_ws", None) is orig_ws:
                mp.setattr(mod, "_ws", self._ws)
        mp.setattr(torch, "empty", self._empty)
        mp.setattr(torch, "empty_like", self._empty_like)
        try:
            from m3l_amd import _lib as L
            lib = L.lib()
        except Exception:      # noqa: BLE001  (no library built: the CPU tests of the helper need none)
            lib = None
        if lib is not None:
            for name in L.EXPORTS:
                if name.endswith("_ws_bytes") or "_ws_bytes_" in name:
                    mp.setattr(lib, name, self._recording(name, getattr(lib, name)))
        return self

    def __exit__(self, *exc):
        self._mp.__exit__(*exc)
        self._mp = None
        self.records = []            # the blocks go back to the allocator: one context, one registry
        return False

    # ---- the check
    def violations(self):
        if "cuda" in self.device_types and torch.cuda.is_available():
            torch.cuda.synchronize()
        flags = []
        for r in self.records:
            g = r.guard
            flags.append((r.block[:g] != self.fill).any())
            flags.append((r.block[g + r.nbytes:] != self.fill).any())
        if not flags:
            return []
        hit = torch.stack(flags).cpu().tolist()
        out = []
        for i, r in enumerate(self.records):
            for side, bad in (("before", hit[2 * i]), ("after", hit[2 * i + 1])):
                if not bad:
                    continue
                g = r.guard
                region = r.block[:g] if side == "before" else r.block[g + r.nbytes:]
                first = int(torch.nonzero(region != self.fill)[0])
                # offset in bytes relative to the payload: negative = in front of its first byte, else past its last byte
                off = first - g if side == "before" else first
                out.append(dict(shape=r.shape, dtype=r.dtype, kind=r.kind, site=r.site, side=side, offset=off,
                                count=int((region != self.fill).sum())))
        return out

    def check(self, where=""):
        v = self.violations()
        if v:
            lines = [f"{x['kind']} {tuple(x['shape'])} {x['dtype']} allocated at {x['site'][0]}:{x['site'][1]}: {x['count']} guard byte(s) changed "
                     f"{x['side']} the payload, first at byte offset {x['offset']:+d} "
                     f"({'from its start' if x['side'] == 'before' else 'past its end'})" for x in v]
            raise GuardViolation(f"write outside a buffer{(' ' + where) if where else ''} (fill 0x{self.fill:02X}):\n  " + "\n  ".join(lines))


def _default_device():
    get = getattr(torch, "get_default_device", None)
    return get() if get is not None else torch.device("cpu")


class NoGuard:
    """Stands in for a MemGuard in the unguarded run of a workload."""
    fill = None

    def check(self, where=""):
        pass

    def alloc(self, shape, dtype, device, kind="tensor", site=None):
        return _REAL_EMPTY(shape, dtype=dtype, device=device)


def flatten(out, prefix=""):
    """{name: tensor} of a nested dict / list / tuple of tensors (None entries dropped)."""
    flat = {}
    if isinstance(out, torch.Tensor):
        flat[prefix or "out"] = out
    elif isinstance(out, dict):
        for k, v in out.items():
            flat.update(flatten(v, f"{prefix}.{k}" if prefix else str(k)))
    elif isinstance(out, (list, tuple)):
        for i, v in enumerate(out):
            flat.update(flatten(v, f"{prefix}[{i}]"))
    elif isinstance(out, (bool, int, float)):
        flat[prefix or "out"] = torch.tensor(out, dtype=torch.float64)
    elif out is not None:
        raise TypeError(f"{prefix}: {type(out).__name__}")
    return flat


def clone_out(out):
    """Detached copies that own their memory (made with the real allocator: call it before the context closes)."""
    return {k: v.detach().clone() for k, v in flatten(out).items()}


def differing(a, b):
    """Names whose tensors are not bit-identical (torch.equal: a NaN differs from everything, so poison that was read shows)."""
    a, b = flatten(a), flatten(b)
    bad = sorted(set(a) ^ set(b))
    for k in a:
        if k in b and not (a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k])):
            bad.append(k)
    return bad


def nonfinite(out):
    return [k for k, v in flatten(out).items() if v.dtype.is_floating_point and not bool(torch.isfinite(v).all())]


def run_contract(monkeypatch, work, device_types=("cuda",), callers="m3l_amd", need_ws=True, fills=FILLS):
    """The contract for one workload.  work(g) runs it once — g is a MemGuard (or a NoGuard in the first, unguarded run); it calls
    g.check() wherever it wants the guards looked at (after the forward, after the backward) and returns its results as a nested
    dict / list of tensors.  Asserts: bit-identical results across the unguarded run and one guarded run per fill, all finite, guards
    intact, something was guarded, every workspace request had the size its *_ws_bytes function returned.  Returns the guards' counts."""
    ref = clone_out(work(NoGuard()))
    bad = nonfinite(ref)
    assert not bad, f"non-finite results in the unguarded run: {bad}"
    counts = []
    for fill in fills:
        with MemGuard(monkeypatch, fill, device_types=device_types, callers=callers) as g:
            out = work(g)
            g.check("at the end of the run")
            got = clone_out(out)
            counts.append((g.n_ws, g.n_tensors))
            assert g.n_tensors > 0, "no tensor allocation went through the guard"
            assert g.n_ws > 0 or not need_ws, "no workspace request went through the guard"
            assert not g.ws_unmatched, f"workspace requests that no *_ws_bytes call sized: {g.ws_unmatched}"
        bad = nonfinite(got)
        assert not bad, f"non-finite results with memory pre-filled with 0x{fill:02X}: {bad}"
        bad = differing(ref, got)
        assert not bad, f"results depend on what memory held before the call (fill 0x{fill:02X} vs unguarded): {bad}"
    return counts
