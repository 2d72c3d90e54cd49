"""Poisoned, red-zoned buffers for the kernel tests (test code only: no kernels, no allocator settings).

Inside a `Guard` scope every `torch.empty` / `torch.empty_like` for a guarded device is replaced by an allocation that
  * is filled with a pattern chosen per scope - A: the 32-bit word 0x7FC0BEEF (a quiet NaN with a recognisable payload as
    float, a large positive number as int32 / int64), B: all-zero bits - through an integer view, so the payload survives;
  * lies between two red zones of 64 KiB of pattern A (a design choice: wider than a mis-indexed row of the test shapes,
    and a multiple of 512 bytes so that the data pointer keeps the allocator's alignment);
  * reports storage_offset() 0 and the strides / contiguity of the plain result (the binding derives `x_lead` and
    plane-ness from them): it is a DLPack re-import of the middle of the backing buffer, not a slice view.
The backing buffers are held until the scope ends (so the caching allocator recycles nothing inside it); then, after one
synchronize, every red zone must still be pattern A bit for bit and every ticket counter of `_native._sync_bufs` zero.
A violation names the allocation site, the side and the first and last damaged byte.

While the current stream is capturing, allocations pass straight through (captured graphs stay the production ones).
Not seen: reads whose value is discarded, writes further than 64 KiB from a buffer, memory allocated from C++ or under
capture, `torch.zeros` (its contract is "cleared") - DESIGN.md 14.
"""
import atexit
import collections
import linecache
import os
import sys

import pytest
import torch
from torch.utils import dlpack as _dlpack

PATTERN_A = 0x7FC0BEEF
ZONE = 64 * 1024                    # bytes on each side
assert ZONE % 512 == 0
_HERE = os.path.abspath(__file__)

_stack = []                         # active scopes, innermost last
_saved = None                       # (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like) of the unpatched module
                                    # while a scope is active
totals = {"scopes": 0, "allocations": 0, "data_bytes": 0, "passed_through_capture": 0}


class GuardViolation(AssertionError):
    pass


def _site():
    f = sys._getframe(2)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    return ("?", 0) if f is None else (f.f_code.co_filename, f.f_lineno)


def _capturing(device):
    return device.type == "cuda" and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class Guard:
    """Context manager; `pattern` "A" or "B"; `devices`: device types whose allocations are guarded."""

    def __init__(self, pattern="A", devices=("cuda",), check_sync_bufs=True):
        assert pattern in ("A", "B")
        self.pattern, self.devices, self.check_sync_bufs = pattern, tuple(devices), check_sync_bufs
        self.records = []           # (backing uint8 tensor, data bytes, site)
        self.allocations = 0
        self.data_bytes = 0
        self._tmpl = {}
        # call sites seen: ("empty" | "zeros", file, line) -> count.  torch.zeros / torch.zeros_like are only observed
        # (their contract is "cleared"): a test can assert that both arms of a "zeros if ... else empty" decision ran
        self.sites = collections.Counter()

    def source_lines(self, kind):
        """the source text of the call sites of `kind` ("empty" / "zeros") seen in this scope"""
        return {linecache.getline(f, n).strip() for (k, f, n) in self.sites if k == kind}

    # ---- allocation ---------------------------------------------------------------------------------------
    def _template(self, device):
        t = self._tmpl.get(device)
        if t is None:
            t = _saved[0]((ZONE + 4) // 4, dtype=torch.int32, device=device).fill_(PATTERN_A).view(torch.uint8)
            self._tmpl[device] = t
        return t

    def wants(self, device, kwargs):
        if device.type not in self.devices or kwargs.get("pin_memory") or kwargs.get("out") is not None:
            return False
        if kwargs.get("layout", torch.strided) is not torch.strided:
            return False
        return True

    def allocate(self, meta, device, requires_grad, site):
        """A guarded tensor with the size / stride / dtype of `meta` (the plain call's result on the meta device)."""
        nbytes = meta.numel() * meta.element_size()
        total = ZONE + (nbytes + 3) // 4 * 4 + ZONE
        backing = _saved[0](total // 4, dtype=torch.int32, device=device)
        backing.fill_(PATTERN_A)
        backing = backing.view(torch.uint8)
        data = backing[ZONE:ZONE + nbytes]
        if self.pattern == "B":
            data.zero_()
        # storage offset 0 over the middle of the backing buffer; the capsule keeps the backing storage alive
        flat = _dlpack.from_dlpack(_dlpack.to_dlpack(data)).view(meta.dtype)
        assert flat.storage_offset() == 0 and flat.data_ptr() == backing.data_ptr() + ZONE
        out = _saved[0](0, dtype=meta.dtype, device=device).set_(flat.untyped_storage(), 0, meta.size(), meta.stride())
        assert out.data_ptr() == flat.data_ptr() and out._base is None
        if requires_grad:
            out.requires_grad_()
        self.records.append((backing, nbytes, site))
        self.sites[("empty",) + tuple(site)] += 1
        self.allocations += 1
        self.data_bytes += nbytes
        return out

    # ---- scope --------------------------------------------------------------------------------------------
    def __enter__(self):
        global _saved
        if not _stack:
            _saved = (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like)
            torch.empty, torch.empty_like, torch.zeros, torch.zeros_like = _empty, _empty_like, _zeros, _zeros_like
        _stack.append(self)
        return self

    def __exit__(self, et, ev, tb):
        global _saved
        assert _stack and _stack[-1] is self
        try:
            if et is None:
                self.check()
        finally:
            _stack.pop()
            if not _stack:
                torch.empty, torch.empty_like, torch.zeros, torch.zeros_like = _saved
                _saved = None
            totals["scopes"] += 1
            totals["allocations"] += self.allocations
            totals["data_bytes"] += self.data_bytes
            self.records = []
        return False

    def violations(self):
        """[(site, side, first, last)]: red-zone bytes that are no longer pattern A; offsets are bytes from the nearer end of
        the data (lo: 1 = the byte just in front of it; hi: 0 = the byte just behind it)."""
        if torch.cuda.is_available() and any(b.is_cuda for b, _, _ in self.records):
            torch.cuda.synchronize()
        def zone_diff(rec, side):
            backing, nbytes, _ = rec
            tmpl = self._template(backing.device)
            lo = 0 if side == "lo" else ZONE + nbytes
            return backing[lo:lo + ZONE] != tmpl[lo % 4:lo % 4 + ZONE]

        keys = [(r, side) for r in self.records for side in ("lo", "hi")]
        by_dev = {}
        for i, (r, side) in enumerate(keys):
            by_dev.setdefault(r[0].device, []).append((i, zone_diff(r, side).any().reshape(1)))
        bad = []
        for fl in by_dev.values():          # one transfer per device, not one per zone
            hit = torch.cat([f for _, f in fl]).cpu().tolist()
            bad += [i for (i, _), h in zip(fl, hit) if h]
        out = []
        for i in sorted(bad):
            r, side = keys[i]
            pos = zone_diff(r, side).nonzero().reshape(-1)
            first, last = int(pos[0]), int(pos[-1])
            if side == "lo":
                first, last = ZONE - last, ZONE - first
            out.append((r[2], side, first, last))
        return out

    def check(self):
        v = self.violations()
        if v:
            raise GuardViolation("write outside a buffer: " + "; ".join(
                "%s:%d %s red zone damaged, bytes %d..%d %s the data" % (s[0], s[1], side, a, b,
                                                                          "in front of" if side == "lo" else "behind")
                for s, side, a, b in v))
        if self.check_sync_bufs:
            from kinetic_gan_amd import _native
            for key, buf in _native._sync_bufs.items():
                nz = buf.nonzero().reshape(-1)
                if nz.numel():
                    raise GuardViolation("ticket counters of %r not back at zero: %d non-zero, first at %d"
                                         % (key, nz.numel(), int(nz[0])))


def _device_of(kwargs, like=None):
    d = kwargs.get("device")
    if d is None:
        if like is not None:
            return like.device
        d = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
    d = torch.device(d)
    if d.type == "cuda" and d.index is None and torch.cuda.is_available():
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def _empty(*args, **kwargs):
    g = _stack[-1]
    device = _device_of(kwargs)
    if not g.wants(device, kwargs):
        return _saved[0](*args, **kwargs)
    if _capturing(device):
        totals["passed_through_capture"] += 1
        return _saved[0](*args, **kwargs)
    kw = dict(kwargs)
    kw["device"] = "meta"
    rg = kw.pop("requires_grad", False)
    meta = _saved[0](*args, **kw)
    if meta.numel() == 0:
        return _saved[0](*args, **kwargs)
    return g.allocate(meta, device, rg, _site())


def _empty_like(inp, **kwargs):
    g = _stack[-1]
    device = _device_of(kwargs, like=inp)
    if not g.wants(device, kwargs) or inp.layout is not torch.strided:
        return _saved[1](inp, **kwargs)
    if _capturing(device):
        totals["passed_through_capture"] += 1
        return _saved[1](inp, **kwargs)
    kw = dict(kwargs)
    kw["device"] = "meta"
    rg = kw.pop("requires_grad", False)
    meta = _saved[1](inp, **kw)
    if meta.numel() == 0:
        return _saved[1](inp, **kwargs)
    return g.allocate(meta, device, rg, _site())


def _zeros(*args, **kwargs):
    _stack[-1].sites[("zeros",) + tuple(_site())] += 1
    return _saved[2](*args, **kwargs)


def _zeros_like(*args, **kwargs):
    _stack[-1].sites[("zeros",) + tuple(_site())] += 1
    return _saved[3](*args, **kwargs)


def empty(*args, **kwargs):
    """`torch.empty` through the innermost active scope (plain `torch.empty` outside one): for a test's own `out=` buffers
    and workspaces."""
    return torch.empty(*args, **kwargs)


def empty_like(t, **kwargs):
    return torch.empty_like(t, **kwargs)


def zeros(*size, **kwargs):
    """`torch.zeros` as a guarded buffer: cleared by the test, red-zoned by the harness"""
    return torch.empty(*size, **kwargs).zero_()


def full(size, fill_value, **kwargs):
    """`torch.full` as a guarded buffer (an accumulate-into destination, or an output pre-filled by the test)"""
    if kwargs.get("dtype") is None:
        kwargs["dtype"] = torch.tensor(fill_value).dtype
    return torch.empty(size, **kwargs).fill_(fill_value)


def ones(*size, **kwargs):
    return torch.empty(*size, **kwargs).fill_(1)


def poison_count(t):
    """number of aligned 32-bit words of `t` that hold pattern A"""
    t = t.detach()
    if t.numel() == 0:
        return 0
    raw = t.contiguous().reshape(-1).view(torch.uint8)
    raw = raw[:raw.numel() // 4 * 4]
    if raw.numel() == 0:
        return 0
    if raw.data_ptr() % 4:
        raw = raw.clone()
    return int((raw.view(torch.int32) == PATTERN_A).sum())


def assert_no_poison(t, what=""):
    n = poison_count(t)
    assert n == 0, "%s%d of %d elements were never written (they still hold the poison word 0x%08X)" % (
        what + ": " if what else "", n, t.numel(), PATTERN_A)


@pytest.fixture
def guarded():
    """the test body runs under pattern A and red zones; the check runs when the test ends"""
    with Guard("A") as g:
        yield g


@pytest.fixture(autouse=True)
def guard_all():
    """import into a module to put every test of it under pattern A and red zones"""
    with Guard("A") as g:
        yield g


def _write_totals():
    path = os.environ.get("KG_GUARD_STATS")
    if path and totals["scopes"]:
        with open(path, "a") as f:
            f.write("guard pid %d: %d scopes, %d allocations poisoned and red-zoned, %d data bytes, %d passed through under capture\n"
                    % (os.getpid(), totals["scopes"], totals["allocations"], totals["data_bytes"],
                       totals["passed_through_capture"]))


atexit.register(_write_totals)
