"""The harness of tests/guard.py must be able to fail: run on CPU tensors with its device filter opened.

The only deliberate out-of-range writes of the suite are here, made with plain torch indexing into a guarded buffer's own
backing storage (CPU memory owned by the test).  The last part re-runs the host-logic files - where the native entry
points are the torch definitions of oracle/prim_ref.py - with every `torch.empty` / `torch.empty_like` poisoned: the Python
side of the package must not depend on uninitialised memory, so a poison failure on the GPU points at a kernel or at the
binding's "this launch writes all of it" assumptions."""
import importlib
import inspect
import itertools

import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build
from oracle import prim_ref
from tests import guard
from tests.guard import PATTERN_A, ZONE, Guard, GuardViolation, assert_no_poison
from tests.util import emulated_native

CPU = ("cpu", "cuda")


def close(a, b, tol=2e-5):
    """the comparison of tests/test_kernels_gpu.py"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= tol * ref + 1e-30, f"max err {err:.3e} vs ref max {ref:.3e}"


def test_guarded_tensor_looks_like_the_plain_one():
    like = torch.zeros(2, 3, 4, 5).permute(1, 0, 2, 3)          # channel-major, as a plane tensor
    calls = [lambda: torch.empty(3, 5), lambda: torch.empty((2, 3, 4, 5), dtype=torch.float64),
             lambda: torch.empty(7, dtype=torch.int64, device="cpu"), lambda: torch.empty(5, dtype=torch.uint8),
             lambda: torch.empty(6, dtype=torch.float16), lambda: torch.empty_like(like),
             lambda: torch.empty_like(like, dtype=torch.int32), lambda: torch.empty(4, 4, requires_grad=True)]
    plain = [c() for c in calls]
    with Guard("A", devices=CPU) as g:
        guarded = [c() for c in calls]
        assert g.allocations == len(calls)
        for p, q, rec in zip(plain, guarded, g.records):
            assert (q.shape, q.stride(), q.storage_offset(), q.dtype, q.device) == \
                   (p.shape, p.stride(), p.storage_offset(), p.dtype, p.device)
            assert q.is_contiguous() == p.is_contiguous() and q.requires_grad == p.requires_grad and q._base is None
            backing, nbytes, site = rec
            assert nbytes == p.numel() * p.element_size() and site[0] == __file__
            # the zones are whole multiples of 512 bytes: the data pointer keeps the allocator's alignment modulo 512
            assert ZONE % 512 == 0 and q.data_ptr() - backing.data_ptr() == ZONE
            assert q.data_ptr() % 512 == backing.data_ptr() % 512
            assert q.data_ptr() % 64 == p.data_ptr() % 64 == 0          # (what the CPU allocator gives)
        # a plane tensor keeps its own lead inside the data region
        pl = _native.new_plane(2, 3, 4, 5, torch.device("cpu"))
        assert pl.storage_offset() == _native.PLANE_LEAD and _native.is_plane(pl)
        assert pl.data_ptr() - g.records[-1][0].data_ptr() == ZONE + 4 * _native.PLANE_LEAD


def test_patterns_and_assert_no_poison():
    with Guard("A", devices=CPU):
        f = torch.empty(33)
        i = torch.empty(5, dtype=torch.int64)
        assert f.isnan().all() and (f.view(torch.int32) == PATTERN_A).all()
        assert (i == (PATTERN_A << 32 | PATTERN_A)).all() and (i > 0).all()
        f[:32] = 1.0                                     # one element is never written
        with pytest.raises(AssertionError, match="1 of 33 elements were never written"):
            assert_no_poison(f)
        f[32] = 2.0
        assert_no_poison(f)
        assert_no_poison(torch.full((4,), float("nan")))          # an ordinary NaN is not the poison word
    with Guard("B", devices=CPU):
        z = torch.empty(33)
        assert (z.view(torch.int32) == 0).all()


@pytest.mark.parametrize("side", ["lo", "hi"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_a_write_next_to_the_buffer_is_reported(side, dtype):
    n = 37
    with pytest.raises(GuardViolation) as e:
        with Guard("B", devices=CPU) as g:
            t = torch.empty(n, dtype=dtype)
            t.zero_()
            backing, nbytes, site = g.records[0]
            line = inspect.currentframe().f_lineno - 3
            es = t.element_size()
            assert nbytes == n * es
            # one element in front of / behind the data, written through the backing storage the test owns
            at = ZONE - es if side == "lo" else ZONE + nbytes
            backing[at:at + es] = 0
    msg = str(e.value)
    assert "%s:%d" % (__file__, line) in msg and side + " red zone" in msg
    # offsets count from the nearer end of the data: lo 1 = the byte just in front, hi 0 = the byte just behind
    assert ("bytes 1..%d in front of" % es if side == "lo" else "bytes 0..%d behind" % (es - 1)) in msg


def test_intact_zones_pass_and_far_damage_is_located():
    with Guard("A", devices=CPU) as g:
        t = torch.empty(1000)
        t.fill_(3.0)
        assert g.violations() == []
        g.records[0][0][ZONE + 4000 + 100:ZONE + 4000 + 108] = 7
        assert [(v[1], v[2], v[3]) for v in g.violations()] == [("hi", 100, 107)]
        g.records[0][0][ZONE + 4000 + 100:ZONE + 4000 + 108] = g.records[0][0][4:12]      # repair: same phase of the word
        assert g.violations() == []


def test_torch_empty_is_restored_also_after_an_exception():
    e0, l0, z0, zl0 = torch.empty, torch.empty_like, torch.zeros, torch.zeros_like
    with Guard("A", devices=CPU) as g:
        assert torch.empty is not e0 and torch.empty_like is not l0
        torch.zeros(3), torch.zeros_like(torch.ones(2))          # observed (call sites), not replaced
        assert g.allocations == 0 and len(g.source_lines("zeros")) == 1
        with Guard("B", devices=CPU):                   # scopes nest: the innermost pattern applies
            assert (torch.empty(3) == 0).all()
        assert torch.empty(3).isnan().all()
    assert torch.empty is e0 and torch.empty_like is l0
    with pytest.raises(ZeroDivisionError):
        with Guard("A", devices=CPU):
            1 / 0
    assert torch.empty is e0 and torch.empty_like is l0
    with pytest.raises(GuardViolation):
        with Guard("A", devices=CPU) as g:
            torch.empty(4)
            g.records[0][0][0] = 0
    assert torch.empty is e0 and torch.empty_like is l0 and not guard._stack
    assert torch.zeros is z0 and torch.zeros_like is zl0


def test_other_allocations_are_untouched():
    with Guard("A") as g:                               # the default filter: device tensors only
        a = torch.empty(16)
        b = torch.empty_like(a)
        c = torch.empty(16, device="meta")
        assert g.allocations == 0 and not g.records and a.device.type == b.device.type == "cpu" and c.is_meta
    with Guard("A", devices=CPU) as g:
        out = torch.zeros(4)
        assert torch.empty(4, out=out) is out and torch.empty(0).numel() == 0
        assert (torch.zeros(8) == 0).all() and (torch.ones(8) == 1).all()
        assert g.allocations == 0
        if torch.cuda.is_available():                   # (pinned host buffers: the feeder's and the checkpoint writer's)
            p = torch.empty(16, pin_memory=True)
            assert p.is_pinned() and g.allocations == 0


def _mix3_last_row_unwritten(real, fake, alpha):
    """kg_mix3's definition with a tile-edge bug: the last sample of the result is never written"""
    ref = prim_ref.mix3(real, fake, alpha)
    out = torch.empty(ref.shape, dtype=ref.dtype, device=ref.device)
    out[:-1] = ref[:-1]
    return out


@pytest.mark.parametrize("pattern", ["A", "B"])
def test_an_unwritten_row_hides_behind_lucky_memory_but_not_behind_poison(pattern, monkeypatch):
    """The masking the harness exists to remove.  The last sample's right answer is what the memory happens to hold (all
    zeros: real and fake end with a zero sample) - as when the caching allocator hands back the block that the previous
    kernel path filled with the same answer.  Under pattern B the broken entry point passes close(); under pattern A
    close() fails (NaN <= x is false) and assert_no_poison names the cause."""
    g0 = torch.Generator().manual_seed(0)
    real, fake, alpha = torch.randn(3, 2, 4, 5, generator=g0), torch.randn(3, 2, 4, 5, generator=g0), torch.rand(3, generator=g0)
    real[-1] = 0
    fake[-1] = 0
    want = prim_ref.mix3(real, fake, alpha)
    with emulated_native():
        assert _native.mix3 is prim_ref.mix3
        monkeypatch.setattr(_native, "mix3", _mix3_last_row_unwritten)
        with Guard(pattern, devices=CPU):
            got = _native.mix3(real, fake, alpha)
            if pattern == "B":
                close(got, want)
                assert_no_poison(got)
            else:
                with pytest.raises(AssertionError, match="max err nan"):
                    close(got, want)
                with pytest.raises(AssertionError, match="40 of 360 elements were never written"):
                    assert_no_poison(got)
        monkeypatch.undo()
        with Guard("A", devices=CPU):                   # the entry point as defined passes under poison
            close(_native.mix3(real, fake, alpha), want)


# ---- the host-logic files once more, under pattern A ---------------------------------------------------------------------
# module -> context its own autouse fixture provides (None: the module has no autouse fixture)
HOST_LOGIC = {"tests.test_host_logic_cpu": emulated_native, "tests.test_train_cpu": None,
              "tests.test_sampler_cpu": None, "tests.test_ema_cpu": None}


def _cases():
    out = []
    for modname in HOST_LOGIC:
        mod = importlib.import_module(modname)
        for name, fn in vars(mod).items():
            if not name.startswith("test_") or not inspect.isfunction(fn):
                continue
            axes = []
            for m in getattr(fn, "pytestmark", []):
                assert m.name == "parametrize", (modname, name, m.name)      # (a skip / xfail mark would need restating here)
                names = [s.strip() for s in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
                axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in m.args[1]])
            for combo in itertools.product(*axes):
                kw = {}
                for d in combo:
                    kw.update(d)
                out.append(pytest.param(modname, name, kw, id="%s::%s[%s]" % (modname.split(".")[-1], name,
                                                                               "-".join(str(v) for v in kw.values()))))
    return out


HOST_CASES = _cases()


@pytest.fixture(scope="module")
def lib():
    """(the module fixture of test_sampler_cpu / test_ema_cpu)"""
    build.build()
    return _native.load_library()


def test_host_logic_case_count_does_not_drop():
    assert len(HOST_CASES) >= 67, len(HOST_CASES)


@pytest.mark.parametrize("modname,name,kw", HOST_CASES)
def test_host_logic_does_not_depend_on_uninitialised_memory(modname, name, kw, request):
    fn = getattr(importlib.import_module(modname), name)
    args = dict(kw)
    for p in inspect.signature(fn).parameters:
        if p not in args:
            args[p] = request.getfixturevalue(p)         # tmp_path, monkeypatch, golden_dir, lib
    ctx = HOST_LOGIC[modname]
    with Guard("A", devices=CPU) as g:
        if ctx is None:
            fn(**args)
        else:
            with ctx():
                fn(**args)
    request.config.stash.setdefault(_POISONED, []).append(g.allocations)


_POISONED = pytest.StashKey()


def test_host_logic_rerun_poisoned_allocations(request):
    """(runs after the cases above: they did go through the harness)"""
    counts = request.config.stash.get(_POISONED, [])
    if len(counts) == len(HOST_CASES):                  # the whole file ran, not a -k selection
        assert sum(counts) > 5000, sum(counts)
