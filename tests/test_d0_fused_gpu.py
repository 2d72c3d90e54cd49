"""-m gpu: discriminator block 0 with its label bias formed inside the gcn launch (kg_aggconv_label) and the two-launch
kg_label_bias_bwd, against their plain-torch definitions (oracle/prim_ref.py), and the critic trunk on either block-0
route through the bench-path comparison with the host oracle."""
import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd import disc_trunk
from kinetic_gan_amd._native import WView
from oracle import prim_ref as pr
from tests import guard
from tests.guard import guard_all  # noqa: F401  (autouse: every test of this module runs on poisoned, red-zoned buffers)

pytestmark = pytest.mark.gpu
TOL = 2e-5          # the project's kernel tolerance (tests/test_kernels_gpu.py): |a-b| <= TOL * max|ref|
K, M = 3, 32        # block 0: three partitions, 32 output channels


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def layouts(x):
    """the same logical tensor in NCHW and in channel-major storage"""
    cm = x.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
    return [("nchw", x.contiguous()), ("cntv", cm)]


def close(a, b, tol, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    print(f"{what} max err {err:.3e} ref max {ref:.3e} rel {err / max(ref, 1e-30):.2e} (bound {tol:.0e})")
    assert err <= tol * ref + 1e-30, f"{what} max err {err:.3e} vs ref max {ref:.3e} (rel {err / max(ref, 1e-30):.2e})"


def block0(ds, seed=1):
    """block 0's masked kept-column adjacency with live non-unit importances, its neighbour table and counts"""
    from kinetic_gan_amd.graph import build_graph
    g = build_graph(ds)
    keep = torch.as_tensor(g.keep(0))
    V = g.num_node[0]
    imp = 0.5 + torch.rand(3, V, V, generator=torch.Generator().manual_seed(seed))
    ak = (torch.as_tensor(g.As[0], dtype=torch.float32) * imp)[:, :, keep].contiguous()
    W = ak.shape[2]
    tab = torch.full((K, W, nv.AGGCONV_P), -1, dtype=torch.int32)
    pcount = [0, 0, 0]
    for k in range(K):
        for w in range(W):
            vs = torch.nonzero(ak[k, :, w]).flatten().tolist()
            pcount[k] = max(pcount[k], len(vs))
            tab[k, w, :len(vs)] = torch.tensor(vs, dtype=torch.int32)
    return ak, tab, pcount


def problem(ds, L, Cd, N, T, seed=0):
    ak, nbr, pcount = block0(ds)
    J, cin = L, L + Cd
    V = ak.shape[1]
    x = rnd(N, Cd, T, V, seed=seed + 2)
    wg = rnd(K * M, cin, 1, 1, seed=seed + 4) / (K * cin) ** 0.5
    emb = rnd(L, J, seed=seed + 3)
    labels = torch.randint(0, L, (N,), generator=torch.Generator().manual_seed(seed + 5))
    wv = WView(sT=M * cin, sO=cin, sI=1)                    # the data columns sit behind the J label columns
    return dict(ak=ak, nbr=nbr, pcount=pcount, J=J, cin=cin, x=x, wg=wg, emb=emb, labels=labels, wv=wv)


def fused(p, x, labels, want_xa, d):
    return nv.aggconv_label(x.to(d), p["ak"].to(d), p["nbr"].to(d), p["pcount"], p["wg"].reshape(-1)[p["J"]:].to(d), p["wv"],
                            M, labels.to(d), p["emb"].to(d), p["wg"].to(d), p["cin"], p["J"], want_xa=want_xa)


# (dataset, classes L = label channels J, data channels, N, T): h36m / ntu / ntu120 class counts, both clip lengths,
# ragged sample counts (workgroups of two threads per column) and 192 samples (one thread per column)
FWD_CASES = [(ds, L, cd, n, T) for (ds, L, cd) in [("h36m", 10, 2), ("ntu", 60, 3), ("ntu", 120, 3)]
             for (n, T) in [(13, 64), (5, 256)]] + [("ntu", 60, 3, 192, 64)]


@pytest.mark.parametrize("ds,L,Cd,N,T", FWD_CASES)
def test_aggconv_label_vs_definition(ds, L, Cd, N, T):
    """z = sum_k W_k (x A_k) + bias[label_n] in one launch against prim_ref.aggconv(add=prim_ref.label_bias_fwd(...),
    add_tstride=0), with and without the aggregated planes, NCHW and channel-major inputs."""
    d = dev()
    p = problem(ds, L, Cd, N, T)
    zl = pr.label_bias_fwd(p["labels"], p["emb"], p["wg"], K, M, p["cin"], p["J"], p["ak"])
    for want_xa in (True, False):
        ro, rxa = pr.aggconv(p["x"], p["ak"], p["nbr"], p["pcount"], p["wg"].reshape(-1)[p["J"]:], p["wv"], M, add=zl,
                             add_tstride=0, want_xa=want_xa)
        for name, xl in layouts(p["x"]):
            out, xa = fused(p, xl, p["labels"], want_xa, d)
            close(out, ro, TOL, f"{ds} L={L} N={N} T={T} {name} xa={want_xa}: z")
            if want_xa:
                close(xa, rxa, TOL, f"{ds} L={L} N={N} T={T} {name}: xa")
            else:
                assert xa is None


@pytest.mark.parametrize("ds,L,Cd,N,T", [("ntu", 60, 3, 13, 64), ("h36m", 10, 2, 192, 64)])
def test_aggconv_label_matches_composed_launches(ds, L, Cd, N, T):
    """the bias is formed in the arithmetic order of kg_label_bias_fwd and added where kg_aggconv adds `add`: the fused
    launch reproduces the composed pair bit for bit"""
    d = dev()
    p = problem(ds, L, Cd, N, T, seed=7)
    to = lambda t: t.to(d)
    zl = nv.label_bias_fwd(to(p["labels"]), to(p["emb"]), to(p["wg"]), K, M, p["cin"], p["J"], to(p["ak"]))
    ref, rxa = nv.aggconv(to(p["x"]), to(p["ak"]), to(p["nbr"]), p["pcount"], to(p["wg"].reshape(-1)[p["J"]:]), p["wv"], M,
                          add=zl, add_tstride=0, want_xa=True)
    out, xa = fused(p, p["x"], p["labels"], True, d)
    assert torch.equal(out, ref) and torch.equal(xa, rxa)


@pytest.mark.parametrize("ds,L,Cd,N,T", [("ntu", 60, 3, 13, 64), ("h36m", 10, 2, 9, 256)])
def test_aggconv_label_out_of_range_labels(ds, L, Cd, N, T):
    """a label outside [0, L) turns exactly that sample's output into NaN (and is never used as an index); every other
    sample is bit-equal to the clean run"""
    d = dev()
    p = problem(ds, L, Cd, N, T, seed=3)
    clean, cxa = fused(p, p["x"], p["labels"], True, d)
    bad = p["labels"].clone()
    bad[0], bad[4], bad[N - 1] = L, 1 << 40, -1
    out, xa = fused(p, p["x"], bad, True, d)
    out, clean = out.cpu(), clean.cpu()
    assert torch.isfinite(clean).all()
    for i in (0, 4, N - 1):
        assert torch.isnan(out[i]).all(), i
    good = [i for i in range(N) if i not in (0, 4, N - 1)]
    assert torch.equal(out[good], clean[good])
    assert torch.equal(xa, cxa)                           # the aggregated planes do not depend on the label


def _bwd_case(ds, L, N, T, labels, seed=0):
    ak, _, _ = block0(ds, seed=seed + 1)
    Cd = 3
    J, cin = L, L + Cd
    W = ak.shape[2]
    emb, wg = rnd(L, J, seed=seed + 3), rnd(K * M, cin, 1, 1, seed=seed + 4) * 0.1
    gz = [t for _, t in layouts(rnd(N, M, T, W, seed=seed + 5))]
    return ak, J, cin, emb, wg, gz


def _run_bwd(d, gz, labels, emb, wg, J, cin, ak, accumulate=True):
    L = emb.shape[0]
    demb = guard.full((L, J), 0.5, device=d)
    dw = guard.full((K * M * cin,), 0.25, device=d)
    dak = guard.full(tuple(ak.shape), 2.0, device=d)
    nv.label_bias_bwd(gz.to(d), labels.to(d), emb.to(d), wg.to(d), K, M, cin, J, ak.to(d), demb=demb, dw=dw, dak=dak,
                      accumulate=accumulate, dak_accumulate=accumulate)
    return demb, dw, dak


BWD_CASES = [
    # dataset, L, N, T, label pattern
    ("ntu", 60, 128, 64, "random, five empty classes"),
    ("ntu", 60, 64, 64, "one class"),
    ("h36m", 10, 300, 16, "random"),                      # more samples than one 256-label chunk
    ("ntu", 120, 7, 256, "random, five empty classes"),
]


@pytest.mark.parametrize("ds,L,N,T,pattern", BWD_CASES)
def test_label_bias_bwd_two_launches(ds, L, N, T, pattern):
    """the per-(class, channel) launch + the finishing launch against prim_ref.label_bias_bwd at the existing test's
    bound (1e-4): accumulated and overwritten outputs, NCHW and channel-major gz, data columns of dw untouched, and
    two calls bit for bit"""
    d = dev()
    gen = torch.Generator().manual_seed(9)
    if pattern == "one class":
        labels = torch.full((N,), 7, dtype=torch.int64)
    elif "empty" in pattern:
        labels = torch.randint(0, L - 5, (N,), generator=gen)
    else:
        labels = torch.randint(0, L, (N,), generator=gen)
    ak, J, cin, emb, wg, gzs = _bwd_case(ds, L, N, T, labels)
    for gz in gzs:
        for accumulate in (True, False):
            demb, dw, dak = _run_bwd(d, gz, labels, emb, wg, J, cin, ak, accumulate)
            rdemb = torch.full((L, J), 0.5)
            rdw = torch.full((K * M * cin,), 0.25)
            rdak = torch.full(tuple(ak.shape), 2.0)
            pr.label_bias_bwd(gz, labels, emb, wg, K, M, cin, J, ak, demb=rdemb, dw=rdw, dak=rdak, accumulate=accumulate,
                              dak_accumulate=accumulate)
            close(demb, rdemb, 1e-4, f"{ds} L={L} N={N} {pattern} acc={accumulate}: demb")
            close(dw, rdw, 1e-4, f"{ds} L={L} N={N} {pattern} acc={accumulate}: dw")
            close(dak, rdak, 1e-4, f"{ds} L={L} N={N} {pattern} acc={accumulate}: dak")
            assert torch.equal(dw.view(K * M, cin)[:, J:].cpu(), torch.full((K * M, cin - J), 0.25))
            again = _run_bwd(d, gz, labels, emb, wg, J, cin, ak, accumulate)
            for a_, b_ in zip((demb, dw, dak), again):
                assert torch.equal(a_, b_)
    if "empty" in pattern:
        # the classes without a sample get exactly the accumulated value back
        demb, _, _ = _run_bwd(d, gzs[0], labels, emb, wg, J, cin, ak)
        assert torch.equal(demb[L - 5:].cpu(), torch.full((5, J), 0.5))


def test_label_bias_bwd_skips_out_of_range_labels():
    """samples whose label lies outside [0, L) contribute nothing (and are never used as an index)"""
    d = dev()
    L, N, T = 60, 40, 64
    labels = torch.randint(0, L, (N,), generator=torch.Generator().manual_seed(4))
    ak, J, cin, emb, wg, gzs = _bwd_case("ntu", L, N, T, labels, seed=2)
    gz = gzs[0]
    bad = labels.clone()
    bad[3], bad[17], bad[N - 1] = L, -1, 1 << 40
    got = _run_bwd(d, gz, bad, emb, wg, J, cin, ak)
    keep = [i for i in range(N) if i not in (3, 17, N - 1)]
    rdemb, rdw, rdak = torch.full((L, J), 0.5), torch.full((K * M * cin,), 0.25), torch.full(tuple(ak.shape), 2.0)
    pr.label_bias_bwd(gz[keep], labels[keep], emb, wg, K, M, cin, J, ak, demb=rdemb, dw=rdw, dak=rdak)
    for a_, b_, nm in zip(got, (rdemb, rdw, rdak), ("demb", "dw", "dak")):
        close(a_, b_, 1e-4, nm)


@pytest.mark.parametrize("fused_route", [True, False])
@pytest.mark.parametrize("cfg,n", [("ntu", 64), ("h36m", 64)])
def test_bench_path_with_and_without_fused_block0(cfg, n, fused_route, monkeypatch):
    """the bench composition against the host oracle (eager and replayed from a hipGraph) with block 0 on either route:
    kg_aggconv_label (the default) or the class table + lookup + kg_aggconv (KG_D0_FUSED=0); and that the fused entry
    really ran / did not run"""
    from tests.test_parity_gpu import _bench_path_vs_oracle
    monkeypatch.setattr(disc_trunk, "D0_FUSED", fused_route)
    calls = {"n": 0}
    f0 = nv.aggconv_label

    def counted(*a, **k):
        calls["n"] += 1
        return f0(*a, **k)
    monkeypatch.setattr(nv, "aggconv_label", counted)
    _bench_path_vs_oracle(cfg, n)
    assert (calls["n"] > 0) if fused_route else (calls["n"] == 0), calls
