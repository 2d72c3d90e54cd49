"""Nearest-neighbour search and memorisation scores without a GPU: the float64 definition (tests/nn_def.py) on a hand-worked
example, the argument checks and workspace size of kg_nn, metrics.nearest / memorisation / nn_two_sample with the binding
replaced by the definition, and the condition that keeps the GPU tests' error model honest."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build
from kinetic_gan_amd import metrics

import abi_layout
import nn_def
import prdc_def

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


@pytest.fixture
def on_definition(monkeypatch):
    """metrics on the CPU: _native.nn is the definition, and nothing is moved to a device"""
    calls = []

    def nn(*args, **kw):
        calls.append((args, kw))
        return nn_def.native_nn(*args, **kw)

    monkeypatch.setattr(_native, "nn", nn)
    monkeypatch.setattr(metrics, "_as_cuda", metrics._as_f32)
    return calls


def test_header_declares_and_library_exports(lib):
    header = open(os.path.join(ROOT, "include", "kgan_hip.h")).read()
    for sym in ("kg_nn_workspace_bytes", "kg_nn"):
        assert "%s(const KgNnArgs* a" % sym in header
        assert getattr(lib, sym) is not None and sym in _native.EXPORTS
    assert "#define KG_NN_MAX_K 32" in header and _native.NN_MAX_K == 32
    assert "#define KG_NN_MAX_POINTS %d" % _native.NN_MAX_POINTS in header and _native.NN_MAX_POINTS == 1 << 24
    assert "kg_nn.hip" in build.SOURCES


def test_abi_version_unchanged(lib):
    assert lib.kg_abi_version() == 9


def test_nn_struct_matches_header():
    abi_layout.assert_mirror("KgNnArgs")


def _valid_args():
    a = _native._NnArgs()
    a.query, a.base = 0x1000, 0x2000
    a.q_sc, a.q_sp, a.q_so = 0, 4800, 0
    a.b_sc, a.b_sp, a.b_so = 0, 4800, 0
    a.Q, a.N, a.d_outer, a.d_inner, a.classes, a.k = 100, 90, 3, 1600, 2, 5
    a.tile, a.split = 32, 4
    a.idx, a.d2, a.ws = 0x3000, 0x4000, 0x5000
    return a


@pytest.mark.parametrize("field,value,needle", [
    ("query", None, b"null pointer query"), ("base", None, b"null pointer base"), ("idx", None, b"null pointer idx"),
    ("d2", None, b"null pointer d2"), ("ws", None, b"null pointer ws"),
    ("Q", 0, b"Q=0"), ("N", 0, b"N=0"), ("N", -3, b"N=-3"), ("classes", 0, b"classes=0"), ("d_outer", 0, b"d_outer=0"),
    ("d_inner", 0, b"d_inner=0"), ("k", 0, b"k=0"), ("k", 33, b"k=33"), ("N", 4, b"k=5 > N=4"),
    ("tile", 16, b"tile=16"), ("tile", -1, b"tile=-1"), ("split", -1, b"split=-1"),
    ("split", _native.NN_MAX_SPLIT + 1, b"split=%d" % (_native.NN_MAX_SPLIT + 1)), ("N", 3, b"k=5 > N=3"),
    ("ws_bytes", 64, b"ws_bytes=64"),
    ("Q", _native.NN_MAX_POINTS + 1, b"Q=%d above the cap" % (_native.NN_MAX_POINTS + 1)),
    ("N", _native.NN_MAX_POINTS + 1, b"N=%d above the cap" % (_native.NN_MAX_POINTS + 1))])
def test_kg_nn_rejects_bad_arguments_without_gpu(lib, field, value, needle):
    a = _valid_args()
    need = lib.kg_nn_workspace_bytes(ctypes.byref(a))
    assert need == 2 * 100 * 4 * 5 * 8
    a.ws_bytes = need
    setattr(a, field, value)
    if field not in ("query", "base", "idx", "d2", "ws", "ws_bytes"):
        assert lib.kg_nn_workspace_bytes(ctypes.byref(a)) < 0
        assert needle in lib.kg_last_error(), lib.kg_last_error()
    assert lib.kg_nn(ctypes.byref(a), None) < 0
    assert needle in lib.kg_last_error(), lib.kg_last_error()


def test_k_limits_and_exclude_self(lib):
    """k = N passes, k = N with exclude_self is refused by name, k = N - 1 passes with it; split may not exceed N"""
    f = _native.nn_workspace_bytes
    assert f(7, 20, 1, 7, 1, 20, split=1) == 7 * 20 * 8
    assert f(20, 20, 1, 7, 1, 19, exclude_self=True, split=1) == 20 * 19 * 8
    with pytest.raises(RuntimeError, match=r"k=20 > N=20 - 1 neighbours \(exclude_self=1\)"):
        f(20, 20, 1, 7, 1, 20, exclude_self=True)
    with pytest.raises(RuntimeError, match="split=21"):
        f(20, 20, 1, 7, 1, 1, split=21)
    assert f(40, 33, 1, 3, 1, 32, split=4) == 40 * 4 * 32 * 8


def test_workspace_formula_and_automatic_plan(lib):
    """classes * Q * split * k * 8 with the forced split; the automatic plan takes chunks of whole column tiles, at most
    NN_MAX_SPLIT of them, and none where the row tiles fill the chip alone; nothing grows with Q x N"""
    f = _native.nn_workspace_bytes
    for classes, Q, N, k, split in ((1, 40, 40, 3, 3), (3, 53, 37, 5, 5), (2, 150, 300, 5, 2), (1, 6000, 40000, 1, 6)):
        assert f(Q, N, 3, 1600, classes, k, split=split) == classes * Q * split * k * 8
        assert f(Q, N, 3, 1600, classes, k, tile=64, split=split) == f(Q, N, 3, 1600, classes, k, tile=32, split=split)
    auto = lambda Q, N, c=1, k=5: f(Q, N, 1, 75, c, k) // (c * Q * k * 8)      # noqa: E731  (the plan's split)
    assert auto(6000, 40000) == 7               # 94 row tiles of 64: 7 chunks of 104 column tiles make 658 workgroups
    assert auto(70, 40000) == _native.NN_MAX_SPLIT
    assert auto(40000, 40000) == 1              # 625 row tiles of 64 fill the chip
    assert auto(40, 40) == 2 and auto(10, 10) == 1
    assert auto(100, 100, c=60) == 4            # 240 row tiles of 32, 4 column tiles
    for Q, N in ((1, 1), (5, 1 << 24), (1 << 24, 5), (4096, 4096)):
        s = auto(Q, N, k=1)
        assert 1 <= s <= min(_native.NN_MAX_SPLIT, N)


def test_launches_of_2_to_24_workgroups_are_rejected(lib):
    """the search launch has classes x row tiles x split workgroups and stays below 2^24 of them, as does the merge launch"""
    big = _native.NN_MAX_POINTS
    assert _native.nn_workspace_bytes(big, 100, 1, 7, 1, 1, tile=64, split=1) == big * 8
    with pytest.raises(RuntimeError, match=r"classes=1 x Q=16777216 x split=32 make \d+ workgroups"):
        _native.nn_workspace_bytes(big, 100, 1, 7, 1, 1, tile=32, split=32)
    # the merge launch has a wave per query, four to a workgroup: 3 classes of 2^24 queries pass, 4 are 2^24 workgroups
    assert _native.nn_workspace_bytes(big, 100, 1, 7, 3, 1, tile=64, split=1) == 3 * big * 8
    with pytest.raises(RuntimeError, match="classes=4 .* make 16777216 workgroups"):
        _native.nn_workspace_bytes(big, 100, 1, 7, 4, 1, tile=64, split=1)


def test_definition_hand_worked_example():
    """1-D.  base = 0, 4, 2, 2, 9 (2 twice: a duplicate), queries = 3, 2, 10.
    q = 3: d2 = 9 1 1 1 36 -> the three ties at 1 in index order 1, 2, 3, then 0.
    q = 2: d2 = 4 4 0 0 49 -> the duplicates at 0 (2, 3), then the tie at 4 (0, 1).
    q = 10: d2 = 100 36 64 64 1 -> 4, 1, 2, 3."""
    b = torch.tensor([[0.0], [4.0], [2.0], [2.0], [9.0]])
    q = torch.tensor([[3.0], [2.0], [10.0]])
    out = nn_def.knn(q, b, 4)
    assert out["idx"].tolist() == [[1, 2, 3, 0], [2, 3, 0, 1], [4, 1, 2, 3]]
    assert out["d2"].tolist() == [[1, 1, 1, 9], [0, 0, 4, 4], [1, 36, 64, 64]]
    # the set against itself: without exclude_self every point finds itself first (the duplicate finds the LOWER twin first);
    # with it the pair i == j is left out by index, so a twin is the neighbour at 0 and never the point itself
    assert nn_def.knn(b, b, 1)["idx"][:, 0].tolist() == [0, 1, 2, 2, 4]
    loo = nn_def.knn(b, b, 2, exclude_self=True)
    assert loo["idx"].tolist() == [[2, 3], [2, 3], [3, 0], [2, 0], [1, 2]]
    assert loo["d2"].tolist() == [[4, 4], [4, 4], [0, 4], [0, 4], [25, 49]]
    assert nn_def.knn(b, b, 4, exclude_self=True)["idx"][0].tolist() == [2, 3, 1, 4]       # k = N - 1
    # decided: q = 10 has its first two distances (1, 36) apart and a tie (64, 64) further on; the others tie at once
    assert nn_def.knn(q, b, 3, t=nn_def.tau(1))["decided"].tolist() == [False, False, False]
    assert nn_def.knn(q, b, 1, t=nn_def.tau(1))["decided"].tolist() == [False, False, True]


def _view(x):
    """(K, n, D) contiguous -> the view _native.nn takes"""
    return _native.PrdcView(x, x.stride(0), x.stride(1), 0)


def test_definition_behind_the_binding_reads_views_and_affines():
    """nn_def.native_nn reads what kg_nn reads: strided crops, and the affine as two fp32 roundings on the set only"""
    g = torch.Generator().manual_seed(0)
    long = torch.randn((9, 3, 8, 5), generator=g)
    crop = long[:, :, :6]
    flat = crop.reshape(1, 9, 90).contiguous()
    v = _native.PrdcView(long, 0, long.stride(0), long.stride(1))
    i1, d1 = nn_def.native_nn(v, v, 9, 9, 3, 30, 1, 3, exclude_self=True)
    i2, d2 = nn_def.native_nn(_view(flat), _view(flat), 9, 9, 1, 90, 1, 3, exclude_self=True)
    assert torch.equal(i1, i2) and torch.equal(d1, d2)
    scale, shift = 0.37, -1.25
    norm = flat.mul(scale).add(shift)
    i3, d3 = nn_def.native_nn(_view(norm), _view(flat), 9, 9, 1, 90, 1, 3, b_affine=(scale, shift))
    i4, d4 = nn_def.native_nn(_view(norm), _view(norm), 9, 9, 1, 90, 1, 3)
    assert torch.equal(i3, i4) and torch.equal(d3, d4) and d3[0, :, 0].eq(0).all()


# the real-valued shapes of tests/test_nn_gpu.py (Q, N, D, k)
GPU_REAL_SHAPES = [(200, 300, 75, 5), (70, 130, 4800, 5), (300, 700, 4800, 5), (65, 257, 48, 32), (128, 1000, 2048, 8)]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("Q,N,D,k", GPU_REAL_SHAPES)
def test_error_model_decides_almost_every_query(Q, N, D, k, seed):
    """asserted on the definition alone: at most 5 % of the queries are undecided at every real-valued GPU shape"""
    b, q = prdc_def.make_data(seed, 1, N, Q, D)
    share = nn_def.undecided_share(q, b, k)
    print("undecided", Q, N, D, k, seed, share)
    assert share <= 0.05


def test_nearest_argument_errors_without_gpu():
    x = torch.zeros(12, 2, 4, 3)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.nearest(x, torch.zeros(12, 2, 5, 3))
    with pytest.raises(ValueError, match=r"\(N, C, T, V\)"):
        metrics.nearest(x[0], x)
    ragged = [0] * 5 + [1] * 7
    with pytest.raises(ValueError, match="nearest: class 1 has 7 base samples"):
        metrics.nearest(x, x, labels_query=[0] * 6 + [1] * 6, labels_base=ragged)
    with pytest.raises(ValueError, match="class 0 has 5 query samples, per_class=6"):
        metrics.nearest(x, x, labels_query=ragged, labels_base=[0] * 6 + [1] * 6, per_class=6)
    with pytest.raises(ValueError, match="11 labels_query for 12 samples"):
        metrics.nearest(x, x, labels_query=[0] * 11)
    with pytest.raises(ValueError, match="k=13 outside"):
        metrics.nearest(x, x, k=13)
    with pytest.raises(ValueError, match=r"k=12 outside \[1, min\(32, N=12 - 1\)\]"):
        metrics.nearest(x, x, k=12, exclude_self=True)
    with pytest.raises(ValueError, match="k=33 outside"):
        metrics.nearest(torch.zeros(40, 1, 1, 2), torch.zeros(40, 1, 1, 2), k=33)
    away = types.SimpleNamespace(fits=False, data=None, labels=None, scale=1.0, shift=0.0)
    with pytest.raises(ValueError, match="ResidentDataset given as base does not fit"):
        metrics.nearest(x, away)
    other = types.SimpleNamespace(fits=True, data=torch.zeros(12, 2, 6, 3), labels=torch.zeros(12, dtype=torch.int64),
                                  scale=0.5, shift=-1.0)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.nearest(x, other)


def test_memorisation_and_two_sample_argument_errors_without_gpu():
    x = torch.zeros(12, 2, 4, 3)
    lab = [0, 1] * 6
    with pytest.raises(ValueError, match="labels_train is needed"):
        metrics.memorisation(x, lab, x)
    with pytest.raises(ValueError, match="labels_heldout is needed"):
        metrics.memorisation(x, lab, x, lab, heldout=x)
    with pytest.raises(ValueError, match="heldout samples .* and train samples .* differ in shape"):
        metrics.memorisation(x, lab, x, lab, heldout=torch.zeros(3, 2, 5, 3), labels_heldout=[0] * 3)
    with pytest.raises(ValueError, match="11 labels_gen for 12 samples"):
        metrics.memorisation(x, lab[:11], x, lab)
    with pytest.raises(ValueError, match="at least 2 training samples"):
        metrics.memorisation(x, lab, x[:1], [0])
    with pytest.raises(ValueError, match=r"train_loo must be the \(12,\) fp32"):
        metrics.memorisation(x, lab, x, lab, train_loo=torch.zeros(11))
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.nn_two_sample(x, torch.zeros(12, 2, 5, 3))
    with pytest.raises(ValueError, match=r"6 real and 4 fake samples per class \(the test needs \|R\| = \|F\|"):
        metrics.nn_two_sample(x[:8], x, [0, 1] * 4, lab)
    with pytest.raises(ValueError, match="class 1 has 7 real samples"):
        metrics.nn_two_sample(x, x, lab, [0] * 5 + [1] * 7)
    with pytest.raises(ValueError, match="needs 2"):
        metrics.nn_two_sample(x[:2], x[:2], [0, 1], [0, 1])
    assert metrics.NN_TWO_SAMPLE_NAMES == ("acc_real", "acc_fake", "acc")


def test_nearest_on_the_definition(on_definition):
    """global and class-by-class searches, the index back into the base batch, a ResidentDataset read in place"""
    train, lab_t, gen, lab_g, copied = nn_def.planted(0, 60, 24, 3, 5, 5, 3)
    out = metrics.nearest(gen, train, k=2)
    assert out["idx"].shape == (1, 24, 2) and out["index"][0, :6, 0].tolist() == copied.tolist()
    ref = nn_def.knn(torch.tensor(gen).reshape(24, -1), torch.tensor(train).reshape(60, -1), 2)
    assert torch.equal(out["idx"][0].long(), ref["idx"]) and torch.equal(out["d2"][0], ref["d2"].float())
    # with labels: class c of the queries against class c of the base; `index` names the sample in the base batch
    out = metrics.nearest(gen, train, labels_query=lab_g, labels_base=lab_t, per_class=6)
    assert out["idx"].shape == (3, 6, 1) and out["rows_base"].shape == (3, 6)
    for c in range(3):
        rq, rb = out["rows_query"][c], out["rows_base"][c]
        assert (lab_g[rq] == c).all() and (lab_t[rb] == c).all()
        ref = nn_def.knn(torch.tensor(gen[rq]).reshape(6, -1), torch.tensor(train[rb]).reshape(6, -1), 1)
        assert out["index"][c, :, 0].tolist() == rb[ref["idx"][:, 0].numpy()].tolist()
    # a resident, unnormalised training set: searched in place through its affine, its labels by default
    scale, shift = 0.4, -0.3
    raw = torch.tensor((train - shift) / scale)
    ds = types.SimpleNamespace(fits=True, data=raw, labels=torch.tensor(lab_t), scale=scale, shift=shift)
    on_definition.clear()
    out = metrics.nearest(gen, ds, k=1)
    (args, kw), = on_definition
    assert args[1].t.data_ptr() == raw.data_ptr() and kw["b_affine"] == (scale, shift) and kw["q_affine"] is None
    assert out["index"][0, :6, 0].tolist() == copied.tolist()
    out = metrics.nearest(gen, ds, labels_query=lab_g, per_class=6)
    assert out["rows_base"].shape == (3, 6) and (lab_t[out["rows_base"][2]] == 2).all()


def test_memorisation_planted_copies_on_the_definition(on_definition):
    """a quarter of the generated samples are training samples plus 1e-4 noise: exactly those come out unauthentic, each with
    the copied sample as its neighbour; the held-out set (fresh draws of the training model) is what a perfect generator scores"""
    train, lab_t, gen, lab_g, copied = nn_def.planted(0, 120, 40, 3, 5, 5, 4)
    held, lab_h, _, _, _ = nn_def.planted(7, 30, 4, 3, 5, 5, 4)
    out = metrics.memorisation(gen, lab_g, train, lab_t, heldout=held, labels_heldout=lab_h)
    assert out["authentic"].tolist() == [False] * 10 + [True] * 30
    assert out["nn_index"][:10].tolist() == copied.tolist() and out["nn_index"].dtype == torch.int64
    assert out["counts"].dtype == torch.int64 and out["counts"][0].item() == 30
    assert out["authenticity"].dtype == torch.float32 and out["authenticity"].item() == 0.75
    agree = int((lab_t[out["nn_index"].numpy()] == lab_g).sum())
    assert agree >= 10 and out["counts"][1].item() == agree
    assert out["label_agreement"].item() == np.float32(agree / 40)
    # the definition of authenticity, from the float64 distances
    d_tt = nn_def.distances(torch.tensor(train).reshape(120, -1), torch.tensor(train).reshape(120, -1), True).min(1).values
    d_gt = nn_def.distances(torch.tensor(gen).reshape(40, -1), torch.tensor(train).reshape(120, -1))
    near = d_gt.argmin(1)
    assert out["authentic"].tolist() == (d_gt.min(1).values >= d_tt[near]).tolist()
    assert out["heldout_nn_d2"].shape == (30,) and 0 <= out["heldout_authenticity"].item() <= 1
    assert out["heldout_counts"][0].item() == int(out["heldout_authentic"].sum())
    # the train -> train pass is returned, and passed back in it is not repeated
    assert torch.equal(out["train_loo_d2"], d_tt.float())
    on_definition.clear()
    again = metrics.memorisation(gen, lab_g, train, lab_t, train_loo=out["train_loo_d2"])
    assert len(on_definition) == 1 and torch.equal(again["authentic"], out["authentic"])


def test_two_sample_tie_rules_on_the_definition(on_definition):
    """1-D, one class, n = 3.  R = 0, 4, 10; F = 2, 4, 11.
    reals: 0 -> RR 16, RF 4: wrong; 4 -> RR 16, RF 0: wrong; 10 -> RR 36, RF 1: wrong.
    fakes: 2 -> FF 4, FR 4: a tie between a fake and a real neighbour goes to the REAL one: wrong; 4 -> FF 4, FR 0: wrong;
    11 -> FF 49, FR 1: wrong.  Then R = 0, 1, 10; F = 3, 5, 12: real 1 has RR 1 <= RF 4: correct; real 0 RR 1 <= RF 9;
    real 10 RR 81 > RF 4: wrong; fake 3 FF 4 = FR 4: the tie is real: wrong; fake 5 FF 4 < FR 16: correct; fake 12 FF 49 > FR 4."""
    def run(R, F):
        r = torch.tensor(R, dtype=torch.float32).reshape(-1, 1, 1, 1)
        f = torch.tensor(F, dtype=torch.float32).reshape(-1, 1, 1, 1)
        return metrics.nn_two_sample(f, r)
    out = run([0, 4, 10], [2, 4, 11])
    assert out["counts"].tolist() == [[0, 0]] and out["acc"].tolist() == [0.0]
    out = run([0, 1, 10], [3, 5, 12])
    assert out["counts"].tolist() == [[2, 1]]
    assert out["acc_real"].tolist() == [np.float32(2 / 3)] and out["acc_fake"].tolist() == [np.float32(1 / 3)]
    assert out["acc"].tolist() == [0.5] and out["mean"].tolist() == [np.float32(2 / 3), np.float32(1 / 3), 0.5]
    # a real tie on the real side counts as correct (<=): R = 0, 2, F = 1, 9: real 0 has RR 4 > RF 1; R = 0, 1, F = 2, 9:
    # real 1 has RR 1 <= RF 1
    assert run([0, 1], [2, 9])["counts"].tolist() == [[2, 1]]
    # identical sets: every real ties with its fake twin at 0 and wins (RR > 0 = RF: wrong!) - copies drive acc_fake to 0
    out = run([0, 3, 7], [0, 3, 7])
    assert out["counts"].tolist() == [[0, 0]]
    # per class against the definition
    R, F = prdc_def.make_data(3, 3, 20, 20, 30)
    lab = np.repeat(np.arange(3), 20)
    out = metrics.nn_two_sample(F.reshape(60, 2, 3, 5), R.reshape(60, 2, 3, 5), lab, lab)
    want = [list(nn_def.two_sample(F[c], R[c])) for c in range(3)]
    assert out["counts"].tolist() == want
    tot = np.sum(want, 0)
    assert out["mean"].tolist() == [np.float32(tot[0] / 60), np.float32(tot[1] / 60), np.float32(tot.sum() / 120)]
    assert len(on_definition) == 5 * 4          # four searches a call
