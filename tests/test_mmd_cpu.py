"""MMD evaluation without a GPU: the float64 definition (tests/mmd_def.py) against the reference's own outputs
(tests/golden/mmd_ref.npz, made by tests/golden/make_mmd_fixtures.py), the sample selection rule, the argument checks
of kg_mmd and the ctypes mirror of KgMmdArgs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native, build
from kinetic_gan_amd import metrics
from kinetic_gan_amd.feeder import Feeder

import abi_layout
import mmd_def

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture_case(golden_dir, name):
    d = np.load(os.path.join(golden_dir, "mmd_ref.npz"))
    real = d[name + "_real_q"].astype(np.float32) / np.float32(127)
    lab = d[name + "_labels"]
    scale, shift = d[name + "_fake_scale"], d[name + "_fake_shift"]
    fake = (real * scale[lab][:, None, None, None] + shift[lab][:, None, None, None]).astype(np.float32)
    return fake, real, lab, d


@pytest.mark.parametrize("name", ["h36m", "ntu"])
@pytest.mark.parametrize("mode", ["avg", "joint"])
def test_f64_definition_matches_reference_fixtures(golden_dir, name, mode):
    """at every bandwidth whose MMD is >= 100 x the reference's roundoff (propagated through sqrt and the frame
    mean), the float64 definition reproduces the reference's fp32 compute_sequence_mmd to rel 1e-4"""
    fake, real, lab, d = fixture_case(golden_dir, name)
    ref_seq = d["%s_seq_%s" % (name, mode)]
    bws = mmd_def.BANDWIDTHS
    checked = 0
    for c in range(ref_seq.shape[0]):
        i = int(np.flatnonzero(lab == c)[0])
        g0 = torch.tensor(fake[i]).permute(2, 1, 0).double()        # (V, T, C)
        r0 = torch.tensor(real[i]).permute(2, 1, 0).double()
        mine = np.array(mmd_def.sequence_mmd(g0, r0, bws, mode))
        err = mmd_def.sequence_roundoff(g0, r0, bws, mode)
        ok = np.abs(mine) > 100 * err                # (NaN - a negative MMD^2 somewhere - is not compared)
        for b in np.flatnonzero(ok):
            assert abs(mine[b] - ref_seq[c, b]) <= 1e-4 * abs(mine[b]), (c, b, mine[b], ref_seq[c, b])
            checked += 1
        # the winning bandwidth is always among the well-conditioned ones here (the fixture is built that way)
        assert ok[int(np.nanargmax(ref_seq[c]))]
    assert checked >= 2 * ref_seq.shape[0]
    mean, _, _ = mmd_def.calculate_mmd(torch.tensor(fake).double(), torch.tensor(real).double(), lab, mode)
    ref = float(d["%s_calc_%s" % (name, mode)])
    assert abs(mean - ref) <= 1e-5 * abs(ref), (mean, ref)


def test_definition_quirks():
    """m = 1 gives NaN (0 / 0); a NaN or a negative value never wins the per-class maximum, which starts at 0"""
    x = torch.zeros(1, 3, dtype=torch.float64)
    assert np.isnan(mmd_def.mmd2(x, x + 1, [1.0]).item())
    assert mmd_def.class_value([float("nan"), float("nan")]) == 0.0
    assert mmd_def.class_value([float("nan"), 0.2, float("nan"), 0.1]) == 0.2
    assert mmd_def.class_value([-1.0]) == 0.0


class _LabelFeeder:
    """the parts of Feeder that select_reference_samples reads: sample i holds the value i everywhere"""

    def __init__(self, labels, C=2, T=6, V=3, norm=False, dataset="h36m"):
        self.label = np.asarray(labels)
        self.C, self.T, self.V, self.norm, self.dataset = C, T, V, norm, dataset
        n = self.label.size
        self.data = np.broadcast_to(np.arange(n, dtype=np.float32)[:, None, None, None], (n, C, T, V)).copy()
        self.data[:, :, :, 0] += np.arange(T, dtype=np.float32) * 1000      # frame index visible in vertex 0
        self.min, self.max = self.data.min(), self.data.max()


def test_selection_index_zero_only_for_class_zero():
    # index 0 carries label 1: class 0 is scanned from index 0, class 1 from index 1 (the script's reset-then-increment)
    labels = [1, 0, 1, 0, 1, 1, 2, 2, 0, 2, 1]
    f = _LabelFeeder(labels)
    data, lab, idx = metrics.select_reference_samples(f, classes=[0, 1, 2], t_size=4, per_class=2)
    assert idx.tolist() == mmd_def.select_scan(labels, [0, 1, 2], per_class=2) == [1, 3, 2, 4, 6, 7]
    assert lab.tolist() == [0, 0, 1, 1, 2, 2]
    assert data.shape == (6, 2, 4, 3)                                  # cropped to t_size frames
    assert np.array_equal(data[:, 0, 0, 1], idx.astype(np.float32))
    assert np.array_equal(data[0, 0, :, 0] - 1, np.arange(4) * 1000)
    # class 0 does take index 0 when it carries label 0
    labels = [0, 1, 0, 1]
    got = metrics.select_reference_samples(_LabelFeeder(labels), classes=[0, 1], t_size=6, per_class=2)[2]
    assert got.tolist() == mmd_def.select_scan(labels, [0, 1], per_class=2) == [0, 2, 1, 3]


def test_selection_matches_scan_on_random_labels():
    rng = np.random.RandomState(5)
    for trial in range(20):
        labels = rng.randint(0, 4, size=60)
        classes = rng.permutation(4)[:3]
        try:
            want = mmd_def.select_scan(labels, classes, per_class=3)
        except IndexError:
            with pytest.raises(ValueError):
                metrics.select_reference_samples(_LabelFeeder(labels), classes=classes, per_class=3)
            continue
        got = metrics.select_reference_samples(_LabelFeeder(labels), classes=classes, per_class=3)[2]
        assert got.tolist() == want


def test_selection_short_class_names_it():
    labels = [1, 0, 0, 2, 2, 1]          # class 1: one sample from index 1 on (index 0 is never read for it)
    with pytest.raises(ValueError, match=r"class 1 \(label 1\)"):
        metrics.select_reference_samples(_LabelFeeder(labels), classes=[0, 1, 2], per_class=2)
    with pytest.raises(IndexError):
        mmd_def.select_scan(labels, [0, 1, 2], per_class=2)


def test_selection_on_feeder_normalises_like_getitem(golden_dir):
    """through the package Feeder on the committed feeder fixture: the vectorised read equals feeder[i] cropped"""
    f = Feeder(os.path.join(golden_dir, "feeder_h36m_data.npy"), os.path.join(golden_dir, "feeder_h36m_label.pkl"),
               norm=True, dataset="h36m")
    data, lab, idx = metrics.select_reference_samples(f, classes=[3, 2], t_size=10, per_class=2)
    assert idx.tolist() == mmd_def.select_scan(f.label, [3, 2], per_class=2)
    for k, i in enumerate(idx):
        assert np.array_equal(data[k], f[int(i)][0][:, :10, :].astype(np.float32))


def test_metrics_argument_errors_without_gpu():
    with pytest.raises(Exception, match="undefined mode"):
        metrics.MMD("frames").compute_sequence_mmd(torch.zeros(4, 2, 3), torch.zeros(4, 2, 3), 1.0)
    with pytest.raises(ValueError, match="m=4 != n=5"):
        metrics.mmd_sweep(torch.zeros(4, 2, 3), torch.zeros(5, 2, 3), [1.0], "avg")
    with pytest.raises(ValueError, match="m=4 != n=3"):
        metrics.MMD("avg").rkhs_mmd(torch.zeros(4, 3), torch.zeros(3, 3), 1.0)
    with pytest.raises(ValueError, match="class 1 has no sample"):
        metrics.calculate_mmd(torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 4, 5), np.eye(3)[[0, 2]], "avg")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.load_library()


def _valid_args():
    a = _native._MmdArgs()
    a.x, a.y = 0x1000, 0x2000
    a.x_sp, a.x_sd, a.y_sp, a.y_sd = 1, 16, 1, 16
    a.m, a.n, a.dim, a.groups, a.classes, a.nbw = 16, 16, 3, 32, 10, 14
    for b in range(14):
        a.bw[b] = 10.0 ** (b - 4)
    a.mmd2, a.mmd, a.result, a.ws = 0x3000, 0x4000, 0x5000, 0x6000
    return a


@pytest.mark.parametrize("field,value,needle", [
    ("n", 17, b"m=16 != n=17"), ("m", 0, b"m=0"), ("dim", 0, b"dim=0"), ("nbw", 0, b"nbw=0"), ("nbw", 17, b"nbw=17"),
    ("bw", -1.0, b"bw[3]"), ("bw", 0.0, b"bw[3]"), ("x", None, b"null pointer x"), ("y", None, b"null pointer y"),
    ("mmd2", None, b"null pointer mmd2"), ("mmd", None, b"null pointer mmd"), ("result", None, b"null pointer result"),
    ("ws", None, b"null pointer ws"), ("ws_bytes", 4, b"ws_bytes=4"), ("groups", 0, b"groups=0")])
def test_kg_mmd_rejects_bad_arguments_without_gpu(lib, field, value, needle):
    a = _valid_args()
    need = lib.kg_mmd_workspace_bytes(ctypes.byref(a))
    assert need == 10 * 32 * 14 * 4            # m = 16: one 16 x 16 tile per (class, frame)
    a.ws_bytes = need
    if field == "bw":
        a.bw[3] = value
    else:
        setattr(a, field, value)
    if field in ("n", "m", "dim", "nbw", "bw", "groups"):
        assert lib.kg_mmd_workspace_bytes(ctypes.byref(a)) < 0
        assert needle in lib.kg_last_error()
    if field == "m" and value == 0:
        a.n = 0
    assert lib.kg_mmd(ctypes.byref(a), None) < 0
    assert needle in lib.kg_last_error(), lib.kg_last_error()


def test_kg_mmd_m1_is_valid(lib):
    a = _valid_args()
    a.m = a.n = 1
    assert lib.kg_mmd_workspace_bytes(ctypes.byref(a)) == 10 * 32 * 14 * 4


def test_mmd_struct_matches_header():
    abi_layout.assert_mirror("KgMmdArgs")
    assert _native.MMD_MAX_BW == 16
