"""MMD evaluation of generated actions (evaluation/mmd-actions.py of the reference) on the kg_mmd HIP kernels, and
precision / recall / density / coverage of sample sets on the kg_prdc kernels (``prdc``) and the Frechet distance of
pose / motion / caller features in fp64 on the kg_frechet kernels (``frechet``, ``frechet_features``), and nearest training
samples with the memorisation scores built on them on the kg_nn kernels (``nearest``, ``memorisation``, ``nn_two_sample``),
at the end, and kinematic plausibility - bone lengths, symmetry, smoothness - on the kg_kin kernels (``kinematics``,
``kinematics_real``, ``kinematics_sets``).

The reference scores samples with a kernel two-sample statistic (MMD) under 14 RBF bandwidths 10^-4 .. 10^9: per class
the first selected fake and real sample, each a set of V points (joints) per frame (``avg``: the mean over frames of
the per-frame MMD, points of dimension C) or one set of V points of dimension C*T (``joint``); the class value is the
largest MMD over the bandwidths (NaN never wins, never below 0), the score the mean over classes.  It runs every
(class, bandwidth, frame) as separate torch calls, each ending in a host sync (143 k of them for H36M at T = 1024).

Here one kg_mmd call computes every (class, frame, bandwidth) in one launch plus one single-workgroup finishing launch
and leaves the result on the device (``calculate_mmd``, ``mmd_sweep``).  ``MMD`` keeps the reference class's surface
(methods return Python floats, one sync each).  ``select_reference_samples`` is the script's sample selection.

Numerics: the result is defined against a float64 evaluation of the same formula (tests/mmd_def.py); at the
bandwidths where every kernel value is 1 - O(1e-8) the reference's own fp32 values are roundoff.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native

DEFAULT_BANDWIDTHS = tuple(10.0 ** j for j in range(-4, 10))      # mmd-actions.py:106: 10 ** j, j = -4 .. 9
MODES = ("avg", "joint")


def _as_f32(t) -> torch.Tensor:
    t = torch.as_tensor(t)
    return t if t.dtype == torch.float32 else t.float()


def _as_cuda(t) -> torch.Tensor:
    """fp32 tensor on the current GPU (numpy arrays and CPU tensors are copied there: the computation has no CPU path)"""
    t = _as_f32(t)
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return t


def _check_mode(mode: str):
    if mode not in MODES:
        raise ValueError("undefined mode %r (MMD modes: 'avg', 'joint')" % (mode,))


def _check_pair(a: torch.Tensor, b: torch.Tensor, what: str):
    if a.shape[0] != b.shape[0]:
        raise ValueError("%s: m=%d != n=%d (both sets need the same number of points)" % (what, a.shape[0], b.shape[0]))
    if a.shape[1:] != b.shape[1:]:
        raise ValueError("%s: shapes %s and %s differ beyond the point axis" % (what, tuple(a.shape), tuple(b.shape)))


def _seq_view(seq: torch.Tensor, mode: str) -> Tuple[_native.MmdView, int, int]:
    """(N, L, D) sequence -> (view, dim, groups): avg = L groups of N points of dimension D; joint = one group of N
    points of dimension L*D (the reference's ``view(-1, L*D)``: a copy only where that view would not exist)"""
    n, L, D = seq.shape
    if mode == "avg":
        return _native.MmdView(seq, seq.stride(0), seq.stride(2), seq.stride(1), 0), D, L
    if L > 1 and D > 1 and seq.stride(1) != D * seq.stride(2):
        seq = seq.contiguous()
    sd = seq.stride(2) if D > 1 else seq.stride(1)
    return _native.MmdView(seq, seq.stride(0), sd, 0, 0), L * D, 1


def _bandwidths(bandwidths) -> list:
    bws = [float(b) for b in (bandwidths if isinstance(bandwidths, (list, tuple, np.ndarray, torch.Tensor))
                              else [bandwidths])]
    return bws


def mmd_sweep(seq1, seq2, bandwidths: Sequence[float] = DEFAULT_BANDWIDTHS, mode: str = "avg") -> torch.Tensor:
    """``compute_sequence_mmd`` of (N, L, D) sequences for every bandwidth at once: Tensor (nbw,) on the device, no
    host sync.  avg: mean over the L frames of the per-frame MMD; joint: the MMD of the flattened (N, L*D) sets."""
    _check_mode(mode)
    seq1, seq2 = _as_f32(seq1), _as_f32(seq2)
    if seq1.dim() != 3:
        raise ValueError("mmd_sweep: sequences are (N, L, D), got %s" % (tuple(seq1.shape),))
    _check_pair(seq1, seq2, "mmd_sweep")
    seq1, seq2 = _as_cuda(seq1), _as_cuda(seq2)
    x, dim, groups = _seq_view(seq1, mode)
    y, _, _ = _seq_view(seq2, mode)
    out = _native.mmd(x, y, seq1.shape[0], seq2.shape[0], dim, groups, 1, _bandwidths(bandwidths))
    return out["mmd"][0]


class MMD:
    """The reference's ``MMD`` class (evaluation/mmd-actions.py:14-76) on the HIP kernels.  ``use_torch`` is kept for
    the signature; inputs may be CUDA tensors, CPU tensors or numpy arrays and are evaluated on the GPU."""

    def __init__(self, mode: str, use_torch: int = 1):
        self.mode = mode
        self.use_torch = use_torch

    def reset(self, new_mode: str):
        self.mode = new_mode

    def rkhs_mmd(self, samples_1, samples_2, bandwidth: float) -> float:
        """sqrt(sum_{i != j} [k(x_i,x_j) + k(y_i,y_j) - 2 k(x_i,y_j)] / (m (m-1))) of two (m, dim) sets"""
        s1, s2 = _as_f32(samples_1), _as_f32(samples_2)
        if s1.dim() != 2:
            raise ValueError("rkhs_mmd: samples are (m, dim), got %s" % (tuple(s1.shape),))
        _check_pair(s1, s2, "rkhs_mmd")
        s1, s2 = _as_cuda(s1), _as_cuda(s2)
        x = _native.MmdView(s1, s1.stride(0), s1.stride(1), 0, 0)
        y = _native.MmdView(s2, s2.stride(0), s2.stride(1), 0, 0)
        return _native.mmd(x, y, s1.shape[0], s2.shape[0], s1.shape[1], 1, 1, [float(bandwidth)])["mmd"].item()

    def compute_sequence_mmd(self, sequence_1, sequence_2, bandwidth: float) -> float:
        _check_mode(self.mode)
        return mmd_sweep(sequence_1, sequence_2, [float(bandwidth)], self.mode).item()


def _class_index(labels, n: int) -> Tuple[np.ndarray, int]:
    """labels -> (class index per sample, number of classes); one-hot rows (the reference's form) or class ids"""
    if isinstance(labels, torch.Tensor):
        labels = labels.cpu().numpy()           # (one sync when the labels live on the device)
    lab = np.asarray(labels)
    if lab.ndim == 2:
        k = lab.shape[-1]
        lab = lab.argmax(-1)
    else:
        lab = lab.astype(np.int64)
        k = int(lab.max()) + 1 if lab.size else 0
    if lab.shape[0] != n:
        raise ValueError("calculate_mmd: %d labels for %d samples" % (lab.shape[0], n))
    return lab, k


def calculate_mmd(gen, real, labels, mode: str = "avg", bandwidths: Sequence[float] = DEFAULT_BANDWIDTHS,
                  per_class: bool = False):
    """The ``calcualte_mmd`` protocol (mmd-actions.py:79-115) over all classes in one kg_mmd call.

    gen, real: (N, C, T, V) as the feeder produces them (fake, real: the reference's argument order); labels: one-hot
    (N, K) or class ids (N,).  For each class k < K the first sample labelled k of each set is compared.  Returns the
    mean over classes as a 0-d device tensor; with ``per_class=True`` also (result (K,), mmd (K, nbw)).  No host sync
    (labels that live on the device are read once).  When the first samples of the classes are not evenly spaced in
    the batch they are gathered first (one copy); the reference protocol's batches (``select_reference_samples``)
    are, and are read in place."""
    _check_mode(mode)
    gen, real = _as_f32(gen), _as_f32(real)
    if gen.dim() != 4:
        raise ValueError("calculate_mmd: samples are (N, C, T, V), got %s" % (tuple(gen.shape),))
    if gen.shape != real.shape:
        raise ValueError("calculate_mmd: gen %s and real %s differ" % (tuple(gen.shape), tuple(real.shape)))
    lab, k = _class_index(labels, gen.shape[0])
    first = np.full(k, -1, dtype=np.int64)
    seen = np.unique(lab, return_index=True)
    first[seen[0]] = seen[1]
    missing = np.flatnonzero(first < 0)
    if missing.size:
        raise ValueError("calculate_mmd: class %d has no sample" % missing[0])
    gen, real = _as_cuda(gen), _as_cuda(real)
    step = int(first[1] - first[0]) if k > 1 else 1
    if k > 1 and (step <= 0 or np.any(np.diff(first) != step)):
        gen = torch.stack([gen[int(i)] for i in first])       # (no index upload: capturable in a graph)
        real = torch.stack([real[int(i)] for i in first])
        base, step = 0, 1
    else:
        base = int(first[0])
    _, C, T, V = gen.shape
    views = []
    for t in (gen, real):
        sc = step * t.stride(0)
        if mode == "avg":
            views.append(_native.MmdView(t[base], t.stride(3), t.stride(1), t.stride(2), sc))
        else:
            if C > 1 and T > 1 and t.stride(1) != T * t.stride(2):
                raise ValueError("calculate_mmd: joint mode needs each sample's (C, T) block contiguous in T "
                                 "(got strides %s)" % (t.stride(),))
            sd = t.stride(2) if T > 1 else t.stride(1)
            views.append(_native.MmdView(t[base], t.stride(3), sd, 0, sc))
    dim, groups = (C, T) if mode == "avg" else (C * T, 1)
    out = _native.mmd(views[0], views[1], V, V, dim, groups, k, _bandwidths(bandwidths), want_mean=True)
    if per_class:
        return out["mean"], out["result"], out["mmd"]
    return out["mean"]


PRDC_NAMES = ("precision", "recall", "density", "coverage")


def _label_ids(labels, n: int, what: str, who: str = "prdc") -> Tuple[np.ndarray, int]:
    """labels -> (class id per sample, classes the labels can name); None = one class"""
    if labels is None:
        return np.zeros(n, dtype=np.int64), 1
    if isinstance(labels, torch.Tensor):
        labels = labels.cpu().numpy()           # (one sync when the labels live on the device)
    lab = np.asarray(labels)
    if lab.ndim == 2:
        k = lab.shape[-1]
        lab = lab.argmax(-1)
    else:
        lab = lab.astype(np.int64)
        k = int(lab.max()) + 1 if lab.size else 0
    if lab.shape[0] != n:
        raise ValueError("%s: %d %s for %d samples" % (who, lab.shape[0], what, n))
    return lab, k


def _class_rows(lab: np.ndarray, classes: int, per_class: Optional[int], what: str, who: str = "prdc") -> np.ndarray:
    """(classes, count) sample indices: the first ``per_class`` samples of every class in index order (default: all of
    them; the classes must then hold the same number)"""
    rows = [np.flatnonzero(lab == c) for c in range(classes)]
    if per_class is None:
        count = rows[0].size
        for c, r in enumerate(rows):
            if r.size != count:
                raise ValueError("%s: class %d has %d %s samples, class 0 has %d (ragged classes: pass per_class)"
                                 % (who, c, r.size, what, count))
    else:
        count = int(per_class)
        for c, r in enumerate(rows):
            if r.size < count:
                raise ValueError("%s: class %d has %d %s samples, per_class=%d needed" % (who, c, r.size, what, count))
    if count < 1:
        raise ValueError("%s: class 0 has no %s sample" % (who, what))
    return np.stack([r[:count] for r in rows])


def _prdc_view(t: torch.Tensor, idx: np.ndarray):
    """(view, d_outer, d_inner) of the samples idx (classes, count) of t (N, C, T, V) on the device: read in place when
    idx is evenly spaced along both axes, else gathered once; a (C, T, V) block that is not outer x contiguous inner
    (a crop in T is: outer = C) is made contiguous"""
    K, cnt = idx.shape
    ps = int(idx[0, 1] - idx[0, 0]) if cnt > 1 else 1
    cs = int(idx[1, 0] - idx[0, 0]) if K > 1 else 0
    even = ps > 0 and cs >= 0 and np.array_equal(idx, idx[0, 0] + cs * np.arange(K)[:, None] + ps * np.arange(cnt)[None, :])
    if even:
        base = int(idx[0, 0])
    else:
        t = t.index_select(0, torch.as_tensor(idx.reshape(-1), device=t.device))
        base, ps, cs = 0, 1, cnt
    _, C, T, V = t.shape
    if not ((V == 1 or t.stride(3) == 1) and (T == 1 or t.stride(2) == V)):
        t = t.contiguous()
    if C == 1 or t.stride(1) == T * V:
        d_outer, d_inner, so = 1, C * T * V, 0
    else:
        d_outer, d_inner, so = C, T * V, t.stride(1)
    return _native.PrdcView(t[base], cs * t.stride(0), ps * t.stride(0), so), d_outer, d_inner


def _view_pair(a: torch.Tensor, idx_a: np.ndarray, b: torch.Tensor, idx_b: np.ndarray):
    """(view of a, view of b, d_outer, d_inner): _prdc_view of both sets with ONE split of the dimension"""
    av, d_outer, d_inner = _prdc_view(a, idx_a)
    bv, bo, bi = _prdc_view(b, idx_b)
    if (bo, bi) != (d_outer, d_inner):          # one side is a crop, the other is not: both as channel rows
        C, T, V = a.shape[1:]
        av, bv = (v if v.so or C == 1 else v._replace(so=T * V) for v in (av, bv))
        d_outer, d_inner = C, T * V
    return av, bv, d_outer, d_inner


def prdc(gen, real, labels_gen=None, labels_real=None, k: int = 5, per_class: Optional[int] = None,
         per_point: bool = False) -> dict:
    """Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) per class on the
    sequences themselves (a sample = one point of dimension C*T*V), in one kg_prdc call (three launches).

    gen (Nf, C, T, V), real (Nr, C, T, V): fake, real - calculate_mmd's argument order; CUDA tensors, CPU tensors or
    numpy.  Labels: one-hot (N, K) or class ids (N,); without labels everything is one class.  For every class the first
    ``per_class`` samples of each set are used (default: all; every class must then hold the same number within a set -
    ragged classes raise ValueError naming the class).  Samples that lie class by class and evenly spaced in the batch are
    read in place through strides, otherwise they are gathered once.  Returns device tensors: ``mean`` (4,) - the plain
    mean over classes in the order PRDC_NAMES -, ``values`` (K, 4), ``counts`` (K, 4) int32 (cP, cR, cD, cC); with
    ``per_point`` also ``radii_real`` (K, n), ``radii_fake`` (K, m) (squared k-th-neighbour distances), ``fake_hits``
    (K, m) int32 and ``real_flags`` (K, n) uint8 (bit 0: recall, bit 1: coverage).  No host sync (labels that live on
    the device are read once)."""
    gen, real = _as_f32(gen), _as_f32(real)
    if gen.dim() != 4 or real.dim() != 4:
        raise ValueError("prdc: samples are (N, C, T, V), got %s and %s" % (tuple(gen.shape), tuple(real.shape)))
    if gen.shape[1:] != real.shape[1:]:
        raise ValueError("prdc: gen samples %s and real samples %s differ in shape" % (tuple(gen.shape[1:]),
                                                                                      tuple(real.shape[1:])))
    lab_g, kg = _label_ids(labels_gen, gen.shape[0], "labels_gen")
    lab_r, kr = _label_ids(labels_real, real.shape[0], "labels_real")
    classes = max(kg, kr)
    if classes < 1:
        raise ValueError("prdc: no samples")
    idx_r = _class_rows(lab_r, classes, per_class, "real")
    idx_g = _class_rows(lab_g, classes, per_class, "fake")
    n, m = idx_r.shape[1], idx_g.shape[1]
    if not 1 <= k <= min(_native.PRDC_MAX_K, min(n, m) - 1):
        raise ValueError("prdc: k=%d outside [1, min(%d, min(n=%d, m=%d) - 1)]" % (k, _native.PRDC_MAX_K, n, m))
    gen, real = _as_cuda(gen), _as_cuda(real)
    rv, gv, d_outer, d_inner = _view_pair(real, idx_r, gen, idx_g)
    return _native.prdc(rv, gv, n, m, d_outer, d_inner, classes, k, want_mean=True, per_point=per_point)


FRECHET_MODES = ("pose", "motion")
FRECHET_TERMS = ("dmu2", "tr_real", "tr_fake", "tr_sqrt")


def _frechet_view(t: torch.Tensor, idx: np.ndarray) -> _native.FrechetView:
    """view of the samples idx (classes, count) of t (N, C, T, V) on the device: read in place when idx is evenly spaced
    along both axes, else gathered once; only the joint axis has to be contiguous (a crop in T is read in place)"""
    K, cnt = idx.shape
    ps = int(idx[0, 1] - idx[0, 0]) if cnt > 1 else 1
    cs = int(idx[1, 0] - idx[0, 0]) if K > 1 else 0
    even = ps > 0 and cs >= 0 and np.array_equal(idx, idx[0, 0] + cs * np.arange(K)[:, None] + ps * np.arange(cnt)[None, :])
    if even:
        base = int(idx[0, 0])
    else:
        t = t.index_select(0, torch.as_tensor(idx.reshape(-1), device=t.device))
        base, ps, cs = 0, 1, cnt
    if (t.shape[3] > 1 and t.stride(3) != 1) or min(t.stride()) < 0:
        t = t.contiguous()
    return _native.FrechetView(t[base], cs * t.stride(0), ps * t.stride(0), t.stride(2), t.stride(1))


def frechet(gen, real, labels_gen=None, labels_real=None, mode: str = "pose", per_class: Optional[int] = None,
            moments: bool = False) -> dict:
    """Frechet distance per class between the frames (``pose``: a point is one frame, dimension C*V) or the frame
    differences (``motion``: x[:, :, f + 1] - x[:, :, f], formed in fp64) of generated and real sequences, in fp64, in one
    kg_frechet call (four launches):

        FD = |mu_r - mu_f|^2 + tr S_r + tr S_f - 2 tr sqrt(S_r S_f)        (unbiased covariances)

    gen (Nf, C, T, V), real (Nr, C, T, V): fake, real - prdc's argument order and prdc's conventions: labels one-hot
    (N, K), class ids (N,) or None for one class; the first ``per_class`` samples of every class (default: all; ragged
    classes raise ValueError); samples that lie evenly spaced in the batch are read in place, otherwise gathered once.
    C*V must not exceed 96 and either set needs two points.  Returns device tensors: ``mean`` () fp64 - the plain mean over
    classes -, ``values`` (K,), ``terms`` (K, 4) in the order FRECHET_TERMS, ``sweeps`` (K, 2) int32 (Jacobi sweeps of
    the two eigen-problems); with ``moments`` also ``mu_real``, ``mu_fake`` (K, d) and ``cov_real``, ``cov_fake``
    (K, d, d).  ``mode="both"`` returns {"pose": ..., "motion": ...} from two calls.  No host sync (labels that live on
    the device are read once)."""
    if mode == "both":
        return {md: frechet(gen, real, labels_gen, labels_real, md, per_class, moments) for md in FRECHET_MODES}
    if mode not in FRECHET_MODES:
        raise ValueError("frechet: undefined mode %r ('pose', 'motion' or 'both')" % (mode,))
    gen, real = _as_f32(gen), _as_f32(real)
    if gen.dim() != 4 or real.dim() != 4:
        raise ValueError("frechet: samples are (N, C, T, V), got %s and %s" % (tuple(gen.shape), tuple(real.shape)))
    if gen.shape[1:] != real.shape[1:]:
        raise ValueError("frechet: gen samples %s and real samples %s differ in shape" % (tuple(gen.shape[1:]),
                                                                                         tuple(real.shape[1:])))
    _, C, T, V = real.shape
    diff = mode == "motion"
    if C * V > _native.FRECHET_MAX_DIM:
        raise ValueError("frechet: d = C*V = %d above %d" % (C * V, _native.FRECHET_MAX_DIM))
    if T < 1 + diff:
        raise ValueError("frechet: T=%d frames, mode %r needs %d" % (T, mode, 1 + diff))
    lab_g, kg = _label_ids(labels_gen, gen.shape[0], "labels_gen")
    lab_r, kr = _label_ids(labels_real, real.shape[0], "labels_real")
    classes = max(kg, kr)
    if classes < 1:
        raise ValueError("frechet: no samples")
    idx_r = _class_rows(lab_r, classes, per_class, "real")
    idx_g = _class_rows(lab_g, classes, per_class, "fake")
    n, m = idx_r.shape[1], idx_g.shape[1]
    if min(n, m) * (T - diff) < 2:
        raise ValueError("frechet: n=%d, m=%d samples of %d points each: either set needs two points" % (n, m, T - diff))
    gen, real = _as_cuda(gen), _as_cuda(real)
    return _native.frechet(_frechet_view(real, idx_r), _frechet_view(gen, idx_g), n, m, T, diff, C, V, classes,
                           want_mean=True, moments=moments)


def frechet_features(feat_gen, feat_real, labels_gen=None, labels_real=None, per_class: Optional[int] = None,
                     moments: bool = False) -> dict:
    """``frechet`` on (N, d) feature matrices of the caller's own extractor (d <= 96): a row is a point."""
    feat_gen, feat_real = _as_f32(feat_gen), _as_f32(feat_real)
    if feat_gen.dim() != 2 or feat_real.dim() != 2:
        raise ValueError("frechet_features: features are (N, d), got %s and %s" % (tuple(feat_gen.shape),
                                                                                   tuple(feat_real.shape)))
    if feat_gen.shape[1] != feat_real.shape[1]:
        raise ValueError("frechet_features: gen features %s and real features %s differ in shape"
                         % (tuple(feat_gen.shape[1:]), tuple(feat_real.shape[1:])))
    return frechet(feat_gen[:, None, None, :], feat_real[:, None, None, :], labels_gen, labels_real, "pose", per_class, moments)


KIN_NAMES = ("bone_cv", "asymmetry", "speed", "accel", "jerk", "still")


def _kin_tables(dataset: str, bones, mirror, who: str):
    """(bones, mirror) as lists of int pairs: the dataset's skeleton (graph.py) unless the caller brings a bone list - then
    the mirror pairs are the caller's too (none given: no asymmetry term)"""
    if bones is None:
        from .graph import Graph_h36m, graph_ntu
        if dataset not in ("ntu", "h36m"):
            raise ValueError("%s: undefined dataset %r ('ntu' or 'h36m'; or pass bones)" % (who, dataset))
        g = graph_ntu if dataset == "ntu" else Graph_h36m
        bones, mirror = g.bones, (g.mirror_bones if mirror is None else mirror)
    elif mirror is None:
        mirror = ()
    out = []
    for name, tab in (("bones", bones), ("mirror", mirror)):
        tab = np.asarray(tab, dtype=np.int64).reshape(-1, 2) if len(tab) else np.zeros((0, 2), dtype=np.int64)
        out.append([(int(u), int(v)) for u, v in tab])
    return out[0], out[1]


def _kin_check(x: torch.Tensor, what: str, bones, mirror, still_eps: float, who: str):
    """the limits of kg_kin_desc as ValueErrors naming the argument"""
    if x.dim() != 4:
        raise ValueError("%s: %s samples are (N, C, T, V), got %s" % (who, what, tuple(x.shape)))
    _, C, T, V = x.shape
    if C not in (2, 3):
        raise ValueError("%s: %s has C=%d channels, 2 or 3 expected" % (who, what, C))
    if not 1 <= V <= _native.KIN_MAX_JOINTS:
        raise ValueError("%s: %s has V=%d joints, outside [1, %d]" % (who, what, V, _native.KIN_MAX_JOINTS))
    if T < _native.KIN_MIN_FRAMES:
        raise ValueError("%s: %s has T=%d frames, jerk needs %d" % (who, what, T, _native.KIN_MIN_FRAMES))
    if C * T * V > _native.KIN_MAX_ELEMS:
        raise ValueError("%s: %s has C*T*V = %d values per sample, above %d" % (who, what, C * T * V, _native.KIN_MAX_ELEMS))
    if not 1 <= len(bones) <= _native.KIN_MAX_BONES:
        raise ValueError("%s: %d bones, outside [1, %d]" % (who, len(bones), _native.KIN_MAX_BONES))
    if len(mirror) > _native.KIN_MAX_MIRROR:
        raise ValueError("%s: %d mirror pairs, above %d" % (who, len(mirror), _native.KIN_MAX_MIRROR))
    if any(not 0 <= j < V for b in bones for j in b):
        raise ValueError("%s: bones name a joint outside [0, V=%d) of %s (wrong dataset?)" % (who, V, what))
    if any(not 0 <= j < len(bones) for p in mirror for j in p):
        raise ValueError("%s: mirror names a bone outside [0, %d)" % (who, len(bones)))
    if not (np.isfinite(still_eps) and still_eps >= 0):
        raise ValueError("%s: still_eps=%r is not a finite number >= 0" % (who, still_eps))


def _kin_side(x: torch.Tensor, idx: np.ndarray, bones, mirror, still_eps: float, out=None):
    """(desc (K, count, 6), degenerate (K,)) of the samples idx (K, count) of x (N, C, T, V): one kg_kin_desc launch"""
    _, C, T, V = x.shape
    return _native.kin_desc(_frechet_view(x, idx), idx.shape[1], T, C, V, idx.shape[0], bones, mirror, still_eps, out=out)


def kinematics_real(real, labels_real=None, dataset: str = "ntu", bones=None, mirror=None, per_class: Optional[int] = None,
                    still_eps: float = 1e-3, classes: Optional[int] = None, with_degenerate: bool = False):
    """The real side of ``kinematics`` once: the descriptor matrix (K, n, 6) fp32 on the device that ``kinematics_sets``
    reads (one kg_kin_desc launch).  ``classes``: the number of classes when the labels do not name the last one.  With
    ``with_degenerate`` returns (desc, degenerate (K,) int32)."""
    who = "kinematics_real"
    real = _as_f32(real)
    bones, mirror = _kin_tables(dataset, bones, mirror, who)
    _kin_check(real, "real", bones, mirror, still_eps, who)
    lab_r, kr = _label_ids(labels_real, real.shape[0], "labels_real", who)
    K = max(kr, int(classes or 0))
    if K < 1:
        raise ValueError("%s: no samples" % who)
    idx_r = _class_rows(lab_r, K, per_class, "real", who)
    desc, degenerate = _kin_side(_as_cuda(real), idx_r, bones, mirror, still_eps)
    return (desc, degenerate) if with_degenerate else desc


def kinematics_sets(sets, real_desc: torch.Tensor, labels=None, dataset: str = "ntu", bones=None, mirror=None,
                    per_class: Optional[int] = None, still_eps: float = 1e-3) -> dict:
    """Up to four generated sets (each (Nf, C, T, V), sharing ``labels`` and the shape) against the cached real descriptors
    of ``kinematics_real``: one kg_kin_desc launch per set, then ONE kg_kin_scores call (two launches) for all of them.
    Returns device tensors ``w1_mean`` (nsets, 6), ``scores`` (nsets, 6) fp32 (the one rounding of w1_mean: the word an
    evaluation record carries), ``w1`` (nsets, K, 6), ``mean_real`` (K, 6), ``mean_fake`` (nsets, K, 6), ``nonfinite``
    (nsets + 1, K) int32 (row 0: the real side), ``degenerate`` (nsets, K) int32 and ``desc`` (nsets, K, m, 6).  Every set's
    slices are, bit for bit, the results of its own ``kinematics`` call."""
    who = "kinematics_sets"
    sets = [_as_f32(s) for s in sets]
    if not 1 <= len(sets) <= _native.KIN_MAX_SETS:
        raise ValueError("%s: %d sets, 1 to %d expected" % (who, len(sets), _native.KIN_MAX_SETS))
    if real_desc.dim() != 3 or real_desc.shape[2] != _native.KIN_DESC or real_desc.dtype != torch.float32:
        raise ValueError("%s: real_desc is the (K, n, 6) fp32 result of kinematics_real, got %s" % (who, tuple(real_desc.shape)))
    bones, mirror = _kin_tables(dataset, bones, mirror, who)
    for g, s in enumerate(sets):
        _kin_check(s, "sets[%d]" % g, bones, mirror, still_eps, who)
        if s.shape != sets[0].shape:
            raise ValueError("%s: sets[%d] has shape %s, sets[0] %s" % (who, g, tuple(s.shape), tuple(sets[0].shape)))
    lab, kg = _label_ids(labels, sets[0].shape[0], "labels", who)
    K = real_desc.shape[0]
    if kg > K:
        raise ValueError("%s: labels name %d classes, real_desc has %d" % (who, kg, K))
    idx = _class_rows(lab, K, per_class, "fake", who)
    m, n = idx.shape[1], real_desc.shape[1]
    if n + m > _native.KIN_MAX_POINTS:
        raise ValueError("%s: n + m = %d + %d values per class, above %d" % (who, n, m, _native.KIN_MAX_POINTS))
    dev = torch.device("cuda", torch.cuda.current_device())
    desc = torch.empty((len(sets), K, m, _native.KIN_DESC), dtype=torch.float32, device=dev)
    degenerate = [_kin_side(_as_cuda(s), idx, bones, mirror, still_eps, out=desc[g])[1] for g, s in enumerate(sets)]
    out = _native.kin_scores(real_desc.contiguous(), [desc[g] for g in range(len(sets))])
    out.update(degenerate=torch.stack(degenerate), desc=desc)
    return out


def kinematics(gen, real, labels_gen=None, labels_real=None, dataset: str = "ntu", bones=None, mirror=None,
               per_class: Optional[int] = None, still_eps: float = 1e-3, per_sample: bool = False) -> dict:
    """Kinematic plausibility of generated skeleton sequences against real ones.  Every sample gets six
    dimensionless descriptors, KIN_NAMES: the variation of its bone lengths over time, the left / right asymmetry of its
    mean bone lengths, mean joint speed, acceleration and jerk in units of its own mean bone length, and the share of
    (joint, frame) steps that do not move; per class and descriptor the score is the Wasserstein-1 distance between the
    real and the generated samples' values (smaller is better).  fp64 throughout, in three launches of kg_kin_desc (one per
    side) and kg_kin_scores.

    gen (Nf, C, T, V), real (Nr, C, T, V): ``frechet``'s argument order and conventions - labels one-hot (N, K), class ids
    (N,) or None for one class; the first ``per_class`` samples of every class (default: all; ragged classes raise
    ValueError); evenly spaced samples and crops in T are read in place.  The two tensors may differ in value scale (raw
    real data against normalised generated data): the descriptors are invariant under x * scale + shift, nothing is
    normalised.  The skeleton is ``dataset``'s (graph.py: bones, mirror_bones) unless ``bones`` (B, 2) joint pairs - and
    then ``mirror`` (M, 2) pairs of bone indices, default none - are given.  C in (2, 3), V <= 32, T >= 4, C*T*V <= 32768,
    n + m <= 16384 per class.  Returns device tensors: ``w1_mean`` (6,) fp64 - the plain mean over classes -, ``scores``
    (6,) its fp32 rounding, ``w1`` (K, 6), ``mean_real``, ``mean_fake`` (K, 6) the class means of the descriptors,
    ``nonfinite`` (2, K) int32 samples with a non-finite descriptor (row 0: real) and ``degenerate``, ``degenerate_real``
    (K,) int32 samples whose bones all have length zero (their descriptors are zero); with ``per_sample`` also ``desc_real``
    (K, n, 6) and ``desc_fake`` (K, m, 6).  No host sync (labels that live on the device are read once)."""
    who = "kinematics"
    gen, real = _as_f32(gen), _as_f32(real)
    bones, mirror = _kin_tables(dataset, bones, mirror, who)
    _kin_check(gen, "gen", bones, mirror, still_eps, who)
    _kin_check(real, "real", bones, mirror, still_eps, who)
    if gen.shape[1:] != real.shape[1:]:
        raise ValueError("%s: gen samples %s and real samples %s differ in shape" % (who, tuple(gen.shape[1:]),
                                                                                    tuple(real.shape[1:])))
    lab_g, kg = _label_ids(labels_gen, gen.shape[0], "labels_gen", who)
    lab_r, kr = _label_ids(labels_real, real.shape[0], "labels_real", who)
    classes = max(kg, kr)
    if classes < 1:
        raise ValueError("%s: no samples" % who)
    idx_r = _class_rows(lab_r, classes, per_class, "real", who)
    idx_g = _class_rows(lab_g, classes, per_class, "fake", who)
    n, m = idx_r.shape[1], idx_g.shape[1]
    if n + m > _native.KIN_MAX_POINTS:
        raise ValueError("%s: n + m = %d + %d values per class, above %d (pass per_class)" % (who, n, m, _native.KIN_MAX_POINTS))
    desc_r, deg_r = _kin_side(_as_cuda(real), idx_r, bones, mirror, still_eps)
    desc_f, deg_f = _kin_side(_as_cuda(gen), idx_g, bones, mirror, still_eps)
    res = _native.kin_scores(desc_r, [desc_f])
    out = dict(w1_mean=res["w1_mean"][0], scores=res["scores"][0], w1=res["w1"][0], mean_real=res["mean_real"],
               mean_fake=res["mean_fake"][0], nonfinite=res["nonfinite"], degenerate=deg_f, degenerate_real=deg_r)
    if per_sample:
        out.update(desc_real=desc_r, desc_fake=desc_f)
    return out


CLS_NAMES = ("accuracy", "feature_fd", "diversity", "multimodality")


def cls_pair_tables(label_ids, n_classes: int, diversity_pairs: int, multimodality_pairs: int, seed: int = 0):
    """The two pair tables of kg_cls_scores for N samples with class ids ``label_ids`` - Action2Motion's sampling, on the
    host with numpy only: (div_pairs (Sd, 2), mm_pairs (n_classes * Sl, 2)) int32 row indices.  ONE
    ``np.random.RandomState(seed)``, drawn in this order:

      1. ``first = choice(N, Sd, replace=False)``, then ``second = choice(N, Sd, replace=False)``: diversity pair p is
         (first[p], second[p]);
      2. for every class c = 0 .. n_classes - 1 with its n_c members in index order: ``choice(n_c, Sl, replace=False)``
         twice, mapped to row indices: multimodality pair c * Sl + q is (first_c[q], second_c[q]).

    The two draws of a pair are independent: a pair may hold the same row twice.  ValueError when Sd > N, when a class has
    fewer than Sl members or when a label is outside [0, n_classes)."""
    lab = np.asarray(label_ids).astype(np.int64).reshape(-1)
    n, k, sd, sl = lab.size, int(n_classes), int(diversity_pairs), int(multimodality_pairs)
    if k < 1 or sd < 1 or sl < 1:
        raise ValueError("cls_pair_tables: n_classes=%d, diversity_pairs=%d, multimodality_pairs=%d must be >= 1" % (k, sd, sl))
    if lab.size and (lab.min() < 0 or lab.max() >= k):
        raise ValueError("cls_pair_tables: a label outside [0, %d)" % k)
    if sd > n:
        raise ValueError("cls_pair_tables: diversity_pairs=%d above the %d samples" % (sd, n))
    members = [np.flatnonzero(lab == c) for c in range(k)]
    for c, m in enumerate(members):
        if m.size < sl:
            raise ValueError("cls_pair_tables: class %d has %d samples, multimodality_pairs=%d needed" % (c, m.size, sl))
    rng = np.random.RandomState(int(seed))
    first = rng.choice(n, sd, replace=False)
    second = rng.choice(n, sd, replace=False)
    div = np.stack([first, second], 1).astype(np.int32)
    mm = np.empty((k * sl, 2), dtype=np.int32)
    for c, m in enumerate(members):
        a = rng.choice(m.size, sl, replace=False)
        b = rng.choice(m.size, sl, replace=False)
        mm[c * sl:(c + 1) * sl, 0], mm[c * sl:(c + 1) * sl, 1] = m[a], m[b]
    return div, mm


def _classifier_pass(clf, x, ids: Optional[np.ndarray], batch: int, want_pred: bool = False):
    """features (N, d) and the correct count (0-d int64 on the device, None without labels) of x in chunks of ``batch``;
    ``want_pred``: (features, pred (N,) int32) instead, every chunk written into its rows of ONE matrix / vector
    (``cls_head_fwd(feat_out=, pred_out=)``: no cat, no host read, no stock add)"""
    dev = next(clf.parameters()).device
    x = torch.as_tensor(x) if not torch.is_tensor(x) else x
    if want_pred:
        n = int(x.shape[0])
        feat = torch.empty((n, clf.feat_dim), dtype=torch.float32, device=dev)
        pred = torch.empty(n, dtype=torch.int32, device=dev)
        with torch.no_grad():
            for lo in range(0, n, batch):
                hi = min(n, lo + batch)
                h = clf._trunk(x[lo:hi].to(dev, dtype=torch.float32))
                _native.cls_head_fwd(h, clf.fc1.weight.detach(), clf.fc1.bias.detach(), clf.fcn.weight.detach(),
                                     clf.fcn.bias.detach(), None, feat_out=feat[lo:hi], pred_out=pred[lo:hi])
        return feat, pred
    feats, correct = [], None
    with torch.no_grad():
        for lo in range(0, x.shape[0], batch):
            xb = x[lo:lo + batch].to(dev, dtype=torch.float32)
            yb = None if ids is None else torch.as_tensor(ids[lo:lo + batch], dtype=torch.int64).to(dev)
            out = clf.classify(xb, yb)
            feats.append(out["features"])
            if yb is not None:
                c = out["correct"].to(torch.int64)
                correct = c if correct is None else correct + c
    return torch.cat(feats, 0), correct


def classifier_scores(clf, gen, labels_gen, real, labels_real=None, per_class: Optional[int] = None, batch: int = 512,
                      class_fd: bool = True, diversity_pairs: int = 0, multimodality_pairs: int = 0, pair_seed: int = 0) -> dict:
    """The protocol of Action2Motion / ACTOR with a ``classifier.Classifier`` trained on the user's own data:
    ``accuracy`` (and the integer ``correct``) - the recognition accuracy of the generated samples ``gen`` (N, C, T, V)
    against their conditioning labels; ``accuracy_real`` when ``labels_real`` is given; ``feature_fd`` - the Frechet distance
    of all generated against all real features as one set (``frechet_features`` without labels); with ``labels_real``
    also ``feature_fd_class_mean`` / ``feature_fd_per_class`` (``frechet_features`` with both label vectors and
    ``per_class``; ``class_fd=False`` leaves these two out).  Labels are one-hot rows or class ids.  Features are computed in chunks of ``batch`` without autograd;
    the Frechet values stay fp64 device tensors, the accuracies are host numbers (one read); ``features_gen`` /
    ``features_real`` (N, d) are handed back as well.

    ``diversity_pairs`` and ``multimodality_pairs`` both above 0: one kg_cls_scores call on the generated set
    with the tables ``cls_pair_tables(labels_gen, clf.n_classes, ..., pair_seed)`` also gives ``diversity``,
    ``multimodality`` (0-d fp64), ``correct_per_class`` and ``count_per_class`` (K,) int32, ``pred_gen`` (N,) int32 and
    ``pair_tables``; with ``labels_real`` a second call with the real set's own tables gives ``diversity_real`` /
    ``multimodality_real`` - all device tensors, no extra host read."""
    n_g, n_r = int(gen.shape[0]), int(real.shape[0])
    ids_g, _ = _label_ids(labels_gen, n_g, "labels_gen")
    ids_r = None if labels_real is None else _label_ids(labels_real, n_r, "labels_real")[0]
    sd, sl = int(diversity_pairs), int(multimodality_pairs)
    if (sd > 0) != (sl > 0) or sd < 0 or sl < 0:
        raise ValueError("classifier_scores: diversity_pairs=%d and multimodality_pairs=%d: both 0 or both above 0" % (sd, sl))
    if sd:
        return _classifier_scores_pairs(clf, gen, ids_g, real, ids_r, per_class, batch, class_fd, sd, sl, int(pair_seed))
    feat_g, cor_g = _classifier_pass(clf, gen, ids_g, batch)
    feat_r, cor_r = _classifier_pass(clf, real, ids_r, batch)
    out = {"correct": int(cor_g), "features_gen": feat_g, "features_real": feat_r}
    out["accuracy"] = out["correct"] / float(n_g)
    if cor_r is not None:
        out["correct_real"] = int(cor_r)
        out["accuracy_real"] = out["correct_real"] / float(n_r)
    out["feature_fd"] = frechet_features(feat_g, feat_r)["mean"]
    if ids_r is not None and class_fd:
        res = frechet_features(feat_g, feat_r, ids_g, ids_r, per_class)
        out["feature_fd_class_mean"], out["feature_fd_per_class"] = res["mean"], res["values"]
    return out


def _classifier_scores_pairs(clf, gen, ids_g, real, ids_r, per_class, batch, class_fd, sd, sl, seed) -> dict:
    """``classifier_scores`` with the pair counts on: every set goes through the trunk once, its chunks land in one feature
    matrix and one prediction vector, and ONE kg_cls_scores call per labelled set gives the integer counts and the means"""
    K = int(clf.n_classes)
    feat_g, pred_g = _classifier_pass(clf, gen, None, batch, want_pred=True)
    feat_r, pred_r = _classifier_pass(clf, real, None, batch, want_pred=True)
    dev = feat_g.device

    def scores(feat, pred, ids):
        div, mm = cls_pair_tables(ids, K, sd, sl, seed)
        res = _native.cls_scores([feat], [pred], torch.as_tensor(ids, dtype=torch.int64).to(dev), torch.as_tensor(div).to(dev),
                                 torch.as_tensor(mm).to(dev), K)
        return res, (div, mm)

    res_g, tables_g = scores(feat_g, pred_g, ids_g)
    res_r, tables_r = scores(feat_r, pred_r, ids_r) if ids_r is not None else (None, None)
    # (the ONE host read: the counts of both sets)
    counts = torch.cat([res_g["correct"]] + ([] if res_r is None else [res_r["correct"]])).tolist()
    out = {"correct": int(counts[0]), "features_gen": feat_g, "features_real": feat_r}
    out["accuracy"] = out["correct"] / float(feat_g.shape[0])
    if res_r is not None:
        out["correct_real"] = int(counts[1])
        out["accuracy_real"] = out["correct_real"] / float(feat_r.shape[0])
    out["feature_fd"] = frechet_features(feat_g, feat_r)["mean"]
    if ids_r is not None and class_fd:
        res = frechet_features(feat_g, feat_r, ids_g, ids_r, per_class)
        out["feature_fd_class_mean"], out["feature_fd_per_class"] = res["mean"], res["values"]
    out.update(diversity=res_g["scores64"][0, 1], multimodality=res_g["scores64"][0, 2],
               correct_per_class=res_g["correct_per_class"][0], count_per_class=res_g["count_per_class"],
               pred_gen=pred_g, pair_tables=tables_g)
    if res_r is not None:
        out.update(diversity_real=res_r["scores64"][0, 1], multimodality_real=res_r["scores64"][0, 2], pred_real=pred_r,
                   pair_tables_real=tables_r)
    return out


# ---- nearest training samples, memorisation scores, the 1-NN two-sample test (kg_nn.hip) --------------------

NN_TWO_SAMPLE_NAMES = ("acc_real", "acc_fake", "acc")


def _nn_side(x, who: str, what: str):
    """(samples (n, C, T, V) where they lie, (scale, shift) or None, the labels the object carries or None) of one side of a
    search: a batch, or a ``train.ResidentDataset`` - its ``data`` is on the device, cropped, NOT normalised, and is searched
    in place through the dataset's affine"""
    if all(hasattr(x, f) for f in ("fits", "data", "scale", "shift")):
        if not x.fits or x.data is None:
            raise ValueError("%s: the ResidentDataset given as %s does not fit the device (fits=False): pass the samples"
                             % (who, what))
        affine = (float(x.scale), float(x.shift))
        return x.data, None if affine == (1.0, 0.0) else affine, getattr(x, "labels", None)
    return _as_f32(x), None, None


def _nn_check_pair(q: torch.Tensor, b: torch.Tensor, who: str, names=("query", "base")):
    if q.dim() != 4 or b.dim() != 4:
        raise ValueError("%s: samples are (N, C, T, V), got %s and %s" % (who, tuple(q.shape), tuple(b.shape)))
    if q.shape[1:] != b.shape[1:]:
        raise ValueError("%s: %s samples %s and %s samples %s differ in shape"
                         % (who, names[0], tuple(q.shape[1:]), names[1], tuple(b.shape[1:])))


def _nn_check_k(k: int, N: int, exclude_self: bool, who: str):
    most = min(_native.NN_MAX_K, N - (1 if exclude_self else 0))
    if not 1 <= k <= most:
        raise ValueError("%s: k=%d outside [1, min(%d, N=%d%s)]" % (who, k, _native.NN_MAX_K, N, " - 1" if exclude_self else ""))


NN_METHODS = ("exact", "gram")


def _nn_method(method, who: str) -> bool:
    """True for the matrix-core pre-filter (kg_nn_gram: the same bits), False for the exact search"""
    if method not in NN_METHODS:
        raise ValueError("%s: method=%r is none of %s" % (who, method, ", ".join(repr(m) for m in NN_METHODS)))
    return method == "gram"


def _nn_rows(q, idx_q: np.ndarray, qa, b, idx_b: np.ndarray, ba, k: int, exclude_self: bool, gram: bool = False,
             stats: Optional[list] = None):
    """one kg_nn call on the samples idx_q (classes, Q) of q and idx_b (classes, N) of b -> (idx, d2) (classes, Q, k);
    ``gram``: one kg_nn_gram call (and one kg_nn_norms of the base) instead, its (classes, 2) stats appended to ``stats``"""
    q, b = _as_cuda(q), _as_cuda(b)
    qv, bv, d_outer, d_inner = _view_pair(q, idx_q, b, idx_b)
    if gram:
        idx, d2, st = _native.nn_gram([qv.t], qv.sc, qv.sp, qv.so, bv, idx_q.shape[1], idx_b.shape[1], d_outer, d_inner,
                                      idx_q.shape[0], k, exclude_self=exclude_self, q_affine=qa, b_affine=ba)
        if stats is not None:
            stats.append(st[0])
        return idx[0], d2[0]
    return _native.nn(qv, bv, idx_q.shape[1], idx_b.shape[1], d_outer, d_inner, idx_q.shape[0], k,
                      exclude_self=exclude_self, q_affine=qa, b_affine=ba)


def _nn_gram_k(k: int, who: str):
    if k >= _native.NN_MAX_K:
        raise ValueError("%s: method='gram' keeps more than k candidates per row: k=%d must be below %d" % (who, k, _native.NN_MAX_K))


def nearest(query, base, k: int = 1, exclude_self: bool = False, labels_query=None, labels_base=None,
            per_class: Optional[int] = None, method: str = "exact") -> dict:
    """The k nearest ``base`` samples of every ``query`` sample (a sample = one point of dimension C*T*V) in one kg_nn call:
    exact, ties to the lower index, a duplicate is a neighbour at distance 0.

    query (Nq, C, T, V), base (Nb, C, T, V): CUDA tensors, CPU tensors or numpy, read in place where the samples lie evenly
    spaced (a crop in T included); either may be a ``train.ResidentDataset``, whose unnormalised ``data`` is searched in
    place with the dataset's (scale, shift) - nothing is copied - and whose labels stand in for missing ``labels_base``.
    Without labels it is ONE global search.  With labels (one-hot or ids) the search runs class by class on the selection of
    ``prdc``: the first ``per_class`` samples of every class on each side (default: all; a side's classes must then hold the
    same number).  ``exclude_self`` leaves pair i == j out by index: a set searched against itself.
    Returns device tensors ``idx`` (K, Q, k) int32 - the neighbour's position inside its class's selection -, ``d2``
    (K, Q, k) squared distances, non-decreasing along k, ``index`` (K, Q, k) int64 - the neighbour's index in ``base`` -, and
    the selections ``rows_query`` (K, Q), ``rows_base`` (K, N) as numpy indices.  No host sync (labels that live on the
    device are read once).
    ``method="gram"``: the same bits through kg_nn_gram - the matrix-core pre-filter with exact re-score (k below
    32) -; the result then carries ``certified`` / ``fallback`` (K,) int32: the rows the filter's certificate settled and the
    rows that went through the exact search."""
    who = "nearest"
    gram = _nn_method(method, who)
    q, qa, _ = _nn_side(query, who, "query")
    b, ba, own = _nn_side(base, who, "base")
    _nn_check_pair(q, b, who)
    if labels_base is None and labels_query is not None:
        labels_base = own
    lab_q, kq = _label_ids(labels_query, q.shape[0], "labels_query", who)
    lab_b, kb = _label_ids(labels_base, b.shape[0], "labels_base", who)
    classes = max(kq, kb)
    if classes < 1:
        raise ValueError("%s: no samples" % who)
    idx_q = _class_rows(lab_q, classes, per_class, "query", who)
    idx_b = _class_rows(lab_b, classes, per_class, "base", who)
    _nn_check_k(k, idx_b.shape[1], exclude_self, who)
    if gram:
        _nn_gram_k(k, who)
    stats = []
    idx, d2 = _nn_rows(q, idx_q, qa, b, idx_b, ba, k, exclude_self, gram, stats)
    rows = torch.as_tensor(idx_b, device=idx.device)
    index = torch.gather(rows, 1, idx.reshape(classes, -1).long()).reshape(idx.shape)
    out = dict(idx=idx, d2=d2, index=index, rows_query=idx_q, rows_base=idx_b)
    if gram:
        out.update(certified=stats[0][:, 0], fallback=stats[0][:, 1])
    return out


def _share(count: torch.Tensor, of: int) -> torch.Tensor:
    """an integer tally over its denominator: evaluated in float64, rounded once"""
    return (count.double() / float(of)).float()


def memorisation(gen, labels_gen, train, labels_train=None, heldout=None, labels_heldout=None, train_loo=None,
                 method: str = "exact") -> dict:
    """Does the generator replay its training set?  One global search gen -> train (k = 1) and one train -> train (k = 1,
    leave-one-out); a generated sample that lies closer to its nearest training sample than that sample lies to any OTHER
    training sample counts as a copy (authenticity, Alaa et al. 2022).

    gen (Ng, C, T, V) with its conditioning labels; ``train``: a batch with ``labels_train``, or a ``train.ResidentDataset``
    (searched in place, its own labels by default).  ``train_loo``: the (Nt,) leave-one-out distances of an earlier call
    (``train_loo_d2`` of its result) - the train -> train pass depends on the training set alone and is then not repeated.
    Returns device tensors: ``nn_index`` (Ng,) int64 and ``nn_d2`` (Ng,) - the nearest training sample i* of every generated
    sample and its squared distance -, ``authentic`` (Ng,) bool = [d2(f_j, r_i*) >= d2_loo(r_i*)], ``authenticity`` = their
    share, ``label_agreement`` = the share whose nearest training sample carries the conditioning label, ``counts`` (2,)
    int64 (authentic, agreeing), ``train_loo_d2`` (Nt,).  With ``heldout`` (real samples the generator never saw, with
    ``labels_heldout``) the same for it as queries under ``heldout_*``: what a perfect generator scores.  Tallies are
    integers on the device; the shares are evaluated in float64 and rounded once.
    ``method="gram"``: every search through kg_nn_gram (the same bits; ``nearest``); ``certified`` / ``fallback`` (and
    ``heldout_*``, ``train_loo_*`` when that pass ran) are then the 0-d int32 row counts of each search."""
    who = "memorisation"
    gram = _nn_method(method, who)
    t, ta, own = _nn_side(train, who, "train")
    if labels_train is None:
        labels_train = own
    if labels_train is None:
        raise ValueError("%s: labels_train is needed (the training set carries none)" % who)
    sets = [("", "gen", _as_f32(gen), labels_gen, "labels_gen")]
    if heldout is not None:
        sets.append(("heldout_", "heldout", _as_f32(heldout), labels_heldout, "labels_heldout"))
    nt = t.shape[0] if t.dim() == 4 else 0
    labs = []
    for _, what, x, lab, name in sets:
        _nn_check_pair(x, t, who, (what, "train"))
        if lab is None:
            raise ValueError("%s: %s is needed" % (who, name))
        labs.append(_label_ids(lab, x.shape[0], name, who)[0])
    lab_t = _label_ids(labels_train, nt, "labels_train", who)[0]
    if nt < 2:
        raise ValueError("%s: the leave-one-out pass needs at least 2 training samples, got %d" % (who, nt))
    if train_loo is not None and (train_loo.dim() != 1 or train_loo.shape[0] != nt or train_loo.dtype != torch.float32):
        raise ValueError("%s: train_loo must be the (%d,) fp32 leave-one-out distances of this training set" % (who, nt))
    t = _as_cuda(t)                             # (once: up to three searches read it)
    rows_t = np.arange(nt)[None, :]
    out, stats = {}, []
    if train_loo is None:
        train_loo = _nn_rows(t, rows_t, ta, t, rows_t, ta, 1, True, gram, stats)[1].reshape(-1)
        if gram:
            out.update(train_loo_certified=stats[-1][0, 0], train_loo_fallback=stats[-1][0, 1])
    out["train_loo_d2"] = train_loo
    lab_t = torch.as_tensor(lab_t, device=train_loo.device)
    for (pre, _, x, _, _), lab in zip(sets, labs):
        idx, d2 = _nn_rows(x, np.arange(x.shape[0])[None, :], None, t, rows_t, ta, 1, False, gram, stats)
        if gram:
            out.update({pre + "certified": stats[-1][0, 0], pre + "fallback": stats[-1][0, 1]})
        idx, d2 = idx.reshape(-1).long(), d2.reshape(-1)
        authentic = d2 >= train_loo[idx]
        agree = lab_t[idx] == torch.as_tensor(lab, device=idx.device)
        counts = torch.stack([authentic.sum(), agree.sum()])
        out.update({pre + "nn_index": idx, pre + "nn_d2": d2, pre + "authentic": authentic, pre + "counts": counts,
                    pre + "authenticity": _share(counts[0], x.shape[0]),
                    pre + "label_agreement": _share(counts[1], x.shape[0])})
    return out


MEMORISATION_NAMES = ("authenticity", "label_agreement")


def _as_points(x, who: str, what: str):
    """a (n, d) feature matrix as (n, 1, 1, d) samples - one point of dimension d each, searched with d_outer = 1 -, its rows
    read in place (a column slice of a wider matrix keeps its row stride)"""
    x = _as_f32(x)
    if x.dim() != 2:
        raise ValueError("%s: %s is a (n, d) feature matrix, got %s" % (who, what, tuple(x.shape)))
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    return x.unsqueeze(1).unsqueeze(1)


def memorisation_features(feat_gen, labels_gen, feat_train, labels_train, feat_heldout=None, labels_heldout=None,
                          train_loo=None, method: str = "exact") -> dict:
    """``memorisation`` in a feature space: (n, d) fp32 matrices - a classifier's features of the generated, the training and
    (optionally) the held-out samples - searched as points of dimension d (kg_nn with d_outer = 1).  Arguments, result keys
    and their meaning are those of ``memorisation``; a copy is now a generated sample whose FEATURES lie closer to a training
    sample's than that sample's lie to any other training sample's.  ValueError for argument errors, before the GPU is
    touched."""
    who = "memorisation_features"
    gen = _as_points(feat_gen, who, "feat_gen")
    train = _as_points(feat_train, who, "feat_train")
    held = None if feat_heldout is None else _as_points(feat_heldout, who, "feat_heldout")
    if labels_train is None:
        raise ValueError("%s: labels_train is needed" % who)
    return memorisation(gen, labels_gen, train, labels_train, held, labels_heldout, train_loo, method)


def memorisation_sets(sets, labels, train, labels_train=None, train_loo=None, method: str = "exact", train_norms=None) -> dict:
    """``memorisation`` of 1 to 4 generated sets that share one label vector against ONE training set, in ONE kg_nn_sets call
    (two launches whatever the number of sets) plus ONE kg_nn_scores launch: the Evaluator's form.

    ``sets``: a list of (n, C, T, V) batches or of (n, d) feature matrices, all of one shape; ``labels`` (n,) their shared
    conditioning labels; ``train``: a batch, a ``train.ResidentDataset`` (searched in place, its own labels by default) or a
    (N, d) feature matrix, with ``labels_train``; ``train_loo`` as in ``memorisation``.  Returns device tensors ``nn_index``
    (nsets, n) int64, ``nn_d2`` (nsets, n), ``counts`` (nsets, 2) int64 (authentic, agreeing), ``authenticity`` and
    ``label_agreement`` (nsets,) fp32, ``counts_per_class`` (nsets, classes, 2) int32 by the conditioning label, and
    ``train_loo_d2`` (N,).  Entry g of each equals, bit for bit, the same key of ``memorisation(sets[g], labels, train, ...)``
    (``memorisation_features`` for matrices).  No host synchronisation (labels that live on the device are read once).
    ``method="gram"``: ONE kg_nn_gram call instead of kg_nn_sets (the same bits); ``certified`` / ``fallback``
    (nsets,) int32 are then its row counts; ``train_norms``: ``_native.nn_norms`` of the training set as it is searched here
    (else that launch is made), handed back as ``train_norms``."""
    who = "memorisation_sets"
    gram = _nn_method(method, who)
    sets = list(sets) if isinstance(sets, (list, tuple)) else None
    if not sets or len(sets) > _native.NN_MAX_SETS:
        raise ValueError("%s: sets is a list of 1 to %d batches or feature matrices" % (who, _native.NN_MAX_SETS))
    xs = [_as_f32(x) for x in sets]
    if any(x.shape != xs[0].shape for x in xs):
        raise ValueError("%s: the sets differ in shape: %s" % (who, [tuple(x.shape) for x in xs]))
    flat = xs[0].dim() == 2
    if flat:
        xs = [_as_points(x, who, "set %d" % g) for g, x in enumerate(xs)]
        if not all(hasattr(train, f) for f in ("fits", "data", "scale", "shift")):
            train = _as_points(train, who, "train")
    t, ta, own = _nn_side(train, who, "train")
    if labels_train is None:
        labels_train = own
    if labels_train is None:
        raise ValueError("%s: labels_train is needed (the training set carries none)" % who)
    for g, x in enumerate(xs):
        _nn_check_pair(x, t, who, ("set %d" % g, "train"))
    if labels is None:
        raise ValueError("%s: labels is needed" % who)
    n, nt = xs[0].shape[0], t.shape[0]
    lab, kq = _label_ids(labels, n, "labels", who)
    lab_t, kt = _label_ids(labels_train, nt, "labels_train", who)
    if nt < 2:
        raise ValueError("%s: the leave-one-out pass needs at least 2 training samples, got %d" % (who, nt))
    if n < 1:
        raise ValueError("%s: the sets hold no sample" % who)
    if train_loo is not None and (train_loo.dim() != 1 or train_loo.shape[0] != nt or train_loo.dtype != torch.float32):
        raise ValueError("%s: train_loo must be the (%d,) fp32 leave-one-out distances of this training set" % (who, nt))
    classes = max(kq, kt, 1)
    if classes > _native.NN_SCORES_MAX_CLASSES:
        raise ValueError("%s: %d classes, at most %d" % (who, classes, _native.NN_SCORES_MAX_CLASSES))
    t = _as_cuda(t)
    xs = [_as_cuda(x) for x in xs]
    rows, rows_t = np.arange(n)[None, :], np.arange(nt)[None, :]
    if train_loo is None:
        train_loo = _nn_rows(t, rows_t, ta, t, rows_t, ta, 1, True, gram)[1].reshape(-1)
    views = [_view_pair(x, rows, t, rows_t) for x in xs]
    if any((v[0].sc, v[0].sp, v[0].so, v[2], v[3]) != (views[0][0].sc, views[0][0].sp, views[0][0].so, views[0][2], views[0][3])
           for v in views):                     # the sets are walked with shared strides
        views = [_view_pair(x.contiguous(), rows, t, rows_t) for x in xs]
    qv, bv, d_outer, d_inner = views[0]
    extra = {}
    if gram:
        if train_norms is None:
            train_norms = _native.nn_norms(bv, nt, d_outer, d_inner, 1, ta)
        idx, d2, st = _native.nn_gram([v[0].t for v in views], qv.sc, qv.sp, qv.so, bv, n, nt, d_outer, d_inner, 1, 1, b_affine=ta,
                                      base_norms=train_norms)
        extra = dict(certified=st[:, 0, 0], fallback=st[:, 0, 1], train_norms=train_norms)
    else:
        idx, d2 = _native.nn_sets([v[0].t for v in views], qv.sc, qv.sp, qv.so, bv, n, nt, d_outer, d_inner, 1, 1, b_affine=ta)
    dev = idx.device
    res = _native.nn_scores(idx, d2, torch.as_tensor(lab.astype(np.int32), device=dev),
                            torch.as_tensor(lab_t.astype(np.int32), device=dev), train_loo, classes, per_class=True)
    return dict(nn_index=idx.reshape(len(xs), n).long(), nn_d2=d2.reshape(len(xs), n), counts=res["counts"],
                authenticity=res["scores"][:, 0], label_agreement=res["scores"][:, 1],
                counts_per_class=res["counts_per_class"], train_loo_d2=train_loo, **extra)


def nn_two_sample(gen, real, labels_gen=None, labels_real=None, per_class: Optional[int] = None, method: str = "exact") -> dict:
    """The leave-one-out 1-NN two-sample test (Lopez-Paz & Oquab 2017; Xu et al. 2018) per class: every sample of R u F, with
    |R| = |F| = n per class, is classified by its nearest OTHER sample of the union; the accuracy of an indistinguishable
    generator is 0.5, ``acc_fake`` -> 0 means copies of real samples, -> 1 a separable (or collapsed) fake set.

    Built from four k = 1 searches (R -> R and F -> F leave-one-out, R -> F, F -> R); a tie between a real and a fake
    neighbour goes to the real one: real i is correct iff d2_RR(i) <= d2_RF(i), fake j iff d2_FF(j) < d2_FR(j).  Arguments
    and selection as ``prdc``.  Returns device tensors ``acc_real``, ``acc_fake``, ``acc`` (K,), ``counts`` (K, 2) int64
    (correct reals, correct fakes) and ``mean`` (3,) - the class means in the order NN_TWO_SAMPLE_NAMES.  Tallies are
    integers on the device; every quotient is evaluated in float64 and rounded once.
    ``method="gram"``: the four searches through kg_nn_gram (the same bits); ``certified`` / ``fallback`` (K,) int32 are then
    the row counts summed over the four."""
    who = "nn_two_sample"
    gram = _nn_method(method, who)
    gen, real = _as_f32(gen), _as_f32(real)
    _nn_check_pair(gen, real, who, ("gen", "real"))
    lab_g, kg = _label_ids(labels_gen, gen.shape[0], "labels_gen", who)
    lab_r, kr = _label_ids(labels_real, real.shape[0], "labels_real", who)
    classes = max(kg, kr)
    if classes < 1:
        raise ValueError("%s: no samples" % who)
    idx_r = _class_rows(lab_r, classes, per_class, "real", who)
    idx_g = _class_rows(lab_g, classes, per_class, "fake", who)
    n = idx_r.shape[1]
    if idx_g.shape[1] != n:
        raise ValueError("%s: %d real and %d fake samples per class (the test needs |R| = |F|: pass per_class)"
                         % (who, n, idx_g.shape[1]))
    if n < 2:
        raise ValueError("%s: %d samples per class and set, the leave-one-out search needs 2" % (who, n))
    gen, real = _as_cuda(gen), _as_cuda(real)
    d, stats = {}, []
    for key, (a, ia), (b, ib) in (("rr", (real, idx_r), (real, idx_r)), ("rf", (real, idx_r), (gen, idx_g)),
                                  ("ff", (gen, idx_g), (gen, idx_g)), ("fr", (gen, idx_g), (real, idx_r))):
        d[key] = _nn_rows(a, ia, None, b, ib, None, 1, key in ("rr", "ff"), gram, stats)[1].reshape(classes, n)
    counts = torch.stack([(d["rr"] <= d["rf"]).sum(1), (d["ff"] < d["fr"]).sum(1)], dim=1)
    total = counts.sum(0)
    out = dict(acc_real=_share(counts[:, 0], n), acc_fake=_share(counts[:, 1], n), acc=_share(counts.sum(1), 2 * n),
               counts=counts,
               mean=torch.stack([_share(total[0], classes * n), _share(total[1], classes * n),
                                 _share(total.sum(), 2 * classes * n)]))
    if gram:
        tot = torch.stack(stats).sum(0)
        out.update(certified=tot[:, 0], fallback=tot[:, 1])
    return out


def select_reference_samples(feeder, classes: Optional[Sequence[int]] = None, t_size: int = 64, per_class: int = 100):
    """The sample selection of mmd-actions.py:131-163, vectorised on the label vector.

    For class classes[c] (default: the ``arange(10 if h36m else 60)`` of the script) the first ``per_class`` samples
    with that label are taken in index order - scanning from index 0 for the first class and from index 1 for every
    later one (the script resets its index to 0 and increments it at once) - each read as ``feeder[i]`` (normalised
    when the feeder normalises, first person for NTU) and cropped to ``t_size`` frames.  Returns (data (K*per_class,
    C, t, V) fp32 numpy, labels (K*per_class,): the position of the class in ``classes``, dataset indices).  A class
    with fewer samples raises ValueError (the script dies with an IndexError)."""
    if classes is None:
        classes = np.arange(10 if feeder.dataset == "h36m" else 60)
    classes = np.asarray(classes)
    lab = np.asarray(feeder.label)
    picks = []
    for c, cv in enumerate(classes):
        start = 0 if c == 0 else 1
        idx = np.flatnonzero(lab[start:] == cv)[:per_class] + start
        if idx.size < per_class:
            raise ValueError("select_reference_samples: class %d (label %d) has %d samples from index %d, %d needed"
                             % (c, int(cv), idx.size, start, per_class))
        picks.append(idx)
    index = np.concatenate(picks) if picks else np.zeros(0, dtype=np.int64)
    order = np.argsort(index, kind="stable")            # the memory map is read forwards
    raw = np.empty((index.size, feeder.C, min(t_size, feeder.T), feeder.V), dtype=np.float32)
    sel = index[order]
    block = feeder.data[sel, :, :t_size, :, 0] if feeder.dataset == "ntu" else feeder.data[sel, :, :t_size]
    block = np.asarray(block)
    if feeder.norm:
        block = 2 * ((block - feeder.min) / (feeder.max - feeder.min)) - 1     # Feeder.__getitem__, elementwise
    raw[order] = block
    labels = np.repeat(np.arange(classes.size), per_class)
    return raw, labels, index


# ---- reconstruction error: projection of real motions into W (project.Projector, kg_proj.hip) -----------------------

RECON_NAMES = ("recon_pos", "recon_vel", "recon_bone")


def reconstruction(G, real, labels_real=None, dataset: str = "ntu", per_class: Optional[int] = None, scale: float = 1.0,
                   shift: float = 0.0, mask=None, **projector_kw) -> dict:
    """How well the generator can represent given motions: the first ``per_class`` real samples of every class (``frechet``'s
    conventions: one-hot rows or class ids, default all, ragged classes raise) are projected into W in batches of the
    Projector's ``n`` (``projector_kw``: the arguments of ``project.Projector``; default n = min(samples, 64)) and scored by the
    terms of their best objective.  Smaller is better; on held-out data this is a per-sample recall without a k-NN radius or a
    feature extractor, on training data it complements ``memorisation``.  Leaves on the device: ``values`` (K, 3) the class
    means of the best L_pos, L_vel, L_bone (``RECON_NAMES``), ``mean`` (3,) their mean over classes, ``per_sample`` (K, P, 4) =
    [L, L_pos, L_vel, L_bone], ``best_w`` (K, P, D), ``recon`` (K, P, C, T, V) and ``nonfinite`` (K, P) int32.  ``scale`` /
    ``shift`` / ``mask``: as in ``Projector.project``, shared by all samples (mask (T, V))."""
    from .project import Projector
    who = "reconstruction"
    real = _as_f32(real)
    if real.dim() != 4:
        raise ValueError("%s: real samples are (N, C, T, V), got %s" % (who, tuple(real.shape)))
    lab, K = _label_ids(labels_real, real.shape[0], "labels_real", who)
    idx = _class_rows(lab, K, per_class, "real", who)
    P = idx.shape[1]
    flat, classes = idx.reshape(-1), np.repeat(np.arange(K), P)
    n = int(projector_kw.pop("n", min(flat.size, 64)))
    proj = Projector(G, n, dataset=dataset, **projector_kw)
    dev = proj.device
    real = real.to(dev)
    rows = []
    for b in range(0, flat.size, n):
        cnt = min(n, flat.size - b)
        pad = np.zeros(n - cnt, dtype=np.int64)                          # a short last batch is filled up with its first sample
        sel = np.concatenate([flat[b:b + cnt], flat[b:b + 1][pad]])
        lb = np.concatenate([classes[b:b + cnt], classes[b:b + 1][pad]])
        out = proj.project(real.index_select(0, torch.as_tensor(sel, device=dev)), lb, mask=mask, scale=scale, shift=shift)
        rows.append({k: out[k][:cnt] for k in ("best_loss", "best_w", "recon", "nonfinite")})
    cat = {k: torch.cat([r[k] for r in rows], 0) for k in rows[0]}
    per_sample = cat["best_loss"].reshape(K, P, 4)
    values = per_sample[:, :, 1:].mean(1)
    return dict(values=values, mean=values.mean(0), per_sample=per_sample, best_w=cat["best_w"].reshape(K, P, -1),
                recon=cat["recon"].reshape((K, P) + tuple(cat["recon"].shape[1:])), nonfinite=cat["nonfinite"].reshape(K, P))
