"""Scoring the generator during training and keeping the best weights on the device.

The live weights of a WGAN-GP generator jump from step to step and the reference's released generators are iterations
picked by hand.  ``Evaluator`` picks them: one ``evaluate()`` is ONE fixed launch sequence - a captured
hipGraph on a single stream - that

  1. draws one ``Sampler`` round of ``pairs`` samples per class from every named generator (all Samplers share one seed
     and advance their counters in lock-step: every generator is scored on the same z, noise and truncation draws);
  2. lays the round out NCHW where ``joint`` mode needs each sample's (C, T) block contiguous (one copy into a static
     buffer, inside the replay);
  3. scores it with kg_mmd per requested mode - the reference protocol (``metrics.calculate_mmd``: one fake against one
     real sample per class, 14 bandwidths, per-class maximum) applied to ``pairs`` (fake, real) pairs per class and
     averaged over classes and pairs;
  4. kg_eval_record: appends (iteration, every score, improved) to a record on the device and decides whether the
     selected score is the best so far (strictly smaller; a NaN never wins);
  5. kg_copy_if: when it is, copies the selected generator - its flat parameters and every module buffer (BatchNorm
     running statistics and batch counters) - into a snapshot.

Five further score families add columns to the record, in this order (``FAMILIES`` is the one table that
the names, the set-up, the launch sequence, the Sampler list, the state and its compatibility check are all driven by):

  prdc          ``prdc_per_class > 0``: ``"<g>/precision"``, ``"<g>/recall"``, ``"<g>/density"``,
                ``"<g>/coverage"`` (larger is better) - ONE kg_prdc_sets call (three launches for all generators) against the
                real samples' k-th-neighbour radii (kg_prdc_radii);
  frechet       ``frechet_per_class > 0``: ``"<g>/pose_fd"`` / ``"<g>/motion_fd"`` (smaller is better) - ONE
                kg_frechet_sets call per mode (four launches for all generators) against the real side's cache
                (kg_frechet_real);
  classifier    ``classifier`` and ``classifier_per_class > 0``, the Action2Motion / ACTOR protocol in the
                feature space of a trained ``classifier.Classifier``: the round goes through its trunk and head in chunks of
                ``classifier_batch`` (plane slices read in place, features and predictions written into static matrices),
                then ONE kg_frechet_sets call against the real features' cache and ONE kg_cls_scores call for all
                generators: ``"<g>/accuracy"`` (larger is better), ``"<g>/feature_fd"`` (smaller is better),
                ``"<g>/diversity"`` and ``"<g>/multimodality"`` (closer to the real set's value - ``classifier_real`` - is
                better: recorded, never selected by);
  memorisation  ``memorisation`` (``"features"`` or ``"raw"``), whether the generators replay the training set
                ``memorisation_train``: every generator's query set - the classifier round's feature matrices in feature
                space, a round of ``memorisation_per_class`` samples per class in raw space - goes through ONE kg_nn_sets
                call (k = 1, two launches for all generators) against the training set and ONE kg_nn_scores launch:
                ``"<g>/authenticity"`` (the share of samples that lie no closer to their nearest training sample than that
                sample lies to another training sample: noise scores 1, a copier 0, the value to be near is
                ``memorisation_real["authenticity"]`` - recorded, never selected by) and ``"<g>/label_agreement"`` (the
                share whose nearest training sample carries the conditioning label; larger is better);
  kinematics    ``kinematics_per_class > 0``, whether the samples are bodies at all: ONE kg_kin_desc_sets
                launch over all generators' rounds and ONE kg_kin_scores call (two launches) measure, per descriptor, the
                class-averaged Wasserstein-1 distance to the real samples' descriptors (``kinematics_real`` holds their
                means): ``"<g>/bone_cv"``, ``"<g>/asymmetry"``, ``"<g>/speed"``, ``"<g>/accel"``, ``"<g>/jerk"``,
                ``"<g>/still"`` (all smaller is better; a generator that emits non-finite values records NaN, which never
                wins).

The rounds.  A family scores a Sampler round of its own count of samples per class from every generator, read in place
through strides - never the MMD round, so that the MMD columns stay bit for bit what they are without it.  The sharing rule
(``round_owners``): a family reads the round of the FIRST family, in the order above, that draws the same number of samples
per class; only that family - the round's owner - has Samplers, and its round runs inside its own scores, before any reader's.
Memorisation in feature space draws no round at all: it reads the classifier's feature matrices.

The real side.  A family is held against that many real samples per class, class by class on the device: selected and
uploaded once per count (families of equal count alias one tensor; nothing writes to it), and everything a family derives
from them - radii, Frechet caches, real features, leave-one-out distances, descriptors, the real side's own scores - is
computed once, at construction, from the data.  It is deterministic, so none of it is part of the state.

The record goes through the narrowest entry point that the families which are on allow: kg_eval_record (8 scores, smaller is
better), kg_eval_record2 (32 scores and a sense: precision .. coverage, accuracy and label_agreement are better when larger)
or, with the kinematic columns, kg_eval_record3 (64 scores).

Nothing synchronises the host; everything is read through pointers when the launches run, so the captured evaluation
follows the training replays in between.  ``records()``, ``best()`` and ``state_dict()`` read the device; the Evaluator
never writes to a generator.  Definitions the tests pin this against: tests/eval_def.py.
"""
from __future__ import annotations

import csv
import warnings
from typing import Callable, Dict, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _native as nv
from . import metrics
from .replay import capture_keeping
from .sample import Sampler


def pair_rows(labels, n_classes: int, pairs: int) -> np.ndarray:
    """Indices into a labelled sample set in the Sampler's row order: entry ``j * n_classes + c`` is the ``j``-th sample
    (in index order) whose label is ``c``.  ValueError when a class has fewer than ``pairs`` samples."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    rows = np.empty(pairs * n_classes, dtype=np.int64)
    for c in range(n_classes):
        idx = np.flatnonzero(lab == c)
        if idx.size < pairs:
            raise ValueError("pair_rows: class %d has %d samples, %d needed" % (c, idx.size, pairs))
        rows[c::n_classes] = idx[:pairs]
    return rows


def default_select(names: Sequence[str], modes: Sequence[str]) -> str:
    """``"ema/<mode>"`` when an averaged generator is scored, else ``"live/<mode>"``, else the first generator; the mode
    is ``avg`` when it is requested, else the first one"""
    mode = "avg" if "avg" in modes else modes[0]
    gen = "ema" if "ema" in names else ("live" if "live" in names else names[0])
    return "%s/%s" % (gen, mode)


NO_SENSE = ("diversity", "multimodality", "authenticity")      # closer to the real set's value is better: neither direction is
MEMORISATION_MODES = ("features", "raw")


def score_sense(name: str) -> str:
    """``"max"`` for precision / recall / density / coverage, accuracy and label_agreement (larger is better), ``"min"`` for the
    MMD modes, every Frechet distance and the six kinematic W1 distances; ValueError for diversity / multimodality / authenticity, which have no better
    direction"""
    last = str(name).rsplit("/", 1)[-1]
    if last in NO_SENSE:
        raise ValueError("score_sense: %r is better the closer it is to the real set's value: it cannot decide a selection" % (name,))
    return "max" if last in metrics.PRDC_NAMES or last in ("accuracy", "label_agreement") else "min"


def score_names(generators: Sequence[str], modes: Sequence[str], prdc: bool = False, frechet: Sequence[str] = (),
                classifier: bool = False, memorisation: bool = False, kinematics: bool = False) -> list:
    """The record's columns: ``"<g>/<mode>"`` generator by generator, then - with precision / recall / density / coverage
    on - ``"<g>/<name>"`` generator by generator in the order of ``metrics.PRDC_NAMES``, then - with the Frechet modes
    ``frechet`` (of ``metrics.FRECHET_MODES``) - ``"<g>/pose_fd"`` and / or ``"<g>/motion_fd"`` generator by generator, then -
    with ``classifier`` - ``"<g>/<name>"`` generator by generator in the order of ``metrics.CLS_NAMES``, then - with
    ``memorisation`` - ``"<g>/<name>"`` generator by generator in the order of ``metrics.MEMORISATION_NAMES``, then - with
    ``kinematics`` - ``"<g>/<name>"`` generator by generator in the order of ``metrics.KIN_NAMES``"""
    on = dict(prdc=prdc, frechet=frechet, classifier=classifier, memorisation=memorisation, kinematics=kinematics)
    names = ["%s/%s" % (g, m) for g in generators for m in modes]
    for f in FAMILIES:
        names += ["%s/%s" % (g, q) for g in generators for q in f.columns(on[f.key])]
    return names


def class_rows(labels, n_classes: int, per_class: int) -> np.ndarray:
    """(n_classes * per_class,) indices, class by class: the first ``per_class`` samples (in index order) of class 0, then of
    class 1, ...  ValueError when a class has fewer."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    rows = []
    for c in range(n_classes):
        idx = np.flatnonzero(lab == c)
        if idx.size < per_class:
            raise ValueError("class_rows: class %d has %d samples, %d needed" % (c, idx.size, per_class))
        rows.append(idx[:per_class])
    return np.concatenate(rows)


def write_metrics_csv(path: str, records: dict) -> None:
    """``metrics.csv``: a header, then one row per evaluation - iteration, every score (``repr`` of the fp32 value: it
    reads back bit for bit), improved (0 / 1)."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["iteration"] + list(records["names"]) + ["improved"])
        for it, row, imp in zip(records["iteration"], records["scores"], records["improved"]):
            w.writerow([int(it)] + [repr(float(v)) for v in row] + [int(imp)])


def _flat_storage(params):
    """The parameters as ONE flat fp32 tensor when they are views into one storage (``FlatParams``, the weight average):
    (flat, offsets in elements); else (None, None)."""
    st = params[0].untyped_storage()
    if any(p.untyped_storage().data_ptr() != st.data_ptr() or p.dtype != torch.float32 or not p.is_contiguous() for p in params):
        return None, None
    lo = min(p.storage_offset() for p in params)
    hi = max(p.storage_offset() + p.numel() for p in params)
    flat = torch.empty(0, dtype=torch.float32, device=params[0].device).set_(st, lo, (hi - lo,))
    return flat, [p.storage_offset() - lo for p in params]


def _kinematics_state(ev) -> dict:
    """what a state keeps of the kinematic columns: the count, the threshold and the skeleton tables"""
    return {"per_class": int(ev.kinematics_per_class), "still_eps": float(ev.kinematics_still_eps),
            "bones": [[int(v) for v in b] for b in ev.kinematics_bones],
            "mirror": [[int(v) for v in p] for p in ev.kinematics_mirror]}


class Family(NamedTuple):
    """One score family of the record.  The functions take the Evaluator - or an Evaluator-like object of before the family
    existed (``check_compatible``), which lacks its attributes: there the family is off."""
    key: str              # its key in the state and in ``round_owners``; its methods are _<key>_setup and _<key>_scores
    on: Callable          # (ev) -> what ``score_names`` takes for it: falsy when the family is off
    columns: Callable     # (that value) -> its column names per generator
    state: Callable       # (ev) -> what it contributes to the state: the options its columns depend on
    count: Callable       # (ev) -> the samples per class of the round it draws (0: none)
    samplers: str         # the attribute that holds its Samplers ({} unless it owns its round)
    off: Callable         # () -> the public attributes it has when it is off
    record: int           # the narrowest of RECORDS that takes its columns


RECORDS = (("eval_record", "EVAL_MAX_SCORES"), ("eval_record2", "EVAL2_MAX_SCORES"), ("eval_record3", "EVAL3_MAX_SCORES"))
FAMILIES = (
    Family("prdc", lambda ev: ev.prdc_per_class, lambda on: metrics.PRDC_NAMES if on else (),
           lambda ev: {"per_class": ev.prdc_per_class, "k": ev.prdc_k},
           lambda ev: ev.prdc_per_class, "prdc_samplers", lambda: dict(prdc_real=None, prdc_radii=None), 1),
    Family("frechet", lambda ev: ev.frechet_modes if ev.frechet_per_class else (), lambda modes: ["%s_fd" % f for f in modes],
           lambda ev: {"per_class": ev.frechet_per_class, "modes": list(ev.frechet_modes)},
           lambda ev: ev.frechet_per_class, "frechet_samplers", lambda: dict(frechet_real=None, frechet_cache={}), 1),
    Family("classifier", lambda ev: getattr(ev, "classifier_per_class", 0), lambda on: metrics.CLS_NAMES if on else (),
           lambda ev: {"per_class": ev.classifier_per_class, "diversity_pairs": ev.diversity_pairs,
                       "multimodality_pairs": ev.multimodality_pairs},
           lambda ev: ev.classifier_per_class, "cls_samplers", lambda: dict(classifier_real=None), 1),
    Family("memorisation", lambda ev: getattr(ev, "memorisation", None), lambda on: metrics.MEMORISATION_NAMES if on else (),
           lambda ev: {"mode": ev.memorisation, "per_class": ev.memorisation_per_class},
           lambda ev: ev.memorisation_per_class if ev.memorisation == "raw" else 0,      # (feature space: the classifier's matrices)
           "mem_samplers", lambda: dict(memorisation_real=None), 1),
    Family("kinematics", lambda ev: getattr(ev, "kinematics_per_class", 0), lambda on: metrics.KIN_NAMES if on else (),
           _kinematics_state, lambda ev: ev.kinematics_per_class, "kin_samplers", lambda: dict(kinematics_real=None), 2),
)


def round_owners(counts) -> dict:
    """The sharing rule.  ``counts``: {family: samples per class of its round; 0: it draws none}, in the record's order.
    Returns {family: the family whose round it reads, or None: it owns its Samplers (or draws no round)} - the owner is the
    first family in the order with the same non-zero count, so an owner is never itself a reader."""
    first, owners = {}, {}
    for key, n in counts.items():
        owner = first.setdefault(int(n), key) if n else key
        owners[key] = None if owner == key else owner
    return owners


def plain_state(v):
    """A state value as ``check_compatible`` compares it, whether it comes from ``state_dict()`` or back from a file: numpy and
    Python integers as int, floats as float, tuples, lists and arrays as lists, dicts as dicts; str (and None) as they are"""
    if isinstance(v, dict):
        return {k: plain_state(x) for k, x in v.items()}
    if isinstance(v, (tuple, list, np.ndarray)):
        return [plain_state(x) for x in v]
    if isinstance(v, (bool, np.bool_, int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    return v


class Evaluator:
    """``generators``: {name: Generator} (one or more); the real side: a ``Feeder`` (``metrics.select_reference_samples``
    with ``per_class=pairs``, cropped to the generator's ``t_size``), or ``real`` (N, C, T, V) with class ids
    ``real_labels`` (N,) - the first ``pairs`` samples of every class in index order.  Score names are
    ``"<generator>/<mode>"``; ``select`` names the one that decides (default: ``default_select``).  ``iteration``: a
    one-element int64 device tensor read when an evaluation runs (``TrainLoop.step_dev``), None records -1.
    ``prdc_per_class`` (0: off): also score precision / recall / density / coverage with ``prdc_k`` neighbours on that many
    fake and real samples per class (``"<generator>/precision"`` ...; ``select`` may name one of them: larger is better).
    ``frechet_per_class`` (0: off): also score the Frechet distance of the ``frechet_modes`` (``"pose"``, ``"motion"``) on
    that many fake and real samples per class (``"<generator>/pose_fd"``, ``"<generator>/motion_fd"``; smaller is better).
    ``classifier`` (a trained ``classifier.Classifier``; None or ``classifier_per_class`` 0: off): also score accuracy, feature
    Frechet distance, diversity (``diversity_pairs`` pairs) and multimodality (``multimodality_pairs`` pairs per class) on that
    many fake and real samples per class, features computed in chunks of ``classifier_batch``; ``classifier_real`` then holds
    the real set's own values.  The Evaluator never writes to the classifier and never changes its mode.
    ``memorisation`` (None: off; ``"features"``: in the classifier's feature space, which needs ``classifier`` and
    ``classifier_per_class`` and scores that round; ``"raw"``: on ``memorisation_per_class`` samples per class): also score
    authenticity and label agreement against the training set ``memorisation_train`` - a ``train.ResidentDataset`` (raw space
    searches it in place through its (scale, shift)) or (N, C, T, V) samples with ``memorisation_train_labels``.  ``memorisation_real`` holds the two scores of the selected
    real samples as queries: what a perfect generator scores - but only when ``real`` is held out from the training set
    (real samples that ARE training samples lie at distance 0 from themselves and score authenticity 0).  The Evaluator never
    writes to the training set.  ``memorisation_method`` (``"exact"``, ``"gram"``): with ``"gram"`` every search - the one-off
    leave-one-out pass included - runs through kg_nn_gram, the matrix-core pre-filter with exact re-score: the
    same bits in every column; the six launches are part of the captured evaluation, and ``memorisation_stats`` holds the (sets, 1, 2) certified / fallback row counts of the last call.
    ``kinematics_per_class`` (0: off): also score the six kinematic W1 distances of ``metrics.kinematics`` on that many fake
    and real samples per class, on the skeleton of ``kinematics_dataset`` (``"ntu"`` or ``"h36m"``) or the caller's
    ``kinematics_bones`` (B, 2) joint pairs and ``kinematics_mirror`` (M, 2) pairs of bone indices; ``kinematics_still_eps``
    is the threshold of the ``still`` descriptor.  ``kinematics_real`` then holds the real side's descriptor means (by
    ``metrics.KIN_NAMES``), ``"class_means"`` (K, 6) and its ``"degenerate"`` / ``"nonfinite"`` sample counts.
    Which family draws a round and which reads another's (``round_owner``; the ``*_samplers`` of a reader are empty), and that
    the real side is derived once here and is no part of the state: the module docstring, stated there once."""

    def __init__(self, generators: Dict[str, torch.nn.Module], real, real_labels=None, pairs: int = 10,
                 modes: Sequence[str] = ("avg", "joint"), select: Optional[str] = None, seed: int = 0,
                 trunc: Optional[float] = None, trunc_mode: str = "-", iteration: Optional[torch.Tensor] = None,
                 ring_len: int = 1024, use_graph: bool = True, t_size: Optional[int] = None, prdc_per_class: int = 0,
                 prdc_k: int = 5, frechet_per_class: int = 0, frechet_modes: Sequence[str] = ("pose", "motion"),
                 classifier=None, classifier_per_class: int = 0, classifier_batch: int = 512, diversity_pairs: int = 200,
                 multimodality_pairs: int = 20, memorisation: Optional[str] = None, memorisation_train=None,
                 memorisation_train_labels=None, memorisation_per_class: int = 0, memorisation_method: str = "exact", *,
                 kinematics_per_class: int = 0, kinematics_dataset: Optional[str] = None, kinematics_bones=None,
                 kinematics_mirror=None, kinematics_still_eps: float = 1e-3):
        if not generators:
            raise ValueError("Evaluator: at least one generator")
        self._check_classifier_options(classifier, classifier_per_class, classifier_batch, diversity_pairs, multimodality_pairs)
        self._check_memorisation_options(memorisation, memorisation_train, memorisation_per_class)
        self.memorisation_method = str(memorisation_method)
        self._mem_gram = metrics._nn_method(memorisation_method, "Evaluator")
        self.memorisation_stats = None
        self._check_frechet_options(frechet_per_class, frechet_modes)
        self._check_prdc_options(prdc_per_class, prdc_k)
        self._check_kinematics_options(kinematics_per_class, kinematics_dataset, kinematics_bones, kinematics_mirror,
                                       kinematics_still_eps)
        self.modes = tuple(modes)
        for m in self.modes:
            metrics._check_mode(m)
        if not self.modes:
            raise ValueError("Evaluator: at least one mode")
        self.gens = dict(generators)
        self.names = score_names(list(self.gens), self.modes, **{f.key: f.on(self) for f in FAMILIES})
        # (the entry point by its name: looked up in _native at every call)
        self._record, most = RECORDS[max([f.record for f in FAMILIES if f.on(self)], default=0)]
        most = getattr(nv, most)
        if len(self.names) > most:
            raise ValueError("Evaluator: %d scores, at most %d fit one record" % (len(self.names), most))
        self.select = default_select(list(self.gens), self.modes) if select is None else str(select)
        if self.select not in self.names:
            raise ValueError("Evaluator: select %r is none of %s" % (self.select, self.names))
        self._select = self.names.index(self.select)
        self.maximise = score_sense(self.select) == "max"
        self._worst = float("-inf") if self.maximise else float("inf")
        self.pairs, self.seed, self.ring_len = int(pairs), int(seed), int(ring_len)
        if self.pairs < 1 or self.ring_len < 1:
            raise ValueError("Evaluator: pairs and ring_len must be >= 1")
        first = next(iter(self.gens.values()))
        self.device = dev = next(first.parameters()).device
        self.use_graph = bool(use_graph) and dev.type == "cuda"
        self.iteration = iteration
        # every generator behind its own Sampler; this class runs their launch sequences inside its own capture
        self.samplers = {k: Sampler(G, qtd=self.pairs, seed=self.seed, trunc=trunc, trunc_mode=trunc_mode, use_graph=False)
                         for k, G in self.gens.items()}
        s0 = next(iter(self.samplers.values()))
        self.n_classes, self.n = s0.n_classes, s0.n
        if any(s.n_classes != self.n_classes for s in self.samplers.values()):
            raise ValueError("Evaluator: the generators differ in their number of classes")
        t_size = int(t_size) if t_size is not None else int(first.t_size)
        # the round pool: Samplers for the owners of a round only (round_owners); the MMD Samplers above stay outside it
        counts = {f.key: f.count(self) for f in FAMILIES}
        self.round_owner = round_owners(counts)
        self._pool = {}
        for f in FAMILIES:
            owns = counts[f.key] and self.round_owner[f.key] is None
            self._pool[f.key] = {k: Sampler(G, qtd=counts[f.key], seed=self.seed, trunc=trunc, trunc_mode=trunc_mode, use_graph=False)
                                 for k, G in self.gens.items()} if owns else {}
            setattr(self, f.samplers, self._pool[f.key])
        # the families' real side, once per count: (K*P, C, t, V) class by class on the device; nothing writes to it
        self._real_sides = {}

        def real_side(per_class):                # (called by the set-ups, after the checks that need no samples)
            if per_class not in self._real_sides:
                self._real_sides[per_class] = torch.as_tensor(self._select_real(real, real_labels, per_class, "classes", t_size)).to(dev)
            return self._real_sides[per_class]

        extra = {"memorisation": (memorisation_train, memorisation_train_labels)}
        for f in FAMILIES:
            if f.on(self):
                getattr(self, "_%s_setup" % f.key)(real_side, *extra.get(f.key, ()))
            else:
                for k, v in f.off().items():
                    setattr(self, k, v)
        # the real side, once: row j*K + c = the j-th selected real sample of class c (the Sampler's label order)
        self.real = torch.as_tensor(self._select_real(real, real_labels, self.pairs, "pairs", t_size)).to(dev)
        self._pair_labels = np.arange(self.n)                  # every (fake, real) pair is a "class" of the kg_mmd call
        self._nchw = None
        if "joint" in self.modes and self.real.shape[1] > 1 and self.real.shape[2] > 1:
            self._nchw = {k: torch.zeros(self.real.shape, dtype=torch.float32, device=dev) for k in self.gens}
        # the record
        n = len(self.names)
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.ring_val = torch.full((self.ring_len, n), float("nan"), dtype=torch.float32, device=dev)
        self.ring_iter = torch.full((self.ring_len, 2), -1, dtype=torch.int64, device=dev)
        self.best_val = torch.full((1,), self._worst, dtype=torch.float32, device=dev)
        self.best_iter = torch.full((1,), -1, dtype=torch.int64, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.n_evals = 0                     # host mirror of count
        self._flushed = 0
        self._hist = []                      # (iteration (k,), scores (k, n), improved (k,)) blocks already read
        # the snapshot of the selected generator: its flat parameters + one tensor per module buffer
        G = self.gens[self.select.split("/")[0]]
        params = [p.detach() for p in G.parameters()]
        flat, offs = _flat_storage(params)
        if flat is not None:
            self.snap_flat = torch.zeros_like(flat)
            self._jobs = [(flat, self.snap_flat)]
        else:                                # per-tensor storage: packed, one job per parameter
            offs = list(np.cumsum([0] + [p.numel() for p in params[:-1]]))
            self.snap_flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=dev)
            self._jobs = [(p.contiguous().view(-1), self.snap_flat[o:o + p.numel()]) for p, o in zip(params, offs)]
        self._snap_offsets = [int(o) for o in offs]
        self._G_sel = G
        self.snap_buffers = {k: torch.zeros_like(b) for k, b in G.named_buffers()}
        self._jobs += [(b.detach(), self.snap_buffers[k]) for k, b in G.named_buffers()]
        self._best_G = None
        self._scores = None
        self._graph = None

    def _check_frechet_options(self, frechet_per_class, frechet_modes):
        self.frechet_per_class = int(frechet_per_class)
        if self.frechet_per_class < 0:
            raise ValueError("Evaluator: frechet_per_class=%d < 0" % self.frechet_per_class)
        # (the modes in the order of metrics.FRECHET_MODES, whatever order they were asked for in)
        self.frechet_modes = tuple(f for f in metrics.FRECHET_MODES if f in tuple(frechet_modes)) if self.frechet_per_class else ()
        if self.frechet_per_class and (not self.frechet_modes or set(frechet_modes) - set(metrics.FRECHET_MODES)):
            raise ValueError("Evaluator: frechet_modes %r: one or more of %s" % (tuple(frechet_modes), metrics.FRECHET_MODES))

    def _check_classifier_options(self, classifier, per_class, batch, diversity_pairs, multimodality_pairs):
        self.classifier_per_class = int(per_class) if classifier is not None else 0
        if int(per_class) < 0:
            raise ValueError("Evaluator: classifier_per_class=%d < 0" % int(per_class))
        self.classifier = classifier if self.classifier_per_class else None
        self.classifier_batch = int(batch)
        self.diversity_pairs, self.multimodality_pairs = int(diversity_pairs), int(multimodality_pairs)
        if self.classifier_per_class and (self.classifier_batch < 1 or self.diversity_pairs < 1 or self.multimodality_pairs < 1):
            raise ValueError("Evaluator: classifier_batch=%d, diversity_pairs=%d, multimodality_pairs=%d must be >= 1" % (
                self.classifier_batch, self.diversity_pairs, self.multimodality_pairs))

    def _check_memorisation_options(self, mode, train, per_class):
        """(after the classifier's options) ``memorisation_per_class`` becomes the number of samples per class that are scored"""
        self.memorisation = None if mode is None else str(mode)
        self.memorisation_per_class = int(per_class)
        if self.memorisation is None:
            return
        if self.memorisation not in MEMORISATION_MODES:
            raise ValueError("Evaluator: memorisation=%r is none of %s" % (mode, MEMORISATION_MODES))
        if train is None:
            raise ValueError("Evaluator: memorisation=%r needs the training set (memorisation_train)" % self.memorisation)
        if self.memorisation == "features":
            if not self.classifier_per_class:
                raise ValueError("Evaluator: memorisation='features' scores the classifier round's features: it needs "
                                 "classifier= and classifier_per_class > 0")
            if self.memorisation_per_class:
                raise ValueError("Evaluator: memorisation='features' scores the classifier round (classifier_per_class=%d "
                                 "samples per class); memorisation_per_class=%d is for memorisation='raw'" % (
                                     self.classifier_per_class, self.memorisation_per_class))
            self.memorisation_per_class = self.classifier_per_class
        elif self.memorisation_per_class < 1:
            raise ValueError("Evaluator: memorisation='raw' needs memorisation_per_class >= 1, got %d" % self.memorisation_per_class)

    def _check_kinematics_options(self, per_class, dataset, bones, mirror, still_eps):
        """the skeleton tables (``metrics._kin_tables``); the limits that need the samples' shape follow in the set-up"""
        self.kinematics_per_class = int(per_class)
        self.kinematics_still_eps = float(still_eps)
        self.kinematics_bones, self.kinematics_mirror = None, None
        if self.kinematics_per_class < 0:
            raise ValueError("Evaluator: kinematics_per_class=%d < 0" % self.kinematics_per_class)
        if not self.kinematics_per_class:
            return
        if dataset is None and bones is None:
            raise ValueError("Evaluator: kinematics_per_class=%d needs the skeleton: kinematics_dataset ('ntu' or 'h36m') or "
                             "kinematics_bones" % self.kinematics_per_class)
        if 2 * self.kinematics_per_class > nv.KIN_MAX_POINTS:
            raise ValueError("Evaluator: kinematics_per_class=%d: real + generated = %d values per class, above the cap of %d" % (
                self.kinematics_per_class, 2 * self.kinematics_per_class, nv.KIN_MAX_POINTS))
        self.kinematics_bones, self.kinematics_mirror = metrics._kin_tables(dataset, bones, mirror, "Evaluator: kinematics_dataset")

    def _check_prdc_options(self, prdc_per_class, prdc_k):
        self.prdc_per_class, self.prdc_k = int(prdc_per_class), int(prdc_k)
        if self.prdc_per_class < 0:
            raise ValueError("Evaluator: prdc_per_class=%d < 0" % self.prdc_per_class)
        if self.prdc_per_class and not 1 <= self.prdc_k <= min(nv.PRDC_MAX_K, self.prdc_per_class - 1):
            raise ValueError("Evaluator: prdc_k=%d outside [1, min(%d, prdc_per_class=%d - 1)]" % (
                self.prdc_k, nv.PRDC_MAX_K, self.prdc_per_class))
        if self.prdc_per_class > nv.PRDC_MAX_POINTS:
            raise ValueError("Evaluator: prdc_per_class=%d above the cap of %d points per class" % (
                self.prdc_per_class, nv.PRDC_MAX_POINTS))

    def _select_real(self, real, real_labels, per_class, order, t_size) -> np.ndarray:
        """The first ``per_class`` real samples of every class as one contiguous fp32 host array (n_classes * per_class, C,
        t, V): from a ``Feeder`` (``metrics.select_reference_samples``, cropped to ``t_size``) or from ``real`` with
        ``real_labels``.  ``order="pairs"``: the Sampler's row order (``pair_rows``); ``"classes"``: class by class
        (``class_rows``; a Feeder's selection is in that order already, so it is left as it is)."""
        K = self.n_classes
        if real_labels is None and hasattr(real, "label") and hasattr(real, "data"):
            data, lab, _ = metrics.select_reference_samples(real, np.arange(K), t_size, per_class=per_class)
        else:
            data = real.detach().cpu().numpy() if isinstance(real, torch.Tensor) else np.asarray(real)
            lab = real_labels.detach().cpu().numpy() if isinstance(real_labels, torch.Tensor) else np.asarray(real_labels)
        rows = (pair_rows if order == "pairs" else class_rows)(lab, K, per_class)
        return np.ascontiguousarray(np.asarray(data, dtype=np.float32)[rows])

    def _rounds(self, key):
        """This evaluation's round of every generator for the family ``key``: run here when the family owns it, else the one
        its owner ran earlier in this evaluation (``round_owners``).  Each is (P*K, C, T, V) with row j*K + c = sample j of
        class c and read in place - so it has to have the real side's sample shape, be a plane, and all of them the same
        strides.  Returns (outs, sn, sc)."""
        owner = self.round_owner[key]
        real_shape = self._real_sides[getattr(self, key + "_per_class")].shape
        outs = []
        for s in self._pool[owner or key].values():
            if owner is None:
                s._round()
            out = s._out
            if tuple(out.shape[1:]) != tuple(real_shape[1:]) or not nv.is_plane(out):
                raise ValueError("Evaluator: generated samples %s against real samples %s" % (
                    tuple(out.shape[1:]), tuple(real_shape[1:])))
            outs.append(out)
        sn, sc = nv._sn_sc(outs[0])
        if any(nv._sn_sc(q) != (sn, sc) for q in outs):
            raise ValueError("Evaluator: the generators' rounds differ in their strides")
        return outs, sn, sc

    # ---- precision / recall / density / coverage -----------------------------------------------------------
    def _prdc_setup(self, real_side):
        """the real samples' radii (one kg_prdc_radii launch) and the workspace"""
        dev, K, P = self.device, self.n_classes, self.prdc_per_class
        self.prdc_real = real_side(P)
        self._prdc_D = int(np.prod(self.prdc_real.shape[1:]))
        self._prdc_rv = nv.PrdcView(self.prdc_real, P * self._prdc_D, self._prdc_D, 0)
        with torch.cuda.device(dev):
            self.prdc_radii = nv.prdc_radii(self._prdc_rv, P, 1, self._prdc_D, K, self.prdc_k)
            sets = min(len(self.gens), nv.PRDC_MAX_SETS)
            nbytes = nv.prdc_sets_workspace_bytes(sets, P, P, 1, self._prdc_D, K, self.prdc_k)
            self._prdc_ws = torch.empty(max(1, nbytes // 4), dtype=torch.int32, device=dev)

    def _prdc_scores(self):
        """the PRDC rounds of all generators, then ONE kg_prdc_sets per PRDC_MAX_SETS generators: the (nsets, 4) class means,
        whose elements are the scores"""
        K, P = self.n_classes, self.prdc_per_class
        outs, sn, sc = self._rounds("prdc")
        _, C, T, V = outs[0].shape
        d_outer, d_inner, so = (1, C * T * V, 0) if C == 1 else (C, T * V, sc)
        rv = self._prdc_rv if d_outer == 1 else self._prdc_rv._replace(so=T * V)
        scores = []
        for part in nv._chunks(outs, nv.PRDC_MAX_SETS):
            res = nv.prdc_sets(rv, part, sn, K * sn, so, self.prdc_radii, P, P, d_outer, d_inner, K, self.prdc_k,
                               want_mean=True, ws=self._prdc_ws)
            scores += [res["mean"][g, i:i + 1] for g in range(len(part)) for i in range(4)]
        return scores

    # ---- Frechet pose / motion distance --------------------------------------------------------------------
    def _frechet_setup(self, real_side):
        """the checks; per mode the real side's cache (one kg_frechet_real call) and the workspace"""
        dev, K, P = self.device, self.n_classes, self.frechet_per_class
        self.frechet_real = real_side(P)
        _, C, T, V = self.frechet_real.shape
        if C * V > nv.FRECHET_MAX_DIM:
            raise ValueError("Evaluator: frechet needs d = C*V = %d <= %d" % (C * V, nv.FRECHET_MAX_DIM))
        if "motion" in self.frechet_modes and T < 2:
            raise ValueError("Evaluator: frechet mode 'motion' needs two frames, the samples have %d" % T)
        D = C * T * V
        rv = nv.FrechetView(self.frechet_real, P * D, D, V, T * V if C > 1 else 0)
        with torch.cuda.device(dev):
            self.frechet_cache = {f: nv.frechet_real(rv, P, T, f == "motion", C, V, K) for f in self.frechet_modes}
            sets = min(len(self.gens), nv.FRECHET_MAX_SETS)
            nbytes = max(nv.frechet_sets_workspace_bytes(sets, P, T, f == "motion", C, V, K) for f in self.frechet_modes)
            self._frechet_ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)

    def _frechet_scores(self):
        """the Frechet rounds of all generators, then per mode ONE kg_frechet_sets per FRECHET_MAX_SETS generators: the mean32
        words, which are the scores - generator by generator, mode by mode"""
        K, P = self.n_classes, self.frechet_per_class
        outs, sn, sc = self._rounds("frechet")
        _, C, T, V = outs[0].shape
        so = sc if C > 1 else 0
        per_mode = {}
        for f in self.frechet_modes:
            words = []
            for part in nv._chunks(outs, nv.FRECHET_MAX_SETS):
                res = nv.frechet_sets(self.frechet_cache[f], part, sn, K * sn, V, so, P, T, f == "motion", C, V, K,
                                      ws=self._frechet_ws)
                words += [res["mean32"][g:g + 1] for g in range(len(part))]
            per_mode[f] = words
        return [per_mode[f][g] for g in range(len(outs)) for f in self.frechet_modes]

    # ---- accuracy / feature FD / diversity / multimodality of a trained classifier ------------------------
    def _classifier_features(self, x, feat, pred):
        """the rows of x (n, C, T, V) through the classifier's trunk and head in chunks of ``classifier_batch``: plane slices
        read in place, features and predictions written into their rows of feat (n, F) / pred (n,); no autograd, no tape"""
        clf = self.classifier
        w = [p.detach() for p in (clf.fc1.weight, clf.fc1.bias, clf.fcn.weight, clf.fcn.bias)]
        with torch.no_grad():
            for lo in range(0, x.shape[0], self.classifier_batch):
                hi = min(x.shape[0], lo + self.classifier_batch)
                nv.cls_head_fwd(clf._trunk(x[lo:hi]), *w, None, feat_out=feat[lo:hi], pred_out=pred[lo:hi])

    def _classifier_setup(self, real_side):
        """the checks; the real samples' features as ONE set through kg_frechet_real (the unconditional feature FD of
        ``metrics.classifier_scores``) and their own accuracy / diversity / multimodality (``classifier_real``); the
        generators' pair tables from the Sampler's label vector and static feature / prediction buffers"""
        clf, dev, K, P = self.classifier, self.device, self.n_classes, self.classifier_per_class
        F = int(clf.feat_dim)
        if int(clf.n_classes) != K:
            raise ValueError("Evaluator: the classifier has %d classes, the generators %d" % (int(clf.n_classes), K))
        if next(clf.parameters()).device != dev:
            raise ValueError("Evaluator: the classifier is on %s, the generators on %s" % (next(clf.parameters()).device, dev))
        if not 1 <= F <= nv.FRECHET_MAX_DIM:
            raise ValueError("Evaluator: the classifier's feat_dim=%d outside [1, %d]" % (F, nv.FRECHET_MAX_DIM))
        if self.diversity_pairs > K * P or self.multimodality_pairs > P:
            raise ValueError("Evaluator: diversity_pairs=%d above K*P=%d or multimodality_pairs=%d above P=%d" % (
                self.diversity_pairs, K * P, self.multimodality_pairs, P))
        real_x = real_side(P)
        _, C, T, V = real_x.shape
        c_in = int(clf.st_gcn_networks[0].in_channels)
        if c_in != C or int(clf.t_size) != T:
            raise ValueError("Evaluator: the classifier takes (%d channels, %d frames), the samples have (%d, %d)" % (
                c_in, int(clf.t_size), C, T))
        n = K * P
        lab_gen = np.tile(np.arange(K), P)               # the Sampler's label vector: row j*K + c has class c
        lab_real = np.repeat(np.arange(K), P)
        self._cls_labels = torch.as_tensor(lab_gen, dtype=torch.int64).to(dev)
        self._cls_tables = tuple(torch.as_tensor(t).to(dev) for t in metrics.cls_pair_tables(
            lab_gen, K, self.diversity_pairs, self.multimodality_pairs, self.seed))
        self._cls_feat = {k: torch.zeros((n, F), dtype=torch.float32, device=dev) for k in self.gens}
        self._cls_pred = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in self.gens}
        with torch.cuda.device(dev):
            feat_r = torch.zeros((n, F), dtype=torch.float32, device=dev)
            pred_r = torch.zeros(n, dtype=torch.int32, device=dev)
            self._classifier_features(real_x, feat_r, pred_r)
            self._cls_cache = nv.frechet_real(nv.FrechetView(feat_r, 0, F, 0, 0), n, 1, False, 1, F, 1)
            tabs = [torch.as_tensor(t).to(dev) for t in metrics.cls_pair_tables(
                lab_real, K, self.diversity_pairs, self.multimodality_pairs, self.seed)]
            res = nv.cls_scores([feat_r], [pred_r], torch.as_tensor(lab_real, dtype=torch.int64).to(dev), *tabs, K)
            self.classifier_real = {"accuracy": res["scores64"][0, 0], "diversity": res["scores64"][0, 1],
                                    "multimodality": res["scores64"][0, 2], "correct_per_class": res["correct_per_class"][0],
                                    "features": feat_r}
            sets = min(len(self.gens), nv.FRECHET_MAX_SETS)
            self._cls_ws = torch.empty(nv.frechet_sets_workspace_bytes(sets, n, 1, False, 1, F, 1) // 8, dtype=torch.float64,
                                       device=dev)

    def _classifier_scores(self):
        """the classifier rounds of all generators, their features; then per group of generators ONE kg_frechet_sets and ONE
        kg_cls_scores: the score words are one-element views of mean32 and scores - per generator in the order of
        metrics.CLS_NAMES"""
        K, P = self.n_classes, self.classifier_per_class
        n, F = K * P, int(self.classifier.feat_dim)
        outs, _, _ = self._rounds("classifier")
        keys = list(self.gens)
        for k, out in zip(keys, outs):
            self._classifier_features(out, self._cls_feat[k], self._cls_pred[k])
        words = []
        for part in nv._chunks(keys, min(nv.FRECHET_MAX_SETS, nv.CLS_MAX_SETS)):
            feats = [self._cls_feat[k] for k in part]
            preds = [self._cls_pred[k] for k in part]
            fd = nv.frechet_sets(self._cls_cache, feats, 0, F, 0, 0, n, 1, False, 1, F, 1, ws=self._cls_ws)
            sc = nv.cls_scores(feats, preds, self._cls_labels, *self._cls_tables, K)
            for g in range(len(feats)):
                words += [sc["scores"][g, 0:1], fd["mean32"][g:g + 1], sc["scores"][g, 1:2], sc["scores"][g, 2:3]]
        return words

    # ---- authenticity / label agreement against the training set -------------------------------------------
    def _memorisation_setup(self, real_side, train, train_labels):
        """the checks; the training side: its int32 labels, in feature space its features (through the classifier in chunks of
        ``classifier_batch``, a ResidentDataset normalised chunk by chunk with the arithmetic of its gather), the train -> train
        leave-one-out distances (one kg_nn with exclude_self) and the real side's own two scores (``memorisation_real``); the
        workspace"""
        who = "Evaluator"
        dev, K, P = self.device, self.n_classes, self.memorisation_per_class
        t, ta, own = metrics._nn_side(train, who, "memorisation_train")
        if train_labels is None:
            train_labels = own
        if train_labels is None:
            raise ValueError("Evaluator: memorisation_train_labels is needed (the training set carries none)")
        if t.dim() != 4:
            raise ValueError("Evaluator: memorisation_train holds (N, C, T, V) samples, got %s" % (tuple(t.shape),))
        N = int(t.shape[0])
        if N > nv.NN_MAX_POINTS:
            raise ValueError("Evaluator: %d training samples, kg_nn takes at most %d" % (N, nv.NN_MAX_POINTS))
        if N < 2:
            raise ValueError("Evaluator: the leave-one-out pass needs at least 2 training samples, got %d" % N)
        if K > nv.NN_SCORES_MAX_CLASSES:
            raise ValueError("Evaluator: %d classes, kg_nn_scores takes at most %d" % (K, nv.NN_SCORES_MAX_CLASSES))
        lab_t = metrics._label_ids(train_labels, N, "memorisation_train_labels", who)[0]
        real_x = real_side(P)
        if tuple(t.shape[1:]) != tuple(real_x.shape[1:]):
            raise ValueError("Evaluator: the training samples are (channels, frames, joints) = %s, the generators' %s" % (
                tuple(t.shape[1:]), tuple(real_x.shape[1:])))
        if t.device != dev:
            t = t.to(dev)
        t = t.contiguous()                      # (a ResidentDataset's array is: nothing is copied)
        _, C, T, V = real_x.shape
        n = K * P
        self._mem_train, self._mem_N = t, N
        lab_real = np.repeat(np.arange(K), P)
        self._mem_qlab = torch.as_tensor(np.tile(np.arange(K), P).astype(np.int32)).to(dev)    # the Sampler's label vector
        self._mem_blab = torch.as_tensor(lab_t.astype(np.int32)).to(dev)
        with torch.cuda.device(dev):
            if self.memorisation == "features":
                F = int(self.classifier.feat_dim)
                feat = torch.zeros((N, F), dtype=torch.float32, device=dev)
                pred = torch.zeros(N, dtype=torch.int32, device=dev)
                for lo in range(0, N, self.classifier_batch):
                    x = t[lo:lo + self.classifier_batch]
                    if ta is not None:          # (x * scale) + shift in two roundings: the normalised sample's bits
                        x = x * ta[0] + ta[1]
                    self._classifier_features(x, feat[lo:lo + self.classifier_batch], pred[lo:lo + self.classifier_batch])
                self.memorisation_train_features = feat
                self._mem_dims, self._mem_q = (1, F), (0, F, 0)
                self._mem_bv, self._mem_ba = nv.PrdcView(feat, 0, F, 0), None
                real_q, train_q = self.classifier_real["features"], feat
            else:
                D = C * T * V
                self._mem_dims = (1, D) if C == 1 else (C, T * V)
                self._mem_q = None              # (the rounds' strides, read when they exist)
                self._mem_bv, self._mem_ba = nv.PrdcView(t, 0, D, 0 if C == 1 else T * V), ta
                real_q, train_q = real_x, (train if ta is not None else t)     # (a ResidentDataset: through its affine)
            d_outer, d_inner = self._mem_dims
            bv = self._mem_bv
            if self._mem_gram:                  # the training side's norms, once; the one-off pass through the pre-filter too
                self._mem_norms = nv.nn_norms(bv, N, d_outer, d_inner, 1, self._mem_ba)
                self._mem_loo = nv.nn_gram([bv.t], bv.sc, bv.sp, bv.so, bv, N, N, d_outer, d_inner, 1, 1, exclude_self=True,
                                           q_affine=self._mem_ba, b_affine=self._mem_ba,
                                           base_norms=self._mem_norms)[1].reshape(-1)
            else:
                self._mem_loo = nv.nn(bv, bv, N, N, d_outer, d_inner, 1, 1, exclude_self=True, q_affine=self._mem_ba,
                                      b_affine=self._mem_ba)[1].reshape(-1)
            res = metrics.memorisation_sets([real_q], lab_real, train_q, lab_t, train_loo=self._mem_loo,
                                            method=self.memorisation_method)
            self.memorisation_real = {"authenticity": res["authenticity"][0], "label_agreement": res["label_agreement"][0],
                                      "counts": res["counts"][0]}
            sizes = {min(nv.NN_MAX_SETS, len(self.gens) - q) for q in range(0, len(self.gens), nv.NN_MAX_SETS)}
            ws_bytes = nv.nn_gram_workspace_bytes if self._mem_gram else nv.nn_sets_workspace_bytes
            nbytes = max(ws_bytes(g, n, N, d_outer, d_inner, 1, 1) for g in sizes)
            self._mem_ws = torch.empty(max(1, nbytes // 4), dtype=torch.int32, device=dev)

    def _memorisation_scores(self):
        """the query sets of all generators - the classifier round's feature matrices, or the raw rounds read in place -, then
        per group of generators ONE kg_nn_sets (k = 1) and ONE kg_nn_scores: the score words are one-element views of scores,
        per generator in the order of metrics.MEMORISATION_NAMES"""
        K, P, N = self.n_classes, self.memorisation_per_class, self._mem_N
        d_outer, d_inner = self._mem_dims
        if self.memorisation == "features":
            qs, (q_sc, q_sp, q_so) = [self._cls_feat[k] for k in self.gens], self._mem_q
        else:
            qs, sn, sc = self._rounds("memorisation")
            q_sc, q_sp, q_so = 0, sn, (0 if d_outer == 1 else sc)
        words = []
        for part in nv._chunks(qs, nv.NN_MAX_SETS):
            if self._mem_gram:
                idx, d2, self.memorisation_stats = nv.nn_gram(part, q_sc, q_sp, q_so, self._mem_bv, K * P, N, d_outer, d_inner, 1,
                                                              1, b_affine=self._mem_ba, base_norms=self._mem_norms,
                                                              ws=self._mem_ws)
            else:
                idx, d2 = nv.nn_sets(part, q_sc, q_sp, q_so, self._mem_bv, K * P, N, d_outer, d_inner, 1, 1,
                                     b_affine=self._mem_ba, ws=self._mem_ws)
            sc_ = nv.nn_scores(idx, d2, self._mem_qlab, self._mem_blab, self._mem_loo, K)
            for g in range(len(part)):
                words += [sc_["scores"][g, 0:1], sc_["scores"][g, 1:2]]
        return words

    # ---- kinematic plausibility: W1 of six descriptors against the real set --------------------------------
    def _kinematics_setup(self, real_side):
        """the checks (``metrics._kin_check``); the real samples' descriptors (one kg_kin_desc launch) with their own means and
        counts (``kinematics_real``); the static descriptor matrices and the workspace"""
        dev, K, P = self.device, self.n_classes, self.kinematics_per_class
        bones, mirror, eps = self.kinematics_bones, self.kinematics_mirror, self.kinematics_still_eps
        real_x = real_side(P)
        metrics._kin_check(real_x, "real", bones, mirror, eps, "Evaluator: kinematics")
        if K * P >= 1 << 24:
            raise ValueError("Evaluator: kinematics_per_class=%d: %d samples, kg_kin_desc takes fewer than 2^24" % (P, K * P))
        _, C, T, V = real_x.shape
        D = C * T * V
        with torch.cuda.device(dev):
            desc, degenerate = nv.kin_desc(nv.FrechetView(real_x, P * D, D, V, T * V), P, T, C, V, K, bones, mirror, eps)
            self._kin_real_desc = desc
            finite = torch.isfinite(desc).all(dim=2)                        # (K, P)
            means = desc.double().mean(dim=1)                               # (K, 6)
            self.kinematics_real = dict({q: means[:, i].mean() for i, q in enumerate(metrics.KIN_NAMES)}, class_means=means,
                                        degenerate=degenerate, nonfinite=(~finite).sum(dim=1).to(torch.int32))
            sets = min(len(self.gens), nv.KIN_MAX_SETS)
            self._kin_desc = torch.zeros((sets, K, P, nv.KIN_DESC), dtype=torch.float32, device=dev)
            nbytes = nv.kin_desc_sets_workspace_bytes(sets, P, T, C, V, K, bones, mirror, eps)
            self._kin_ws = torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)

    def _kinematics_scores(self):
        """the kinematic rounds of all generators, then per group of up to KIN_MAX_SETS generators ONE kg_kin_desc_sets - the
        rounds read in place through their shared strides: row j*K + c, so the class stride is a sample and the sample stride
        K samples - and ONE kg_kin_scores against the cached real descriptors: the score words are one-element views of
        scores (nsets, 6), per generator in the order of metrics.KIN_NAMES"""
        K, P = self.n_classes, self.kinematics_per_class
        outs, sn, sc = self._rounds("kinematics")
        _, C, T, V = outs[0].shape
        words = []
        for part in nv._chunks(outs, nv.KIN_MAX_SETS):
            desc, _ = nv.kin_desc_sets(
                part, sn, K * sn, V, sc, P, T, C, V, K, self.kinematics_bones, self.kinematics_mirror, self.kinematics_still_eps,
                out=self._kin_desc[:len(part)], ws=self._kin_ws)
            res = nv.kin_scores(self._kin_real_desc, [desc[g] for g in range(len(part))])
            words += [res["scores"][g, i:i + 1] for g in range(len(part)) for i in range(nv.KIN_DESC)]
        return words

    # ---- the launch sequence -------------------------------------------------------------------------------------------
    def _round(self):
        """what a graph holds: per generator a Sampler round, the re-layout, kg_mmd per mode; then the record, then the
        conditional snapshot"""
        scores = []
        for k, s in self.samplers.items():
            s._round()
            out = s._out
            if self._nchw is not None:
                self._nchw[k].copy_(out)
                out = self._nchw[k]
            for mode in self.modes:
                scores.append(metrics.calculate_mmd(out, self.real, self._pair_labels, mode).reshape(1))
        for f in FAMILIES:
            if f.on(self):
                scores += getattr(self, "_%s_scores" % f.key)()
        sense = {} if self._record == "eval_record" else {"maximise": self.maximise}
        getattr(nv, self._record)(scores, self._select, self.iteration, self.count, self.ring_val, self.ring_iter, self.best_val,
                                  self.best_iter, self.flag, **sense)
        nv.copy_if(self.flag, self._jobs)
        self._scores = scores                # (under capture: the graph's own memory, kept alive with it)

    def _state_tensors(self):
        ts = [s.step_dev for s in self._all_samplers()]
        ts += [self.count, self.ring_val, self.ring_iter, self.best_val, self.best_iter, self.flag, self.snap_flat]
        return ts + list(self.snap_buffers.values())

    def _all_samplers(self):
        return list(self.samplers.values()) + [s for group in self._pool.values() for s in group.values()]

    def _capture(self):
        """Single-stream capture, no parallel branches.  The warm-up rounds in front of it are real evaluations:
        everything they move is put back."""
        return capture_keeping(self._round, self._state_tensors(), self.device)

    @torch.no_grad()
    def evaluate(self) -> None:
        """One evaluation, enqueued on the current stream; no host synchronisation (a full record ring is read first)."""
        if self.n_evals - self._flushed >= self.ring_len:
            self._flush()
        if self.use_graph:
            if self._graph is None:
                self._graph = self._capture()
            self._graph.replay()
        else:
            self._round()
        for s in self._all_samplers():
            s.step_count += 1
        self.n_evals += 1

    # ---- reading ---------------------------------------------------------------------------------------------------------
    def _flush(self):
        k = self.n_evals - self._flushed
        if k <= 0:
            return
        raw = torch.cat([self.ring_val.view(torch.uint8).reshape(-1), self.ring_iter.view(torch.uint8).reshape(-1)]).cpu().numpy()
        nb = self.ring_val.numel() * 4       # ONE device -> host read
        val = raw[:nb].view(np.float32).reshape(self.ring_len, -1)
        it = raw[nb:].view(np.int64).reshape(self.ring_len, 2)
        slots = np.arange(self._flushed, self.n_evals) % self.ring_len
        self._hist.append((it[slots, 0].copy(), val[slots].copy(), it[slots, 1].astype(bool)))
        self._flushed = self.n_evals

    def records(self) -> dict:
        """Every evaluation since the record began, in evaluation order: dict(names, iteration (n,) int64, scores
        (n, nscores) fp32, improved (n,) bool).  Synchronises (one bulk read of what has not been read yet)."""
        self._flush()
        n = len(self.names)
        if not self._hist:
            return {"names": list(self.names), "iteration": np.zeros(0, np.int64), "scores": np.zeros((0, n), np.float32),
                    "improved": np.zeros(0, bool)}
        return {"names": list(self.names), "iteration": np.concatenate([h[0] for h in self._hist]),
                "scores": np.concatenate([h[1] for h in self._hist]), "improved": np.concatenate([h[2] for h in self._hist])}

    def best(self) -> dict:
        """{"value", "iteration"} of the best evaluation so far (+inf - or -inf when the deciding score is better when
        larger -, -1 before the first finite one).  Synchronises."""
        return {"value": float(self.best_val.item()), "iteration": int(self.best_iter.item())}

    def best_generator(self):
        """A ``Generator`` whose parameters and buffers are views into the snapshot (built once, in eval mode;
        ``state_dict()`` has the reference's keys in the reference's order).  It follows every later snapshot."""
        if self._best_G is not None:
            return self._best_G
        from .wgan_gp import rebuild_generator
        E = rebuild_generator(self._G_sel)
        for p, off in zip(E.parameters(), self._snap_offsets):
            p.data = self.snap_flat[off:off + p.numel()].view(p.shape)
            p.requires_grad_(False)
        names = iter(self.snap_buffers)
        for me in E.modules():
            for k in list(me._buffers):
                me._buffers[k] = self.snap_buffers[next(names)]
        assert [k for k, _ in E.named_buffers()] == list(self.snap_buffers)
        self._best_G = E
        return E

    # ---- resume ----------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        rec = self.records()
        s0 = next(iter(self.samplers.values()))
        sd = {"seed": self.seed, "step": s0.step_count, "pairs": self.pairs, "select": self.select, "modes": list(self.modes),
              "names": list(self.names), "count": self.n_evals, "ring_val": self.ring_val.cpu(), "ring_iter": self.ring_iter.cpu(),
              "best_val": self.best_val.cpu(), "best_iter": self.best_iter.cpu(),
              "snapshot": {"flat": self.snap_flat.cpu(), "buffers": {k: b.cpu() for k, b in self.snap_buffers.items()}},
              "records": {k: rec[k] for k in ("iteration", "scores", "improved")}}
        for f in FAMILIES:                   # (the options only: the real side is recomputed from the data)
            if f.on(self):
                sd[f.key] = f.state(self)
        return sd

    def check_compatible(self, sd: dict) -> None:
        # (called unbound on Evaluator-like objects of before a family existed: FAMILIES reads them with defaults)
        for f in FAMILIES:
            mine = plain_state(f.state(self)) if f.on(self) else None
            if plain_state(sd.get(f.key)) != mine:
                raise ValueError("Evaluator.load_state_dict: %s is %r in the state, %r here" % (f.key, sd.get(f.key), mine))
        for k, mine in (("pairs", self.pairs), ("select", self.select), ("modes", list(self.modes)), ("names", list(self.names))):
            if (list(sd[k]) if isinstance(mine, list) else sd[k]) != mine:
                raise ValueError("Evaluator.load_state_dict: %s is %r in the state, %r here" % (k, sd[k], mine))
        if tuple(sd["ring_val"].shape) != tuple(self.ring_val.shape) or tuple(sd["snapshot"]["flat"].shape) != tuple(self.snap_flat.shape) \
                or set(sd["snapshot"]["buffers"]) != set(self.snap_buffers):
            raise ValueError("Evaluator.load_state_dict: the record ring or the snapshot of the state has another shape")

    def load_state_dict(self, sd: dict) -> None:
        """Continues bit for bit: the same draws, the same record, the same best so far and its snapshot."""
        self.check_compatible(sd)
        for s in self._all_samplers():
            s.load_state_dict({"seed": sd["seed"], "step": sd["step"]})
        if int(sd["seed"]) != self.seed:
            self.seed, self._graph = int(sd["seed"]), None      # (the seed is a launch argument)
        self.n_evals = self._flushed = int(sd["count"])
        self.count.fill_(self.n_evals)
        self.ring_val.copy_(sd["ring_val"])
        self.ring_iter.copy_(sd["ring_iter"])
        self.best_val.copy_(sd["best_val"])
        self.best_iter.copy_(sd["best_iter"])
        self.flag.zero_()
        self.snap_flat.copy_(sd["snapshot"]["flat"])
        for k, b in self.snap_buffers.items():
            b.copy_(sd["snapshot"]["buffers"][k])
        r = sd["records"]
        self._hist = [(np.asarray(r["iteration"], np.int64).copy(), np.asarray(r["scores"], np.float32).copy(),
                       np.asarray(r["improved"], bool).copy())] if len(r["iteration"]) else []
        torch.cuda.synchronize(self.device)

    def reset(self) -> None:
        """A fresh record (``TrainLoop.load_state_dict`` of a state without one); the Sampler counters start again at 0."""
        warnings.warn("Evaluator: the loaded state holds no evaluation record; it starts a fresh one")
        for s in self._all_samplers():
            s.load_state_dict({"seed": self.seed, "step": 0})
        self.n_evals = self._flushed = 0
        self._hist = []
        self.count.zero_()
        self.ring_val.fill_(float("nan"))
        self.ring_iter.fill_(-1)
        self.best_val.fill_(self._worst)
        self.best_iter.fill_(-1)
        self.flag.zero_()
        self.snap_flat.zero_()
        for b in self.snap_buffers.values():
            b.zero_()
