"""Evaluator(memorisation_method="gram") on the MI355X: at the small shapes of
tests/test_eval_memorisation_gpu.py every metrics.csv column equals the "exact" run bit for bit, in raw and in feature space,
with two generators (live + ema in a training loop: "a" and "b" here); the one-off leave-one-out pass and the real side's
scores agree as well; an evaluation makes ONE kg_nn_gram call (six launches) whatever the number of generators."""
import numpy as np
import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd.evaluate import Evaluator, write_metrics_csv

from test_eval_classifier_gpu import DEV, K, P, flat_generator, make_ev, same_bits, trained  # noqa: F401
from test_eval_memorisation_gpu import kind_kw, mem_state, training_set

pytestmark = pytest.mark.gpu
N_ROUND = K * P


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    nv.load_library()


@pytest.fixture(scope="module")
def runs(trained):  # noqa: F811
    Ga, Gb = flat_generator(1), flat_generator(2)
    out = {"Ga": Ga, "Gb": Gb, "clf": trained}
    for kind in ("features", "raw"):
        train, lab = training_set(Ga, kind)
        base, mem = kind_kw(kind, trained, train, lab)
        out[kind + "/set"] = (train, lab)
        for method in ("exact", "gram"):
            it = torch.full((1,), 2 ** 24 + 3, dtype=torch.int64, device=DEV)
            ev = make_ev({"a": Ga, "b": Gb}, it, memorisation_method=method, **base, **mem)
            assert ev.use_graph and ev.memorisation_method == method
            states = []
            for _ in range(3):
                ev.evaluate()
                states.append(mem_state(ev))
                it += 2
            out[kind, method] = (ev, ev.records(), states)
    return out


@pytest.mark.parametrize("kind", ["features", "raw"])
def test_every_column_equals_the_exact_run(runs, kind, tmp_path):
    (ev_e, rec_e, st_e), (ev_g, rec_g, st_g) = runs[kind, "exact"], runs[kind, "gram"]
    assert rec_g["names"] == rec_e["names"] and rec_g["scores"].shape[0] == 3
    for key in ("iteration", "scores", "improved"):
        assert same_bits(rec_g[key], rec_e[key]), key
    for k in range(3):
        for key in st_e[k]:
            assert same_bits(st_g[k][key], st_e[k][key]), (k, key)
    for name, rec in (("exact", rec_e), ("gram", rec_g)):
        write_metrics_csv(str(tmp_path / (name + ".csv")), rec)
    assert (tmp_path / "gram.csv").read_bytes() == (tmp_path / "exact.csv").read_bytes()
    # the one-off passes: leave-one-out distances and the real side's own scores
    assert same_bits(ev_g._mem_loo, ev_e._mem_loo)
    for key in ("authenticity", "label_agreement", "counts"):
        assert torch.equal(ev_g.memorisation_real[key], ev_e.memorisation_real[key])
    st = ev_g.memorisation_stats
    assert st.shape == (2, 1, 2) and st.dtype == torch.int32 and (st.sum(-1) == N_ROUND).all()
    print(kind, "stats (certified, fallback) per generator:", st[:, 0].tolist())
    assert ev_e.memorisation_stats is None and ev_e.memorisation_method == "exact"
    new = rec_g["scores"][:, -4:]
    assert np.isfinite(new).all() and (new >= 0).all() and (new <= 1).all()


@pytest.mark.parametrize("kind", ["features", "raw"])
@pytest.mark.parametrize("gens", [("a",), ("a", "b")])
def test_one_gram_call_per_evaluation(runs, monkeypatch, kind, gens):
    """construction: the norms of the training side (the Evaluator's and the real side's call), the leave-one-out pass and the
    real side through kg_nn_gram; an evaluation: ONE kg_nn_gram over all generators with the cached norms, ONE kg_nn_scores -
    never kg_nn, kg_nn_sets or kg_nn_norms"""
    calls = {k: [] for k in ("nn_gram", "nn_scores", "nn", "nn_sets", "nn_norms")}
    plain = {k: getattr(nv, k) for k in calls}

    def spy(name):
        def f(first, *a, **kw):
            calls[name].append((len(first) if isinstance(first, (list, tuple)) else 1, kw.get("base_norms")))
            return plain[name](first, *a, **kw)
        return f

    for name in calls:
        monkeypatch.setattr(nv, name, spy(name))
    train, lab = runs[kind + "/set"]
    base, mem = kind_kw(kind, runs["clf"], train, lab)
    G = {"a": runs["Ga"], "b": runs["Gb"]}
    ev = make_ev({g: G[g] for g in gens}, use_graph=False, memorisation_method="gram", **base, **mem)
    assert [c[0] for c in calls["nn_gram"]] == [1, 1] and len(calls["nn_norms"]) == 2 and calls["nn"] == [] and calls["nn_sets"] == []
    counted = {}
    nv.flop_count = counted
    try:
        for _ in range(2):
            for v in calls.values():
                del v[:]
            counted.clear()
            ev.evaluate()
            torch.cuda.synchronize()
            assert [c[0] for c in calls["nn_gram"]] == [len(gens)] and calls["nn_gram"][0][1] is ev._mem_norms
            assert len(calls["nn_scores"]) == 1 and calls["nn"] == [] and calls["nn_sets"] == [] and calls["nn_norms"] == []
            assert "kg_nn_gram" in counted and "kg_nn_sets" not in counted and "kg_nn" not in counted
    finally:
        nv.flop_count = None
    ref = runs[kind, "gram"][1]
    if gens == ("a", "b"):
        assert same_bits(ev.records()["scores"], ref["scores"][:2])


def test_unknown_method_is_refused(runs):
    with pytest.raises(ValueError, match="method='cdist' is none of 'exact', 'gram'"):
        make_ev({"a": runs["Ga"]}, memorisation_method="cdist")
    assert Evaluator.__init__.__defaults__[-1] == "exact"
