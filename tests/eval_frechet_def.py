"""Several fake sets against one real set: the data and the float64 reference of tests/test_eval_frechet_gpu.py, composed from
tests/frechet_def.py (its definition, its error model and its data generator).  Test code only: numpy, no GPU, nothing of
the product."""
import numpy as np

import frechet_def

MODES = ("pose", "motion")
# nsets, K, n, m, t, C, V: d = 1 with exactly two motion points; d = 15 (odd: a padded index); d = 48 (the last size of the
# 3 x 3 register tile) with the maximum number of sets; d = 75 (the 6 x 6 tile, NTU's frame); d = 96 (the cap); 80 and 144
# pose points per class: 2 and 3 chunks of 64, the last one ragged
SHAPES = [(1, 1, 2, 2, 2, 1, 1), (2, 3, 5, 4, 8, 3, 5), (4, 2, 6, 7, 5, 3, 16), (3, 2, 4, 4, 6, 3, 25), (1, 2, 3, 3, 4, 2, 48),
          (2, 2, 5, 9, 16, 3, 5)]
DEF_SHAPES = [s for s in SHAPES if s[5] * s[6] in (15, 75, 96)]
SEED = 1


def make_sets(seed, nsets, K, n, m, C, t, V):
    """real (K, n, C, t, V) and nsets fake sets (K, m, C, t, V), float32: the generator of frechet_def asked for nsets * m
    fakes per class, dealt out to the sets in turn - every set is drawn around the same real set"""
    real, fake = frechet_def.make_data(seed, K, n, nsets * m, C, t, V)
    return real, [np.ascontiguousarray(fake[:, g::nsets]) for g in range(nsets)]


def reference_sets(real, fakes, mode):
    """per fake set (per-class dicts of frechet_def.one_class with their tolerances under "tol", mean over classes); the
    brackets are capped here, on the definition alone (frechet_def.caps), before anything of a kernel is looked at"""
    K, n, C, t, V = real.shape
    fr, d = t - (mode == "motion"), C * V
    out = []
    for fake in fakes:
        m = fake.shape[1]
        per, mean = frechet_def.reference(real, fake, mode)
        xmax = max(np.abs(frechet_def.points(x.reshape((-1,) + x.shape[2:]), mode)).max() for x in (real, fake))
        for ref in per:
            ref["tol"] = frechet_def.tolerances(ref, n * fr, m * fr, d, xmax)
            cap_b, cap_e = frechet_def.caps(n * fr, m * fr, d, ref["scale"])
            assert ref["tol"]["b"] <= cap_b and ref["tol"]["e2e"] <= cap_e, ("the bracket is too wide to test anything", ref["tol"])
        out.append((per, mean))
    return out
