#!/usr/bin/env python3
"""Generate tests/golden/frechet_ref.npz by running the REFERENCE's ``calculate_frechet_distance``
(evaluation/fid-actions.py) on CPU in float64.

The script's module level parses argv and loads a network, so it is never imported: its source is parsed with ``ast`` and
only the ``calculate_frechet_distance`` function is executed, with ``np`` and ``scipy.linalg`` injected.  Only data is
stored, for every case <p> (full-rank sets with P >= 4 d only: the reference's ``sqrtm`` goes its own way on singular
products):

  <p>_real_q   int8 (P_r, d)   real points = real_q / 127 (fp32)
  <p>_fake_q   int8 (P_f, d)   fake points = fake_q / 127 (fp32)
  <p>_fd       float64 ()      calculate_frechet_distance(mean(F), cov(F), mean(R), cov(R)) with np.mean(axis=0) and
                               np.cov(rowvar=False) of the float64 points, as the script's caller forms them

    python tests/golden/make_frechet_fixtures.py <path of the reference checkout>
"""
import ast
import os
import sys

import numpy as np
from scipy import linalg

HERE = os.path.dirname(os.path.abspath(__file__))

# name, P_r, P_f, d, seed
CASES = (("ntu", 320, 300, 75, 21), ("h36m", 200, 200, 48, 22), ("small", 64, 50, 12, 23), ("max", 384, 384, 96, 24))


def load_reference(ref_root):
    src = open(os.path.join(ref_root, "evaluation", "fid-actions.py")).read()
    tree = ast.parse(src)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "calculate_frechet_distance"]
    assert len(keep) == 1, "calculate_frechet_distance not found"
    ns = {"np": np, "linalg": linalg}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "fid-actions.py", "exec"), ns)
    return ns["calculate_frechet_distance"]


def case_data(seed, P_r, P_f, d):
    """int8 correlated Gaussian points, column scales 0.05 .. 1; the fake set mixed a little differently and shifted"""
    g = np.random.RandomState(seed)
    mix = g.randn(d, d) / np.sqrt(d)
    col = g.uniform(0.05, 1.0, size=d)
    mix_f = mix + 0.3 * g.randn(d, d) / np.sqrt(d)
    shift = 0.1 * g.randn(d)
    real = g.randn(P_r, d) @ mix * col
    fake = g.randn(P_f, d) @ mix_f * col * 0.9 + shift
    quant = lambda z: np.clip(np.round(127 * 0.3 * z), -127, 127).astype(np.int8)      # noqa: E731
    return quant(real), quant(fake)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    out = {}
    for name, P_r, P_f, d, seed in CASES:
        assert min(P_r, P_f) >= 4 * d
        real_q, fake_q = case_data(seed, P_r, P_f, d)
        real = (real_q.astype(np.float32) / np.float32(127)).astype(np.float64)
        fake = (fake_q.astype(np.float32) / np.float32(127)).astype(np.float64)
        val = ref(fake.mean(axis=0), np.cov(fake, rowvar=False), real.mean(axis=0), np.cov(real, rowvar=False))
        out.update({name + "_real_q": real_q, name + "_fake_q": fake_q, name + "_fd": np.float64(val)})
        print(name, P_r, P_f, d, "calculate_frechet_distance", val)
    np.savez_compressed(os.path.join(HERE, "frechet_ref.npz"), **out)


if __name__ == "__main__":
    main()
