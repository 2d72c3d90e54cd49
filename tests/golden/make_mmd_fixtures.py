#!/usr/bin/env python3
"""Generate tests/golden/mmd_ref.npz by running the REFERENCE's MMD code (evaluation/mmd-actions.py) on CPU in fp32.

The script's module level parses argv and creates run directories, so it is never imported: its source is parsed with
``ast`` and only the ``MMD`` class and the ``calcualte_mmd`` function are executed, with ``opt`` injected and
``Tensor.cuda`` shimmed to the identity.  Only data is stored:

  <p>_real_q   int8 (N, C, T, V)   real samples = real_q / 127 (fp32, numpy)
  <p>_fake     the fake samples are real * <p>_fake_scale + <p>_fake_shift (fp32, numpy; per class a different pair,
               so that each class's winning bandwidth has an MMD of ~0.05-0.5)
  <p>_labels   int64 (N,)          class ids, in a seeded order (the first sample of a class is not at a fixed stride)
  <p>_seq_<mode>   float64 (K, 14) compute_sequence_mmd(gen0, real0, 10**j), j = -4..9, of each class's first samples
  <p>_calc_<mode>  float64 ()      calcualte_mmd(gen, real, one_hot(labels)) with opt.mmd_mode = mode

for p = h36m (10 classes x 2 samples, T = 32, V = 16) and ntu (60 classes x 1 sample, T = 64, V = 25).

    python tests/golden/make_mmd_fixtures.py <path of the reference checkout>
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = (("h36m", 10, 2, 3, 32, 16, 11), ("ntu", 60, 1, 3, 64, 25, 12))


def load_reference(ref_root):
    src = open(os.path.join(ref_root, "evaluation", "mmd-actions.py")).read()
    tree = ast.parse(src)
    keep = [n for n in tree.body if (isinstance(n, ast.ClassDef) and n.name == "MMD")
            or (isinstance(n, ast.FunctionDef) and n.name == "calcualte_mmd")]
    assert len(keep) == 2, "MMD / calcualte_mmd not found"
    ns = {"np": np, "torch": torch, "opt": types.SimpleNamespace(mmd_mode="avg")}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "mmd-actions.py", "exec"), ns)
    return ns


def case_data(rng, K, per, C, T, V):
    n = K * per
    real_q = rng.randint(-127, 128, size=(n, C, T, V)).astype(np.int8)
    labels = rng.permutation(np.repeat(np.arange(K), per)).astype(np.int64)
    scale = rng.uniform(0.9, 1.3, size=K).astype(np.float32)
    shift = rng.uniform(-0.2, 0.2, size=K).astype(np.float32)
    return real_q, labels, scale, shift


def fake_of(real, labels, scale, shift):
    return (real * scale[labels][:, None, None, None] + shift[labels][:, None, None, None]).astype(np.float32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    torch.Tensor.cuda = lambda self, *a, **k: self
    ref = load_reference(sys.argv[1])
    torch.set_num_threads(8)
    out = {}
    for name, K, per, C, T, V, seed in CASES:
        rng = np.random.RandomState(seed)
        real_q, labels, scale, shift = case_data(rng, K, per, C, T, V)
        real = real_q.astype(np.float32) / np.float32(127)
        fake = fake_of(real, labels, scale, shift)
        out.update({name + "_real_q": real_q, name + "_labels": labels, name + "_fake_scale": scale,
                    name + "_fake_shift": shift})
        gen_l, real_l = fake.transpose(0, 3, 2, 1), real.transpose(0, 3, 2, 1)      # mmd-actions.py:180-181
        one_hot = np.zeros((labels.size, K))
        one_hot[np.arange(labels.size), labels] = 1
        for mode in ("avg", "joint"):
            mmd = ref["MMD"](mode, 1)
            seq = np.zeros((K, 14))
            for c in range(K):
                i = int(np.flatnonzero(labels == c)[0])
                g0, r0 = torch.tensor(np.ascontiguousarray(gen_l[i])), torch.tensor(np.ascontiguousarray(real_l[i]))
                seq[c] = [mmd.compute_sequence_mmd(g0, r0, 10 ** j) for j in range(-4, 10)]
            ref["opt"].mmd_mode = mode
            calc = ref["calcualte_mmd"](gen_l, real_l, one_hot)
            out[name + "_seq_" + mode] = seq
            out[name + "_calc_" + mode] = np.float64(calc)
            print(name, mode, "calcualte_mmd", calc)
    np.savez_compressed(os.path.join(HERE, "mmd_ref.npz"), **out)


if __name__ == "__main__":
    main()
