"""Definitions the tests of precision / recall / density / coverage inside the Evaluator are pinned against.
Test code only: torch / numpy on the host, float64 and integers - everything here is exact.

``given_radii``: the counts of tests/prdc_def.py with the real radii as an ARGUMENT (kg_prdc_sets takes them as an input):
    rho_F(j) = k-th smallest of {d2(f_j, f_l) : l != j}            (computed here, left out by index)
    P_ij = [d2(r_i, f_j) <= rho_R(i)],  Q_ij = [d2(r_i, f_j) <= rho_F(j)]              rho_R: whatever the caller passes
    counts = (#{j : exists i P_ij}, #{i : exists j Q_ij}, sum_ij P_ij, #{i : exists j P_ij})
    fake_hits(j) = sum_i P_ij,  real_flags(i) = [exists j Q_ij] | [exists j P_ij] << 1

``Record2``: the record of tests/eval_def.py with up to 32 scores and a sense:
    improved = maximise ? (s > best_val) : (s < best_val)     strict; best_val starts at -inf when maximising, else +inf
"""
import numpy as np
import torch

import prdc_def


def given_radii_one_class(R, F, rho_R, k):
    R, F = R.double(), F.double()
    rr = torch.as_tensor(rho_R, dtype=torch.float64)
    rf = prdc_def.radii(F, k)
    d = prdc_def.sqdist(R, F)
    counts, hits, flags = prdc_def._counts(d <= rr[:, None], d <= rf[None, :])
    return dict(counts=counts, fake_hits=hits, real_flags=flags, radii_fake=rf)


def given_radii(R, F, rho_R, k):
    """R (K, n, D), F (K, m, D), rho_R (K, n) -> dict with a leading class axis on everything"""
    per = [given_radii_one_class(R[c], F[c], rho_R[c], k) for c in range(R.shape[0])]
    return {key: torch.stack([p[key] for p in per]) for key in per[0]}


class Record2:
    def __init__(self, nscores, select, ring_len, maximise=False):
        assert 1 <= nscores <= 32 and 0 <= select < nscores and ring_len >= 1
        self.nscores, self.select, self.ring_len, self.maximise = nscores, select, ring_len, bool(maximise)
        self.count = 0
        self.ring_val = np.full((ring_len, nscores), np.nan, dtype=np.float32)
        self.ring_iter = np.full((ring_len, 2), -1, dtype=np.int64)
        self.best_val = np.float32(-np.inf if maximise else np.inf)
        self.best_iter = np.int64(-1)
        self.flag = np.int32(0)

    def append(self, scores, iteration=None):
        scores = np.asarray(scores, dtype=np.float32).reshape(self.nscores)
        it = np.int64(-1 if iteration is None else iteration)
        s = scores[self.select]
        improved = bool(s > self.best_val) if self.maximise else bool(s < self.best_val)     # False for a NaN on either side
        k = self.count % self.ring_len
        self.ring_val[k] = scores
        self.ring_iter[k] = (it, int(improved))
        self.flag = np.int32(improved)
        if improved:
            self.best_val, self.best_iter = s, it
        self.count += 1
        return improved
