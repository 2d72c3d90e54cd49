"""Host definition of the evaluation record - what tests/test_eval_cpu.py and tests/test_eval_gpu.py pin
kg_eval_record, kg_copy_if and the layers above them against.  Everything here is exact: fp32 values are compared as
fp32 values, the iteration is an int64, so the GPU tests compare bit for bit and no tolerance exists.

    improved = (s < best_val)            s = scores[select]; strict: a NaN never wins, an equal score keeps the earlier one
    slot     = count mod ring_len:  ring_val[slot] = scores,  ring_iter[slot] = [iteration, improved]
    flag     = improved;  improved: best_val = s, best_iter = iteration;  count += 1
    start    : best_val = +inf, best_iter = -1, count = 0; an absent iteration is recorded as -1

``pair_rows``: the order of the real side - row j*K + c is the j-th sample (in index order) of class c, the label order
of a Sampler round (generate.py:91).  ``copy_if``: dst = src when the flag is set, else dst untouched.
"""
import numpy as np


class Record:
    def __init__(self, nscores, select, ring_len):
        assert 1 <= nscores <= 8 and 0 <= select < nscores and ring_len >= 1
        self.nscores, self.select, self.ring_len = nscores, select, ring_len
        self.count = 0
        self.ring_val = np.full((ring_len, nscores), np.nan, dtype=np.float32)
        self.ring_iter = np.full((ring_len, 2), -1, dtype=np.int64)
        self.best_val = np.float32(np.inf)
        self.best_iter = np.int64(-1)
        self.flag = np.int32(0)

    def append(self, scores, iteration=None):
        scores = np.asarray(scores, dtype=np.float32).reshape(self.nscores)
        it = np.int64(-1 if iteration is None else iteration)
        s = scores[self.select]
        improved = bool(s < self.best_val)              # False for a NaN on either side
        k = self.count % self.ring_len
        self.ring_val[k] = scores
        self.ring_iter[k] = (it, int(improved))
        self.flag = np.int32(improved)
        if improved:
            self.best_val, self.best_iter = s, it
        self.count += 1
        return improved


def pair_rows(labels, n_classes, pairs):
    """indices so that entry j*n_classes + c is the j-th sample with label c; ValueError if a class is short"""
    labels = list(labels)
    out = [None] * (pairs * n_classes)
    for c in range(n_classes):
        idx = [i for i, v in enumerate(labels) if v == c]
        if len(idx) < pairs:
            raise ValueError("class %d has %d samples" % (c, len(idx)))
        for j in range(pairs):
            out[j * n_classes + c] = idx[j]
    return out


def copy_if(flag, src, dst):
    """dst after the launch (numpy arrays of one dtype)"""
    return src.copy() if flag else dst.copy()
