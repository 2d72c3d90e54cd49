"""Host (numpy) definition of what kg_step_inputs writes for iteration s (include/kgan_hip.h): the
yardstick of tests/test_train_cpu.py and tests/test_train_gpu.py.

    Philox4x32-10, key = (seed low word, seed high word), counter = (q, stream + 4 rank, s low word, s high word);
    the four output words of counter q are elements 4q .. 4q+3 of the stream
    uniform  u = (word >> 8) * 2^-24
    normals  from word pairs (x0, x1), (x2, x3):  rad = sqrt(-2 log(1 - u0)),  (rad cos(2 pi u1), rad sin(2 pi u1))
    batch    b = s mod batches_per_epoch, epoch e = s div batches_per_epoch, rows perm_e[(b world + rank) B .. + B) with
             perm_e = RandomState(seed + e).shuffle(arange(N));  real = (x * scale) + shift in fp32, two roundings
"""
import numpy as np

STREAM_Z, STREAM_ALPHA, STREAM_NOISE_D, STREAM_NOISE_G = 0, 1, 2, 3
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter (..., 4), key (..., 2) uint32 arrays (broadcast) -> (..., 4) uint32: Random123's Philox4x32 with 10 rounds"""
    c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
    k = [np.asarray(key[..., i], dtype=np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(W0)) & np.uint64(MASK), (k[1] + np.uint64(W1)) & np.uint64(MASK)]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def counters(n, stream, step, rank=0):
    """the (ceil(n / 4), 4) counters of a stream of n elements"""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    c = np.empty((q.size, 4), dtype=np.uint32)
    c[:, 0] = q & np.uint64(MASK)
    c[:, 1] = stream + 4 * rank
    c[:, 2] = step & MASK
    c[:, 3] = (step >> 32) & MASK
    return c


def words(n, seed, stream, step, rank=0):
    """the first n 32-bit words of a stream"""
    key = np.array([seed & MASK, (seed >> 32) & MASK], dtype=np.uint32)
    return philox4x32_10(counters(n, stream, step, rank), key[None, :]).reshape(-1)[:n]


def uniforms(n, seed, stream, step, rank=0):
    return (words(n, seed, stream, step, rank) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def normals(n, seed, stream, step, rank=0, dtype=np.float32):
    """Box-Muller in `dtype` from the same integer draws (float64: the reference the device is compared against)"""
    w = words((n + 3) // 4 * 4, seed, stream, step, rank).reshape(-1, 2)
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)        # exact in fp32: 24-bit integers
    u0, u1 = u[:, 0].astype(dtype), u[:, 1].astype(dtype)
    one, two_pi = dtype(1.0), dtype(np.float32(6.2831855)) if dtype == np.float32 else dtype(2.0 * np.pi)
    rad = np.sqrt(dtype(-2.0) * np.log(one - u0))
    th = two_pi * u1
    out = np.stack((rad * np.cos(th), rad * np.sin(th)), -1).astype(dtype)
    return out.reshape(-1)[:n]


def permutation(n, seed, epoch):
    idx = np.arange(n)
    np.random.RandomState(seed + epoch).shuffle(idx)
    return idx


def batch_rows(n, batch_size, seed, step, rank=0, world=1):
    """sample indices of iteration `step`"""
    bpe = (n // batch_size) // world
    epoch, b = divmod(step, bpe)
    lo = (b * world + rank) * batch_size
    return permutation(n, seed, epoch)[lo:lo + batch_size]


def batch(feeder, batch_size, t_size, seed, step, rank=0, world=1):
    """(real (B, C, t, V) fp32, labels (B,) int64) of iteration `step` from a Feeder"""
    rows = batch_rows(len(feeder), batch_size, seed, step, rank, world)
    t = min(t_size, feeder.T)
    raw = np.stack([np.asarray(feeder.data[i, :, :t, :, 0] if feeder.dataset == 'ntu' else feeder.data[i, :, :t], dtype=np.float32)
                    for i in rows])
    if feeder.norm:
        span = float(feeder.max) - float(feeder.min)
        scale, shift = 2.0 / span, -2.0 * float(feeder.min) / span - 1.0
    else:
        scale, shift = 1.0, 0.0
    real = (raw * np.float32(scale)).astype(np.float32) + np.float32(shift)
    return real.astype(np.float32), np.asarray(feeder.label, dtype=np.int64)[rows]


def plane_shapes(G, batch_size):
    return [(batch_size, 1, gcn.up_t, G.graph.num_node[gcn.lvl]) for gcn in G.st_gcn_networks]


def noise_planes(shapes, seed, stream, step, rank=0, dtype=np.float32):
    """the planes of one synthesis: consecutive runs of the stream"""
    n = sum(int(np.prod(s)) for s in shapes)
    flat = normals(n, seed, stream, step, rank, dtype)
    out, off = [], 0
    for s in shapes:
        k = int(np.prod(s))
        out.append(flat[off:off + k].reshape(s))
        off += k
    return out


def synthetic_dataset(path, n, c, t, v, n_classes, layout, seed=0):
    """a small .npy / .pkl pair in the reference's layouts: 'ntu' (N, C, T, V, 2) or 'h36m' (N, C, T, V)"""
    import os
    import pickle
    rng = np.random.RandomState(seed)
    shape = (n, c, t, v, 2) if layout == "ntu" else (n, c, t, v)
    data = (rng.rand(*shape) * 3.0 - 1.2).astype(np.float32)
    labels = rng.randint(0, n_classes, n).tolist()
    dp, lp = os.path.join(path, "data.npy"), os.path.join(path, "label.pkl")
    np.save(dp, data)
    with open(lp, "wb") as f:
        pickle.dump((["s%d" % i for i in range(n)], labels), f)
    return dp, lp
