"""Host definition of the generator weight average, in float64 - what tests/test_ema_cpu.py and
tests/test_ema_gpu.py pin kg_adam_step_ema and the layers above it against.

    e_new = e_old + (1 - beta_s) (p_new - e_old)
    beta_s = decay                                        warmup == 0
           = min(decay, (1 + s) / (warmup + s))           otherwise, s = the 1-based count of the optimiser step

``decay`` and ``warmup`` are the launch's arguments, i.e. float32 values, promoted to double; ``e_old`` and ``p_new`` are
the device's own float32 values promoted to double.

Tolerance (derived, per element and step): |e_device - e_def| <= 2^-21 max(|e_old|, |p_new|) =: 2^-21 M.  The device
rounds the difference (<= 2^-24 (|p| + |e|) <= 2^-23 M), the product and the sum (<= 2^-24 M each, the factor 1 - beta_s
is at most 1), and beta_s carries a relative 2^-24 from its fp32 division, which moves (1 - beta_s)(p - e) by at most
2^-23 M: below 3 * 2^-23 M in total, and 2^-21 M leaves room for a contracted multiply-add and a division a few ulp off.
"""
import numpy as np

REL_BOUND = 2.0 ** -21


def beta(step, decay, warmup):
    """beta_s in float64 from the float32 launch arguments"""
    d, w, s = float(np.float32(decay)), float(np.float32(warmup)), float(step)
    if w == 0.0:
        return d
    return min(d, (1.0 + s) / (w + s))


def update(e_old, p_new, step, decay, warmup):
    """e_new in float64; e_old / p_new: arrays (the device's float32 values) or scalars"""
    e = np.asarray(e_old, dtype=np.float64)
    p = np.asarray(p_new, dtype=np.float64)
    return e + (1.0 - beta(step, decay, warmup)) * (p - e)


def bound(e_old, p_new):
    """the per-element tolerance of one step"""
    return REL_BOUND * np.maximum(np.abs(np.asarray(e_old, dtype=np.float64)), np.abs(np.asarray(p_new, dtype=np.float64)))


def adam_step_ema(p, g, m, v, e, lr, b1, b2, eps, step_t, grad_scale, zero_grad, decay, warmup):
    """``_native.adam_step_ema`` on the host for the CPU host-logic tests: the emulated ``_native.adam_step`` (whatever is
    installed at call time), then the definition on the result, rounded to float32."""
    import torch
    from kinetic_gan_amd import _native
    _native.adam_step(p, g, m, v, lr, b1, b2, eps, step_t, grad_scale, zero_grad=zero_grad)
    new = update(e.detach().numpy(), p.detach().numpy(), int(step_t.item()), decay, warmup)
    e.copy_(torch.as_tensor(new.astype(np.float32)))
