"""fp64 twin of the flat optimizers' weight average (svol_ema_flat, include/svol_hip.h): the warm-up schedule, the recursion and the
error bar a device result is held to.  Inputs are fp32 values (the decay included: the kernel takes a float), arithmetic is fp64.

    d_t   = decay                                  warm-up off
    d_t   = min(decay, (1 + t) / (10 + t))         warm-up on, t the 1-based index of the update being averaged
    ema_t = ema_{t-1} + (1 - d_t) * (p_t - ema_{t-1})

The bar of one application to the DEVICE's own previous average: |got - ref| <= 2^-23 * (|ref| + 2 * (1 - d) * |p - ema_prev|).
The kernel rounds three times in fp32, each at most 2^-24 relative: p - ema (scaled by 1 - d on its way into the result), 1 - d
(same scale), and the fma's result (relative to |ref|); the bar is twice that sum.  d itself is formed in double on the device."""
import numpy as np
import torch


def decay_at(decay, warmup, t):
    d = float(np.float32(decay))
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def ema_step(ema_prev, p, d):
    """one application, fp64 tensors out of tensors of any float dtype"""
    e, q = ema_prev.double(), p.double()
    return e + (1.0 - d) * (q - e)


def ema_run(ema0, ps, decay, warmup, t0=1):
    """the recursion over the parameter values ``ps`` of consecutive updates t0, t0 + 1, ...: the list of fp64 averages"""
    out, e = [], ema0.double()
    for k, p in enumerate(ps):
        e = ema_step(e, p, decay_at(decay, warmup, t0 + k))
        out.append(e)
    return out


def bound(ref, p, ema_prev, d):
    return 2.0 ** -23 * (ref.abs() + 2.0 * (1.0 - d) * (p.double() - ema_prev.double()).abs())


def check(got, ema_prev, p, d, what):
    """``got`` (fp32, the device's result) against one fp64 application to ``ema_prev`` (the device's previous average)"""
    ref = ema_step(ema_prev, p, d)
    err, bar = (got.double() - ref).abs(), bound(ref, p, ema_prev, d)
    worst = float((err - bar).max())
    print(f'{what}: d = {d:.6f}, max err = {float(err.max()):.3e}, max err - bar = {worst:.3e}')
    assert bool((err <= bar).all()), (what, float(err.max()), worst)
