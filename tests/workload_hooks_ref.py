"""numpy restatements of the CPU provider's three workload hooks (crates/runmat-accelerate/src/simple_provider.rs:800-883, 985-1064,
1066-1137), operation for operation in f64: the expected values of tests/test_gpu_workload_hooks.py and, checked against exact values
on the CPU, of tests/test_workload_hooks_host.py.  Test infrastructure; the product never imports it."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
SQRT_2 = 1.4142135623730951  # std::f64::consts::SQRT_2
_erf = np.frompyfunc(math.erf, 1, 1)


def erf(x):
    return np.asarray(_erf(np.asarray(x, dtype=np.float64)), dtype=np.float64)


def adam_ref(p0, g, m0, v0, iteration, learn_rate, b1, b2, epsilon):
    """provider_adam_update_values: (parameters, average_grad, average_sq_grad).  m0 / v0 None: zeros."""
    p0, g = np.asarray(p0, dtype=np.float64), np.asarray(g, dtype=np.float64)
    m0 = np.zeros_like(p0) if m0 is None else np.asarray(m0, dtype=np.float64)
    v0 = np.zeros_like(p0) if v0 is None else np.asarray(v0, dtype=np.float64)
    gc = 1.0 - math.pow(b1, float(iteration))
    sc = 1.0 - math.pow(b2, float(iteration))
    with np.errstate(all="ignore"):
        m = b1 * m0 + (1.0 - b1) * g
        v = b2 * v0 + ((1.0 - b2) * g) * g
        step = (learn_rate * (m / gc)) / (np.sqrt(v / sc) + epsilon)
        return p0 - step, m, v


def crossentropy_parts(pred, target):
    """(-t) ln(c) and (1 - t) ln(1 - c) with c = clamp(pred, 1e-12, 1 - 1e-12): the two products of provider_crossentropy_terms."""
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    eps = 1.0e-12
    c = np.where(pred < eps, eps, np.where(pred > 1.0 - eps, 1.0 - eps, pred))
    return (-target) * np.log(c), (1.0 - target) * np.log(1.0 - c)


def crossentropy_ref(pred, target, weights=None, mask=None, multi_label=False):
    first, second = crossentropy_parts(pred, target)
    loss = first - second if multi_label else first
    if weights is not None:
        loss = loss * np.asarray(weights, dtype=np.float64)
    if mask is not None:
        loss = loss * np.asarray(mask, dtype=np.float64)
    return loss


def crossentropy_bound(pred, target, weights=None, mask=None, multi_label=False):
    """4 eps (|t ln c| + |(1 - t) ln(1 - c)|) w m: 2 ulp of the device logarithm, one rounding per product and per subtraction."""
    first, second = crossentropy_parts(pred, target)
    b = np.abs(first) + (np.abs(second) if multi_label else 0.0)
    if weights is not None:
        b = b * np.asarray(weights, dtype=np.float64)
    if mask is not None:
        b = b * np.asarray(mask, dtype=np.float64)
    return 4.0 * EPS * b


def black_scholes_ref(price, strike, rate, time, vol, yld):
    """provider_black_scholes_price_pair over arrays that numpy broadcasts (trailing dimensions aligned, as blsprice aligns them)."""
    price, strike, rate, time, vol, yld = np.broadcast_arrays(*[np.asarray(a, dtype=np.float64) for a in (price, strike, rate, time, vol, yld)])
    with np.errstate(all="ignore"):
        ok = (np.isfinite(price) & np.isfinite(strike) & np.isfinite(rate) & np.isfinite(time) & np.isfinite(vol) & np.isfinite(yld)
              & (price >= 0.0) & (strike > 0.0) & (time >= 0.0) & (vol >= 0.0))
        dp = price * np.exp((-yld) * time)
        ds = strike * np.exp((-rate) * time)
        intrinsic = (time == 0.0) | (vol == 0.0)
        sqrt_time = np.sqrt(time)
        d1 = (np.log(price / strike) + (rate - yld + 0.5 * vol * vol) * time) / (vol * sqrt_time)
        d2 = d1 - vol * sqrt_time

        def ncdf(x):
            return 0.5 * (1.0 + erf(x / SQRT_2))

        call = dp * ncdf(d1) - ds * ncdf(d2)
        put = ds * ncdf(-d2) - dp * ncdf(-d1)
        call = np.where(intrinsic, np.fmax(dp - ds, 0.0), call)
        put = np.where(intrinsic, np.fmax(ds - dp, 0.0), put)
        return np.where(ok, call, np.nan), np.where(ok, put, np.nan)


def black_scholes_bound(price, strike, rate, time, yld):
    """8 eps (S e^{-qT} + K e^{-rT}) (the derivation: tests/test_gpu_workload_hooks.py)."""
    price, strike, rate, time, yld = [np.asarray(a, dtype=np.float64) for a in (price, strike, rate, time, yld)]
    return 8.0 * EPS * (price * np.exp(-yld * time) + strike * np.exp(-rate * time))


def broadcast_index(linear, output_shape, in_shape, strides):
    """provider_broadcast_index (simple_provider.rs:800-837)."""
    offset = 0
    for out_extent, in_extent, stride in zip(output_shape, in_shape, strides):
        coord = 0 if out_extent == 0 else linear % out_extent
        if out_extent != 0:
            linear //= out_extent
        offset += (0 if in_extent == 1 or out_extent == 0 else coord) * stride
    return offset
