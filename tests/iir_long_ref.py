"""Numpy model of `rmhip_iir_filter_long` (runmat_amd/csrc/signal_ops.hip) and the yardsticks its tests share.

The model restates, operation by operation in f64, what the device does for one channel:
  FIR        the CPU's nested sum formed from the innermost term outwards (fir_nested);
  recursive  the chunked scan (chunked_filter): tables H and T_L from S runs of the recurrence over zeros, the chunk length by the L rule
             (choose_chunk), a zero-state pass per chunk, the sequential state pass s(c+1) = T_L s(c) + sz(c), the correction
             y += H s(c), and a sequential run of the tail from its true entry state.
The yardsticks: the sequential recurrence in np.longdouble (exact_filter), the noise floor of the accuracy contract (noise_floor) and the
two bounds (output_bound, state_bound).  The ten filters of the contract are FILTERS."""
import numpy as np

CHUNKS = (256, 512, 1024, 2048, 4096, 8192)
MIN_LEN = 2 * CHUNKS[0]  # shorter signals run the sequential recurrence


def normalise(b, a):
    """(bn, an) of length order = max(nb, na), as the CPU's complex division by a(1) rounds them."""
    b, a = np.asarray(b, dtype=np.float64).ravel(), np.asarray(a, dtype=np.float64).ravel()
    order = max(b.size, a.size)
    a0 = a[0]
    den = a0 * a0 + 0.0
    bn, an = np.zeros(order), np.zeros(order)
    bn[:b.size] = (b * a0 + 0.0) / den
    an[0] = 1.0
    an[1:a.size] = (a[1:] * a0 + 0.0) / den
    return bn, an


def df2t(bn, an, x, st):
    """The sequential recurrence on arrays whose first axis is time (x: N x ..., st: S x ...), in the dtype of its operands."""
    S = bn.size - 1
    ext = np.zeros((S + 1,) + st.shape[1:], dtype=st.dtype)  # the states and, after them, the 0.0 that is the last state's `next`
    ext[:S] = st
    bcol, acol = (v[1:].reshape((S,) + (1,) * (st.ndim - 1)) for v in (bn, an))
    y = np.empty_like(x)
    for n in range(x.shape[0]):
        xn = x[n]
        yv = bn[0] * xn + ext[0]
        y[n] = yv
        ext[:S] = (bcol * xn + ext[1:]) - acol * yv  # every state at once: the same rounded operations as the loop over i
    return y, ext[:S].copy()


def exact_filter(b, a, x, zi=None):
    """The recurrence in np.longdouble on the normalised f64 coefficients.  x: N x channels (or N,), zi: S x channels."""
    bn, an = normalise(b, a)
    x = np.asarray(x, dtype=np.float64)
    st = np.zeros((bn.size - 1,) + x.shape[1:], dtype=np.longdouble)
    if zi is not None:
        st = st + np.asarray(zi, dtype=np.float64).reshape(st.shape)
    return df2t(bn.astype(np.longdouble), an.astype(np.longdouble), x.astype(np.longdouble), st)


def longdouble_is_wide() -> bool:
    return np.finfo(np.longdouble).nmant >= 63


def impulse_response(b, a, n):
    bn, an = normalise(b, a)
    d = np.zeros(n)
    d[0] = 1.0
    return df2t(bn, an, d, np.zeros(bn.size - 1))[0]


def noise_floor(b, a, x, last=None):
    """order * 2^-52 * max_n sum_m |g[m]| |x[n - m]|, the maximum taken over every channel.  x: N x channels (or N,).  `last`: the maximum
    runs over the last `last` samples only, the ones before them are history."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    x = x.reshape(x.shape[0], -1)
    n = x.shape[0]
    g = np.abs(impulse_response(b, a, n))
    size = 1 << int(np.ceil(np.log2(2 * n)))
    G = np.fft.rfft(g, size)
    conv = np.fft.irfft(np.fft.rfft(x, size, axis=0) * G[:, None], size, axis=0)[:n]
    if last is not None:
        conv = conv[n - last:]
    return max(np.size(b), np.size(a)) * 2.0 ** -52 * float(conv.max())


def output_bound(y_ref, y_exact, floor):
    return 8.0 * max(float(np.max(np.abs(y_ref - y_exact))), floor)


def state_bound(zf_ref, zf_exact, b, a, floor):
    bn, an = normalise(b, a)
    return 16.0 * max(float(np.max(np.abs(zf_ref - zf_exact))), float(np.abs(bn).sum() + np.abs(an).sum()) * floor)


# ---- FIR ------------------------------------------------------------------------------------------------------------------------------

def is_fir(an) -> bool:
    return not np.any(an[1:] != 0.0)


def fir_nested(b, a, x, zi=None):
    """y[n] = b0 x[n] + (b1 x[n-1] + (b2 x[n-2] + ... )), the chain ending in + 0.0 or in zi[n] when n < S; the final state the same way."""
    bn, an = normalise(b, a)
    assert is_fir(an)
    x = np.asarray(x, dtype=np.float64).ravel()
    N, S = x.size, bn.size - 1
    z = np.zeros(S) if zi is None else np.asarray(zi, dtype=np.float64).ravel()
    y = np.empty(N)
    for n in range(N):
        K = min(n, S)
        acc = z[n] if n < S else 0.0
        for k in range(K, 0, -1):
            acc = bn[k] * x[n - k] + acc
        y[n] = bn[0] * x[n] + acc
    zf = np.empty(S)
    for i in range(S):  # zf[i] = b[i+1] x[N-1] + (b[i+2] x[N-2] + ...): K terms, ending in zi[i + N] when the signal is that short
        K = min(N, S - i)
        acc = z[i + N] if i + N < S else 0.0
        for k in range(K, 0, -1):
            acc = bn[i + k] * x[N - k] + acc
        zf[i] = acc
    return y, zf


# ---- recursive: the chunked scan --------------------------------------------------------------------------------------------------------

def tables(bn, an, L):
    """H (L x S): zero-input response at sample k to unit state i; T (S x S): column i is the state after L samples from unit state i."""
    S = bn.size - 1
    H, T = df2t(bn, an, np.zeros((L, S)), np.eye(S))
    return H, T


def admissible(T) -> bool:
    return bool(np.all(np.isfinite(T)) and np.abs(T).sum(axis=1).max() <= 1.0)


def choose_chunk(bn, an, n=None):
    """The smallest L of CHUNKS whose T_L is finite with largest absolute row sum <= 1 (None: the filter is not contractive over a chunk).
    With a signal length n only chunks that fit twice are tried; 0 says the signal is too short for the first admissible one."""
    for L in CHUNKS:
        if n is not None and 2 * L > n:
            return 0
        if admissible(tables(bn, an, L)[1]):
            return L
    return None


def chunked_filter(b, a, x, zi=None, L=None):
    """-> (y, zf, L), or None when the request is declined.  One channel."""
    bn, an = normalise(b, a)
    x = np.asarray(x, dtype=np.float64).ravel()
    N, S = x.size, bn.size - 1
    s = np.zeros(S) if zi is None else np.asarray(zi, dtype=np.float64).ravel().copy()
    if L is None:
        L = choose_chunk(bn, an, N)
    if L is None:
        return None
    if L == 0 or N < 2 * L:
        y, zf = df2t(bn, an, x, s)
        return y, zf, 0
    H, T = tables(bn, an, L)
    nfull = N // L
    # zero-state pass: every full chunk at once
    yz, sz = df2t(bn, an, x[:nfull * L].reshape(nfull, L).T.copy(), np.zeros((S, nfull)))
    y = np.empty(N)
    for c in range(nfull):
        corr = np.zeros(L)
        for i in range(S):
            corr = corr + H[:, i] * s[i]
        y[c * L:(c + 1) * L] = yz[:, c] + corr
        nxt = np.zeros(S)
        for i in range(S):
            nxt = nxt + T[:, i] * s[i]
        s = nxt + sz[:, c]
    y[nfull * L:], zf = df2t(bn, an, x[nfull * L:], s)
    if not (np.all(np.isfinite(y)) and np.all(np.isfinite(zf))):
        return None
    return y, zf, L


# ---- the ten filters of the accuracy contract -------------------------------------------------------------------------------------------

def _conj_poles(count, radius):
    pairs = count // 2
    theta = np.pi * (np.arange(pairs) + 1.0) / (pairs + 1.0)
    return np.concatenate([radius * np.exp(1j * theta), radius * np.exp(-1j * theta)])


def _numerator(k, n):
    return np.random.default_rng(9000 + k).standard_normal(n)


def _random_12_10():
    rng = np.random.default_rng(347)
    return rng.standard_normal(12), np.concatenate([[1.0], 0.05 * rng.standard_normal(9)])


FILTERS = {
    "double_pole_0.9": (_numerator(0, 3), np.poly([0.9, 0.9])),
    "double_pole_0.995": (_numerator(1, 3), np.poly([0.995, 0.995])),
    "integrator": (np.array([1.0]), np.array([1.0, -1.0])),
    "leaky_average": (np.array([0.01]), np.array([1.0, -0.99])),
    "order4_conj_0.9": (_numerator(4, 5), np.real(np.poly(_conj_poles(4, 0.9)))),
    "order8_0.8": (_numerator(5, 9), np.real(np.poly(_conj_poles(8, 0.8)))),
    "order8_0.97": (_numerator(6, 9), np.real(np.poly(_conj_poles(8, 0.97)))),
    "order6_0.99": (_numerator(7, 7), np.real(np.poly(_conj_poles(6, 0.99)))),
    "order16_0.6": (_numerator(8, 17), np.real(np.poly(_conj_poles(16, 0.6)))),
    "random_12_10": _random_12_10(),
}
UNSTABLE = (np.array([1.0]), np.array([1.0, -1.01]))


def ratios(b, a, x, zi, y, zf, y_ref, zf_ref):
    """(output error over its bound's base, state error over its bound's base): the contract is ratio <= 8 and <= 16."""
    ye, ze = exact_filter(b, a, x, zi)
    floor = noise_floor(b, a, x)
    bn, an = normalise(b, a)
    out = float(np.max(np.abs(y - ye))) / max(float(np.max(np.abs(y_ref - ye))), floor)
    st = float(np.max(np.abs(zf - ze))) / max(float(np.max(np.abs(zf_ref - ze))), float(np.abs(bn).sum() + np.abs(an).sum()) * floor)
    return out, st


def exact_states_at(b, a, x, marks):
    """One channel: the longdouble recurrence carried through x, -> {n: the state entering sample n} for n in marks (n = len(x): final)."""
    bn, an = (v.astype(np.longdouble) for v in normalise(b, a))
    order = bn.size
    bl, al = list(bn), list(an)
    st = [np.longdouble(0.0)] * (order - 1) + [np.longdouble(0.0)]  # st[order - 1] stays 0: the `next` of the last state
    out, marks = {}, set(marks)
    n = 0
    for xn in np.asarray(x, dtype=np.float64).astype(np.longdouble):
        if n in marks:
            out[n] = np.array(st[:order - 1], dtype=np.longdouble)
        yv = bl[0] * xn + st[0]
        for i in range(1, order):
            st[i - 1] = (bl[i] * xn + st[i]) - al[i] * yv
        n += 1
    if n in marks:
        out[n] = np.array(st[:order - 1], dtype=np.longdouble)
    return out


def oracle_fir_folded(oracle_iir, b, a, x, zi=None, seg=1024):
    """oracle_iir (the oracle's loop) on one long FIR channel, folded: an FIR output depends on the order - 1 samples before it only, so the
    signal is cut into segments of `seg` samples, each preceded by the S samples before it, and the segments run as the channels of ONE call
    from zero states (the first segment alone carries zi).  Every value is the one the loop over the whole signal produces."""
    x = np.asarray(x, dtype=np.float64).ravel()
    N, S = x.size, max(np.size(b), np.size(a)) - 1
    assert N >= seg + S and S >= 1
    y = np.empty(N)
    y[:seg] = oracle_iir(b, a, x[:seg], 0, zi)[0]
    starts = np.arange(seg, N, seg)
    M = np.zeros((seg + S, starts.size))
    for j, s in enumerate(starts):
        hi = min(N, s + seg)
        M[:hi - (s - S), j] = x[s - S:hi]
    Y = oracle_iir(b, a, M, 0)[0]
    for j, s in enumerate(starts):
        hi = min(N, s + seg)
        y[s:hi] = Y[S:S + hi - s, j]
    return y, oracle_iir(b, a, x[N - S:], 0)[1]
