"""Plain-numpy restatement of `uniform_spectral_estimate` as include/rmhip.h states it (frames by the index formulas, numpy's FFT, row
selection, scaled power).  It shares nothing with the library: tests/test_spectral_host.py checks it against scipy, and
tests/test_gpu_spectral.py checks the device against it."""
import numpy as np

SLIDING, COLUMN_SLIDING, FOLDED_COLUMNS = 0, 1, 2
ONESIDED, TWOSIDED, CENTERED = 0, 1, 2


def centered_shift(nfft):
    """Row r of the centered range is S[(r + shift) % nfft]."""
    return nfft // 2 + 1 if nfft % 2 == 0 else (nfft + 1) // 2


def frames(x, input_len, window, nfft, frame_count, mode, hop=0, input_rows=0, fpc=0):
    """[nfft, frame_count] windowed frames of the flat signal x (real or complex); also the per-frame sum of |x w| over every term
    that entered (what a fold's rounding is proportional to)."""
    x = np.asarray(x).reshape(-1)
    w = np.asarray(window, dtype=np.float64).reshape(-1)
    out = np.zeros((nfft, frame_count), dtype=np.complex128 if np.iscomplexobj(x) else np.float64)
    mass = np.zeros(frame_count)
    for c in range(frame_count):
        if mode == SLIDING:
            base = c * hop
        elif mode == COLUMN_SLIDING:
            base = (c // fpc) * input_rows + (c % fpc) * hop
        else:
            base = c * input_rows
        for r in range(nfft):
            terms = range(r, len(w), nfft) if mode == FOLDED_COLUMNS else ([r] if r < len(w) else [])
            for rr in terms:  # ascending
                src = base + rr
                if src < input_len:
                    t = x[src] * w[rr]
                    out[r, c] += t
                    mass[c] += abs(t)
    return out, mass


def select(S, nfft, rng):
    """Rows of the full spectrum S [nfft, frames] that the range keeps, and the power scale of each row."""
    if rng == ONESIDED:
        rows = nfft // 2 + 1
        scale = np.full(rows, 2.0)
        scale[0] = 1.0
        if nfft % 2 == 0:
            scale[rows - 1] = 1.0
        return S[:rows], scale
    if rng == TWOSIDED:
        return S, np.ones(nfft)
    idx = (np.arange(nfft) + centered_shift(nfft)) % nfft
    return S[idx], np.ones(nfft)


def estimate(x, input_len, window, nfft, frame_count, mode, rng, denominator, hop=0, input_rows=0, fpc=0):
    """(s, ps, scale, frames, mass): s complex [rows, frame_count], ps real [rows, frame_count]."""
    f, mass = frames(x, input_len, window, nfft, frame_count, mode, hop, input_rows, fpc)
    S = np.fft.fft(f, axis=0)
    s, scale = select(S, nfft, rng)
    ps = (s.real ** 2 + s.imag ** 2) * scale[:, None] / denominator
    return s, ps, scale, f, mass
