"""The numpy restatement of uniform_spectral_estimate (tests/spectral_ref.py) against scipy: the three frame modes are what spectrogram,
welch and a folded periodogram compute, each to 1e-12 relative to max(ps); the centered rotation against its index formula."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import spectral_ref as ref  # noqa: E402

signal = pytest.importorskip("scipy.signal")
FS = 2.0 * np.pi
RTOL = 1e-12


def close(got, want):
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= RTOL * np.max(np.abs(want)), float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("rng", [ref.ONESIDED, ref.TWOSIDED])
def test_sliding_is_scipy_spectrogram(rng):
    x = np.random.default_rng(1).standard_normal(1000)
    w = signal.get_window("hann", 64)
    frames = (1000 - 64) // 16 + 1
    _, ps, _, _, _ = ref.estimate(x, x.size, w, 64, frames, ref.SLIDING, rng, FS * np.sum(w * w), hop=16)
    _, _, want = signal.spectrogram(x, fs=FS, window=w, nperseg=64, noverlap=48, nfft=64, detrend=False, return_onesided=rng == ref.ONESIDED,
                                    scaling="density", mode="psd")
    close(ps, want)


def test_column_sliding_averaged_is_scipy_welch():
    x = np.random.default_rng(2).standard_normal((300, 3))
    w = signal.get_window("hamming", 64)
    fpc = (300 - 64) // 32 + 1
    _, ps, _, _, _ = ref.estimate(x.reshape(-1, order="F"), x.size, w, 128, fpc * 3, ref.COLUMN_SLIDING, ref.ONESIDED, FS * np.sum(w * w), hop=32, input_rows=300,
                                  fpc=fpc)
    got = ps.reshape((65, fpc, 3), order="F").mean(axis=1)
    _, want = signal.welch(x, fs=FS, window=w, nperseg=64, noverlap=32, nfft=128, detrend=False, return_onesided=True, scaling="density", axis=0)
    close(got, want)


def test_folded_columns_is_the_dtft_on_the_nfft_grid():
    g = np.random.default_rng(3)
    x = g.standard_normal((150, 4)) + 1j * g.standard_normal((150, 4))
    w = signal.get_window("blackman", 150)
    s, ps, _, _, _ = ref.estimate(x.reshape(-1, order="F"), x.size, w, 64, 4, ref.FOLDED_COLUMNS, ref.TWOSIDED, 3.0, input_rows=150)
    k, t = np.arange(64)[:, None], np.arange(150)[None, :]
    want = np.exp(-2j * np.pi * ((k * t) % 64) / 64) @ (x * w[:, None])
    close(s, want)
    close(ps, np.abs(want) ** 2 / 3.0)


@pytest.mark.parametrize("nfft, order", [(8, [5, 6, 7, 0, 1, 2, 3, 4]), (7, [4, 5, 6, 0, 1, 2, 3])])
def test_centered_rotation(nfft, order):
    assert ref.centered_shift(nfft) == order[0]
    x = np.random.default_rng(nfft).standard_normal(nfft + 3)
    w = np.ones(nfft)
    s, ps, _, f, _ = ref.estimate(x, x.size, w, nfft, 4, ref.SLIDING, ref.CENTERED, 1.0, hop=1)
    S = np.fft.fft(f, axis=0)
    assert s.shape == (nfft, 4) and np.array_equal(s, S[order])
    close(ps, np.abs(S[order]) ** 2)
