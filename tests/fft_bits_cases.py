"""The fixed case list behind tests/golden/fft_bits.json: one smallest shape per route of fft.hip, each result's downloaded bytes as a
SHA-256 digest.  scripts/record_fft_bits.py runs `digests` against the library of a reference revision, tests/test_gpu_fft_bits.py
against the tree: kernels and launch parameters that do not change, on paths without atomics, give the same bits.

Inputs are an integer hash formed in numpy - ((k * 2654435761) mod 2^32) / 2^32 - 0.5 - with no RNG involved."""
import hashlib

import numpy as np

import fft_ref as R
import spectral_ref as S


def values(count, offset=0):
    k = (np.arange(count, dtype=np.uint64) + np.uint64(offset)) * np.uint64(2654435761) % np.uint64(1 << 32)
    return k.astype(np.float64) / float(1 << 32) - 0.5


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def upload(p, shape, cplx=False):
    n = int(np.prod(shape))
    re = p.upload(values(n), shape)
    if not cplx:
        return re
    im = p.upload(values(n, 1 << 20), shape)
    z = p.complex_from_real_imag(re, im)
    p.free(re)
    p.free(im)
    return z


def transform(shape, dim=0, length=None, inverse=False, cplx=False):
    def run(p):
        h = upload(p, shape, cplx)
        out = (p.ifft_dim if inverse else p.fft_dim)(h, length, dim)
        got = p.download(out)
        p.free(out)
        p.free(h)
        return sha(got)
    return run


def sampled_transform(shape, boundaries):
    """A result too large to download whole: the real and imaginary parts of fft_ref.bins_to_check's structured sample, read through gather_linear."""
    def run(p):
        h = upload(p, shape)
        out = p.fft_dim(h, None, 0)
        idx = R.bins_to_check(shape[0], boundaries, seed=11)
        parts = []
        for op in ("real", "imag"):
            plane = p.complex_unary(op, out)
            g = p.gather_linear(plane, idx, (idx.size, 1))
            parts.append(p.download(g))
            p.free(g)
            p.free(plane)
        p.free(out)
        p.free(h)
        return sha(*parts)
    return run


def hilbert(shape, dim):
    def run(p):
        h = upload(p, shape)
        out = p.signal_hilbert(h, None, dim)
        got = p.download(out)
        p.free(out)
        p.free(h)
        return sha(got)
    return run


def spectral(mode, numel, window_len, nfft, frames, rng, hop=0, input_rows=0, fpc=0):
    def run(p):
        from runmat_amd import ProviderSpectralFrameMode as M, ProviderSpectralRequest
        fm = {S.SLIDING: lambda: M.Sliding(hop), S.COLUMN_SLIDING: lambda: M.ColumnSliding(hop, input_rows, fpc), S.FOLDED_COLUMNS: lambda: M.FoldedColumns(input_rows)}[mode]()
        w = values(window_len, 77) + 1.0
        h = upload(p, (numel, 1))
        res = p.uniform_spectral_estimate(ProviderSpectralRequest(h, numel, False, w, nfft, frames, fm, rng, 2.0 * float(np.sum(w * w))))
        s, ps = p.download(res.s), p.download(res.ps)
        for t in (res.s, res.ps, h):
            p.free(t)
        return sha(s, ps)
    return run


# (id, precision, run)
CASES = []
for lg in (1, 3, 11, 12, 13):  # mode 0; lg 11, 12, 13 are the three thread counts
    CASES.append((f"tile0-lg{lg}", "F64", transform((1 << lg,))))
    CASES.append((f"tile0-lg{lg}x3", "F64", transform((1 << lg, 3))))
CASES += [
    ("tile1-5x32", "F64", transform((5, 32), 1)),
    ("tile1-257x4", "F64", transform((257, 4), 1)),
    ("two0-16384", "F64", transform((16384,))),
    ("two1-3x512", "F64", transform((3, 512), 1)),
    ("three-lg23", "F64", sampled_transform((1 << 23,), (1 << 7, 1 << 15))),
    ("chirp-n7", "F64", transform((7,))),
    ("chirp-6x100", "F64", transform((6, 100), 1)),
    ("chirp-n4097", "F64", transform((4097,))),
    ("padded-100to128", "F64", transform((100,), 0, 128)),
    ("truncated-100to64", "F64", transform((100,), 0, 64)),
    ("padded-two0", "F64", transform(((1 << 14) + 5, 2), 0, 1 << 15)),
    ("truncated-two1", "F64", transform((3, 600), 1, 512)),
    ("padded-chirp", "F64", transform((1000,), 0, 1500)),
    ("inverse-4096", "F64", transform((4096,), inverse=True, cplx=True)),
    ("inverse-16384", "F64", transform((16384,), inverse=True, cplx=True)),
    ("inverse-chirp-6x100", "F64", transform((6, 100), 1, inverse=True, cplx=True)),
    ("complex-2048x3", "F64", transform((2048, 3), cplx=True)),
    ("complex-two1-3x512", "F64", transform((3, 512), 1, cplx=True)),
    ("f32-1024x3", "F32", transform((1024, 3))),
    ("f32-inverse-chirp-100", "F32", transform((100,), inverse=True, cplx=True)),
    ("hilbert-1000x2", "F64", hilbert((1000, 2), 0)),
    ("spectral-fused-sliding", "F64", spectral(S.SLIDING, 1000, 64, 64, 59, S.ONESIDED, hop=16)),
    ("spectral-fused-columns", "F64", spectral(S.COLUMN_SLIDING, 900, 64, 128, 20, S.CENTERED, hop=32, input_rows=300, fpc=8)),
    ("spectral-framed-folded", "F64", spectral(S.FOLDED_COLUMNS, 600, 150, 64, 4, S.TWOSIDED, input_rows=150)),
    ("spectral-framed-n100", "F64", spectral(S.SLIDING, 600, 100, 100, 14, S.ONESIDED, hop=37)),
]


def digests(provider_of):
    """{id: digest}; `provider_of(precision)` hands out the provider of "F64" / "F32"."""
    return {cid: run(provider_of(precision)) for cid, precision, run in CASES}
