// provider_kats.cpp -- the reference's provider KATs written against the C++ host-side mirror
// (include/rmhip_provider.hpp).  Mirrors crates/runmat-runtime-integration-tests/tests/gpu.rs:28-60
// (plus / times on [1 2 3 4], [5 6 7 8]) and mtimes.rs:688-706 (column-major matmul round trip), plus one KAT per
// widened entry point (transpose view, syrk, linsolve, mldivide, stochastic_evolution, comparisons).
// Build: g++ -std=c++17 -Iinclude examples/provider_kats.cpp -Lrunmat_amd/csrc -lrmhip -Wl,-rpath,$PWD/runmat_amd/csrc
// Exit code 0 = all KATs pass; 2 = no gfx950 device (the provider has no CPU fallback); 1 = mismatch.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>

#include "rmhip_provider.hpp"

static bool eq(const std::vector<double>& a, std::initializer_list<double> b) {
    return a == std::vector<double>(b);
}

int main() {
    try {
        rmhip::HipProvider p(0);
        auto a = p.upload({1, 2, 3, 4}, {2, 2});
        auto b = p.upload({5, 6, 7, 8}, {2, 2});
        bool ok = eq(p.download(p.elem_add(a, b)).data, {6, 8, 10, 12});
        ok = ok && eq(p.download(p.elem_mul(a, b)).data, {5, 12, 21, 32});
        auto b2 = p.upload({5, 7, 6, 8}, {2, 2});
        ok = ok && eq(p.download(p.matmul(a, b2)).data, {26, 38, 30, 44});
        auto s = p.reduce_sum(a);
        ok = ok && s.shape == std::vector<size_t>({1, 1}) && eq(p.download(s).data, {10});
        try {  // inner dimension mismatch is a soft error (mtimes.rs:628-637)
            p.matmul(a, p.upload({1, 2, 3}, {3, 1}));
            ok = false;
        } catch (const rmhip::ProviderError& e) {
            ok = ok && e.code == RMHIP_ERR_SHAPE;
        }
        auto near = [](const std::vector<double>& v, std::initializer_list<double> w, double tol) {
            if (v.size() != w.size()) return false;
            size_t i = 0;
            for (double x : w)
                if (std::fabs(v[i++] - x) > tol) return false;
            return true;
        };
        // transpose view consumed in place: [1 3; 2 4]' * [5 6; 7 8]   (lib.rs:2532, matmul on a view)
        ok = ok && near(p.download(p.matmul(p.transpose(a), b2)).data, {19, 43, 22, 50}, 1e-12);
        ok = ok && eq(p.download(p.transpose(a)).data, {1, 3, 2, 4});
        // syrk: accelerate/tests/syrk.rs (A' * A), here on [1 3; 2 4]
        ok = ok && near(p.download(p.syrk(a)).data, {5, 11, 11, 25}, 1e-12);
        // cov(x, y) and cov(x, w) through the general entry point (cov.rs:901-1003): x = [1 2 4]', y = [2 1 5]', w = [1 2 1]'
        {
            auto cx = p.upload({1, 2, 4}, {3, 1}), cy = p.upload({2, 1, 5}, {3, 1}), cw = p.upload({1, 2, 1}, {3, 1});
            ok = ok && near(p.download(p.covariance_general(cx, &cy, nullptr, false)).data, {7.0 / 3, 8.0 / 3, 8.0 / 3, 13.0 / 3}, 1e-12);
            ok = ok && near(p.download(p.covariance_general(cx, nullptr, &cw, false)).data, {19.0 / 12}, 1e-12);
            ok = ok && p.download(p.covariance_general(cx, nullptr, nullptr, true)).data == p.download(p.covariance(cx, true)).data;
        }
        // linsolve LT hint: linsolve.rs:1224-1247
        rmhip_linsolve_options_t lt{};
        lt.lower = 1;
        lt.need_rcond = 1;
        auto sol = p.linsolve(p.upload({3, -1, 4, 0, 2, 1, 0, 0, 5}, {3, 3}), p.upload({9, 1, 19}, {3, 1}), lt);
        ok = ok && near(p.download(sol.solution).data, {3, 2, 1}, 1e-12) && sol.reciprocal_condition == 2.0 / 5.0;
        {
            // linsolve's second entry point: 2 I \ [1; 1] = [0.5; 0.5] with rcond 1, which linsolve itself declines once rcond is asked for
            rmhip_linsolve_options_t rq{};
            rq.need_rcond = 1;
            auto two_i = p.upload({2, 0, 0, 2}, {2, 2}), ones = p.upload({1, 1}, {2, 1});
            try {
                p.linsolve(two_i, ones, rq);
                ok = false;
            } catch (const rmhip::ProviderError& e) {
                ok = ok && e.code == RMHIP_ERR_UNSUPPORTED;
            }
            auto r = p.linsolve_rcond(two_i, ones, rq);
            ok = ok && eq(p.download(r.solution).data, {0.5, 0.5}) && r.reciprocal_condition == 1.0;
            // cond's second entry point on the reference's KATs (cond.rs:661-690): [4 -1; 2 3] is 15/7 in One and Inf, diag(5, 2) 2.9 in Fro
            auto m = p.upload({4, 2, -1, 3}, {2, 2});
            ok = ok && near(p.download(p.cond_norm(m, 1)).data, {15.0 / 7.0}, 1e-12) && near(p.download(p.cond_norm(m, 2)).data, {15.0 / 7.0}, 1e-12);
            ok = ok && near(p.download(p.cond_norm(p.upload({5, 0, 0, 2}, {2, 2}), 3)).data, {2.9}, 1e-12);
            ok = ok && std::isinf(p.download(p.cond_norm(p.upload({1, 2, 2, 4}, {2, 2}), 1)).data[0]);
        }
        // mldivide: mldivide.rs:662-680 ([1 2; 3 4] \ [5; 6] = [-4; 4.5])
        ok = ok && near(p.download(p.mldivide(p.upload({1, 3, 2, 4}, {2, 2}), p.upload({5, 6}, {2, 1}))).data, {-4, 4.5}, 1e-12);
        // stochastic_evolution with zero scale: accelerate/tests/stochastic_evolution.rs:17-47
        ok = ok && near(p.download(p.stochastic_evolution(p.upload({1, 2, 3}, {3, 1}), 0.05, 0.0, 4)).data,
                        {std::exp(0.2), 2 * std::exp(0.2), 3 * std::exp(0.2)}, 1e-9);
        // comparisons: 1.0 / 0.0 tensors
        ok = ok && eq(p.download(p.elem_lt(a, b)).data, {1, 1, 1, 1}) && eq(p.download(p.elem_eq(a, a)).data, {1, 1, 1, 1});
        // reduce_moments_nd (lib.rs:2770-2778): E[x] and E[x^2] of [1 3; 2 4] over the rows
        auto mom = p.reduce_moments_nd(a, {0});
        ok = ok && near(p.download(mom.first).data, {1.5, 3.5}, 1e-15) && near(p.download(mom.second).data, {2.5, 12.5}, 1e-15);
        {
            // the unfused implicit-expansion sequence of times.rs:501-543: repmat each operand, elem_mul, free the expansions
            auto col = p.upload({1, 2, 3, 4}, {4, 1});
            auto row = p.upload({10, 20, 30}, {1, 3});
            auto ce = p.repmat(col, {1, 3}), re = p.repmat(row, {4, 1});
            auto prod = p.elem_mul(ce, re);
            p.free(ce);
            p.free(re);
            ok = ok && prod.shape == std::vector<size_t>{4, 3} &&
                 eq(p.download(prod).data, {10, 20, 30, 40, 20, 40, 60, 80, 30, 60, 90, 120});
            // repmat.rs:1044-1060 repmat_gpu_roundtrip; permute.rs:784-792; linspace.rs:495-512; read_scalar / gather_linear
            ok = ok && eq(p.download(p.repmat(p.upload({1, 2}, {2, 1}), {2})).data, {1, 2, 1, 2, 1, 2, 1, 2});
            ok = ok && eq(p.download(p.permute(p.upload({1, 99, 3, 4}, {2, 2}), {1, 0})).data, {1, 3, 99, 4});
            ok = ok && near(p.download(p.linspace(0.0, 1.0, 5)).data, {0.0, 0.25, 0.5, 0.75, 1.0}, 1e-12);
            ok = ok && p.read_scalar(prod, 5) == 40.0 && eq(p.download(p.gather_linear(prod, {11, 0, 6}, {3, 1})).data, {120, 10, 60});
            ok = ok && eq(p.download(p.zeros_like(prod)).data, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
            const double nan = std::nan("");
            ok = ok && eq(p.download(p.map_nan_to_zero(p.upload({1, nan, 3}, {3, 1}))).data, {1, 0, 3}) &&
                 eq(p.download(p.not_nan_mask(p.upload({1, nan, 3}, {3, 1}))).data, {1, 0, 1});
        }
        {
            // uniform_spectral_estimate (lib.rs:2560-2565): two sliding frames of [1 2 3 4 5 6] under a unit window, nfft 4, hop 2, one-sided:
            // fft([1 2 3 4]) = [10, -2+2i, -2, ..], fft([3 4 5 6]) = [18, -2+2i, -2, ..]; ps = |s|^2 * (1, 2, 1) / 2
            rmhip::ProviderSpectralRequest q;
            q.input = p.upload({1, 2, 3, 4, 5, 6}, {6, 1});
            q.input_len = 6, q.window = {1, 1, 1, 1}, q.nfft = 4, q.frame_count = 2, q.denominator = 2.0;
            q.frame_mode.kind = rmhip::ProviderSpectralFrameMode::Sliding, q.frame_mode.hop = 2;
            auto sp = p.uniform_spectral_estimate(q);
            auto sv = p.download(sp.s);
            ok = ok && sp.rows == 3 && sp.cols == 2 && sv.complex_interleaved && sp.s.shape == std::vector<size_t>{3, 2} &&
                 near(sv.data, {10, 0, -2, 2, -2, 0, 18, 0, -2, 2, -2, 0}, 1e-14) && near(p.download(sp.ps).data, {50, 8, 2, 162, 8, 2}, 1e-13);
            q.frame_count = 3;  // the third frame would need x[4 .. 7]: refused by the coverage rule
            try {
                p.uniform_spectral_estimate(q);
                ok = false;
            } catch (const rmhip::ProviderError& e) {
                ok = ok && e.code == RMHIP_ERR_INVALID;
            }
        }
        {
            // signal_envelope (lib.rs:2566-2571): rms over a centred window of 3 on [0 3 4 0] (envelope.rs rms_envelope_uses_centered_window),
            // the analytic envelope of the alternating [1 0 -1 0] (|z| = 1 everywhere, mean 0), and a NaN sample refused as INVALID
            rmhip::ProviderEnvelopeRequest q;
            q.input = p.upload({0, 3, 4, 0}, {4, 1});
            q.channel_len = 4, q.channel_count = 1, q.output_shape = {4, 1};
            q.method.kind = rmhip::ProviderEnvelopeMethod::Rms, q.method.param = 3;
            auto env = p.signal_envelope(q);
            const double r = std::sqrt(25.0 / 3.0);
            ok = ok && env.upper.shape == std::vector<size_t>{4, 1} && near(p.download(env.upper).data, {std::sqrt(4.5), r, r, std::sqrt(8.0)}, 1e-15) &&
                 near(p.download(env.lower).data, {-std::sqrt(4.5), -r, -r, -std::sqrt(8.0)}, 1e-15);
            q.input = p.upload({1, 0, -1, 0}, {4, 1});
            q.method.kind = rmhip::ProviderEnvelopeMethod::Analytic;
            env = p.signal_envelope(q);
            ok = ok && near(p.download(env.upper).data, {1, 1, 1, 1}, 1e-14) && near(p.download(env.lower).data, {-1, -1, -1, -1}, 1e-14);
            q.input = p.upload({1, std::nan(""), -1, 0}, {4, 1});
            try {
                p.signal_envelope(q);
                ok = false;
            } catch (const rmhip::ProviderError& e) {
                ok = ok && e.code == RMHIP_ERR_INVALID;
            }
        }
        {
            // mode_values (lib.rs:2846-2851): the tie of [1 1 2 2] (mode.rs:901-923 mode_ties_return_smallest_with_sorted_set): M = 1, F = 2, C = {[1; 2]}
            rmhip::ProviderModeRequest q;
            q.input = p.upload({1, 1, 2, 2}, {1, 4});
            q.want_frequency = q.want_ties = true;
            auto mo = p.mode_values(q);
            ok = ok && mo.values.shape == std::vector<size_t>{1, 1} && eq(p.download(mo.values).data, {1}) && eq(p.download(mo.frequencies).data, {2}) &&
                 mo.ties.values.shape == std::vector<size_t>{2, 1} && eq(mo.ties.values.data, {1, 2}) && mo.ties.offsets == std::vector<size_t>{0} &&
                 mo.ties.counts == std::vector<size_t>{2};
        }
        {
            // modulate_constellation / modulate_bits_constellation (lib.rs:1961-1977): the Gray 4-QAM table of qammod.rs:675-682 over the symbols
            // [0 1 2 3] and over the bit columns [0 0; 1 1] of qammod.rs:782-791 (one symbol per column), and a symbol of 4 refused as INVALID
            rmhip::ProviderModulationRequest q;
            q.constellation = {-1, 1, -1, -1, 1, 1, 1, -1};
            q.input = p.upload({0, 1, 2, 3}, {1, 4});
            auto pts = p.modulate_constellation(q);
            ok = ok && pts.shape == std::vector<size_t>{1, 4} && p.is_complex(pts) && eq(p.download(pts).data, {-1, 1, -1, -1, 1, 1, 1, -1});
            rmhip::ProviderBitModulationRequest b;
            b.constellation = q.constellation;
            b.input = p.upload({0, 0, 1, 1}, {2, 2});
            b.input_rows = 2, b.bits_per_symbol = 2;
            auto sym = p.modulate_bits_constellation(b);
            ok = ok && sym.shape == std::vector<size_t>{1, 2} && p.is_complex(sym) && eq(p.download(sym).data, {-1, 1, 1, -1});
            q.input = p.upload({0, 4}, {1, 2});
            try {
                p.modulate_constellation(q);
                ok = false;
            } catch (const rmhip::ProviderError& e) {
                ok = ok && e.code == RMHIP_ERR_INVALID && std::string(e.what()).find("symbols must be in range") != std::string::npos;
            }
        }
        {
            // pagefun's second entry point on a hand-computed Gaussian-integer product: [1+i 2; -i 3+2i] * [1-i; 2+i] = [6+2i; 3+6i], and times
            // the real column [1; 2] = [5+i; 6+3i]; pagefun itself declines a complex input
            rmhip::PagefunRequest q;
            auto za = p.complex_from_real_imag(p.upload({1, 0, 2, 3}, {2, 2}), p.upload({1, -1, 0, 2}, {2, 2}));
            auto br = p.upload({1, 2}, {2, 1});
            auto zb = p.complex_from_real_imag(br, p.upload({-1, 1}, {2, 1}));
            q.inputs = {za, zb};
            q.output_shape = {2, 1};
            q.input_page_dims = {{}, {}};
            try {
                p.pagefun(q);
                ok = false;
            } catch (const rmhip::ProviderError& e) {
                ok = ok && e.code == RMHIP_ERR_UNSUPPORTED;
            }
            auto zc = p.complex_pagefun(q);
            ok = ok && zc.shape == std::vector<size_t>{2, 1} && p.is_complex(zc) && eq(p.download(zc).data, {6, 2, 3, 6});
            q.inputs[1] = br;
            ok = ok && eq(p.download(p.complex_pagefun(q)).data, {5, 1, 6, 3});
            // matmul's second entry point on the same operands, and the real column on the left of the complex row [1+i 2]
            try {
                p.matmul(za, br);
                ok = false;
            } catch (const rmhip::ProviderError& e) {
                ok = ok && e.code == RMHIP_ERR_UNSUPPORTED;
            }
            auto zm = p.complex_matmul(za, zb);
            ok = ok && zm.shape == std::vector<size_t>{2, 1} && p.is_complex(zm) && eq(p.download(zm).data, {6, 2, 3, 6});
            ok = ok && eq(p.download(p.complex_matmul(za, br)).data, {5, 1, 6, 3});
            auto zrow = p.complex_from_real_imag(p.upload({1, 2}, {1, 2}), p.upload({1, 0}, {1, 2}));
            ok = ok && eq(p.download(p.complex_matmul(br, zrow)).data, {1, 1, 2, 2, 2, 0, 4, 0});
            // the solves' second entry points undo the product: A \ (A * b) = b, inv(A) * (A * b) = b, and (b.' * A.') / A.' = b.'
            try {
                p.mldivide(za, zm);
                ok = false;
            } catch (const rmhip::ProviderError& e) {
                ok = ok && e.code == RMHIP_ERR_UNSUPPORTED;
            }
            auto zs = p.complex_mldivide(za, zm);
            ok = ok && zs.shape == std::vector<size_t>{2, 1} && p.is_complex(zs) && near(p.download(zs).data, {1, -1, 2, 1}, 1e-12);
            ok = ok && near(p.download(p.complex_matmul(p.complex_inv(za), zm)).data, {1, -1, 2, 1}, 1e-12);
            auto zat = p.complex_from_real_imag(p.upload({1, 2, 0, 3}, {2, 2}), p.upload({1, 0, -1, 2}, {2, 2}));  // A.'
            auto zmt = p.complex_from_real_imag(p.upload({6, 3}, {1, 2}), p.upload({2, 6}, {1, 2}));                // (A * b).'
            auto zr = p.complex_mrdivide(zmt, zat);
            ok = ok && zr.shape == std::vector<size_t>{1, 2} && near(p.download(zr).data, {1, -1, 2, 1}, 1e-12);
        }
        {
            // moving_window's second entry point: the 101-point median (shrinking at the ends) of the ramp 0 .. 199 with a spike at 100, which
            // moving_window itself declines; against the middle of each sorted window
            std::vector<double> ramp(200);
            for (size_t i = 0; i < ramp.size(); ++i) ramp[i] = (double)i;
            ramp[100] = 1e6;
            auto h = p.upload(ramp, {200, 1});
            try {
                p.moving_window(h, {200, 1}, 0, 50, 50, 5, 0, 0.0, false, false);
                ok = false;
            } catch (const rmhip::ProviderError& e) {
                ok = ok && e.code == RMHIP_ERR_UNSUPPORTED;
            }
            auto med = p.download(p.moving_window_long(h, {200, 1}, 0, 50, 50, 5, 0, 0.0, false, false)).data;
            ok = ok && med.size() == ramp.size();
            for (size_t i = 0; ok && i < ramp.size(); ++i) {
                std::vector<double> w(ramp.begin() + (i < 50 ? 0 : i - 50), ramp.begin() + (i + 51 > ramp.size() ? ramp.size() : i + 51));
                std::sort(w.begin(), w.end());
                const size_t mid = w.size() / 2;
                ok = med[i] == (w.size() % 2 ? w[mid] : (w[mid - 1] + w[mid]) / 2.0);
            }
        }
        {
            // chol's second entry point on the reference's chol_gpu_failure_flag (chol.rs:1008-1021): [1 2; 2 1] fails its second pivot, so
            // info = 2 and the factor keeps row 1, [1 2; 0 0] (column-major below) - lower: its transpose; chol itself declines the matrix
            auto h = p.upload({1, 2, 2, 1}, {2, 2});
            try {
                p.chol(h, false);
                ok = false;
            } catch (const rmhip::ProviderError& e) {
                ok = ok && e.code == RMHIP_ERR_UNSUPPORTED;
            }
            auto up = p.chol_info(h, false), low = p.chol_info(h, true);
            ok = ok && up.info == 2 && eq(p.download(up.factor).data, {1, 0, 2, 0}) && low.info == 2 && eq(p.download(low.factor).data, {1, 2, 0, 0});
            auto spd = p.chol_info(p.upload({4, 12, -16, 12, 37, -43, -16, -43, 98}, {3, 3}), false);
            ok = ok && spd.info == 0 && eq(p.download(spd.factor).data, {2, 0, 0, 6, 1, 0, -8, 5, 3});
        }
        {
            // ProviderPrecision::F32 (lib.rs:815-818): host views stay f64, storage is f32, results round once
            rmhip::HipProvider q(0, 32);
            ok = ok && std::string(q.precision()) == "F32";
            auto x = q.upload({0.1, 0.2, 0.3, 16777217.0}, {2, 2});
            ok = ok && eq(q.download(x).data, {(double)0.1f, (double)0.2f, (double)0.3f, 16777216.0});
            auto y = q.elem_add(x, x);  // f64 arithmetic on the f32 values, one rounding
            ok = ok && eq(q.download(y).data, {(double)(float)(2.0 * (double)0.1f), (double)(float)(2.0 * (double)0.2f),
                                               (double)(float)(2.0 * (double)0.3f), 33554432.0});
            auto ai = q.upload({1, 2, 3, 4}, {2, 2});
            auto bi = q.upload({5, 7, 6, 8}, {2, 2});
            ok = ok && eq(q.download(q.matmul(ai, bi)).data, {26, 38, 30, 44});  // f32 matrix cores: integers stay exact
        }
        std::printf(ok ? "provider KATs ok\n" : "provider KATs FAILED\n");
        return ok ? 0 : 1;
    } catch (const rmhip::ProviderError& e) {
        std::fprintf(stderr, "provider unavailable: %s\n", e.what());
        return e.code == RMHIP_ERR_NO_DEVICE ? 2 : 1;
    }
}
