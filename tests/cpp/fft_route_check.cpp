// Host-logic check of the transforms' dispatch (runmat_amd/csrc/fft_plan.h), the functions fft.hip's drivers execute.  No GPU needed.
//   --table       reads one transform per line from stdin - "dim length rank d0 d1 ..." (length -1: the extent) - and prints its path family
//                 and steady-state launch count, "family launches ..." (tests/test_fft_paths_host.py feeds it the cases of
//                 tests/test_gpu_fft_paths.py).  Families: tile0 tile1 two0 two1 three chirp chirp3 onepoint zerofill refused.
//   --sweep       plans a fixed sweep - every power-of-two length at five inners, tiles at every line-count boundary, the entry's own
//                 routes, Bluestein's sizes around every boundary of M and both refusals, the length predicate, the spectral decision -
//                 and prints per group the number of cases and the 64-bit FNV-1a digest of the routes' text; tests/test_host_plan.py
//                 compares with tests/golden/fft_routes.txt, which was taken from the drivers' conditions before the plan was extracted.
//   --dump        the sweep with every route printed under its group's line.
//   --invariants  every tile of the sweep against the kernel's limits: points <= 8 x threads, LDS <= 160 KiB, blocks x lines >= nlines,
//                 radices that multiply to m with the twiddle-free one first.
//   --model       runs every pass of a route on the host, on impulse inputs, with values kept as exponents of w_n (integers mod n) or as
//                 zero - an impulse stays an impulse or a pure root of unity through every pass, so the check is exact - and compares
//                 the output with the transform's definition, exponent for exponent; also: every output element written once, every
//                 work element read after the pass before wrote it, an in-place pass's lines writing what they read, nothing out of bounds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fft_plan.h"

using namespace rmhip::fft_plan;

static const u64 SPEC_FRAMES = 10, SPEC_FPC = 4, SPEC_HOP = 3, SPEC_ROWS = 50;  // the framing of the sweep's spectral cases

static bool g_invariants = false;
static unsigned long g_tiles = 0;
static std::string g_broken;

static void tile_invariants(int log2m, u64 nlines, const TilePlan& t) {
    ++g_tiles;
    const u64 points = 1ull << (log2m + t.log2b);
    u64 prod = 1;
    bool order = true;
    for (int k = 0; k < t.nrad; ++k) prod *= (u64)t.rad[k], order = order && (k == 0 || t.rad[k] == 8);
    const bool ok = points <= 8ull * (u64)t.threads && t.lds <= 160u * 1024u && (t.blocks << t.log2b) >= nlines && prod == (1ull << log2m) && order;
    if (!ok && g_broken.empty()) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "tile lg=%d lines=%llu: lb=%d threads=%d lds=%zu blocks=%llu", log2m, nlines, t.log2b, t.threads, t.lds, t.blocks);
        g_broken = buf;
    }
}

std::string tile_line(int log2m, int mode, u64 nlines) {
    const TilePlan t = plan_tile(log2m, mode, nlines);
    if (g_invariants) tile_invariants(log2m, nlines, t);
    if (t.refused) return "refused lines";
    char buf[160];
    int at = std::snprintf(buf, sizeof buf, "lb=%d thr=%d lds=%zu blocks=%llu rad=", t.log2b, t.threads, t.lds, t.blocks);
    for (int k = 0; k < t.nrad; ++k) at += std::snprintf(buf + at, sizeof buf - at, "%s%d", k ? "," : "", t.rad[k]);
    return buf;
}

static std::string pass_text(const PassGeom& g) {
    char buf[400];
    std::snprintf(buf, sizeof buf, "lines=%llu inner=%llu q=%llu a=%llu,%llu,%llu,%llu b=%llu,%llu,%llu,%llu pk=%llu qk=%llu len=%llu lg=%d mode=%d byi=%d src=%d dst=%d step=%d first=%d last=%d | ",
                  g.nlines, g.inner, g.qcnt, g.a.si, g.a.sq, g.a.so, g.a.sp, g.b.si, g.b.sq, g.b.so, g.b.sp, g.in_pk, g.in_qk, g.in_len, g.log2m, g.mode, g.step_by_i,
                  (int)g.src, (int)g.dst, (int)g.step, g.first ? 1 : 0, g.last ? 1 : 0);
    return buf + tile_line(g.log2m, g.mode, g.nlines);
}

std::string pow2_line(const LineShape& L, u64 n, u64 valid) {
    const Pow2Route r = plan_pow2(L, n, valid);
    if (r.npass == 0) return "refused length\n";
    char buf[80];
    std::snprintf(buf, sizeof buf, "passes=%d work=%llu tables=", r.npass, r.work);
    std::string s = buf;
    for (int k = 0; k < r.ntables; ++k) {
        std::snprintf(buf, sizeof buf, "%s%d:%llu:%llu", k ? "," : "", r.tables[k].kind, r.tables[k].n, r.tables[k].count);
        s += buf;
    }
    s += "\n";
    for (int k = 0; k < r.npass; ++k) s += "  " + pass_text(r.pass[k]) + "\n";
    return s;
}

std::string entry_line(const LineShape& L, u64 n) {
    switch (plan_entry(L.len_in, n)) {
        case ENTRY_ZERO_FILL: return "zero_fill\n";
        case ENTRY_ONE_POINT: return "one_point " + pass_text(one_point_pass(L)) + "\n";
        case ENTRY_POW2: return "pow2\n";
        default: return "chirp\n";
    }
}

std::string chirp_line(const LineShape& L, u64 n) {
    const ChirpPlan p = plan_chirp(L, n);
    char buf[240];
    if (p.refused == CHIRP_LENGTH) std::snprintf(buf, sizeof buf, "refused length M=%llu\n", p.M);
    else if (p.refused == CHIRP_SLAB) std::snprintf(buf, sizeof buf, "refused slab M=%llu\n", p.M);
    else {
        const Slab a = chirp_slab(p, L.outer, 0), z = chirp_slab(p, L.outer, p.nslabs - 1);
        std::snprintf(buf, sizeof buf, "M=%llu slab=%llu per=%llu nslabs=%llu valid=%llu first=%llu:%llu last=%llu:%llu\n", p.M, p.slab, p.outer_per, p.nslabs, p.valid, a.o0,
                      a.oc, z.o0, z.oc);
    }
    return buf;
}

std::string served_line(u64 n, u64 inner) { return length_served(n, inner) ? "served=1\n" : "served=0\n"; }

std::string spectral_line(int mode, int range, u64 nfft, u64 window_len, u64 top, u64 input_len) {
    const u64 wl = spectral_window_points(mode, window_len, nfft);
    const SpectralPlan s = plan_spectral(mode, range, nfft, top, input_len);
    char buf[200];
    std::snprintf(buf, sizeof buf, "wl=%llu fused=%d own=%d direct=%d frames=%d spec=%d rows=%llu shift=%llu\n", wl, s.fused ? 1 : 0, s.own_spectrum ? 1 : 0, s.direct ? 1 : 0,
                  s.alloc_frames ? 1 : 0, s.alloc_spec ? 1 : 0, s.rows, s.shift);
    std::string out = buf;
    if (s.fused) out += "  " + pass_text(spectral_frame_pass(mode, SPEC_FRAMES, SPEC_FPC, SPEC_HOP, SPEC_ROWS, nfft, wl)) + "\n";
    return out;
}

// ---- the sweep -------------------------------------------------------------------------------------------------------------------------------
static bool g_quiet = false;  // --invariants walks the sweep for its tiles, not for its lines

struct Group {
    std::string name, all;
    uint64_t h = 1469598103934665603ull;
    unsigned long count = 0;
    bool dump;
    Group(const std::string& n, bool d) : name(n), dump(d) {}
    void add(const std::string& what, const std::string& line) {
        for (unsigned char ch : line) h = (h ^ ch) * 1099511628211ull;
        ++count;
        if (dump) all += "  " + what + ": " + line;
    }
    ~Group() {
        if (g_quiet) return;
        std::printf("%s %lu %016llx\n", name.c_str(), count, (unsigned long long)h);
        std::fputs(all.c_str(), stdout);
    }
};

static std::string fmt(const char* f, u64 a = 0, u64 b = 0, u64 c = 0, u64 d = 0) {
    char buf[160];
    std::snprintf(buf, sizeof buf, f, a, b, c, d);
    return buf;
}

static void sweep(bool dump) {
    static const u64 INNERS[] = {1, 2, 5, 257, 4096}, OUTERS[] = {1, 3};
    // every power-of-two length: lg 0..28 at each inner and outer, the input shorter, equal, longer and one point; `valid` unset and n / 2
    for (u64 inner : INNERS)
        for (u64 outer : OUTERS) {
            Group g(fmt("pow2 inner=%llu outer=%llu", inner, outer), dump);
            for (int lg = 0; lg <= 28; ++lg) {
                const u64 n = 1ull << lg;
                for (u64 len_in : {n, n > 3 ? n - 3 : 1, n + 5, (u64)1})
                    for (u64 valid : {~0ull, n / 2}) g.add(fmt("lg=%llu len_in=%llu valid=%llu", lg, len_in, valid), pow2_line(LineShape{inner, outer, len_in}, n, valid));
            }
        }
    // tiles: every line length a tile holds, line counts around every power of two up to past MAXB and around the grid limit
    for (int mode = 0; mode <= 2; ++mode) {
        Group g(fmt("tile mode=%llu", mode), dump);
        for (int lg = 0; lg <= 13; ++lg) {
            std::vector<u64> lines;
            for (int b = 0; b <= 10; ++b)
                for (u64 v : {(1ull << b) - 1, 1ull << b, (1ull << b) + 1})
                    if (v) lines.push_back(v);
            for (int b = 0; b <= 8; ++b)
                for (u64 v : {(0x7fffffffull << b) - 1, 0x7fffffffull << b, (0x7fffffffull << b) + 1}) lines.push_back(v);
            for (u64 v : lines) g.add(fmt("lg=%llu lines=%llu", lg, v), tile_line(lg, mode, v) + "\n");
        }
    }
    {
        Group g("entry", dump);
        for (u64 inner : {1, 5})
            for (u64 outer : {1, 3})
                for (u64 cur : {0, 1, 2, 7, 8})
                    for (u64 n : {1, 2, 7, 8}) g.add(fmt("inner=%llu outer=%llu cur=%llu n=%llu", inner, outer, cur, n), entry_line(LineShape{inner, outer, cur}, n));
    }
    // Bluestein: lengths around every boundary of M (2n - 1 = 2^k), both refusals, slabs around 2^27 and work tensors around 2^26
    {
        std::vector<u64> ns = {3, 5, 6, 7, 100, 1000};
        for (int k = 2; k <= 25; ++k)
            for (u64 v : {(1ull << (k - 1)) - 1, (1ull << (k - 1)) + 1, (1ull << (k - 1)) + 2, 3ull << (k - 2)})
                if (v >= 3 && !is_pow2(v)) ns.push_back(v);
        static const u64 CH_INNERS[] = {1, 2, 5, 257, 4096, 8192, (1ull << 22) - 1, 1ull << 22, (1ull << 22) + 1, (1ull << 23) - 1, 1ull << 23, (1ull << 23) + 1, (1ull << 24) - 1, 1ull << 24, (1ull << 24) + 1};
        for (u64 outer : {(u64)1, (u64)3, (u64)1030, 1ull << 20}) {
            Group g(fmt("chirp outer=%llu", outer), dump);
            for (u64 inner : CH_INNERS)
                for (u64 n : ns)
                    for (u64 len_in : {n, n - 2, n + 5, (u64)1}) g.add(fmt("inner=%llu n=%llu len_in=%llu", inner, n, len_in), chirp_line(LineShape{inner, outer, len_in}, n));
        }
    }
    {
        Group g("served", dump);
        std::vector<u64> ns;
        for (int k : {7, 8, 9, 13, 14, 22, 23, 24, 25, 26, 27, 28})
            for (u64 v : {(1ull << k) - 1, 1ull << k, (1ull << k) + 1}) ns.push_back(v);
        for (u64 inner : {(u64)1, (u64)2, (u64)5, (u64)8, (u64)9, (u64)4096})
            for (u64 n : ns) g.add(fmt("n=%llu inner=%llu", n, inner), served_line(n, inner));
    }
    // the spectral decision: three frame modes x three ranges, frames inside, touching and past input_len
    for (int mode = 0; mode <= 2; ++mode)
        for (int range = 0; range <= 2; ++range) {
            Group g(fmt("spectral mode=%llu range=%llu", mode, range), dump);
            for (u64 nfft : {(u64)1, (u64)2, (u64)8, (u64)100, (u64)4096, (u64)8191, (u64)8192, (u64)8193, (u64)16384, (u64)10007})
                for (u64 window_len : {(u64)1, nfft, nfft + 22, nfft / 2 + 1})
                    for (u64 top : {(u64)99999, (u64)100000, (u64)100001})
                        g.add(fmt("nfft=%llu window=%llu top=%llu", nfft, window_len, top), spectral_line(mode, range, nfft, window_len, top, 100000));
        }
}

// ---- --table ---------------------------------------------------------------------------------------------------------------------------------
static int table_mode() {
    char text[512];
    while (std::fgets(text, sizeof text, stdin)) {
        int dim, rank, used = 0;
        long long length;
        if (std::sscanf(text, "%d %lld %d%n", &dim, &length, &rank, &used) != 3 || dim < 0 || rank < 1) {
            std::fprintf(stderr, "bad case line: %s", text);
            return 2;
        }
        std::vector<u64> shape;
        const char* at = text + used;
        for (int k = 0; k < rank; ++k) {
            unsigned long long d;
            int step = 0;
            if (std::sscanf(at, "%llu%n", &d, &step) != 1) return 2;
            shape.push_back(d), at += step;
        }
        while (shape.size() <= (size_t)dim) shape.push_back(1);  // as fft_entry reads a shape
        LineShape L{1, 1, shape[dim]};
        for (int k = 0; k < dim; ++k) L.inner *= shape[k];
        for (size_t k = dim + 1; k < shape.size(); ++k) L.outer *= shape[k];
        const u64 n = length < 0 ? L.len_in : (u64)length;
        switch (plan_entry(L.len_in, n)) {
            case ENTRY_ZERO_FILL: std::printf("zerofill 0\n"); break;
            case ENTRY_ONE_POINT: std::printf("onepoint 1\n"); break;
            case ENTRY_POW2: {
                const Pow2Route r = plan_pow2(L, n);
                static const char* const names[4][2] = {{"refused", "refused"}, {"tile0", "tile1"}, {"two0", "two1"}, {"three", "three"}};
                std::printf("%s %d\n", names[r.npass][L.inner > 1], r.npass);
                break;
            }
            case ENTRY_CHIRP: {
                // steady state, as the case table counts: the chirp and G are cached; per slab two length-M transforms, k_line_mul, k_bluestein_finish
                const ChirpPlan p = plan_chirp(L, n);
                const int passes = p.refused ? 0 : pow2_passes(L.inner, ilog2(p.M));
                if (!passes) std::printf("refused 0\n");
                else std::printf("%s %llu passes=%d M=%llu slabs=%llu\n", passes == 3 ? "chirp3" : "chirp", p.nslabs * (2 * passes + 2), passes, p.M, p.nslabs);
                break;
            }
        }
    }
    return 0;
}

// ---- --model ---------------------------------------------------------------------------------------------------------------------------------
struct Nz {  // a nonzero element: w_n^e at `addr`
    u64 addr, e;
};

struct Model {
    u64 n = 1;  // values are exponents mod n
    std::vector<PassGeom> passes;
    u64 step_len[3] = {0, 0, 0};  // by StepTable
    u64 in_size = 0, work_size = 0, out_size = 0;
    std::string name, error;
    // per pass: the (line, point) pairs that read a source element, as lists per address
    std::vector<std::vector<std::vector<std::pair<u64, u64>>>> readers;

    u64 src_size(const PassGeom& g) const { return g.src == FROM_INPUT ? in_size : work_size; }
    u64 dst_size(const PassGeom& g) const { return g.dst == TO_WORK ? work_size : out_size; }
    static void split(const PassGeom& g, u64 l, u64* i, u64* q, u64* o) { *i = l % g.inner, *q = (l / g.inner) % g.qcnt, *o = l / (g.inner * g.qcnt); }
    bool fail(const std::string& what) {
        if (error.empty()) error = name + ": " + what;
        return false;
    }

    // the addressing alone: bounds, each destination element written once, work elements read after the pass before wrote them, in-place lines
    bool geometry() {
        std::vector<int> work_stamp(work_size, -1);
        readers.assign(passes.size(), {});
        for (size_t p = 0; p < passes.size(); ++p) {
            const PassGeom& g = passes[p];
            const u64 m = 1ull << g.log2m;
            const bool in_place = g.src == FROM_WORK && g.dst == TO_WORK;
            readers[p].assign(src_size(g), {});
            std::vector<int> written(dst_size(g), 0);
            for (u64 l = 0; l < g.nlines; ++l) {
                u64 i, q, o;
                split(g, l, &i, &q, &o);
                std::vector<u64> rd, wr;
                for (u64 pt = 0; pt < m; ++pt) {
                    if (pt * g.in_pk + q * g.in_qk < g.in_len) {
                        const u64 at = i * g.a.si + q * g.a.sq + o * g.a.so + pt * g.a.sp;
                        if (at >= src_size(g)) return fail(fmt("pass %llu line %llu point %llu reads past its buffer", p, l, pt));
                        if (g.src == FROM_WORK && work_stamp[at] != (int)p - 1) return fail(fmt("pass %llu line %llu point %llu reads a work element the pass before did not write", p, l, pt));
                        readers[p][at].push_back({l, pt});
                        rd.push_back(at);
                    }
                    const u64 to = i * g.b.si + q * g.b.sq + o * g.b.so + pt * g.b.sp;
                    if (to >= dst_size(g)) return fail(fmt("pass %llu line %llu result %llu is written past its buffer", p, l, pt));
                    ++written[to];
                    wr.push_back(to);
                }
                if (in_place) {
                    std::sort(rd.begin(), rd.end()), std::sort(wr.begin(), wr.end());
                    if (rd != wr) return fail(fmt("pass %llu line %llu is in place and does not write the elements it read", p, l));
                }
            }
            for (u64 e = 0; e < written.size(); ++e)
                if (written[e] != 1) return fail(fmt("pass %llu writes element %llu %llu times", p, e, written[e]));
            if (g.dst == TO_WORK) std::fill(work_stamp.begin(), work_stamp.end(), (int)p);
        }
        return true;
    }

    // an impulse w_n^c at input element `at` through every pass; `gtab` (or null): mul_in[pos] = w_n^gtab[pos]
    bool run(u64 at, u64 c, bool conj_in, bool conj_out, const std::vector<u64>* gtab, std::vector<Nz>* out) {
        std::vector<Nz> cur = {Nz{at, c % n}}, next;
        std::vector<std::pair<u64, Nz>> hit;  // line -> (point, value)
        for (size_t p = 0; p < passes.size(); ++p) {
            const PassGeom& g = passes[p];
            const u64 m = 1ull << g.log2m;
            hit.clear();
            for (const Nz& s : cur)
                for (const auto& lp : readers[p][s.addr]) hit.push_back({lp.first, Nz{lp.second, s.e}});
            std::sort(hit.begin(), hit.end(), [](const std::pair<u64, Nz>& a, const std::pair<u64, Nz>& b) { return a.first < b.first; });
            next.clear();
            for (size_t h = 0; h < hit.size(); ++h) {
                if (h && hit[h - 1].first == hit[h].first) return fail(fmt("pass %llu line %llu holds two nonzero points: not an impulse", p, hit[h].first));
                u64 i, q, o;
                split(g, hit[h].first, &i, &q, &o);
                const u64 pt = hit[h].second.addr;
                u64 e = hit[h].second.e;
                if (g.first && conj_in) e = (n - e) % n;
                if (g.first && gtab) e = (e + (*gtab)[pt * g.in_pk + q * g.in_qk]) % n;
                const u64 N = step_len[g.step], lm = g.step_by_i ? i : q;
                for (u64 j = 0; j < m; ++j) {
                    u64 v = (e + j * pt % m * (n / m)) % n;
                    if (g.step != STEP_NONE) v = (v + j * lm % N * (n / N)) % n;
                    if (g.last && conj_out) v = (n - v) % n;
                    next.push_back(Nz{i * g.b.si + q * g.b.sq + o * g.b.so + j * g.b.sp, v});
                }
            }
            cur.swap(next);
        }
        out->swap(cur);
        return true;
    }
};

static unsigned long long g_checked = 0;

// compares a run's nonzero output with `want` (element -> exponent, -1: zero); `want` is left all -1
static bool compare(Model& M, const std::vector<Nz>& got, std::vector<long long>& want, u64 nonzero) {
    if (got.size() != nonzero) return M.fail(fmt("%llu nonzero outputs where %llu are due", got.size(), nonzero));
    bool ok = true;
    for (const Nz& z : got) {
        if (want[z.addr] != (long long)z.e) ok = false;
        want[z.addr] = -1;  // (a second write to the same element then fails as well)
    }
    g_checked += M.out_size;
    return ok || M.fail("an output exponent differs from the transform's");
}

// a transform route of the lines L against the definition: every impulse position of every line, conjugations off and on, with and without mul_in
static bool model_route(Model& M, const LineShape& L, u64 n, u64 in_len) {
    const u64 lines = L.inner * L.outer;
    M.in_size = lines * L.len_in, M.out_size = lines * n, M.n = n;
    if (!M.geometry()) return false;
    std::vector<u64> gtab(std::max<u64>(in_len, 1));
    for (u64 pos = 0; pos < gtab.size(); ++pos) gtab[pos] = (5 * pos * pos + 3) % n;
    std::vector<long long> want(M.out_size, -1);
    std::vector<Nz> got;
    for (int variant = 0; variant < 8; ++variant) {
        const bool ci = variant & 1, co = variant & 2, mul = variant & 4;
        for (u64 o = 0; o < L.outer; ++o)
            for (u64 i = 0; i < L.inner; ++i)
                for (u64 k = 0; k < L.len_in; ++k) {
                    const u64 c = (2 * (k + i + o) + 1) % n;  // odd
                    if (!M.run(i + L.inner * (k + L.len_in * o), c, ci, co, mul ? &gtab : nullptr, &got)) return false;
                    u64 nonzero = 0;
                    if (k < in_len) {
                        nonzero = n;
                        const u64 e0 = ((ci ? (n - c) % n : c) + (mul ? gtab[k] : 0)) % n;
                        for (u64 j = 0; j < n; ++j) {
                            const u64 e = (e0 + j * k % n) % n;
                            want[i + L.inner * (j + n * o)] = (long long)(co ? (n - e) % n : e);
                        }
                    }
                    if (!compare(M, got, want, nonzero)) return M.fail(fmt("impulse at line (%llu, %llu) point %llu, variant %llu", i, o, k, variant));
                }
    }
    return true;
}

static bool model_pow2(std::string* error, const char* how, const Pow2Route& r, const LineShape& L, int lg, u64 in_len) {
    Model M;
    M.name = fmt((std::string(how) + " lg=%llu inner=%llu outer=%llu len_in=%llu").c_str(), lg, L.inner, L.outer, L.len_in) + fmt(" in_len=%llu", in_len);
    M.passes.assign(r.pass, r.pass + r.npass);
    M.work_size = r.work;
    M.step_len[STEP_N] = r.ntables >= 2 ? r.tables[0].n : 0, M.step_len[STEP_N1] = r.ntables >= 4 ? r.tables[2].n : 0;
    if (r.npass == 0) M.fail("refused");
    else model_route(M, L, 1ull << lg, in_len);
    *error = M.error;
    return M.error.empty();
}

// the fused frames of the spectral estimate against the transform of the zero-padded frame (the real window taken as 1)
static bool model_frames(std::string* error, int mode, u64 window_len) {
    const u64 nfft = 8, hop = 3, frames = 7, fpc = 3, input_rows = 16, wl = spectral_window_points(mode, window_len, nfft);
    Model M;
    M.name = fmt("frames mode=%llu window=%llu", mode, window_len);
    M.passes = {spectral_frame_pass(mode, frames, fpc, hop, input_rows, nfft, wl)};
    M.n = nfft, M.out_size = nfft * frames;
    std::vector<u64> base(frames);
    for (u64 f = 0; f < frames; ++f) base[f] = mode == FRAMES_SLIDING ? f * hop : (f / fpc) * input_rows + (f % fpc) * hop;
    M.in_size = *std::max_element(base.begin(), base.end()) + wl;  // `top`: the fused path is taken only when every frame lies inside the input
    std::vector<long long> want(M.out_size, -1);
    std::vector<Nz> got;
    if (M.geometry())
        for (u64 x = 0; x < M.in_size; ++x) {
            const u64 c = (2 * x + 1) % nfft;
            if (!M.run(x, c, false, false, nullptr, &got)) break;
            u64 nonzero = 0;
            for (u64 f = 0; f < frames; ++f)
                if (x >= base[f] && x - base[f] < wl)
                    for (u64 j = 0; j < nfft; ++j) want[f * nfft + j] = (long long)((c + j * (x - base[f])) % nfft), ++nonzero;
            if (!compare(M, got, want, nonzero)) {
                M.fail(fmt("impulse at %llu", x));
                break;
            }
        }
    *error = M.error;
    return M.error.empty();
}

static int model_mode() {
    std::string error;
    unsigned long cases = 0;
    bool ok = true;
    // per length: the input shorter, equal and longer than n, and `valid` below len_in
    auto lengths = [&](const char* how, int lg, u64 inner, u64 outer, int builder) {
        const u64 n = 1ull << lg;
        for (u64 len_in : {n - 3, n, n + 5})
            for (u64 valid : {~0ull, len_in - 2}) {
                if (!ok) return;
                const LineShape L{inner, outer, len_in};
                const u64 in_len = std::min<u64>(std::min<u64>(len_in, n), valid);
                const Pow2Route r = builder == 0 ? plan_pow2(L, n, valid) : (builder == 1 ? one_pass(L, lg, in_len) : (builder == 2 ? two_pass(L, lg, in_len) : three_pass(L, lg, in_len)));
                ok = model_pow2(&error, how, r, L, lg, in_len);
                ++cases;
            }
    };
    for (int lg : {9, 10})  // through the rule: a trailing dimension past one tile takes two passes
        for (u64 inner : {2, 3}) lengths("plan_pow2", lg, inner, 1, 0);
    for (int lg = 4; lg <= 8; ++lg)
        for (u64 inner : {1, 2, 3})
            for (u64 outer : {1, 2}) lengths("two_pass", lg, inner, outer, 2);
    for (int lg = 6; lg <= 9; ++lg)
        for (u64 outer : {1, 2}) lengths("three_pass", lg, 1, outer, 3);
    for (int lg : {3, 5})  // one tile: mode 0 (inner == 1) and mode 1
        for (u64 inner : {1, 3})
            for (u64 outer : {1, 3}) lengths("one_pass", lg, inner, outer, 1);
    for (u64 inner : {1, 3})  // the one-point pass: inputs without a point, with one and with several
        for (u64 outer : {1, 2})
            for (u64 cur : {0, 1, 4}) {
                if (!ok) break;
                const LineShape L{inner, outer, cur};
                Pow2Route r{};
                r.npass = 1, r.pass[0] = one_point_pass(L);
                ok = model_pow2(&error, "one_point_pass", r, L, 0, std::min<u64>(cur, 1));
                ++cases;
            }
    for (int mode : {(int)FRAMES_SLIDING, (int)FRAMES_COLUMN_SLIDING})
        for (u64 window_len : {8, 5, 11}) {
            if (ok) ok = model_frames(&error, mode, window_len), ++cases;
        }
    if (!ok) {
        std::printf("fft model FAILED: %s\n", error.c_str());
        return 1;
    }
    std::printf("fft model ok: %lu cases, %llu output exponents\n", cases, g_checked);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--sweep")) return sweep(false), 0;
    if (argc == 2 && !std::strcmp(argv[1], "--dump")) return sweep(true), 0;
    if (argc == 2 && !std::strcmp(argv[1], "--table")) return table_mode();
    if (argc == 2 && !std::strcmp(argv[1], "--model")) return model_mode();
    if (argc == 2 && !std::strcmp(argv[1], "--invariants")) {
        g_invariants = g_quiet = true;
        sweep(false);
        if (!g_broken.empty()) {
            std::printf("fft tile invariants FAILED: %s\n", g_broken.c_str());
            return 1;
        }
        std::printf("fft tile invariants ok: %lu tiles\n", g_tiles);
        return 0;
    }
    std::fprintf(stderr, "usage: fft_route_check --table < cases | --sweep | --dump | --invariants | --model\n");
    return 2;
}
