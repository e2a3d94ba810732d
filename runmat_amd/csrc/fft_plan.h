// fft_plan.h -- which passes, tiles, work buffers and tables a transform along one dimension gets, as pure host functions.  The
// drivers of fft.hip (fft_pow2, fft_bluestein, fft_entry, spectral_entry) describe the lines, call a plan function and execute what
// they get through launch_pass: a size rule or a pass's addressing lives here or it does not exist.  No HIP header, no Context, no
// pointers - a pass names its buffers by role - so tests/cpp/fft_route_check.cpp compiles this file with a plain host compiler,
// prints what a shape will launch (--table), checks the rules against digests taken from the drivers' former conditions
// (tests/golden/fft_routes.txt), the tiles against the kernel's limits (--invariants) and the addressing of every route exactly, by
// running its passes on impulses whose values are exponents of w_n (--model).  A new route is one more builder here, and --model
// tells its author on the CPU whether its strides are right.
#pragma once
#include <algorithm>
#include <cstddef>

namespace rmhip {
namespace fft_plan {

typedef unsigned long long u64;

// ---- geometry the rules and the kernel share (fft.hip: `using namespace fft_plan`) ----------------------------------------------------------
constexpr int TILE = 4096;        // complex points per workgroup (512 threads, two workgroups per CU) ...
constexpr int TILE_SMALL = 2048;  // ... half of that for lines of up to 2048 points (256 threads, four per CU) ...
constexpr int TILE_BIG = 8192;    // ... or a whole 8192-point line (1024 threads, one workgroup per CU: 132 KiB of LDS)
constexpr int MAXB = 256;         // lines per workgroup
constexpr int STEP_LO = 12;       // step twiddle w_n^t = lo[t & 4095] * hi[t >> 12]

// ---- thresholds --------------------------------------------------------------------------------------------------------------------------
// A line along a trailing dimension (inner > 1) is read across neighbouring lines - short transforms, many lines per tile -, so
// one tile serves it up to 2^8 points; a line along dimension 0 up to a whole TILE_BIG tile.
constexpr int kOneTileLgTrailing = 8;
// The longest lines the drivers take ("fft: length %llu" beyond): every factor of the three passes along dimension 0, and both of the two
// passes along a trailing dimension, then still fit a tile.
constexpr int kMaxLg = 27;          // inner == 1
constexpr int kMaxLgTrailing = 24;  // inner > 1
// Three passes along dimension 0 from 2^23: measured crossover (scripts/fft_long_ab.py): 2^22 equal, 2^23 0.33 -> 0.22 ms,
// 2^24 0.78 -> 0.49 ms.  Two factors of a very long line pass 2048 and a tile holds one or two lines: the strided side of each pass
// moves 16- or 32-byte pieces (a 2^24-point vector: 0.80 ms).
constexpr int kThreePassLg = 23;
// Bluestein: the chirp convolution's length M (a power of two >= 2n - 1) is at most 2^24; a slab of inner * M points of the two work
// tensors [inner, M, outer'] at most 2^27, and as many outer indices at a time as keep each tensor at 2^26 points (~1 GiB): whole
// outer slabs at a time.
constexpr u64 kChirpMaxM = 1ull << 24;
constexpr u64 kChirpMaxSlab = 1ull << 27;
constexpr u64 kChirpWorkPoints = 1ull << 26;

inline int ilog2(u64 v) {
    int l = 0;
    while ((1ull << l) < v) ++l;
    return l;
}
inline bool is_pow2(u64 v) { return v && !(v & (v - 1)); }

// ---- a pass --------------------------------------------------------------------------------------------------------------------------------
struct Side {  // where point p of line (i, q, o) lives: element offset i*si + q*sq + o*so + p*sp
    u64 si, sq, so, sp;
};
enum Source { FROM_INPUT, FROM_WORK };    // the caller's input (real or complex), or the route's work buffer (complex)
enum Dest { TO_WORK, TO_OUTPUT };
enum StepTable { STEP_NONE, STEP_N, STEP_N1 };  // the step twiddle's tables: none, those of the length n, those of N1 = m2 m3

// The pointer-free part of the kernel's FftPass.  Line l = i + inner * (q + qcnt * o); point p of it is read at a, exists iff
// p*in_pk + q*in_qk < in_len (else it reads as zero; the same position indexes mul_in / the window), and result j is written at b
// after the step twiddle w_N^(j * (step_by_i ? i : q)).
struct PassGeom {
    u64 nlines, inner, qcnt;
    Side a, b;
    u64 in_pk, in_qk, in_len;
    int log2m, mode, step_by_i;  // mode: see k_fft_tile
    Source src;
    Dest dst;
    StepTable step;
    bool first, last;  // the first pass of a route carries conj_in / mul_in, the last one conj_out / scale / round32
};

// ---- the tile of a pass ------------------------------------------------------------------------------------------------------------------
struct TilePlan {
    int log2b;         // 2^log2b lines per workgroup
    int nrad, rad[5];  // the tile's radices, (4 or 2,) 8, 8, ...
    int threads;       // 256 / 512 / 1024: the k_fft_tile instantiation
    size_t lds;        // dynamic LDS bytes
    u64 blocks;
    bool refused;      // more than 2^31 - 1 workgroups ("fft: %llu lines")
};

inline void set_radices(int log2m, int* nrad, int* rad) {
    int rem = log2m;
    *nrad = 0;
    if (rem % 3 == 2) rad[(*nrad)++] = 4, rem -= 2;  // the odd radix first: that pass has no twiddles
    if (rem % 3 == 1) rad[(*nrad)++] = 2, rem -= 1;
    while (rem >= 3) rad[(*nrad)++] = 8, rem -= 3;
}

inline TilePlan plan_tile(int log2m, int mode, u64 nlines) {
    TilePlan t{};
    set_radices(log2m, &t.nrad, t.rad);
    const size_t m = (size_t)1 << log2m;
    // lines of up to 2048 points take half-size tiles (256 threads, 37 KiB: four workgroups per CU instead of two - the same threads per CU
    // in more independent phases: 3-7 % on every shape measured), unless that would leave fewer than eight neighbouring lines to a tile
    const size_t cap = m <= (size_t)TILE_SMALL && (mode == 0 || m * 8 <= (size_t)TILE_SMALL) ? (size_t)TILE_SMALL : (size_t)TILE;
    int lb = 0;
    while ((m << (lb + 1)) <= cap && (1 << (lb + 1)) <= MAXB && (1ull << lb) < nlines) ++lb;
    t.log2b = lb;
    t.blocks = (nlines + (1ull << lb) - 1) >> lb;
    t.refused = t.blocks > 0x7fffffffull;
    const size_t tile = m << lb, B = (size_t)1 << lb;
    // two padded planes (re, im: one pad slot per eight), then per line two 64-bit bases and two 32-bit words
    t.lds = (2 * (tile + (tile >> 3) + 1) + 2 * B) * sizeof(double) + 2 * B * sizeof(unsigned);
    t.threads = tile > (size_t)TILE ? 1024 : (tile <= (size_t)TILE_SMALL ? 256 : 512);
    return t;
}

// ---- power-of-two transforms -----------------------------------------------------------------------------------------------------------------
// A set of lines in tensor layout: point k of line (i, o) at element i + inner * (k + len_in * o) of the input and at
// i + inner * (k + n * o) of the complex result.
struct LineShape {
    u64 inner, outer, len_in;  // len_in: points the input holds per line
};

struct TableSpec {  // k_fft_table's (kind, n, count)
    int kind;
    u64 n, count;
};

struct Pow2Route {
    int npass;  // 1..3, or 0: the length is refused ("fft: length %llu")
    PassGeom pass[3];
    u64 work;         // complex points of the work buffer (0: none)
    int ntables;      // 0, 2 (STEP_N's lo, hi) or 4 (then STEP_N1's lo, hi)
    TableSpec tables[4];
};

// the rule: how many passes a power-of-two length 2^lg takes at this inner (0: refused)
inline int pow2_passes(u64 inner, int lg) {
    if (inner == 1 ? (1ull << lg) <= (u64)TILE_BIG : lg <= kOneTileLgTrailing) return 1;
    if (lg > (inner == 1 ? kMaxLg : kMaxLgTrailing)) return 0;
    return inner == 1 && lg >= kThreePassLg ? 3 : 2;
}

inline void step_tables(u64 n, TableSpec* lo_hi) {
    lo_hi[0] = TableSpec{0, n, std::min<u64>(n, 1ull << STEP_LO)};
    lo_hi[1] = TableSpec{1, n, std::max<u64>(1, n >> STEP_LO)};
}

// one tile per 2^log2b lines: points contiguous along dimension 0 (mode 0), neighbouring lines contiguous otherwise (mode 1)
inline Pow2Route one_pass(const LineShape& L, int lg, u64 in_len) {
    const u64 n = 1ull << lg;
    Pow2Route r{};
    r.npass = 1;
    PassGeom& P = r.pass[0];
    P.nlines = L.inner * L.outer, P.inner = L.inner, P.qcnt = 1;
    P.a = Side{1, 0, L.len_in * L.inner, L.inner};
    P.b = Side{1, 0, n * L.inner, L.inner};
    P.in_pk = 1, P.in_qk = 0, P.in_len = in_len;
    P.log2m = lg, P.mode = L.inner > 1 ? 1 : 0;
    P.src = FROM_INPUT, P.dst = TO_OUTPUT, P.step = STEP_NONE;
    P.first = P.last = true;
    return r;
}

// n = m1 * m2: (1) length-m1 transforms over k1 of x[k1 * m2 + k2], times w_n^(j1 k2), into T[j1 * m2 + k2];
//              (2) length-m2 transforms over k2 of T[j1 * m2 + k2] into y[j1 + m1 * j2]
inline Pow2Route two_pass(const LineShape& L, int lg, u64 in_len) {
    const u64 n = 1ull << lg, lines = L.inner * L.outer;
    const int l1 = lg / 2, l2 = lg - l1;
    const u64 m1 = 1ull << l1, m2 = 1ull << l2;
    Pow2Route r{};
    r.npass = 2, r.work = n * lines, r.ntables = 2;
    step_tables(n, r.tables);
    PassGeom& A = r.pass[0];
    A.nlines = lines * m2, A.inner = L.inner, A.qcnt = m2;
    A.a = Side{1, L.inner, L.len_in * L.inner, m2 * L.inner};
    A.b = Side{1, L.inner, n * L.inner, m2 * L.inner};
    A.in_pk = m2, A.in_qk = 1, A.in_len = in_len;
    A.log2m = l1, A.mode = 1;  // neighbouring lines (i, then k2) are neighbours in memory
    A.src = FROM_INPUT, A.dst = TO_WORK, A.step = STEP_N, A.first = true;
    PassGeom& B = r.pass[1];
    B.nlines = lines * m1, B.inner = L.inner, B.qcnt = m1;
    B.a = Side{1, L.inner * m2, n * L.inner, L.inner};
    B.b = Side{1, L.inner, n * L.inner, m1 * L.inner};
    B.in_pk = 1, B.in_qk = 0, B.in_len = m2;
    B.log2m = l2, B.mode = L.inner > 1 ? 1 : 2;
    B.src = FROM_WORK, B.dst = TO_OUTPUT, B.step = STEP_NONE, B.last = true;
    return r;
}

// Along dimension 0 only (L.inner == 1).  n = m1 m2 m3, k = k1 m2 m3 + k2 m3 + k3, j = j1 + m1 j2 + m1 m2 j3, every pass reading and
// writing neighbouring lines:
//   (A) over k1 (stride m2 m3), lines (k', o), k' = k2 m3 + k3, times w_n^(j1 k')          -> T[o][j1][k']
//   (B) over k2 (stride m3),   lines (k3, j1, o),            times w_{m2 m3}^(j2 k3)       -> T[o][j1][j2][k3]   (in place)
//   (C) over k3 (contiguous),  lines (j1, j2, o)                                           -> y[o][j1 + m1 j2 + m1 m2 j3]
inline Pow2Route three_pass(const LineShape& L, int lg, u64 in_len) {
    const u64 n = 1ull << lg, lines = L.inner * L.outer;
    const int l1 = lg / 3, l2 = (lg - l1) / 2, l3 = lg - l1 - l2;
    const u64 m1 = 1ull << l1, m2 = 1ull << l2, m3 = 1ull << l3, N1 = m2 * m3;
    Pow2Route r{};
    r.npass = 3, r.work = n * lines, r.ntables = 4;
    step_tables(n, r.tables);
    step_tables(N1, r.tables + 2);
    PassGeom& A = r.pass[0];
    A.nlines = lines * N1, A.inner = 1, A.qcnt = N1;
    A.a = Side{0, 1, L.len_in, N1};
    A.b = Side{0, 1, n, N1};
    A.in_pk = N1, A.in_qk = 1, A.in_len = in_len;
    A.log2m = l1, A.mode = 1;
    A.src = FROM_INPUT, A.dst = TO_WORK, A.step = STEP_N, A.first = true;
    PassGeom& B = r.pass[1];
    B.nlines = lines * m1 * m3, B.inner = m3, B.qcnt = m1;
    B.a = Side{1, N1, n, m3};
    B.b = Side{1, N1, n, m3};
    B.in_pk = 1, B.in_qk = 0, B.in_len = m2;
    B.log2m = l2, B.mode = 1, B.step_by_i = 1;
    B.src = FROM_WORK, B.dst = TO_WORK, B.step = STEP_N1;
    PassGeom& C = r.pass[2];
    C.nlines = lines * m1 * m2, C.inner = m1, C.qcnt = m2;
    C.a = Side{N1, m3, n, 1};
    C.b = Side{1, m1, n, m1 * m2};
    C.in_pk = 1, C.in_qk = 0, C.in_len = m3;
    C.log2m = l3, C.mode = 2;
    C.src = FROM_WORK, C.dst = TO_OUTPUT, C.step = STEP_NONE, C.last = true;
    return r;
}

// The route of a length-n transform (n a power of two) of the lines L; input points from `valid` on read as zero whatever the input holds.
inline Pow2Route plan_pow2(const LineShape& L, u64 n, u64 valid = ~0ull) {
    const int lg = ilog2(n);
    const u64 in_len = std::min<u64>(std::min<u64>(L.len_in, n), valid);
    switch (pow2_passes(L.inner, lg)) {
        case 1: return one_pass(L, lg, in_len);
        case 2: return two_pass(L, lg, in_len);
        case 3: return three_pass(L, lg, in_len);
        default: return Pow2Route{};
    }
}

// ---- the entry's own routes ------------------------------------------------------------------------------------------------------------------
enum EntryRoute { ENTRY_ZERO_FILL, ENTRY_ONE_POINT, ENTRY_POW2, ENTRY_CHIRP };

// `cur` points per line in the input, n in the result.  A one-point transform is the point itself (or zero where the input has none);
// a longer transform of lines without a point is all zeros: a memset, no launch.
inline EntryRoute plan_entry(u64 cur, u64 n) {
    if (n == 1) return ENTRY_ONE_POINT;
    if (cur == 0) return ENTRY_ZERO_FILL;
    return is_pow2(n) ? ENTRY_POW2 : ENTRY_CHIRP;
}

// the tile kernel with m = 1 has no pass to run: it stages the points and stores them
inline PassGeom one_point_pass(const LineShape& L) {
    PassGeom P{};
    P.nlines = L.inner * L.outer, P.inner = L.inner, P.qcnt = 1;
    P.a = Side{1, 0, L.len_in * L.inner, L.inner};
    P.b = Side{1, 0, L.inner, L.inner};
    P.in_pk = 1, P.in_qk = 0, P.in_len = std::min<u64>(L.len_in, 1);
    P.log2m = 0, P.mode = 1;
    P.src = FROM_INPUT, P.dst = TO_OUTPUT, P.step = STEP_NONE;
    P.first = P.last = true;  // (fft_entry hands it no conjugation: the two of an inverse cancel on a single point)
    return P;
}

// ---- Bluestein ---------------------------------------------------------------------------------------------------------------------------
enum ChirpRefusal { CHIRP_OK, CHIRP_LENGTH, CHIRP_SLAB };  // "fft: length %llu" / "fft: %llu lines of chirp length %llu along a trailing dimension"

struct ChirpPlan {
    ChirpRefusal refused;
    u64 M;          // the convolution's power-of-two length >= 2n - 1
    u64 slab;       // inner * M
    u64 outer_per;  // outer indices per piece of the work tensors
    u64 nslabs;
    u64 valid;      // input points the first transform reads (the rest of its M-long lines is zero)
};

// The length rule comes first: fft_bluestein builds the chirp and G (tables of n and M) between the two refusals.
inline ChirpPlan plan_chirp(const LineShape& L, u64 n) {
    ChirpPlan p{};
    p.M = 1;
    while (p.M < 2 * n - 1) p.M <<= 1;
    if (p.M > kChirpMaxM) {
        p.refused = CHIRP_LENGTH;
        return p;
    }
    p.slab = L.inner * p.M;
    if (p.slab > kChirpMaxSlab) {
        p.refused = CHIRP_SLAB;
        return p;
    }
    p.outer_per = std::min<u64>(L.outer, std::max<u64>(1, kChirpWorkPoints / p.slab));
    p.nslabs = (L.outer + p.outer_per - 1) / p.outer_per;
    p.valid = std::min<u64>(L.len_in, n);
    return p;
}

struct Slab {
    u64 o0, oc;  // outer indices o0 .. o0 + oc
};
inline Slab chirp_slab(const ChirpPlan& p, u64 outer, u64 k) {
    const u64 o0 = k * p.outer_per;
    return Slab{o0, std::min<u64>(p.outer_per, outer - o0)};
}

// whether fft_pow2 / fft_bluestein transform lines of n points at this inner
inline bool length_served(u64 n, u64 inner) {
    if (is_pow2(n)) return pow2_passes(inner, ilog2(n)) != 0;
    return plan_chirp(LineShape{inner, 1, n}, n).refused == CHIRP_OK;
}

// ---- framed spectra (spectral_entry) -------------------------------------------------------------------------------------------------------
enum FrameMode { FRAMES_SLIDING = 0, FRAMES_COLUMN_SLIDING = 1, FRAMES_FOLDED_COLUMNS = 2 };

// window points a frame reads: the folded mode reads all of the window, the others truncate it at nfft
inline u64 spectral_window_points(int mode, u64 window_len, u64 nfft) { return mode == FRAMES_FOLDED_COLUMNS ? window_len : std::min<u64>(window_len, nfft); }

struct SpectralPlan {
    bool fused;         // k_fft_tile loads the frames straight from the signal; else k_spectral_frame writes them out first
    bool own_spectrum;  // a one-point frame is its own spectrum: the frame kernel writes what the finish kernel reads
    bool direct;        // two-sided: the transform's output IS `s`
    bool alloc_frames, alloc_spec;  // the [nfft, frames] temporaries that exist (the window's copy always does)
    u64 rows, shift;    // rows of `s` / `ps`; the centered range's rotation (common.rs:221-227)
};

// `top`: one past the largest source index any frame forms.  A power-of-two frame that one tile holds is fused unless it is folded or
// reaches past input_len.
inline SpectralPlan plan_spectral(int mode, int range, u64 nfft, u64 top, u64 input_len) {
    SpectralPlan s{};
    s.fused = is_pow2(nfft) && nfft >= 2 && nfft <= (u64)TILE_BIG && mode != FRAMES_FOLDED_COLUMNS && top <= input_len;
    s.rows = range == 0 ? nfft / 2 + 1 : nfft;
    s.shift = nfft % 2 == 0 ? nfft / 2 + 1 : (nfft + 1) / 2;
    s.direct = range == 1;
    s.own_spectrum = nfft == 1 && !s.fused;
    s.alloc_frames = !s.fused && !(s.own_spectrum && s.direct);
    s.alloc_spec = !s.direct && !s.own_spectrum;
    return s;
}

// The fused frames: frame c starts at c * hop (Sliding) or at (c / fpc) * input_rows + (c % fpc) * hop (ColumnSliding), holds wl
// windowed points and is zero-padded to nfft; spectrum c goes to [nfft, frames] column c.
inline PassGeom spectral_frame_pass(int mode, u64 frames, u64 fpc, u64 hop, u64 input_rows, u64 nfft, u64 wl) {
    const bool columns = mode == FRAMES_COLUMN_SLIDING;
    PassGeom P{};
    P.nlines = frames, P.inner = 1, P.qcnt = columns ? fpc : 1;
    P.a = columns ? Side{0, hop, input_rows, 1} : Side{0, 0, hop, 1};
    P.b = Side{0, nfft, nfft * P.qcnt, 1};
    P.in_pk = 1, P.in_qk = 0, P.in_len = wl;
    P.log2m = ilog2(nfft), P.mode = 0;
    P.src = FROM_INPUT, P.dst = TO_OUTPUT, P.step = STEP_NONE;
    P.first = P.last = true;
    return P;
}

}  // namespace fft_plan
}  // namespace rmhip
