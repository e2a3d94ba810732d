// lu_plan.h -- which driver, panel kernel, triangular-solve kernel and schedule an LU factorisation or a substitution gets, as pure host
// functions.  The drivers of lu.hip (lu_factor_device, getrf_rec, launch_trsm_fused, getrf_blocked, getrf_super, substitute_few_rhs) and
// the solves of solve.cpp fill in the problem and the site, call a plan_* function and execute what they get: a size rule lives here or
// it does not exist.  No HIP header, no Context, no environment reads (lu_knobs() / lu_process_knobs() in lu.hip read RMHIP_LU_* and
// hand the values in): tests/cpp/lu_route_check.cpp compiles this file with a plain host compiler, prints what a given order and knob
// setting will launch (--table) and checks the rules against digests taken from the drivers' former conditions
// (tests/golden/lu_routes.txt).  The measurements that justify a threshold stand beside it; notes on schedules that were tried and lost
// stay with the stream choreography in lu.hip.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace rmhip {

// The RMHIP_LU_* environment knobs (docs/KNOBS.md), each read by one of the two functions declared in common.h (lu.hip) and nowhere else.
struct LuKnobs {  // read on every call: tests flip these inside one process
    bool fast = true;             // RMHIP_LU_FAST=0: the grid-wide pivot rule on the solve path too
    double tau = 8.0;             // RMHIP_LU_TAU: the solve path's multiplier bound
    bool pad = true;              // RMHIP_LU_PAD=0: the solves factor at the order they were given
    int lookahead = -1;           // RMHIP_LU_LOOKAHEAD: 1 forces the look-ahead driver, 0 disables it, -1 (unset) by order
    long nb = -1;                 // RMHIP_LU_NB: panel width of the one-level look-ahead driver (-1: by order)
    bool panel_columns = false;   // RMHIP_LU_PANEL=columns: the one-launch-per-column panels
    bool panel_debug = false;     // RMHIP_LU_PANEL_DEBUG=1: phase ticks of the panel kernels on stderr
    bool subst_pair = false;      // RMHIP_LU_SUBST=pair: launch-per-block substitution instead of k_subst_chain
    bool verbose = false;         // RMHIP_LU_VERBOSE
    bool timeline = false;        // RMHIP_LU_TIMELINE
    bool test_retry = false;      // RMHIP_LU_TEST_RETRY (test hook)
    bool test_growth = false;     // RMHIP_LU_TEST_GROWTH (test hook)
    bool test_subst_retry = false;  // RMHIP_LU_TEST_SUBST_RETRY (test hook)
};
struct LuProcessKnobs {  // read once per process: tests set these in a fresh subprocess
    bool super = true;            // RMHIP_LU_SUPER=0: the one-level driver on the solve path
    std::vector<std::pair<size_t, size_t>> super_seq;  // RMHIP_LU_SUPER_SEQ: super-panel plan (W, nb) (empty: by order)
    std::pair<size_t, size_t> super_late{128, 128};    // RMHIP_LU_SUPER_LATE
    long super_rows = -1;         // RMHIP_LU_SUPER_ROWS (-1: by order)
    int iprep = -1;               // RMHIP_LU_IPREP (-1: by order)
    bool iprep_split = true;      // RMHIP_LU_IPREP_SPLIT
    long small_upd = 1024;        // RMHIP_LU_SMALL_UPD (dgemm.hip)
    bool rb_mfma = true;          // RMHIP_LU_RB_MFMA
    bool trsm_mfma = true;        // RMHIP_LU_TRSM_MFMA
    int skip = 0;                 // RMHIP_LU_SKIP: phase bit mask (results are garbage)
};

// ---- geometry the rules and the kernels share (lu.hip: `using namespace lu_plan`) ----------------------------------------------------------
namespace lu_plan {
constexpr int BASE_W = 64;   // base panel width (columns factored one launch each)
constexpr int TRSM_W = 128;  // base triangular solve size (one fused launch)
constexpr int TRSM_SW = TRSM_W + 1;  // LDS row stride (doubles) of a 65..128-wide solve; 65 for <= 64
// per-column panels (k_lu_col)
constexpr int MAX_PANEL_BLOCKS = 1024;  // 64 rows per block => up to 65536 rows per panel
constexpr int PANEL_JT = 8;             // panel columns per thread (unrolled batch; keep the code small)
constexpr int PANEL_GROUPS = BASE_W / PANEL_JT;
constexpr int PANEL_ROWS = 64;  // rows per block (32 was measured slower: 278 vs 246 ms at n = 16384)
constexpr int PANEL_THREADS = PANEL_ROWS * PANEL_GROUPS;
// persistent panels (k_lu_panel2)
constexpr int PK_MAXB = 256;  // at most one block per CU
constexpr int P2_ROWS = 256;
constexpr int P2_THREADS = P2_ROWS;
constexpr int P2_WAVES = P2_THREADS / 64;
constexpr int P2_ONEHOP_MAXB = 32;
constexpr int P2_RB = BASE_W + 16;  // row stride of the wave candidate buffer (the dump runs in groups of 16 slots and may overshoot by 12)
constexpr size_t P2_LDS_DOUBLES = (size_t)P2_ONEHOP_MAXB * BASE_W + (size_t)P2_WAVES * P2_RB;  // 18.5 KiB
// solve-path panels (k_rp_top, k_rp_below, k_rp_below_mfma)
constexpr int RT_ROWS = 256;    // rows of the top block = threads of k_rp_top
constexpr int RBM_JT = 2;       // 16-row tiles per wave (32 rows: 64 accumulator registers - the wave must fit beside an update block's two waves per SIMD)
constexpr int RB_THREADS = 64;
constexpr int RU_MAX_RHS = 8;   // right-hand sides the few-column substitution kernels serve
// update-stream dgemm blocks ask for 84 KiB of LDS (73.7 needed): one per CU, leaving 76 KiB for a panel
// block (66 KiB) or a main-stream dgemm block (73.7 KiB)
constexpr size_t kSidePad = 84 * 1024 - 73728;

// ---- thresholds --------------------------------------------------------------------------------------------------------------------------
// Look-ahead (second stream): default from kmin = 5120; RMHIP_LU_LOOKAHEAD=1 forces it for every kmin > nb, =0 disables it.  From an
// interleaved sweep (scripts/lu_knobs.py, ms for x = A\b): n = 6144: 38.7 without look-ahead, 33.6 with nb 128, 34.9 with 256, 36.8 with
// 512; 8192: 51.2 (nb 512) / 48.4 (256) / 47.2 (128); 10240: 67.3 / 63.4 / 62.2; 12288: 84.7 / 80.6 / 81.2; 16384: 130.8 / 130.7 / -;
// 5120: 31.6 without, 27.9 with; 4096: 22.2 without, 22.6-24 with.
constexpr size_t kBlockedMin = 5120;
// Solve path (one-workgroup panels: nothing has to be co-resident, and the chain is all there is at these sizes): from 1152 -
// n = 1280 3.30 -> 2.52 ms, 1536 3.63 -> 2.95, 2048 4.30 -> 3.91, 3072 8.06 -> 5.98, 4096 9.92 -> 8.17 (5120: 16.9 without,
// 10.6 with; 1024: 2.03 / 2.00).
constexpr size_t kBlockedMinFast = 1152;
constexpr size_t kNbWideFrom = 12288;  // default panel width of the look-ahead driver: 128 below, 256 from here (the sweep above)
// two-level driver (super-panels) on the solve path from kmin = 8192 (RMHIP_LU_SUPER=0: the one-level driver)
constexpr size_t kSuperMin = 8192;
// k_rp_top: like k_lu_panel2 the block ASKS for more LDS than it uses (48.6 KiB static) so that it does not share its CU with an
// update-stream dgemm block: every column step would run slower beside one (the phase-dependent values of the drivers apply)
constexpr long kTopPadKb = 96;  // (96: the workgroup has its CU to itself; 32: 78.3 -> 77.3 ms at n = 16384)
// k_lu_panel2: the block needs 18.5 KiB of LDS but ASKS for 82.5: it then does not fit beside an update-stream dgemm block
// (84 KiB) and waits for a CU of its own.  Sharing a CU costs more than the wait: with the panel waves on the
// same SIMDs as a dgemm wave every column step slows down, and the column chain is the critical path
// (n = 16384: 135 ms sharing, 123 ms exclusive).
constexpr long kPanelPadKb = 64;
// getrf_blocked, panel width by phase.  While the trailing matrix is large the update stream is the bottleneck and the main stream
// idles a third of the time: wider panels there (fewer, deeper rank-k updates: the dgemm runs 53 instead of 47
// TFLOP/s at k = 512 with one block per CU).  Once the panel chain is the critical path (about the last 8192
// columns) the narrower panel wins.  n = 16384: 128.3 -> 125.2 ms (interleaved, scripts/lu_env_ab.sh); giving the
// main stream a share of the trailing columns as well (its dgemm blocks fit beside the update stream's) measured
// nothing (127.3 vs 127.9).
constexpr size_t kNbEarly = 512, kEarlyRows = 10240;  // (10240 since the update stream's eight-wave dgemm: 113.7 -> 112.7 ms; 8192 before)
// third tier: once the panel chain is the critical path, a narrower panel moves more of each update from the main stream
// (look-ahead columns) to the idle update stream
// (n = 16384, interleaved: 123.1 / 124.2 ms without, 120.8 / 120.6 with 128 below 6144 rows; 64 below 3072: 122.9 / 121.6)
constexpr size_t kNbLate = 128, kLateRows = 8192;  // (8192 since the two-pass solve and the third stream: 98.4 vs 99.1 ms at n = 16384; 6144 before)
// the very first panel is narrower (the update stream has nothing to do until it is factored: 128 columns instead of
// 512 start it 1.5 ms earlier; n = 16384: 108.9 -> 107.9 ms); the second one realigns to multiples of the wide width
constexpr size_t kNbFirst = 128;
// getrf_blocked, split update: on the update stream the interchanges and triangular solves are 14 % of the throughput-bound first half,
// and the matrix cores idle meanwhile.  While more than kSplitRows rows remain (6144: into the beginning of the late phase; 8192
// measured 0.5 ms slower at n = 16384 and 8192) the trailing columns - at least kSplitMinCols of them - are cut at a fixed column csplit
// into A | B.  csplit stays put (so A_j lies inside A_{j-1}) until A has shrunk below 1 / kSplitShrink of the range or to fewer than
// kSplitMinA columns, then it moves to the middle again, rounded to kSplitAlign.
constexpr size_t kSplitRows = 6144, kSplitMinCols = 2048, kSplitMinA = 256, kSplitShrink = 5, kSplitAlign = 128;
// getrf_super: the large-order plan (defaults by order, interleaved runs of scripts/lu_super_ab.sh: n = 16384 69.7-69.9 ms with
// 256 / 1024 / 2048-column super-panels of 256-column panels down to 4096 remaining rows against 71.6-72.7 with the 512-column plan;
// 12288 41.0-41.5 against 40.9, 8192 22.1 against 20.8: the shorter plan stays below 14336)
constexpr size_t kSuperLargeMin = 14336;
// The solves pad a ragged order from here (lu_pad_rows)
constexpr size_t kPadMin = 2048;
constexpr size_t kPadMaxOrder = 65535;  // k_lu_pad_identity's blockIdx.y
// k_subst_chain: four or more 128-row blocks (below, the launches do not matter), in groups of four right-hand sides
constexpr size_t kChainMinBlocks = 4, kChainGroup = 4;

inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
inline size_t min_of(size_t a, size_t b) { return a < b ? a : b; }
}  // namespace lu_plan

// ---- the factorisation as a whole (lu_factor_device) ---------------------------------------------------------------------------------------
struct LuProblem {
    size_t rows = 0, cols = 0;
    int mode = 0;                 // 0: the reference's pivot sequence (`lu`); 1: the solve path (pivots unobservable)
    bool deferred_guard = false;  // the caller folds the status words into a guard of its own (csrc/sharded.cpp): nothing is read back
};
struct LuSite {  // the context's state that bears on the choice
    int num_cus = 256;
    bool one_xcd_ok = true;     // panels may place their blocks on one XCD (cleared when such a panel timed out once)
    bool conservative = false;  // the spread placement timed out as well: per-column panels from now on
};
enum class LuDriver { rec, blocked, super };  // getrf_rec, getrf_blocked, getrf_super
struct LuRoute {
    LuDriver driver = LuDriver::rec;
    size_t nb = 0;            // panel width of getrf_blocked
    bool persistent = true;   // k_lu_panel2 for base panels (they need all their blocks co-resident: 18.5 KiB of LDS and 270 VGPRs per
                              // 4-wave block, at most one per CU beside a dgemm block, so up to num_cus blocks)
    bool fast = false;        // solve path: k_rp_top + k_rp_below*, pivoting restricted to each panel's top block
    bool use_linv = false;    // matrix-core triangular solves with k_rp_top's inverted diagonal blocks (every base panel 64 columns wide)
    bool screen = false;      // the first panel's multipliers are read back at once (the early way out of the solve path)
    double tau = 8.0;
    const char* unsupported = nullptr;  // set: no driver serves the request, and this is the message
};

inline LuRoute plan_lu_factor(const LuProblem& p, const LuSite& site, const LuKnobs& knobs, const LuProcessKnobs& pknobs) {
    using namespace lu_plan;
    LuRoute r;
    if (p.rows > 0x7fffffffULL || p.cols > 0x7fffffffULL) return r.unsupported = "lu: dimension exceeds 2^31", r;
    const size_t kmin = min_of(p.rows, p.cols);
    r.persistent = !(knobs.panel_columns || site.conservative);
    // RMHIP_LU_FAST=0 keeps the grid-wide pivot rule everywhere; RMHIP_LU_TAU sets the multiplier bound
    r.fast = p.mode == 1 && knobs.fast && r.persistent;
    r.tau = knobs.tau;
    r.use_linv = r.fast && pknobs.trsm_mfma && !knobs.panel_debug;
    r.screen = !p.deferred_guard;
    r.nb = knobs.nb >= 0 ? (size_t)knobs.nb : (kmin < kNbWideFrom ? 128 : 256);
    r.nb = r.nb < 64 ? 64 : (r.nb / 64) * 64;
    bool blocked = kmin >= (r.fast ? kBlockedMinFast : kBlockedMin) && kmin > r.nb;
    if (knobs.lookahead >= 0) blocked = kmin > r.nb && knobs.lookahead == 1;
    // look-ahead needs the persistent panels: with one launch per column the panel kernels wait behind the update's dgemm blocks
    if (!r.persistent) blocked = false;
    const bool super = blocked && r.fast && pknobs.super && kmin >= kSuperMin;
    r.driver = super ? LuDriver::super : (blocked ? LuDriver::blocked : LuDriver::rec);
    return r;
}

// ---- one base panel of at most BASE_W columns (getrf_rec's base case) ------------------------------------------------------------------------
enum class PanelKind { top, persistent, columns };  // k_rp_top (+ rows below), k_lu_panel2, k_lu_col per column + k_build_plist
enum class PanelBelow { none, mfma, valu };          // k_rp_below_mfma, k_rp_below
struct PanelRoute {
    PanelKind kind = PanelKind::columns;
    unsigned grid = 0, threads = 0;
    size_t lds_bytes = 0;   // dynamic LDS the launch asks for (top and persistent: padding included)
    int bstride = 1;        // persistent: 8 places the blocks on one XCD
    size_t top_rows = 0;    // top: rows of the one-workgroup block
    bool inverses = false;  // top: k_rp_top also inverts U's and L's 16 x 16 diagonal blocks (for k_rp_below_mfma and k_trsm_lower_mfma)
    PanelBelow below = PanelBelow::none;
    unsigned below_grid = 0;
    size_t steps = 0;       // columns: launches of k_lu_col after the initial one
    const char* unsupported = nullptr;
};

// Most blocks a base panel may have and still sit on ONE XCD, one per CU (0: never - after such a panel timed out once, see
// lu_factor_device).  One-XCD placement when every block finds a CU of its own on one XCD: the exchange hop drops from a write-through +
// a miss in another XCD's L2 to two accesses of one L2 (scripts/micro/xcd_exchange.hip: 2.1-2.5 -> 1.45 us per step).
inline size_t one_xcd_block_limit(const LuSite& site) { return site.one_xcd_ok ? (size_t)site.num_cus / 8 : 0; }
// does the panel that starts at row / column j sit on one XCD?
inline bool panel_on_one_xcd(size_t rows, size_t j, const LuSite& site) {
    return lu_plan::ceil_div(rows - j, lu_plan::P2_ROWS) <= one_xcd_block_limit(site);
}

// panel_pad_kb: the LDS pad the driver in charge asks for in this phase (LuState::panel_pad_kb; -1: the kernel's default)
inline PanelRoute plan_base_panel(size_t rows, size_t j0, size_t w, const LuRoute& route, const LuSite& site, long panel_pad_kb,
                                  const LuProcessKnobs& pknobs, bool debug) {
    using namespace lu_plan;
    PanelRoute p;
    const bool skip = pknobs.skip & 1;
    const size_t below_rows = rows - j0;
    if (route.fast && !skip) {
        // solve path: ONE workgroup factors the top RT_ROWS rows with partial pivoting (no exchange), k_rp_below* turns every row below
        // into multipliers and records the largest one
        p.kind = PanelKind::top;
        p.grid = 1, p.threads = RT_ROWS;
        p.lds_bytes = (size_t)(panel_pad_kb >= 0 ? (panel_pad_kb > kTopPadKb ? kTopPadKb : panel_pad_kb) : kTopPadKb) * 1024;
        p.top_rows = min_of(below_rows, RT_ROWS);
        p.inverses = pknobs.rb_mfma && w == (size_t)BASE_W && !debug;
        if (const size_t nrows = below_rows - p.top_rows) {
            p.below = p.inverses ? PanelBelow::mfma : PanelBelow::valu;
            p.below_grid = (unsigned)ceil_div(nrows, p.inverses ? 16 * RBM_JT : RB_THREADS);
        }
        return p;
    }
    const size_t nbp = ceil_div(below_rows, P2_ROWS);
    if (route.persistent && nbp <= (size_t)PK_MAXB && nbp <= (size_t)site.num_cus && !skip) {
        // one launch factors the panel, interchanges its own columns and leaves the row-move list for the others
        p.kind = PanelKind::persistent;
        p.bstride = nbp <= one_xcd_block_limit(site) ? 8 : 1;
        p.grid = (unsigned)nbp * (unsigned)p.bstride, p.threads = P2_THREADS;
        p.lds_bytes = P2_LDS_DOUBLES * sizeof(double) + (size_t)(panel_pad_kb >= 0 ? panel_pad_kb : kPanelPadKb) * 1024;
        return p;
    }
    const size_t nb = ceil_div(below_rows, PANEL_ROWS);  // one block per PANEL_ROWS rows
    if (nb > (size_t)MAX_PANEL_BLOCKS) return p.unsupported = "lu: more than 65536 rows per panel not supported yet", p;
    static_assert(MAX_PANEL_BLOCKS * PANEL_ROWS == 65536, "the message above names the limit");
    p.kind = PanelKind::columns;
    p.grid = (unsigned)nb, p.threads = PANEL_THREADS;
    p.steps = skip ? 0 : w;
    return p;
}

// split point of a panel wider than BASE_W (getrf_rec): half, rounded up to 16 columns
inline size_t rec_split(size_t w) {
    const size_t h = ((w / 2 + 15) / 16) * 16;
    return h >= w ? w / 2 : h;
}
// split point of a triangular solve wider than the base TRSM_W: whole base blocks on the left
inline size_t trsm_split(size_t w) {
    const size_t h = ((w / 2 + lu_plan::TRSM_W - 1) / lu_plan::TRSM_W) * lu_plan::TRSM_W;
    return h >= w ? w / 2 : h;
}

// ---- one triangular solve of at most TRSM_W rows (launch_trsm_fused) -----------------------------------------------------------------------
enum class TrsmKernel { mfma4, mfma8, two_pass, fused };  // k_trsm_lower_mfma<4|8>, k_trsm_lower_2p, k_trsm_fused
struct TrsmRoute {
    TrsmKernel kernel = TrsmKernel::fused;
    int NC = 1;  // columns a wave solves per pass (two_pass, fused: the template argument, with `threads`); 16 per block for the mfma kernels
    unsigned grid = 0;
    size_t lds_bytes = 0;
};
// mode 0: unit lower, 1: lower, 2: upper.  operands_aligned: T is a diagonal block of the solve-path factorisation in flight and B allows
// 16-byte accesses; inverses_ready: k_rp_top's inverted 16 x 16 blocks exist for all of T (the launcher's questions, it holds the pointers)
inline TrsmRoute plan_trsm(int mode, size_t w, size_t nc, int num_cus, bool in_lookahead, bool inverses_ready, bool operands_aligned) {
    using namespace lu_plan;
    TrsmRoute r;
    if (mode == 0 && operands_aligned && inverses_ready && (w == 64 || w == 128)) {
        // the matrix-core solve with k_rp_top's inverted 16 x 16 blocks
        r.kernel = w == 64 ? TrsmKernel::mfma4 : TrsmKernel::mfma8;
        r.NC = 16, r.grid = (unsigned)ceil_div(nc, 16);
        return r;
    }
    const size_t waves_on_chip = (size_t)num_cus * 4;  // one wave per SIMD
    const bool many = nc > 2 * waves_on_chip;
    r.NC = many ? 4 : 1;  // with 512 threads, else 256
    const size_t per_block = (size_t)(many ? 512 / 64 : 256 / 64) * r.NC;  // columns one block solves per pass
    const size_t want = ceil_div(nc, per_block) < 1 ? 1 : ceil_div(nc, per_block);
    // inside the look-ahead LU a 65..128-wide unit-lower solve takes the two-pass kernel (66 KiB: it shares CUs with the update
    // stream's dgemm blocks, where the 132 KiB one-pass kernel waits for a whole CU)
    if (mode == 0 && w > 64 && in_lookahead) {
        r.kernel = TrsmKernel::two_pass;
        r.lds_bytes = (size_t)64 * TRSM_SW * sizeof(double);
        r.grid = (unsigned)min_of(want, (size_t)num_cus);
        return r;
    }
    r.kernel = TrsmKernel::fused;
    r.lds_bytes = w * (w > 64 ? (size_t)TRSM_SW : (size_t)65) * sizeof(double);
    r.grid = (unsigned)min_of(want, (size_t)num_cus * (w <= 64 ? 2 : 1));
    return r;
}

// ---- the one-level look-ahead driver (getrf_blocked): one step per panel ------------------------------------------------------------------------
struct BlockedStep {
    size_t j = 0, w = 0;      // panel [j, j + w)
    long panel_pad_kb = -1;   // LDS pad of this panel's blocks (plan_base_panel)
    size_t la_w = 0, t0 = 0;  // the main stream updates the next panel's la_w columns; trailing columns [t0, cols)
    bool next_late = false;   // the next panel sits on one XCD: persistent, XCD-avoiding update kernels
    bool split = false;       // the trailing columns go through the third stream in two parts [t0, csplit) | [csplit, cols)
    size_t csplit = 0;
    bool moved = false;       // csplit moved at this step: its first part waits for all of the previous step
    size_t a_end = 0;         // right edge of the previous step's first part
};
struct BlockedPlan {
    // Late phase (the next panel fits one XCD, plan_base_panel places it there): the update stream's dgemm runs as a persistent
    // kernel whose workgroups leave the panel's XCD at once (k_dgemm_w8p), and the panel blocks drop their LDS pad so that
    // such a placeholder can always be scheduled beside them.  The panel chain is the critical path there and everything
    // the update stream does disturbs it (without ANY update work in that phase the solve takes 95.7 instead of 108.4 ms):
    // this keeps the panel's CUs free (no drain before a panel or a 132 KiB triangular solve starts) and its L2 quiet.
    // (Not on the solve path: its panel is one workgroup and k_rp_below's workgroups fit beside a dgemm block, so there is no XCD to
    // keep free; n = 16384: 78.8 -> 76.4 ms without the persistent form.)
    bool late_counters = false;  // the driver allocates the persistent kernels' tile counters and the panel's XCD word
    std::vector<BlockedStep> steps;
};

inline BlockedPlan plan_blocked(size_t rows, size_t cols, size_t kmin, size_t nb, bool fast, const LuSite& site) {
    using namespace lu_plan;
    BlockedPlan plan;
    plan.late_counters = !fast && site.one_xcd_ok;
    const size_t nb_early = kNbEarly < nb ? nb : kNbEarly, nb_late = kNbLate > nb ? nb : kNbLate;
    const auto width_at = [&](size_t j) {
        if (kNbFirst < nb_early && kmin > kEarlyRows + nb_early) {
            if (j == 0) return kNbFirst;
            if (j == kNbFirst) return nb_early - kNbFirst;
        }
        if (kmin - j > kEarlyRows) return nb_early;
        if (kmin - j <= kLateRows) return nb_late;
        return nb;
    };
    size_t a_end = cols, csplit = 0;
    for (size_t j = 0; j < kmin;) {
        BlockedStep st;
        st.j = j;
        st.w = min_of(kmin - j, width_at(j));
        const bool early = kmin - j > kEarlyRows;  // the throughput-bound phase
        // While the trailing matrix is large the machine is throughput bound on the update dgemm (one block per CU: ~50 TFLOP/s
        // in place, 56 alone) and the main stream has slack, so the panel blocks drop their LDS pad there and start beside a
        // dgemm block instead of waiting for a CU to drain (n = 16384: 119.9 -> 118.8 ms).  Letting the update stream drop ITS
        // pad there as well (two dgemm blocks per CU) starves the main stream: a retiring block's slot goes to the next block
        // of the same kernel, stream priority or not (138 ms).  In the late phase (panel on one XCD) the panel blocks drop their pad
        // too, see BlockedPlan.
        const bool late_xcd = plan.late_counters && panel_on_one_xcd(rows, j, site);
        st.panel_pad_kb = (late_xcd || early) ? 0 : -1;
        const size_t next = j + st.w;
        if (next < kmin) st.la_w = min_of(kmin - next, width_at(next));  // there is a next panel
        st.t0 = next + st.la_w;
        st.next_late = plan.late_counters && next < rows && panel_on_one_xcd(rows, next, site);
        st.split = kmin - j > kSplitRows && cols > st.t0 && cols - st.t0 >= kSplitMinCols;
        if (st.split) {
            if (csplit < st.t0 + kSplitMinA || csplit >= cols || (csplit - st.t0) * kSplitShrink < (cols - st.t0)) {
                csplit = st.t0 + (((cols - st.t0) / 2 + kSplitAlign - 1) / kSplitAlign) * kSplitAlign;
                st.moved = true;
            }
            if (csplit >= cols) st.split = false;
        }
        st.csplit = csplit;
        st.a_end = a_end;
        plan.steps.push_back(st);
        a_end = st.split ? csplit : cols;
        j = next;
    }
    return plan;
}

// ---- the two-level driver (getrf_super): super-panels of W columns in panels of nb --------------------------------------------------------------
struct SuperPanel {
    size_t s0, s1, nb;
};
struct SuperStep {
    size_t j, w;      // panel [j, j + w)
    bool boundary;    // the super-panel's last panel
    size_t la_w, t0;  // look-ahead columns [j + w, t0) on the main stream (at a boundary: the next super-panel's first panel)
};
struct SuperPlan {
    std::vector<SuperPanel> panels;
    // incremental block rows of U for the next super-panel's columns (iprep_columns): 12288 40.4-40.8 -> 39.3-39.9 ms with the 512-column
    // plan; with the large-order plan the far stream delivers those columns too late - the mid stream stalls behind the wait and
    // 16384 goes 69.4 -> 73 ms (docs/EXPERIMENTS.md R5 22)
    bool iprep = false;
    bool iprep_split = true;

    bool multi(size_t J) const { return panels[J].s1 - panels[J].s0 > panels[J].nb; }  // more than one panel
    // right edge of the k-th super-panel after J (the last one's where there are fewer)
    size_t s1_after(size_t J, size_t k) const { return panels[lu_plan::min_of(J + k, panels.size() - 1)].s1; }
    // the far stream's first update at boundary J ends here: the columns of the super-panel after next
    size_t far_cut(size_t J, size_t cols) const { return lu_plan::min_of(s1_after(J, 2), cols); }
    // at boundary J with incremental block rows, the mid stream updates [t0, iprep_cut) first: the second panel's columns, which the main
    // stream's next look-ahead update waits for
    size_t iprep_cut(size_t J, size_t t0) const {
        const size_t S1n = s1_after(J, 1);
        if (J + 1 >= panels.size()) return S1n;
        const size_t nbn = panels[J + 1].nb;
        return (iprep_split && t0 + nbn < S1n) ? t0 + nbn : S1n;
    }
    std::vector<SuperStep> steps(size_t J, size_t kmin) const {
        using lu_plan::min_of;
        std::vector<SuperStep> out;
        const size_t S1 = panels[J].s1, nbJ = panels[J].nb;
        for (size_t j = panels[J].s0; j < S1;) {
            const size_t w = min_of(S1 - j, nbJ), next = j + w;
            const bool boundary = next == S1;
            size_t la_w = 0;
            if (next < kmin) la_w = boundary ? min_of(panels[J + 1].s1 - next, panels[J + 1].nb) : min_of(S1 - next, nbJ);
            out.push_back({j, w, boundary, la_w, next + la_w});
            j = next;
        }
        return out;
    }
};

// super-panels (W, nb) from the sequence while more than super_rows rows remain, single `late` panels afterwards
inline SuperPlan plan_super(size_t kmin, const LuProcessKnobs& pknobs) {
    using namespace lu_plan;
    using Seq = std::vector<std::pair<size_t, size_t>>;
    SuperPlan plan;
    const bool large = kmin >= kSuperLargeMin;
    const Seq seq = !pknobs.super_seq.empty() ? pknobs.super_seq
                                              : (large ? Seq{{256, 256}, {1024, 256}, {2048, 256}} : Seq{{512, 512}, {1024, 512}, {2048, 512}});
    const size_t super_rows = pknobs.super_rows >= 0 ? (size_t)pknobs.super_rows : (large ? 4096 : 6144);
    for (size_t s0 = 0, i = 0; s0 < kmin;) {
        const size_t rem = kmin - s0;
        std::pair<size_t, size_t> e = pknobs.super_late;
        if (rem > super_rows) {
            e = seq[min_of(i++, seq.size() - 1)];
            // do not overshoot the switch point by much
            if (e.first > rem - super_rows && rem - super_rows >= e.second) e.first = ceil_div(rem - super_rows, e.second) * e.second;
        }
        const size_t s1 = min_of(s0 + e.first, kmin);
        plan.panels.push_back({s0, s1, min_of(e.second, e.first)});
        s0 = s1;
    }
    plan.iprep = pknobs.iprep >= 0 ? pknobs.iprep != 0 : !large;
    plan.iprep_split = pknobs.iprep_split;
    return plan;
}

// ---- substitution (lu_substitute_device) and the order the solves factor at -------------------------------------------------------------------
enum class SubstForm { chain, pair, rec };  // k_subst_chain per direction; k_trsm_fused + k_rhs_update per block; trsm_*_rec with dgemm
struct SubstRoute {
    SubstForm form = SubstForm::rec;
    size_t nblk = 0;   // chain, pair: blocks of TRSM_W rows
    size_t group = 0;  // chain: right-hand sides per launch
};
// One launch per direction (k_subst_chain) when the system is big enough for the launches to matter and the chain's workgroups (one per
// 128 rows) fit the chip; RMHIP_LU_SUBST=pair keeps the launch-per-block form, and so does a context whose chain timed out once.
inline SubstRoute plan_substitute(size_t n, size_t nrhs, int num_cus, bool subst_pair, bool chain_failed, bool skip16) {
    using namespace lu_plan;
    SubstRoute r;
    if (nrhs > (size_t)RU_MAX_RHS || skip16) return r;
    r.nblk = ceil_div(n, TRSM_W);
    const bool chain = !subst_pair && r.nblk >= kChainMinBlocks && r.nblk <= (size_t)num_cus && !chain_failed;
    r.form = chain ? SubstForm::chain : SubstForm::pair;
    r.group = chain ? kChainGroup : 0;
    return r;
}

// Order the solves factor at.  The blocked driver's trailing updates are whole 128 x 128 x 16 tiles only when n is a multiple of
// 128; otherwise EVERY update of the factorisation runs a guarded kernel (n = 10000: 37.0 ms against 31.7 at 10240, n = 13001: 55.6
// against 47.2 at 13056).  The solves therefore factor [A 0; 0 I] at the next multiple of 128 - 2-4 % more flops, all of them on
// the fast kernels - and drop the padded unknowns (zero).  `lu` itself returns factors of the order it was given.
// pad_knob: RMHIP_LU_PAD (read per call: the tests compare both forms).
inline size_t lu_pad_rows(size_t n, bool pad_knob) {
    using namespace lu_plan;
    if (!pad_knob || n < kPadMin || n % 128 == 0) return n;
    const size_t np = ceil_div(n, 128) * 128;
    return np <= kPadMaxOrder ? np : n;
}

}  // namespace rmhip
