// Host-logic check of the LU dispatch (runmat_amd/csrc/lu_plan.h), the functions the drivers of lu.hip and solve.cpp execute.
//   --table   reads one case per line from stdin and prints what the plan launches for it, one line per case
//             (tests/test_lu_exact_host.py feeds it the tables of tests/test_gpu_lu_exact.py):
//               lu    rows cols mode num_cus <knobs>      a factorisation as `lu` (mode 0) or a solve (mode 1) requests it
//               solve n nrhs num_cus <knobs>              mldivide: padding, factorisation at the padded order, substitution
//             <knobs>: fast lookahead nb panel_columns panel_debug subst_pair pad  super rb_mfma trsm_mfma super_rows iprep  seq late
//             (seq and late as RMHIP_LU_SUPER_SEQ / RMHIP_LU_SUPER_LATE spell them, "-" for unset)
//   --sweep   plans a fixed sweep per rule and prints per group the number of cases and the 64-bit FNV-1a digest of the routes' lines;
//             tests/test_host_plan.py compares with tests/golden/lu_routes.txt, which was taken from the drivers' own conditions before
//             the plan was extracted from them.
//   --dump    the sweep with every route printed under its group's line.
// No GPU needed.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "lu_plan.h"

using namespace rmhip;
using namespace rmhip::lu_plan;

static std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

static const char* name_of(LuDriver d) { return d == LuDriver::rec ? "rec" : (d == LuDriver::blocked ? "blocked" : "super"); }
static const char* name_of(PanelKind k) { return k == PanelKind::top ? "top" : (k == PanelKind::persistent ? "persistent" : "columns"); }
static const char* name_of(PanelBelow b) { return b == PanelBelow::none ? "none" : (b == PanelBelow::mfma ? "mfma" : "valu"); }
static const char* name_of(TrsmKernel k) {
    return k == TrsmKernel::mfma4 ? "mfma4" : (k == TrsmKernel::mfma8 ? "mfma8" : (k == TrsmKernel::two_pass ? "two_pass" : "fused"));
}
static const char* name_of(SubstForm f) { return f == SubstForm::chain ? "chain" : (f == SubstForm::pair ? "pair" : "rec"); }

static std::string line_of(const LuRoute& r) {
    if (r.unsupported) return std::string("unsupported: ") + r.unsupported + "\n";
    return fmt("%s nb=%zu persistent=%d fast=%d linv=%d screen=%d tau=%g\n", name_of(r.driver), r.nb, r.persistent, r.fast, r.use_linv,
               r.screen, r.tau);
}
static std::string line_of(const PanelRoute& p) {
    if (p.unsupported) return std::string("unsupported: ") + p.unsupported + "\n";
    return fmt("%s grid=%u threads=%u lds=%zu bstride=%d top_rows=%zu inverses=%d below=%s below_grid=%u steps=%zu\n", name_of(p.kind), p.grid,
               p.threads, p.lds_bytes, p.bstride, p.top_rows, p.inverses, name_of(p.below), p.below_grid, p.steps);
}
static std::string line_of(const TrsmRoute& t) {
    return fmt("%s NC=%d grid=%u lds=%zu\n", name_of(t.kernel), t.NC, t.grid, t.lds_bytes);
}
static std::string line_of(const BlockedStep& s) {
    return fmt("j=%zu w=%zu pad=%ld la_w=%zu t0=%zu next_late=%d split=%d csplit=%zu moved=%d a_end=%zu\n", s.j, s.w, s.panel_pad_kb,
               s.la_w, s.t0, s.next_late, s.split, s.csplit, s.moved, s.a_end);
}
static std::string lines_of(const BlockedPlan& p) {
    std::string out = fmt("blocked late_counters=%d steps=%zu\n", p.late_counters, p.steps.size());
    for (const BlockedStep& s : p.steps) out += line_of(s);
    return out;
}
static std::string lines_of(const SuperPlan& p, size_t kmin, size_t cols) {
    std::string out = fmt("super panels=%zu iprep=%d\n", p.panels.size(), p.iprep);
    for (size_t J = 0; J < p.panels.size(); ++J) {
        const SuperPanel& sp = p.panels[J];
        out += fmt("J=%zu s0=%zu s1=%zu nb=%zu multi=%d s1n=%zu s1nn=%zu far_cut=%zu\n", J, sp.s0, sp.s1, sp.nb, p.multi(J), p.s1_after(J, 1), p.s1_after(J, 2),
                   p.far_cut(J, cols));
        for (const SuperStep& st : p.steps(J, kmin))
            out += fmt("  j=%zu w=%zu boundary=%d la_w=%zu t0=%zu t1=%zu\n", st.j, st.w, st.boundary, st.la_w, st.t0, st.boundary ? p.iprep_cut(J, st.t0) : 0);
    }
    return out;
}
static std::string line_of(const SubstRoute& s) { return fmt("%s nblk=%zu group=%zu\n", name_of(s.form), s.nblk, s.group); }

// ---- the kernels a factorisation launches, by walking the plans the way the drivers do -----------------------------------------------
// A MODEL of lu.hip's drivers for --table, kept by hand: rec() follows getrf_rec (base case, rec_split, the solve and update between the
// halves), run() follows lu_factor_device's dispatch, getrf_blocked (one panel, then the updates of the look-ahead and the trailing
// columns) and getrf_super (inner panels, the incremental block rows, the boundary's W-wide solve and update).  It records WHICH kernels
// and panel widths occur, not their order, streams or counts.  Approximations: the launcher's test that an operand allows 16-byte
// accesses is taken as "the block's first column is even" (the workspace's leading dimension is even and its base aligned); the solves'
// column counts at a super-panel boundary are those of the whole range, not of each stream's share; row interchanges and dgemm are
// named once wherever a driver may launch them.  A change of a driver's recursion or update structure has to be made here as well -
// getrf_rec, getrf_blocked and getrf_super say so.  The --sweep digests do not go through this model.
struct Walk {
    LuRoute route;
    LuSite site;
    LuProcessKnobs pk;
    bool debug = false;
    size_t rows = 0, cols = 0;
    bool in_lookahead = false;
    long pad_kb = -1;  // LuState::panel_pad_kb as the driver in charge sets it
    std::vector<unsigned char> linv_ok;
    std::set<std::string> seen;
    std::set<size_t> panel_widths;  // of getrf_rec calls made by a driver

    void trsm(size_t j, size_t w, size_t nc) {  // trsm_lower_rec on the diagonal block at column j
        if (w == 0 || nc == 0) return;
        if (w > (size_t)TRSM_W) {
            const size_t h = trsm_split(w);
            trsm(j, h, nc);
            seen.insert("dgemm");
            trsm(j + h, w - h, nc);
            return;
        }
        bool ready = route.use_linv && j % 16 == 0 && (j + w) / 16 <= linv_ok.size();
        for (size_t q = j / 16; ready && q < (j + w) / 16; ++q) ready = linv_ok[q] != 0;
        const TrsmRoute t = plan_trsm(0, w, nc, site.num_cus, in_lookahead, ready, route.use_linv && j % 2 == 0);
        seen.insert(std::string("trsm:") + name_of(t.kernel));
    }
    void laswp() { seen.insert("k_laswp_lists"); }
    bool rec(size_t j0, size_t w) {
        if (w == 0 || j0 >= rows) return true;
        if (w <= (size_t)BASE_W) {
            const PanelRoute p = plan_base_panel(rows, j0, w, route, site, pad_kb, pk, debug);
            if (p.unsupported) return false;
            seen.insert(std::string("panel:") + name_of(p.kind));
            if (p.below != PanelBelow::none) seen.insert(std::string("below:") + name_of(p.below));
            if (p.kind == PanelKind::top && p.inverses && route.use_linv)
                for (size_t q = j0 / 16; q < (j0 + BASE_W) / 16 && q < linv_ok.size(); ++q) linv_ok[q] = 1;
            if (p.bstride > 1) seen.insert("one_xcd");
            laswp();
            return true;
        }
        const size_t h = rec_split(w);
        const size_t hk = (j0 + h <= rows) ? h : (rows - j0);
        if (!rec(j0, h)) return false;
        trsm(j0, hk, w - h);
        if (j0 + h < rows) {
            seen.insert("dgemm");
            if (!rec(j0 + h, w - h)) return false;
        }
        return true;
    }
    bool panel(size_t j, size_t w) {
        panel_widths.insert(w);
        return rec(j, w);
    }
    void update(size_t j, size_t w, size_t c0, size_t c1) {
        if (c1 <= c0) return;
        trsm(j, w, c1 - c0);
        if (j + w < rows) seen.insert("dgemm");
    }
    bool run(size_t kmin) {
        linv_ok.assign(rows / 16 + 8, 0);
        if (route.driver == LuDriver::rec) {
            if (!panel(0, kmin)) return false;
            if (cols > rows) {
                seen.insert("wide_tail");
                trsm(0, rows, cols - rows);
            }
            return true;
        }
        in_lookahead = true;
        if (route.driver == LuDriver::blocked) {
            const BlockedPlan plan = plan_blocked(rows, cols, kmin, route.nb, route.fast, site);
            for (const BlockedStep& st : plan.steps) {
                pad_kb = st.panel_pad_kb;
                if (!panel(st.j, st.w)) return false;
                update(st.j, st.w, st.j + st.w, st.t0);
                update(st.j, st.w, st.t0, cols);
                if (st.split) seen.insert("split");
            }
            return true;
        }
        const SuperPlan plan = plan_super(kmin, pk);
        pad_kb = 0;
        for (size_t J = 0; J < plan.panels.size(); ++J) {
            const SuperPanel& sp = plan.panels[J];
            for (const SuperStep& st : plan.steps(J, kmin)) {
                if (!panel(st.j, st.w)) return false;
                if (!st.boundary) {
                    update(st.j, st.w, st.j + st.w, sp.s1);
                    if (plan.iprep && sp.s1 < plan.s1_after(J, 1)) trsm(st.j, st.w, plan.s1_after(J, 1) - sp.s1);
                } else if (plan.iprep && plan.multi(J)) {
                    trsm(st.j, st.w, plan.s1_after(J, 1) - (st.j + st.w));
                    update(sp.s0, sp.s1 - sp.s0, plan.s1_after(J, 1), cols);
                } else {
                    update(sp.s0, sp.s1 - sp.s0, st.j + st.w, cols);
                }
            }
        }
        return true;
    }
};

struct Knobs {
    LuKnobs k;
    LuProcessKnobs pk;
};

static std::vector<std::pair<size_t, size_t>> parse_seq(const char* v) {  // as lu.hip's knob reader spells RMHIP_LU_SUPER_SEQ
    std::vector<std::pair<size_t, size_t>> out;
    if (!std::strcmp(v, "-")) return out;
    while (v && *v) {
        char* end = nullptr;
        const size_t W = (size_t)std::strtoull(v, &end, 10);
        size_t nb = W;
        if (end && *end == ':') nb = (size_t)std::strtoull(end + 1, &end, 10);
        if (W >= 64) out.emplace_back((W / 64) * 64, nb < 64 ? 64 : (nb / 64) * 64);
        v = end;
        while (v && (*v == ',' || *v == '/' || *v == ' ')) ++v;
        if (!end) break;
    }
    return out;
}

static bool read_knobs(const char* text, Knobs* kn) {
    int fast, la, pc, pd, sp, pad, super, rb, tm, iprep;
    long nb, srows;
    char seq[128], late[64];
    if (std::sscanf(text, "%d %d %ld %d %d %d %d %d %d %d %ld %d %127s %63s", &fast, &la, &nb, &pc, &pd, &sp, &pad, &super, &rb, &tm, &srows, &iprep, seq,
                    late) != 14)
        return false;
    kn->k.fast = fast, kn->k.lookahead = la, kn->k.nb = nb, kn->k.panel_columns = pc, kn->k.panel_debug = pd, kn->k.subst_pair = sp, kn->k.pad = pad;
    kn->pk.super = super, kn->pk.rb_mfma = rb, kn->pk.trsm_mfma = tm, kn->pk.super_rows = srows, kn->pk.iprep = iprep;
    kn->pk.super_seq = parse_seq(seq);
    const auto l = parse_seq(late);
    if (!l.empty()) kn->pk.super_late = l[0];
    return true;
}

static std::string factor_line(size_t rows, size_t cols, int mode, int num_cus, const Knobs& kn) {
    LuProblem p;
    p.rows = rows, p.cols = cols, p.mode = mode;
    LuSite site;
    site.num_cus = num_cus;
    Walk w;
    w.route = plan_lu_factor(p, site, kn.k, kn.pk);
    if (w.route.unsupported) return std::string("unsupported: ") + w.route.unsupported;
    w.site = site, w.pk = kn.pk, w.debug = kn.k.panel_debug, w.rows = rows, w.cols = cols;
    if (!w.run(rows < cols ? rows : cols)) return "unsupported: panel";
    std::string out = fmt("driver=%s nb=%zu fast=%d", name_of(w.route.driver), w.route.nb, w.route.fast);
    out += " widths=";
    for (size_t x : w.panel_widths) out += fmt("%zu,", x);
    for (const std::string& s : w.seen) out += " " + s;
    return out;
}

static int table_mode() {
    char text[1024];
    while (std::fgets(text, sizeof text, stdin)) {
        Knobs kn;
        unsigned long long a, b;
        int mode, cus, used = 0;
        if (std::sscanf(text, "lu %llu %llu %d %d %n", &a, &b, &mode, &cus, &used) == 4 && read_knobs(text + used, &kn)) {
            std::printf("%s\n", factor_line(a, b, mode, cus, kn).c_str());
        } else if (std::sscanf(text, "solve %llu %llu %d %n", &a, &b, &cus, &used) == 3 && read_knobs(text + used, &kn)) {
            const size_t np = lu_pad_rows(a, kn.k.pad);
            const SubstRoute s = plan_substitute(np, b, cus, kn.k.subst_pair, false, false);
            std::printf("order=%zu padded=%d subst=%s groups=%zu %s\n", np, np > a, name_of(s.form), s.form == SubstForm::chain ? (size_t)((b + s.group - 1) / s.group) : (size_t)0,
                        factor_line(np, np, 1, cus, kn).c_str());
        } else {
            std::fprintf(stderr, "bad case line: %s", text);
            return 2;
        }
    }
    return 0;
}

// ---- the sweep ---------------------------------------------------------------------------------------------------------------------------
struct Group {
    bool dump;
    std::string name, all;
    uint64_t h = 1469598103934665603ull;
    unsigned long count = 0;
    Group(bool d, const std::string& n) : dump(d), name(n) {}
    void add(const std::string& what, const std::string& lines) {
        for (unsigned char ch : lines) h = (h ^ ch) * 1099511628211ull;
        ++count;
        if (dump) all += "  " + what + ": " + lines;
    }
    ~Group() {
        std::printf("%s %lu %016llx\n", name.c_str(), count, (unsigned long long)h);
        std::fputs(all.c_str(), stdout);
    }
};

static const int CUS[] = {256, 64, 304};

static void sweep_factor(bool dump) {
    static const size_t KMIN[] = {1, 63, 64, 65, 128, 129, 1151, 1152, 1153, 5119, 5120, 5121, 8191, 8192, 8193, 12287, 12288, 14335, 14336, 16384};
    struct Setting {
        const char* name;
        void (*set)(LuKnobs&, LuProcessKnobs&, LuSite&);
    };
    static const Setting SET[] = {
        {"default", [](LuKnobs&, LuProcessKnobs&, LuSite&) {}},
        {"RMHIP_LU_FAST=0", [](LuKnobs& k, LuProcessKnobs&, LuSite&) { k.fast = false; }},
        {"RMHIP_LU_TAU=2", [](LuKnobs& k, LuProcessKnobs&, LuSite&) { k.tau = 2.0; }},
        {"RMHIP_LU_LOOKAHEAD=0", [](LuKnobs& k, LuProcessKnobs&, LuSite&) { k.lookahead = 0; }},
        {"RMHIP_LU_LOOKAHEAD=1", [](LuKnobs& k, LuProcessKnobs&, LuSite&) { k.lookahead = 1; }},
        {"RMHIP_LU_NB=0", [](LuKnobs& k, LuProcessKnobs&, LuSite&) { k.nb = 0; }},
        {"RMHIP_LU_NB=64", [](LuKnobs& k, LuProcessKnobs&, LuSite&) { k.nb = 64; }},
        {"RMHIP_LU_NB=200", [](LuKnobs& k, LuProcessKnobs&, LuSite&) { k.nb = 200; }},
        {"RMHIP_LU_NB=512", [](LuKnobs& k, LuProcessKnobs&, LuSite&) { k.nb = 512; }},
        {"RMHIP_LU_LOOKAHEAD=1+NB=64", [](LuKnobs& k, LuProcessKnobs&, LuSite&) { k.lookahead = 1, k.nb = 64; }},
        {"RMHIP_LU_PANEL=columns", [](LuKnobs& k, LuProcessKnobs&, LuSite&) { k.panel_columns = true; }},
        {"RMHIP_LU_PANEL_DEBUG=1", [](LuKnobs& k, LuProcessKnobs&, LuSite&) { k.panel_debug = true; }},
        {"RMHIP_LU_SUPER=0", [](LuKnobs&, LuProcessKnobs& p, LuSite&) { p.super = false; }},
        {"RMHIP_LU_TRSM_MFMA=0", [](LuKnobs&, LuProcessKnobs& p, LuSite&) { p.trsm_mfma = false; }},
        {"conservative", [](LuKnobs&, LuProcessKnobs&, LuSite& s) { s.conservative = true; }},
        {"one_xcd_off", [](LuKnobs&, LuProcessKnobs&, LuSite& s) { s.one_xcd_ok = false; }},
    };
    for (const Setting& st : SET)
        for (int cus : CUS) {
            LuKnobs k;
            LuProcessKnobs pk;
            LuSite site;
            site.num_cus = cus;
            st.set(k, pk, site);
            Group g(dump, fmt("factor %s cus=%d", st.name, cus));
            for (size_t kmin : KMIN)
                for (int shape = 0; shape < 3; ++shape)  // square, tall, wide
                    for (int mode = 0; mode < 2; ++mode)
                        for (int deferred = 0; deferred < 2; ++deferred) {
                            LuProblem p;
                            p.rows = shape == 1 ? kmin + 3000 : kmin, p.cols = shape == 2 ? kmin + 3000 : kmin, p.mode = mode, p.deferred_guard = deferred;
                            g.add(fmt("%zu x %zu mode %d deferred %d", p.rows, p.cols, mode, deferred), line_of(plan_lu_factor(p, site, k, pk)));
                        }
            for (int shape = 0; shape < 2; ++shape) {  // the refusal
                LuProblem p;
                p.rows = shape ? 64 : 0x80000000ull, p.cols = shape ? 0x80000000ull : 64;
                g.add(fmt("%zu x %zu", p.rows, p.cols), line_of(plan_lu_factor(p, site, k, pk)));
            }
        }
}

static void sweep_panel(bool dump) {
    static const size_t BELOW[] = {1, 64, 255, 256, 257, 2048, 2049, 8191, 8192, 8193, 9728, 9729, 16384, 16385, 65535, 65536, 65537, 77824, 77825, 100000};
    static const size_t J0[] = {0, 64, 4096};
    static const size_t W[] = {8, 16, 63, 64};
    static const long PAD[] = {-1, 0, 32, 64, 128};
    for (int kind = 0; kind < 3; ++kind)  // the route's panels: solve path, persistent, per column
        for (int xcd = 1; xcd >= 0; --xcd)
            for (int cus : CUS) {
                LuRoute route;
                route.fast = kind == 0, route.persistent = kind != 2;
                LuSite site;
                site.num_cus = cus, site.one_xcd_ok = xcd;
                Group g(dump, fmt("panel %s one_xcd=%d cus=%d", kind == 0 ? "fast" : (kind == 1 ? "persistent" : "columns"), xcd, cus));
                for (size_t below : BELOW)
                    for (size_t j0 : J0)
                        for (size_t w : W)
                            for (long pad : PAD)
                                for (int sw = 0; sw < 4; ++sw) {  // default, RMHIP_LU_RB_MFMA=0, panel debug, RMHIP_LU_SKIP=1
                                    LuProcessKnobs pk;
                                    pk.rb_mfma = sw != 1, pk.skip = sw == 3 ? 1 : 0;
                                    g.add(fmt("rows-j0 %zu j0 %zu w %zu pad %ld sw %d", below, j0, w, pad, sw),
                                          line_of(plan_base_panel(j0 + below, j0, w, route, site, pad, pk, sw == 2)));
                                }
            }
}

static void sweep_trsm(bool dump) {
    static const size_t W[] = {1, 16, 63, 64, 65, 127, 128};
    for (int cus : CUS) {
        Group g(dump, fmt("trsm cus=%d", cus));
        const size_t edge = (size_t)8 * cus;
        const size_t NC[] = {1, 15, 16, 17, 255, 256, 257, edge - 1, edge, edge + 1, 4 * edge, 4 * edge + 1, 100000};
        for (int mode = 0; mode < 3; ++mode)
            for (size_t w : W)
                for (size_t nc : NC)
                    for (int la = 0; la < 2; ++la)
                        for (int ready = 0; ready < 2; ++ready)
                            for (int aligned = 0; aligned < 2; ++aligned)
                                g.add(fmt("mode %d w %zu nc %zu la %d ready %d aligned %d", mode, w, nc, la, ready, aligned),
                                      line_of(plan_trsm(mode, w, nc, cus, la, ready, aligned)));
        for (size_t w : {1, 15, 16, 17, 31, 32, 33, 64, 65, 100, 128, 129, 200, 255, 256, 257, 300, 512, 1000, 2048, 8192})
            g.add(fmt("splits of %zu", w), fmt("rec %zu trsm %zu\n", rec_split(w), trsm_split(w)));
    }
}

static void sweep_blocked(bool dump) {
    struct Case {
        size_t rows, cols, nb;
    };
    static const Case CASES[] = {{300, 300, 64},     {300, 300, 128},     {700, 700, 256},     {1153, 1153, 64},    {1153, 1153, 128},   {2176, 2176, 128},
                                 {5120, 5120, 128},  {8192, 8192, 128},   {8320, 8320, 256},   {10240, 10240, 128}, {10752, 10752, 128}, {11000, 11000, 128},
                                 {12288, 12288, 256}, {16384, 16384, 256}, {16384, 16384, 512}, {16384, 16384, 1024}, {200, 330, 64},      {330, 200, 64},
                                 {9000, 16384, 128}, {16384, 9000, 128}};
    for (int fast = 0; fast < 2; ++fast)
        for (int xcd = 1; xcd >= 0; --xcd)
            for (int cus : CUS) {
                LuSite site;
                site.num_cus = cus, site.one_xcd_ok = xcd;
                Group g(dump, fmt("blocked fast=%d one_xcd=%d cus=%d", fast, xcd, cus));
                for (const Case& c : CASES)
                    g.add(fmt("%zu x %zu nb %zu", c.rows, c.cols, c.nb), lines_of(plan_blocked(c.rows, c.cols, c.rows < c.cols ? c.rows : c.cols, c.nb, fast, site)));
            }
}

static void sweep_super(bool dump) {
    struct Setting {
        const char* name;
        void (*set)(LuProcessKnobs&);
    };
    static const Setting SET[] = {
        {"default", [](LuProcessKnobs&) {}},
        {"alternative", [](LuProcessKnobs& p) { p.super_seq = {{512, 256}, {1024, 256}}, p.super_rows = 2048, p.super_late = {512, 128}; }},
        {"RMHIP_LU_SUPER_ROWS=0", [](LuProcessKnobs& p) { p.super_rows = 0; }},
        {"RMHIP_LU_IPREP=0", [](LuProcessKnobs& p) { p.iprep = 0; }},
        {"RMHIP_LU_IPREP=1", [](LuProcessKnobs& p) { p.iprep = 1; }},
        {"RMHIP_LU_IPREP_SPLIT=0", [](LuProcessKnobs& p) { p.iprep_split = false; }},
    };
    for (const Setting& st : SET) {
        LuProcessKnobs pk;
        st.set(pk);
        Group g(dump, fmt("super %s", st.name));
        for (size_t kmin : {8192, 8200, 10240, 12288, 13001, 14335, 14336, 16384, 20000})
            for (size_t extra : {0, 1, 5000}) g.add(fmt("kmin %zu cols %zu", (size_t)kmin, kmin + extra), lines_of(plan_super(kmin, pk), kmin, kmin + extra));
    }
}

static void sweep_subst(bool dump) {
    for (int cus : CUS) {
        Group g(dump, fmt("subst cus=%d", cus));
        const size_t top = (size_t)128 * cus;
        for (size_t n : {(size_t)1, (size_t)64, (size_t)128, (size_t)383, (size_t)384, (size_t)385, (size_t)512, (size_t)513, (size_t)2176, top - 1, top, top + 1, top + 129})
            for (size_t nrhs = 1; nrhs <= 9; ++nrhs)
                for (int sw = 0; sw < 4; ++sw)  // default, RMHIP_LU_SUBST=pair, after a time-out, RMHIP_LU_SKIP=16
                    g.add(fmt("n %zu nrhs %zu sw %d", n, nrhs, sw), line_of(plan_substitute(n, nrhs, cus, sw == 1, sw == 2, sw == 3)));
    }
    Group g(dump, "pad");
    for (size_t n : {1, 127, 128, 129, 2047, 2048, 2049, 2100, 2176, 4095, 4096, 4097, 10000, 13001, 65407, 65408, 65409, 65535, 65536, 65537, 100000})
        for (int pad = 0; pad < 2; ++pad) g.add(fmt("n %zu pad %d", (size_t)n, pad), fmt("%zu\n", lu_pad_rows(n, pad)));
}

static int sweep_mode(bool dump) {
    sweep_factor(dump);
    sweep_panel(dump);
    sweep_trsm(dump);
    sweep_blocked(dump);
    sweep_super(dump);
    sweep_subst(dump);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--table")) return table_mode();
    if (argc == 2 && !std::strcmp(argv[1], "--sweep")) return sweep_mode(false);
    if (argc == 2 && !std::strcmp(argv[1], "--dump")) return sweep_mode(true);
    std::fprintf(stderr, "usage: lu_route_check --table < cases | --sweep | --dump\n");
    return 2;
}
