// rmhip_ops.cpp -- the operator half of the C ABI (include/rmhip.h): fused elementwise / fused
// reduction dispatch, per-op kernels, reductions, the matmul family, rank / cond / pinv, covariance, transpose, rng, pagefun, modulation.
// The dense solves (lu, mldivide, mrdivide, inv, linsolve, rmhip_blk_*) are solve.cpp.
// Host-side logic mirrors the provider duties of the reference's backends:
//   broadcast shape/stride preparation  backend/wgpu/provider/ops/elementwise.rs:1655-1697
//   reduction geometry handed in by     crates/runmat-vm/src/accel/fusion.rs:540-915 (reduce_len, num_slices)
//   output shapes of the plain reducers crates/runmat-accelerate/src/simple_provider.rs:6728-6806
#include <mutex>
#include <unordered_map>
#include <memory>
#include <string>
#include <algorithm>
#include <functional>
#include <cmath>
#include <cstring>

#include "codegen.h"
#include <limits>

#include "common.h"
#include "host_shape.h"
#include "modulate_check.h"
#include "reduce_plan.h"
#include "wgsl_front.h"

using namespace rmhip;

// (declared in common.h: workload_ops.hip fetches its operands the same way)
int rmhip::get_operand(Context* c, rmhip_buf id, Buffer* out, bool* native) {
    if (*native) {
        RMHIP_TRY(c->get_raw(id, out));
        if (out->dtype == DT_F32 && out->lazy()) {  // materialise the view once, as f32
            RMHIP_TRY(c->settle_view(id));
            RMHIP_TRY(c->get_raw(id, out));
        }
        if (out->dtype == DT_F32 && !out->lazy()) return RMHIP_OK;
        *native = false;
    }
    return c->get(id, out);
}

namespace {

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Operand of a broadcasting elementwise launch (rmhip_binary, rmhip_fused_elementwise): as get_operand, but a repmat view
// stays a view - the launch indexes its base with stride 0 (host_shape.h refined_strides).
int get_bcast_operand(Context* c, rmhip_buf id, Buffer* out, bool* native, bool keep_rng = false) {
    RMHIP_TRY(c->get_raw(id, out, keep_rng));
    if (out->rng_lazy) return RMHIP_OK;  // (f64 contexts only; consumed in registers by the streaming kernel)
    if (out->tview) {
        RMHIP_TRY(c->settle_view(id));
        RMHIP_TRY(c->get_raw(id, out));
    }
    if (*native) {
        if (out->dtype == DT_F32) return RMHIP_OK;
        *native = false;
    }
    if (out->dtype == DT_F64) return RMHIP_OK;
    return c->get(id, out);  // f32 storage read by the f64 variant: tiled (if a view) and widened
}

// refined_strides over Buffers; an operand whose tiling conflicts with another view's is materialised and the preparation repeated
int bcast_prepare(Context* c, const rmhip_buf* ids, std::vector<Buffer>* in, bool f32, const size_t* out_shape, size_t rank,
                  std::vector<uint64_t>* rshape, std::vector<std::vector<uint64_t>>* strides, const char* what) {
    for (size_t attempt = 0; attempt <= in->size(); ++attempt) {
        std::vector<OperandDims> ops(in->size());
        for (size_t k = 0; k < in->size(); ++k) {
            ops[k].shape = (*in)[k].shape;
            ops[k].base = (*in)[k].rep_base;
        }
        size_t bad = 0;
        const int rc = refined_strides(ops, out_shape, rank, rshape, strides, &bad);
        if (rc == 0) return RMHIP_OK;
        if (rc == 1) return fail(RMHIP_ERR_SHAPE, "%s: input %zu does not broadcast to the output shape", what, bad);
        RMHIP_TRY(c->settle_view(ids[bad]));
        if (f32) RMHIP_TRY(c->get_raw(ids[bad], &(*in)[bad]));
        else RMHIP_TRY(c->get(ids[bad], &(*in)[bad]));
    }
    return fail(RMHIP_ERR_UNSUPPORTED, "%s: could not reconcile the operands' tilings", what);
}

// Precision 32: may this product run on the f32 matrix cores (sgemm.hip)?  RMHIP_F32_MATMUL=f64 keeps the widen ->
// dgemm -> round-once path (the CPU's `single` result exactly), which also serves k == 0.  Read per call: tests flip
// the variable.
bool f32_gemm_eligible(const Context* c, size_t m, size_t n, size_t k) {
    (void)m;
    (void)n;
    if (c->precision != 32 || k == 0) return false;
    const char* mode = std::getenv("RMHIP_F32_MATMUL");
    return !(mode && std::strcmp(mode, "f64") == 0);
}

}  // namespace

// ---- parsed-request cache ---------------------------------------------------------------------------
// The planner re-sends the same shader text for every execution of a fusion group; lexing and parsing it
// (2.5-4 KB) cost 7-17 us per call (measured: 13 us for a 3-op request, 23 us for the 14-op chain, against
// 6 us for a per-op call), i.e. more than the kernel at 1024^2.  Parsed programs are immutable and shared.
namespace {
template <typename Prog>
struct ParseCache {
    std::mutex mu;
    std::unordered_map<std::string, std::shared_ptr<const Prog>> map;
    template <typename ParseFn>
    std::shared_ptr<const Prog> get(const char* shader, ParseFn parse, std::string* err) {
        std::string key(shader);
        {
            std::lock_guard<std::mutex> lk(mu);
            auto it = map.find(key);
            if (it != map.end()) return it->second;
        }
        auto prog = std::make_shared<Prog>();
        if (!parse(key, prog.get(), err)) return nullptr;
        std::lock_guard<std::mutex> lk(mu);
        if (map.size() > 4096) map.clear();  // unbounded growth guard; entries are cheap to rebuild
        map.emplace(std::move(key), prog);
        return prog;
    }
};
ParseCache<ElementwiseProgram> g_ew_parse_cache;
ParseCache<ReductionProgram> g_red_parse_cache;
}  // namespace

extern "C" {

int rmhip_wgsl_translate(const char* shader, int kind, char* out, size_t cap, size_t* needed) {
    if (!shader) return fail(RMHIP_ERR_INVALID, "null shader");
    std::string err, src;
    if (kind == 0 || (kind & 0x100)) {
        ElementwiseProgram p;
        if (!parse_elementwise_wgsl(shader, &p, &err)) return fail(RMHIP_ERR_COMPILE, "WGSL front-end: %s", err.c_str());
        if ((kind & 0x100) && p.f32) return fail(RMHIP_ERR_UNSUPPORTED, "lazy random_normal operands are f64 only");
        src = generate_elementwise_source(p, EwTuning::from_env(), 0u, p.f32, (kind & 0x100) ? (unsigned)(kind & 0xff) : 0u);
    } else {
        ReductionProgram p;
        if (!parse_reduction_wgsl(shader, &p, &err)) return fail(RMHIP_ERR_COMPILE, "WGSL front-end: %s", err.c_str());
        src = generate_reduction_source(p, p.f32);
    }
    if (needed) *needed = src.size() + 1;
    if (out && cap) {
        const size_t n = std::min(cap - 1, src.size());
        std::memcpy(out, src.data(), n);
        out[n] = '\0';
    }
    return RMHIP_OK;
}

int rmhip_wgsl_compile_check(const char* shader, int kind) {
    if (!shader) return fail(RMHIP_ERR_INVALID, "null shader");
    std::string err, src;
    if (kind == 0 || (kind & 0x100)) {
        ElementwiseProgram p;
        if (!parse_elementwise_wgsl(shader, &p, &err)) return fail(RMHIP_ERR_COMPILE, "WGSL front-end: %s", err.c_str());
        if ((kind & 0x100) && p.f32) return fail(RMHIP_ERR_UNSUPPORTED, "lazy random_normal operands are f64 only");
        src = generate_elementwise_source(p, EwTuning::from_env(), 0u, p.f32, (kind & 0x100) ? (unsigned)(kind & 0xff) : 0u);
    } else {
        ReductionProgram p;
        if (!parse_reduction_wgsl(shader, &p, &err)) return fail(RMHIP_ERR_COMPILE, "WGSL front-end: %s", err.c_str());
        src = generate_reduction_source(p, p.f32);
    }
    std::vector<char> code;
    return compile_to_code_object(src, &code);
}

int rmhip_fused_elementwise(rmhip_ctx* ctx, const char* shader, const rmhip_buf* inputs, size_t n_in,
                            const size_t* out_shape, size_t rank, size_t len, size_t n_out, rmhip_buf* out_ids) {
    CTX_OR_FAIL(ctx);
    ScopedTimer timer(&c->tel.fused_elementwise_count, &c->tel.fused_elementwise_ns);
    if (!shader || !inputs || !out_ids || (rank && !out_shape)) return fail(RMHIP_ERR_INVALID, "fused_elementwise: null argument");
    if (n_in == 0) return fail(RMHIP_ERR_INVALID, "fused_elementwise: no inputs");  // elementwise.rs:1574
    if (n_in > 24) return fail(RMHIP_ERR_UNSUPPORTED, "fused_elementwise: more than 24 inputs");
    if (rank > 8 + 8) return fail(RMHIP_ERR_UNSUPPORTED, "fused_elementwise: rank too large");
    if (shape_numel(out_shape, rank) != len) return fail(RMHIP_ERR_SHAPE, "fused_elementwise: len %zu != prod(output_shape)", len);
    if (len == 0) return fail(RMHIP_ERR_UNSUPPORTED, "fusion: zero-length execution not supported");  // fusion_exec.rs:273
    std::string err;
    const std::shared_ptr<const ElementwiseProgram> prog_ptr = g_ew_parse_cache.get(shader, parse_elementwise_wgsl, &err);
    if (!prog_ptr) return fail(RMHIP_ERR_COMPILE, "WGSL front-end: %s", err.c_str());
    const ElementwiseProgram& prog = *prog_ptr;
    if ((size_t)prog.n_inputs != n_in) return fail(RMHIP_ERR_INVALID, "fused_elementwise: shader binds %d inputs, got %zu", prog.n_inputs, n_in);
    if (prog.outputs.size() != n_out) return fail(RMHIP_ERR_INVALID, "fused_elementwise: shader writes %zu outputs, caller expects %zu", prog.outputs.size(), n_out);

    if (prog.f32 != (c->precision == 32))
        return fail(RMHIP_ERR_COMPILE, "%s shader handed to an %s provider (precision() is %s)", prog.f32 ? "f32" : "f64",
                    c->precision == 32 ? "F32" : "F64", c->precision == 32 ? "F32" : "F64");
    std::vector<Buffer> in(n_in);
    std::vector<uint64_t> oshape(out_shape, out_shape + rank);
    std::vector<std::vector<uint64_t>> strides(n_in);
    // Lazy random_normal operands (Buffer::rng_lazy) stay lazy only for the streaming kernel over 16-byte vectors: every operand is
    // either a plain full-size tensor of the output's shape or a 1-element tensor.  Any other request materialises them first.
    unsigned rng_mask = 0;
    if (c->precision != 32 && c->n_rng_lazy != 0) {  // (no lazy record alive in this context: nothing to look for)
        bool any = false, eligible = len >= 2;
        auto extents = [](const std::vector<size_t>& sh) {
            std::vector<size_t> e;
            for (size_t d : sh)
                if (d != 1) e.push_back(d);
            return e;
        };
        const std::vector<size_t> want = extents(std::vector<size_t>(out_shape, out_shape + rank));
        for (size_t k = 0; k < n_in; ++k) {
            RMHIP_TRY(c->get_raw(inputs[k], &in[k], /*keep_rng=*/true));
            any |= in[k].rng_lazy;
        }
        if (any) {
            for (size_t k = 0; k < n_in && eligible; ++k) {
                const Buffer& b = in[k];
                const bool full = b.numel == len && extents(b.shape) == want;
                if (b.rng_lazy) eligible = full;
                else eligible = !b.lazy() && b.dtype == DT_F64 && (b.numel == 1 || (full && aligned16(b.data())));
            }
            for (size_t k = 0; k < n_in; ++k) {
                if (!in[k].rng_lazy) continue;
                if (eligible) rng_mask |= 1u << k;
                else RMHIP_TRY(c->settle_rng(inputs[k]));
            }
        }
        for (auto& b : in) b = Buffer();
    }
    // f32 storage is read and written in place by the f32 variant of the generated kernel; a mixed operand list
    // (externally wrapped f64 memory, transpose views) runs the f64 variant on widened copies
    bool f32 = c->precision == 32;
    size_t tried = 0;  // when the native attempt gives up at operand tried - 1, that one already holds its f64 copy
    // repmat views are read in place (stride 0 over their base)
    for (; tried < n_in && f32; ++tried) RMHIP_TRY(get_bcast_operand(c, inputs[tried], &in[tried], &f32));
    for (size_t k = 0; k < n_in; ++k)
        if (!f32 && (k + 1 != tried || in[k].dtype == DT_F32)) {
            bool no = false;
            RMHIP_TRY(get_bcast_operand(c, inputs[k], &in[k], &no, (rng_mask >> k) & 1u));
        }
    RMHIP_TRY(bcast_prepare(c, inputs, &in, f32, out_shape, rank, &oshape, &strides, "fused_elementwise"));
    RMHIP_TRACEF("fused_elementwise: operands ready (f32 storage path %d)", (int)f32);
    collapse(&oshape, &strides);
    const size_t crank = oshape.size();
    if (crank > 8) return fail(RMHIP_ERR_UNSUPPORTED, "fused_elementwise: broadcast rank %zu > 8 after collapsing", crank);

    bool fast = crank == 1;
    unsigned mask = 0;
    if (fast)
        for (size_t k = 0; k < n_in; ++k)
            if (strides[k][0] == 0) mask |= 1u << k;
    if (!fast) mask = 0;
    if (rng_mask && !fast) {  // (not expected after the eligibility test above: materialise and run the request again)
        for (size_t k = 0; k < n_in; ++k)
            if ((rng_mask >> k) & 1u) RMHIP_TRY(c->settle_rng(inputs[k]));
        return rmhip_fused_elementwise(ctx, shader, inputs, n_in, out_shape, rank, len, n_out, out_ids);
    }

    std::shared_ptr<FusedKernel> kern;
    RMHIP_TRY(get_elementwise_kernel(c, prog, mask, f32, &kern, rng_mask));
    RMHIP_TRACEF("fused_elementwise: kernel ready (fast %d mask %x)", (int)fast, mask);

    std::vector<Buffer> outs(n_out);
    std::vector<rmhip_buf> ids(n_out, 0);
    for (size_t k = 0; k < n_out; ++k) {
        int rc = f32 ? c->new_buffer_f32(out_shape, rank, &ids[k], &outs[k]) : c->new_buffer(out_shape, rank, &ids[k], &outs[k]);
        if (rc != RMHIP_OK) {
            for (size_t j = 0; j < k; ++j) rmhip_free(ctx, ids[j]);
            return rc;
        }
    }

    std::vector<const double*> in_ptr(n_in);
    std::vector<double*> out_ptr(n_out);
    for (size_t k = 0; k < n_in; ++k) in_ptr[k] = in[k].data();
    for (size_t k = 0; k < n_out; ++k) out_ptr[k] = outs[k].data();
    std::vector<void*> args;
    std::vector<unsigned long long> rng_states(n_in, 0);
    for (size_t k = 0; k < n_in; ++k) {
        rng_states[k] = in[k].rng_state;
        if ((rng_mask >> k) & 1u) args.push_back(&rng_states[k]);  // the stream state the tensor was drawn at, by value
        else args.push_back(&in_ptr[k]);
    }
    for (size_t k = 0; k < n_out; ++k) args.push_back(&out_ptr[k]);
    unsigned long long rng_jm = 1, rng_jp = 0;

    const EwTuning& t = kern->tuning;
    hipError_t e;
    hipFunction_t fn = nullptr;          // the form launched, by the function itself: the record below names what ran
    uint64_t grid_blocks = 0, unroll = 1;
    if (fast) {
        bool vec_ok = true;
        for (size_t k = 0; k < n_in; ++k)
            if (!((mask >> k) & 1u) && !((rng_mask >> k) & 1u) && !aligned16(in_ptr[k])) vec_ok = false;
        for (size_t k = 0; k < n_out; ++k)
            if (!aligned16(out_ptr[k])) vec_ok = false;
        unsigned long long n = len;
        args.push_back(&n);
        const size_t work = vec_ok ? len / (f32 ? 4 : 2) : len;
        int n_stream = 0;
        for (size_t k = 0; k < n_in; ++k) n_stream += ((mask >> k) & 1u) ? 0 : 1;
        unroll = (uint64_t)t.unroll_for(n_stream, program_is_heavy(prog));
        const size_t per_block = (size_t)t.block * unroll;
        size_t want = (work + per_block - 1) / per_block;
        // a kernel that generates normals is VALU-bound and pays a skip-ahead + 10 KiB of table staging per block: one resident set of
        // blocks (2048 threads per CU) walks the tensor instead of blocks_per_cu waves of them
        const size_t cap = rng_mask ? (size_t)c->num_cus * std::max(1, 2048 / t.block) : (size_t)c->num_cus * t.blocks_per_cu;
        if (want < 1) want = 1;
        const unsigned grid = (unsigned)std::min(want, cap);
        if (rng_mask) {
            if (!vec_ok) {  // (outputs are fresh allocations and the inputs were tested above)
                for (size_t k = 0; k < n_out; ++k) rmhip_free(ctx, ids[k]);
                return fail(RMHIP_ERR_HIP, "fused_elementwise: unaligned buffer beside a lazy random_normal operand");
            }
            // one 16-byte vector is one Box-Muller pair (two draws): the thread's state jumps 2 * grid * block steps per iteration
            lcg_jump_host(2ull * grid * (unsigned long long)t.block, &rng_jm, &rng_jp);
            args.push_back(&rng_jm);
            args.push_back(&rng_jp);
            for (size_t k = 0; k < n_in; ++k) c->lazy_randn_fused += (rng_mask >> k) & 1u;
        }
        fn = vec_ok ? kern->fn_fast : kern->fn_fast1;
        grid_blocks = grid;
        e = hipModuleLaunchKernel(fn, grid, 1, 1, t.block, 1, 1, 0, c->stream, args.data(), nullptr);
    } else {
        std::vector<unsigned long long> p(11 + 8 * n_in, 0);
        const unsigned long long d0 = oshape[0];
        const unsigned long long per_block = (unsigned long long)t.bcast_block * t.bcast_elems;
        const unsigned long long nchunks = (d0 + per_block - 1) / per_block;
        unsigned long long outer = 1;
        p[0] = d0;
        p[1] = nchunks;
        p[2] = crank;
        for (size_t d = 0; d < 8; ++d) p[3 + d] = d < crank ? oshape[d] : 1;
        for (size_t d = 1; d < crank; ++d) outer *= oshape[d];
        for (size_t k = 0; k < n_in; ++k)
            for (size_t d = 0; d < crank; ++d) p[11 + 8 * k + d] = strides[k][d];
        args.push_back(p.data());
        if (d0 < 128 && outer >= 64 && len < 0x80000000ULL) {  // short dim 0, many outer indices: flat threads (32-bit index + stride cannot wrap below 2^31)
            unsigned n32 = (unsigned)len;
            args.push_back(&n32);
            const unsigned long long want = (len + 255) / 256, cap = (unsigned long long)c->num_cus * 16;
            fn = kern->fn_bcast_flat;
            grid_blocks = std::min(want, cap);
            e = hipModuleLaunchKernel(fn, (unsigned)grid_blocks, 1, 1, 256, 1, 1, 0, c->stream, args.data(), nullptr);
        } else {
            const unsigned long long blocks = nchunks * outer;
            const unsigned long long gx = std::min<unsigned long long>(blocks, 1048576ULL);
            const unsigned long long gy = (blocks + gx - 1) / gx;
            if (gy > 65535ULL) {
                for (size_t k = 0; k < n_out; ++k) rmhip_free(ctx, ids[k]);
                return fail(RMHIP_ERR_UNSUPPORTED, "fused_elementwise: broadcast grid too large");
            }
            fn = kern->fn_bcast;
            grid_blocks = gx * gy;
            e = hipModuleLaunchKernel(fn, (unsigned)gx, (unsigned)gy, 1, t.bcast_block, 1, 1, 0, c->stream, args.data(), nullptr);
        }
    }
    if (e != hipSuccess) {
        for (size_t k = 0; k < n_out; ++k) rmhip_free(ctx, ids[k]);
        return fail(RMHIP_ERR_HIP, "fused_elementwise launch: %s", hipGetErrorString(e));
    }
    c->tel.kernel_launches++;
    // form: 0 rm_ew_fast, 1 rm_ew_fast1, 2 rm_ew_bcast, 3 rm_ew_bcast_flat; grid: blocks launched (gx * gy for rm_ew_bcast);
    // unroll: the streaming forms' vectors per thread and trip
    const uint64_t form = fn == kern->fn_fast ? 0 : fn == kern->fn_fast1 ? 1 : fn == kern->fn_bcast ? 2 : 3;
    const uint64_t wg = fast ? t.block : fn == kern->fn_bcast ? t.bcast_block : 256;
    if (n_out == 1)
        c->record_launch("fused_elementwise", {{"len", len}, {"inputs", n_in}, {"rank", rank}},
                         {{"wg", wg}, {"form", form}, {"grid", grid_blocks}, {"unroll", unroll}});
    else
        c->record_launch("fused_elementwise_multi", {{"len", len}, {"inputs", n_in}, {"rank", rank}, {"num_outputs", n_out}},
                         {{"wg", wg}, {"form", form}, {"grid", grid_blocks}, {"unroll", unroll}});
    for (size_t k = 0; k < n_out; ++k) out_ids[k] = ids[k];
    RMHIP_TRACEF("fused_elementwise: launched");
    return RMHIP_OK;
}

int rmhip_fused_reduction(rmhip_ctx* ctx, const char* shader, const rmhip_buf* inputs, size_t n_in,
                          const size_t* out_shape, size_t rank, size_t reduce_len, size_t num_slices,
                          uint32_t workgroup_size, int flavor, double custom_scale, rmhip_buf* out) {
    (void)workgroup_size;
    CTX_OR_FAIL(ctx);
    ScopedTimer timer(&c->tel.fused_reduction_count, &c->tel.fused_reduction_ns);
    if (!shader || !inputs || !out) return fail(RMHIP_ERR_INVALID, "fused_reduction: null argument");
    if (n_in == 0 || n_in > 24) return fail(RMHIP_ERR_UNSUPPORTED, "fused_reduction: unsupported input count %zu", n_in);
    if (reduce_len * num_slices == 0) return fail(RMHIP_ERR_UNSUPPORTED, "fusion: zero-length execution not supported");  // fusion_exec.rs:489
    if (shape_numel(out_shape, rank) != num_slices)
        return fail(RMHIP_ERR_SHAPE, "fused_reduction: prod(output_shape) != num_slices %zu", num_slices);
    if (flavor < RMHIP_FLAVOR_SUM || flavor > RMHIP_FLAVOR_CUSTOM_SCALE) return fail(RMHIP_ERR_INVALID, "fused_reduction: bad flavor %d", flavor);
    std::string err;
    const std::shared_ptr<const ReductionProgram> prog_ptr = g_red_parse_cache.get(shader, parse_reduction_wgsl, &err);
    if (!prog_ptr) return fail(RMHIP_ERR_COMPILE, "WGSL front-end: %s", err.c_str());
    const ReductionProgram& prog = *prog_ptr;
    if ((size_t)prog.n_inputs != n_in) return fail(RMHIP_ERR_INVALID, "fused_reduction: shader binds %d inputs, got %zu", prog.n_inputs, n_in);

    if (prog.f32 != (c->precision == 32))
        return fail(RMHIP_ERR_COMPILE, "%s shader handed to an %s provider (precision() is %s)", prog.f32 ? "f32" : "f64",
                    c->precision == 32 ? "F32" : "F64", c->precision == 32 ? "F32" : "F64");
    const size_t total = reduce_len * num_slices;
    std::vector<Buffer> in(n_in);
    std::vector<unsigned long long> mult(n_in);
    bool f32 = c->precision == 32;  // f32 operands are read in place, partials and the result are f64 (narrowed on return)
    size_t tried = 0;
    for (; tried < n_in && f32; ++tried) RMHIP_TRY(get_operand(c, inputs[tried], &in[tried], &f32));
    for (size_t k = 0; k < n_in; ++k) {
        if (!f32 && k + 1 != tried) RMHIP_TRY(c->get(inputs[k], &in[k]));
        if (in[k].numel == total) mult[k] = 1;
        else if (in[k].numel == 1) mult[k] = 0;  // scalar operand uploaded as a 1-element tensor (fusion_exec.rs:522-543)
        else return fail(RMHIP_ERR_SHAPE, "fused_reduction: input %zu has %zu elements, expected %zu", k, in[k].numel, total);
    }
    std::shared_ptr<FusedKernel> kern;
    RMHIP_TRY(get_reduction_kernel(c, prog, f32, &kern));

    // axis 0: slice s is contiguous (pre=1, red, post=slices); axis 1: element (s, r) at s + r*slices.
    const size_t pre = prog.axis == 0 ? 1 : num_slices;
    const size_t post = prog.axis == 0 ? num_slices : 1;
    std::vector<const double*> in_ptr(n_in);
    std::vector<void*> args;
    for (size_t k = 0; k < n_in; ++k) {
        in_ptr[k] = in[k].data();
        args.push_back(&in_ptr[k]);
        args.push_back(&mult[k]);
    }
    // the 16-byte forms need every full-size input aligned to its pair
    bool pairs_ok = true;
    for (size_t k = 0; k < n_in && pairs_ok; ++k)
        if (mult[k] && (((uintptr_t)in_ptr[k]) & (f32 ? 7u : 15u)) != 0) pairs_ok = false;
    // which generated kernel on which grid, how many partials per slice, which finalize: reduce_plan.h route_reduction
    const ReduceRoute rt = route_reduction(pre, reduce_len, post, c->num_cus, c->num_xcc, f32 ? 4u : 8u, pairs_ok, REDUCE_GENERATED);
    if (!rt.valid) return fail(RMHIP_ERR_UNSUPPORTED, "fused_reduction: geometry exceeds launch limits");
    const size_t nparts = (size_t)(rt.nslices * rt.nsplit);
    RMHIP_TRY(c->ensure_scratch(2 * nparts * sizeof(double)));
    double* pv = c->scratch;
    double* pn = c->scratch + nparts;

    Buffer ob;
    rmhip_buf oid = 0;
    RMHIP_TRY(c->new_buffer(out_shape, rank, &oid, &ob));

    unsigned long long u_pre = pre, u_red = reduce_len, u_nsplit = rt.nsplit, u_nslices = rt.nslices;
    int tx = (int)rt.span;
    unsigned win = rt.span;
    hipFunction_t fn = nullptr;
    switch (rt.kernel) {
        case ReduceKernel::CONTIG:
        case ReduceKernel::CONTIG_V2:  // two adjacent elements per call of the value functor (+12-18 % on plain tensors; the Monte-Carlo payoff sum 160 -> us)
            fn = rt.kernel == ReduceKernel::CONTIG ? kern->fn_contig : kern->fn_contig2;
            args.insert(args.end(), {&u_red, &u_nslices, &u_nsplit, &pv, &pn});
            break;
        case ReduceKernel::STRIDED:
            fn = kern->fn_strided;
            args.insert(args.end(), {&u_pre, &u_red, &u_nsplit, &tx, &pv, &pn});
            break;
        case ReduceKernel::STRIDED_V2:  // two adjacent slices per thread
            fn = kern->fn_strided2;
            args.insert(args.end(), {&u_pre, &u_red, &u_nsplit, &win, &pv, &pn});
            break;
        default:
            rmhip_free(ctx, oid);
            return fail(RMHIP_ERR_UNSUPPORTED, "fused_reduction: no generated kernel for route %s", reduce_kernel_name(rt.kernel));
    }
    hipError_t e = hipModuleLaunchKernel(fn, rt.gx, rt.gy, rt.gz, rt.block, 1, 1, 0, c->stream, args.data(), nullptr);
    if (e == hipSuccess) {
        const double* cpv = pv;
        const double* cpn = pn;
        int mean = flavor == RMHIP_FLAVOR_MEAN ? 1 : 0;
        int omit = prog.omitnan ? 1 : 0;
        double scale = flavor == RMHIP_FLAVOR_CUSTOM_SCALE ? custom_scale : 1.0;
        double* optr = ob.data();
        void* fargs[] = {&cpv, &cpn, &u_nslices, &u_nsplit, &u_red, &mean, &omit, &scale, &optr};
        if (rt.flat_final) {
            e = hipModuleLaunchKernel(kern->fn_final_flat, (unsigned)ceil_div_u64(rt.nslices, 256), 1, 1, 256, 1, 1, 0, c->stream, fargs, nullptr);
        } else {
            const unsigned fb = (unsigned)ceil_div_u64(rt.nslices, 4);
            e = hipModuleLaunchKernel(kern->fn_final, fb, 1, 1, 256, 1, 1, 0, c->stream, fargs, nullptr);
        }
    }
    if (e != hipSuccess) {
        rmhip_free(ctx, oid);
        return fail(RMHIP_ERR_HIP, "fused_reduction launch: %s", hipGetErrorString(e));
    }
    c->tel.kernel_launches += 2;
    c->record_launch("fused_reduction", {{"reduce_len", reduce_len}, {"slices", num_slices}, {"rank", rank}},
                     {{"wg", (uint64_t)(pre == 1 ? rt.block : 256)}, {"flavor", (uint64_t)flavor}});
    *out = oid;
    return RMHIP_OK;
}

int rmhip_unary(rmhip_ctx* ctx, int op, rmhip_buf a, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (op < 0 || op >= RMHIP_UNARY_OP_COUNT) return fail(RMHIP_ERR_UNSUPPORTED, "unary op %d not supported by provider", op);
    Buffer ab, ob;
    bool f32 = c->precision == 32;
    RMHIP_TRY(get_operand(c, a, &ab, &f32));
    int rc;
    if (f32) {
        RMHIP_TRY(c->new_buffer_f32(ab.shape.data(), ab.shape.size(), out, &ob));
        rc = launch_unary_f32(c, op, ab.data_f32(), ob.data_f32(), ab.numel);
    } else {
        RMHIP_TRY(c->new_buffer(ab.shape.data(), ab.shape.size(), out, &ob));
        rc = launch_unary(c, op, ab.data(), ob.data(), ab.numel);
    }
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

int rmhip_scalar(rmhip_ctx* ctx, int op, rmhip_buf a, double s, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (op < 0 || op >= RMHIP_SCALAR_OP_COUNT) return fail(RMHIP_ERR_UNSUPPORTED, "scalar op %d not supported by provider", op);
    Buffer ab, ob;
    bool f32 = c->precision == 32;
    RMHIP_TRY(get_operand(c, a, &ab, &f32));
    int rc;
    if (f32) {
        RMHIP_TRY(c->new_buffer_f32(ab.shape.data(), ab.shape.size(), out, &ob));
        rc = launch_scalar_f32(c, op, ab.data_f32(), s, ob.data_f32(), ab.numel);
    } else {
        RMHIP_TRY(c->new_buffer(ab.shape.data(), ab.shape.size(), out, &ob));
        rc = launch_scalar(c, op, ab.data(), s, ob.data(), ab.numel);
    }
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

int rmhip_binary(rmhip_ctx* ctx, int op, rmhip_buf a, rmhip_buf b, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (op < 0 || op >= RMHIP_BINARY_OP_COUNT) return fail(RMHIP_ERR_UNSUPPORTED, "binary op %d not supported by provider", op);
    Buffer ab, bb, ob;
    bool f32 = c->precision == 32;
    // repmat views stay views: the reference's callers expand with `repmat`, call `elem_*`, free (times.rs:501-543)
    RMHIP_TRY(get_bcast_operand(c, a, &ab, &f32));
    RMHIP_TRY(get_bcast_operand(c, b, &bb, &f32));
    if (!f32 && ab.dtype == DT_F32) RMHIP_TRY(c->get(a, &ab));  // b turned out not to be plain f32 storage
    // broadcast_shapes (broadcast.rs:8-47): front-pad, extents equal or 1
    const size_t rank = std::max(ab.shape.size(), bb.shape.size());
    if (rank > 16) return fail(RMHIP_ERR_UNSUPPORTED, "binary: rank too large");
    std::vector<size_t> oshape(rank);
    for (size_t d = 0; d < rank; ++d) {
        const size_t ea = d < rank - ab.shape.size() ? 1 : ab.shape[d - (rank - ab.shape.size())];
        const size_t eb = d < rank - bb.shape.size() ? 1 : bb.shape[d - (rank - bb.shape.size())];
        if (ea == eb) oshape[d] = ea;
        else if (ea == 1) oshape[d] = eb;
        else if (eb == 1) oshape[d] = ea;
        else
            return fail(RMHIP_ERR_SHAPE, "size mismatch between inputs (dimension %zu has lengths %zu and %zu)", d + 1, ea, eb);
    }
    if (f32) RMHIP_TRY(c->new_buffer_f32(oshape.data(), rank, out, &ob));
    else RMHIP_TRY(c->new_buffer(oshape.data(), rank, out, &ob));
    int rc;
    if (ab.numel == ob.numel && bb.numel == ob.numel && ab.rep_base.empty() && bb.rep_base.empty()) {
        rc = f32 ? launch_binary_same_f32(c, op, ab.data_f32(), bb.data_f32(), ob.data_f32(), ob.numel)
                 : launch_binary_same(c, op, ab.data(), bb.data(), ob.data(), ob.numel);
    } else {
        std::vector<std::vector<uint64_t>> strides;
        std::vector<uint64_t> os;
        const rmhip_buf ids[2] = {a, b};
        std::vector<Buffer> in = {ab, bb};
        rc = bcast_prepare(c, ids, &in, f32, oshape.data(), rank, &os, &strides, "binary");
        if (rc) {
            rmhip_free(ctx, *out);
            return rc;
        }
        ab = in[0];
        bb = in[1];
        collapse(&os, &strides);
        if (os.size() > 8) {
            rmhip_free(ctx, *out);
            return fail(RMHIP_ERR_UNSUPPORTED, "binary: broadcast rank %zu > 8 after collapsing", os.size());
        }
        BroadcastDesc d{};
        d.rank = (int)os.size();
        for (size_t i = 0; i < os.size(); ++i) {
            d.out_shape[i] = os[i];
            d.stride_a[i] = strides[0][i];
            d.stride_b[i] = strides[1][i];
        }
        rc = f32 ? launch_binary_bcast_f32(c, op, ab.data_f32(), bb.data_f32(), ob.data_f32(), ob.numel, d)
                 : launch_binary_bcast(c, op, ab.data(), bb.data(), ob.data(), ob.numel, d);
    }
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

// ---- complex operands of the same hooks (complex_ew.hip).  Everything that can refuse does so before the output is created. ----------
int rmhip_complex_unary(rmhip_ctx* ctx, int op, rmhip_buf a, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (op < 0 || op >= RMHIP_COMPLEX_UNARY_OP_COUNT) return fail(RMHIP_ERR_UNSUPPORTED, "complex unary op %d not supported by provider", op);
    Buffer ab, ob;
    RMHIP_TRY(c->lookup(a, &ab));
    if (!ab.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "complex_unary: tensor %llu is real (rmhip_unary / rmhip_real_part serve it)", (unsigned long long)a);
    const bool real_result = complex_unary_is_real(op), f32 = real_result && c->precision == 32;
    if (!real_result) RMHIP_TRY(c->new_buffer_complex(ab.shape.data(), ab.shape.size(), out, &ob));
    else if (f32) RMHIP_TRY(c->new_buffer_f32(ab.shape.data(), ab.shape.size(), out, &ob));
    else RMHIP_TRY(c->new_buffer(ab.shape.data(), ab.shape.size(), out, &ob));
    const int rc = launch_complex_unary(c, op, ab.data(), ob.data(), f32, ab.numel);
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

int rmhip_complex_scalar(rmhip_ctx* ctx, int op, rmhip_buf a, double s, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (op < RMHIP_SADD || op > RMHIP_SRDIV) return fail(RMHIP_ERR_UNSUPPORTED, "scalar op %d is not served for complex operands", op);
    Buffer ab, ob;
    RMHIP_TRY(c->lookup(a, &ab));
    if (!ab.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "complex_scalar: tensor %llu is real (rmhip_scalar serves it)", (unsigned long long)a);
    RMHIP_TRY(c->new_buffer_complex(ab.shape.data(), ab.shape.size(), out, &ob));
    static const int kBinary[6] = {RMHIP_ADD, RMHIP_SUB, RMHIP_MUL, RMHIP_DIV, RMHIP_SUB, RMHIP_DIV};
    const bool reversed = op == RMHIP_SRSUB || op == RMHIP_SRDIV;  // s - z, s ./ z: the scalar is the left operand
    const int rc = reversed ? launch_complex_binary_same(c, kBinary[op], 2, nullptr, false, ab.data(), true, s, ob.data(), ob.numel)
                            : launch_complex_binary_same(c, kBinary[op], 1, ab.data(), true, nullptr, false, s, ob.data(), ob.numel);
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

int rmhip_complex_binary(rmhip_ctx* ctx, int op, rmhip_buf a, rmhip_buf b, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (op < RMHIP_ADD || op > RMHIP_DIV) return fail(RMHIP_ERR_UNSUPPORTED, "binary op %d is not served for complex operands", op);
    Buffer ab, bb, ob;
    RMHIP_TRY(c->lookup(a, &ab));
    RMHIP_TRY(c->lookup(b, &bb));
    if (!ab.cplx && !bb.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "complex_binary: both operands are real (rmhip_binary serves them)");
    // a real operand as plain f64: a lazy view is materialised, f32 storage widened
    if (!ab.cplx) RMHIP_TRY(c->get(a, &ab));
    if (!bb.cplx) RMHIP_TRY(c->get(b, &bb));
    const int kind = ab.cplx && bb.cplx ? 0 : (ab.cplx ? 1 : 2);
    // broadcast_shapes (broadcast.rs:8-47), as rmhip_binary
    const size_t rank = std::max(ab.shape.size(), bb.shape.size());
    if (rank > 16) return fail(RMHIP_ERR_UNSUPPORTED, "binary: rank too large");
    std::vector<size_t> oshape(rank);
    for (size_t d = 0; d < rank; ++d) {
        const size_t ea = d < rank - ab.shape.size() ? 1 : ab.shape[d - (rank - ab.shape.size())];
        const size_t eb = d < rank - bb.shape.size() ? 1 : bb.shape[d - (rank - bb.shape.size())];
        if (ea == eb) oshape[d] = ea;
        else if (ea == 1) oshape[d] = eb;
        else if (eb == 1) oshape[d] = ea;
        else
            return fail(RMHIP_ERR_SHAPE, "size mismatch between inputs (dimension %zu has lengths %zu and %zu)", d + 1, ea, eb);
    }
    const size_t on = shape_numel(oshape.data(), rank);
    const bool fast = (ab.numel == on || ab.numel == 1) && (bb.numel == on || bb.numel == 1);
    BroadcastDesc d{};
    if (!fast && on) {
        std::vector<std::vector<uint64_t>> strides;
        std::vector<uint64_t> os;
        const rmhip_buf ids[2] = {a, b};
        std::vector<Buffer> in = {ab, bb};
        RMHIP_TRY(bcast_prepare(c, ids, &in, false, oshape.data(), rank, &os, &strides, "complex_binary"));
        collapse(&os, &strides);
        if (os.size() > 8) return fail(RMHIP_ERR_UNSUPPORTED, "complex_binary: broadcast rank %zu > 8 after collapsing", os.size());
        d.rank = (int)os.size();
        for (size_t i = 0; i < os.size(); ++i) {
            d.out_shape[i] = os[i];
            d.stride_a[i] = strides[0][i];
            d.stride_b[i] = strides[1][i];
        }
    }
    RMHIP_TRY(c->new_buffer_complex(oshape.data(), rank, out, &ob));
    if (on == 0) return RMHIP_OK;
    const int rc = fast ? launch_complex_binary_same(c, op, kind, ab.data(), ab.numel == on, bb.data(), bb.numel == on, 0.0, ob.data(), on)
                        : launch_complex_binary_bcast(c, op, kind, ab.data(), bb.data(), ob.data(), on, d);
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

int rmhip_reduce(rmhip_ctx* ctx, int op, rmhip_buf a, int dim, int nan_mode, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (op < 0 || op >= RMHIP_REDUCE_OP_COUNT) return fail(RMHIP_ERR_UNSUPPORTED, "reduce op %d not supported by provider", op);
    Buffer ab, ob;
    bool f32 = c->precision == 32;  // f32 storage is read in place; the (small) result is f64 and narrowed on return
    RMHIP_TRY(get_operand(c, a, &ab, &f32));
    if (dim < 0) {
        const size_t oshape[2] = {1, 1};  // simple_provider.rs:6743
        RMHIP_TRY(c->new_buffer(oshape, 2, out, &ob));
        int rc = f32 ? launch_reduce_mid_f32(c, op, nan_mode, ab.data_f32(), 1, ab.numel, 1, ob.data())
                     : launch_reduce_all(c, op, nan_mode, ab.data(), ab.numel, ob.data());
        if (rc) rmhip_free(ctx, *out);
        return rc;
    }
    std::vector<size_t> shape = normalize_matrix_shape(ab.shape);
    if ((size_t)dim >= shape.size()) return fail(RMHIP_ERR_UNSUPPORTED, "reduce: dim %d out of range for rank %zu", dim, shape.size());
    size_t pre = 1, post = 1;
    for (int d = 0; d < dim; ++d) pre *= shape[d];
    for (size_t d = dim + 1; d < shape.size(); ++d) post *= shape[d];
    const size_t red = shape[dim];
    std::vector<size_t> oshape = shape;
    oshape[dim] = 1;
    RMHIP_TRY(c->new_buffer(oshape.data(), oshape.size(), out, &ob));
    int rc = f32 ? launch_reduce_mid_f32(c, op, nan_mode, ab.data_f32(), pre, red, post, ob.data())
                 : launch_reduce_mid(c, op, nan_mode, ab.data(), pre, red, post, ob.data());
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

namespace {
// [pre, red, post] view of `shape` around `dim` (dim < 0: everything is reduced) and the output shape (extent 1 at `dim`; [1,1] for all)
struct DimView {
    size_t pre = 1, red = 1, post = 1;
    std::vector<size_t> oshape;
};
int dim_view(const Buffer& b, int dim, const char* what, DimView* v) {
    const std::vector<size_t> shape = normalize_matrix_shape(b.shape);
    if (dim < 0) {
        v->red = b.numel;
        v->oshape = {1, 1};
        return RMHIP_OK;
    }
    if ((size_t)dim >= shape.size()) return fail(RMHIP_ERR_UNSUPPORTED, "%s: dim %d out of range for rank %zu", what, dim, shape.size());
    for (int d = 0; d < dim; ++d) v->pre *= shape[d];
    for (size_t d = dim + 1; d < shape.size(); ++d) v->post *= shape[d];
    v->red = shape[dim];
    v->oshape = shape;
    v->oshape[dim] = 1;
    return RMHIP_OK;
}
}  // namespace

int rmhip_reduce_minmax_dim(rmhip_ctx* ctx, int op, rmhip_buf a, int dim, int nan_mode, rmhip_buf* values, rmhip_buf* indices) {
    CTX_OR_FAIL(ctx);
    if (!values || !indices) return fail(RMHIP_ERR_INVALID, "reduce_minmax_dim: null output");
    if (op != RMHIP_RMIN && op != RMHIP_RMAX) return fail(RMHIP_ERR_INVALID, "reduce_minmax_dim: op must be RMHIP_RMIN or RMHIP_RMAX");
    if (dim < 0) return fail(RMHIP_ERR_INVALID, "reduce_minmax_dim: dim must be >= 0");
    Buffer ab, vb, ib;
    bool f32 = c->precision == 32;  // f32 storage is read in place and widened in registers (exact, order preserving); outputs are narrowed on return
    RMHIP_TRY(get_operand(c, a, &ab, &f32));
    DimView v;
    RMHIP_TRY(dim_view(ab, dim, "reduce_minmax_dim", &v));
    if (ab.numel == 0) return fail(RMHIP_ERR_UNSUPPORTED, "reduce_minmax_dim: empty tensor");
    RMHIP_TRY(c->new_buffer(v.oshape.data(), v.oshape.size(), values, &vb));
    int rc = c->new_buffer(v.oshape.data(), v.oshape.size(), indices, &ib);
    if (!rc)
        rc = f32 ? launch_argreduce_f32(c, op, nan_mode, ab.data_f32(), v.pre, v.red, v.post, vb.data(), ib.data())
                 : launch_argreduce(c, op, nan_mode, ab.data(), v.pre, v.red, v.post, vb.data(), ib.data());
    if (rc) {
        rmhip_free(ctx, *values);
        if (*indices) rmhip_free(ctx, *indices);
        return rc;
    }
    c->record_launch(op == RMHIP_RMIN ? "reduce_min_dim" : "reduce_max_dim", {{"reduce_len", v.red}, {"slices", v.pre * v.post}}, {{"wg", 256}});
    return RMHIP_OK;
}

int rmhip_reduce_std(rmhip_ctx* ctx, rmhip_buf a, int dim, int normalization, int nan_mode, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (normalization != 0 && normalization != 1) return fail(RMHIP_ERR_INVALID, "reduce_std: normalization must be 0 (sample) or 1 (population)");
    Buffer ab, ob;
    bool f32 = c->precision == 32;
    RMHIP_TRY(get_operand(c, a, &ab, &f32));
    DimView v;
    RMHIP_TRY(dim_view(ab, dim, "reduce_std", &v));
    if (ab.numel == 0) return fail(RMHIP_ERR_UNSUPPORTED, "reduce_std: empty tensor");
    RMHIP_TRY(c->new_buffer(v.oshape.data(), v.oshape.size(), out, &ob));
    const int rc = f32 ? launch_reduce_std_f32(c, normalization, nan_mode, ab.data_f32(), v.pre, v.red, v.post, ob.data())
                       : launch_reduce_std(c, normalization, nan_mode, ab.data(), v.pre, v.red, v.post, ob.data());
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

int rmhip_reduce_truth(rmhip_ctx* ctx, int op, rmhip_buf a, int dim, int omit_nan, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (op < 0 || op >= RMHIP_TRUTH_OP_COUNT) return fail(RMHIP_ERR_INVALID, "reduce_truth: bad op %d", op);
    Buffer ab, ob;
    bool f32 = c->precision == 32;
    RMHIP_TRY(get_operand(c, a, &ab, &f32));
    DimView v;
    RMHIP_TRY(dim_view(ab, dim, "reduce_truth", &v));
    if (ab.numel == 0) return fail(RMHIP_ERR_UNSUPPORTED, "reduce_truth: empty tensor");
    RMHIP_TRY(c->new_buffer(v.oshape.data(), v.oshape.size(), out, &ob));
    const int rc = f32 ? launch_reduce_truth_f32(c, op, omit_nan, ab.data_f32(), v.pre, v.red, v.post, ob.data())
                       : launch_reduce_truth(c, op, omit_nan, ab.data(), v.pre, v.red, v.post, ob.data());
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

int rmhip_cumulative(rmhip_ctx* ctx, int op, rmhip_buf a, int dim, int reverse, int nan_mode, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (op != 0 && op != 1) return fail(RMHIP_ERR_INVALID, "cumulative: op must be 0 (sum) or 1 (prod)");
    if (dim < 0) return fail(RMHIP_ERR_INVALID, "cumulative: dim must be >= 0");
    Buffer ab, ob;
    RMHIP_TRY(c->get(a, &ab));
    const std::vector<size_t> shape = normalize_matrix_shape(ab.shape);
    DimView v;
    RMHIP_TRY(dim_view(ab, dim, "cumulative", &v));
    RMHIP_TRY(c->new_buffer(shape.data(), shape.size(), out, &ob));
    const int rc = launch_cumulative(c, op, reverse, nan_mode, ab.data(), v.pre, v.red, v.post, ob.data());
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

int rmhip_reduce_nd(rmhip_ctx* ctx, int op, rmhip_buf a, const size_t* dims_zero_based, size_t ndims, int nan_mode,
                    rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out || (!dims_zero_based && ndims)) return fail(RMHIP_ERR_INVALID, "reduce_nd: null argument");
    Buffer ab;
    RMHIP_TRY(c->get_raw(a, &ab));  // shape only
    const size_t rank = normalize_matrix_shape(ab.shape).size();
    // nd.rs:62-72: dims beyond the rank are ignored, duplicates dropped, ascending order
    std::vector<size_t> dims;
    for (size_t i = 0; i < ndims; ++i)
        if (dims_zero_based[i] < rank) dims.push_back(dims_zero_based[i]);
    std::sort(dims.begin(), dims.end());
    dims.erase(std::unique(dims.begin(), dims.end()), dims.end());
    if (dims.empty()) return fail(RMHIP_ERR_INVALID, "reduce_nd: no valid dims to reduce");
    // the CPU reduces one dimension after the other in ascending order (mean of means, mean.rs:1107-1116)
    rmhip_buf cur = a;
    for (size_t i = 0; i < dims.size(); ++i) {
        rmhip_buf next = 0;
        const int rc = rmhip_reduce(ctx, op, cur, (int)dims[i], nan_mode, &next);
        if (cur != a) rmhip_free(ctx, cur);
        if (rc) return rc;
        cur = next;
    }
    *out = cur;
    return RMHIP_OK;
}

int rmhip_reduce_moments_nd(rmhip_ctx* ctx, rmhip_buf a, const size_t* dims_zero_based, size_t ndims, rmhip_buf* mean_out,
                            rmhip_buf* ex2_out) {
    CTX_OR_FAIL(ctx);
    if (!mean_out || !ex2_out) return fail(RMHIP_ERR_INVALID, "reduce_moments_nd: null output");
    size_t numel = 0;
    RMHIP_TRY(rmhip_numel(ctx, a, &numel));
    if (numel == 0) return fail(RMHIP_ERR_UNSUPPORTED, "reduce_moments_nd: empty tensor");  // nd.rs:318
    // The CPU's mean(x, dims) and mean(x .^ 2, dims) are means of means, one dimension after the other in ascending order
    // (mean.rs:1107-1116).  The first step is the only one that reads the whole tensor: ONE pass gives both of its results (sum and
    // sum of squares side by side, reduce2.hip SqAcc - x .* x is never materialised); the later steps run on the small intermediates.
    Buffer ab;
    RMHIP_TRY(c->get(a, &ab));
    const std::vector<size_t> shape = normalize_matrix_shape(ab.shape);
    std::vector<size_t> dims;  // nd.rs:62-72: dims beyond the rank are ignored, duplicates dropped, ascending order
    for (size_t i = 0; i < ndims; ++i)
        if (dims_zero_based && dims_zero_based[i] < shape.size()) dims.push_back(dims_zero_based[i]);
    std::sort(dims.begin(), dims.end());
    dims.erase(std::unique(dims.begin(), dims.end()), dims.end());
    if (dims.empty()) return fail(RMHIP_ERR_INVALID, "reduce_nd: no valid dims to reduce");
    const size_t d0 = dims[0];
    size_t pre = 1, post = 1;
    for (size_t i = 0; i < d0; ++i) pre *= shape[i];
    for (size_t i = d0 + 1; i < shape.size(); ++i) post *= shape[i];
    std::vector<size_t> oshape = shape;
    oshape[d0] = 1;
    rmhip_buf mean = 0, ex2 = 0;
    Buffer mb, eb;
    RMHIP_TRY(c->new_buffer(oshape.data(), oshape.size(), &mean, &mb));
    int rc = c->new_buffer(oshape.data(), oshape.size(), &ex2, &eb);
    if (!rc) rc = launch_reduce_moments(c, ab.data(), pre, shape[d0], post, mb.data(), eb.data());
    if (!rc && dims.size() > 1) {
        rmhip_buf m2 = 0, e2 = 0;
        rc = rmhip_reduce_nd(ctx, RMHIP_RMEAN, mean, dims.data() + 1, dims.size() - 1, 0, &m2);
        if (!rc) rc = rmhip_reduce_nd(ctx, RMHIP_RMEAN, ex2, dims.data() + 1, dims.size() - 1, 0, &e2);
        if (rc && m2) rmhip_free(ctx, m2);
        if (!rc) {
            rmhip_free(ctx, mean);
            rmhip_free(ctx, ex2);
            mean = m2;
            ex2 = e2;
        }
    }
    if (rc) {
        if (mean) rmhip_free(ctx, mean);
        if (ex2) rmhip_free(ctx, ex2);
        return rc;
    }
    *mean_out = mean;
    *ex2_out = ex2;
    return RMHIP_OK;
}

int rmhip_dot(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf b, int dim, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer ab, bb, ob;
    bool f32 = c->precision == 32;
    RMHIP_TRY(get_operand(c, a, &ab, &f32));
    RMHIP_TRY(get_operand(c, b, &bb, &f32));
    if (!f32 && ab.dtype == DT_F32) RMHIP_TRY(c->get(a, &ab));
    const std::vector<size_t> sa = normalize_matrix_shape(ab.shape), sb = normalize_matrix_shape(bb.shape);
    if (sa != sb) return fail(RMHIP_ERR_SHAPE, "dot: A and B must be the same size");
    int d = dim;
    if (d < 0) {  // first non-singleton dimension
        d = 0;
        for (size_t i = 0; i < sa.size(); ++i)
            if (sa[i] != 1) {
                d = (int)i;
                break;
            }
    }
    if ((size_t)d >= sa.size()) return fail(RMHIP_ERR_UNSUPPORTED, "dot: dim %d out of range for rank %zu", d, sa.size());
    size_t pre = 1, post = 1;
    for (int i = 0; i < d; ++i) pre *= sa[i];
    for (size_t i = d + 1; i < sa.size(); ++i) post *= sa[i];
    std::vector<size_t> oshape = sa;
    oshape[d] = 1;
    RMHIP_TRY(c->new_buffer(oshape.data(), oshape.size(), out, &ob));
    int rc = f32 ? launch_reduce_dot_f32(c, ab.data_f32(), bb.data_f32(), pre, sa[d], post, ob.data())
                 : launch_reduce_dot(c, ab.data(), bb.data(), pre, sa[d], post, ob.data());
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

// `take_matmul_sources`: rmhip_matmul notes which operands a product came from; the take removes the note
static void note_matmul_sources(Context* c, rmhip_buf product, rmhip_buf a, rmhip_buf b) {
    std::lock_guard<std::mutex> lk(c->mu);
    c->matmul_sources[product] = {a, b};
}

int rmhip_take_matmul_sources(rmhip_ctx* ctx, rmhip_buf product, rmhip_buf* lhs, rmhip_buf* rhs, int* found) {
    CTX_OR_FAIL(ctx);
    if (!lhs || !rhs || !found) return fail(RMHIP_ERR_INVALID, "take_matmul_sources: null result");
    *lhs = *rhs = 0;
    *found = 0;
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->matmul_sources.find(product);
    if (it == c->matmul_sources.end()) return RMHIP_OK;
    const std::pair<uint64_t, uint64_t> src = it->second;
    c->matmul_sources.erase(it);
    if (c->table.count(product) && c->table.count(src.first) && c->table.count(src.second)) {
        *lhs = src.first;
        *rhs = src.second;
        *found = 1;
    }
    return RMHIP_OK;
}

int rmhip_matmul(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf b, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    ScopedTimer timer(&c->tel.matmul_count, &c->tel.matmul_ns);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer ab, bb, ob;
    // Precision 32: both operands in f32 storage run on the f32 matrix cores (sgemm.hip; f32 accumulation like the
    // reference's F32 backend), whatever m and n are: few-tile / long-k shapes included, which launch_sgemm_trans splits
    // along k itself (f32 partials, summed in f64 and rounded once).  RMHIP_F32_MATMUL=f64 keeps the widen -> dgemm ->
    // round-once path (the CPU's `single` result exactly); it is also what mixed operands and k == 0 use.
    if (c->precision == 32) {
        Buffer ra, rb;
        RMHIP_TRY(c->get_raw(a, &ra));
        RMHIP_TRY(c->get_raw(b, &rb));
        if (!ra.rep_base.empty()) {
            RMHIP_TRY(c->settle_view(a));
            RMHIP_TRY(c->get_raw(a, &ra));
        }
        if (!rb.rep_base.empty()) {
            RMHIP_TRY(c->settle_view(b));
            RMHIP_TRY(c->get_raw(b, &rb));
        }
        if (ra.dtype == DT_F32 && rb.dtype == DT_F32 && ra.shape.size() == 2 && rb.shape.size() == 2) {
            if (ra.tview && rb.tview) {
                RMHIP_TRY(c->settle_view(b));
                RMHIP_TRY(c->get_raw(b, &rb));
            }
            const size_t m = ra.shape[0], k = ra.shape[1], kb = rb.shape[0], n = rb.shape[1];
            if (k != kb) return fail(RMHIP_ERR_SHAPE, "matmul: inner dims must agree (%zux%zu * %zux%zu)", m, k, kb, n);
            if (f32_gemm_eligible(c, m, n, k)) {
                const size_t oshape[2] = {m, n};
                RMHIP_TRY(c->new_buffer_f32(oshape, 2, out, &ob));
                int rc = launch_sgemm_trans(c, ra.tview, rb.tview, m, n, k, ra.data_f32(), ra.tview ? k : m, rb.data_f32(),
                                            rb.tview ? n : k, ob.data_f32(), m);
                if (rc) rmhip_free(ctx, *out);
                else {
                    c->record_launch("matmul", {{"m", m}, {"n", n}, {"k", k}}, {{"mfma_f32", 1}, {"ta", (uint64_t)ra.tview}, {"tb", (uint64_t)rb.tview}});
                    note_matmul_sources(c, *out, a, b);
                }
                return rc;
            }
        }
    }
    // transpose views are consumed in place (A'*B, A*B'); with both operands transposed B is materialised
    RMHIP_TRY(c->get_view(a, &ab));
    RMHIP_TRY(c->get_view(b, &bb));
    if (ab.tview && bb.tview) RMHIP_TRY(c->get(b, &bb));
    if (ab.shape.size() != 2 || bb.shape.size() != 2) return fail(RMHIP_ERR_UNSUPPORTED, "matmul: only 2D supported");  // simple_provider.rs:7705
    const size_t m = ab.shape[0], k = ab.shape[1], kb = bb.shape[0], n = bb.shape[1];
    if (k != kb) return fail(RMHIP_ERR_SHAPE, "matmul: inner dims must agree (%zux%zu * %zux%zu)", m, k, kb, n);
    const size_t oshape[2] = {m, n};
    RMHIP_TRY(c->new_buffer(oshape, 2, out, &ob));
    int rc = RMHIP_OK;
    if (k == 0) rc = launch_fill(c, ob.data(), ob.numel, 0.0);
    else if (ab.tview || bb.tview)  // storage: A' is k x m (ld k), B' is n x k (ld n)
        rc = launch_dgemm_trans(c, ab.tview, bb.tview, m, n, k, 1.0, ab.data(), ab.tview ? k : m, bb.data(), bb.tview ? n : k,
                                0.0, ob.data(), m);
    else rc = launch_dgemm(c, m, n, k, 1.0, ab.data(), m, bb.data(), k, 0.0, ob.data(), m);
    if (rc) rmhip_free(ctx, *out);
    else {
        c->record_launch("matmul", {{"m", m}, {"n", n}, {"k", k}}, {{"mfma_f64", 1}, {"ta", (uint64_t)ab.tview}, {"tb", (uint64_t)bb.tview}});
        note_matmul_sources(c, *out, a, b);
    }
    return rc;
}

int rmhip_matmul_power_step(rmhip_ctx* ctx, rmhip_buf lhs, rmhip_buf rhs, double epsilon, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    // simple_provider.rs:7859-7884 composed from the provider's own ops: P = lhs*rhs; acc_c = sum_r P(r,c)^2 (+ eps);
    // P(:,c) /= sqrt(acc_c).  The column sums run in the reduction kernels over the product functor (reduce_kernels.hip), the division in the broadcast kernel.
    rmhip_buf p = 0, sq = 0, sq_eps = 0, norms = 0;
    int rc = rmhip_matmul(ctx, lhs, rhs, &p);
    if (!rc) rc = rmhip_dot(ctx, p, p, 0, &sq);
    if (!rc) rc = rmhip_scalar(ctx, RMHIP_SADD, sq, epsilon, &sq_eps);
    if (!rc) rc = rmhip_unary(ctx, RMHIP_SQRT, sq_eps, &norms);
    if (!rc) rc = rmhip_binary(ctx, RMHIP_DIV, p, norms, out);
    for (rmhip_buf t : {p, sq, sq_eps, norms})
        if (t) rmhip_free(ctx, t);
    return rc;
}

int rmhip_image_normalize(rmhip_ctx* ctx, rmhip_buf input, const rmhip_image_normalize_t* d, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out || !d) return fail(RMHIP_ERR_INVALID, "image_normalize: null argument");
    if (!std::isfinite(d->epsilon)) return fail(RMHIP_ERR_INVALID, "image_normalize: epsilon must be finite");
    if (d->epsilon < 0.0) return fail(RMHIP_ERR_INVALID, "image_normalize: epsilon must be non-negative");
    Buffer ib, ob;
    bool f32 = c->precision == 32 && d->batch <= 256;  // more planes than that: the f64 kernels on a widened copy (special.hip IN_MAX_BATCH)
    RMHIP_TRY(get_operand(c, input, &ib, &f32));
    if (ib.shape.size() != 3) return fail(RMHIP_ERR_SHAPE, "image_normalize: expected 3-D tensor, got rank %zu", ib.shape.size());
    if (ib.shape[0] != d->batch || ib.shape[1] != d->height || ib.shape[2] != d->width)
        return fail(RMHIP_ERR_SHAPE, "image_normalize: descriptor dims (%zu, %zu, %zu) do not match tensor shape (%zu, %zu, %zu)",
                    d->batch, d->height, d->width, ib.shape[0], ib.shape[1], ib.shape[2]);
    int rc;
    if (f32) {
        RMHIP_TRY(c->new_buffer_f32(ib.shape.data(), 3, out, &ob));
        rc = image_normalize_device_f32(c, ib.data_f32(), ob.data_f32(), d->batch, d->height, d->width, d->epsilon, d->has_gain,
                                        d->gain, d->has_bias, d->bias, d->clamp_zero, d->has_gamma, d->gamma);
    } else {
        RMHIP_TRY(c->new_buffer(ib.shape.data(), 3, out, &ob));
        rc = image_normalize_device(c, ib.data(), ob.data(), d->batch, d->height, d->width, d->epsilon, d->has_gain, d->gain,
                                    d->has_bias, d->bias, d->clamp_zero, d->has_gamma, d->gamma);
    }
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

// rank / cond / pinv: the CPU decomposes with nalgebra's SVD (rank.rs:280-295, cond.rs:326-330, 448-467, pinv.rs:276-285); here the one-sided
// Jacobi decomposition of svdsolve.hip supplies the singular values (relative accuracy) and the pseudo-inverse.
static int matrix_dims_2d(const char* who, const Buffer& b, size_t* rows, size_t* cols) {
    for (size_t d = 2; d < b.shape.size(); ++d)
        if (b.shape[d] != 1) return fail(RMHIP_ERR_INVALID, "%s: inputs must be 2-D matrices or vectors", who);
    *rows = b.shape.empty() ? 1 : b.shape[0];
    *cols = b.shape.size() < 2 ? 1 : b.shape[1];
    return RMHIP_OK;
}

static int scalar_result(Context* c, double v, rmhip_buf* out) {
    const size_t one[2] = {1, 1};
    Buffer ob;
    RMHIP_TRY(c->new_buffer(one, 2, out, &ob));
    return launch_fill(c, ob.data(), 1, v);
}

int rmhip_rank(rmhip_ctx* ctx, rmhip_buf matrix, int has_tolerance, double tolerance, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer mb;
    RMHIP_TRY(c->get(matrix, &mb));
    size_t rows, cols;
    RMHIP_TRY(matrix_dims_2d("rank", mb, &rows, &cols));
    if (rows == 0 || cols == 0) return scalar_result(c, 0.0, out);  // rank.rs:283-285
    std::vector<double> sv;
    RMHIP_TRY(svd_values_host(c, "rank", mb.data(), rows, cols, &sv));
    const double cutoff = has_tolerance ? tolerance : svd_default_tolerance(sv, rows, cols);
    size_t r = 0;
    for (double v : sv) r += (std::isinf(v) || v > cutoff) ? 1 : 0;
    return scalar_result(c, (double)r, out);
}

int rmhip_cond(rmhip_ctx* ctx, rmhip_buf matrix, int norm, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (norm != 0) return fail(RMHIP_ERR_UNSUPPORTED, "cond: only the 2-norm is served (the 1 / inf / fro forms invert on the CPU path)");
    Buffer mb;
    RMHIP_TRY(c->get(matrix, &mb));
    size_t rows, cols;
    RMHIP_TRY(matrix_dims_2d("cond", mb, &rows, &cols));
    if (rows == 0 || cols == 0) return scalar_result(c, 0.0, out);  // cond.rs:278-280
    std::vector<double> sv;
    RMHIP_TRY(svd_values_host(c, "cond", mb.data(), rows, cols, &sv));
    double mn = INFINITY, mx = 0.0;  // singular_value_cond, cond.rs:448-467
    for (double v : sv) {
        const double a = std::fabs(v);
        if (!std::isfinite(a)) return scalar_result(c, INFINITY, out);
        mn = a < mn ? a : mn, mx = a > mx ? a : mx;
    }
    return scalar_result(c, mn == 0.0 ? INFINITY : mx / mn, out);
}

int rmhip_rcond(rmhip_ctx* ctx, rmhip_buf matrix, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer mb;
    RMHIP_TRY(c->get(matrix, &mb));
    size_t rows, cols;
    RMHIP_TRY(matrix_dims_2d("rcond", mb, &rows, &cols));
    if (rows != cols) return fail(RMHIP_ERR_INVALID, "rcond: input must be a square matrix.");
    if (rows == 0) return scalar_result(c, INFINITY, out);  // rcond.rs:311-313
    std::vector<double> sv;
    RMHIP_TRY(svd_values_host(c, "rcond", mb.data(), rows, cols, &sv));
    return scalar_result(c, svd_rcond(sv), out);  // singular_value_rcond, common/linalg.rs:241-259
}

int rmhip_pinv(rmhip_ctx* ctx, rmhip_buf matrix, int has_tolerance, double tolerance, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (has_tolerance && !(tolerance >= 0.0)) return fail(RMHIP_ERR_INVALID, "pinv: tolerance must be >= 0");
    Buffer mb, ob;
    RMHIP_TRY(c->get(matrix, &mb));
    size_t rows, cols;
    RMHIP_TRY(matrix_dims_2d("pinv", mb, &rows, &cols));
    const size_t oshape[2] = {cols, rows};
    RMHIP_TRY(c->new_buffer(oshape, 2, out, &ob));
    if (ob.numel == 0) return RMHIP_OK;  // pinv.rs:245-248
    const int rc = svd_pinv_device(c, mb.data(), rows, cols, has_tolerance ? tolerance : -1.0, ob.data());
    if (rc != RMHIP_OK) {
        rmhip_free(ctx, *out);
        *out = 0;
    }
    return rc;
}

int rmhip_covariance(rmhip_ctx* ctx, rmhip_buf matrix, int biased, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer mb;
    RMHIP_TRY(c->get_raw(matrix, &mb));  // shape only: the steps below fetch the data themselves
    if (mb.shape.size() > 2) return fail(RMHIP_ERR_UNSUPPORTED, "covariance: only 2D supported");
    const std::vector<size_t> ms = normalize_matrix_shape(mb.shape);
    const size_t rows = ms[0], cols = ms[1];
    const size_t oshape[2] = {cols, cols};
    const double denom = biased ? (double)rows : (double)rows - 1.0;
    if (cols == 0 || denom <= 0.0) {  // cov.rs:920-934: empty, or the all-NaN matrix
        Buffer ob;
        RMHIP_TRY(c->new_buffer(oshape, 2, out, &ob));
        int rc0 = launch_fill(c, ob.data(), ob.numel, std::numeric_limits<double>::quiet_NaN());
        if (rc0) rmhip_free(ctx, *out);
        return rc0;
    }
    rmhip_buf means = 0, centred = 0, gram = 0;
    int rc = rmhip_reduce(ctx, RMHIP_RMEAN, matrix, 0, 0, &means);       // [1, cols]
    if (!rc && gram_skinny_applies(rows, cols) && solve_knobs().gram_skinny) {
        // many samples of a few variables: centred on the way, no centred copy, no 256-wide MFMA tiles of 8-32 columns (special.hip)
        // (the division by the denominator and the diagonal rule ride on its second kernel).  f32 storage is read in place; the
        // products and sums are f64 either way and the result rounds once on the way out.
        Buffer xb, mub, ob;
        bool f32 = c->precision == 32;
        rc = get_operand(c, matrix, &xb, &f32);
        if (!rc) rc = c->get(means, &mub);
        if (!rc) rc = c->new_buffer(oshape, 2, out, &ob);
        if (!rc) {
            rc = f32 ? gram_skinny_device_f32(c, xb.data_f32(), rows, cols, mub.data(), denom, true, ob.data())
                     : gram_skinny_device(c, xb.data(), rows, cols, mub.data(), denom, true, ob.data());
            if (rc) rmhip_free(ctx, *out);
        }
        rmhip_free(ctx, means);
        return rc;
    } else {
        if (!rc) rc = rmhip_binary(ctx, RMHIP_SUB, matrix, means, &centred);  // broadcast over rows
        if (!rc) rc = rmhip_syrk(ctx, centred, &gram);                        // Xc' * Xc
    }
    if (!rc) {
        // gram / denom and the CPU's diagonal rules on an f64 result; at precision 32 `gb` is a widened copy and the result
        // is rounded to f32 storage on return (writing through Context::get of an f32 buffer would only touch a temporary)
        Buffer gb, ob;
        rc = c->get(gram, &gb);
        if (!rc) rc = c->new_buffer(oshape, 2, out, &ob);
        if (!rc) {
            rc = launch_scalar(c, RMHIP_SDIV, gb.data(), denom, ob.data(), ob.numel);
            if (!rc) rc = cov_sanitize_diag_device(c, ob.data(), cols);
            if (rc) rmhip_free(ctx, *out);
        }
    }
    for (rmhip_buf t : {means, centred, gram})
        if (t) rmhip_free(ctx, t);
    return rc;
}

int rmhip_covariance_general(rmhip_ctx* ctx, rmhip_buf matrix, rmhip_buf second_or_0, rmhip_buf weights_or_0, int biased, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    if (!second_or_0 && !weights_or_0) return rmhip_covariance(ctx, matrix, biased, out);
    *out = 0;
    Buffer mb, sb, wb;
    RMHIP_TRY(c->lookup(matrix, &mb));  // every id is known before any operand is judged
    if (second_or_0) RMHIP_TRY(c->lookup(second_or_0, &sb));
    if (weights_or_0) RMHIP_TRY(c->lookup(weights_or_0, &wb));
    RMHIP_TRY(c->get_raw(matrix, &mb));  // shape only; refuses complex-interleaved storage
    if (second_or_0) RMHIP_TRY(c->get_raw(second_or_0, &sb));
    if (weights_or_0) RMHIP_TRY(c->get_raw(weights_or_0, &wb));
    if (mb.shape.size() > 2 || sb.shape.size() > 2) return fail(RMHIP_ERR_UNSUPPORTED, "covariance: only 2D supported");
    const std::vector<size_t> ms = normalize_matrix_shape(mb.shape);
    const size_t rows = ms[0], cols1 = ms[1];
    size_t cols2 = 0;
    if (second_or_0) {  // combine_tensors, cov.rs:901-914
        const std::vector<size_t> ss = normalize_matrix_shape(sb.shape);
        if (ss[0] != rows) return fail(RMHIP_ERR_SHAPE, "covariance: inputs must have the same number of rows (got %zu and %zu)", rows, ss[0]);
        cols2 = ss[1];
    }
    const size_t cols = cols1 + cols2;
    if (weights_or_0) {
        const std::vector<size_t> ws = normalize_matrix_shape(wb.shape);
        if (wb.shape.size() > 2 || (ws[0] != 1 && ws[1] != 1)) return fail(RMHIP_ERR_SHAPE, "covariance: weight vector must be 1-D");
        if (wb.numel != rows) return fail(RMHIP_ERR_SHAPE, "covariance: weight vector length mismatch (expected %zu elements)", rows);
        if (rows == 0) return fail(RMHIP_ERR_INVALID, "covariance: weight vector cannot be empty");
    }
    const size_t oshape[2] = {cols, cols};
    auto all_nan = [&]() {  // cov.rs:920-934, 966-972: empty, or the all-NaN matrix
        Buffer ob;
        RMHIP_TRY(c->new_buffer(oshape, 2, out, &ob));
        const int rc0 = launch_fill(c, ob.data(), ob.numel, std::numeric_limits<double>::quiet_NaN());
        if (rc0) {
            rmhip_free(ctx, *out);
            *out = 0;
        }
        return rc0;
    };
    if (cols == 0) return all_nan();
    double denom = biased ? (double)rows : (double)rows - 1.0;
    if (!weights_or_0 && denom <= 0.0) return all_nan();
    // f32 storage is read in place when every operand holds it; otherwise all of them are read as f64 (widened / materialised copies)
    bool native = c->precision == 32;
    Buffer xb, x2b, wgt;
    for (int pass = 0; pass < 2; ++pass) {
        bool n1 = native, n2 = native, n3 = native;
        RMHIP_TRY(get_operand(c, matrix, &xb, &n1));
        if (second_or_0) RMHIP_TRY(get_operand(c, second_or_0, &x2b, &n2));
        if (weights_or_0) RMHIP_TRY(get_operand(c, weights_or_0, &wgt, &n3));
        if (n1 == native && (!second_or_0 || n2 == native) && (!weights_or_0 || n3 == native)) break;
        native = false;
    }
    const bool f32 = native;
    std::shared_ptr<Allocation> stat;  // means, sum_w, bad-weight count
    RMHIP_TRY(c->alloc_device(cols + 2, &stat));
    const void *xp = xb.data(), *x2p = second_or_0 ? x2b.data() : nullptr, *wp = weights_or_0 ? wgt.data() : nullptr;
    RMHIP_TRY(f32 ? cov_wsums_device_f32(c, (const float*)xp, (const float*)x2p, cols1, rows, cols, (const float*)wp, stat->ptr)
                  : cov_wsums_device(c, (const double*)xp, (const double*)x2p, cols1, rows, cols, (const double*)wp, stat->ptr));
    if (weights_or_0) {  // the call's only synchronisation: (sum_w, bad count)
        double host[2] = {0.0, 0.0};
        RMHIP_HIP_CHECK(hipMemcpyAsync(host, stat->ptr + cols, sizeof host, hipMemcpyDeviceToHost, c->stream));
        RMHIP_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (host[1] != 0.0) return fail(RMHIP_ERR_INVALID, "covariance: weights must be non-negative finite values");
        denom = host[0] - 1.0;  // `biased` is ignored, cov.rs:958-972
        if (host[0] <= 0.0 || denom <= 0.0) return all_nan();
    }
    Buffer ob;
    int rc = RMHIP_OK;
    if (gram_skinny_applies(rows, cols) && solve_knobs().gram_skinny) {
        RMHIP_TRY(c->new_buffer(oshape, 2, out, &ob));
        if (weights_or_0)
            rc = f32 ? gram_skinny_w_device_f32(c, (const float*)xp, (const float*)x2p, cols1, rows, cols, (const float*)wp, stat->ptr, denom, ob.data())
                     : gram_skinny_w_device(c, (const double*)xp, (const double*)x2p, cols1, rows, cols, (const double*)wp, stat->ptr, denom, ob.data());
        else
            rc = f32 ? gram_skinny_device_f32(c, (const float*)xp, rows, cols1, stat->ptr, denom, true, ob.data(), (const float*)x2p, cols2)
                     : gram_skinny_device(c, (const double*)xp, rows, cols1, stat->ptr, denom, true, ob.data(), (const double*)x2p, cols2);
    } else {
        // every other shape: one centring pass writes sqrt(w) (M - 1 mu) for both operands, the MFMA path multiplies Y' Y
        std::shared_ptr<Allocation> centred, gram;
        RMHIP_TRY(c->alloc_device(rows * cols, &centred));
        RMHIP_TRY(c->alloc_device(cols * cols, &gram));
        RMHIP_TRY(f32 ? cov_centre_device_f32(c, (const float*)xp, (const float*)x2p, cols1, rows, cols, (const float*)wp, stat->ptr, centred->ptr)
                      : cov_centre_device(c, (const double*)xp, (const double*)x2p, cols1, rows, cols, (const double*)wp, stat->ptr, centred->ptr));
        RMHIP_TRY(launch_dgemm_trans(c, true, false, cols, cols, rows, 1.0, centred->ptr, rows, centred->ptr, rows, 0.0, gram->ptr, cols));
        RMHIP_TRY(c->new_buffer(oshape, 2, out, &ob));
        rc = cov_finish_device(c, gram->ptr, cols, denom, ob.data());
    }
    if (rc) {
        rmhip_free(ctx, *out);
        *out = 0;
    }
    return rc;
}

int rmhip_diag_extract(rmhip_ctx* ctx, rmhip_buf matrix, long long offset, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer mb;
    RMHIP_TRY(c->get(matrix, &mb));
    for (size_t d = 2; d < mb.shape.size(); ++d)
        if (mb.shape[d] != 1) return fail(RMHIP_ERR_SHAPE, "diag: input must be 2-D");
    const size_t rows = mb.shape.empty() ? 1 : mb.shape[0], cols = mb.shape.size() < 2 ? 1 : mb.shape[1];
    if (rows == 1 || cols == 1 || mb.shape.size() <= 1) return fail(RMHIP_ERR_SHAPE, "diag: matrix input required");
    size_t len = 0;  // simple_provider.rs:2357-2376
    if (offset >= 0) {
        const size_t shift = (size_t)offset;
        len = shift >= cols ? 0 : std::min(rows, cols - shift);
    } else {
        const size_t shift = (size_t)(-offset);
        len = shift >= rows ? 0 : std::min(rows - shift, cols);
    }
    const size_t oshape[2] = {len, 1};
    Buffer ob;
    RMHIP_TRY(c->new_buffer(oshape, 2, out, &ob));
    int rc = diag_extract_device(c, mb.data(), rows, offset, len, ob.data());
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

int rmhip_syrk(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    ScopedTimer timer(&c->tel.matmul_count, &c->tel.matmul_ns);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer ab, ob;
    bool f32 = c->precision == 32;
    RMHIP_TRY(get_operand(c, a, &ab, &f32));
    if (ab.shape.size() > 2) return fail(RMHIP_ERR_UNSUPPORTED, "syrk: only 2D supported");
    const std::vector<size_t> as = normalize_matrix_shape(ab.shape);
    const size_t rows = as[0], cols = as[1];
    const size_t oshape[2] = {cols, cols};
    if (f32 && f32_gemm_eligible(c, cols, cols, rows)) {  // A' * A on the f32 matrix cores
        RMHIP_TRY(c->new_buffer_f32(oshape, 2, out, &ob));
        int rc = launch_sgemm_trans(c, true, false, cols, cols, rows, ab.data_f32(), rows, ab.data_f32(), rows, ob.data_f32(), cols);
        if (rc) rmhip_free(ctx, *out);
        return rc;
    }
    if (f32) RMHIP_TRY(c->get(a, &ab));  // f64 kernel on a widened copy
    RMHIP_TRY(c->new_buffer(oshape, 2, out, &ob));
    int rc = RMHIP_OK;
    if (rows == 0) rc = launch_fill(c, ob.data(), ob.numel, 0.0);
    else if (!f32 && c->precision == 64 && gram_skinny_applies(rows, cols) && solve_knobs().gram_skinny)
        rc = gram_skinny_device(c, ab.data(), rows, cols, nullptr, 1.0, false, ob.data());
    else rc = launch_dgemm_trans(c, true, false, cols, cols, rows, 1.0, ab.data(), rows, ab.data(), rows, 0.0, ob.data(), cols);
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

int rmhip_matmul_epilogue(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf b, const rmhip_matmul_epilogue_t* ep, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    ScopedTimer timer(&c->tel.matmul_count, &c->tel.matmul_ns);
    if (!out || !ep) return fail(RMHIP_ERR_INVALID, "matmul_epilogue: null argument");
    Buffer ab, bb, ob, rs, cs, dg;
    RMHIP_TRY(c->get(a, &ab));
    RMHIP_TRY(c->get(b, &bb));
    if (ab.shape.size() != 2 || bb.shape.size() != 2) return fail(RMHIP_ERR_UNSUPPORTED, "matmul: only 2D supported");
    const size_t m = ab.shape[0], k = ab.shape[1], kb = bb.shape[0], n = bb.shape[1];
    if (k != kb) return fail(RMHIP_ERR_SHAPE, "matmul: inner dims must agree (%zux%zu * %zux%zu)", m, k, kb, n);
    GemmEpilogue e{EP_ACTIVE, ep->alpha, ep->beta, nullptr, nullptr, ep->clamp_min, ep->clamp_max, ep->pow_exponent, nullptr};
    if (ep->row_scale) {
        RMHIP_TRY(c->get(ep->row_scale, &rs));
        if (rs.numel < m) return fail(RMHIP_ERR_SHAPE, "matmul_epilogue: row scale length %zu < %zu rows", rs.numel, m);
        e.row_scale = rs.data();
        e.flags |= EP_ROW | (ep->row_op ? EP_ROW_DIV : 0);
    }
    if (ep->col_scale) {
        RMHIP_TRY(c->get(ep->col_scale, &cs));
        if (cs.numel < n) return fail(RMHIP_ERR_SHAPE, "matmul_epilogue: col scale length %zu < %zu cols", cs.numel, n);
        e.col_scale = cs.data();
        e.flags |= EP_COL | (ep->col_op ? EP_COL_DIV : 0);
    }
    Buffer dg_raw;  // diag_output is written IN PLACE: f32 storage gets the widened copy narrowed back after the launch
    if (ep->diag_output) {
        RMHIP_TRY(c->get_raw(ep->diag_output, &dg_raw));
        if (dg_raw.lazy()) return fail(RMHIP_ERR_UNSUPPORTED, "matmul_epilogue: diag_output must not be a transpose / repmat view");
        RMHIP_TRY(c->detach_views_of(ep->diag_output));  // written in place
        RMHIP_TRY(c->get(ep->diag_output, &dg));
        const size_t expected = m < n ? m : n;
        if (dg.numel < expected)  // simple_provider.rs:7790-7799
            return fail(RMHIP_ERR_SHAPE, "matmul_epilogue: diag_output length %zu insufficient for diag size %zu", dg.numel, expected);
        e.diag = dg.data();
        e.flags |= EP_DIAG;
    }
    if (ep->has_clamp_min) e.flags |= EP_CLAMP_MIN;
    if (ep->has_clamp_max) e.flags |= EP_CLAMP_MAX;
    if (ep->has_pow) e.flags |= EP_POW;
    const size_t oshape[2] = {m, n};
    RMHIP_TRY(c->new_buffer(oshape, 2, out, &ob));
    int rc = launch_dgemm_epilogue(c, m, n, k, ab.data(), m, bb.data(), k ? k : 1, ob.data(), m, e);
    if (!rc && ep->diag_output && dg_raw.dtype == DT_F32) rc = launch_narrow(c, dg.data(), dg_raw.data_f32(), dg_raw.numel);
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

int rmhip_transpose(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer ab;
    RMHIP_TRY(c->get_raw(a, &ab));  // the alias keeps the operand's storage type
    if (ab.shape.size() > 2) return fail(RMHIP_ERR_UNSUPPORTED, "transpose: only 2D supported");
    if (!ab.rep_base.empty()) {  // a view of a repmat view: tile first
        RMHIP_TRY(c->settle_view(a));
        RMHIP_TRY(c->get_raw(a, &ab));
    }
    const std::vector<size_t> as = normalize_matrix_shape(ab.shape);
    // No data moves: the result aliases the operand's storage as a transpose view (a view of a view is the plain
    // base again; a vector's transpose has the same memory layout).  RMHIP_EAGER_TRANSPOSE=1 materialises at once.
    Buffer r;
    r.alloc = ab.alloc;
    r.shape = {as[1], as[0]};
    r.numel = ab.numel;
    r.tview = (as[0] == 1 || as[1] == 1) ? false : !ab.tview;
    r.dtype = ab.dtype;
    RMHIP_TRY(c->register_buffer(std::move(r), out));
    if (const char* e = std::getenv("RMHIP_EAGER_TRANSPOSE"))
        if (e[0] == '1') RMHIP_TRY(c->settle_view(*out));
    return RMHIP_OK;
}

int rmhip_set_rng_state(rmhip_ctx* ctx, uint64_t state) {
    CTX_OR_FAIL(ctx);
    c->rng_state = state;
    return RMHIP_OK;
}

int rmhip_set_lazy_random(rmhip_ctx* ctx, int enabled, size_t min_numel) {
    CTX_OR_FAIL(ctx);
    c->lazy_randn = enabled != 0;
    if (min_numel) c->lazy_randn_min = min_numel;
    return RMHIP_OK;
}

int rmhip_lazy_random_stats(rmhip_ctx* ctx, uint64_t* created, uint64_t* fused, uint64_t* materialised) {
    CTX_OR_FAIL(ctx);
    if (created) *created = c->lazy_randn_created;
    if (fused) *fused = c->lazy_randn_fused;
    if (materialised) *materialised = c->lazy_randn_materialised;
    return RMHIP_OK;
}

int rmhip_get_rng_state(rmhip_ctx* ctx, uint64_t* state) {
    CTX_OR_FAIL(ctx);
    if (!state) return fail(RMHIP_ERR_INVALID, "null state");
    *state = c->rng_state;
    return RMHIP_OK;
}

int rmhip_rng_seed(rmhip_ctx* ctx, uint64_t seed) {  // mix_seed, random.rs:128-141
    CTX_OR_FAIL(ctx);
    uint64_t s;
    if (seed == 0) s = 0x9e3779b97f4a7c15ULL;
    else {
        uint64_t z = seed + 0x9e3779b97f4a7c15ULL;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        s = z ^ (z >> 31);
        if (s == 0) s = 0x9e3779b97f4a7c15ULL;
    }
    c->rng_state = s;
    return RMHIP_OK;
}

int rmhip_random_uniform(rmhip_ctx* ctx, const size_t* shape, size_t rank, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    Buffer ob;
    int rc;
    if (c->precision == 32) {
        RMHIP_TRY(c->new_buffer_f32(shape, rank, out, &ob));
        rc = launch_rng_uniform_f32(c, c->rng_state, ob.data_f32(), ob.numel);
    } else {
        RMHIP_TRY(c->new_buffer(shape, rank, out, &ob));
        rc = launch_rng_uniform(c, c->rng_state, ob.data(), ob.numel);
    }
    if (rc) {
        rmhip_free(ctx, *out);
        return rc;
    }
    c->rng_state = lcg_advance(c->rng_state, ob.numel);
    return RMHIP_OK;
}

int rmhip_random_normal(rmhip_ctx* ctx, const size_t* shape, size_t rank, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    Buffer ob;
    int rc;
    if (c->precision != 32 && c->lazy_randn && out && (rank == 0 || shape) && shape_numel(shape, rank) >= c->lazy_randn_min &&
        shape_numel(shape, rank) >= 2) {
        // Lazy record: no storage, no launch.  A streaming fused elementwise kernel that reads it generates the normals in registers
        // (8 B per sample never written and never read back); anything else materialises it under this id with k_rng_normal on the
        // recorded state.  The stream advances now, exactly as for an eager call.
        Buffer b;
        b.shape.assign(shape, shape + rank);
        b.numel = shape_numel(shape, rank);
        b.rng_lazy = true;
        b.rng_state = c->rng_state;
        const size_t numel = b.numel;
        RMHIP_TRY(c->register_buffer(std::move(b), out));
        c->lazy_randn_created++;
        c->rng_state = lcg_advance(c->rng_state, 2 * ((numel + 1) / 2));
        return RMHIP_OK;
    }
    if (c->precision == 32) {
        RMHIP_TRY(c->new_buffer_f32(shape, rank, out, &ob));
        rc = launch_rng_normal_f32(c, c->rng_state, ob.data_f32(), ob.numel);
    } else {
        RMHIP_TRY(c->new_buffer(shape, rank, out, &ob));
        rc = launch_rng_normal(c, c->rng_state, ob.data(), ob.numel);
    }
    if (rc) {
        rmhip_free(ctx, *out);
        return rc;
    }
    c->rng_state = lcg_advance(c->rng_state, 2 * ((ob.numel + 1) / 2));  // whole pairs are consumed
    return RMHIP_OK;
}

namespace {
// one transformed draw per element (or whole Box-Muller pairs): allocate in the provider's storage type, launch, advance the stream
int random_dist(rmhip_ctx* ctx, Context* c, const size_t* shape, size_t rank, rmhip_buf* out, bool pairs, bool consumes,
                const std::function<int(double*, float*, size_t)>& launch) {
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer ob;
    int rc;
    if (c->precision == 32) {
        RMHIP_TRY(c->new_buffer_f32(shape, rank, out, &ob));
        rc = launch((double*)nullptr, ob.data_f32(), ob.numel);
    } else {
        RMHIP_TRY(c->new_buffer(shape, rank, out, &ob));
        rc = launch(ob.data(), (float*)nullptr, ob.numel);
    }
    if (rc) {
        rmhip_free(ctx, *out);
        return rc;
    }
    if (consumes) c->rng_state = lcg_advance(c->rng_state, pairs ? 2 * ((ob.numel + 1) / 2) : ob.numel);
    return RMHIP_OK;
}
}  // namespace

int rmhip_random_unifrnd(rmhip_ctx* ctx, double a, double b, const size_t* shape, size_t rank, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    return random_dist(ctx, c, shape, rank, out, false, true,
                       [&](double* o64, float* o32, size_t n) { return launch_rng_unifrnd(c, c->rng_state, a, b, o64, o32, n); });
}

int rmhip_random_exponential(rmhip_ctx* ctx, double mu, const size_t* shape, size_t rank, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    return random_dist(ctx, c, shape, rank, out, false, true,
                       [&](double* o64, float* o32, size_t n) { return launch_rng_exponential(c, c->rng_state, mu, o64, o32, n); });
}

int rmhip_random_normrnd(rmhip_ctx* ctx, double mu, double sigma, const size_t* shape, size_t rank, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    return random_dist(ctx, c, shape, rank, out, true, true,
                       [&](double* o64, float* o32, size_t n) { return launch_rng_normrnd(c, c->rng_state, mu, sigma, o64, o32, n); });
}

int rmhip_random_integer_range(rmhip_ctx* ctx, long long lower, long long upper, const size_t* shape, size_t rank, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    // simple_provider.rs:3689-3698: an empty range, or one of more than 2^53 values (not exactly representable), is an error
    if (lower > upper) return fail(RMHIP_ERR_INVALID, "random_integer_range: lower bound must be <= upper bound");
    const __int128 span128 = (__int128)upper - (__int128)lower + 1;
    if (span128 > ((__int128)1 << 53)) return fail(RMHIP_ERR_INVALID, "random_integer_range: integer range exceeds 2^53 and cannot be represented exactly");
    const unsigned long long span = (unsigned long long)span128;
    if (span == 1) {  // one value: no draws are consumed (simple_provider.rs:3703-3704)
        if (!out) return fail(RMHIP_ERR_INVALID, "null out");
        Buffer ob;
        RMHIP_TRY(c->new_buffer(shape, rank, out, &ob));  // (narrowed on return at precision 32, as rmhip_fill)
        const int rc = launch_fill(c, ob.data(), ob.numel, (double)lower);
        if (rc) rmhip_free(ctx, *out);
        return rc;
    }
    return random_dist(ctx, c, shape, rank, out, false, true,
                       [&](double* o64, float* o32, size_t n) { return launch_rng_integer_range(c, c->rng_state, lower, span, o64, o32, n); });
}

int rmhip_stochastic_evolution(rmhip_ctx* ctx, rmhip_buf state, double drift, double scale, uint32_t steps, rmhip_buf* out) {
    return rmhip_stochastic_evolution_sharded(ctx, state, drift, scale, steps, 0, out);
}

int rmhip_stochastic_evolution_sharded(rmhip_ctx* ctx, rmhip_buf state, double drift, double scale, uint32_t steps,
                                       uint64_t draws_per_step, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "null out");
    Buffer sb;
    bool f32 = c->precision == 32;
    RMHIP_TRY(get_operand(c, state, &sb, &f32));
    Buffer ob;
    if (f32) RMHIP_TRY(c->new_buffer_f32(sb.shape.data(), sb.shape.size(), out, &ob));
    else RMHIP_TRY(c->new_buffer(sb.shape.data(), sb.shape.size(), out, &ob));
    if (sb.numel == 0) return RMHIP_OK;
    int rc = RMHIP_OK;
    if (steps == 0) {  // stochastic_evolution.rs:16-18: nothing drawn, state unchanged
        hipError_t e = hipMemcpyAsync(ob.data(), sb.data(), (f32 ? sizeof(float) : sizeof(double)) * sb.numel, hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) rc = fail(RMHIP_ERR_HIP, "stochastic_evolution: %s", hipGetErrorString(e));
    } else {
        const uint64_t local = 2ULL * ((sb.numel + 1) / 2);
        if (draws_per_step && draws_per_step < local)
            rc = fail(RMHIP_ERR_INVALID, "stochastic_evolution: draws_per_step %llu < the shard's own %llu",
                      (unsigned long long)draws_per_step, (unsigned long long)local);
        if (!rc)
            rc = f32 ? launch_stochastic_evolution_f32(c, c->rng_state, sb.data_f32(), ob.data_f32(), sb.numel, drift, scale, steps, draws_per_step)
                     : launch_stochastic_evolution(c, c->rng_state, sb.data(), ob.data(), sb.numel, drift, scale, steps, draws_per_step);
        if (!rc) c->rng_state = lcg_advance(c->rng_state, (uint64_t)steps * (draws_per_step ? draws_per_step : local));
    }
    if (rc) rmhip_free(ctx, *out);
    return rc;
}

}  // extern "C"

// pagefun(@mtimes) (include/rmhip.h; kernels pagefun.hip, complex_pagefun.hip and dgemm.hip k_pgemm_w8).
namespace {

// What rmhip_pagefun and rmhip_complex_pagefun share: the request's validation, which restates build_pagefun_request
// (pagefun.rs:450-530) so that a malformed request never reaches a kernel, and the PageMap.  `who` heads the messages; `cplx_entry`:
// the call came through rmhip_complex_pagefun, which takes interleaved operands (extents count logical elements) and refuses a pair of
// real ones; the real entry point refuses an interleaved operand where it meets it.
struct PagefunPlan {
    Buffer raw[2];  // the table entries as they are (storage kind, shape): operands are settled by the caller
    size_t m = 0, n = 0, k = 0, pages = 1, vol[2] = {1, 1};
    PageMap pm{};
    bool dense[2] = {false, false};  // not broadcast: the operand's page of output page p is page p
};

int pagefun_plan(Context* c, const char* who, bool cplx_entry, int op, const rmhip_buf* inputs, size_t n_inputs, const size_t* page_dims,
                 size_t page_rank, const size_t* input_page_dims, const size_t* output_shape, size_t out_rank, PagefunPlan* plan) {
    if (op != RMHIP_PAGEFUN_MTIMES) return fail(RMHIP_ERR_UNSUPPORTED, "%s: unknown op %d", who, op);
    if (n_inputs != 2 || !inputs) return fail(RMHIP_ERR_INVALID, "%s: @mtimes takes exactly two inputs (got %zu)", who, n_inputs);
    if (page_rank && (!page_dims || !input_page_dims)) return fail(RMHIP_ERR_INVALID, "%s: page dimensions missing", who);
    if (!output_shape && out_rank) return fail(RMHIP_ERR_INVALID, "%s: null output shape", who);
    Buffer* const raw = plan->raw;
    size_t rows[2], cols[2];
    size_t* const vol = plan->vol;
    for (int i = 0; i < 2; ++i) {
        RMHIP_TRY(c->lookup(inputs[i], &raw[i]));
        if (raw[i].cplx && !cplx_entry) return fail(RMHIP_ERR_UNSUPPORTED, "%s: complex input; the host path answers", who);
        const std::vector<size_t>& s = raw[i].shape;  // canonical_matrix_shape (pagefun.rs:899-911)
        rows[i] = s.empty() ? 1 : (s.size() == 1 ? 1 : s[0]);
        cols[i] = s.empty() ? 1 : (s.size() == 1 ? s[0] : s[1]);
        for (size_t d = 0; d < page_rank; ++d) vol[i] *= input_page_dims[i * page_rank + d];
        if (raw[i].numel != rows[i] * cols[i] * vol[i])
            return fail(RMHIP_ERR_INVALID, "%s: input %d holds %zu elements, not %zu x %zu x %zu", who, i, raw[i].numel, rows[i], cols[i], vol[i]);
    }
    if (cplx_entry && !raw[0].cplx && !raw[1].cplx)
        return fail(RMHIP_ERR_UNSUPPORTED, "%s: both operands are real (rmhip_pagefun serves them)", who);
    const size_t m = rows[0], k = cols[0], n = cols[1];
    if (k != rows[1]) return fail(RMHIP_ERR_SHAPE, "%s: inner matrix dimensions must agree (%zux%zu * %zux%zu)", who, m, k, rows[1], n);
    size_t pages = 1;
    for (size_t d = 0; d < page_rank; ++d) {
        const size_t ea = input_page_dims[d], eb = input_page_dims[page_rank + d];
        size_t want;  // the builtin's rule: a zero extent wins, then equal extents or 1
        if (ea == 0 || eb == 0) want = 0;
        else if (ea == 1 || ea == eb) want = eb;
        else if (eb == 1) want = ea;
        else return fail(RMHIP_ERR_SHAPE, "%s: page dimension %zu mismatch (%zu vs %zu)", who, d + 3, ea, eb);
        if (page_dims[d] != want) return fail(RMHIP_ERR_INVALID, "%s: page_dims[%zu] = %zu, the inputs give %zu", who, d, page_dims[d], want);
        pages *= want;
    }
    if (out_rank != page_rank + 2 || output_shape[0] != m || output_shape[1] != n)
        return fail(RMHIP_ERR_INVALID, "%s: output shape must be [m, n, page_dims...]", who);
    for (size_t d = 0; d < page_rank; ++d)
        if (output_shape[2 + d] != page_dims[d]) return fail(RMHIP_ERR_INVALID, "%s: output shape must be [m, n, page_dims...]", who);
    if (m > 0xffffffffULL || n > 0xffffffffULL || k > 0xffffffffULL)
        return fail(RMHIP_ERR_UNSUPPORTED, "%s: a page side exceeds 2^32", who);
    // page strides in elements (0 along a broadcast dimension); dimensions of extent 1 dropped, neighbours whose strides continue each
    // other merged (a dense operand collapses to one dimension)
    std::vector<unsigned long long> dims, sa, sb;
    unsigned long long cur[2] = {(unsigned long long)m * k, (unsigned long long)k * n};
    for (size_t d = 0; d < page_rank; ++d) {
        const size_t e[2] = {input_page_dims[d], input_page_dims[page_rank + d]};
        const unsigned long long s0 = e[0] == 1 ? 0 : cur[0], s1 = e[1] == 1 ? 0 : cur[1];
        cur[0] *= e[0];
        cur[1] *= e[1];
        if (page_dims[d] == 1) continue;
        if (!dims.empty() && s0 == sa.back() * dims.back() && s1 == sb.back() * dims.back()) {
            dims.back() *= page_dims[d];
            continue;
        }
        dims.push_back(page_dims[d]);
        sa.push_back(s0);
        sb.push_back(s1);
    }
    if (m != 0 && n != 0 && pages != 0 && dims.size() > (size_t)kPageRankMax)
        return fail(RMHIP_ERR_UNSUPPORTED, "%s: %zu page dimensions after collapsing (at most %d)", who, dims.size(), kPageRankMax);
    PageMap& pm = plan->pm;
    pm.rank = (int)dims.size();
    for (size_t d = 0; d < dims.size() && d < (size_t)kPageRankMax; ++d) {
        pm.dims[d] = dims[d];
        pm.sa[d] = sa[d];
        pm.sb[d] = sb[d];
    }
    plan->m = m, plan->n = n, plan->k = k, plan->pages = pages;
    plan->dense[0] = vol[0] == pages, plan->dense[1] = vol[1] == pages;
    return RMHIP_OK;
}

}  // namespace

extern "C" {

// The tier is chosen here from (m, n, k, page count, broadcast pattern) and recorded as record_launch("pagefun", {m, n, k, pages},
// {tier, ...}).
int rmhip_pagefun(rmhip_ctx* ctx, int op, const rmhip_buf* inputs, size_t n_inputs, const size_t* page_dims, size_t page_rank,
                  const size_t* input_page_dims, const size_t* output_shape, size_t out_rank, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "pagefun: null out");
    *out = 0;
    PagefunPlan pl;
    RMHIP_TRY(pagefun_plan(c, "pagefun", false, op, inputs, n_inputs, page_dims, page_rank, input_page_dims, output_shape, out_rank, &pl));
    const size_t m = pl.m, n = pl.n, k = pl.k, pages = pl.pages;
    const size_t* const vol = pl.vol;
    const bool* const dense = pl.dense;
    const PageMap& pm = pl.pm;
    Buffer ob;
    RMHIP_TRY(c->new_buffer(output_shape, out_rank, out, &ob));
    if (ob.numel == 0) return RMHIP_OK;
    // settle lazy operands (transpose / repmat views, lazy random_normal) and widen f32 storage: f64 data in plain layout
    Buffer ab, bb;
    int rc = c->get(inputs[0], &ab);
    if (!rc) rc = c->get(inputs[1], &bb);
    int tier = 0;
    unsigned tuning = 0;
    if (rc) {
    } else if (k == 0) {
        rc = launch_fill(c, ob.data(), ob.numel, 0.0);  // matmul_real's empty sum
    } else if (vol[0] == 1 && dense[1] && n * pages <= 0xffffffffULL) {
        tier = 1;  // C(m, n P) = A(m, k) B(k, n P): bit for bit the 2-D matmul of the reshaped B
        rc = launch_dgemm(c, m, n * pages, k, 1.0, ab.data(), m, bb.data(), k, 0.0, ob.data(), m);
    } else if (m <= 32 && n <= 32 && k <= 32) {
        tier = 2;
        rc = launch_pagefun_tiny(c, ab.data(), bb.data(), ob.data(), (unsigned)m, (unsigned)n, (unsigned)k, pages, pm, dense[0], dense[1], &tuning);
    } else if (m >= 256 && n >= 256) {
        tier = 4;
        rc = launch_pgemm_w8(c, ab.data(), bb.data(), ob.data(), (unsigned)m, (unsigned)n, (unsigned)k, pages, pm);
    } else {
        tier = 3;
        rc = launch_pagefun_mfma(c, ab.data(), bb.data(), ob.data(), (unsigned)m, (unsigned)n, (unsigned)k, pages, pm);
    }
    if (rc) {
        rmhip_free(ctx, *out);
        *out = 0;
        return rc;
    }
    c->record_launch("pagefun", {{"m", m}, {"n", n}, {"k", k}, {"pages", pages}},
                     {{"tier", (uint64_t)tier}, {"page_rank", (uint64_t)pm.rank}, {"pages_per_block", tuning}});
    return RMHIP_OK;
}


// The complex sibling: at least one operand interleaved, the result interleaved.  A real operand is settled to plain f64 (views, lazy
// normals, f32 storage); record_launch("complex_pagefun", {m, n, k, pages}, {tier, kind, page_rank, pages_per_block}).
int rmhip_complex_pagefun(rmhip_ctx* ctx, int op, const rmhip_buf* inputs, size_t n_inputs, const size_t* page_dims, size_t page_rank,
                          const size_t* input_page_dims, const size_t* output_shape, size_t out_rank, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "complex_pagefun: null out");
    *out = 0;
    PagefunPlan pl;
    RMHIP_TRY(pagefun_plan(c, "complex_pagefun", true, op, inputs, n_inputs, page_dims, page_rank, input_page_dims, output_shape, out_rank, &pl));
    const size_t m = pl.m, n = pl.n, k = pl.k, pages = pl.pages;
    const int kind = pl.raw[0].cplx && pl.raw[1].cplx ? 0 : (pl.raw[0].cplx ? 1 : 2);
    Buffer ob;
    RMHIP_TRY(c->new_buffer_complex(output_shape, out_rank, out, &ob));
    if (ob.numel == 0) return RMHIP_OK;
    Buffer ab, bb;
    int rc = c->get_any(inputs[0], &ab);
    if (!rc) rc = c->get_any(inputs[1], &bb);
    int tier = 0;
    unsigned tuning = 0;
    if (rc) {
    } else if (k == 0) {
        rc = launch_fill(c, ob.data(), 2 * ob.numel, 0.0);  // the three loops' empty sums: (+0, +0)
    } else if (m <= 32 && n <= 32 && k <= 32) {
        tier = 2;
        rc = launch_cpage_small(c, kind, ab.data(), bb.data(), ob.data(), (unsigned)m, (unsigned)n, (unsigned)k, pages, pl.pm, pl.dense[0], pl.dense[1],
                                &tuning);
    } else {
        tier = 3;
        rc = launch_cpage_mfma(c, kind, ab.data(), bb.data(), ob.data(), (unsigned)m, (unsigned)n, (unsigned)k, pages, pl.pm);
    }
    if (rc) {
        rmhip_free(ctx, *out);
        *out = 0;
        return rc;
    }
    c->record_launch("complex_pagefun", {{"m", m}, {"n", n}, {"k", k}, {"pages", pages}},
                     {{"tier", (uint64_t)tier}, {"kind", (uint64_t)kind}, {"page_rank", (uint64_t)pl.pm.rank}, {"pages_per_block", tuning}});
    return RMHIP_OK;
}

// matmul's second entry point: a 2-D product with at least one complex-interleaved operand, the result interleaved (include/rmhip.h;
// kernels cgemm.hip).  plan_cgemm (gemm_plan.h) decides: a product of at most 32 on every side is one page of the complex
// pagefun's bit-exact small tier; anything larger is ONE real product through launch_dgemm over the interleaved rows, between a split
// of B into its planes and a join of the product's halves.  A real operand is settled to plain f64 as for complex pagefun.
// record_launch("complex_matmul", {m, n, k}, {kind, route}), route 2 small and 4 embed (numbered after the pagefun tiers).
int rmhip_complex_matmul(rmhip_ctx* ctx, rmhip_buf a, rmhip_buf b, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "complex_matmul: null out");
    *out = 0;
    Buffer ra, rb;
    RMHIP_TRY(c->lookup(a, &ra));
    RMHIP_TRY(c->lookup(b, &rb));
    if (!ra.cplx && !rb.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "complex_matmul: both operands are real (rmhip_matmul serves them)");
    if (ra.shape.size() != 2 || rb.shape.size() != 2) return fail(RMHIP_ERR_UNSUPPORTED, "matmul: only 2D supported");
    const size_t m = ra.shape[0], k = ra.shape[1], kb = rb.shape[0], n = rb.shape[1];
    if (k != kb) return fail(RMHIP_ERR_SHAPE, "matmul: inner dims must agree (%zux%zu * %zux%zu)", m, k, kb, n);
    const int kind = ra.cplx && rb.cplx ? 0 : (ra.cplx ? 1 : 2);
    const CgemmPlan pl = plan_cgemm(kind, m, n, k, c->precision == 32);
    if (pl.unsupported) return fail(RMHIP_ERR_UNSUPPORTED, "%s", pl.unsupported);
    const size_t oshape[2] = {m, n};
    Buffer ob;
    RMHIP_TRY(c->new_buffer_complex(oshape, 2, out, &ob));
    if (ob.numel == 0) return RMHIP_OK;
    Buffer ab, bb;
    int rc = c->get_any(a, &ab);
    if (!rc) rc = c->get_any(b, &bb);
    int route = 0;
    if (rc) {
    } else if (k == 0) {
        rc = launch_fill(c, ob.data(), 2 * ob.numel, 0.0);  // the three loops' empty sums: (+0, +0)
    } else if (!std::strcmp(pl.route, "small")) {
        route = 2;
        PageMap pm{};  // one page of each operand: rank 0, offsets 0
        rc = launch_cpage_small(c, kind, ab.data(), bb.data(), ob.data(), (unsigned)m, (unsigned)n, (unsigned)k, 1, pm, true, true, nullptr);
    } else {
        route = 4;
        std::shared_ptr<Allocation> ws;  // [planes: 2kn][T: MN]; back in the pool on return, stream order keeps it until the kernels are done
        if (pl.workspace) rc = c->alloc_device(pl.workspace, &ws);
        double* const planes = ws ? ws->ptr : nullptr;
        double* const T = ws ? ws->ptr + (pl.split_b ? 2 * k * n : 0) : nullptr;
        if (!rc && pl.split_b) rc = launch_cgemm_split_b(c, bb.data(), planes, k * n);
        if (!rc)
            rc = launch_dgemm(c, pl.M, pl.N, pl.K, 1.0, ab.data(), pl.lda, pl.split_b ? planes : bb.data(), pl.ldb, 0.0,
                              pl.join ? T : ob.data(), pl.M);
        if (!rc && pl.join) rc = launch_cgemm_join(c, kind, T, ob.data(), m * n);
    }
    if (rc) {
        rmhip_free(ctx, *out);
        *out = 0;
        return rc;
    }
    c->record_launch("complex_matmul", {{"m", m}, {"n", n}, {"k", k}}, {{"kind", (uint64_t)kind}, {"route", (uint64_t)route}});
    return RMHIP_OK;
}

}  // extern "C"

// ---- modulation (comms_ops.hip) ---------------------------------------------------------------------------------------------------------
namespace {

// What the two modulation hooks share once their arguments passed: the operand (f32 storage read in place by a precision-32 context, views
// and lazy normals materialised), the table on the device, the complex result, the launch and the one read of the verdict key.
// bps == 0: symbols.  `message`: the CPU's text for codes 1, 2, 3 (modulate_check.h).
int modulate_run(Context* c, rmhip_ctx* ctx, rmhip_buf input, const double* constellation, size_t n_values, unsigned bps, const std::vector<size_t>& out_shape,
                 const char* const message[3], rmhip_buf* out) {
    bool f32 = c->precision == 32;
    Buffer ib, ob;
    if (f32) RMHIP_TRY(get_operand(c, input, &ib, &f32));
    else RMHIP_TRY(c->get(input, &ib));
    const size_t order = n_values / 2, n = ib.numel;
    if (order > 0xffffffffull) return fail(RMHIP_ERR_UNSUPPORTED, "modulation: a constellation of %zu points (symbol numbers are 32-bit on the device)", order);
    RMHIP_TRY(c->new_buffer_complex(out_shape.data(), out_shape.size(), out, &ob));
    if (n == 0) return RMHIP_OK;
    // the host's table, as rmhip_spectral_estimate takes its window; a precision-32 context rounds a complex result's VALUES through f32
    std::vector<double> rounded;
    if (c->precision == 32) {
        rounded.assign(constellation, constellation + n_values);
        for (double& v : rounded) v = (double)(float)v;
        constellation = rounded.data();
    }
    std::shared_ptr<Allocation> table, key;
    int rc = c->alloc_device(n_values, &table);
    if (rc == RMHIP_OK) rc = c->alloc_device(1, &key);
    unsigned long long* const key_dev = rc == RMHIP_OK ? reinterpret_cast<unsigned long long*>(key->ptr) : nullptr;
    unsigned long long verdict = MOD_KEY_NONE;
    auto hip_ok = [&](hipError_t e, const char* what) {
        if (rc == RMHIP_OK && e != hipSuccess) rc = fail(RMHIP_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    };
    if (rc == RMHIP_OK) hip_ok(hipMemcpyAsync(table->ptr, constellation, n_values * sizeof(double), hipMemcpyHostToDevice, c->stream), "table upload");
    if (rc == RMHIP_OK) hip_ok(hipMemsetAsync(key_dev, 0xff, sizeof(unsigned long long), c->stream), "verdict reset");
    if (rc == RMHIP_OK)
        rc = bps ? launch_modulate_bits(c, ib.data(), f32, table->ptr, order, n, bps, ob.data(), key_dev)
                 : launch_modulate_symbols(c, ib.data(), f32, table->ptr, order, n, ob.data(), key_dev);
    // the call's only synchronisation (it also outlives `rounded`)
    if (rc == RMHIP_OK) hip_ok(hipMemcpyAsync(&verdict, key_dev, sizeof(verdict), hipMemcpyDeviceToHost, c->stream), "verdict read");
    if (rc == RMHIP_OK) hip_ok(hipStreamSynchronize(c->stream), "verdict read");
    else (void)hipStreamSynchronize(c->stream);
    if (rc == RMHIP_OK && verdict != MOD_KEY_NONE) {
        const unsigned code = mod_key_code(verdict);
        rc = fail(RMHIP_ERR_INVALID, "%s", message[code >= 1 && code <= 3 ? code - 1 : 2]);
    }
    if (rc != RMHIP_OK) {
        rmhip_free(ctx, *out);
        *out = 0;
    }
    return rc;
}

}  // namespace

extern "C" {

int rmhip_modulate_constellation(rmhip_ctx* ctx, rmhip_buf input, const double* constellation, size_t n_values, rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "modulate_constellation: null out");
    *out = 0;
    Buffer raw;
    RMHIP_TRY(c->lookup(input, &raw));
    // simple_provider.rs:4148-4156
    if (raw.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "modulate_constellation requires a real-valued symbol input");
    if (n_values == 0 || n_values % 2 != 0 || !constellation)
        return fail(RMHIP_ERR_INVALID, "modulate_constellation requires interleaved real/imag constellation pairs");
    static const char* const kMessage[3] = {"modulate_constellation: symbols must be finite integers",
                                            "modulate_constellation: symbols must be nonnegative integers",
                                            "modulate_constellation: symbols must be in range"};
    return modulate_run(c, ctx, input, constellation, n_values, 0, raw.shape, kMessage, out);
}

int rmhip_modulate_bits_constellation(rmhip_ctx* ctx, rmhip_buf input, size_t input_rows, size_t bits_per_symbol, const double* constellation, size_t n_values,
                                      rmhip_buf* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return fail(RMHIP_ERR_INVALID, "modulate_bits_constellation: null out");
    *out = 0;
    Buffer raw;
    RMHIP_TRY(c->lookup(input, &raw));
    // simple_provider.rs:4215-4259, in its order
    if (raw.cplx) return fail(RMHIP_ERR_UNSUPPORTED, "modulate_bits_constellation requires a real-valued bit input");
    if (n_values == 0 || n_values % 2 != 0 || !constellation)
        return fail(RMHIP_ERR_INVALID, "modulate_bits_constellation requires interleaved real/imag constellation pairs");
    if (input_rows == 0 || bits_per_symbol == 0) return fail(RMHIP_ERR_INVALID, "modulate_bits_constellation: invalid bit grouping");
    if (input_rows % bits_per_symbol != 0) return fail(RMHIP_ERR_INVALID, "modulate_bits_constellation: bit rows must be a multiple of bits_per_symbol");
    if (raw.shape.empty() || raw.shape[0] != input_rows)
        return fail(RMHIP_ERR_INVALID, "modulate_bits_constellation: input_rows must match the input leading dimension");
    // the CPU shifts a usize; symbols here are cut out of 32 bits (the wgpu provider caps the order at u32 as well)
    if (bits_per_symbol > (size_t)MOD_BPS_MAX)
        return fail(RMHIP_ERR_UNSUPPORTED, "modulate_bits_constellation: %zu bits per symbol (at most %d are served)", bits_per_symbol, MOD_BPS_MAX);
    std::vector<size_t> out_shape = raw.shape;
    out_shape[0] = input_rows / bits_per_symbol;
    static const char* const kMessage[3] = {"modulate_bits_constellation: bits must be finite", "modulate_bits_constellation: bits must be 0 or 1",
                                            "modulate_bits_constellation: symbols must be in range"};
    return modulate_run(c, ctx, input, constellation, n_values, (unsigned)bits_per_symbol, out_shape, kMessage, out);
}

}  // extern "C"
