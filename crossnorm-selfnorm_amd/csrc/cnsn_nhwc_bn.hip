// Channels-last single-launch BatchNorm2d (+ add) + ReLU (cnsn_nhwc_bn_kernels.h): host side and the C ABI entry points
// (include/cnsn_hip.h, ABI 9, added in round 8).  The geometry is this family's own (row chunks x column blocks of the R x C
// matrix); barrier booking and the co-resident launch are those of the other single launches (cnsn_nhwc_fused_host.h).
#include "../../include/cnsn_hip.h"
#include "cnsn_nhwc_bn_kernels.h"
#include "cnsn_nhwc_fused_host.h"

namespace cnsn {

using namespace nhwc_host;

namespace {

int bn_act_parse(const cnsn_bn_act_t* d) {
    const int st = parse_desc_head(d);
    return st ? st : parse_bn_tail(d->bn);
}

long long rows_of(const cnsn_bn_act_t& d) { return (long long)d.N * d.H * d.W; }
size_t tensor_bytes(const cnsn_bn_act_t& d) { return (size_t)rows_of(d) * d.C * elem_bytes(d.dtype); }

// the column blocks of the R x C matrix: the widest block (up to 256 vector columns) with which kBnActTiles tiles of at least
// kBnActMinRows rows exist, else the narrowest (8 vector columns = 128 contiguous bytes of a row); the row chunks: as many as
// the tile target asks for, none shorter than kBnActMinRows rows.  `eval`: the plain launch — a workgroup per tile of
// kBnActEvalIters rows per thread.  A pure function of the shape.
BnActGeom bn_act_geom(const cnsn_bn_act_t& d, bool eval = false) {
    BnActGeom g{};
    g.R = (int)rows_of(d);
    g.C = d.C;
    g.tc = d.C / vec_of(d.dtype);
    const long long slots = g.R / kBnActMinRows > 0 ? g.R / kBnActMinRows : 1;  // row chunks of full length the matrix has
    for (int t = 256; t >= 8; t >>= 1) {
        g.ncb = (g.tc + t - 1) / t;
        g.tcb = (g.tc + g.ncb - 1) / g.ncb;  // (balanced: the last block is not a sliver)
        if (eval || (long long)g.ncb * slots >= kBnActTiles) break;
    }
    g.ncb = (g.tc + g.tcb - 1) / g.tcb;
    g.rows = kBlock / g.tcb;
    if (eval) {
        g.chunk = g.rows * kBnActEvalIters;
    } else {
        long long want = (kBnActTiles + g.ncb - 1) / g.ncb;
        if (want > slots) want = slots;
        g.chunk = (int)((g.R + want - 1) / want);
    }
    g.wpc = (g.R + g.chunk - 1) / g.chunk;
    // the shift's samples: a pixel inside the plane of the images a quarter, a half and three quarters through the batch
    for (int i = 0; i < 3; ++i) {
        const int n = (i + 1) * d.N / 4 < d.N ? (i + 1) * d.N / 4 : d.N - 1;
        g.ks[i] = n * d.H * d.W + shift_sample_pixel(d.H, d.W, i);
    }
    return g;
}

// the shape conditions of either launch: whole 16-byte vectors, 32-bit row numbers and side-array offsets
bool bn_act_shape_ok(const cnsn_bn_act_t& d) {
    if ((d.C * elem_bytes(d.dtype)) % 16 != 0) return false;
    const long long R = rows_of(d);
    if (R < 2 || R >= ((long long)1 << 30) || d.C > (1 << 20)) return false;
    return true;
}

// the single launch takes the call (a pure function of it).  check_health: the forward — no unforgiven time-out, the co-resident
// kernels allowed (cnsn_resident_enable / CNSN_RESIDENT), CNSN_NHWC_FUSED not 0 and, above 2, the tensor within that many MiB.  AUTO
// (mode 1) has no size rule of its own: the launch measured faster than BatchNorm2d + ReLU at every site of a ResNet-50 down to
// the 13 MB of the 7x7 ones (profiles/r08_bn_act.md).  The backward of a forward that ran these kernels asks none of that
// again: what is left is a function of the shape alone, so the backward of an eligible forward is eligible.  Eval mode: the plain launch, forward only; it has no
// barrier, so neither health nor the resident switch bear on it — CNSN_NHWC_FUSED=0 still switches it off
bool bn_act_ok(const cnsn_bn_act_t& d, bool backward) {
    if (!bn_act_shape_ok(d)) return false;
    if (!d.bn.training) {
        if (backward || fused_mode() == 0) return false;
        const BnActGeom g = bn_act_geom(d, true);
        return (long long)g.ncb * g.wpc < ((long long)1 << 31);
    }
    if (!backward && !single_launch_allowed(tensor_bytes(d))) return false;
    const BnActGeom g = bn_act_geom(d);
    if ((long long)g.ncb * g.wpc < 8) return false;  // (a grid of at least one workgroup per barrier group)
    return (size_t)2 * g.wpc * g.C * 4 < ((size_t)1 << 31);
}

// part [2][wpc][C] | stat / coef [2][C] | barrier block
struct BnActWs { float *part, *coef; void* bar; size_t bytes; };
BnActWs bn_act_layout(const BnActGeom& g, void* workspace) {
    Carver c(workspace);
    return {c.take((size_t)2 * g.wpc * g.C * 4), c.take((size_t)2 * g.C * 4), c.take<void>(kBarBlock), c.bytes()};
}
size_t bn_act_extra_bytes(const cnsn_bn_act_t& d) {
    return d.bn.training ? bn_act_layout(bn_act_geom(d), nullptr).bytes : Carver(nullptr).bytes();  // (eval: no workspace)
}

cnsn_problem_t context_of(const cnsn_bn_act_t& d) {
    cnsn_problem_t p{};  // (resident_bar_area reads the context alone)
    p.context = d.context;
    p.context_bytes = d.context_bytes;
    return p;
}

BnActArgs make_bn_act_args(const cnsn_bn_act_t& d, const BnActGeom& g, const BnActWs& w) {
    BnActArgs a{};
    a.g = g;
    a.ntiles = g.ncb * g.wpc;
    a.relu = d.relu ? 1 : 0;
    a.bn = bn_head_dev(d.bn);
    set_bn_count(a, (double)g.R);
    a.part = w.part;
    a.stat = a.coef = w.coef;
    init_grid_bar(a.bar);
    return a;
}

int bn_act_forward(const cnsn_bn_act_t& d, const void* x, const void* addend, void* y, float* saved, void* workspace,
                   hipStream_t stream) {
    int status = CNSN_E_UNSUPPORTED;
    if (!d.bn.training) {  // the running statistics: one plain launch
        const BnActGeom g = bn_act_geom(d, true);
        const BnHeadDev bn = bn_head_dev(d.bn, false);
        dispatch_t(d.dtype, [&](auto tt, auto vt) {
            using T = typename decltype(tt)::type;
            constexpr int VEC = decltype(vt)::value;
            with_flag(addend != nullptr, [&](auto at) {
                constexpr bool ADD = decltype(at)::value;
                nhwc_bnact_eval_kernel<T, VEC, ADD><<<g.ncb * g.wpc, kBlock, 0, stream>>>(g, bn, d.relu ? 1 : 0, (const T*)x,
                                                                                          (const T*)addend, (T*)y);
                status = launch_status();
            });
        });
        return status;
    }
    const BnActGeom g = bn_act_geom(d);
    const BnActWs w = bn_act_layout(g, workspace);
    BnActArgs a = make_bn_act_args(d, g, w);
    if (saved) a.stat = saved;  // (written through: the backward's launch reads it like any other memory)
    a.keep = keep_first_read(1, tensor_bytes(d));  // (the addend is read once, in phase C)
    const cnsn_problem_t pr = context_of(d);
    int grid = 0;
    dispatch_t(d.dtype, [&](auto tt, auto vt) {
        using T = typename decltype(tt)::type;
        constexpr int VEC = decltype(vt)::value;
        const size_t lds = (size_t)2 * g.rows * g.tcb * VEC * 4;
        with_flag(addend != nullptr, [&](auto at) {
            constexpr bool ADD = decltype(at)::value;
            auto go = [&](auto kern) {
                status = launch_coresident(pr, kern, lds, a, a.bar, a.ntiles, w.bar, stream, &grid, (const T*)x,
                                           (const T*)addend, (T*)y);
            };
            a.keep ? go(nhwc_bnact_fwd_kernel<T, VEC, ADD, true>) : go(nhwc_bnact_fwd_kernel<T, VEC, ADD, false>);
        });
    });
    if (knob(K_DEBUG))
        fprintf(stderr, "[cnsn] nhwc bn_act fwd: R=%d C=%d tiles=%d (ncb=%d tcb=%d rows=%d chunk=%d) keep=%d -> status %d grid=%d\n", g.R,
                g.C, a.ntiles, g.ncb, g.tcb, g.rows, g.chunk, a.keep, status, grid);
    return status;
}

int bn_act_backward(const cnsn_bn_act_t& d, const void* gy, const void* x, const void* addend, const float* saved, void* dx,
                    void* d_addend, float* d_w, float* d_b, void* workspace, hipStream_t stream) {
    const BnActGeom g = bn_act_geom(d);
    const BnActWs w = bn_act_layout(g, workspace);
    BnActArgs a = make_bn_act_args(d, g, w);
    a.saved = saved;
    a.d_w = d_w;
    a.d_b = d_b;
    const bool add = d.relu && addend;  // (without the ReLU the addend's gradient is grad_y itself: nothing to read or write)
    a.keep = keep_first_read(add ? 3 : 2, tensor_bytes(d));
    const cnsn_problem_t pr = context_of(d);
    // launch_coresident cannot decline a call bn_act_ok accepts: the grid is occupancy (>= 1: no scratch, 128 VGPRs) x at least
    // 8 compute units, a multiple of 8 and at most the tiles, which are >= 8 here
    int status = CNSN_E_UNSUPPORTED, grid = 0;
    dispatch_t(d.dtype, [&](auto tt, auto vt) {
        using T = typename decltype(tt)::type;
        constexpr int VEC = decltype(vt)::value;
        const size_t lds = (size_t)2 * g.rows * g.tcb * VEC * 4;
        with_flag(add, [&](auto at) {
            constexpr bool ADD = decltype(at)::value;
            auto go = [&](auto kern) {
                status = launch_coresident(pr, kern, lds, a, a.bar, a.ntiles, w.bar, stream, &grid, (const T*)gy,
                                           (const T*)x, (const T*)addend, (T*)dx, (T*)d_addend);
            };
            a.keep ? go(nhwc_bnact_bwd_kernel<T, VEC, ADD, true>) : go(nhwc_bnact_bwd_kernel<T, VEC, ADD, false>);
        });
    });
    if (knob(K_DEBUG))
        fprintf(stderr, "[cnsn] nhwc bn_act bwd: R=%d C=%d tiles=%d (ncb=%d tcb=%d rows=%d chunk=%d) keep=%d -> status %d grid=%d\n", g.R,
                g.C, a.ntiles, g.ncb, g.tcb, g.rows, g.chunk, a.keep, status, grid);
    return status;
}

}  // namespace
}  // namespace cnsn

using namespace cnsn;

extern "C" {

int cnsn_bn_act_plan(const cnsn_bn_act_t* desc, int has_addend, int backward) {
    (void)has_addend;  // (the addend changes the tensor passes, not whether the launch applies)
    const int st = bn_act_parse(desc);
    if (st) return st;
    return bn_act_ok(*desc, backward != 0) ? 1 : 0;
}

size_t cnsn_bn_act_saved_floats(const cnsn_bn_act_t* desc) {
    if (bn_act_parse(desc) != CNSN_OK) return 0;
    return (size_t)2 * desc->C;
}

size_t cnsn_bn_act_workspace_bytes(const cnsn_bn_act_t* desc) {
    if (bn_act_parse(desc) != CNSN_OK || !bn_act_shape_ok(*desc)) return 0;
    return bn_act_extra_bytes(*desc);
}

int cnsn_forward_bn_act(const cnsn_bn_act_t* desc, const void* x, const void* addend, void* y, float* saved, void* workspace,
                        size_t workspace_bytes, void* stream) {
    const int st = bn_act_parse(desc);
    if (st) return st;
    const cnsn_bn_act_t& d = *desc;
    if (!bn_act_ok(d, false)) return CNSN_E_UNSUPPORTED;
    if (!x || !y || !workspace) return CNSN_E_NULL;
    if (!d.bn.weight || !d.bn.bias || !d.bn.running_mean || !d.bn.running_var) return CNSN_E_NULL;
    if (!aligned16(x) || !aligned16(y) || !aligned16(workspace) || (addend && !aligned16(addend)) || (saved && !aligned16(saved)))
        return CNSN_E_ALIGN;
    if (workspace_bytes < bn_act_extra_bytes(d)) return CNSN_E_WORKSPACE;
    return bn_act_forward(d, x, addend, y, saved, workspace, (hipStream_t)stream);
}

int cnsn_backward_bn_act(const cnsn_bn_act_t* desc, const void* grad_y, const void* x, const void* addend, const float* saved,
                         void* grad_x, void* grad_addend, float* d_weight, float* d_bias, void* workspace, size_t workspace_bytes,
                         void* stream) {
    const int st = bn_act_parse(desc);
    if (st) return st;
    const cnsn_bn_act_t& d = *desc;
    if (!bn_act_ok(d, true)) return CNSN_E_UNSUPPORTED;
    if (!grad_y || !x || !saved || !grad_x || !workspace || !d.bn.weight || !d.bn.bias) return CNSN_E_NULL;
    if (d.relu && addend && !grad_addend) return CNSN_E_NULL;
    if (!aligned16(grad_y) || !aligned16(x) || !aligned16(saved) || !aligned16(grad_x) || !aligned16(workspace) ||
        (addend && !aligned16(addend)) || (grad_addend && !aligned16(grad_addend)))
        return CNSN_E_ALIGN;
    if (workspace_bytes < bn_act_extra_bytes(d)) return CNSN_E_WORKSPACE;
    return bn_act_backward(d, grad_y, x, addend, saved, grad_x, grad_addend, d_weight, d_bias, workspace, (hipStream_t)stream);
}

}  // extern "C"
