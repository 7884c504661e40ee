// Channels-last single-launch Instance-Batch normalisation (cnsn_nhwc_ibn_kernels.h): host side and the C ABI entry points
// (include/cnsn_hip.h, ABI 9).  Geometry, barrier booking and the co-resident launch are the SelfNorm single-launch kernels'
// (cnsn_nhwc_fused_host.h); the descriptor is turned into the cnsn_problem_t they plan with.
#include "../../include/cnsn_hip.h"
#include "cnsn_nhwc_fused_host.h"
#include "cnsn_nhwc_ibn_kernels.h"

namespace cnsn {

using namespace nhwc_host;

namespace {

bool has_bn(const cnsn_ibn_t& d) { return d.half < d.C; }

// the descriptor's shape checks, then the problem the single-launch machinery plans with (SelfNorm's fields unused but for the
// layout and the context)
int ibn_parse(const cnsn_ibn_t* d, Plan& pl) {
    const int st = parse_desc_head(d);
    if (st) return st;
    if (d->half < 0 || d->half > d->C) return CNSN_E_SHAPE;
    if (has_bn(*d) && parse_bn_tail(d->bn)) return CNSN_E_STRUCT;
    cnsn_problem_t p{};
    p.struct_bytes = (int32_t)sizeof(cnsn_problem_t);
    p.dtype = d->dtype;
    p.N = d->N;
    p.C = d->C;
    p.H = d->H;
    p.W = d->W;
    for (int i = 0; i < 4; ++i) p.content_box[i] = p.style_box[i] = -1;
    p.layout = CNSN_LAYOUT_NHWC;
    p.strategy = CNSN_STRATEGY_AUTO;
    p.context = d->context;
    p.context_bytes = d->context_bytes;
    return make_plan(&p, pl);
}

// the single launch takes the call (a pure function of it).  The forward asks what nhwc_fused_ok asks of the SelfNorm single
// launches: no unforgiven time-out, the co-resident kernels allowed (cnsn_resident_enable / CNSN_RESIDENT), CNSN_NHWC_FUSED not 0 and,
// above 2, the tensor within that many MiB.  check_health false: the backward of a forward that ran these kernels — no other backward
// reads its record, so neither the health of the persistent launches nor the switches are asked again; what is left is a function
// of the shape alone, so the backward of an eligible forward is eligible
bool ibn_ok(const Plan& pl, const cnsn_ibn_t& d, bool check_health) {
    const cnsn_problem_t& p = pl.pr;
    if ((p.C * elem_bytes(p.dtype)) % 16 != 0 || p.C % CNSN_NHWC_GC != 0) return false;  // (16-byte vectors; whole phase-B groups)
    if (d.half <= 0 || d.half % CNSN_NHWC_GC != 0) return false;  // (a phase-B group is all InstanceNorm or all BatchNorm)
    if (p.N < 2 || p.N > kBlock || p.H * p.W < 2) return false;   // (phase B: a thread per instance)
    if (pl.P * IB_ROWS >= ((size_t)1 << 29)) return false;       // (CohBuf: 32-bit byte offsets)
    if (check_health && !single_launch_allowed(tensor_bytes(pl))) return false;
    const NhwcGeom g = nhwc_fused_geom(pl);
    if ((long)g.N * g.S * g.ncb < 8) return false;                // (a grid of at least one workgroup per barrier group)
    return (size_t)g.S * 2 * g.P * 4 < ((size_t)1 << 31);
}

// part [S][2][P] | kshift [P] | coef [3][P] (forward without `saved`) / cX, c0 (backward) | barrier block
struct IbnWs { float *part, *kshift, *coefb; void* bar; size_t bytes; };
IbnWs ibn_layout(const NhwcGeom& g, void* workspace) {
    Carver c(workspace);
    return {c.take((size_t)g.S * 2 * g.P * 4), c.take(g.P * 4), c.take(3 * g.P * 4), c.take<void>(kBarBlock), c.bytes()};
}
size_t ibn_extra_bytes(const Plan& pl) { return ibn_layout(nhwc_fused_geom(pl), nullptr).bytes; }

NhwcIbnArgs make_ibn_args(const Plan& pl, const NhwcGeom& ng, const cnsn_ibn_t& d, int gc, const IbnWs& w) {
    NhwcIbnArgs a{};
    a.f = make_args(pl, ng, d.relu ? 1 : 0, gc);
    a.f.training = has_bn(d) && d.bn.training ? 1 : 0;
    a.half = d.half;
    a.eps_in = d.eps_in;
    a.in_w = d.in_weight;
    a.in_b = d.in_bias;
    if (has_bn(d)) a.bn = bn_head_dev(d.bn);
    set_bn_count(a, (double)ng.N * (double)ng.M);
    a.f.part = w.part;
    a.f.kshift = w.kshift;
    a.f.coefb = w.coefb;
    return a;
}

}  // namespace

int nhwc_ibn_forward(Plan& pl, const cnsn_ibn_t& d, const void* x, const void* addend, void* y, float* saved, void* workspace,
                     hipStream_t stream) {
    const NhwcGeom ng = nhwc_fused_geom(pl);
    const IbnWs w = ibn_layout(ng, workspace);
    NhwcIbnArgs a = make_ibn_args(pl, ng, d, CNSN_NHWC_GC, w);
    a.saved = saved;
    a.coef = saved ? saved : a.f.coefb;
    a.f.keep = keep_first_read(addend ? 2 : 1, tensor_bytes(pl));
    int status = CNSN_E_UNSUPPORTED;
    dispatch_t(pl.pr.dtype, [&](auto tt, auto vt) {
        using T = typename decltype(tt)::type;
        constexpr int VEC = decltype(vt)::value;
        const size_t lds = (size_t)2 * ng.rows * ng.tcb * VEC * 4;
        with_add(addend ? ADD_PRE : ADD_NONE, [&](auto at) {
            constexpr int ADD = decltype(at)::value;
            if constexpr (ADD != ADD_POST) {
                auto go = [&](auto kern) {
                    status = launch_fused(pl, kern, lds, a, a.f, w.bar, stream, (const T*)x, (const T*)addend, (T*)y);
                };
                a.f.keep ? go(nhwc_ibn_fwd_kernel<T, VEC, ADD, true>) : go(nhwc_ibn_fwd_kernel<T, VEC, ADD, false>);
            }
        });
    });
    if (knob(K_DEBUG))
        fprintf(stderr, "[cnsn] nhwc ibn fwd: tiles=%d (S=%d rows=%d tcb=%d) groups=%d half=%d keep=%d -> status %d\n", a.f.ntiles,
                ng.S, ng.rows, ng.tcb, a.f.ngroups, d.half, a.f.keep, status);
    return status;
}

int nhwc_ibn_backward(Plan& pl, const cnsn_ibn_t& d, const void* gy, const void* x, const void* addend, const float* saved, void* dx,
                      float* d_in_w, float* d_in_b, float* d_bn_w, float* d_bn_b, void* workspace, hipStream_t stream) {
    const NhwcGeom ng = nhwc_fused_geom(pl);
    const IbnWs w = ibn_layout(ng, workspace);
    NhwcIbnArgs a = make_ibn_args(pl, ng, d, CNSN_NHWC_GC_BWD, w);
    a.saved = const_cast<float*>(saved);
    a.d_in_w = d_in_w;
    a.d_in_b = d_in_b;
    a.d_bn_w = d_bn_w;
    a.d_bn_b = d_bn_b;
    a.f.keep = keep_first_read(addend ? 3 : 2, tensor_bytes(pl));
    // launch_fused cannot decline a call ibn_ok(pl, d, false) accepts: the grid is occupancy (>= 1: no scratch, 128 VGPRs) x at
    // least 8 compute units (grid_for keeps 8 whatever the head-room), a multiple of 8 and at most the tiles, which are >= 8 here
    int status = CNSN_E_UNSUPPORTED;
    dispatch_t(pl.pr.dtype, [&](auto tt, auto vt) {
        using T = typename decltype(tt)::type;
        constexpr int VEC = decltype(vt)::value;
        const size_t lds = (size_t)2 * ng.rows * ng.tcb * VEC * 4;
        with_add(addend ? ADD_PRE : ADD_NONE, [&](auto at) {
            constexpr int ADD = decltype(at)::value;
            if constexpr (ADD != ADD_POST) {
                auto go = [&](auto kern) {
                    status = launch_fused(pl, kern, lds, a, a.f, w.bar, stream, (const T*)gy, (const T*)x, (const T*)addend,
                                          (T*)dx);
                };
                a.f.keep ? go(nhwc_ibn_bwd_kernel<T, VEC, ADD, true>) : go(nhwc_ibn_bwd_kernel<T, VEC, ADD, false>);
            }
        });
    });
    if (knob(K_DEBUG))
        fprintf(stderr, "[cnsn] nhwc ibn bwd: tiles=%d (S=%d rows=%d tcb=%d) groups=%d half=%d keep=%d -> status %d\n", a.f.ntiles,
                ng.S, ng.rows, ng.tcb, a.f.ngroups, d.half, a.f.keep, status);
    return status;
}

}  // namespace cnsn

using namespace cnsn;

extern "C" {

int cnsn_ibn_plan(const cnsn_ibn_t* desc, int has_addend, int backward) {
    (void)has_addend;  // (the addend changes the tensor passes, not whether the launch applies)
    Plan pl;
    const int st = ibn_parse(desc, pl);
    if (st) return st;
    return ibn_ok(pl, *desc, backward == 0) ? 1 : 0;
}

size_t cnsn_ibn_saved_floats(const cnsn_ibn_t* desc) {
    Plan pl;
    if (ibn_parse(desc, pl) != CNSN_OK) return 0;
    return (size_t)IB_ROWS * pl.P;
}

size_t cnsn_ibn_workspace_bytes(const cnsn_ibn_t* desc) {
    Plan pl;
    if (ibn_parse(desc, pl) != CNSN_OK) return 0;
    return ibn_extra_bytes(pl);
}

int cnsn_forward_ibn(const cnsn_ibn_t* desc, const void* x, const void* addend, void* y, float* saved, void* workspace,
                     size_t workspace_bytes, void* stream) {
    Plan pl;
    const int st = ibn_parse(desc, pl);
    if (st) return st;
    const cnsn_ibn_t& d = *desc;
    if (!ibn_ok(pl, d, true)) return CNSN_E_UNSUPPORTED;
    if (!x || !y || !workspace) return CNSN_E_NULL;
    if (has_bn(d) && (!d.bn.weight || !d.bn.bias || !d.bn.running_mean || !d.bn.running_var)) return CNSN_E_NULL;
    if (!aligned16(x) || !aligned16(y) || !aligned16(workspace) || (addend && !aligned16(addend)) || (saved && !aligned16(saved)))
        return CNSN_E_ALIGN;
    if (workspace_bytes < ibn_extra_bytes(pl)) return CNSN_E_WORKSPACE;
    return nhwc_ibn_forward(pl, d, x, addend, y, saved, workspace, (hipStream_t)stream);
}

int cnsn_backward_ibn(const cnsn_ibn_t* desc, const void* grad_y, const void* x, const void* addend, const float* saved, void* grad_x,
                      float* d_in_weight, float* d_in_bias, float* d_bn_weight, float* d_bn_bias, void* workspace,
                      size_t workspace_bytes, void* stream) {
    Plan pl;
    const int st = ibn_parse(desc, pl);
    if (st) return st;
    const cnsn_ibn_t& d = *desc;
    if (!ibn_ok(pl, d, false)) return CNSN_E_UNSUPPORTED;
    if (!grad_y || !x || !saved || !grad_x || !workspace) return CNSN_E_NULL;
    if (has_bn(d) && !d.bn.weight) return CNSN_E_NULL;
    if (!aligned16(grad_y) || !aligned16(x) || !aligned16(saved) || !aligned16(grad_x) || !aligned16(workspace) ||
        (addend && !aligned16(addend)))
        return CNSN_E_ALIGN;
    if (workspace_bytes < ibn_extra_bytes(pl)) return CNSN_E_WORKSPACE;
    return nhwc_ibn_backward(pl, d, grad_y, x, addend, saved, grad_x, d_in_weight, d_in_bias, d_bn_weight, d_bn_bias, workspace,
                             (hipStream_t)stream);
}

}  // extern "C"
