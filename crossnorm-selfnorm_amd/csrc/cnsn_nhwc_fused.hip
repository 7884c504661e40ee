// Channels-last single-launch kernels (cnsn_nhwc_fused_kernels.h): host side.
#include "cnsn_nhwc.h"

#include "cnsn_nhwc_fused_host.h"

namespace cnsn {

using namespace nhwc_host;

namespace {
// part [S][2][P] | forward: kshift, gate (without `saved`) / backward: cX, c0 | barrier block
struct FusedWs { float *part, *side; void* bar; size_t bytes; };
FusedWs fused_layout(const NhwcGeom& g, void* workspace) {
    Carver c(workspace);  // (a braced list is evaluated left to right)
    return {c.take((size_t)g.S * 2 * g.P * 4), c.take(4 * g.P * 4), c.take<void>(kBarBlock), c.bytes()};
}
// part [S][kBnFwd][P] | kshift (conv), kshift (identity), gate / cX, c0 | e0, e1 (x 2 with a BatchNorm2d on the skip path) | barrier block
struct BnHeadWs { float *part, *side, *chan; void* bar; size_t bytes; };
BnHeadWs bnhead_layout(const NhwcGeom& g, void* workspace) {
    Carver c(workspace);
    return {c.take((size_t)g.S * kBnFwd * g.P * 4), c.take(4 * g.P * 4), c.take(4 * (size_t)g.C * 4), c.take<void>(kBarBlock), c.bytes()};
}
}  // namespace

NhwcGeom nhwc_fused_geom(const Plan& pl) {
    const cnsn_problem_t& p = pl.pr;
    NhwcGeom g;
    g.N = p.N;
    g.C = p.C;
    g.M = p.H * p.W;
    g.tc = p.C / vec_of(p.dtype);
    // tiles: two per workgroup of the persistent grid (CNSN_NHWC_WG_PER_CU x the compute units).  First narrower column blocks
    // — down to 64 vector columns: a wave still reads 1 KB of one pixel's row at a time, and nothing is paid for the split —
    // then pixel chunks, each of which costs a row of partial sums per plane (8 floats a chunk and plane against a 7x7 plane's
    // 49 elements): at least 8 pixels per thread and chunk where the plane allows it.
    const long target = 2l * CNSN_NHWC_WG_PER_CU * reshost::cu_count();
    g.tcb = g.tc < kBlock ? g.tc : kBlock;
    while (g.tcb > 64 && g.tcb % 2 == 0 && (long)g.N * ((g.tc + g.tcb - 1) / g.tcb) < target) g.tcb /= 2;
    g.rows = kBlock / g.tcb;
    g.ncb = (g.tc + g.tcb - 1) / g.tcb;
    const long per_chunk = (long)g.N * g.ncb;
    int S = (int)((target + per_chunk - 1) / per_chunk);
    const int s_max = g.M / (8 * g.rows) > 0 ? g.M / (8 * g.rows) : 1;
    if (S > s_max) S = s_max;
    if (S < 1) S = 1;
    g.mchunk = (g.M + S - 1) / S;
    g.S = (g.M + g.mchunk - 1) / g.mchunk;
    g.P = pl.P;
    nhwc_shift_samples(g, p.H, p.W);
    return g;
}

bool nhwc_slim_record(const Plan& pl) {
    const cnsn_problem_t& p = pl.pr;
    return p.layout == CNSN_LAYOUT_NHWC && !p.cn_active && p.sn_active && !p.sn_two;
}

bool nhwc_fused_ok(const Plan& pl, bool check_health) {
    const cnsn_problem_t& p = pl.pr;
    if (!nhwc_slim_record(pl) || !nhwc_supported(pl, false)) return false;
    if (p.strategy == CNSN_STRATEGY_TWO_PASS || p.strategy == CNSN_STRATEGY_LOCAL || p.strategy == CNSN_STRATEGY_MONO) return false;
    if (check_health && resident_degraded()) return false;  // a persistent launch gave up and nobody re-armed since: not even when forced
    const int mode = fused_mode();
    if (mode == 0) return false;
    if (p.N > kBlock || p.C % CNSN_NHWC_GC != 0 || p.H * p.W < 2) return false;  // (phase B: a thread per instance)
    if (check_health && p.strategy == CNSN_STRATEGY_AUTO && !resident_auto_enabled()) return false;
    if (mode > 2 && p.strategy == CNSN_STRATEGY_AUTO && tensor_bytes(pl) > ((size_t)mode << 20)) return false;
    const NhwcGeom g = nhwc_fused_geom(pl);
    return (long)g.N * g.S * g.ncb >= 8;  // (a grid of at least one workgroup per barrier group: launch_coresident declines fewer tiles)
}

size_t nhwc_fused_extra_bytes(const Plan& pl) { return fused_layout(nhwc_fused_geom(pl), nullptr).bytes; }

int nhwc_fused_forward(Plan& pl, int add, int relu, const void* x, const void* addend, GateDev gg, void* y, float* saved,
                       void* workspace, size_t workspace_bytes, hipStream_t stream, void* sum_out) {
    if (!nhwc_fused_ok(pl)) return CNSN_E_UNSUPPORTED;
    if (add != ADD_NONE && !addend) return CNSN_E_NULL;
    const NhwcGeom ng = nhwc_fused_geom(pl);
    const FusedWs w = fused_layout(ng, workspace);
    if (workspace_bytes < w.bytes) return CNSN_E_WORKSPACE;
    NhwcFusedArgs a = make_args(pl, ng, relu, CNSN_NHWC_GC);
    a.part = w.part;
    a.kshift = w.side;
    a.slim = saved;
    a.sum_out = add == ADD_PRE ? sum_out : nullptr;
    a.gout = saved ? saved + (size_t)SL_G * pl.P : a.kshift + pl.P;
    a.keep = keep_first_read(add == ADD_PRE ? 2 : 1, tensor_bytes(pl));
    int status = CNSN_E_UNSUPPORTED;
    dispatch_t(pl.pr.dtype, [&](auto tt, auto vt) {
        using T = typename decltype(tt)::type;
        constexpr int VEC = decltype(vt)::value;
        const size_t lds = (size_t)2 * ng.rows * ng.tcb * VEC * 4;
        auto go = [&](auto kern) {
            status = launch_fused(pl, kern, lds, a, a, w.bar, stream, (const T*)x, (const T*)addend, (T*)y, gg);
        };
        if (a.sum_out)  // (the second read is of what phase A wrote: the first one need not stay in the caches)
            return go(nhwc_fused_fwd_kernel<T, VEC, ADD_PRE, false, true>);
        with_add(add, [&](auto at) {
            constexpr int ADD = decltype(at)::value;
            a.keep ? go(nhwc_fused_fwd_kernel<T, VEC, ADD, true>) : go(nhwc_fused_fwd_kernel<T, VEC, ADD, false>);
        });
    });
    if (knob(K_DEBUG))
        fprintf(stderr, "[cnsn] nhwc single-launch fwd: tiles=%d (S=%d rows=%d tcb=%d) groups=%d keep=%d -> status %d\n", a.ntiles,
                ng.S, ng.rows, ng.tcb, a.ngroups, a.keep, status);
    return status;
}

int nhwc_fused_backward(Plan& pl, int add, int relu, const void* gy, const void* x, const void* addend, GateDev gg,
                        const float* saved, void* dx, void* d_addend, GateGradDev dg, void* workspace, size_t workspace_bytes,
                        hipStream_t stream) {
    if (!nhwc_fused_ok(pl)) return CNSN_E_UNSUPPORTED;
    if (!saved) return CNSN_E_NULL;
    if (add == ADD_POST && relu && !d_addend) return CNSN_E_NULL;
    const NhwcGeom ng = nhwc_fused_geom(pl);
    const FusedWs w = fused_layout(ng, workspace);
    if (workspace_bytes < w.bytes) return CNSN_E_WORKSPACE;
    // the backward of an epilogue without ReLU and without PRE add is the plain backward
    const int eff_add = (relu || add == ADD_PRE) ? add : ADD_NONE;
    if (eff_add != ADD_NONE && !addend) return CNSN_E_NULL;
    NhwcFusedArgs a = make_args(pl, ng, relu, CNSN_NHWC_GC_BWD);
    a.keep = keep_first_read(eff_add != ADD_NONE ? 3 : 2, tensor_bytes(pl));  // (G is one more tensor in flight than forward)
    a.part = w.part;
    a.coefb = w.side;
    a.slim = const_cast<float*>(saved);
    int status = CNSN_E_UNSUPPORTED;
    dispatch_t(pl.pr.dtype, [&](auto tt, auto vt) {
        using T = typename decltype(tt)::type;
        constexpr int VEC = decltype(vt)::value;
        const size_t lds = (size_t)2 * ng.rows * ng.tcb * VEC * 4;
        auto go = [&](auto kern) {
            status = launch_fused(pl, kern, lds, a, a, w.bar, stream, (const T*)gy, (const T*)x, (const T*)addend, (T*)dx, (T*)d_addend, gg,
                                  dg);
        };
        with_add(eff_add, [&](auto at) {
            constexpr int ADD = decltype(at)::value;
            a.keep ? go(nhwc_fused_bwd_kernel<T, VEC, ADD, true>) : go(nhwc_fused_bwd_kernel<T, VEC, ADD, false>);
        });
    });
    if (knob(K_DEBUG))
        fprintf(stderr, "[cnsn] nhwc single-launch bwd: tiles=%d (S=%d rows=%d tcb=%d) groups=%d keep=%d -> status %d\n", a.ntiles,
                ng.S, ng.rows, ng.tcb, a.ngroups, a.keep, status);
    return status;
}

void nhwc_slim_from_saved(const Plan& pl, const double* saved_d, float* slim, hipStream_t stream) {
    const int blocks = (int)((pl.P + kBlock - 1) / kBlock);
    nhwc_slim_from_saved_kernel<<<blocks, kBlock, 0, stream>>>(saved_d, pl.pr.N, pl.pr.C, slim);
}

void nhwc_saved_from_slim(const Plan& pl, const float* slim, int relu, double* saved_d, float* rows, hipStream_t stream) {
    const int blocks = (int)((pl.P + kBlock - 1) / kBlock);
    nhwc_saved_from_slim_kernel<<<blocks, kBlock, 0, stream>>>(slim, pl.pr.N, pl.pr.C, relu, saved_d, rows);
}

// ------------------------------------------------------------------------------------------------------------------------
// the block's last BatchNorm2d in front of the op (cnsn_nhwc_bnhead_kernels.h): y = act(SelfNorm(BatchNorm2d(conv_out) + identity))
// (ADD_PRE), y = act(SelfNorm(BatchNorm2d(conv_out)) + identity) (ADD_POST), y = SelfNorm(BatchNorm2d(conv_out)) (ADD_NONE)
// ------------------------------------------------------------------------------------------------------------------------
// check_health false: the BACKWARD of a forward that ran these kernels — there is no other kernel that reads its record, so it
// runs them whatever has happened to the cluster strategy in between (a bounded wait at worst: DESIGN.md section 6)
bool nhwc_bnhead_ok(const Plan& pl, bool check_health) {
    const cnsn_problem_t& p = pl.pr;
    if (!nhwc_fused_ok(pl, check_health) || !p.sn_training || p.N < 2 || p.C % kBnGc != 0) return false;
    const NhwcGeom g = nhwc_fused_geom(pl);
    if ((long)g.N * g.S * g.ncb < 8) return false;                // (a grid of at least one workgroup per barrier group)
    return (size_t)g.S * kBnFwd * g.P * 4 < ((size_t)1 << 31);  // (32-bit byte offsets into the partial sums: CohBuf)
}

namespace {
NhwcBnArgs make_bn_args(const Plan& pl, const NhwcGeom& ng, int relu, const cnsn_bn_tail_t& bn, const cnsn_bn_tail_t* bn2, float* bn_stats,
                        const BnHeadWs& w) {
    NhwcBnArgs a{};
    a.f = make_args(pl, ng, relu, kBnGc);
    a.bn = bn_head_dev(bn);
    if (bn2) a.bn2 = bn_head_dev(*bn2);
    set_bn_count(a, (double)ng.N * (double)ng.M);
    a.bn_stats = bn_stats;
    a.f.part = w.part;
    a.f.kshift = w.side;
    a.kshift_b = w.side + pl.P;
    a.f.gout = w.side + 2 * pl.P;   // forward without `saved`
    a.f.coefb = w.side + 2 * pl.P;  // backward: cX, c0
    a.chan = w.chan;
    return a;
}
const char* add_name(int add) { return add == ADD_PRE ? "pre" : (add == ADD_POST ? "post" : "none"); }
// the modes without a PRE add take no BatchNorm2d on the skip path, and ADD_NONE no ReLU (the IBN layer behind it has its own)
bool bnhead_mode_ok(int add, int relu, const cnsn_bn_tail_t* bn2) { return add == ADD_PRE || (!bn2 && !(add == ADD_NONE && relu)); }
}  // namespace

size_t nhwc_bnhead_extra_bytes(const Plan& pl) { return bnhead_layout(nhwc_fused_geom(pl), nullptr).bytes; }

int nhwc_bnhead_forward(Plan& pl, int add, int relu, const cnsn_bn_tail_t& bn, const cnsn_bn_tail_t* bn2, const void* conv_out,
                        const void* identity, GateDev gg, void* y, float* saved, float* bn_stats, void* workspace, size_t workspace_bytes,
                        hipStream_t stream) {
    if (!nhwc_bnhead_ok(pl) || !bn.training || (bn2 && !bn2->training) || !bnhead_mode_ok(add, relu, bn2)) return CNSN_E_UNSUPPORTED;
    if (add != ADD_NONE && !identity) return CNSN_E_NULL;
    const NhwcGeom ng = nhwc_fused_geom(pl);
    const BnHeadWs w = bnhead_layout(ng, workspace);
    if (workspace_bytes < w.bytes) return CNSN_E_WORKSPACE;
    NhwcBnArgs a = make_bn_args(pl, ng, relu, bn, bn2, bn_stats, w);
    a.f.slim = saved;
    if (saved) a.f.gout = saved + (size_t)SL_G * pl.P;
    a.f.keep = keep_first_read(add == ADD_PRE ? 2 : 1, tensor_bytes(pl));  // (without a PRE add phase A reads conv_out alone)
    int status = CNSN_E_UNSUPPORTED;
    dispatch_t(pl.pr.dtype, [&](auto tt, auto vt) {
        using T = typename decltype(tt)::type;
        constexpr int VEC = decltype(vt)::value;
        const size_t lds = (size_t)3 * ng.rows * ng.tcb * VEC * 4;
        auto go = [&](auto kern) {
            status = launch_fused(pl, kern, lds, a, a.f, w.bar, stream, (const T*)conv_out, (const T*)identity, (T*)y, gg);
        };
        if (bn2)
            return a.f.keep ? go(nhwc_bnhead_fwd_kernel<T, VEC, true, true>) : go(nhwc_bnhead_fwd_kernel<T, VEC, false, true>);
        with_add(add, [&](auto at) {
            constexpr int ADD = decltype(at)::value;
            a.f.keep ? go(nhwc_bnhead_fwd_kernel<T, VEC, true, false, ADD>) : go(nhwc_bnhead_fwd_kernel<T, VEC, false, false, ADD>);
        });
    });
    if (knob(K_DEBUG))
        fprintf(stderr, "[cnsn] nhwc bn-block fwd: tiles=%d (S=%d rows=%d tcb=%d) groups=%d keep=%d -> status %d mode=%s\n", a.f.ntiles,
                ng.S, ng.rows, ng.tcb, a.f.ngroups, a.f.keep, status, add_name(add));
    return status;
}

int nhwc_bnhead_backward(Plan& pl, int add, int relu, const cnsn_bn_tail_t& bn, const cnsn_bn_tail_t* bn2, const void* gy,
                         const void* conv_out, const void* identity, GateDev gg, const float* saved, const float* bn_stats, void* d_conv,
                         void* d_identity, GateGradDev dg, float* dbn_w, float* dbn_b, float* dbn2_w, float* dbn2_b, void* workspace,
                         size_t workspace_bytes, hipStream_t stream) {
    if (!nhwc_bnhead_ok(pl, false) || !bn.training || (bn2 && !bn2->training) || !bnhead_mode_ok(add, relu, bn2))
        return CNSN_E_UNSUPPORTED;
    // a POST add without a ReLU: the identity's gradient is grad_y itself, nothing of the identity is read or written
    const int eff_add = (add == ADD_POST && !relu) ? ADD_NONE : add;
    if (!saved || !bn_stats || !d_conv || !dbn_w || !dbn_b || (bn2 && (!dbn2_w || !dbn2_b))) return CNSN_E_NULL;
    if (eff_add != ADD_NONE && (!identity || !d_identity)) return CNSN_E_NULL;
    const NhwcGeom ng = nhwc_fused_geom(pl);
    const BnHeadWs w = bnhead_layout(ng, workspace);
    if (workspace_bytes < w.bytes) return CNSN_E_WORKSPACE;
    NhwcBnArgs a = make_bn_args(pl, ng, relu, bn, bn2, const_cast<float*>(bn_stats), w);
    a.f.slim = const_cast<float*>(saved);
    a.dbn_w = dbn_w;
    a.dbn_b = dbn_b;
    a.dbn2_w = dbn2_w;
    a.dbn2_b = dbn2_b;
    a.f.keep = keep_first_read(eff_add != ADD_NONE ? 3 : 2, tensor_bytes(pl));
    int status = CNSN_E_UNSUPPORTED;
    dispatch_t(pl.pr.dtype, [&](auto tt, auto vt) {
        using T = typename decltype(tt)::type;
        constexpr int VEC = decltype(vt)::value;
        const size_t lds = (size_t)3 * ng.rows * ng.tcb * VEC * 4;
        auto go = [&](auto kern) {
            status = launch_fused(pl, kern, lds, a, a.f, w.bar, stream, (const T*)gy, (const T*)conv_out, (const T*)identity,
                                  (T*)d_conv, (T*)d_identity, gg, dg);
        };
        if (bn2)
            return a.f.keep ? go(nhwc_bnhead_bwd_kernel<T, VEC, true, true>) : go(nhwc_bnhead_bwd_kernel<T, VEC, false, true>);
        with_add(eff_add, [&](auto at) {
            constexpr int ADD = decltype(at)::value;
            a.f.keep ? go(nhwc_bnhead_bwd_kernel<T, VEC, true, false, ADD>) : go(nhwc_bnhead_bwd_kernel<T, VEC, false, false, ADD>);
        });
    });
    if (knob(K_DEBUG))
        fprintf(stderr, "[cnsn] nhwc bn-block bwd: tiles=%d (S=%d rows=%d tcb=%d) groups=%d keep=%d -> status %d mode=%s\n", a.f.ntiles,
                ng.S, ng.rows, ng.tcb, a.f.ngroups, a.f.keep, status, add_name(add));
    return status;
}

}  // namespace cnsn
